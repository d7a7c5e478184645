"""Element-wise checker of the training path's glue kernels: the entropy models' backward kernels, the rate term, the
elementwise / gather / reduction kernels of csrc/train.hip (tests/test_gpu_train_glue.py on the GPU,
tests/test_glue_checker.py for the checker itself on the CPU).  It does for them what gemm_check.py does for the GEMMs
and takes Guarded, ratio, check_out, gelu_grad64 and the constants from there.

Every kernel gets (ref, bound): ref in float64 from inputs already rounded to the dtype the kernel reads, bound a
PER-ELEMENT bound built from the kernel's own formula by a running error analysis.  The class E carries (value,
error bound) pairs in float64 through the formula, one rule per f32 operation.  u = 2^-23 is an ulp relative to the
lower end of the binade; IEEE add, mul and div are correctly rounded, off by r = u / 2 at the most, and a contracted
fma rounds once where mul + add round twice, so it stays inside the same bound:

    a + b, a - b      e = ea + eb + r |a +- b|       a difference such as pb - pa or su - sl is therefore bounded through
                                                      the errors of BOTH operands, i.e. through pa + pb, never through
                                                      the (possibly cancelled) result
    a * b             e = |a| eb + |b| ea + ea eb + r |a b|
    a / b             e = (ea + |a / b| eb) / (|b| - eb) + r |a / b|
    f(a), f monotone  e = max |f(a +- ea) - f(a)| + k u |f(a)|: the exact image of the input interval (monotone f attains
                      its extremes at the interval's ends) plus the library's own error.  k = 4 ulp for expf, log1pf,
                      tanhf, erfcf, logf, sqrtf: the HIP math API documentation tabulates a maximum ulp error per
                      single-precision function, and 4 covers every one used here.  This is where the conditioning terms
                      come from: exp(-a^2 / 2) moves by about a^2 2u relatively when a moves by 2u relatively, tanh' and
                      sigmoid' shrink the error of a saturated argument, erfc in the tail (lik near 1e-9) amplifies it
                      by about 2 x^2.
    every operation   e += 2^-126: a result below the smallest normal f32 may be flushed to zero (a likelihood
                      gradient of 1e-62 is a plain 0 in f32)
    f32 constant      e = u |c| (0.11f, 1 / sqrt(2 pi), -1 / sqrt 2, 1 / (-ln2 num_pixels) are not exactly the reals)
    sum of rows terms e = sum e_i + (rows + 2) u sum |t_i|    any order, any tree (gemm_check's argument)
    bf16 store        e += 2^-8 (|v| + e)
    acc0 + v          e += u (|acc0| + |v| + e)               accumulation into a non-zero f32 buffer
    gelu_grad(p)      d = ERF_F32_ERR / 2 + |GELU''(p)| u |p| + 4 2^-24 |g| (gemm_check.dgrad_reference's derivation)
                      + |p| phi(p) (2u p^2 + 4u): the exp(-p^2 / 2) of the p phi(p) term, argument rounded twice

No constant comes from running a kernel.  Branch decisions (LowerBound pass-through, signs, round) are taken from
the float64 reference; where an f32 evaluation may legitimately decide otherwise the element is in the SKIP MASK
(computed from the reference alone): unclamped likelihood in [1e-10, 1e-8], |sigma - 0.11| < 1e-3,
0 < |x~ - mu| < 1e-4, fractional part of v - m within 1e-3 of .5.  Skipped elements are excluded from the bound
check only (they must be finite), and a case may skip at most 2 % (SKIP_CAP; asserted by the tests).  A skipped element
that feeds a SUM (the EntropyBottleneck's parameter gradients) cannot be left out of it: its whole term is added to
the sum's bound instead.  A sign decision such as `ds < 0` on an element whose ds is within its own error of zero needs
no mask: either outcome is within the element's error of the other.

Gradient references of the two entropy models are float64 torch.autograd through oracle.train_oracle (gc_train,
eb_train's forms, aux_loss, lower_bound, quantize_ste); the eval forms x~ = round(v - m).detach() + m are written out
here.  The E evaluation of the kernel's formula must agree with autograd to float64 accuracy (test_glue_checker.py), so
the bound belongs to the same function the reference computes.

The any-order bound of a sum of rows terms exceeds the suite's older scalar bound 1e-5 max|ref| as soon as
rows + 2 > 83 (84 u > 1e-5); test_glue_checker.py's sanity limit therefore covers the elementwise outputs and the short
sums, and says so.
"""
import math
from types import SimpleNamespace as NS

import torch

import parity_log
from gemm_check import BF16_ROUND, ERF_F32_ERR, U, Guarded, check_out, gelu_grad64, ratio  # noqa: F401
from oracle import train_oracle as orc
from oracle.mcm_oracle import eb_logits

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LIBM_ULP = 4
R = U / 2  # add, mul, div are correctly rounded: half an ulp
TINY = 2.0 ** -126  # the smallest normal f32: a result below it may be flushed to zero
SKIP_CAP = 0.02
EB_PRE = "eb."


# ------------------------------------------------------------------------------------ running error analysis
def _t(x):
    return x.double() if isinstance(x, torch.Tensor) else torch.tensor(float(x), dtype=F64)


class E:
    """float64 value v and a bound e on |f32 evaluation - v| (module docstring)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = _t(v)
        self.e = torch.zeros_like(self.v) if e is None else _t(e)

    @staticmethod
    def lift(x):
        return x if isinstance(x, E) else E(x)

    @staticmethod
    def const(c):
        """a real constant the kernel holds in f32"""
        return E(c, U * abs(c))

    def __add__(self, o):
        o = E.lift(o)
        v = self.v + o.v
        return E(v, self.e + o.e + R * v.abs() + TINY)

    __radd__ = __add__

    def __neg__(self):
        return E(-self.v, self.e)

    def __sub__(self, o):
        return self + (-E.lift(o))

    def __rsub__(self, o):
        return E.lift(o) + (-self)

    def __mul__(self, o):
        o = E.lift(o)
        v = self.v * o.v
        return E(v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e + R * v.abs() + TINY)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.lift(o)
        v = self.v / o.v
        den = (o.v.abs() - o.e).clamp_min(1e-300)
        return E(v, (self.e + v.abs() * o.e) / den + R * v.abs() + TINY)

    def __rtruediv__(self, o):
        return E.lift(o) / self

    def exact(self, k):
        """times a power of two, or a 0 / 1 mask: no rounding"""
        k = _t(k)
        return E(self.v * k, self.e * k.abs())

    def abs(self):
        return E(self.v.abs(), self.e)

    def mono(self, f, ulps=LIBM_ULP):
        v = f(self.v)
        e = torch.maximum((f(self.v + self.e) - v).abs(), (f(self.v - self.e) - v).abs())
        return E(v, e + ulps * U * v.abs() + TINY)

    def sum(self, dim):
        rows = self.v.shape[dim]
        return E(self.v.sum(dim), self.e.sum(dim) + (rows + 2) * U * self.v.abs().sum(dim))

    def where(self, mask, other):
        other = E.lift(other)
        return E(torch.where(mask, self.v, other.v), torch.where(mask, self.e, other.e))

    def store(self, dtype):
        return E(self.v, self.e + BF16_ROUND * (self.v.abs() + self.e)) if dtype == BF16 else self

    def acc(self, acc0):
        """accumulation into a non-zero f32 buffer"""
        a = _t(acc0)
        return E(self.v + a, self.e + U * (a.abs() + self.v.abs() + self.e))

    def out(self):
        return self.v, self.e


def cat(es, dim):
    return E(torch.cat([x.v for x in es], dim), torch.cat([x.e for x in es], dim))


def exact_out(values, dtype=F32):
    """(ref, bound) of a kernel that moves values: bitwise, after the cast where asked"""
    ref = values.to(dtype).double()
    return ref, torch.zeros_like(ref)


def check(metric, g, ref, bound, skip=None, log=True):
    """gemm_check.check_out with a skip mask: skipped elements must be finite, and are bounded by nothing else"""
    if skip is not None and bool(skip.any()):
        out = g.result().reshape(ref.shape)
        assert bool(torch.isfinite(out[skip]).all()), f"{metric}: a skipped element is not finite"
        bound = torch.where(skip, torch.full_like(bound, float("inf")), bound)
    if log:
        metric = f"{metric}:{'bf16' if g.buf.dtype == BF16 else 'f32'}"  # the output's dtype
    if log and g.buf.dtype == F32:  # f32: a ratio above 0.5 is reported with its element
        out = g.result().reshape(ref.shape)
        err = (out - ref).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
        if r.numel() and float(torch.nan_to_num(r, nan=float("inf")).max()) > 0.5:
            i = int(torch.nan_to_num(r, nan=float("inf")).argmax())
            where = dict(index=i, out=float(out.flatten()[i]), ref=float(ref.flatten()[i]),
                         element_bound=float(bound.flatten()[i]))
            print(f"{metric}: error / bound = {float(r.flatten()[i]):.3g} at {where}")
            parity_log.record(metric + ":worst_element", float(r.flatten()[i]), 1.0, **where)
    return check_out(metric, g, ref.reshape(g.M, g.N), bound.reshape(g.M, g.N), log=log)


def written(values, dtype=F32, init=None):
    """a CPU Guarded buffer holding `values` (2-D, or 1-D as one row), as a correct kernel would leave it"""
    v = values.reshape(1, -1) if values.dim() != 2 else values
    g = Guarded(v.shape[0], v.shape[1], dtype, init=init)
    g.block()[...] = v.to(dtype)
    return g


def pad(t, ld, fill=float("nan")):
    """rows of t, ld elements apart; the padding is NaN, so a kernel that reads it shows"""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def remap_rows(rows, G, Gs, off):
    """source rows of the kernels' row-group map: sr = (r / G) * Gs + off + r % G"""
    r = torch.arange(rows)
    return (r // G) * Gs + off + r % G


# ------------------------------------------------------------------------------------ GaussianConditional backward
GC_SHAPES = {"small": dict(n=2, HW=9, sw=5, Mtot=16, yoff=7), "three_wg": dict(n=3, HW=16, sw=11, Mtot=40, yoff=24)}
# seeds fixed on the CPU; measured skipped elements (likelihood band / sigma band / near-zero / tie):
#   small    seed 3: train 0 / 0 / 0 / 0 of 90, eval 0 / 0 / 0 / 0 of 90
#   three_wg seed 7: train 9 / 0 / 0 / 0 of 528 (1.7 %), eval 2 / 0 / 0 / 2 of 528 (0.8 %)
# census of three_wg (train): likelihood clamped 94 blocked / 75 passing, sigma < 0.11 70 passing / 27 blocked, 6 exact
# zeros of x~ - mu (eval: 87 / 68, 70 / 29, 66); test_glue_checker.test_gc_census_and_skip asserts the classes and the cap
GC_SEEDS = {"small": 3, "three_wg": 7}


def gc_case(shape, seed=None):
    """the issue's probe recipe: y ~ 3 N(0,1), mu ~ N(0,1), sigma a third in [0.02, 0.09] and the rest in
    [0.13, 2.63], uniform noise; six exact x~ == mu elements (y 1.5, noise 0.25, mu 1.75: exactly representable)"""
    d = GC_SHAPES[shape]
    n, HW, sw, Mtot, yoff = d["n"], d["HW"], d["sw"], d["Mtot"], d["yoff"]
    g = _gen(GC_SEEDS[shape] if seed is None else seed)
    M = n * HW
    y = 3 * torch.randn(M, Mtot, generator=g)
    mu = torch.randn(M, sw, generator=g)
    small = torch.rand(M, sw, generator=g) < 1 / 3
    sigma = torch.where(small, 0.02 + 0.07 * torch.rand(M, sw, generator=g), 0.13 + 2.5 * torch.rand(M, sw, generator=g))
    noise = torch.rand(n, Mtot, HW, generator=g) - 0.5
    glik = torch.randn(n, Mtot, HW, generator=g)
    gyp = torch.randn(M, Mtot, generator=g)
    dy0 = torch.randn(M, Mtot, generator=g)
    for k in range(6):  # exact zeros of x~ - mu, in training (1.5 + 0.25 - 1.75) and in eval (round(-0.25) = 0)
        m, c = (5 * k + 1) % M, (2 * k) % sw
        y[m, yoff + c], mu[m, c] = 1.5, 1.75
        noise[m // HW, yoff + c, m % HW] = 0.25
    return NS(shape=shape, n=n, HW=HW, sw=sw, Mtot=Mtot, yoff=yoff, M=M, y=y, mu=mu, sigma=sigma, noise=noise, glik=glik,
              gyp=gyp, dy0=dy0, ldy=Mtot + 8, ld_ms=sw + 3, ldg=Mtot + 3)


def _mc(c, t):
    """slice of an NCHW [n][Mtot][HW] tensor as [pixel m][slice channel]"""
    return t[:, c.yoff:c.yoff + c.sw, :].permute(0, 2, 1).reshape(c.M, c.sw)


def gc_autograd(c, training, use_glik=True, use_gyp=True, dtype=F64):
    """(dy slice, dmu, dsigma) by torch.autograd through the oracle in `dtype`, and the unclamped likelihood"""
    sl = slice(c.yoff, c.yoff + c.sw)
    y = c.y[:, sl].to(dtype).requires_grad_(True)
    mu = c.mu.to(dtype).requires_grad_(True)
    sg = c.sigma.to(dtype).requires_grad_(True)
    glik = _mc(c, c.glik).to(dtype) if use_glik else torch.zeros(c.M, c.sw, dtype=dtype)
    gyp = c.gyp[:, sl].to(dtype) if use_gyp else torch.zeros(c.M, c.sw, dtype=dtype)
    if training:
        nz = _mc(c, c.noise).to(dtype)
        xt = y + nz
        lik = orc.gc_train(y, sg, mu, nz)
    else:  # x~ = round(y - mu) + mu: moves with mu, no gradient through round
        xt = torch.round(y - mu).detach() + mu
        lik = orc.gc_train(xt, sg, mu, torch.zeros_like(xt))
    yhp = orc.quantize_ste(y - mu) + mu
    ((glik * lik).sum() + (gyp * yhp).sum()).backward()
    with torch.no_grad():
        v = (xt - mu).abs()
        s = sg.clamp_min(0.11)
        k = -(2 ** -0.5)
        raw = 0.5 * torch.erfc(k * ((0.5 - v) / s)) - 0.5 * torch.erfc(k * ((-0.5 - v) / s))
    zero = torch.zeros_like(y)
    return NS(dy=y.grad if y.grad is not None else zero, dmu=mu.grad if mu.grad is not None else zero,
              dsigma=sg.grad if sg.grad is not None else zero, raw=raw.detach(), dd=(xt - mu).detach(), glik=glik)


def gc_skip(c, training, a):
    """the skip mask and its parts, from the float64 reference alone"""
    band = (a.raw >= 1e-10) & (a.raw <= 1e-8)
    sig = (c.sigma.double() - 0.11).abs() < 1e-3
    near0 = (a.dd.abs() > 0) & (a.dd.abs() < 1e-4)
    if training:
        tie = torch.zeros_like(band)
    else:
        d = c.y[:, c.yoff:c.yoff + c.sw].double() - c.mu.double()
        tie = ((d - torch.floor(d)) - 0.5).abs() < 1e-3
    return NS(band=band, sig=sig, near0=near0, tie=tie, any=band | sig | near0 | tie)


def gc_census(c, a):
    """branch classes of gc_bwd_kernel, counted on the reference"""
    clamped = a.raw < 1e-9
    small = c.sigma.double() < 0.11
    # ds before the sigma bound: dsigma of the reference where it passed, else its sign from the formula below
    ds = gc_formula(c, a, a.training, F32).ds_pre.v
    return dict(lik_blocked=int((clamped & (a.glik >= 0)).sum()), lik_passes=int((clamped & (a.glik < 0)).sum()),
                sigma_passes=int((small & (ds < 0)).sum()), sigma_blocked=int((small & (ds > 0)).sum()),
                exact_zero=int((a.dd == 0).sum()))


def gc_formula(c, a, training, out_dtype, use_gyp=True, dy0=True):
    """gc_bwd_kernel's formula in E arithmetic, its branches decided by the reference `a`"""
    sl = slice(c.yoff, c.yoff + c.sw)
    yv, mv, sr = E(c.y[:, sl]), E(c.mu), E(c.sigma)
    if training:
        xt = yv + E(_mc(c, c.noise))
    else:
        xt = E(torch.round(yv.v - mv.v)) + mv
    s = sr.where(sr.v >= 0.11, E.const(0.11))
    dd = xt - mv
    v = dd.abs()
    aa, bb = (0.5 - v) / s, (-0.5 - v) / s
    g = E(a.glik).exact(((a.raw >= 1e-9) | (a.glik < 0)).double())
    c0 = E.const(1.0 / math.sqrt(2.0 * math.pi))
    pa = c0 * (aa * aa).exact(-0.5).mono(torch.exp)
    pb = c0 * (bb * bb).exact(-0.5).mono(torch.exp)
    dv = g * (pb - pa) / s
    ds_pre = g * (bb * pb - aa * pa) / s
    ds = ds_pre.exact(((sr.v >= 0.11) | (ds_pre.v < 0)).double())
    ddd = dv.exact(torch.sign(a.dd))
    gyp = E(c.gyp[:, sl]) if use_gyp else E(torch.zeros(c.M, c.sw))
    if training:
        dyv, dmv = gyp + ddd, -ddd
    else:
        dyv, dmv = gyp, E(torch.zeros(c.M, c.sw))  # -ddd + ddd: exactly zero
    dy = dyv.acc(c.dy0[:, sl]) if dy0 else dyv
    return NS(dy=dy, dmu=dmv.store(out_dtype), dsigma=ds.store(out_dtype), ds_pre=ds_pre, ddd=ddd)


def gc_bwd_reference(c, training, out_dtype, use_glik=True, use_gyp=True):
    """{dy [M][Mtot] (the slice accumulated into dy0, the other columns untouched), dmu, dsigma: (ref, bound)}, the
    skip mask [M][sw] and the reference's intermediates"""
    a = gc_autograd(c, training, use_glik, use_gyp)
    a.training = training
    f = gc_formula(c, a, training, out_dtype, use_gyp)
    sl = slice(c.yoff, c.yoff + c.sw)
    dy_ref, dy_bound = c.dy0.double().clone(), torch.zeros(c.M, c.Mtot, dtype=F64)
    dy_ref[:, sl] += a.dy
    dy_bound[:, sl] = f.dy.e
    skip = gc_skip(c, training, a)
    dy_skip = torch.zeros(c.M, c.Mtot, dtype=torch.bool)
    dy_skip[:, sl] = skip.any
    out = {"dy": (dy_ref, dy_bound, dy_skip), "dmu": (a.dmu, f.dmu.e, skip.any), "dsigma": (a.dsigma, f.dsigma.e, skip.any)}
    return out, skip, a, f


# ------------------------------------------------------------------------------------ EntropyBottleneck backward
def eb_module(tmae, C, seed=0):
    """tmae.EntropyBottleneck(C) perturbed as the kernel tests' _eb_module does"""
    from test_gpu_kernels import _eb_module

    return _eb_module(tmae, C, seed)


EB_KEYS = [f"_matrix{i}" for i in range(5)] + [f"_bias{i}" for i in range(5)] + [f"_factor{i}" for i in range(4)]
EB_SIZES = {"sub_wave": (2, 9), "one_pass": (3, 35), "two_pass": (3, 91)}  # (n, HW): n HW = 18, 105, 273
# seeds fixed on the CPU; training form: clamped share 28 % / 30 % / 30 %, likelihood band (the skipped dz elements)
# 0 of 90 / 0 of 525 / 1 of 1365; the eval form skips nothing (dz = gzhat there).  test_glue_checker.test_eb_census
# asserts the shares, the classes and the cap
EB_SEEDS = {"sub_wave": 11, "one_pass": 12, "two_pass": 13}
EB_FAR = (1.2, 2.5)  # clamped elements sit at this multiple of their channel's clamp threshold (same side)


def eb_thresholds(sd):
    """per channel, the largest |x| on either side at which the float64 likelihood still reaches 1e-9 -> [C][2]
    (negative side, positive side), from a scan of the density in steps of 0.005"""
    C = sd[EB_PRE + "_matrix0"].shape[0]
    sd64 = {k: v.double() for k, v in sd.items()}
    xs = torch.linspace(-10, 10, 4001, dtype=F64)
    x = xs.reshape(1, 1, -1).expand(C, 1, -1)
    lo, up = eb_logits(sd64, EB_PRE, x - 0.5), eb_logits(sd64, EB_PRE, x + 0.5)
    sg = -torch.sign(lo + up)
    ok = (torch.sigmoid(sg * up) - torch.sigmoid(sg * lo)).abs()[:, 0, :] >= 1e-9
    thr = torch.empty(C, 2, dtype=F64)
    for c in range(C):
        idx = torch.nonzero(ok[c]).flatten()
        thr[c, 0], thr[c, 1] = -xs[idx[0]], xs[idx[-1]]
    assert bool((thr > 0.05).all()) and bool((thr < 9.5).all()), thr
    return thr


def eb_case(eb, size, seed=None):
    """eb: a tmae.EntropyBottleneck(C) perturbed like test_gpu_kernels._eb_module, on the CPU; one raw _matrix entry
    is set to 21 (past the softplus threshold).  The density's tails are logistic and the perturbed channels clamp
    anywhere between |x| = 0.5 and 3, so a single Gaussian z that clamps 5 % .. 50 % puts far more than 2 % of the
    elements into the band [1e-10, 1e-8].  The case therefore places x = z + noise itself, from the float64 density
    alone: 7 in 10 elements ~ N(0,1) thr / 4 (unclamped), 3 in 10 at EB_FAR thr on either side (clamped, yet with a
    gradient that f32 still holds), thr the channel's clamp threshold on that side; a few elements at +-60 (certain
    clamps, zero gradient); an element within 2e-3 of a round-to-nearest tie of z - median is moved by a quarter"""
    n, HW = EB_SIZES[size]
    sd = {EB_PRE + k: v.detach().clone().float().cpu() for k, v in eb.state_dict().items()}
    sd[EB_PRE + "_matrix2"][1, 2, 0] = 21.0
    C = sd[EB_PRE + "_matrix0"].shape[0]
    g = _gen(EB_SEEDS[size] if seed is None else seed)
    N = n * HW
    thr = eb_thresholds(sd).float()
    noise = torch.rand(n, C, HW, generator=g) - 0.5
    side = (torch.rand(N, C, generator=g) < 0.5).long()  # 0: negative
    t = torch.gather(thr.t(), 0, side)  # [N][C]
    sgn = side.float() * 2 - 1
    far = torch.rand(N, C, generator=g) < 0.3
    mag = EB_FAR[0] + (EB_FAR[1] - EB_FAR[0]) * torch.rand(N, C, generator=g)
    core = torch.randn(N, C, generator=g) * thr.min(1).values.reshape(1, C) / 4
    x = torch.where(far, sgn * mag * t, core)
    z = x - noise.permute(0, 2, 1).reshape(N, C)  # NHWC
    for k in range(8):
        z[(7 * k + 2) % N, k % C] = 60.0 if k % 2 else -60.0
    d = z - sd[EB_PRE + "quantiles"][:, 0, 1].reshape(1, C)
    z = torch.where(((d - torch.floor(d)) - 0.5).abs() < 2e-3, z + 0.25, z)
    glik = torch.randn(n, C, HW, generator=g)
    gzhat = torch.randn(N, C, generator=g)
    acc0 = {k: torch.randn(sd[EB_PRE + k].shape, generator=g) for k in EB_KEYS}
    return NS(size=size, n=n, HW=HW, C=C, N=N, sd=sd, z=z, noise=noise, glik=glik, gzhat=gzhat, acc0=acc0)


def _cn(c, t):
    """NCHW [n][C][HW] -> [C][n HW] (the oracle's and the kernel's per-channel element order)"""
    return t.permute(1, 0, 2).reshape(c.C, c.N)


def eb_autograd(c, training, use_glik=True, use_gzhat=True, dtype=F64):
    """dz [N][C] and the fourteen parameter gradients by autograd through the oracle's forms, in `dtype`"""
    sd = {k: v.to(dtype).requires_grad_(k[len(EB_PRE):] in EB_KEYS) for k, v in c.sd.items()}
    z = c.z.to(dtype).requires_grad_(True)
    values = z.t().reshape(c.C, 1, c.N)
    med = sd[EB_PRE + "quantiles"][:, :, 1:2].detach()
    if training:
        x = values + _cn(c, c.noise).to(dtype).reshape(c.C, 1, c.N)
    else:
        x = torch.round(values - med).detach() + med
    lower, upper = eb_logits(sd, EB_PRE, x - 0.5), eb_logits(sd, EB_PRE, x + 0.5)
    sign = (-torch.sign(lower + upper)).detach()
    raw = torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower))
    lik = orc.lower_bound(raw, 1e-9)
    zhat = orc.quantize_ste(values - med) + med
    glik = _cn(c, c.glik).to(dtype).reshape(c.C, 1, c.N) if use_glik else torch.zeros_like(raw)
    gz = c.gzhat.to(dtype).t().reshape(c.C, 1, c.N) if use_gzhat else torch.zeros_like(raw)
    ((glik * lik).sum() + (gz * zhat).sum()).backward()
    grads = {k: (sd[EB_PRE + k].grad if sd[EB_PRE + k].grad is not None else torch.zeros_like(sd[EB_PRE + k])).detach()
             for k in EB_KEYS}
    return NS(dz=z.grad.detach(), grads=grads, raw=raw.detach().reshape(c.C, c.N), sign=sign.reshape(c.C, c.N),
              glik=glik.detach().reshape(c.C, c.N), x=x.detach().reshape(c.C, c.N))


def _softplus_k(x):
    return torch.where(x > 20.0, x, torch.log1p(torch.exp(x.clamp_max(30.0))))


def _sigmoid_e(x):
    """1 / (1 + expf(-x)): expf's relative error d moves the quotient by d (1 - sigmoid) <= d relatively; the addition
    and the division round once each.  An overflowing expf gives 0 for a value below the smallest normal (TINY)"""
    return x.mono(torch.sigmoid, ulps=LIBM_ULP + 2)


def eb_pack(sd):
    """eb_load: the packed per-channel quantities as E tensors [C][1]"""
    def col(key, i, j=0):
        return sd[EB_PRE + key][:, i, j].double().reshape(-1, 1)

    sp = lambda t: E(t).mono(_softplus_k, ulps=2 * LIBM_ULP + 1)  # noqa: E731  log1pf(expf(x))
    w = NS()
    w.sp0 = [sp(col("_matrix0", j)) for j in range(3)]
    w.b0 = [E(col("_bias0", j)) for j in range(3)]
    w.tf0 = [E(col("_factor0", j)).mono(torch.tanh) for j in range(3)]
    w.sp = [[sp(col(f"_matrix{l + 1}", e // 3, e % 3)) for e in range(9)] for l in range(3)]
    w.bl = [[E(col(f"_bias{l + 1}", j)) for j in range(3)] for l in range(3)]
    w.tf = [[E(col(f"_factor{l + 1}", j)).mono(torch.tanh) for j in range(3)] for l in range(3)]
    w.sp4 = [sp(col("_matrix4", 0, k)) for k in range(3)]
    w.b4 = E(col("_bias4", 0))
    return w


def eb_net(w, v, go=None):
    """eb_fwd_bwd in E arithmetic: f(v); with go also the 58 packed gradient terms per element and df/dv * go"""
    u, th, h = [[None] * 3 for _ in range(4)], [[None] * 3 for _ in range(4)], [[None] * 3 for _ in range(4)]
    for j in range(3):
        u[0][j] = w.sp0[j] * v + w.b0[j]
        th[0][j] = u[0][j].mono(torch.tanh)
        h[0][j] = u[0][j] + w.tf0[j] * th[0][j]
    for l in range(3):
        for i in range(3):
            u[l + 1][i] = (w.sp[l][3 * i] * h[l][0] + w.sp[l][3 * i + 1] * h[l][1] + w.sp[l][3 * i + 2] * h[l][2]) + w.bl[l][i]
            th[l + 1][i] = u[l + 1][i].mono(torch.tanh)
            h[l + 1][i] = u[l + 1][i] + w.tf[l][i] * th[l + 1][i]
    f = (w.sp4[0] * h[3][0] + w.sp4[1] * h[3][1] + w.sp4[2] * h[3][2]) + w.b4
    if go is None:
        return f
    gr = [None] * 58
    dh = [go * w.sp4[k] for k in range(3)]
    for k in range(3):
        gr[54 + k] = go * h[3][k]
    gr[57] = go
    for l in (2, 1, 0):
        du = [dh[i] * (1.0 + w.tf[l][i] * (1.0 - th[l + 1][i] * th[l + 1][i])) for i in range(3)]
        dprev = [None] * 3
        for i in range(3):
            gr[45 + 3 * l + i] = dh[i] * th[l + 1][i]
            gr[36 + 3 * l + i] = du[i]
            for j in range(3):
                gr[9 + 9 * l + 3 * i + j] = du[i] * h[l][j]
                t = w.sp[l][3 * i + j] * du[i]
                dprev[j] = t if dprev[j] is None else dprev[j] + t
        dh = dprev
    d = None
    for j in range(3):
        du = dh[j] * (1.0 + w.tf0[j] * (1.0 - th[0][j] * th[0][j]))
        gr[6 + j] = dh[j] * th[0][j]
        gr[3 + j] = du
        gr[j] = du * v
        t = w.sp0[j] * du
        d = t if d is None else d + t
    return f, gr, d


def eb_formula(c, a, training, accumulate, use_gzhat=True):
    """eb_bwd_kernel's formula in E arithmetic -> dz E [N][C], {key: E in the parameter's shape}, band [C][N]"""
    w = eb_pack(c.sd)
    med = c.sd[EB_PRE + "quantiles"][:, 0, 1].double().reshape(-1, 1)
    zv = E(c.z.double().t())
    x = zv + E(_cn(c, c.noise)) if training else E(torch.round(zv.v - med)) + E(med)
    xu, xl = x + 0.5, x - 0.5
    upper, lower = eb_net(w, xu), eb_net(w, xl)
    s = a.sign
    su, sl = _sigmoid_e(upper.exact(s)), _sigmoid_e(lower.exact(s))
    sg = torch.sign(su.v - sl.v)
    G = E(a.glik)  # unmasked: the terms are linear in it, the LowerBound mask is applied at the end
    gu = (G * su * (1.0 - su)).exact(sg * s)
    glo = (G * sl * (1.0 - sl)).exact(-sg * s)
    _, gru, dvu = eb_net(w, xu, gu)
    _, grl, dvl = eb_net(w, xl, glo)
    passes = ((a.raw >= 1e-9) | (a.glik < 0)).double()
    band = (a.raw >= 1e-10) & (a.raw <= 1e-8)
    unsure = band & (a.glik >= 0)  # an f32 evaluation may decide the clamp the other way: the whole term is error

    def masked(t):
        return E(t.v * passes, torch.where(unsure, t.v.abs() + t.e, t.e * passes))

    gz = E(c.gzhat.double().t()) if use_gzhat else None
    live = masked(dvu + dvl) if training else E(torch.zeros(c.C, c.N))
    dz = live if gz is None else (gz + live if training else gz)
    tot = [cat([masked(gru[k]), masked(grl[k])], 1).sum(1) for k in range(58)]  # [C] each

    def chain(t, key, i, j, kind):
        p = c.sd[EB_PRE + key][:, i, j].double()
        if kind == "sp":  # softplus' = sigmoid below the threshold 20, 1 above
            fac = _sigmoid_e(E(p)).where(p <= 20.0, E(torch.ones_like(p)))
            return t * fac
        if kind == "tf":
            th = E(p).mono(torch.tanh)
            return t * (1.0 - th * th)
        return t

    out = {}

    def put(key, i, j, e):
        if key not in out:
            shp = c.sd[EB_PRE + key].shape
            out[key] = E(torch.zeros(shp, dtype=F64))
        out[key].v[:, i, j], out[key].e[:, i, j] = e.v, e.e

    for k in range(3):
        put("_matrix0", k, 0, chain(tot[k], "_matrix0", k, 0, "sp"))
        put("_bias0", k, 0, tot[3 + k])
        put("_factor0", k, 0, chain(tot[6 + k], "_factor0", k, 0, "tf"))
        put("_matrix4", 0, k, chain(tot[54 + k], "_matrix4", 0, k, "sp"))
    put("_bias4", 0, 0, tot[57])
    for l in range(3):
        for e in range(9):
            put(f"_matrix{l + 1}", e // 3, e % 3, chain(tot[9 + 9 * l + e], f"_matrix{l + 1}", e // 3, e % 3, "sp"))
        for j in range(3):
            put(f"_bias{l + 1}", j, 0, tot[36 + 3 * l + j])
            put(f"_factor{l + 1}", j, 0, chain(tot[45 + 3 * l + j], f"_factor{l + 1}", j, 0, "tf"))
    if accumulate:
        out = {k: v.acc(c.acc0[k]) for k, v in out.items()}
    return E(dz.v.t(), dz.e.t()), out, band


def eb_bwd_reference(c, training, accumulate=False, use_glik=True, use_gzhat=True):
    """{"dz" and the fourteen keys: (ref, bound, skip)}; dz's skip is the likelihood band (and round ties in eval)"""
    a = eb_autograd(c, training, use_glik, use_gzhat)
    dz, grads, band = eb_formula(c, a, training, accumulate, use_gzhat)
    skip = band.t() if training else torch.zeros(c.N, c.C, dtype=torch.bool)
    if not training:
        med = c.sd[EB_PRE + "quantiles"][:, 0, 1].double().reshape(1, -1)
        d = c.z.double() - med
        tie = ((d - torch.floor(d)) - 0.5).abs() < 1e-3
        assert not bool(tie.any()), "eb case: a round tie (choose another seed)"
    out = {"dz": (a.dz, dz.e, skip)}
    for k in EB_KEYS:
        ref = a.grads[k] + (c.acc0[k].double() if accumulate else 0.0)
        out[k] = (ref, grads[k].e, None)
    return out, a, NS(dz=dz, grads=grads, band=band)


def eb_census(a):
    clamped = a.raw < 1e-9
    return dict(blocked=int((clamped & (a.glik >= 0)).sum()), passes=int((clamped & (a.glik < 0)).sum()),
                share=float(clamped.double().mean()), band=int(((a.raw >= 1e-10) & (a.raw <= 1e-8)).sum()))


def eb_aux_autograd(sd, dtype=F64):
    sd = {k: v.detach().clone().to(dtype) for k, v in sd.items()}
    q = sd[EB_PRE + "quantiles"].requires_grad_(True)
    orc.aux_loss(sd, EB_PRE).backward()
    return q.grad.detach()


def eb_aux_reference(sd, gout=None, acc0=None):
    """(ref, bound) of tmae_eb_aux_bwd's dq [C][1][3] = g sign(f(q) - target) f'(q), and the distance of every
    quantile from the kink f(q) == target, in units of q"""
    ref = eb_aux_autograd(sd)
    w = eb_pack(sd)
    q = sd[EB_PRE + "quantiles"][:, 0, :].double()  # [C][3]
    f, _, d = eb_net(w, E(q), E(torch.ones_like(q)))
    r = f.v - sd[EB_PRE + "target"].double().reshape(1, 3)
    out = d.exact(torch.sign(r))
    g = 1.0 if gout is None else float(gout)
    if gout is not None:
        out = out * E(torch.full_like(q, g))
        ref = ref * g
    if acc0 is not None:
        out = out.acc(acc0.double().reshape(-1, 3))
        ref = ref + acc0.double()
    kink = (r.abs() / d.v.abs().clamp_min(1e-300)).min()
    return ref.reshape(1, -1), out.e.reshape(1, -1), float(kink), out.v.reshape(1, -1)


# ------------------------------------------------------------------------------------ rate term
def bpp_case(ny, nz, seed=5):
    """likelihoods in [1e-9, 1], log-uniform, with exact 1e-9 (as f32) and 1.0 on both sides of the i < na seam"""
    g = _gen(seed)
    y = torch.exp(torch.rand(ny, generator=g) * math.log(1e-9)).clamp(1e-9, 1.0)
    z = torch.exp(torch.rand(nz, generator=g) * math.log(1e-9)).clamp(1e-9, 1.0)
    y[0], y[-1], z[0], z[-1] = 1e-9, 1.0, 1.0, 1e-9
    return y, z


def bpp_sum_reference(y, z, num_pixels):
    """accumulated in f64 by the kernel: each term logf(v) is off by 2u |log v| + u at the most (the function's ulps,
    and an absolute u near log 1 = 0); the f32 store of the scaled sum rounds once more"""
    lv = torch.cat([torch.log(y.double()), torch.log(z.double())])
    scale = 1.0 / (-math.log(2.0) * num_pixels)
    ref = lv.sum() * scale
    bound = (2 * U * lv.abs() + U).sum() * abs(scale)
    return ref.reshape(1, 1), (bound + U * (ref.abs() + bound)).reshape(1, 1)


def bpp_bwd_reference(lik, gout, num_pixels):
    out = E(torch.full_like(lik.double(), float(gout))) * E.const(1.0 / (-math.log(2.0) * num_pixels)) / E(lik)
    ref = float(gout) / (lik.double() * (-math.log(2.0) * num_pixels))
    return ref.reshape(1, -1), out.e.reshape(1, -1), out.v.reshape(1, -1)


# ------------------------------------------------------------------------------------ elementwise backward pieces
def lrp_case(rows=37, C=20, seed=6):
    g = _gen(seed)
    t = torch.randn(rows, C, generator=g) * 4
    t[0, :4] = torch.tensor([12.0, -12.0, 0.0, 9.5])  # saturated tanh
    return NS(rows=rows, C=C, t=t, g32=torch.randn(rows, C, generator=g), g32b=torch.randn(rows, C, generator=g),
              g16=torch.randn(rows, C, generator=g))


def lrp_reference(c, dtype, use=("g32", "g32b", "g16")):
    """dt = g 0.5 (1 - tanh(t)^2) in dtype and gsum = g (f32); g16 is read in dtype"""
    g = None
    for name in ("g32", "g32b", "g16"):
        if name in use:
            v = getattr(c, name)
            e = E(v.to(dtype) if name == "g16" else v)
            g = e if g is None else g + e
    if g is not None and "g32" not in use:
        g = E(g.v, g.e + U * g.v.abs())  # the kernel starts from 0.0f + ...: one more (exact) addition, kept for slack
    th = E(c.t).mono(torch.tanh)
    dt = (g.exact(0.5) * (1.0 - th * th)).store(dtype)
    ref_g = g.v
    ref_dt = ref_g * 0.5 * (1.0 - torch.tanh(c.t.double()) ** 2)
    return {"dt": (ref_dt, dt.e), "gsum": (ref_g, g.e)}


def gelu_factor(pre):
    """(GELU'(p), bound d on common.h gelu_grad's error) in float64"""
    p = pre.double()
    g, g2 = gelu_grad64(p)
    phi = torch.exp(-0.5 * p * p) / math.sqrt(2.0 * math.pi)
    d = 0.5 * ERF_F32_ERR + g2 * (U * p.abs()) + 4 * 2.0 ** -24 * g.abs() + p.abs() * phi * (2 * U * p * p + 4 * U)
    return g, d


def gelu_bwd_reference(dy, pre, dtype):
    """out = dy gelu'(pre) in dtype (dy, pre already in the dtypes the kernel reads; pre None: out = dy)"""
    a = dy.double()
    if pre is None:
        ref, bound = a, torch.zeros_like(a)
    else:
        g, d = gelu_factor(pre)
        ref = a * g
        bound = a.abs() * d + U * ref.abs()
    if dtype == BF16:
        bound = bound + BF16_ROUND * (ref.abs() + bound)
    return ref, bound


def unshuffle_index(n, H, W, C4):
    """for out [n H W][C4]: (row of the pixel-shuffled [n 2H 2W][C4 / 4] tensor, its column)"""
    m = torch.arange(n * H * W).reshape(-1, 1)
    co = torch.arange(C4).reshape(1, -1)
    b, rem = m // (H * W), m % (H * W)
    y, x = rem // W, rem % W
    c, si, sj = co // 4, (co // 2) % 2, co % 2
    at = (b * 2 * H + 2 * y + si) * 2 * W + 2 * x + sj
    return at, c.expand_as(at)


def gelu_case(total=1000, seed=4):
    g = _gen(seed)
    pre = torch.linspace(-6, 6, total)[torch.randperm(total, generator=g)]
    pre[0] = 0.0
    return torch.randn(total, generator=g), pre


def unshuffle_case(n=2, H=3, W=5, C4=12, seed=14):
    g = _gen(seed)
    rows, c = n * 4 * H * W, C4 // 4
    return NS(n=n, H=H, W=W, C4=C4, dy=torch.randn(rows, c, generator=g), pre=torch.randn(rows, c, generator=g) * 2)


def unshuffle_reference(c, dy_dt, dt, use_pre=True, swap=False):
    at, ch = unshuffle_index(c.n, c.H, c.W, c.C4)
    if swap:  # the fault: sub-pixel (i, j) taken as (j, i)
        co = torch.arange(c.C4).reshape(1, -1)
        m = torch.arange(c.n * c.H * c.W).reshape(-1, 1)
        b, rem = m // (c.H * c.W), m % (c.H * c.W)
        y, x = rem // c.W, rem % c.W
        at = (b * 2 * c.H + 2 * y + co % 2) * 2 * c.W + 2 * x + (co // 2) % 2
    dy = c.dy.to(dy_dt)[at, ch]
    pre = c.pre.to(dt)[at, ch] if use_pre else None
    return dy, pre, gelu_bwd_reference(dy, pre, dt)


def colsum_case(rows, C, total=None, seed=15):
    g = _gen(seed + rows + C)
    return torch.randn(total or rows, C, generator=g) + 0.25, torch.randn(C, generator=g)



# ------------------------------------------------------------------------------------ reductions
def colsum_reference(x, rows, G=None, Gs=0, off=0, acc0=None):
    """column sums over the (remapped) rows of x (already in the dtype the kernel reads)"""
    src = remap_rows(rows, G or max(rows, 1), Gs, off)
    t = x.double()[src]
    ref = t.sum(0)
    bound = (rows + 2) * U * t.abs().sum(0)
    if acc0 is not None:
        bound = bound + U * (acc0.double().abs() + ref.abs() + bound)
        ref = ref + acc0.double()
    return ref.reshape(1, -1), bound.reshape(1, -1)


def ln_case(rows, D, G=None, Gs=0, off=0, seed=8):
    g = _gen(seed + D + rows)
    src = remap_rows(rows, G or max(rows, 1), Gs, off)
    total = int(src.max()) + 1 + (1 if G else 0)
    return NS(rows=rows, D=D, G=G, Gs=Gs, off=off, src=src, total=total, eps=1e-6,
              x=torch.randn(total, D, generator=g) * 1.5 + 0.3, gamma=1 + 0.1 * torch.randn(D, generator=g),
              dy=torch.randn(rows, D, generator=g), dres=torch.randn(total, D, generator=g),
              dg0=torch.randn(D, generator=g), db0=torch.randn(D, generator=g), dr0=torch.randn(D, generator=g))


def ln_bwd_reference(c, use_dres, op_dtype=None, accumulate=False):
    """layernorm_bwd_kernel's formula in E arithmetic (its value IS the float64 reference: the same closed form as
    autograd's, checked against torch.autograd in test_glue_checker.py).  Returns {dx (remapped rows only), dxop,
    dgamma, dbeta, dres_colsum: (ref, bound)}"""
    D = c.D
    x, dy, gm = E(c.x[c.src]), E(c.dy), E(c.gamma.reshape(1, D))
    invD = 1.0 / D
    mean = x.sum(1) * E.const(invD) if D & (D - 1) else x.sum(1).exact(invD)
    mean = E(mean.v.reshape(-1, 1), mean.e.reshape(-1, 1))
    d = x - mean
    q = (d * d).sum(1) / float(D) + E.const(c.eps)
    rstd = 1.0 / q.mono(torch.sqrt)
    rstd = E(rstd.v.reshape(-1, 1), rstd.e.reshape(-1, 1))
    xh = d * rstd
    gg = dy * gm
    sa, sb = gg.sum(1) / float(D), (gg * xh).sum(1) / float(D)
    sa, sb = E(sa.v.reshape(-1, 1), sa.e.reshape(-1, 1)), E(sb.v.reshape(-1, 1), sb.e.reshape(-1, 1))
    dx = rstd * (gg - sa - xh * sb)
    if use_dres:
        dx = dx + E(c.dres[c.src])
    out = {"dx": dx.out(), "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0)}
    if op_dtype is not None:
        out["dxop"] = dx.store(op_dtype).out()
    if use_dres:
        out["dres_colsum"] = E(c.dres[c.src]).sum(0)
    for k, a0 in (("dgamma", c.dg0), ("dbeta", c.db0), ("dres_colsum", c.dr0)):
        if k in out:
            e = out[k].acc(a0) if accumulate else out[k]
            out[k] = (e.v.reshape(1, -1), e.e.reshape(1, -1))
    return out


def dec_gather_case(n, L, D, seed=9):
    g = _gen(seed + L)
    ids = torch.stack([torch.randperm(L, generator=g) for _ in range(n)])
    return NS(n=n, L=L, D=D, ids=ids, grad=torch.randn(n * (L + 1), D, generator=g), dmask0=torch.randn(D, generator=g))


def dec_gather_reference(c, ntok, dtype, accumulate=False):
    """tok_grad [n ntok][D]: token k of image b sat at decoder row 0 (k == 0) or 1 + ids[b][k - 1]; dmask [D]: the sum
    over the images and the masked positions mi in [ntok - 1, L) of row 1 + ids[b][mi]"""
    g = c.grad.reshape(c.n, c.L + 1, c.D)
    rows = torch.cat([torch.zeros(c.n, 1, dtype=torch.long), 1 + c.ids[:, :ntok - 1]], 1)
    tok = torch.gather(g, 1, rows.unsqueeze(-1).expand(-1, -1, c.D)).reshape(c.n * ntok, c.D)
    mrows = 1 + c.ids[:, ntok - 1:]
    terms = torch.gather(g, 1, mrows.unsqueeze(-1).expand(-1, -1, c.D)).double().reshape(-1, c.D)
    ref = terms.sum(0)
    bound = (terms.shape[0] + 2) * U * terms.abs().sum(0)
    if accumulate:
        bound = bound + U * (c.dmask0.double().abs() + ref.abs() + bound)
        ref = ref + c.dmask0.double()
    tref = tok.double()
    tbound = BF16_ROUND * tref.abs() if dtype == BF16 else torch.zeros_like(tref)
    return {"tok": (tref, tbound), "dmask": (ref.reshape(1, -1), bound.reshape(1, -1))}


def patch_gather_values(imgs, ids, keep, P):
    """[n keep][Kw] f32: rows (c, py, px) of the kept patches, Kw = C P P rounded up to 8, the tail zero"""
    n, C, H, W = imgs.shape
    Gw = W // P
    KP = C * P * P
    Kw = (KP + 7) // 8 * 8
    out = torch.zeros(n * keep, Kw)
    for b in range(n):
        for k in range(keep):
            p = int(ids[b, k])
            hy, hx = p // Gw, p % Gw
            out[b * keep + k, :KP] = imgs[b, :, hy * P:(hy + 1) * P, hx * P:(hx + 1) * P].reshape(-1)
    return out


# ------------------------------------------------------------------------------------ forward extras
def lse_reference(qkv, B, T, H, dh, scale):
    """lse[b][h][t] = log2 sum_j exp(scale q_t . k_j) (base 2, as tmae_mha_bwd reads it), float64, from qkv already
    rounded to the operand dtype.  Each score is a length-dh dot product: off by (dh + 2) u sum |q k| scale at the
    most, plus the rounding of the scale product; log2 sum exp is 1-Lipschitz in the max norm of the scores up to
    1 / ln 2; the sum of the T exponentials is off by (T + 2) u relatively, i.e. by (T + 2) u / ln 2 after the log2;
    the exp2 / log2 evaluations and the running-max rescaling add a few ulps of the result and of 1."""
    t = qkv.double().reshape(B, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    q, k = t[0], t[1]
    s = (q @ k.transpose(-2, -1)) * scale
    S = (q.abs() @ k.abs().transpose(-2, -1)) * scale
    ref = torch.logsumexp(s, -1) / math.log(2.0)
    e_s = ((dh + 2) * U * S + 2 * U * s.abs()).max(-1).values
    bound = (e_s + (T + 2) * U) / math.log(2.0) + 2 * LIBM_ULP * U * (ref.abs() + 1.0)
    return ref.reshape(1, -1), bound.reshape(1, -1)
