"""Element-wise checker of the FORWARD entropy models and of the coding kernels (tests/test_gpu_entropy_fwd.py on the
GPU, tests/test_glue_checker.py for the checker itself on the CPU): the sibling of glue_check.py, whose E arithmetic,
eb_pack / eb_net, Guarded and check it uses.

Why the older metric is not enough: likelihoods lie in [1e-9, 1] and the loss is -log2(lik), so the RELATIVE error of
every element counts; max|a - b| / max|b| < 1e-5 sees nothing below 1e-4.

Every kernel gets (ref, bound) per element.  ref is float64 from inputs already rounded to f32; bound carries the
kernel's own formula through E (glue_check's rules: half an ulp per add / mul / div, 4 ulp per libm call and the exact
image of the argument's interval, u |c| per f32 constant, 2^-126 for flush to zero):

  GaussianConditional  s = max(sigma, 0.11f) (the constant's u |c| first); x~ = y + noise, or rint(fl32(y - mu)) + mu
                       with mu subtracted back in f32 as compressai does; v = |x~ - mu|;
                       raw = 0.5 erfc(k (0.5 - v) / s) - 0.5 erfc(k (-0.5 - v) / s), k = -1 / sqrt 2 as f32;
                       lik = max(raw, 1e-9f)
  EntropyBottleneck    x = z + noise, or rint(fl32(z - med)) + med; lower, upper = f(x -+ 0.5) through eb_pack / eb_net;
                       s = -sign(lower + upper); raw = |sigmoid(s upper) - sigmoid(s lower)|; the same clamp
  aux loss             sum over 3 C terms |f(q) - target|: the any-order sum rule
  pmf rows, tails      the two raw forms without the clamp; tail = 2 lower[0] (GC), sigmoid(lower[0]) +
                       sigmoid(-upper[max_length - 1]) (EB: upstream's last sample of the PADDED range)

No element is skipped, and the reasons are written here once:
  * both clamps are continuous.  |max(a', c') - max(a, c)| <= max(|a' - a|, |c' - c|), so whichever side of 1e-9 (or of
    0.11) the f32 evaluation lands on, the output is within max(bound of raw, u 1e-9) of max(raw, 1e-9): 1e-9f is not
    1e-9, hence the u 1e-9.  The same holds for max(sigma, 0.11f) through E.const.
  * the EB sign choice is symmetric: |sigmoid(s u) - sigmoid(s l)| is the same real number for s = +-1.  Where
    |lower + upper| is within its own error of zero the f32 evaluation may pick the other s; there the bound is the
    larger of the two forms' bounds (plus the float64 distance of the two forms, which is rounding only).
  * rintf acts on fl32(y - mu), a correctly rounded f32 difference, which torch computes bit for bit on the CPU: the
    rounded integer is taken from that f32 evaluation, never from a float64 difference (a tie 0.5 in f32 can be
    0.5 + 1e-9 in float64).
Everything else is integer or rounded once, so its reference is exact and its bound 0: yhat32, zhat (a bf16 store
carries 2^-8 |v|), symbols, indexes, dequantised values, the inverse permutation, the coder order
[slice][image][channel][pixel].

Integer outputs go into GuardedInt: sentinel-filled, guard elements on all sides.
"""
import math
from types import SimpleNamespace as NS

import torch

import glue_check as gk
import parity_log
from gemm_check import BF16_ROUND
from glue_check import BF16, F32, F64, E, U, Guarded
from oracle import coding_oracle as co
from oracle import mcm_oracle as orc

I32, I64 = torch.int32, torch.int64
SENTINEL = -0x5A5A5A5
LIK_MIN = 1e-9
K_ERFC = -1.0 / math.sqrt(2.0)


class GuardedInt(Guarded):
    """Guarded for integer dtypes: SENTINEL where the float buffers hold NaN"""

    def __init__(self, M, N, dtype=I32, device="cpu", init=None):
        self.M, self.N, self.ld = M, N, N + 2 * self.GC
        self.buf = torch.full((M + 2 * self.GR, self.ld), SENTINEL, dtype=dtype, device=device)
        if init is not None:
            self.block()[...] = init.to(dtype).to(device)

    def guard_hits(self):
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        keep[self.GR:self.GR + self.M, self.GC:self.GC + self.N] = False
        return int((self.buf[keep] != SENTINEL).sum())

    def result(self):
        return self.block().detach().cpu().long()


def flat(g):
    """(the whole storage of a Guarded as one row, offset of its view()): what a kernel's pointer arithmetic sees"""
    return g.buf.view(-1), g.GR * g.ld + g.GC


def check_exact(metric, g, ref, log=True):
    """integer outputs: guards at the sentinel, every element equal; logs 0 (or the count of wrong elements)"""
    hits = g.guard_hits()
    assert hits == 0, f"{metric}: {hits} guard elements outside the {g.M} x {g.N} block were written"
    out = g.result().reshape(-1)
    bad = int((out != ref.reshape(-1).long()).sum())
    if log:
        parity_log.record(metric + ":int", float(bad), 1.0)
    assert bad == 0, f"{metric}: {bad} of {out.numel()} integer elements differ"
    return 0.0


def check_bits(metric, g, values, log=True):
    """a float output that must be bitwise `values` (already in the output's dtype, or cast to it here)"""
    ref = values.to(g.buf.dtype).double().reshape(g.M, g.N)
    return gk.check(metric, g, ref, torch.zeros_like(ref), log=log)


# ------------------------------------------------------------------------------------ the two likelihood formulas
def clamp_lik(raw):
    """max(raw, 1e-9f) -> (ref, bound): module docstring, first bullet"""
    return raw.v.clamp_min(LIK_MIN), torch.maximum(raw.e, torch.full_like(raw.e, U * LIK_MIN))


def rint32(a, b=None):
    """rintf(fl32(a - b)) as the kernel computes it (round half to even on the f32 difference)"""
    d = a.float() if b is None else a.float() - b.float()
    return torch.round(d)


def gc_raw(x, sigma, mu=None, noise=None, scale_bound=0.11):
    """gc_slices_kernel / gc_likelihood_kernel in E arithmetic from f32 tensors of one shape -> NS(raw E before the
    clamp, xt f32 bitwise x~, dd E x~ - mu).  noise None: the eval form"""
    if noise is not None:
        xt = E(x) + E(noise)
        xt32 = x.float() + noise.float()
    elif mu is not None:
        qi = rint32(x, mu)
        xt = E(qi) + E(mu)
        xt32 = qi + mu.float()
    else:
        xt = E(rint32(x))
        xt32 = rint32(x)
    dd = xt - E(mu) if mu is not None else xt
    v = dd.abs()
    sr = E(sigma)
    s = sr.where(sr.v >= scale_bound, E.const(scale_bound))
    k = E.const(K_ERFC)
    up = (k * ((0.5 - v) / s)).mono(torch.erfc).exact(0.5)
    lo = (k * ((-0.5 - v) / s)).mono(torch.erfc).exact(0.5)
    return NS(raw=up - lo, xt32=xt32, dd=dd, s=s)


def gc_oracle64(x, sigma, mu, noise, scale_bound=0.11):
    """the oracle's own float64 evaluation at the same x~ (the quantised value comes from the f32 difference)"""
    m = torch.zeros_like(x.double()) if mu is None else mu.double()
    if noise is None:
        xq = rint32(x, mu).double() + m
        return orc.gaussian_conditional(xq, sigma.double(), m, torch.zeros_like(xq), scale_bound)
    return orc.gaussian_conditional(x.double(), sigma.double(), m, noise.double(), scale_bound)


def eb_raw(sd, x):
    """|sigmoid(s upper) - sigmoid(s lower)| at x (E [C][N]) -> NS(raw E with the sign-symmetric bound, lower, upper,
    ambiguous: the elements whose sign an f32 evaluation may decide otherwise)"""
    w = gk.eb_pack(sd)
    lower, upper = gk.eb_net(w, x - 0.5), gk.eb_net(w, x + 0.5)
    ssum = lower + upper
    s = -torch.sign(ssum.v)

    def form(sg):
        return (gk._sigmoid_e(upper.exact(sg)) - gk._sigmoid_e(lower.exact(sg))).abs()

    raw, alt = form(s), form(-s)
    amb = ssum.v.abs() <= ssum.e
    e = torch.where(amb, torch.maximum(raw.e, alt.e + (alt.v - raw.v).abs()), raw.e)
    return NS(raw=E(raw.v, e), lower=lower, upper=upper, ambiguous=amb, sum=ssum)


def eb_x(sd, z_cn, noise_cn=None, med_index=1):
    """the EntropyBottleneck's evaluation point from z [C][N] f32 -> (x E, zhat f32 [C][N] bitwise)"""
    med = sd[gk.EB_PRE + "quantiles"][:, 0, med_index].float().reshape(-1, 1)
    qi = rint32(z_cn, med)
    zhat = qi + med
    x = E(z_cn) + E(noise_cn) if noise_cn is not None else E(qi) + E(med)
    return x, zhat, qi


def eb_aux_loss_reference(sd):
    """(ref, bound) [1][1] of tmae_eb_aux_loss: a sum of 3 C terms, any order"""
    w = gk.eb_pack(sd)
    q = sd[gk.EB_PRE + "quantiles"][:, 0, :].double()
    t = (gk.eb_net(w, E(q)) - E(sd[gk.EB_PRE + "target"].double().reshape(1, 3))).abs()
    tot = E(t.v.reshape(-1), t.e.reshape(-1)).sum(0)
    return tot.v.reshape(1, 1), tot.e.reshape(1, 1)


def gc_pmf_reference(table, center, max_length):
    """gc_pmf_kernel: pmf [n][max_length] and tail [n], each (ref, bound); no clamp"""
    j = torch.arange(max_length).reshape(1, -1)
    s = E((j - center.reshape(-1, 1).long()).abs())  # an integer below 2^24: exact in f32
    sc = E(table.float().reshape(-1, 1))
    k = E.const(K_ERFC)
    up = (k * ((0.5 - s) / sc)).mono(torch.erfc).exact(0.5)
    lo = (k * ((-0.5 - s) / sc)).mono(torch.erfc).exact(0.5)
    pmf = up - lo
    tail = E(lo.v[:, 0], lo.e[:, 0]).exact(2.0)
    return pmf.out(), (tail.v.reshape(1, -1), tail.e.reshape(1, -1))


def eb_pmf_reference(sd, start, max_length):
    """eb_pmf_kernel: x = (float)j + start[c]; tail from lower at j = 0 and upper at the padded range's last sample"""
    j = torch.arange(max_length, dtype=F32).reshape(1, -1)
    x = E(j) + E(start.float().reshape(-1, 1))
    r = eb_raw(sd, x)
    last = max_length - 1
    tail = gk._sigmoid_e(E(r.lower.v[:, 0], r.lower.e[:, 0])) + gk._sigmoid_e(-E(r.upper.v[:, last], r.upper.e[:, last]))
    return r.raw.out(), (tail.v.reshape(1, -1), tail.e.reshape(1, -1))


def build_indexes32(sigma, table, bound=0.11):
    """(nscale - 1) - #{t < nscale - 1 : max(sigma, bound as f32) <= table[t]}, every comparison in f32"""
    s = torch.maximum(sigma.float(), torch.tensor(bound, dtype=F32))
    t = table.float()
    return (t.numel() - 1) - (s.unsqueeze(-1) <= t[:-1]).sum(-1)


# ------------------------------------------------------------------------------------ GaussianConditional cases
def model_table():
    """compressai.models.google.get_scale_table(): the model's 64 entries, 0.11f .. 256"""
    return torch.exp(torch.linspace(math.log(0.11), math.log(256), 64))


def low_table():
    """a table with entries below the scale bound: with the model's table (table[0] == 0.11f) indexes taken from the
    unbounded sigma equal the bounded ones, so that fault can only show against this one"""
    return torch.exp(torch.linspace(math.log(0.03), math.log(64), 24))


TIES = (0.5, 1.5, 2.5, -0.5)


def plant_t(table):
    """the scale-table entries that sigma is set to, and to one ulp either side of (64 entries: 0, 9, 32, 62)"""
    n = table.numel()
    return [0, n // 7, n // 2, n - 2]


def gc_elements(N, seed, table):
    """glue_check.gc_case's recipe (y ~ 3 N(0,1), mu ~ N(0,1), sigma a third in [0.02, 0.09] and the rest in
    [0.13, 2.63], uniform noise) with 15 % of the elements moved into the tails, y = mu +- max(sigma, .11) U(1, 6.5),
    and four elements of every class of gc_census planted at seeded places -> flat f32 tensors"""
    g = gk._gen(seed)
    r = lambda: torch.rand(N, generator=g)  # noqa: E731
    y, mu = 3 * torch.randn(N, generator=g), torch.randn(N, generator=g)
    sigma = torch.where(r() < 1 / 3, 0.02 + 0.07 * r(), 0.13 + 2.5 * r())
    noise = r() - 0.5
    side = torch.where(r() < 0.5, -1.0, 1.0)
    y = torch.where(r() < 0.15, mu + side * sigma.clamp_min(0.11) * (1 + 5.5 * r()), y)
    slots = iter(torch.randperm(N, generator=g).tolist())
    take = lambda: torch.tensor([next(slots) for _ in range(4)])  # noqa: E731
    tab = table.float()
    inf = torch.tensor(float("inf"))
    sigma[take()] = torch.tensor(0.11, dtype=F32)
    sigma[take()] = tab[plant_t(tab)]
    sigma[take()] = torch.nextafter(tab[plant_t(tab)], inf)
    sigma[take()] = torch.nextafter(tab[plant_t(tab)], -inf)
    sigma[take()] = tab[-1] * torch.tensor([1.5, 2.0, 4.0, 1.001])
    for d in TIES:  # quarters: mu, y and y - mu are exact in f32 and in float64
        i = take()
        mu[i] = 0.25 * torch.tensor([1.0, -2.0, 3.0, 5.0])
        y[i] = mu[i] + d
    y[take()] = torch.tensor([0.5, 2.5, -0.5, -2.5])  # ties of rint(x) itself: the form without means
    i = take()  # x~ == mu in training (1.5 + 0.25 - 1.75) and in eval (round(-0.25) + mu)
    y[i], noise[i], mu[i] = 1.5, 0.25, 1.75
    return NS(y=y, mu=mu, sigma=sigma, noise=noise)


def gc_census(x, mu, sigma, noise, table, scale_bound=0.11):
    """the classes the case is there for, counted on the reference alone (mu None: the form without means)"""
    r = gc_raw(x, sigma, mu, noise, scale_bound)
    tab = table.float()
    inf = torch.tensor(float("inf"))
    m = torch.zeros_like(x) if mu is None else mu
    d32, d64 = x.float() - m.float(), x.double() - m.double()
    out = dict(clamped=int((r.raw.v < LIK_MIN).sum()), low=int(((r.raw.v >= LIK_MIN) & (r.raw.v < 1e-4)).sum()),
               sigma_below=int((sigma.double() < 0.11).sum()), sigma_011f=int((sigma == torch.tensor(0.11, dtype=F32)).sum()),
               sigma_on_table=int(torch.isin(sigma, tab).sum()),
               sigma_ulp_above=int(torch.isin(sigma, torch.nextafter(tab, inf)).sum()),
               sigma_ulp_below=int(torch.isin(sigma, torch.nextafter(tab, -inf)).sum()),
               sigma_past_table=int((sigma > tab[-1]).sum()), sign_zero=int((r.dd.v == 0).sum()))
    out["x_tie"] = int((x.double() - torch.floor(x.double()) == 0.5).sum())
    for t in TIES:
        out[f"tie_{t}"] = int(((d32 == t) & (d64 == t)).sum())
    return out


# (n, HW, sw): nslices = 2, yoff = 3, Mtot = yoff + 2 sw + 4.  The tiled kernel runs where HW (sw + 1) <= 4800.
GCF_SHAPES = {"sub_pass": (2, 9, 5),  # 45 elements per workgroup: less than one pass of 1024 threads
              "ragged_pass": (3, 35, 32),  # 1120: the second pass ragged
              "last_tiled": (2, 145, 32),  # 145 x 33 = 4785, the last tiled shape
              "first_element": (1, 146, 32)}  # 4818: the element kernel, 9344 elements = 36.5 workgroups
# seeds fixed on the CPU; measured on the reference, clamped / unclamped below 1e-4 of the slice elements, training | eval
# (test_glue_checker.test_gcf_census prints every class and asserts at least 4 of each):
#   sub_pass      seed 31:   180 elements,   39 /   19 |   32 /   28
#   ragged_pass   seed 32:  6720 elements, 1766 /  698 | 1614 / 1139
#   last_tiled    seed 33: 18560 elements, 4911 / 1999 | 4482 / 3196
#   first_element seed 34:  9344 elements, 2475 /  966 | 2252 / 1576
#   flat (tmae_gc_likelihood_fwd) seed 35: 528 elements, 125 / 45 | 119 / 75 with means, 131 / 53 | 118 / 80 without
# i.e. about a quarter clamped and a third to two fifths below 1e-4.  Planted in every case: sigma == 0.11f 5 (one of
# them table[0]), on a table entry 8, one ulp above / below 4 / 4, past the table 4, ties of y - mu 4 each at 0.5,
# 1.5, 2.5, -0.5, ties of rint(x) 8, x~ == mu 4 in training (eval: every |y - mu| < 0.5 as well)
GCF_SEEDS = {"sub_pass": 31, "ragged_pass": 32, "last_tiled": 33, "first_element": 34, "flat": 35}
NSL, YOFF = 2, 3


def to_nchw(t_mc, n, HW):
    """[n HW][ch] -> flat NCHW [n][ch][HW]"""
    return t_mc.reshape(n, HW, -1).permute(0, 2, 1).reshape(-1)


def coder_order(t, n, HW):
    """[slice][n HW][sw] -> flat [slice][image][channel][pixel]"""
    return t.reshape(t.shape[0], n, HW, -1).permute(0, 1, 3, 2).reshape(-1)


def gcf_case(shape, table, n=None, HW=None):
    """slice case: element values from gc_elements laid out [slice][pixel row m][channel]; the rest of y, the noise
    and the initial contents of every output are random"""
    n0, HW0, sw = GCF_SHAPES[shape]
    n, HW = n or n0, HW or HW0
    M = n * HW
    assert M == n0 * HW0
    Mtot = YOFF + NSL * sw + 4
    el = gc_elements(NSL * M * sw, GCF_SEEDS[shape], table)
    g = gk._gen(GCF_SEEDS[shape] + 1000)
    y, noise = 3 * torch.randn(M, Mtot, generator=g), torch.rand(M, Mtot, generator=g) - 0.5
    sl = slice(YOFF, YOFF + NSL * sw)
    y[:, sl] = el.y.reshape(NSL, M, sw).permute(1, 0, 2).reshape(M, NSL * sw)
    noise[:, sl] = el.noise.reshape(NSL, M, sw).permute(1, 0, 2).reshape(M, NSL * sw)
    c = NS(shape=shape, n=n, HW=HW, sw=sw, nsl=NSL, yoff=YOFF, Mtot=Mtot, M=M, sl=sl, y=y, noise=noise, table=table,
           mu=el.mu.reshape(NSL, M, sw), sigma=el.sigma.reshape(NSL, M, sw),
           lik0=2 + torch.rand(M, Mtot, generator=g), yh0=torch.randn(M, Mtot, generator=g),
           yh32_0=torch.randn(M, Mtot + 3, generator=g), ldy=Mtot + 8, ld_ms=sw + 3)
    c.ms_stride = M * c.ld_ms + 5
    return c


def gcf_slices(c, t_mc):
    """[M][Mtot] -> the slice elements [slice][M][sw]"""
    return t_mc[:, c.sl].reshape(c.M, c.nsl, c.sw).permute(1, 0, 2)


def gcf_rows(c, t):
    """[slice][M][sw] -> [M][nslices sw]"""
    return t.permute(1, 0, 2).reshape(c.M, c.nsl * c.sw)


def gcf_inputs(c, training, device="cpu"):
    """what the kernel reads: rows ldy / ld_ms apart and slices ms_stride apart, all padding NaN; noise NCHW"""
    def ms(t):
        out = torch.full((c.nsl * c.ms_stride,), float("nan"))
        for j in range(c.nsl):
            out[j * c.ms_stride:j * c.ms_stride + c.M * c.ld_ms].view(c.M, c.ld_ms)[:, :c.sw] = t[j]
        return out.to(device)

    return NS(y=gk.pad(c.y, c.ldy).to(device), mu=ms(c.mu), sigma=ms(c.sigma),
              noise=to_nchw(c.noise, c.n, c.HW).contiguous().to(device) if training else None)


def gcf_outputs(c, yt, code, device="cpu", yhat32=True):
    """guarded outputs holding the initial contents; yhat32 is three columns wider so that no two leading dimensions
    agree (asserted)"""
    o = NS(lik=Guarded(1, c.M * c.Mtot, F32, device=device, init=to_nchw(c.lik0, c.n, c.HW).reshape(1, -1)),
           yhat=Guarded(c.M, c.Mtot, yt, device=device, init=c.yh0),
           yhat32=Guarded(c.M, c.Mtot + 3, F32, device=device, init=c.yh32_0) if yhat32 else None)
    if code:
        total = c.nsl * c.M * c.sw
        o.sym, o.idx = GuardedInt(1, total, device=device), GuardedInt(1, total, device=device)
    lds = [c.ldy, c.ld_ms, c.Mtot, o.yhat.ld] + ([o.yhat32.ld] if yhat32 else [])
    assert len(set(lds)) == len(lds), lds
    return o


def gcf_reference(c, training, yt, code=False):
    """{lik, yhat, yhat32: (ref, bound) over the WHOLE buffers (untouched elements keep their initial contents, bound
    0), sym, idx: exact}, and the E parts"""
    ys, nz = gcf_slices(c, c.y), gcf_slices(c, c.noise) if training else None
    r = gc_raw(ys, c.sigma, c.mu, nz)
    lik, bound = clamp_lik(r.raw)
    assert float((lik - gc_oracle64(ys, c.sigma, c.mu, nz)).abs().max()) <= 1e-13
    lik_ref, lik_b = c.lik0.double().clone(), torch.zeros(c.M, c.Mtot, dtype=F64)
    lik_ref[:, c.sl], lik_b[:, c.sl] = gcf_rows(c, lik), gcf_rows(c, bound)
    qi = rint32(ys, c.mu)
    q = gcf_rows(c, qi + c.mu)  # f32: rounded once
    yh_ref, yh_b = c.yh0.to(yt).double().clone(), torch.zeros(c.M, c.Mtot, dtype=F64)
    yh_ref[:, c.sl] = q.double()
    if yt == BF16:
        yh_b[:, c.sl] = BF16_ROUND * q.double().abs()
    y32_ref = c.yh32_0.double().clone()
    y32_ref[:, c.sl] = q.double()
    out = {"lik": (to_nchw(lik_ref, c.n, c.HW).reshape(1, -1), to_nchw(lik_b, c.n, c.HW).reshape(1, -1)),
           "yhat": (yh_ref, yh_b), "yhat32": (y32_ref, torch.zeros_like(y32_ref))}
    if code:
        out["sym"] = coder_order(qi.long(), c.n, c.HW)
        out["idx"] = coder_order(build_indexes32(c.sigma, c.table), c.n, c.HW)
    return out, NS(raw=r.raw, q=q, qi=qi, skipped=0)


GCF_MUTANTS = ("cancelling", "yoff", "ld_swap", "nchw_transposed", "half_away", "lt", "unbounded_sigma", "order_swap",
               "no_clamp")


def gcf_emulate(c, inp, o, code, mutant=None):
    """gc_slices_kernel restated on the CPU: the kernel's index arithmetic on the flat buffers, its formula in torch
    f32.  `mutant` applies one fault of GCF_MUTANTS"""
    n, HW, sw, nsl, Mtot = c.n, c.HW, c.sw, c.nsl, c.Mtot
    yoff = c.yoff + (1 if mutant == "yoff" else 0)
    i = torch.arange(n * HW * nsl * sw)
    m, r = i // (nsl * sw), i % (nsl * sw)
    j, cc = r // sw, r % sw
    ch = yoff + j * sw + cc
    b, pix = m // HW, m % HW
    yv = inp.y.reshape(-1)[m * c.ldy + ch]
    mv = inp.mu[j * c.ms_stride + m * c.ld_ms + cc]
    sv = inp.sigma[j * c.ms_stride + m * c.ld_ms + cc]
    nchw = (b * Mtot + ch) * HW + pix if mutant != "nchw_transposed" else (b * HW + pix) * Mtot + ch
    d = yv - mv
    qi = torch.round(d) if mutant != "half_away" else torch.sign(d) * torch.floor(d.abs() + 0.5)
    q = qi + mv
    xt = yv + inp.noise[nchw] if inp.noise is not None else q
    s = torch.maximum(sv, torch.tensor(0.11, dtype=F32))
    val = (xt - mv).abs()
    k = torch.tensor(K_ERFC, dtype=F32)
    if mutant == "cancelling":  # Phi((v + .5) / s) - Phi((v - .5) / s), arguments positive: the difference cancels
        raw = 0.5 * torch.erfc(k * ((val + 0.5) / s)) - 0.5 * torch.erfc(k * ((val - 0.5) / s))
    else:
        raw = 0.5 * torch.erfc(k * ((0.5 - val) / s)) - 0.5 * torch.erfc(k * ((-0.5 - val) / s))
    lik = raw if mutant == "no_clamp" else torch.maximum(raw, torch.tensor(1e-9, dtype=F32))
    buf, off = flat(o.lik)
    buf[off + nchw] = lik
    ld_yhat, ld32 = o.yhat.ld, o.yhat32.ld if o.yhat32 is not None else 0
    if mutant == "ld_swap":
        ld_yhat, ld32 = ld32, ld_yhat
    buf, off = flat(o.yhat)
    buf[off + m * ld_yhat + ch] = q.to(buf.dtype)
    if o.yhat32 is not None:
        buf, off = flat(o.yhat32)
        buf[off + m * ld32 + ch] = q
    if code:
        pos = j * n * sw * HW + (b * sw + cc) * HW + pix
        if mutant == "order_swap":
            pos = (b * nsl + j) * sw * HW + cc * HW + pix
        t = c.table.float()
        sx = sv if mutant == "unbounded_sigma" else s
        cmp = sx.unsqueeze(-1) < t[:-1] if mutant == "lt" else sx.unsqueeze(-1) <= t[:-1]
        buf, off = flat(o.sym)
        buf[off + pos] = qi.to(I32)
        buf, off = flat(o.idx)
        buf[off + pos] = ((t.numel() - 1) - cmp.sum(-1)).to(I32)
    return NS(lik=lik, nchw=nchw)


def gcf_check(tag, o, out, log=True):
    """every output of one launch against its reference; returns the ratios"""
    r = {"lik": gk.check(f"{tag}:lik", o.lik, *out["lik"], log=log),
         "yhat": gk.check(f"{tag}:yhat", o.yhat, *out["yhat"], log=log)}
    if o.yhat32 is not None:
        r["yhat32"] = gk.check(f"{tag}:yhat32", o.yhat32, *out["yhat32"], log=log)
    if "sym" in out:
        r["sym"] = check_exact(f"{tag}:symbols", o.sym, out["sym"], log=log)
        r["idx"] = check_exact(f"{tag}:indexes", o.idx, out["idx"], log=log)
    return r


def flat_case(table, total=528):
    """tmae_gc_likelihood_fwd: 528 elements, three workgroups, the last ragged"""
    return gc_elements(total, GCF_SEEDS["flat"], table)


def flat_reference(el, training, means, scale_bound=0.11):
    mu, nz = el.mu if means else None, el.noise if training else None
    r = gc_raw(el.y, el.sigma, mu, nz, scale_bound)
    lik, bound = clamp_lik(r.raw)
    assert float((lik - gc_oracle64(el.y, el.sigma, mu, nz, scale_bound)).abs().max()) <= 1e-13
    return (lik.reshape(1, -1), bound.reshape(1, -1)), r.xt32, r


# ------------------------------------------------------------------------------------ EntropyBottleneck cases
# seeds fixed on the CPU; (C, HW) with n = 2.  Measured on the reference, training | eval: clamped, elements below /
# above the median, lower + upper negative / positive (test_glue_checker.test_ebf_restatement_fits_and_census); no
# element's sign is within its error of zero:
#   (5, 3)   seed 41:   30 elements,   7, 12 / 18, 15 / 15     |   8, 5 / 6, 11 / 19
#   (5, 9)   seed 42:   90 elements,  30, 38 / 52, 49 / 41     |  36, 23 / 28, 37 / 53
#   (70, 3)  seed 43:  420 elements, 119, 216 / 204, 214 / 206 | 115, 111 / 111, 211 / 209
#   (70, 9)  seed 44: 1260 elements, 356, 609 / 651, 648 / 612 | 362, 344 / 333, 645 / 615
EBF_SEEDS = {(5, 3): 41, (5, 9): 42, (70, 3): 43, (70, 9): 44}
EBF_N = 2


def ebf_case(eb, HW, n=EBF_N):
    """glue_check.eb_case's placement (7 in 10 elements in the density's core, 3 in 10 at 1.2 .. 2.5 clamp thresholds,
    a few at +-60, one raw _matrix2 entry at 21) at this file's shapes"""
    sd = {gk.EB_PRE + k: v.detach().clone().float().cpu() for k, v in eb.state_dict().items()}
    sd[gk.EB_PRE + "_matrix2"][1, 2, 0] = 21.0
    C = sd[gk.EB_PRE + "_matrix0"].shape[0]
    g = gk._gen(EBF_SEEDS[(C, HW)])
    N = n * HW
    thr = gk.eb_thresholds(sd).float()
    noise = torch.rand(n, C, HW, generator=g) - 0.5
    side = (torch.rand(N, C, generator=g) < 0.5).long()
    t = torch.gather(thr.t(), 0, side)
    far = torch.rand(N, C, generator=g) < 0.3
    mag = gk.EB_FAR[0] + (gk.EB_FAR[1] - gk.EB_FAR[0]) * torch.rand(N, C, generator=g)
    core = torch.randn(N, C, generator=g) * thr.min(1).values.reshape(1, C) / 4
    x = torch.where(far, (side.float() * 2 - 1) * mag * t, core)
    z = x - noise.permute(0, 2, 1).reshape(N, C)
    for k in range(4):
        z[(7 * k + 2) % N, k % C] = 60.0 if k % 2 else -60.0
    return NS(n=n, HW=HW, C=C, N=N, sd=sd, z=z, noise=noise)


def ebf_reference(c, training, zt=F32, med_index=1):
    """{lik: (ref, bound) NCHW [1][n C HW], zhat: (ref, bound) NHWC [N][C] bitwise (bf16: its rounding), sym: exact
    NCHW}, and the parts"""
    z_cn = c.z.t().contiguous()  # [C][N]
    nz = gk._cn(c, c.noise) if training else None
    x, zhat, qi = eb_x(c.sd, z_cn, nz, med_index)
    r = eb_raw(c.sd, x)
    lik, bound = clamp_lik(r.raw)
    nchw = lambda t: t.reshape(c.C, c.n, c.HW).permute(1, 0, 2).reshape(1, -1)  # noqa: E731
    zh = zhat.t().double()
    zb = BF16_ROUND * zh.abs() if zt == BF16 else torch.zeros_like(zh)
    out = {"lik": (nchw(lik), nchw(bound)), "zhat": (zh, zb), "sym": nchw(qi.long()).reshape(-1)}
    return out, NS(raw=r.raw, x=x, r=r, zhat=zhat, skipped=0)


def ebf_census(c, p):
    med = c.sd[gk.EB_PRE + "quantiles"][:, 0, 1].double().reshape(-1, 1)
    return dict(clamped=int((p.raw.v < LIK_MIN).sum()), below_median=int((p.x.v < med).sum()),
                above_median=int((p.x.v > med).sum()), sum_negative=int((p.r.sum.v < 0).sum()),
                sum_positive=int((p.r.sum.v > 0).sum()), ambiguous=int(p.r.ambiguous.sum()))


def ebf_restate(c, training, med_index=1, clamp=True):
    """the oracle's f32 EntropyBottleneck on the case -> (lik NCHW flat, zhat NHWC [N][C]); med_index 0: the fault
    'median taken from quantile 0'"""
    sd = {k: v.clone() for k, v in c.sd.items()}
    if med_index != 1:
        sd[gk.EB_PRE + "quantiles"][:, 0, 1] = c.sd[gk.EB_PRE + "quantiles"][:, 0, med_index]
    z = c.z.reshape(c.n, c.HW, c.C).permute(0, 2, 1).reshape(c.n, c.C, c.HW, 1)
    lik, zhat = orc.entropy_bottleneck(sd, gk.EB_PRE, z, c.noise.reshape(c.n, c.C, c.HW, 1) if training else None)
    if not clamp:
        values = z.permute(1, 0, 2, 3).reshape(c.C, 1, -1)
        med = sd[gk.EB_PRE + "quantiles"][:, :, 1:2]
        x = values + gk._cn(c, c.noise).reshape(c.C, 1, -1) if training else torch.round(values - med) + med
        lo, up = orc.eb_logits(sd, gk.EB_PRE, x - 0.5), orc.eb_logits(sd, gk.EB_PRE, x + 0.5)
        sg = -torch.sign(lo + up)
        lik = (torch.sigmoid(sg * up) - torch.sigmoid(sg * lo)).abs().reshape(c.C, c.n, c.HW).permute(1, 0, 2)
    return lik.reshape(-1), zhat.reshape(c.n, c.C, c.HW).permute(0, 2, 1).reshape(c.N, c.C)


def narrow_quantiles(sd):
    """a copy of sd whose quantiles sit 1 .. 3 samples from the median, unevenly: the channels' pmf lengths differ, the
    tail masses are far above f32's underflow, and upstream's tail (the PADDED range's last sample) differs from the
    one at each channel's own last sample"""
    sd = {k: v.clone() for k, v in sd.items()}
    q = sd[gk.EB_PRE + "quantiles"]
    k = torch.arange(q.shape[0])
    q[:, 0, 0] = q[:, 0, 1] - (0.6 + (k % 3).float())
    q[:, 0, 2] = q[:, 0, 1] + (0.7 + ((k + 1) % 3).float())
    return sd


def pmf_tables(sd, table):
    """centres, starts and lengths as oracle/coding_oracle.py derives them"""
    _, _, center, gl = co.gc_pmf(table)
    _, _, start, el = co.eb_pmf(sd, gk.EB_PRE)
    return NS(center=center, gc_length=gl, start=start, eb_length=el)


# ------------------------------------------------------------------------------------ permutations
def perm_case(n=3, L=100, seed=51):
    g = gk._gen(seed)
    return torch.stack([torch.randperm(L, generator=g) for _ in range(n)])


def invert_reference(p, init=SENTINEL):
    """inverse[b][p[b][j]] = j for p in [0, L); slots no entry names keep `init`"""
    n, L = p.shape
    inv = torch.full((n, L), init, dtype=I64)
    for b in range(n):
        for j in range(L):
            v = int(p[b, j])
            if 0 <= v < L:
                inv[b, v] = j
    return inv
