"""Cases and references of the forward and backward at a per-image quantiser step: the kernels
tmae_gc_slices_fwd_q and tmae_gc_bwd_q, tmae_lic_stack's chain with cq, and the model's training forward with q.  The
sibling of qstep_check.py (the coder's kernels, §3.17), whose restatement and cases it extends, of entropy_check.py
(layouts, the likelihood's E bound) and of glue_check.py (gc_bwd's reference, skip mask and cap).
tests/test_qtrain_host.py checks this file on the CPU; tests/test_gpu_qtrain_kernels.py and test_gpu_qtrain_model.py
check the kernels and the model against it.

Per element, in f32, with delta = qstep(q[image]) (every line one rounded operation, as the kernels compute it):

    t     = fl(fl(y - mu) / delta)               qi = rint(t)
    y_hat = fl(fl(qi delta) + mu)                 qstep_check.restate: bit for bit
    s     = max(fl(sigma / delta), bound)
    v     = |fl(t + noise)| in training, |qi| in eval
    lik   = max(Phi((1/2 - v) / s) - Phi((-1/2 - v) / s), 1e-9)

Forward.  y_hat is compared bit for bit.  The eval likelihood is compared bit for bit with tmae_gc_slices_code_q's on
the GPU.  The training likelihood gets (ref, bound): ref in float64 from the f32 inputs, bound from the formula above in
glue_check's E arithmetic; it is entropy_check.gc_raw's derivation with t = (y - mu) / delta and sigma / delta in place
of y - mu and sigma, i.e. one more correctly rounded division on either argument.  No element is skipped (both clamps are
continuous: entropy_check's first bullet; the scale clamp takes the larger of the two sides' errors).

Backward (gradient table of DESIGN.md §3.18).  The reference is float64 torch.autograd through oracle.train_oracle's
lower_bound of the formula above with y_hat straight-through (d/dy = 1, d/dmu = 0); the bound carries gcq_bwd_kernel's
formula through E with the branches decided by the reference.  In eval the rounded value comes from the f32 evaluation
of t (torch's f32 arithmetic on the CPU is the kernel's, operation for operation), so no tie needs a mask.  Skipped, from
the reference alone, as glue_check.gc_skip does: unclamped likelihood in [1e-10, 1e-8], |sigma / delta - bound| < 1e-3,
0 < |t + noise| < 1e-4 in training; at most glue_check.SKIP_CAP of a case.
"""
import functools
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

import entropy_check as ek
import glue_check as gk
import qstep_check as qk
from glue_check import BF16, F32, F64, E, U  # noqa: F401
from oracle import train_oracle as orc

F = np.float32
BOUND = 0.11
Q3 = qk.Q3
_TABLE2 = np.array([1.0, 2.0], dtype=F)  # restate() wants a scale table; its indexes are not used here


def deltas(q):
    return [qk.qstep(v) for v in q]


# ------------------------------------------------------------------------------------ the restatement, forward
def restate_fwd(y, mu, sigma, noise, delta, bound=BOUND):
    """numpy f32 arrays of one shape (delta broadcastable; noise None: eval) -> NS(t, qi, yhat, sdiv, s, v), every
    line one f32 operation: qstep_check.restate plus the likelihood's argument"""
    r = qk.restate(y, mu, sigma, delta, _TABLE2, bound)
    v = np.abs(r.qi) if noise is None else np.abs(r.t + np.asarray(noise, dtype=F))
    assert v.dtype == F
    return NS(t=r.t, qi=r.qi, yhat=r.yhat, sdiv=r.sdiv, s=r.s, v=v)


def lik32(v, s):
    """the likelihood of the restatement's v and s in f32 (libm's erfc, so not bit for bit the kernel's)"""
    v, s = torch.from_numpy(np.asarray(v, dtype=F)), torch.from_numpy(np.asarray(s, dtype=F))
    k = torch.tensor(ek.K_ERFC, dtype=F32)
    raw = 0.5 * torch.erfc(k * ((0.5 - v) / s)) - 0.5 * torch.erfc(k * ((-0.5 - v) / s))
    return torch.maximum(raw, torch.tensor(1e-9, dtype=F32))


def _scale_E(sigma, delta, bound):
    """s = max(sigma / delta, bound f32) in E: the clamp is continuous, so the error is the larger side's"""
    sr = E(sigma) / E(delta)
    return E(sr.v.clamp_min(bound), torch.maximum(sr.e, torch.full_like(sr.e, U * bound))), sr


def _raw_E(v, s):
    k = E.const(ek.K_ERFC)
    up = (k * ((0.5 - v) / s)).mono(torch.erfc).exact(0.5)
    lo = (k * ((-0.5 - v) / s)).mono(torch.erfc).exact(0.5)
    return up - lo


def lik_train_reference(y, mu, sigma, noise, delta, bound=BOUND):
    """(ref float64, bound) of the training likelihood from f32 tensors of one shape: entropy_check.gc_raw's
    derivation with the two divisions by delta"""
    y, mu, sigma, noise, delta = (torch.as_tensor(np.asarray(a, dtype=F)) for a in (y, mu, sigma, noise, delta))
    t = (E(y) - E(mu)) / E(delta.expand_as(y))
    s, _ = _scale_E(sigma, delta.expand_as(y), bound)
    return ek.clamp_lik(_raw_E((t + E(noise)).abs(), s))


def lik64(y, mu, sigma, noise, delta, bound=BOUND):
    """the definition in plain float64 (no E): what lik_train_reference's ref must equal"""
    y, mu, sigma, noise, delta = (torch.as_tensor(np.asarray(a, dtype=F)).double() for a in (y, mu, sigma, noise, delta))
    v = ((y - mu) / delta + noise).abs()
    s = (sigma / delta).clamp_min(bound)
    k = -(2 ** -0.5)
    return (0.5 * torch.erfc(k * ((0.5 - v) / s)) - 0.5 * torch.erfc(k * ((-0.5 - v) / s))).clamp_min(1e-9)


# ------------------------------------------------------------------------------------ slice cases, forward
def build_case(name, HW, sw, nsl, q, seed):
    """qstep_check.case's construction for any (HW, sw, nslices) and len(q) images, with training noise [M][Mtot]"""
    n = len(q)
    M = n * HW
    table = ek.model_table()
    Mtot = qk.YOFF + nsl * sw + 4
    per = nsl * HW * sw
    mu, sigma, ysl, delta = (np.empty((nsl, M, sw), dtype=F) for _ in range(4))
    for b in range(n):
        el, _ = qk.elements(per, seed + 100 * b, table, qk.qstep(q[b]))
        rows = slice(b * HW, (b + 1) * HW)
        for a, src in ((mu, el.mu), (sigma, el.sigma), (ysl, el.y)):
            a[:, rows, :] = src.reshape(nsl, HW, sw)
        delta[:, rows, :] = qk.qstep(q[b])
    g = gk._gen(seed + 1000)
    y = 3 * torch.randn(M, Mtot, generator=g)
    sl = slice(qk.YOFF, qk.YOFF + nsl * sw)
    y[:, sl] = torch.from_numpy(ysl).permute(1, 0, 2).reshape(M, nsl * sw)
    c = NS(shape=name, n=n, HW=HW, sw=sw, nsl=nsl, yoff=qk.YOFF, Mtot=Mtot, M=M, sl=sl, y=y, table=table,
           mu=torch.from_numpy(mu), sigma=torch.from_numpy(sigma), delta=delta, q=tuple(q),
           lik0=2 + torch.rand(M, Mtot, generator=g), yh0=torch.randn(M, Mtot, generator=g),
           yh32_0=torch.randn(M, Mtot + 3, generator=g), ldy=Mtot + 8, ld_ms=sw + 3)
    c.noise = torch.rand(M, Mtot, generator=g) - 0.5
    c.ms_stride = M * c.ld_ms + 5
    return c


@functools.lru_cache(None)
def fwd_case(shape):
    """qstep_check.case(shape) (three images at q = Q3, the coder tests' elements) with training noise added"""
    c = NS(**vars(qk.case(shape)))
    c.noise = torch.rand(c.M, c.Mtot, generator=gk._gen(qk.SEEDS[shape] + 2000)) - 0.5
    return c


@functools.lru_cache(None)
def fwd_reference(shape):
    """training outputs of fwd_case(shape): {"lik": (ref, bound) over the whole NCHW buffer, "yhat32": f32 values over
    the whole buffer (the restatement's, bit for bit), "yhat": the same before the cast}, and the restatement"""
    c = fwd_case(shape)
    ys, nz = ek.gcf_slices(c, c.y).contiguous().numpy(), ek.gcf_slices(c, c.noise).contiguous().numpy()
    r = restate_fwd(ys, c.mu.numpy(), c.sigma.numpy(), nz, c.delta)
    lik, lb = lik_train_reference(ys, c.mu.numpy(), c.sigma.numpy(), nz, c.delta)
    lik_ref, lik_b = c.lik0.double().clone(), torch.zeros(c.M, c.Mtot, dtype=F64)
    lik_ref[:, c.sl], lik_b[:, c.sl] = ek.gcf_rows(c, lik), ek.gcf_rows(c, lb)
    q32 = ek.gcf_rows(c, torch.from_numpy(r.yhat))
    yh, y32 = c.yh0.clone(), c.yh32_0.clone()
    yh[:, c.sl] = q32
    y32[:, c.sl] = q32
    out = {"lik": (ek.to_nchw(lik_ref, c.n, c.HW).reshape(1, -1), ek.to_nchw(lik_b, c.n, c.HW).reshape(1, -1)),
           "yhat": yh, "yhat32": y32}
    return out, r


# the tiled form against the element form on the same values: three images of 96 pixels (96 x 17 = 1632 floats, the
# LDS tile) and the same 288 rows as ONE image (288 x 17 = 4896 > 4800, one element per thread); one q, so that the
# single image's step is every row's
TILE_Q, TILE_HW, TILE_SW, TILE_NSL = 11, 96, 16, 2


@functools.lru_cache(None)
def tile_cases():
    a = build_case("tile96", TILE_HW, TILE_SW, TILE_NSL, (TILE_Q,) * 3, 71)
    b = NS(**vars(a))
    b.n, b.HW, b.q = 1, 3 * TILE_HW, (TILE_Q,)
    assert a.HW * (a.sw + 1) <= 4800 < b.HW * (b.sw + 1)
    return a, b


# ------------------------------------------------------------------------------------ GaussianConditional backward
GCQ_SHAPES = {"small": dict(HW=9, sw=5, Mtot=16, yoff=7),       # 135 elements: part of one workgroup
              "three_wg": dict(HW=16, sw=11, Mtot=40, yoff=24)}  # 528: three workgroups, the last one ragged
GCQ_SEEDS = {"small": 23, "three_wg": 27}
N_IMAGES = 3
PLANT = (0.9, 0.98, 1.02, 1.1)  # sigma = these multiples of bound x delta, per image: both sides of the scale gate


@functools.lru_cache(None)
def gcq_case(shape, q=Q3):
    """glue_check.gc_case's recipe in units of each image's step: y ~ 3 N(0,1) delta, mu ~ N(0,1) delta, sigma / delta
    a third in [0.02, 0.09] and the rest in [0.13, 2.63], uniform noise, Gaussian glik / gyp / dy0; per image, sigma
    planted at PLANT x bound x delta"""
    d = GCQ_SHAPES[shape]
    n, HW, sw, Mtot, yoff = N_IMAGES, d["HW"], d["sw"], d["Mtot"], d["yoff"]
    g = gk._gen(GCQ_SEEDS[shape])
    M = n * HW
    dl = torch.tensor([float(v) for v in deltas(q)], dtype=F32).repeat_interleave(HW).reshape(M, 1)
    y = 3 * torch.randn(M, Mtot, generator=g) * dl
    mu = torch.randn(M, sw, generator=g) * dl
    small = torch.rand(M, sw, generator=g) < 1 / 3
    sigma = torch.where(small, 0.02 + 0.07 * torch.rand(M, sw, generator=g), 0.13 + 2.5 * torch.rand(M, sw, generator=g))
    sigma = sigma * dl
    noise = torch.rand(n, Mtot, HW, generator=g) - 0.5
    glik = torch.randn(n, Mtot, HW, generator=g)
    gyp = torch.randn(M, Mtot, generator=g)
    dy0 = torch.randn(M, Mtot, generator=g)
    for b in range(n):
        for k, mult in enumerate(PLANT):
            m, c = b * HW + (2 * k + 1) % HW, (3 * k + b) % sw
            sigma[m, c] = torch.tensor(BOUND * mult, dtype=F32) * dl[m, 0]
    return NS(shape=shape, n=n, HW=HW, sw=sw, Mtot=Mtot, yoff=yoff, M=M, y=y, mu=mu, sigma=sigma, noise=noise,
              glik=glik, gyp=gyp, dy0=dy0, ldy=Mtot + 8, ld_ms=sw + 3, ldg=Mtot + 3, q=tuple(q), delta=dl)


def _t32(c):
    """(y - mu) / delta as the kernel evaluates it: two f32 operations"""
    sl = slice(c.yoff, c.yoff + c.sw)
    return (c.y[:, sl] - c.mu) / c.delta


def gcq_autograd(c, training, use_glik=True, use_gyp=True, dtype=F64, bound=BOUND):
    """(dy slice, dmu, dsigma) by torch.autograd through oracle.train_oracle.lower_bound in `dtype`, and the
    reference's intermediates"""
    sl = slice(c.yoff, c.yoff + c.sw)
    y = c.y[:, sl].to(dtype).requires_grad_(True)
    mu = c.mu.to(dtype).requires_grad_(True)
    sg = c.sigma.to(dtype).requires_grad_(True)
    dl = c.delta.to(dtype)
    glik = gk._mc(c, c.glik).to(dtype) if use_glik else torch.zeros(c.M, c.sw, dtype=dtype)
    gyp = c.gyp[:, sl].to(dtype) if use_gyp else torch.zeros(c.M, c.sw, dtype=dtype)
    t = (y - mu) / dl
    qi = torch.round(_t32(c)).to(dtype)  # rint of the f32 evaluation: a constant of the graph
    dd = t + gk._mc(c, c.noise).to(dtype) if training else qi
    sr = sg / dl
    s = orc.lower_bound(sr, bound)
    v = dd.abs()
    k = -(2 ** -0.5)
    raw = 0.5 * torch.erfc(k * ((0.5 - v) / s)) - 0.5 * torch.erfc(k * ((-0.5 - v) / s))
    lik = orc.lower_bound(raw, 1e-9)
    yhp = (qi * dl + mu).detach() + (y - y.detach())  # straight-through: d/dy = 1, d/dmu = 0
    ((glik * lik).sum() + (gyp * yhp).sum()).backward()
    zero = torch.zeros(c.M, c.sw, dtype=dtype)
    return NS(dy=y.grad if y.grad is not None else zero, dmu=mu.grad if mu.grad is not None else zero,
              dsigma=sg.grad if sg.grad is not None else zero, raw=raw.detach(), dd=dd.detach(), sr=sr.detach(),
              glik=glik, training=training)


def gcq_skip(c, a, bound=BOUND):
    band = (a.raw >= 1e-10) & (a.raw <= 1e-8)
    sig = (a.sr - bound).abs() < 1e-3
    near0 = (a.dd.abs() > 0) & (a.dd.abs() < 1e-4) if a.training else torch.zeros_like(band)
    return NS(band=band, sig=sig, near0=near0, any=band | sig | near0)


def gcq_formula(c, a, out_dtype, use_gyp=True, bound=BOUND):
    """gcq_bwd_kernel's formula in E arithmetic, its branches decided by the reference `a`"""
    sl = slice(c.yoff, c.yoff + c.sw)
    dl = E(c.delta.expand(c.M, c.sw))
    if a.training:
        dd = (E(c.y[:, sl]) - E(c.mu)) / dl + E(gk._mc(c, c.noise))
    else:
        dd = E(torch.round(_t32(c)))
    sr = E(c.sigma) / dl
    s = sr.where(sr.v >= bound, E.const(bound))
    v = dd.abs()
    aa, bb = (0.5 - v) / s, (-0.5 - v) / s
    g = E(a.glik).exact(((a.raw >= 1e-9) | (a.glik < 0)).double())
    c0 = E.const(1.0 / math.sqrt(2.0 * math.pi))
    pa = c0 * (aa * aa).exact(-0.5).mono(torch.exp)
    pb = c0 * (bb * bb).exact(-0.5).mono(torch.exp)
    sd = s * dl
    dv = g * (pb - pa) / sd
    ds_pre = g * (bb * pb - aa * pa) / sd
    ds = ds_pre.exact(((sr.v >= bound) | (ds_pre.v < 0)).double())
    gyp = E(c.gyp[:, sl]) if use_gyp else E(torch.zeros(c.M, c.sw))
    if a.training:
        ddd = dv.exact(torch.sign(a.dd))
        dyv, dmv = gyp + ddd, -ddd
    else:
        ddd = E(torch.zeros(c.M, c.sw))
        dyv, dmv = gyp, ddd
    return NS(dy=dyv.acc(c.dy0[:, sl]), dmu=dmv.store(out_dtype), dsigma=ds.store(out_dtype), ds_pre=ds_pre, ddd=ddd)


def gcq_bwd_reference(c, training, out_dtype, use_glik=True, use_gyp=True):
    """{dy [M][Mtot] (the slice accumulated into dy0, the other columns untouched), dmu, dsigma: (ref, bound, skip)},
    the skip mask's parts, the reference and the formula: glue_check.gc_bwd_reference's shape"""
    a = gcq_autograd(c, training, use_glik, use_gyp)
    f = gcq_formula(c, a, out_dtype, use_gyp)
    sl = slice(c.yoff, c.yoff + c.sw)
    dy_ref, dy_bound = c.dy0.double().clone(), torch.zeros(c.M, c.Mtot, dtype=F64)
    dy_ref[:, sl] += a.dy
    dy_bound[:, sl] = f.dy.e
    skip = gcq_skip(c, a)
    dy_skip = torch.zeros(c.M, c.Mtot, dtype=torch.bool)
    dy_skip[:, sl] = skip.any
    out = {"dy": (dy_ref, dy_bound, dy_skip), "dmu": (a.dmu, f.dmu.e, skip.any), "dsigma": (a.dsigma, f.dsigma.e, skip.any)}
    return out, skip, a, f


def gcq_census(c, a, f, bound=BOUND):
    """branch classes of gcq_bwd_kernel counted on the reference, per image (every image has its own step)"""
    clamped = a.raw < 1e-9
    small = a.sr < bound
    ds = f.ds_pre.v
    out = []
    for b in range(c.n):
        r = slice(b * c.HW, (b + 1) * c.HW)
        out.append(dict(lik_blocked=int((clamped & (a.glik >= 0))[r].sum()), lik_passes=int((clamped & (a.glik < 0))[r].sum()),
                        lik_open=int((~clamped)[r].sum()), sigma_open=int((~small)[r].sum()),
                        sigma_passes=int((small & (ds < 0))[r].sum()), sigma_blocked=int((small & (ds > 0))[r].sum()),
                        positive=int((a.dd > 0)[r].sum()), negative=int((a.dd < 0)[r].sum())))
    return out


GCQ_MUTANTS = ("gate_on_sigma", "no_delta_in_dsigma", "eval_moves_mu", "ste_to_mu", "sign_dropped")


def gcq_bwd_emulate(c, training, out_dtype, use_glik=True, use_gyp=True, mutant=None, bound=BOUND):
    """gcq_bwd_kernel restated in torch f32 on the CPU -> (dy [M][Mtot], dmu, dsigma) as the kernel would leave them;
    `mutant` applies one fault of GCQ_MUTANTS"""
    sl = slice(c.yoff, c.yoff + c.sw)
    f32 = lambda x: torch.tensor(x, dtype=F32)  # noqa: E731
    t = _t32(c)
    sr = c.sigma / c.delta
    s = torch.maximum(sr, f32(bound))
    dd = t + gk._mc(c, c.noise) if training else torch.round(t)
    v = dd.abs()
    a, bb = (0.5 - v) / s, (-0.5 - v) / s
    k = f32(ek.K_ERFC)
    lik = 0.5 * torch.erfc(k * a) - 0.5 * torch.erfc(k * bb)
    g = gk._mc(c, c.glik).clone() if use_glik else torch.zeros(c.M, c.sw)
    g = torch.where((lik >= f32(1e-9)) | (g < 0), g, torch.zeros_like(g))
    c0 = f32(1.0 / math.sqrt(2.0 * math.pi))
    pa, pb = c0 * torch.exp(-0.5 * a * a), c0 * torch.exp(-0.5 * bb * bb)
    sd = s if mutant == "no_delta_in_dsigma" else s * c.delta
    dv = g * (pb - pa) / (s * c.delta)
    ds = g * (bb * pb - a * pa) / sd
    gate = (c.sigma >= f32(bound)) if mutant == "gate_on_sigma" else (sr >= f32(bound))
    ds = torch.where(gate | (ds < 0), ds, torch.zeros_like(ds))
    sg = torch.ones_like(dd) if mutant == "sign_dropped" else torch.sign(dd)
    ddd = dv * sg if (training or mutant == "eval_moves_mu") else torch.zeros_like(dv)
    gyp = c.gyp[:, sl] if use_gyp else torch.zeros(c.M, c.sw)
    dy = c.dy0.clone()
    dy[:, sl] += gyp + (ddd if training else 0)
    dmu = -ddd + (gyp if mutant == "ste_to_mu" else 0)
    return dy, dmu.to(out_dtype), ds.to(out_dtype)


# ------------------------------------------------------------------------------------ the model's training forward
def mcm_forward_q(sd, cfg, imgs, scores, z_noise, y_noise, q, bound=BOUND, lanes=8):
    """oracle.train_oracle.mcm_forward_train with the quantiser step of §3.18 per image in the slice loop, composed
    from its parts (the way qstep_check.oracle_coded is composed from mcm_oracle's) -> (x_hat, y_likelihood,
    z_likelihood, t: every (y - mu) / delta the loop rounded, sym: the rounded values, gate: sigma / delta >= bound);
    in the dtype of sd / imgs, differentiable"""
    import torch.nn.functional as Fn

    from oracle import ids as ids_oracle
    from oracle import mcm_oracle as O

    p, K, D = cfg.patch_size, cfg.num_keep_patches, cfg.encoder_embed_dim
    n = imgs.shape[0]
    shuf, rest = ids_oracle.ids_shuffle(scores.float().cpu().numpy(), K, lanes)
    shuf, rest = torch.from_numpy(shuf), torch.from_numpy(rest)
    x = Fn.conv2d(imgs, sd["encoder_embed.proj.weight"], sd["encoder_embed.proj.bias"], stride=p)
    x = x.flatten(2).transpose(1, 2)
    pos = sd["encoder_pos_embed"]
    x = x + pos[:, 1:, :]
    x = torch.gather(x, 1, shuf[:, :K].unsqueeze(-1).repeat(1, 1, D))
    cls = (sd["cls_token"] + pos[:, :1, :]).expand(n, -1, -1)
    x = torch.cat((cls, x), dim=1)
    for i in range(cfg.encoder_depth):
        x = O.block(x, sd, f"encoder_blocks.{i}.", cfg.encoder_num_heads, cfg.norm_eps)
    x = O.layer_norm(x, sd, "encoder_norm.", cfg.norm_eps)[:, 1:, :]
    g = int(K ** 0.5)
    y = x.reshape(-1, g, g, D).permute(0, 3, 1, 2).contiguous()
    y = O.seq_convs(y, sd, "g_a.", O.G_A)
    z = O.seq_convs(y, sd, "h_a.", O.H_A)
    z_lik, z_hat = orc.eb_train(sd, "entropy_bottleneck.", z, z_noise)
    ls = O.seq_convs(z_hat, sd, "h_s_scale.", O.H_S)
    lm = O.seq_convs(z_hat, sd, "h_s_mean.", O.H_S)
    S = cfg.num_slices
    hh, ww = y.shape[2:]
    yn = y_noise.to(y.dtype).chunk(S, 1)
    delta = torch.tensor([float(v) for v in deltas(q)], dtype=y.dtype).reshape(n, 1, 1, 1)
    kc = float(-(2 ** -0.5))
    yhat, liks, ts, syms, gates = [], [], [], [], []
    for i, ys in enumerate(y.chunk(S, 1)):
        sup = yhat[:S // 2]
        mean_support = torch.cat([lm] + sup, dim=1)
        mu = O.seq_convs(mean_support, sd, f"cc_transform_mean.{i}.", O.CC)[:, :, :hh, :ww]
        sigma = O.seq_convs(torch.cat([ls] + sup, dim=1), sd, f"cc_transform_scale.{i}.", O.CC)[:, :, :hh, :ww]
        t = (ys - mu) / delta
        qi = torch.round(t).detach()
        sr = sigma / delta
        s = orc.lower_bound(sr, bound)
        v = torch.abs(t + yn[i])
        raw = 0.5 * torch.erfc(kc * ((0.5 - v) / s)) - 0.5 * torch.erfc(kc * ((-0.5 - v) / s))
        liks.append(orc.lower_bound(raw, 1e-9))
        yh = (qi * delta + mu).detach() + (ys - ys.detach())  # y_hat_pre straight-through: d/dy = 1, d/dmu = 0
        lrp = O.seq_convs(torch.cat([mean_support, yh], dim=1), sd, f"lrp_transform.{i}.", O.CC)
        yhat.append(yh + 0.5 * torch.tanh(lrp))
        ts.append(t.detach().reshape(-1))
        syms.append(qi.reshape(-1))
        gates.append((sr.detach() >= bound).reshape(-1))
    tk = O.seq_convs(torch.cat(yhat, dim=1), sd, "g_s.", O.G_S).permute(0, 2, 3, 1).contiguous().view(-1, K, D)
    xd = O.linear(tk, sd, "decoder_embed.")
    L = rest.shape[1]
    mask = sd["mask_token"].repeat(n, L + 1 - xd.shape[1], 1)
    x_ = torch.gather(torch.cat([xd[:, 1:, :], mask], dim=1), 1, rest.unsqueeze(-1).repeat(1, 1, xd.shape[2]))
    x = torch.cat([xd[:, :1, :], x_], dim=1) + sd["decoder_pos_embed"]
    for i in range(cfg.decoder_depth):
        x = O.block(x, sd, f"decoder_blocks.{i}.", cfg.decoder_num_heads, cfg.norm_eps)
    x = O.layer_norm(x, sd, "decoder_norm.", cfg.norm_eps)
    x_hat = O.unpatchify(O.linear(x, sd, "decoder_pred.")[:, 1:, :], p, cfg.in_chans)
    return NS(x_hat=x_hat, y_lik=torch.cat(liks, dim=1), z_lik=z_lik, t=torch.cat(ts), sym=torch.cat(syms),
              gate=torch.cat(gates))
