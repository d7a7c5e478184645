"""Cases and references of the per-image quantiser step kernels (tmae_gc_slices_code_q / tmae_gc_indexes_q /
tmae_gc_dequantize_q): the sibling of entropy_check.py, whose layouts (gcf_inputs / gcf_outputs), E
arithmetic (gc_raw, clamp_lik) and Guarded buffers it uses.  tests/test_qstep_host.py checks this file on the CPU,
tests/test_gpu_qstep_kernels.py the kernels against it.

The reference is a numpy f32 RESTATEMENT: the kernels round every operation to f32 on its own, numpy's float32
arithmetic does the same, so symbols, indexes and both y_hat outputs are compared bit for bit and no element is skipped:

    delta = ldexp(F[q mod 8], floor(q / 8))          bitstream.qstep, the mirror of tmae_qstep
    t = fl(fl(y - mu) / delta); qi = rint(t)         round half to even
    y_hat = fl(fl(qi delta) + mu)
    s = max(fl(sigma / delta), bound as f32); index = (nscale - 1) - #{t < nscale - 1 : s <= table[t]}

The likelihood max(Phi((0.5 - |qi|) / s) - Phi((-0.5 - |qi|) / s), 1e-9) takes entropy_check.gc_raw's form without
means at x = qi and sigma = fl(sigma / delta), both exact f32 inputs from the restatement: the same float64 reference,
the same E bound and the same clamp rule as for the existing kernel.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np
import torch

import entropy_check as ek
import glue_check as gk
from glue_check import F64

YOFF = 3
TIES = (0.5, -0.5, 1.5, -1.5, 2.5)
Q3 = (-32, 0, 11)  # a power of two, one, and a step that is no power of two
F = np.float32


def qstep(q):
    from textmae_amd import bitstream

    return bitstream.qstep(int(q))


# ------------------------------------------------------------------------------------ the restatement
def restate(y, mu, sigma, delta, table, bound=0.11):
    """numpy f32 arrays of one shape (delta broadcastable) -> NS(qi f32, sym int64, yhat f32, s f32 bounded, sdiv f32
    unbounded, idx int64); every line one f32 operation"""
    y, mu, sigma, delta = (np.asarray(a, dtype=F) for a in (y, mu, sigma, delta))
    d = y - mu
    t = d / delta
    qi = np.rint(t)
    p = qi * delta
    yhat = p + mu
    sdiv = sigma / delta
    s = np.maximum(sdiv, F(bound))
    tab = np.asarray(table, dtype=F)
    idx = (tab.size - 1) - (s[..., None] <= tab[:-1]).sum(-1)
    assert all(a.dtype == F for a in (d, t, qi, p, yhat, sdiv, s))
    return NS(qi=qi, sym=qi.astype(np.int64), yhat=yhat, s=s, sdiv=sdiv, idx=idx.astype(np.int64), t=t)


def restate64(y, mu, sigma, delta, table, bound=0.11):
    """the same in float64 from the f32 inputs (delta is the f32 step): what the restatement approximates"""
    y, mu, sigma, delta = (np.asarray(a, dtype=np.float64) for a in (y, mu, sigma, delta))
    t = (y - mu) / delta
    qi = np.rint(t)
    s = np.maximum(sigma / delta, float(F(bound)))
    tab = np.asarray(table, dtype=F).astype(np.float64)
    idx = (tab.size - 1) - (s[..., None] <= tab[:-1]).sum(-1)
    return NS(t=t, qi=qi, yhat=qi * delta + mu, s=s, idx=idx)


def dequantize(sym, mu, delta):
    """tmae_gc_dequantize_q restated: fl(fl((float)sym delta) + mu)"""
    p = np.asarray(sym).astype(F) * np.asarray(delta, dtype=F)
    return p + np.asarray(mu, dtype=F)


def likelihood_reference(r, bound=0.11):
    """(ref float64, bound) of the likelihood from the restatement's qi and fl(sigma / delta): entropy_check's method"""
    raw = ek.gc_raw(torch.from_numpy(r.qi), torch.from_numpy(r.sdiv), None, None, bound).raw
    return ek.clamp_lik(raw)


# ------------------------------------------------------------------------------------ planting
def _near(x, k=6):
    """x and its k neighbours either side, f32"""
    out, lo, hi = [F(x)], F(x), F(x)
    for _ in range(k):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return out


def solve_quotient(target, delta):
    """an f32 x with fl(x / delta) == target bit for bit, or None"""
    for x in _near(F(target) * F(delta)):
        if F(x) / F(delta) == F(target):
            return F(x)
    return None


def plant_tie(d, delta, k):
    """(y, mu) with fl(fl(y - mu) / delta) == d exactly and y - mu exact; k picks the mean"""
    x = solve_quotient(d, delta)
    if x is None:
        return None
    sgn = -1.0 if x > 0 else 1.0  # a mean of the other sign: y = x + mu is smaller than x, so it is exact
    for m in ((0.0, 0.25, 0.5, 1.0)[k], 0.0):
        mu = F(sgn * m) * F(delta)
        y = F(x + mu)
        if float(y) - float(mu) == float(x) and F(F(y - mu) / F(delta)) == F(d):
            return y, mu
    return None


def elements(N, seed, table, delta):
    """gc_elements' recipe in units of the step (y - mu ~ 3 delta N(0,1) with tails, sigma / delta a third below the
    bound and the rest in [0.13, 2.63]) and, at seeded places, the classes the kernels can get wrong: (y - mu) / delta
    exactly at 0.5, -0.5, 1.5, -1.5, 2.5; sigma / delta exactly on a table entry, one ulp either side of one, exactly
    0.11f, below the bound, past the table -> NS of f32 numpy arrays and the census of what was planted"""
    g = gk._gen(seed)
    r = lambda: torch.rand(N, generator=g)  # noqa: E731
    dl = float(delta)
    mu = torch.randn(N, generator=g) * dl
    y = mu + 3 * dl * torch.randn(N, generator=g)
    sig = torch.where(r() < 1 / 3, 0.02 + 0.07 * r(), 0.13 + 2.5 * r())
    side = torch.where(r() < 0.5, -1.0, 1.0)
    y = torch.where(r() < 0.15, mu + dl * side * sig.clamp_min(0.11) * (1 + 5.5 * r()), y)
    y, mu, sigma = y.numpy().astype(F), mu.numpy().astype(F), (sig * dl).numpy().astype(F)
    slots = iter(torch.randperm(N, generator=g).tolist())
    tab = np.asarray(table, dtype=F)
    planted = {}

    def put_sigma(name, targets):
        n = 0
        for tgt in targets:
            x = solve_quotient(tgt, delta)
            if x is not None and n < 4:
                sigma[next(slots)] = x
                n += 1
        planted[name] = n

    order = [0] + ek.plant_t(torch.from_numpy(tab))[1:] + list(range(1, tab.size - 1))
    put_sigma("on_table", [tab[i] for i in order])
    put_sigma("ulp_above", [np.nextafter(tab[i], F(np.inf)) for i in order])
    put_sigma("ulp_below", [np.nextafter(tab[i], F(-np.inf)) for i in order[1:]])
    put_sigma("at_bound", [F(0.11)])
    for name, mult in (("below_bound", (0.03, 0.05, 0.08, 0.1)), ("past_table", (1.001, 1.5, 2.0, 4.0))):
        base = F(1.0) if name == "below_bound" else tab[-1]
        for m in mult:
            sigma[next(slots)] = F(m) * base * F(delta)
        planted[name] = 4
    for d in TIES:
        n = 0
        for k in range(4):
            got = plant_tie(d, delta, k)
            if got is not None:
                i = next(slots)
                y[i], mu[i] = got
                n += 1
        planted[f"tie_{d}"] = n
    return NS(y=y, mu=mu, sigma=sigma), planted


def census(y, mu, sigma, delta, table, bound=0.11):
    """the planted classes counted on the restatement alone"""
    r = restate(y, mu, sigma, delta, table, bound)
    tab = np.asarray(table, dtype=F)
    exact = (y.astype(np.float64) - mu.astype(np.float64)) == (y - mu).astype(np.float64)
    out = {f"tie_{d}": int(((r.t == F(d)) & exact).sum()) for d in TIES}
    out.update(on_table=int(np.isin(r.sdiv, tab).sum()),
               ulp_above=int(np.isin(r.sdiv, np.nextafter(tab, F(np.inf))).sum()),
               ulp_below=int(np.isin(r.sdiv, np.nextafter(tab, F(-np.inf))).sum()),
               at_bound=int((r.sdiv == F(0.11)).sum()), below_bound=int((r.sdiv < F(bound)).sum()),
               past_table=int((r.sdiv > tab[-1]).sum()))
    return out


# ------------------------------------------------------------------------------------ slice cases
# (HW, sw, nslices) with n = 3: the 4 x 4 map runs the LDS-tiled kernel, HW = 324 (324 x 17 = 5508 floats > 4800, the
# LDS tile bound) the element kernel
SHAPES = {"tiled1": (16, 16, 1), "tiled2": (16, 16, 2), "tiled6": (16, 16, 6), "element2": (324, 16, 2)}
SEEDS = {"tiled1": 61, "tiled2": 62, "tiled6": 63, "element2": 64}
N_IMAGES = 3


@functools.lru_cache(None)
def case(shape, q=Q3):
    """a slice case in entropy_check.gcf_case's layout (so that gcf_inputs / gcf_outputs build the buffers): image b's
    elements generated and planted at its own step delta(q[b]); q None: the case of q = (0, 0, 0)"""
    HW, sw, nsl = SHAPES[shape]
    n, M = N_IMAGES, N_IMAGES * HW
    qs = (0,) * n if q is None else tuple(q)
    table = ek.model_table()
    Mtot = YOFF + nsl * sw + 4
    per = nsl * HW * sw  # elements of one image
    mu, sigma, ysl = (np.empty((nsl, M, sw), dtype=F) for _ in range(3))
    delta = np.empty((nsl, M, sw), dtype=F)
    planted = []
    for b in range(n):
        el, pl = elements(per, SEEDS[shape] + 100 * b, table, qstep(qs[b]))
        planted.append(pl)
        rows = slice(b * HW, (b + 1) * HW)
        for a, src in ((mu, el.mu), (sigma, el.sigma), (ysl, el.y)):
            a[:, rows, :] = src.reshape(nsl, HW, sw)
        delta[:, rows, :] = qstep(qs[b])
    g = gk._gen(SEEDS[shape] + 1000)
    y = 3 * torch.randn(M, Mtot, generator=g)
    sl = slice(YOFF, YOFF + nsl * sw)
    y[:, sl] = torch.from_numpy(ysl).permute(1, 0, 2).reshape(M, nsl * sw)
    c = NS(shape=shape, n=n, HW=HW, sw=sw, nsl=nsl, yoff=YOFF, Mtot=Mtot, M=M, sl=sl, y=y, noise=None, table=table,
           mu=torch.from_numpy(mu), sigma=torch.from_numpy(sigma), delta=delta, q=qs, planted=planted,
           lik0=2 + torch.rand(M, Mtot, generator=g), yh0=torch.randn(M, Mtot, generator=g),
           yh32_0=torch.randn(M, Mtot + 3, generator=g), ldy=Mtot + 8, ld_ms=sw + 3)
    c.ms_stride = M * c.ld_ms + 5
    return c


@functools.lru_cache(None)
def reference(shape, q=Q3, bound=0.11):
    """{sym, idx: exact in the coder's order; yhat32: f32 values over the WHOLE buffer (untouched elements keep their
    initial contents); lik: (ref, bound) over the whole NCHW buffer}, and the restatement's parts"""
    c = case(shape, q)
    ys = ek.gcf_slices(c, c.y).contiguous().numpy()
    r = restate(ys, c.mu.numpy(), c.sigma.numpy(), c.delta, c.table.numpy(), bound)
    lik, lb = likelihood_reference(r, bound)
    lik_ref, lik_b = c.lik0.double().clone(), torch.zeros(c.M, c.Mtot, dtype=F64)
    lik_ref[:, c.sl], lik_b[:, c.sl] = ek.gcf_rows(c, lik), ek.gcf_rows(c, lb)
    q32 = ek.gcf_rows(c, torch.from_numpy(r.yhat))
    yh, y32 = c.yh0.clone(), c.yh32_0.clone()
    yh[:, c.sl] = q32
    y32[:, c.sl] = q32
    out = {"lik": (ek.to_nchw(lik_ref, c.n, c.HW).reshape(1, -1), ek.to_nchw(lik_b, c.n, c.HW).reshape(1, -1)),
           "yhat": yh, "yhat32": y32, "sym": ek.coder_order(torch.from_numpy(r.sym), c.n, c.HW),
           "idx": ek.coder_order(torch.from_numpy(r.idx), c.n, c.HW)}
    return out, r


def yhat_values(c, out, yt):
    """the whole y_hat buffer in the output dtype: the initial contents cast as gcf_outputs casts them, the slice
    elements the restatement's f32 values rounded to nearest even"""
    ref = c.yh0.to(yt)
    ref[:, c.sl] = out["yhat"][:, c.sl].to(yt)
    return ref


# ------------------------------------------------------------------------------------ the model's slice loop at a step
def oracle_coded(sd, cfg, imgs, scores, q):
    """what decode_bytes(encode_bytes(..., q=q)) reconstructs, restated on the CPU from the oracle's parts
    (oracle/mcm_oracle.py: mcm_forward up to the hyperprior, then its slice loop with the quantiser step of §3.17 per
    image, then its g_s and decoder) -> NS(x_hat, sym int64 [slice][image][channel][pixel] flat as the coder orders
    them, t: every (y - mu) / delta the loop rounded, z_t: every z - median the EntropyBottleneck rounded)"""
    from oracle import mcm_oracle as O

    f32 = torch.float32
    ref = O.mcm_forward(sd, cfg, imgs, scores, keep_intermediates=True)
    sd = {k: (v.to(f32) if torch.is_floating_point(v) else v) for k, v in sd.items()}
    y, lm, ls = ref.inter["y"], ref.inter["latent_means"], ref.inter["latent_scales"]
    n, S = y.shape[0], cfg.num_slices
    delta = torch.tensor([float(qstep(v)) for v in q], dtype=f32).reshape(n, 1, 1, 1)
    hh, ww = y.shape[2:]
    yhat, syms, ts = [], [], []
    for i, ys in enumerate(y.chunk(S, 1)):
        sup = yhat[:S // 2]
        mean_support = torch.cat([lm] + sup, dim=1)
        mu = O.seq_convs(mean_support, sd, f"cc_transform_mean.{i}.", O.CC)[:, :, :hh, :ww]
        t = (ys - mu) / delta
        qi = torch.round(t)
        yh = qi * delta + mu
        lrp = O.seq_convs(torch.cat([mean_support, yh], dim=1), sd, f"lrp_transform.{i}.", O.CC)
        yhat.append(yh + 0.5 * torch.tanh(lrp))
        syms.append(qi.long().reshape(-1))  # [image][channel][pixel]
        ts.append(t.reshape(-1))
    K, D = cfg.num_keep_patches, cfg.encoder_embed_dim
    tk = O.seq_convs(torch.cat(yhat, dim=1), sd, "g_s.", O.G_S).permute(0, 2, 3, 1).contiguous().view(-1, K, D)
    xd = O.linear(tk, sd, "decoder_embed.")
    rest = ref.ids_restore
    L = rest.shape[1]
    mask = sd["mask_token"].repeat(n, L + 1 - xd.shape[1], 1)
    x_ = torch.gather(torch.cat([xd[:, 1:, :], mask], dim=1), 1, rest.unsqueeze(-1).repeat(1, 1, xd.shape[2]))
    x = torch.cat([xd[:, :1, :], x_], dim=1) + sd["decoder_pos_embed"]
    for i in range(cfg.decoder_depth):
        x = O.block(x, sd, f"decoder_blocks.{i}.", cfg.decoder_num_heads, cfg.norm_eps)
    x = O.layer_norm(x, sd, "decoder_norm.", cfg.norm_eps)
    x_hat = O.unpatchify(O.linear(x, sd, "decoder_pred.")[:, 1:, :], cfg.patch_size, cfg.in_chans)
    med = sd["entropy_bottleneck.quantiles"][:, 0, 1].reshape(1, -1, 1, 1)
    return NS(x_hat=x_hat, sym=torch.cat(syms), t=torch.cat(ts), z_t=(ref.inter["z"] - med).reshape(-1), n=n)


def near_ties(t, margin=1e-4):
    """how many of the rounded arguments lie within `margin` of a half-integer"""
    t = t.double()
    return int(((t - torch.floor(t) - 0.5).abs() < margin).sum())
