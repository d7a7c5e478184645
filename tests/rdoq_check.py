"""Cases and references of the rate-distortion optimised quantisation of y (tmae_gc_slices_code_rdo,
csrc/coding_rdo.hip and csrc/gc_rdo.h): the sibling of qstep_check.py and qmap_check.py, whose
layouts, planting and restatement it builds on.  tests/test_rdoq_host.py checks this file on the CPU,
tests/test_gpu_rdoq_kernels.py the kernel and tests/test_gpu_rdoq_model.py the model against it.

The reference is a numpy f32 RESTATEMENT of the rule, every line one f32 operation as in the kernel:

    t    = fl(fl(y - mu) / delta);  qi0 = rint(t)             qstep_check.restate
    if qi0 == 0: keep qi0
    qi1  = qi0 - copysign(1, qi0)
    e0 = qi0 - t;  e1 = qi1 - t
    dd   = fl(fl(e1 e1) - fl(e0 e0))
    rhs  = fl(fl(delta delta) dd)
    lhs  = fl(w fl(bits(r, qi0) - bits(r, qi1)))              coder.symbol_bits on the f32 table the kernel reads
    qi   = qi1 if lhs > rhs else qi0
    y_hat = fl(fl(qi delta) + mu);  r, s as in qstep_check.restate

The kernel and this file read the same f32 table entries (coder.rate_table, built once on the host), so no log2 is
taken on either side and symbols, indexes, both y_hat outputs and the per-image counts of moved symbols are compared
bit for bit, no element skipped and no near-tie allowance; the likelihood takes qstep_check.likelihood_reference's
method at the chosen qi.
"""
import copy
import functools
from types import SimpleNamespace as NS

import numpy as np
import torch

import entropy_check as ek
import qmap_check as qm
import qstep_check as qk
from glue_check import F64
from oracle import coding_oracle as co

F = np.float32
Q3 = qk.Q3
W3 = (0.0, 0.5, 1000.0)  # per image: plain rounding, a moderate weight, one at which every saving of bits wins
MODES = ("q", "none", "qmap")  # the step per image at Q3, no step (both pointers NULL), a map per pixel
SHAPES = ("tiled2", "element2")  # the LDS form and the element form
SEEDS = {"tiled2": 262, "element2": 264}
TIES = (1.5, -1.5, 2.5, -2.5)  # rint gives 2, -2, 2, -2: dd = 0, 0, 2, 2


# ------------------------------------------------------------------------------------ tables
@functools.lru_cache(None)
def tables():
    """the CDF tables of the model's 64-entry scale table, built on the CPU (oracle/coding_oracle.gc_update), and their
    rate table -> NS(cdf, sizes, offsets int32 numpy, rate f32 numpy): inputs to the kernel and to the restatement"""
    from textmae_amd import coder

    cdf, sizes, offsets = (np.ascontiguousarray(t.numpy().astype(np.int32)) for t in co.gc_update(ek.model_table()))
    return NS(cdf=cdf, sizes=sizes, offsets=offsets, rate=coder.rate_table(cdf, sizes))


def rate_table64(cdf, sizes):
    """the rate table in float64 from the definition, one entry at a time per row"""
    out = np.zeros((cdf.shape[0], cdf.shape[1] - 1), dtype=np.float64)
    for r in range(cdf.shape[0]):
        for k in range(int(sizes[r]) - 1):
            out[r, k] = 16.0 - np.log2(float(int(cdf[r, k + 1]) - int(cdf[r, k])))
    return out


def equal_pair(tb):
    """(row r >= 1, symbol v >= 2) with v and v - 1 both inside the row's support and of equal frequency: the first"""
    for r in range(1, tb.cdf.shape[0]):
        c = -int(tb.offsets[r])
        freq = np.diff(tb.cdf[r].astype(np.int64))
        for v in range(2, c + 1):
            if freq[v + c] == freq[v - 1 + c]:
                return r, v
    raise AssertionError("no row with two equal neighbouring frequencies")


# ------------------------------------------------------------------------------------ the restatement
def restate(y, mu, sigma, delta, w, table, tb, bound=0.11):
    """numpy f32 arrays of one shape (delta, w broadcastable) -> qstep_check.restate's fields at the CHOSEN qi, and
    qi0, qi1, flipped, b0, b1, db, dd, lhs, rhs of the decision (0 where qi0 == 0)"""
    from textmae_amd import coder

    r0 = qk.restate(y, mu, sigma, delta, table, bound)
    shape = r0.qi.shape
    delta = np.broadcast_to(np.asarray(delta, dtype=F), shape)
    w = np.broadcast_to(np.asarray(w, dtype=F), shape)
    mu = np.asarray(mu, dtype=F)
    qi0, t = r0.qi, r0.t
    nz = qi0 != 0
    qi1 = qi0 - np.copysign(F(1), qi0)
    e0, e1 = qi0 - t, qi1 - t
    a1, a0 = e1 * e1, e0 * e0
    dd = a1 - a0
    d2 = delta * delta
    rhs = d2 * dd
    bits = lambda q: coder.symbol_bits(q.astype(np.int64).reshape(-1), r0.idx.reshape(-1), tb.rate, tb.sizes,  # noqa: E731
                                       tb.offsets).reshape(shape)
    b0, b1 = bits(qi0), bits(qi1)
    db = b0 - b1
    lhs = w * db
    assert all(a.dtype == F for a in (qi1, e0, e1, a1, a0, dd, d2, rhs, b0, b1, db, lhs))
    flipped = nz & (lhs > rhs)
    qi = np.where(flipped, qi1, qi0)
    p = qi * delta
    yhat = p + mu
    assert qi.dtype == F and yhat.dtype == F
    z = lambda a: np.where(nz, a, F(0))  # noqa: E731
    return NS(qi=qi, sym=qi.astype(np.int64), yhat=yhat, s=r0.s, sdiv=r0.sdiv, idx=r0.idx, t=t, qi0=qi0, qi1=z(qi1),
              flipped=flipped, b0=b0, b1=z(b1), db=z(db), dd=z(dd), lhs=z(lhs), rhs=z(rhs), w=w, delta=delta)


# ------------------------------------------------------------------------------------ cases
def _plants(tb):
    """(name, sigma / delta, t or None for the exact ties) of what is planted once per image"""
    r, v = equal_pair(tb)
    tab = ek.model_table().numpy().astype(F)
    mid = float(tab[r - 1]) + 0.5 * (float(tab[r]) - float(tab[r - 1]))  # a scale strictly inside row r's interval
    out = [("one_to_zero", 0.05, 0.6), ("one_to_zero", 0.05, -0.6), ("equal_freq", mid, v + 0.2),
           ("equal_freq", mid, -v - 0.2), ("esc_to_support", 0.05, 2.1), ("esc_to_support", 0.05, -2.1),
           ("both_esc", 0.05, 3.3), ("both_esc", 0.05, -3.3), ("both_esc", 0.05, 10.2), ("both_esc", 0.05, -10.2),
           ("widest", 300.0, 40.3), ("widest", 300.0, -40.3), ("widest", 300.0, 1.45), ("narrowest", 0.05, 1.3)]
    return out + [(f"tie_{d}", 0.3, None) for d in TIES for _ in range(2)]


@functools.lru_cache(None)
def case(shape, mode):
    """qstep_check.case (mode "q": q = Q3; "none": no q, step 1) or qmap_check.case (mode "qmap") with, per image, the
    classes of _plants written over seeded elements at the element's own step, and the per-image weights W3"""
    assert shape in SHAPES and mode in MODES
    base = qk.case(shape) if mode == "q" else qk.case(shape, None) if mode == "none" else qm.case(shape)
    c = copy.copy(base)
    c.y, c.mu, c.sigma = base.y.clone(), base.mu.clone(), base.sigma.clone()
    c.mode, c.w = mode, W3
    c.q = tuple(base.q) if mode == "q" else None
    c.qmap = base.qmap if mode == "qmap" else None
    tb = tables()
    rng = np.random.default_rng(SEEDS[shape] + 10 * MODES.index(mode))
    per = c.nsl * c.HW * c.sw
    for b in range(c.n):
        plants = _plants(tb)
        slots = rng.choice(per, size=len(plants), replace=False)
        for slot, (name, sdiv, t) in zip(slots.tolist(), plants):
            j, rem = divmod(slot, c.HW * c.sw)
            p, ch = divmod(rem, c.sw)
            m = b * c.HW + p
            d = F(c.delta[j, m, ch])
            if t is None:
                got = qk.plant_tie(float(name[4:]), d, 0)
                if got is None:
                    continue
                yv, mv = got
            else:
                yv, mv = F(t) * d, F(0)
            c.mu[j, m, ch], c.sigma[j, m, ch] = float(mv), float(F(sdiv) * d)
            c.y[m, c.yoff + j * c.sw + ch] = float(yv)
    c.wmap = np.repeat(np.asarray(W3, dtype=F), c.HW)[None, :, None]  # [1][M][1]: the weight of every row's image
    return c


@functools.lru_cache(None)
def reference(shape, mode, w=None, bound=0.11):
    """qstep_check.reference's dict for the case at its weights (w: another triple, e.g. zeros) plus "changed": the
    per-image count of moved symbols; and the restatement's parts"""
    c = case(shape, mode)
    wmap = c.wmap if w is None else np.repeat(np.asarray(w, dtype=F), c.HW)[None, :, None]
    ys = ek.gcf_slices(c, c.y).contiguous().numpy()
    r = restate(ys, c.mu.numpy(), c.sigma.numpy(), c.delta, wmap, c.table.numpy(), tables(), bound)
    lik, lb = qk.likelihood_reference(r, bound)
    lik_ref, lik_b = c.lik0.double().clone(), torch.zeros(c.M, c.Mtot, dtype=F64)
    lik_ref[:, c.sl], lik_b[:, c.sl] = ek.gcf_rows(c, lik), ek.gcf_rows(c, lb)
    q32 = ek.gcf_rows(c, torch.from_numpy(r.yhat))
    yh, y32 = c.yh0.clone(), c.yh32_0.clone()
    yh[:, c.sl] = q32
    y32[:, c.sl] = q32
    changed = r.flipped.reshape(c.nsl, c.n, c.HW, c.sw).sum(axis=(0, 2, 3))
    out = {"lik": (ek.to_nchw(lik_ref, c.n, c.HW).reshape(1, -1), ek.to_nchw(lik_b, c.n, c.HW).reshape(1, -1)),
           "yhat": yh, "yhat32": y32, "sym": ek.coder_order(torch.from_numpy(r.sym), c.n, c.HW),
           "idx": ek.coder_order(torch.from_numpy(r.idx), c.n, c.HW), "changed": torch.from_numpy(changed)}
    return out, r


def census(c, r):
    """the classes the kernel can get wrong, counted on the restatement alone -> (classes over the whole case, per image
    (flips, keeps) among the elements with qi0 != 0)"""
    tb = tables()
    ys, mu = ek.gcf_slices(c, c.y).contiguous().numpy(), c.mu.numpy()
    exact = (ys.astype(np.float64) - mu.astype(np.float64)) == (ys - mu).astype(np.float64)
    maxv = tb.sizes.astype(np.int64)[r.idx] - 2
    off = tb.offsets.astype(np.int64)[r.idx]
    v0, v1 = r.qi0.astype(np.int64) - off, np.where(r.qi0 != 0, r.qi1, r.qi0).astype(np.int64) - off
    in0, in1 = (v0 >= 0) & (v0 < maxv), (v1 >= 0) & (v1 < maxv)
    nz, pos = r.qi0 != 0, r.w > 0
    out = {"zero": int((~nz).sum()), "one_to_zero": int((r.flipped & (np.abs(r.qi0) == 1)).sum()),
           "equal_freq_kept": int((nz & pos & in0 & in1 & (r.db == 0) & ~r.flipped).sum()),
           "esc_to_support": int((nz & ~in0 & in1).sum()),
           "both_esc_above": int((nz & ~in0 & ~in1 & (v1 >= maxv)).sum()),
           "both_esc_below": int((nz & ~in0 & ~in1 & (v0 < 0)).sum()),
           "widest_row": int((nz & (r.idx == tb.sizes.size - 1)).sum()), "narrowest_row": int((nz & (r.idx == 0)).sum())}
    for d in TIES:
        out[f"tie_{d}"] = int(((r.t == F(d)) & exact & (r.dd == (F(0) if abs(d) == 1.5 else F(2)))).sum())
    img = lambda a: a.reshape(c.nsl, c.n, c.HW, c.sw).sum(axis=(0, 2, 3))  # noqa: E731
    return out, list(zip(img(r.flipped).tolist(), img(nz & ~r.flipped).tolist()))


# ------------------------------------------------------------------------------------ the model's slice loop
def oracle_coded(sd, cfg, imgs, scores, q, w, tb, table, bound=0.11):
    """qstep_check.oracle_coded with the rule above in its slice loop: what decode_bytes(encode_bytes(..., q=q,
    rdoq=w)) reconstructs, restated on the CPU.  tb: NS(sizes, offsets, rate) of the MODEL's tables, table: its scale
    table -> qstep_check.oracle_coded's fields, and lhs / rhs of every decision taken at qi0 != 0, changed per image"""
    from oracle import mcm_oracle as O

    f32 = torch.float32
    ref = O.mcm_forward(sd, cfg, imgs, scores, keep_intermediates=True)
    sd = {k: (v.to(f32) if torch.is_floating_point(v) else v) for k, v in sd.items()}
    y, lm, ls = ref.inter["y"], ref.inter["latent_means"], ref.inter["latent_scales"]
    n, S = y.shape[0], cfg.num_slices
    delta = np.array([float(qk.qstep(v)) for v in q], dtype=F).reshape(n, 1, 1, 1)
    wv = np.asarray(w, dtype=F).reshape(n, 1, 1, 1)
    hh, ww = y.shape[2:]
    yhat, syms, ts, lhs, rhs, changed = [], [], [], [], [], np.zeros(n, dtype=np.int64)
    for i, ys in enumerate(y.chunk(S, 1)):
        sup = yhat[:S // 2]
        mean_support = torch.cat([lm] + sup, dim=1)
        scale_support = torch.cat([ls] + sup, dim=1)
        mu = O.seq_convs(mean_support, sd, f"cc_transform_mean.{i}.", O.CC)[:, :, :hh, :ww]
        sigma = O.seq_convs(scale_support, sd, f"cc_transform_scale.{i}.", O.CC)[:, :, :hh, :ww]
        r = restate(ys.numpy(), mu.numpy(), sigma.numpy(), delta, wv, table, tb, bound)
        yh = torch.from_numpy(r.yhat)
        lrp = O.seq_convs(torch.cat([mean_support, yh], dim=1), sd, f"lrp_transform.{i}.", O.CC)
        yhat.append(yh + 0.5 * torch.tanh(lrp))
        syms.append(torch.from_numpy(r.sym).reshape(-1))  # [image][channel][pixel]
        ts.append(torch.from_numpy(r.t).reshape(-1))
        nz = r.qi0 != 0
        lhs.append(r.lhs[nz])
        rhs.append(r.rhs[nz])
        changed += r.flipped.reshape(n, -1).sum(axis=1)
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
    return NS(x_hat=x_hat, sym=torch.cat(syms), t=torch.cat(ts), n=n, lhs=np.concatenate(lhs),
              rhs=np.concatenate(rhs), changed=changed)


def near_decisions(lhs, rhs, margin=1e-4):
    """how many decisions have |lhs - rhs| below `margin` of max(|lhs|, |rhs|, 1e-6)"""
    lhs, rhs = np.asarray(lhs, dtype=np.float64), np.asarray(rhs, dtype=np.float64)
    return int((np.abs(lhs - rhs) < margin * np.maximum(np.maximum(np.abs(lhs), np.abs(rhs)), 1e-6)).sum())
