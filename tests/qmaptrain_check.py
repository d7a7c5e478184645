"""Cases and references of the backward and the training forward at a quantiser step per kept patch:
the kernel tmae_gc_bwd_qm, tmae_lic_stack's chain with cqm and the model's training forward with a map.  It does for
qmap_check.py (§3.19) what qtrain_check.py (§3.18) does for qstep_check.py, and changes none of them:

* every function of qtrain_check that takes a case reads the step from c.delta, one value per row (= image x pixel) of
  the [M][sw] slice, so the per-image cases of §3.18 become per-pixel ones by giving them another delta: gcqm_case is
  qtrain_check.gcq_case's recipe with delta[b HW + p] = qstep(qmap[b][p]), the map cycling through qmap_check.CYCLES
  (lengths 5 and 4 do not divide HW = 9 or 16, so a step indexed by row, channel or slice differs from one indexed by
  pixel), y / mu / sigma in units of the element's own step and sigma planted at PLANT x bound x that step;
* the reference (float64 autograd of the definition, the kernel's formula carried through E, the skip mask and its cap)
  is qtrain_check.gcq_bwd_reference on that case: Delta is a function of (image, pixel) and nothing else changes;
* MAP_MUTANTS are the three faults a map adds to qtrain_check.GCQ_MUTANTS: one step per image (pixel 0's), one map row
  for every image (image 0's), the map indexed by the slice channel in place of the pixel.

tests/test_qmaptrain_host.py checks this file on the CPU; tests/test_gpu_qmaptrain_kernels.py and
test_gpu_qmaptrain_model.py check the kernels and the model against it."""
import copy
import functools
from types import SimpleNamespace as NS

import numpy as np
import torch

import glue_check as gk
import qmap_check as mk
import qstep_check as qk
import qtrain_check as tk
from glue_check import F32

F = np.float32
BOUND = tk.BOUND
GCQ_SHAPES = tk.GCQ_SHAPES
# chosen on the reference alone: its skipped share stays under glue_check.SKIP_CAP and every image holds every branch
# class (test_qmaptrain_host asserts both and records the counts; of the seeds 20..79 for three_wg, 20 do)
GCQM_SEEDS = {"small": 31, "three_wg": 47}


def row_steps(qmap):
    """int [n, HW] ladder positions -> f32 [n HW, 1]: the step of every row of a slice"""
    return torch.from_numpy(mk.steps(qmap).reshape(-1, 1).copy())


@functools.lru_cache(None)
def gcqm_case(shape, constant=None):
    """qtrain_check.gcq_case's recipe in units of each PIXEL's step; constant = (q0, q1, q2): a map that is constant
    over each image (the per-image case of §3.18 written as a map), same random draws"""
    d = GCQ_SHAPES[shape]
    n, HW, sw, Mtot, yoff = tk.N_IMAGES, d["HW"], d["sw"], d["Mtot"], d["yoff"]
    qmap = mk.qmap_of(HW) if constant is None else np.repeat(np.array(constant, dtype=np.int32)[:, None], HW, axis=1)
    g = gk._gen(GCQM_SEEDS[shape])
    M = n * HW
    dl = row_steps(qmap)
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
        for k, mult in enumerate(tk.PLANT):
            m, c = b * HW + (2 * k + 1) % HW, (3 * k + b) % sw
            sigma[m, c] = torch.tensor(BOUND * mult, dtype=F32) * dl[m, 0]
    return NS(shape=shape, n=n, HW=HW, sw=sw, Mtot=Mtot, yoff=yoff, M=M, y=y, mu=mu, sigma=sigma, noise=noise,
              glik=glik, gyp=gyp, dy0=dy0, ldy=Mtot + 8, ld_ms=sw + 3, ldg=Mtot + 3, qmap=qmap, delta=dl,
              q=None if constant is None else tuple(constant))


MAP_MUTANTS = ("pixel0_for_the_image", "image0_for_every_image", "indexed_by_channel")


def mutant_case(c, mutant):
    """the case as a faulty kernel would read its map: the inputs stay, only the step of every element changes"""
    d = copy.copy(c)
    if mutant == "pixel0_for_the_image":
        qm = np.repeat(c.qmap[:, :1], c.HW, axis=1)
        d.delta = row_steps(qm)
    elif mutant == "image0_for_every_image":
        qm = np.repeat(c.qmap[:1], c.n, axis=0)
        d.delta = row_steps(qm)
    elif mutant == "indexed_by_channel":  # qmap[b][c] in place of qmap[b][p]: the step of element (row, channel)
        st = mk.steps(c.qmap)  # [n, HW]
        cols = np.arange(c.sw) % c.HW
        d.delta = torch.from_numpy(np.repeat(st[:, cols], c.HW, axis=0).copy())  # [M, sw]
    else:
        raise ValueError(mutant)
    assert not torch.equal(d.delta.expand(c.M, c.sw), c.delta.expand(c.M, c.sw))
    return d


def rejected(out, dy, dmu, ds, tag):
    """how many of the three outputs the checker refuses"""
    bad = 0
    for k, v in (("dy", dy), ("dmu", dmu), ("dsigma", ds)):
        try:
            gk.check(f"{tag}:{k}", gk.written(v.float(), F32), *out[k], log=False)
        except AssertionError:
            bad += 1
    return bad


# ------------------------------------------------------------------------------------ the model's training forward
def mcm_forward_qm(sd, cfg, imgs, scores, z_noise, y_noise, qmap, bound=BOUND, lanes=8):
    """qtrain_check.mcm_forward_q with delta shaped [n, 1, g, g] from a map of clamped ladder positions (int [n, K],
    pixel p of the g x g latent grid = kept token p): the same statements in the same order, so that a map constant over
    each image gives mcm_forward_q's values to the last bit -> the same namespace plus qmap"""
    import torch.nn.functional as Fn

    from oracle import ids as ids_oracle
    from oracle import mcm_oracle as O
    from oracle import train_oracle as orc

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
    qmap = np.asarray(qmap).reshape(n, K)
    delta = torch.tensor([float(qk.qstep(v)) for v in qmap.reshape(-1)], dtype=y.dtype).reshape(n, 1, hh, ww)
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
    tk_ = O.seq_convs(torch.cat(yhat, dim=1), sd, "g_s.", O.G_S).permute(0, 2, 3, 1).contiguous().view(-1, K, D)
    xd = O.linear(tk_, sd, "decoder_embed.")
    L = rest.shape[1]
    mask = sd["mask_token"].repeat(n, L + 1 - xd.shape[1], 1)
    x_ = torch.gather(torch.cat([xd[:, 1:, :], mask], dim=1), 1, rest.unsqueeze(-1).repeat(1, 1, xd.shape[2]))
    x = torch.cat([xd[:, :1, :], x_], dim=1) + sd["decoder_pos_embed"]
    for i in range(cfg.decoder_depth):
        x = O.block(x, sd, f"decoder_blocks.{i}.", cfg.decoder_num_heads, cfg.norm_eps)
    x = O.layer_norm(x, sd, "decoder_norm.", cfg.norm_eps)
    x_hat = O.unpatchify(O.linear(x, sd, "decoder_pred.")[:, 1:, :], p, cfg.in_chans)
    return NS(x_hat=x_hat, y_lik=torch.cat(liks, dim=1), z_lik=z_lik, t=torch.cat(ts), sym=torch.cat(syms),
              gate=torch.cat(gates), qmap=qmap, ids_shuffle=shuf)


def score_map(cfg, scores, q, offsets, lanes=8):
    """the map the model builds from the scores: oracle ids_shuffle, bitstream.select_levels_host (the numpy restatement
    of tmae_qlevels_select) and build_qmap_host -> (levels int32 [n, K], qmap int32 [n, K])"""
    from oracle import ids as ids_oracle
    from textmae_amd import bitstream as bs

    K = cfg.num_keep_patches
    shuf, _ = ids_oracle.ids_shuffle(scores.float().cpu().numpy(), K, lanes)
    n = shuf.shape[0]
    levels, _ = bs.select_levels_host(shuf, K, len(offsets), scores=scores.float().cpu().numpy())
    q = [0] * n if q is None else list(q)
    return np.asarray(levels), np.asarray(bs.build_qmap_host(levels, q, [bs.offsets_row(offsets)] * n))
