"""Training path of the MCM drop-in: MCM.forward under autograd (utils/engine.py:75-91 calls
``model(samples, total_scores)``, ``criterion(out_net, samples)``, ``loss.backward()``).

One ``torch.autograd.Function`` covers the whole model: its forward enqueues the same gfx950 kernels
as inference but keeps every activation the backward needs (GELU inputs, attention log-sum-exp,
per-slice stack activations, ...); its backward is the full reverse pass on HIP kernels (split-K
TN weight gradients, transposed-weight data gradients, LayerNorm / attention / entropy-model
backward) writing every parameter gradient into one flat f32 buffer, whose views are returned to
autograd (AccumulateGrad adopts them as ``p.grad``).  A ``GradSync`` attached to the model all-reduces
that buffer in buckets over RCCL while the backward is still running (data parallel).

Reference semantics reproduced (compressai 1.2.4 / timm 0.4.5 restated):
  * training mode: EntropyBottleneck / GaussianConditional likelihoods of x + U(-1/2, 1/2);
    z_hat, y_hat through quantize_ste (pass-through gradient, MCM.py:742-744, 776);
  * LowerBound backward (gradient passes where x >= bound or grad < 0);
  * the main loss's gradient on ``*.quantiles`` is exactly zero (d z_hat / d median = -1 + 1) and is
    returned as zeros, so clip_grad_norm_ / aux_loss.backward() see what they see in the reference.
The slice loop runs slices 0..ms-1 one by one and slices ms..S-1, which condition on the same support slots, as one
group (TrainExec._group_fwd / _slices_bwd).  The weight cache is train_weights._Weights, the machinery shared with
the MAE executor vit_train._VitTrainBase.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import ops
from . import train_ops as T
from .ops import ACT_GELU, ACT_NONE
from .train_weights import _Weights  # noqa: F401  (re-exported: tests and tools import it from here)
from .vit_train import _SIDE_SLOT_DIV, _bias, _BlockSaved, _block_params, _VitTrainBase  # noqa: F401


def _convs(seq):
    return [l for l in seq if isinstance(l, nn.Conv2d)]


class TrainExec(_VitTrainBase):
    """Workspaces + saved activations of one training forward for (batch, dtype, device)."""

    def __init__(self, m, batch, dtype, device):
        self.m, self.batch, self.dtype, self.device = m, batch, dtype, device
        self.w = _Weights(dtype)
        K = m.num_keep_patches
        self.P = m.encoder_embed.patch_size[0]
        self.img = m.encoder_embed.img_size[0]
        self.L = m.encoder_embed.num_patches
        self.g = int(round(K ** 0.5))
        if self.g * self.g != K:
            raise ValueError(f"num_keep_patches={K} must be a perfect square (MCM.py:729-732)")
        self.hz = ((self.g + 1) // 2 + 1) // 2
        if self.hz * 4 != self.g:
            raise ValueError(f"sqrt(num_keep_patches)={self.g} must be a multiple of 4 so h_s returns to the y grid")
        self.Mp = batch * K
        self.sw = m.latent_depth // m.num_slices
        self.ms = m.num_slices // 2
        # the coder's scale bound of the step kernels, read once: a captured step must not read it back
        gc = m.gaussian_conditional
        self.scale_bound = float(gc.scale_bound) if gc.scale_bound is not None else 0.11
        self.qd = None  # the forward's per-image ladder positions on the device, kept for its backward
        self.mid = [l.out_channels for l in _convs(m.cc_transform_mean[0])]
        S, ms = m.num_slices, self.ms
        self.cm, self.cs, self.cl = ([_convs(seq[i]) for i in range(S)]
                                     for seq in (m.cc_transform_mean, m.cc_transform_scale, m.lrp_transform))
        # slices 0..nser-1 run one by one (each conditions on the ones before); slices ms..S-1 all condition on y_hat
        # slots 0..ms-1 only (max_support_slices, MCM.py:73, 756-758), so two or more of them run as one group
        self.nser = ms if S - ms > 1 else S
        # launch groups: the [mean.. | scale..] stacks and the lrp stacks of each slice group.  A stack's weight packs
        # are always its launch group's (_pack), whichever launch asks and on however many streams: the weight cache
        # keeps one grouping per parameter
        self._lgroup = {}
        self.slice_groups = [(i, 1) for i in range(self.nser)] + ([(self.nser, S - self.nser)] if self.nser < S else [])
        for i0, nbs in self.slice_groups:
            sl = range(i0, i0 + nbs)
            for grp in ([self.cm[i] for i in sl] + [self.cs[i] for i in sl], [self.cl[i] for i in sl]):
                for r, convs in enumerate(grp):
                    self._lgroup[id(convs[0])] = (grp, r)
        # forward counters of the two ViT stages: a staged backward (_MCMEncFn / _MCMDecFn) refuses activations a later
        # forward of that stage -- or a whole forward -- replaced
        self.enc_gen = self.dec_gen = 0
        self._layout()

    def _grad_order(self):
        m = self.m
        out = [m.decoder_pred.weight, m.decoder_pred.bias, m.decoder_norm.weight, m.decoder_norm.bias]
        for blk in reversed(m.decoder_blocks):
            out += _block_params(blk)
        out += [m.decoder_embed.weight, m.decoder_embed.bias, m.mask_token]
        for l in reversed([l for l in m.g_s if isinstance(l, nn.ConvTranspose2d)]):
            out += [l.weight, l.bias]
        for i in reversed(range(m.num_slices)):
            for seq in (m.lrp_transform[i], m.cc_transform_mean[i], m.cc_transform_scale[i]):
                for c in reversed(_convs(seq)):
                    out += [c.weight, c.bias]
        for seq in (m.h_s_mean, m.h_s_scale):
            for c in reversed(_hs_convs(seq)):
                out += [c.weight, c.bias]
        eb = m.entropy_bottleneck
        out += [getattr(eb, f"_matrix{i}") for i in range(5)] + [getattr(eb, f"_bias{i}") for i in range(5)]
        out += [getattr(eb, f"_factor{i}") for i in range(4)] + [eb.quantiles]
        for c in reversed(_convs(m.h_a)):
            out += [c.weight, c.bias]
        for l in reversed([l for l in m.g_a if isinstance(l, nn.Conv2d)]):
            out += [l.weight, l.bias]
        out += [m.encoder_norm.weight, m.encoder_norm.bias]
        for blk in reversed(m.encoder_blocks):
            out += _block_params(blk)
        out += [m.encoder_embed.proj.weight, m.encoder_embed.proj.bias, m.cls_token]
        seen, uniq = set(), []
        for p in out:
            if id(p) not in seen:
                seen.add(id(p))
                uniq.append(p)
        missing = [n for n, p in m.named_parameters() if p.requires_grad and id(p) not in seen]
        if missing:
            raise RuntimeError(f"training executor does not cover parameters {missing}")
        return uniq

    # ------------------------------------------------------------------ forward
    def forward(self, imgs, scores, noise, q=None, qm=None):
        """q: None, B ladder positions (uploaded once, before the first launch) or an int32 [B] device tensor.
        qm: None, or MCM._check_qoffsets' pair (the table of offsets, "scores" or a map of levels in
        image patch order), optionally followed by the offsets' rows already on the device (int32 [B, 16], a captured
        step's static buffer).  q is then the base position; the levels are selected once, after ids_shuffle exists,
        and the map of clamped ladder positions (self.qmd, int32 [B, K]) stays for the backward."""
        m, B, g = self.m, self.batch, self.g
        M, N, hz = m.latent_depth, m.hyperprior_depth, self.hz
        self.qd = q if q is None or torch.is_tensor(q) else torch.tensor(q, dtype=torch.int32).to(self.device)
        self.qmd = self.qm_status = None
        self._qm = None if qm is None else self._map_upload(qm)
        imgs = self._begin(imgs)
        if noise is not None:
            self.z_noise, self.y_noise = (t.float().contiguous() for t in noise)
        elif not m.training:  # eval semantics: round(x - median) + median / round(y - mu) + mu
            self.z_noise = self.y_noise = None
        else:
            self.z_noise = torch.empty((B, N, hz, hz), device=self.device).uniform_(-0.5, 0.5)
            self.y_noise = torch.empty((B, M, g, g), device=self.device).uniform_(-0.5, 0.5)
        self.enc_out = self.enc_fwd(imgs, scores)
        if self._qm is not None:
            self._build_map(scores)
        self._lic_fwd(self.enc_out)
        x_hat = self.dec_fwd(self.gs_out)
        return x_hat, self.YLIK, self.ZLIK

    # ------------------------------------------------------------------ per-patch quantiser steps
    def _map_upload(self, qm):
        """the eval executor's _map_upload: everything of qm that lives on the host goes up before the first launch ->
        (table size, "scores" | int32 [B, L] device tensor, device offsets [B, 16], whether the device checks the map)"""
        from .bitstream import offsets_row

        offs, src = qm[0], qm[1]
        rows = qm[2] if len(qm) > 2 and qm[2] is not None else None
        if rows is None:
            rows = torch.tensor([offsets_row(offs)] * self.batch, dtype=torch.int32).to(self.device)
        on_device = torch.is_tensor(src)
        if isinstance(src, np.ndarray):
            src = torch.from_numpy(src).to(self.device)
        return len(offs), src, rows, on_device

    def _build_map(self, scores):
        """levels of the kept patches (tmae_qlevels_select: from the scores, or the caller's map gathered by
        ids_shuffle), then the clamped ladder positions at the base q (tmae_qmap_build) -> self.qmd; the levels carry
        no gradient.  self.qm_status: int32 [B] on the device when the map came from the device (1 = an entry outside
        the table, that image's levels all zero), else None.  Nothing is read back."""
        nlev, src, rows, on_device = self._qm
        K = self.m.num_keep_patches
        if isinstance(src, str):
            self.qm_levels, _ = ops.qlevels_select(self.shuf, K, nlev, scores=scores.float().contiguous())
        else:
            self.qm_levels, status = ops.qlevels_select(self.shuf, K, nlev, level_map=src)
            self.qm_status = status if on_device else None
        self.qmd = ops.qmap_build(self.qm_levels, self.qd, rows)

    def _begin(self, imgs):
        """what every forward entry starts with: the image check and the weight copies' refresh"""
        m = self.m
        imgs = imgs.float().contiguous()
        if imgs.shape[1:] != (m.encoder_embed.proj.in_channels, self.img, self.img):
            raise ValueError(f"Input image size {tuple(imgs.shape[2:])} doesn't match model ({self.img})")
        self.imgs = imgs
        self.w.refresh()  # one launch for every weight copy the last optimizer step made stale
        return imgs

    def enc_fwd(self, imgs, scores, out_dtype=None):
        """forward_encoder (MCM.py:590-634) of imgs (after _begin): masking ids, kept-patch embedding, cls, blocks,
        encoder_norm without the cls rows -> [B*K, E] in out_dtype (the compute dtype by default); keeps the
        encoder's activations and the shuffle for the backward"""
        m, dt, B, W = self.m, self.dtype, self.batch, self.w
        E, K, P = m.encoder_embed_dim, m.num_keep_patches, self.P
        Te = K + 1
        self.enc_gen += 1
        shuf, rest = ops.ids_shuffle(scores, K, m.sum_lanes)
        self.shuf, self.rest = shuf, rest
        pos_e = m.encoder_pos_embed.detach()
        tok = torch.empty((B * Te, E), dtype=torch.float32, device=self.device)
        self.patches = T.patch_gather(imgs, shuf, self._e(B * K, m.encoder_embed.proj.weight[0].numel()), K, P, dt)
        ops.patch_embed(imgs, shuf, W.nt(m.encoder_embed.proj.weight), m.encoder_embed.proj.bias.detach(), pos_e, tok,
                        K, P, dt, patches=self.patches)
        ops.cls_rows(tok, m.cls_token.detach(), pos_e, B, Te, E)
        self.enc = []
        for blk in m.encoder_blocks:
            tok = self._block_fwd(blk, tok, B, Te)
        self.tok_last = tok
        return ops.layernorm(tok, m.encoder_norm.weight, m.encoder_norm.bias, m.encoder_norm.eps, out_dtype or dt,
                             rows=B * K, row_group=K, group_stride=Te, row_offset=1)

    def _lic_fwd(self, enc_out):
        """g_a, h_a, the entropy models, h_s, the slice loop and g_s (MCM.py:729-792) -> self.gs_out"""
        m, dt, B, W = self.m, self.dtype, self.batch, self.w
        g = self.g
        M, N, hz = m.latent_depth, m.hyperprior_depth, self.hz

        # ---- g_a (MCM.py:735)
        x = enc_out
        self.ga = []  # (input, pre) per GELU layer
        ga = [l for l in m.g_a if isinstance(l, nn.Conv2d)]
        for j, l in enumerate(ga):
            if j < len(ga) - 1:
                h, pre = self._e(self.Mp, l.out_channels), self._e(self.Mp, l.out_channels)
                T.linear_pre(x, W.nt(l.weight), l.bias.detach(), dt, ACT_GELU, h, pre)
                self.ga.append((x, pre))
                x = h
            else:
                self.ga.append((x, None))
                self.Y32 = torch.empty((self.Mp, M), dtype=torch.float32, device=self.device)
                if dt == torch.float32:
                    ops.linear(x, W.nt(l.weight), l.bias.detach(), dt, out=self.Y32)
                    self.YT = self.Y32
                else:
                    self.YT = self._e(self.Mp, M)
                    ops.linear(x, W.nt(l.weight), l.bias.detach(), dt, out=self.YT, out32=self.Y32)

        # ---- h_a (MCM.py:739)
        self.ha = []
        x, cin, H = self.YT, M, g
        convs = _convs(m.h_a)
        for j, c in enumerate(convs):
            last = j == len(convs) - 1
            s = c.stride[0]
            Ho = (H + 2 - 3) // s + 1
            if last:
                out, pre = torch.empty((B * Ho * Ho, c.out_channels), dtype=torch.float32, device=self.device), None
            else:
                out, pre = self._e(B * Ho * Ho, c.out_channels), self._e(B * Ho * Ho, c.out_channels)
            ops.conv3x3(x, cin, cin, B, H, H, W.conv(c.weight), c.bias.detach(), out, c.out_channels, c.out_channels,
                        dt, stride=s, act=ACT_NONE if last else ACT_GELU, pre=pre, ldp=c.out_channels,
                        y_f32=last)
            self.ha.append((x, cin, H, s, pre))
            x, cin, H = out, c.out_channels, Ho
        self.Z = x

        # ---- entropy bottleneck + z_hat (MCM.py:741-744)
        eb = m.entropy_bottleneck
        self.ZLIK = torch.empty((B, N, hz, hz), dtype=torch.float32, device=self.device)
        self.ZHAT = self._e(B * hz * hz, N)
        ops.eb_likelihood(eb, self.Z, B, N, hz * hz, noise=self.z_noise, lik=self.ZLIK, zhat=self.ZHAT,
                          table=torch.empty((N, 59), dtype=torch.float32, device=self.device))

        # ---- h_s (MCM.py:747-748): mean straight into the first M columns of LMS = [latent_means | y_hat slots]
        # h_s_scale into the first M columns of LS, rows 2M apart like LMS and one [Mp][2M] block after it: the mean
        # and scale stacks of a slice then read their inputs with one layout, Mp * 2M elements apart, and run as one
        # 2-problem launch per layer (_group_fwd).  Only LMS is zeroed (the y_hat slots not written yet)
        self.LMS, self.LS = self._e(2, self.Mp, 2 * M).unbind(0)
        self.LMS.zero_()
        self.hs_mean = self._h_s_fwd(m.h_s_mean, self.LMS, 2 * M)
        self.hs_scale = self._h_s_fwd(m.h_s_scale, self.LS, 2 * M)

        # ---- slice loop (MCM.py:751-787)
        self._slices_fwd()

        # ---- g_s (MCM.py:790-792)
        x = self.YH
        self.gs = []
        gs = [l for l in m.g_s if isinstance(l, nn.ConvTranspose2d)]
        for j, l in enumerate(gs):
            cout = l.out_channels
            h = self._e(self.Mp, cout)
            if j < len(gs) - 1:
                pre = self._e(self.Mp, cout)
                T.linear_pre(x, W.t(l.weight), l.bias.detach(), dt, ACT_GELU, h, pre)
            else:
                pre = None
                ops.linear(x, W.t(l.weight), l.bias.detach(), dt, out=h)
            self.gs.append((x, pre))
            x = h
        self.gs_out = x

    def dec_fwd(self, x, tokens=False):
        """forward_decoder (MCM.py:636-688) of x [B*K, E] (compute dtype) under self.shuf: embed + unshuffle (+ the
        off-by-one cls), blocks, norm, then decoder_pred fused with unpatchify -> x_hat f32 [B, C, H, W], or
        (tokens) as a plain linear -> preds f32 [B*L, p*p*C] in the reference's (py, px, c) column order"""
        m, dt, B, W = self.m, self.dtype, self.batch, self.w
        K, P, shuf = m.num_keep_patches, self.P, self.shuf
        Td = self.L + 1
        self.dec_gen += 1
        self.gs_out = x
        Dd, L = m.decoder_embed_dim, self.L
        pos_d = m.decoder_pos_embed.detach()
        dec = torch.empty((B * Td, Dd), dtype=torch.float32, device=self.device)
        ops.decoder_embed(x, W.nt(m.decoder_embed.weight), m.decoder_embed.bias.detach(), pos_d, shuf, dec, B, K, L,
                          dt)
        ops.mask_rows(dec, m.mask_token.detach(), pos_d, shuf, B, L, K, Dd)
        self.dec = []
        for blk in m.decoder_blocks:
            dec = self._block_fwd(blk, dec, B, Td, store=self.dec)
        self.dec_last = dec
        self.dn = ops.layernorm(dec, m.decoder_norm.weight, m.decoder_norm.bias, m.decoder_norm.eps, dt, rows=B * L,
                                row_group=L, group_stride=Td, row_offset=1)
        if tokens:
            return ops.linear(self.dn, W.nt(m.decoder_pred.weight), m.decoder_pred.bias.detach(), dt,
                              out_dtype=torch.float32)
        x_hat = torch.empty((B, m.encoder_embed.proj.in_channels, self.img, self.img), dtype=torch.float32,
                            device=self.device)
        ops.decoder_pred(self.dn, W.nt(m.decoder_pred.weight), m.decoder_pred.bias.detach(), x_hat, B, L, P, dt)
        return x_hat

    def _h_s_fwd(self, seq, out_final, ld_final):
        dt, W, B = self.dtype, self.w, self.batch
        x, cin, H = self.ZHAT, self.m.hyperprior_depth, self.hz
        saved = []
        layers = _hs_layers(seq)
        for j, (c, pshuf) in enumerate(layers):
            last = j == len(layers) - 1
            cout = c.out_channels
            if last:
                out, pre, ldo = out_final, None, ld_final
            else:
                Ho = 2 * H if pshuf else H
                co = cout // 4 if pshuf else cout
                out, pre, ldo = self._e(B * Ho * Ho, co), self._e(B * Ho * Ho, co), co
            ops.conv3x3(x, cin, cin, B, H, H, W.conv(c.weight), c.bias.detach(), out, ldo, cout, dt,
                        act=ACT_NONE if last else ACT_GELU, pixel_shuffle=pshuf, pre=pre, ldp=ldo)
            saved.append((x, cin, H, pshuf, pre))
            if pshuf:
                H, cin = 2 * H, cout // 4
            else:
                cin = cout
            x = out
        return saved

    USE_LIC_STACK = True  # test hook: False runs the per-layer conv launches in the bf16 training forward too
    USE_LIC_LATENT = True  # False: the latent partial sums as two implicit-GEMM conv launches
    USE_LIC_STACK_BWD = True  # False: the slice stacks' data gradients as one conv launch per layer
    FUSE_FIRST_DGRAD = True   # the serial slices' first-layer input gradients inside the fused chain (routed)
    _fused_bwd = False

    def _fused_ok(self):
        m = self.m
        return (self.dtype == torch.bfloat16 and self.USE_LIC_STACK and self.sw % 8 == 0 and m.num_slices > self.ms
                and ops.lic_stack_fits(self.g, self.sw * (self.ms + 1), self.mid))

    def _slices_fwd_fused(self):
        """the slice loop on the fused stacks (lic_stack.hip), as the inference forward runs it (mcm.py _slices), with
        every layer's pre-activation and GELU output kept for the backward (tmae_lic_stack_args.sv_*):
          * the latent-channel parts of every slice's first convs (mean + lrp on latent_means, scale on latent_scales)
            as two conv launches into the partial-sum buffer P, added by each stack's layer-0 epilogue;
          * slices 0..ms-1: ONE launch each -- the mean stack's workgroups go on with the slice's lrp stack, the scale
            stack beside them; their Gaussian likelihoods in one launch after the loop;
          * slices ms..S-1 batched: one launch for their 2 x nbs mean / scale stacks, the likelihoods, one for their
            lrp stacks.
        Weights are packed in fragment order by the per-step relayout (relayout mode 3).  Returns nothing; fills
        self.sl with the records _slices_bwd reads (same shapes as _group_fwd's)."""
        m, dt, W, B, g = self.m, self.dtype, self.w, self.batch, self.g
        M, S, sw, ms, Mp, HW = m.latent_depth, m.num_slices, self.sw, self.ms, self.Mp, g * g
        mid = self.mid
        c0, nl = mid[0], len(mid)
        esz, e4 = self.LMS.element_size(), 4
        lms = self.LMS.data_ptr()
        cm, cs, cl = self.cm, self.cs, self.cl
        self.YPT = self._e(Mp, M)
        self.YPRE = torch.empty((Mp, M), dtype=torch.float32, device=self.device)
        self.YH = self._e(Mp, M)
        self.YLIK = torch.empty((B, M, g, g), dtype=torch.float32, device=self.device)
        # ---- latent-channel partial sums P = [mean (S c0) | lrp (S c0) | scale (S c0)] (no bias: layer 0 adds it)
        Pw = 3 * S * c0
        off_mean, off_lrp, off_scale = 0, S * c0, 2 * S * c0
        P = torch.empty((Mp, Pw), dtype=torch.float32, device=self.device)
        self._P = P
        pb = P.data_ptr()
        if self.USE_LIC_LATENT and ops.lic_latent_fits(g, M) and c0 % 32 == 0:
            # one tmae_lic_latent launch: a block per stack's latent part, [mean | lrp | scale] x slices
            w_lat = W.packed([c[0].weight for c in cm] + [c[0].weight for c in cl] + [c[0].weight for c in cs],
                             ("lic", 0, M))
            nfs = c0 // 16
            ops.lic_latent(B, g, [self.LMS, self.LMS, self.LS], 2 * M, M, w_lat, nfs, w_lat[0].numel(),
                           [0, S * nfs, 2 * S * nfs], 0, S * nfs, pb, Pw)
        else:
            w_ml = W.packed([c[0].weight for c in cm] + [c[0].weight for c in cl], ("conv_lat", M))
            w_s = W.packed([c[0].weight for c in cs], ("conv_lat", M))
            ops.conv3x3(self.LMS, M, 2 * M, B, g, g, w_ml, None, pb, Pw, S * c0, dt, y_f32=True, nb=(1, 2),
                        strides={"w": (0, S * w_ml[0].numel()), "y": (0, S * c0)})
            ops.conv3x3(self.LS, M, 2 * M, B, g, g, w_s, None, pb + off_scale * 4, Pw, S * c0, dt, y_f32=True)

        def stack_weights(convs_per_problem, lo, n0):
            """per layer: packed weights of the problems (layer 0: input channels [lo, lo + n0)) and biases"""
            ws, bs = [], []
            for l in range(nl):
                kind = ("lic", lo, n0) if l == 0 else ("lic", 0, mid[l - 1])
                ws.append(W.packed([c[l].weight for c in convs_per_problem], kind))
                bs.append(W.packed([c[l].bias for c in convs_per_problem], "bias"))
            return ws, bs

        def save_bufs(lead):
            """pre / act per non-last layer, [*lead][Mp][cout] bf16"""
            return [(self._e(*lead, Mp, c), self._e(*lead, Mp, c)) for c in mid[:-1]]

        self.sl = [None] * S
        # ---- slices 0..ms-1: chained launches
        MS = torch.empty((2, ms, Mp, sw), dtype=torch.float32, device=self.device)
        for i in range(ms):
            ny = sw * i
            ws, bs = stack_weights([cm[i], cs[i]], M, ny)
            lw, lb = stack_weights([cl[i]], M, ny + sw)
            st = {"a": (off_scale - off_mean, c0), "y": (ms * Mp * sw, 0)}
            for l in range(nl):
                st[f"w{l}"] = (ws[l][0].numel(), 0)
                st[f"b{l}"] = (bs[l][0].numel(), 0)
            sv_ms = save_bufs((2,))
            sv_l = save_bufs(())
            t = torch.empty((Mp, sw), dtype=torch.float32, device=self.device)
            ch = dict(w=[w[0] for w in lw], b=[b[0] for b in lb], couts=mid, x1=lms + M * esz, c1=ny, ld1=2 * M,
                      y=self.Y32.data_ptr() + i * sw * e4, ldy=M, add=pb + (off_lrp + i * c0) * e4, ld_add=Pw,
                      ypre=self.YPRE.data_ptr() + i * sw * e4, ld_ypre=M, out=self.YH.data_ptr() + i * sw * esz,
                      ld_out=M, out2=lms + (M + i * sw) * esz, ld_out2=2 * M,
                      q=self.qd if self.qmd is None else None, qm=self.qmd)
            save = {"layers": [(pre, act, (Mp * c, 0)) for (act, pre), c in zip(sv_ms, mid)],
                    "chain": [(pre, act, 0) for act, pre in sv_l], "chain_t": t}
            ops.lic_stack(B, g, lms + M * esz, ny, 2 * M, [w[0] for w in ws], [b[0] for b in bs], mid, MS[0, i], sw,
                          True, addend=pb + (off_mean + i * c0) * e4, ld_add=Pw, nb=(2, 1), strides=st, chain=ch,
                          save=save)
            self.sl[i] = {"mean": [(a[0], p_[0]) for a, p_ in sv_ms] + [MS[0, i]],
                          "scale": [(a[1], p_[1]) for a, p_ in sv_ms] + [MS[1, i]],
                          "lrp": list(sv_l) + [t]}
        # Gaussian likelihoods + y_hat_pre (YPT, the backward's lrp input; YPRE) of the chained slices
        self._gc_slices(0, MS[0], MS[1], ms)
        # ---- slices ms..S-1 batched on the support slots 0..ms-1
        i0, nbs = ms, S - ms
        bs_ = range(i0, S)
        ws, bsb = stack_weights([cm[i] for i in bs_] + [cs[i] for i in bs_], M, sw * ms)
        st = {"a": (off_scale - off_mean, c0), "y": (nbs * Mp * sw, Mp * sw)}
        for l in range(nl):
            st[f"w{l}"] = (nbs * ws[l][0].numel(), ws[l][0].numel())
            st[f"b{l}"] = (nbs * bsb[l][0].numel(), bsb[l][0].numel())
        MSB = torch.empty((2, nbs, Mp, sw), dtype=torch.float32, device=self.device)
        sv_b = save_bufs((2, nbs))
        ops.lic_stack(B, g, lms + M * esz, sw * ms, 2 * M, [w[0] for w in ws], [b[0] for b in bsb], mid, MSB, sw, True,
                      addend=pb + (off_mean + i0 * c0) * e4, ld_add=Pw, nb=(2, nbs), strides=st,
                      save={"layers": [(pre, act, (nbs * Mp * c, Mp * c)) for (act, pre), c in zip(sv_b, mid)]})
        self._gc_slices(i0, MSB[0], MSB[1], nbs)
        lw, lb = stack_weights([cl[i] for i in bs_], M, sw * ms + sw)
        st = {"a": (0, c0), "y": (0, sw), "src": (0, sw), "x2": (0, sw)}
        for l in range(nl):
            st[f"w{l}"] = (0, lw[l][0].numel())
            st[f"b{l}"] = (0, lb[l][0].numel())
        sv_lb = save_bufs((nbs,))
        tb = torch.empty((nbs, Mp, sw), dtype=torch.float32, device=self.device)
        ops.lic_stack(B, g, lms + M * esz, sw * ms, 2 * M, [w[0] for w in lw], [b[0] for b in lb], mid,
                      self.YH.data_ptr() + i0 * sw * esz, M, False, x2=self.YPT.data_ptr() + i0 * sw * esz, c2=sw,
                      ld2=M, addend=pb + (off_lrp + i0 * c0) * e4, ld_add=Pw,
                      lrp_src=self.YPRE.data_ptr() + i0 * sw * e4, ld_src=M, nb=(1, nbs), strides=st,
                      save={"layers": [(pre, act, (0, Mp * c)) for (act, pre), c in zip(sv_lb, mid)], "t": tb,
                            "t_s": (0, Mp * sw)})
        for j, i in enumerate(bs_):
            self.sl[i] = {"mean": [(a[0, j], p_[0, j]) for a, p_ in sv_b] + [MSB[0, j]],
                          "scale": [(a[1, j], p_[1, j]) for a, p_ in sv_b] + [MSB[1, j]],
                          "lrp": [(a[j], p_[j]) for a, p_ in sv_lb] + [tb[j]]}

    def _gc_slices(self, i0, mu, sigma, nbs):
        """GaussianConditional + quantize_ste of slices i0..i0+nbs-1 (mu / sigma blocks Mp * sw apart) -> YLIK, YPT,
        YPRE; at the forward's quantiser step when it has one"""
        M, sw, Mp, HW = self.m.latent_depth, self.sw, self.Mp, self.g * self.g
        args = (self.Y32, M, i0 * sw, mu, sigma, Mp * sw, sw, self.y_noise, self.YLIK, M, self.YPT, self.dtype, M,
                self.YPRE, M, self.batch, HW, nbs, sw)
        if self.qmd is not None:
            ops.gc_slices_fwd_qm(*args, self.scale_bound, self.qmd)
        elif self.qd is None:
            ops.gc_slices(*args)
        else:
            ops.gc_slices_fwd_q(*args, self.scale_bound, self.qd)

    def _gc_bwd(self, *args):
        """T.gc_bwd, at the forward's quantiser step, or its map of steps, when it had one"""
        if self.qmd is not None:
            T.gc_bwd_qm(*args, self.scale_bound, self.qmd)
        elif self.qd is None:
            T.gc_bwd(*args)
        else:
            T.gc_bwd_q(*args, self.scale_bound, self.qd)

    def _pack(self, stacks, l, kind, what="weight"):
        """layer l's `kind` copies of the weights (or what="bias") of `stacks` (conv lists: consecutive stacks of one
        launch group) as rows of the group's pack -> (the first stack's row, the element stride to the next one's)"""
        grp, r = self._lgroup[id(stacks[0][0])]
        if any(grp[r + j] is not c for j, c in enumerate(stacks)):
            raise RuntimeError("slice stacks of one launch must be consecutive stacks of one launch group")
        pack = self.w.packed([getattr(c[l], what) for c in grp], kind)
        return pack[r], pack[0].numel()

    def _slices_fwd(self):
        # the fused stack backward reads what the fused forward saved (bf16 pre-activations, [problems][Mp][c])
        self._fused_bwd = self._fused_ok() and self.USE_LIC_STACK_BWD
        if self._fused_ok():
            return self._slices_fwd_fused()
        m, g, Mp = self.m, self.g, self.Mp
        M = m.latent_depth
        self.YPT = self._e(Mp, M)
        self.YPRE = torch.empty((Mp, M), dtype=torch.float32, device=self.device)
        self.YH = self._e(Mp, M)
        self.YLIK = torch.empty((self.batch, M, g, g), dtype=torch.float32, device=self.device)
        self.sl = []
        for i0, nbs in self.slice_groups:
            self.sl += self._group_fwd(i0, nbs, min(i0, self.ms))

    def _group_fwd(self, i0, nbs, k):
        """slices i0..i0+nbs-1 on the support slots 0..k-1 (MCM.py:761-787), one conv launch per layer: their mean and
        scale stacks as 2 x nbs problems (problem (0, j) reads [latent_means | slots] from LMS, (1, j) [latent_scales |
        the same slots] from LS), the Gaussian likelihoods of the nbs slices, their lrp stacks as nbs problems.  Every
        per-problem stride is a shape product: weights and biases come from the launch group's packs, outputs are
        [2][nbs][Mp][cout] / [nbs][Mp][cout].  Returns one saved-activation record per slice,
        {"mean": [(act, pre) x 4, out], "scale": the same, "lrp": [(act, pre) x 4, t]}"""
        m, dt, B, g, Mp = self.m, self.dtype, self.batch, self.g, self.Mp
        M, sw, HW = m.latent_depth, self.sw, g * g
        esz = self.LMS.element_size()
        sl = range(i0, i0 + nbs)
        cms = [self.cm[i] for i in sl] + [self.cs[i] for i in sl]
        cl = [self.cl[i] for i in sl]
        recs = [{"mean": [], "scale": [], "lrp": []} for _ in sl]
        nl = len(cl[0])
        x1, c1, ld1, x1s = self.LMS, M, 2 * M, (Mp * 2 * M, 0)
        x2, c2 = (self.LMS.data_ptr() + M * esz if k else None), sw * k
        for l in range(nl):
            cout = cms[0][l].out_channels
            (w, ws), (b, bs) = self._pack(cms, l, "conv"), self._pack(cms, l, "bias", "bias")
            st = {"x1": x1s, "w": (nbs * ws, ws), "b": (nbs * bs, bs), "y": (nbs * Mp * cout, Mp * cout)}
            if l < nl - 1:
                act, pre = self._e(2, nbs, Mp, cout), self._e(2, nbs, Mp, cout)
                st["pre"] = st["y"]
                ops.conv3x3(x1, c1, ld1, B, g, g, w, b, act, cout, cout, dt, act=ACT_GELU, x2=x2, c2=c2, ld2=2 * M,
                            pre=pre, ldp=cout, nb=(2, nbs), strides=st)
                for j in range(nbs):
                    recs[j]["mean"].append((act[0, j], pre[0, j]))
                    recs[j]["scale"].append((act[1, j], pre[1, j]))
                x1, c1, ld1, x1s, x2, c2 = act, cout, cout, st["y"], None, 0
            else:
                mus = torch.empty((2, nbs, Mp, cout), dtype=torch.float32, device=self.device)
                ops.conv3x3(x1, c1, ld1, B, g, g, w, b, mus, cout, cout, dt, y_f32=True, x2=x2, c2=c2, ld2=2 * M,
                            nb=(2, nbs), strides=st)
                for j in range(nbs):
                    recs[j]["mean"].append(mus[0, j])
                    recs[j]["scale"].append(mus[1, j])
        # GaussianConditional + quantize_ste of the nbs slices (mu / sigma blocks Mp * sw apart)
        self._gc_slices(i0, mus[0], mus[1], nbs)
        # lrp stacks: input [latent_means | slots 0..k-1] (shared) + this slice's y_hat_pre (x2, sw apart)
        x1, c1, ld1, x1s = self.LMS, M + sw * k, 2 * M, (0, 0)
        x2, c2, ld2, x2s = self.YPT.data_ptr() + i0 * sw * esz, sw, M, (0, sw)
        for l in range(nl):
            cout = cl[0][l].out_channels
            (w, ws), (b, bs) = self._pack(cl, l, "conv"), self._pack(cl, l, "bias", "bias")
            st = {"x1": x1s, "x2": x2s, "w": (0, ws), "b": (0, bs)}
            if l < nl - 1:
                act, pre = self._e(nbs, Mp, cout), self._e(nbs, Mp, cout)
                st["y"] = st["pre"] = (0, Mp * cout)
                ops.conv3x3(x1, c1, ld1, B, g, g, w, b, act, cout, cout, dt, act=ACT_GELU, x2=x2, c2=c2, ld2=ld2,
                            pre=pre, ldp=cout, nb=(1, nbs), strides=st)
                for j in range(nbs):
                    recs[j]["lrp"].append((act[j], pre[j]))
                x1, c1, ld1, x1s, x2, c2, ld2, x2s = act, cout, cout, st["y"], None, 0, 0, (0, 0)
            else:
                # y_hat = y_hat_pre + 0.5 tanh(t) into YH (slice j at channels (i0 + j) sw) and, for a slice below ms,
                # into its support slot of LMS; t kept in f32
                t = torch.empty((nbs, Mp, cout), dtype=torch.float32, device=self.device)
                st.update({"y": (0, sw), "src": (0, sw), "y2": (0, sw), "pre": (0, Mp * cout)})
                ops.conv3x3(x1, c1, ld1, B, g, g, w, b, self.YH.data_ptr() + i0 * sw * esz, M, cout, dt,
                            y_f32=(dt == torch.float32), lrp_src=self.YPRE.data_ptr() + i0 * sw * 4, ld_src=M,
                            y2=(self.LMS.data_ptr() + (M + i0 * sw) * esz) if i0 < self.ms else None, ldy2=2 * M,
                            pre=t, ldp=cout, nb=(1, nbs), strides=st)
                for j in range(nbs):
                    recs[j]["lrp"].append(t[j])
        return recs

    # ------------------------------------------------------------------ backward
    def backward(self, dxhat, dylik, dzlik, gflat, sync=None):
        """full reverse pass; every parameter's gradient lands in gflat (views per self.offsets)"""
        m, dt, W, B = self.m, self.dtype, self.w, self.batch
        P, M, N, hz, L = self.P, m.latent_depth, m.hyperprior_depth, self.hz, self.L
        Mp = self.Mp
        self.bwd_begin(gflat, sync)
        G = self.grad
        dxhat = dxhat.float().contiguous() if dxhat is not None else torch.zeros_like(self.imgs)
        dylik = dylik.float().contiguous() if dylik is not None else None
        dzlik = dzlik.float().contiguous() if dzlik is not None else None

        # ---- unpatchify (MCM.py:797), decoder
        dP = T.patchify(dxhat, self._e(B * L, dxhat.shape[1] * P * P), P, dt)
        d = self.dec_bwd(dP)

        # ---- g_s
        gs = [l for l in m.g_s if isinstance(l, nn.ConvTranspose2d)]
        for j in reversed(range(len(gs))):
            l = gs[j]
            x, _ = self.gs[j]
            pre_prev = self.gs[j - 1][1] if j > 0 else None
            cin, cout = l.in_channels, l.out_channels
            self._wg(d, x, cout, cin, Mp, G(l.weight), dt, layout="dense_t", bias=G(l.bias))
            dx = self._e(Mp, cin)
            T.dgrad_linear(d, W.raw(l.weight), Mp, cout, cin, dt, out=dx, pre=pre_prev)
            d = dx
        dYH = d
        self._ready(gs[0].bias)

        # ---- slice loop
        DY, dLM, dLS = self._slices_bwd(dYH, dylik)

        # ---- h_s
        dZH = self._z(B * hz * hz, N)
        self._h_s_bwd(m.h_s_mean, self.hs_mean, dLM, dZH)
        self._h_s_bwd(m.h_s_scale, self.hs_scale, dLS, dZH)
        self._ready(_hs_convs(m.h_s_scale)[0].bias)

        # ---- entropy bottleneck (MCM.py:741-744)
        eb = m.entropy_bottleneck
        dZ = torch.empty((B * hz * hz, N), dtype=torch.float32, device=self.device)
        T.eb_bwd(ops._eb_params(eb), self.Z, self.z_noise, dzlik, dZH, dZ, B, N, hz * hz, self._eb_grads(eb))
        G(eb.quantiles).zero_()
        self._ready(eb.quantiles)

        # ---- h_a (MCM.py:739): dZ -> DY (accumulated with the slice loop's y gradient)
        d = self._cast(dZ)
        convs = _convs(m.h_a)
        for j in reversed(range(len(convs))):
            c = convs[j]
            x, cin, H, s, _ = self.ha[j]
            pre_prev = self.ha[j - 1][4] if j > 0 else None
            cout = c.out_channels
            Ho = (H + 2 - 3) // s + 1
            self._wg(d, x, cout, 9 * cin, B * Ho * Ho, G(c.weight), dt,
                    conv=dict(c1=cin, H=H, W=H, stride=s, cin=cin), layout="conv", bias=G(c.bias))
            if j > 0:
                dx = self._e(B * H * H, cin)
                T.conv_dgrad(d, W.conv_dg(c.weight), B, H, H, s, cout, cin, dt, out=dx, pre=pre_prev)
                d = dx
            else:
                T.conv_dgrad(d, W.conv_dg(c.weight), B, H, H, s, cout, cin, dt, routes=[(DY, M, M)])
        self._ready(convs[0].bias)

        # ---- g_a (MCM.py:735)
        d = self._cast(DY)
        ga = [l for l in m.g_a if isinstance(l, nn.Conv2d)]
        for j in reversed(range(len(ga))):
            l = ga[j]
            x, _ = self.ga[j]
            pre_prev = self.ga[j - 1][1] if j > 0 else None
            cin, cout = l.in_channels, l.out_channels
            self._wg(d, x, cout, cin, Mp, G(l.weight), dt, bias=G(l.bias))
            if j > 0:
                dx = self._e(Mp, cin)
                T.dgrad_linear(d, W.t(l.weight), Mp, cout, cin, dt, out=dx, pre=pre_prev)
            else:
                dx = torch.empty((Mp, cin), dtype=torch.float32, device=self.device)
                T.dgrad_linear(d, W.t(l.weight), Mp, cout, cin, dt, out=dx)
            d = dx
        self._ready(ga[0].bias)
        self.enc_bwd(d)
        self._side_join()

    def enc_bwd(self, denc):
        """encoder backward (MCM.py:590-634) from denc f32 [B*K, E], the gradient of encoder_norm's output without
        the cls rows: every encoder parameter's gradient"""
        m, dt, B = self.m, self.dtype, self.batch
        E, K = m.encoder_embed_dim, m.num_keep_patches
        Te = K + 1
        G = self.grad
        # ---- encoder norm (drops cls, MCM.py:631-632) + blocks
        dt_tok = self._z(B * Te, E)
        dt_op = dt_tok if dt == torch.float32 else self._z(B * Te, E, dtype=dt)
        T.layernorm_bwd(self.tok_last, m.encoder_norm.weight, denc, dt_tok, B * K, E, m.encoder_norm.eps,
                        G(m.encoder_norm.weight), G(m.encoder_norm.bias), dxop=None if dt == torch.float32 else dt_op,
                        row_group=K, group_stride=Te, row_offset=1)
        self._ready(m.encoder_norm.bias)
        for blk, s in zip(reversed(m.encoder_blocks), reversed(self.enc)):
            dt_tok, dt_op = self._block_bwd(blk, s, dt_tok, dt_op, B, Te)
            self._ready(_block_params(blk)[-1])

        # ---- patch embed + cls token (MCM.py:615-626)
        pw = m.encoder_embed.proj.weight
        self._wg(dt_op, self.patches, E, pw[0].numel(), B * K, G(pw), dt, lda=E, a_remap=(K, Te, 1))
        T.colsum(dt_tok, B * K, E, G(m.encoder_embed.proj.bias), row_group=K, group_stride=Te, row_offset=1)
        T.colsum(dt_tok, B, E, G(m.cls_token).view(-1), row_group=1, group_stride=Te, row_offset=0)
        self._ready(m.cls_token)

    def bwd_begin(self, gflat, sync=None):
        self.gflat, self.sync = gflat, sync
        if sync is not None:
            sync.attach(gflat)
        self._side_begin()

    def dec_bwd(self, dP, out_f32=False):
        """decoder backward (MCM.py:636-688) from dP [B*L, p*p*C] (compute dtype), the gradient of decoder_pred's
        token-layout output: every decoder parameter's gradient; -> the gradient of the decoder's input tokens
        [B*K, E] in the compute dtype (g_s goes on with it) or, out_f32, in f32"""
        m, dt, W, B = self.m, self.dtype, self.w, self.batch
        E, K, L, Dd = m.encoder_embed_dim, m.num_keep_patches, self.L, m.decoder_embed_dim
        Td, Mp = L + 1, self.Mp
        G = self.grad
        # ---- decoder_pred (MCM.py:683-686)
        npred = dP.shape[1]
        self._wg(dP, self.dn, npred, Dd, B * L, G(m.decoder_pred.weight), dt, bias=G(m.decoder_pred.bias))
        ddn = torch.empty((B * L, Dd), dtype=torch.float32, device=self.device)
        T.dgrad_linear(dP, W.t(m.decoder_pred.weight), B * L, npred, Dd, dt, out=ddn)
        ddec = self._z(B * Td, Dd)
        ddec_op = ddec if dt == torch.float32 else self._z(B * Td, Dd, dtype=dt)
        T.layernorm_bwd(self.dec_last, m.decoder_norm.weight, ddn, ddec, B * L, Dd, m.decoder_norm.eps,
                        G(m.decoder_norm.weight), G(m.decoder_norm.bias), dxop=None if dt == torch.float32 else ddec_op,
                        row_group=L, group_stride=Td, row_offset=1)
        self._ready(m.decoder_norm.bias)
        for blk, s in zip(reversed(m.decoder_blocks), reversed(self.dec)):
            ddec, ddec_op = self._block_bwd(blk, s, ddec, ddec_op, B, Td)
            self._ready(_block_params(blk)[-1])

        # ---- decoder_embed + mask tokens (MCM.py:657-675)
        dtok = self._e(Mp, Dd)
        T.decoder_embed_bwd_gather(ddec, self.shuf, dtok, B, K, L, Dd, dt, dmask=G(m.mask_token).view(-1))
        self._wg(dtok, self.gs_out, Dd, E, Mp, G(m.decoder_embed.weight), dt, bias=G(m.decoder_embed.bias))
        d = torch.empty((Mp, E), dtype=torch.float32, device=self.device) if out_f32 else self._e(Mp, E)
        T.dgrad_linear(dtok, W.t(m.decoder_embed.weight), Mp, Dd, E, dt, out=d)
        self._ready(m.mask_token)
        return d

    def _eb_grads(self, eb):
        from ._lib import EBParams

        g = EBParams()
        for i in range(5):
            g.matrix[i] = self.grad(getattr(eb, f"_matrix{i}")).data_ptr()
            g.bias[i] = self.grad(getattr(eb, f"_bias{i}")).data_ptr()
            if i < 4:
                g.factor[i] = self.grad(getattr(eb, f"_factor{i}")).data_ptr()
        g.quantiles = self.grad(eb.quantiles).data_ptr()
        return g

    def _h_s_bwd(self, seq, saved, dout32, dZH):
        dt, W, G, B = self.dtype, self.w, self.grad, self.batch
        layers = _hs_layers(seq)
        d = self._cast(dout32)
        for j in reversed(range(len(layers))):
            c, pshuf = layers[j]
            x, cin, H, _, _ = saved[j]
            cout = c.out_channels
            self._wg(d, x, cout, 9 * cin, B * H * H, G(c.weight), dt, conv=dict(c1=cin, H=H, W=H, cin=cin),
                    layout="conv", bias=G(c.bias))
            if j == 0:
                T.conv_dgrad(d, W.conv_dg(c.weight), B, H, H, 1, cout, cin, dt, routes=[(dZH, cin, cin)])
                break
            _, _, Hp, pshuf_prev, pre_prev = saved[j - 1]
            dx = self._e(B * H * H, cin)
            if pshuf_prev:
                # input of this conv = GELU(PixelShuffle(conv_{j-1})): plain data gradient, then unshuffle * gelu'
                T.conv_dgrad(d, W.conv_dg(c.weight), B, H, H, 1, cout, cin, dt, out=dx)
                c4 = cin * 4
                dpre = self._e(B * Hp * Hp, c4)
                T.unshuffle_bwd(dx, cin, pre_prev, cin, dpre, B, Hp, Hp, c4, dt, dy_f32=(dt == torch.float32))
                d = dpre
            else:
                T.conv_dgrad(d, W.conv_dg(c.weight), B, H, H, 1, cout, cin, dt, out=dx, pre=pre_prev)
                d = dx

    def _slices_bwd(self, dYH, dylik):
        m, dt, B, g = self.m, self.dtype, self.batch, self.g
        M, S, sw, ms, Mp, HW = m.latent_depth, m.num_slices, self.sw, self.ms, self.Mp, g * g
        esz = self.LMS.element_size()
        lms = self.LMS.data_ptr()
        DY = self._z(Mp, M)
        dLM, dLS = self._z(2, Mp, M).unbind(0)
        # The scale stack of a slice depends on nothing the mean stack writes: eager on a GPU it runs on its own
        # stream beside the mean stack, its support-channel gradients in their own buffer (dSUP2, added where slice
        # j's lrp backward reads column block j), so the two data-gradient chains never touch the same accumulator.
        # Not under graph capture: HIP's graph executor ran that topology 3.4 ms slower per step (31.4 -> 34.8 ms;
        # eager 31.9 -> 31.4), and 6.5 ms slower with joins only where slices <= 5 read dSUP2 (31.9 -> 38.4), so a
        # captured step keeps both stacks on the compute stream, their layers 4..1 as 2-problem data-gradient
        # launches (same sums either way).  dSUP2 also without the stream: the same sums in the same order.
        dSUP, dSUP2 = self._z(2, Mp, M).unbind(0)
        conc = self._side is not None and not torch.cuda.is_current_stream_capturing()
        if conc and "_scale_stream" not in self.__dict__:
            self._scale_stream = torch.cuda.Stream(device=self.device)
        main = torch.cuda.current_stream(self.device) if conc else None
        joined = None
        deferred = []  # eager only: (slice, mean stack's, scale stack's layer 4..1 weight gradients)
        GS = torch.empty((Mp, M), dtype=torch.float32, device=self.device)
        # slices nser..S-1 ran as one group in the forward (they condition on the fixed support slots 0..ms-1): their
        # backward is batched too, every data gradient of layers 4..1 one launch for all of them
        if self.nser < S:
            self._batched_bwd(self.nser, S - self.nser, dYH, dylik, DY, dLM, dLS, dSUP, dSUP2, GS)
        for i in reversed(range(self.nser)):
            # fresh per slice: the side stream's weight gradients of slice i + 1 may still read the last ones
            dT = self._e(Mp, sw)
            dMU, dSG = self._e(2, Mp, sw).unbind(0)
            k = i  # support slots of a serial slice
            cin_m = M + sw * k
            rec = self.sl[i]
            gs_i = GS.data_ptr() + i * sw * 4
            if joined is not None and i < ms:  # later slices' scale stacks wrote dSUP2's block i (read below)
                main.wait_event(joined)
                joined = None
            # y_hat = y_hat_pre + 0.5 tanh(t)   (MCM.py:782-783)
            T.lrp_bwd(rec["lrp"][-1], sw, dT, sw, Mp, sw, dt, g32=(dSUP.data_ptr() + i * sw * 4) if i < ms else None,
                      ld32=M, g16=dYH.data_ptr() + i * sw * esz, ld16=M, gsum=gs_i, ldgs=M,
                      g32b=(dSUP2.data_ptr() + i * sw * 4) if i < ms else None, ld32b=M)
            self._stack_bwd([(self.cl[i], rec["lrp"], dT,
                              (self.LMS, cin_m, 2 * M, self.YPT.data_ptr() + i * sw * esz, sw, M),
                              [(dLM, M, M), (dSUP, M, sw * k), (gs_i, M, sw)])])
            # GaussianConditional + quantize_ste (MCM.py:771-776)
            self._gc_bwd(self.Y32, M, i * sw, rec["mean"][-1], rec["scale"][-1], sw, self.y_noise, M, dylik, GS, M, DY,
                         M, dMU, dSG, sw, B, HW, sw, dt)
            scale = (self.cs[i], rec["scale"], dSG, (self.LS, M, 2 * M, lms + M * esz if k else None, sw * k, 2 * M),
                     [(dLS, M, M), (dSUP2, M, sw * k)])
            mean = (self.cm[i], rec["mean"], dMU, (self.LMS, cin_m, 2 * M, None, 0, 0),
                    [(dLM, M, M), (dSUP, M, sw * k)])
            if not conc:
                # one stream: layers 4..1 of both stacks as 2-problem data-gradient launches
                self._stack_bwd([mean, scale])
                self._ready(self.cs[i][0].bias)
                continue
            # eager: the scale stack on its own stream, the mean stack first on the compute stream (one-problem
            # launches on rows 0 and 1 of the pair's weight packs).  Their layers 4..1 weight gradients wait for the
            # final join and then run as the same 2-problem launches a captured step issues, so eager and graphed
            # steps sum them with one split plan; the DP hand-offs of these slices follow them.
            fork = torch.cuda.Event()
            fork.record(main)
            im, is_ = [], []
            built = self.w.builds
            self._stack_bwd([mean], defer=im)
            ss = self._scale_stream
            ss.wait_event(fork)
            if self.w.builds != built:  # (first step) the pair's packs were just built on this stream, row 1 too
                ss.wait_stream(main)
            with torch.cuda.stream(ss):
                self._stack_bwd([scale], defer=is_)
            joined = torch.cuda.Event()
            joined.record(ss)
            self._keep.append(dSG)  # read on the scale stream; freed after the backward's join
            deferred.append((i, im, is_))
        if joined is not None:
            main.wait_event(joined)
        for i, im, is_ in deferred:
            for (ia, shp), (ib, _) in zip(im, is_):
                self._wg_many(ia + ib, *shp, layout="conv")
            self._wg_flush()
            self._ready(self.cs[i][0].bias)
        return DY, dLM, dLS

    def _batched_bwd(self, i0, nbs, dYH, dylik, DY, dLM, dLS, dSUP, dSUP2, GS):
        """backward of the slice group i0..i0+nbs-1 (_group_fwd, nbs > 1): per slice the lrp backward, then the lrp
        stacks' layers 4..1 (_stacks_bwd), their first layers one by one (routes into the shared latent / support
        gradients, slices in descending order), the Gaussian backward per slice, then the mean and scale stacks' layers
        4..1 as 2 nbs problems and their first layers one by one (mean before scale per slice).  Weight gradients per
        problem group on the side stream, as for the serial slices."""
        m, dt, W, G, B, g = self.m, self.dtype, self.w, self.grad, self.batch, self.g
        M, sw, Mp, HW = m.latent_depth, self.sw, self.Mp, g * g
        esz = self.LMS.element_size()
        lms = self.LMS.data_ptr()
        k = self.ms
        sl = list(range(i0, i0 + nbs))
        recs = [self.sl[i] for i in sl]
        cl, cm, cs = ([c[i] for i in sl] for c in (self.cl, self.cm, self.cs))
        # ---- lrp: y_hat = y_hat_pre + 0.5 tanh(t) backward, per slice (no support gradients beyond slot ms - 1)
        dT = self._e(nbs, Mp, sw)
        for j, i in enumerate(sl):
            T.lrp_bwd(recs[j]["lrp"][-1], sw, dT[j], sw, Mp, sw, dt, g16=dYH.data_ptr() + i * sw * esz, ld16=M,
                      gsum=GS.data_ptr() + i * sw * 4, ldgs=M)
        dl, _ = self._stacks_bwd([(cl[j], recs[j]["lrp"], dT[j]) for j in range(nbs)])
        cin, cout = M + sw * k + sw, cl[0][0].out_channels
        self._wg_many([{"a": dl[j], "b": self.LMS, "x2": self.YPT.data_ptr() + i * sw * esz, "out": G(cl[j][0].weight),
                        "bias": G(cl[j][0].bias)} for j, i in enumerate(sl)],
                      cout, 9 * cin, Mp, dt, conv=dict(c1=M + sw * k, ld2=M, H=g, W=g, cin=cin), layout="conv",
                      ldb=2 * M)
        for j in reversed(range(nbs)):
            i, c = sl[j], cl[j][0]
            T.conv_dgrad(dl[j], W.conv_dg(c.weight), B, g, g, 1, cout, cin, dt,
                         routes=[(dLM, M, M), (dSUP, M, sw * k), (GS.data_ptr() + i * sw * 4, M, sw)])
        self._wg_flush()
        # ---- GaussianConditional + quantize_ste per slice -> d mu, d sigma of every problem ([mean | scale][slice])
        dMS = self._e(2, nbs, Mp, sw)
        for j, i in enumerate(sl):
            self._gc_bwd(self.Y32, M, i * sw, recs[j]["mean"][-1], recs[j]["scale"][-1], sw, self.y_noise, M, dylik, GS,
                         M, DY, M, dMS[0, j], dMS[1, j], sw, B, HW, sw, dt)
        dms, _ = self._stacks_bwd([(c[j], recs[j][key], dMS[t, j]) for t, (c, key) in enumerate(((cm, "mean"),
                                                                                                (cs, "scale")))
                                   for j in range(nbs)], groups=2)
        firsts = ((cm, (self.LMS, M + sw * k, 2 * M, None, 0, 0), [(dLM, M, M), (dSUP, M, sw * k)]),
                  (cs, (self.LS, M, 2 * M, lms + M * esz, sw * k, 2 * M), [(dLS, M, M), (dSUP2, M, sw * k)]))
        for t, (convs, first, _) in enumerate(firsts):
            x1, c1, ld1, x2, c2, ld2 = first
            cin, cout = c1 + c2, convs[0][0].out_channels
            self._wg_many([{"a": dms[t * nbs + j], "b": x1, "x2": x2, "out": G(convs[j][0].weight),
                            "bias": G(convs[j][0].bias)} for j in range(nbs)],
                          cout, 9 * cin, Mp, dt, conv=dict(c1=c1, ld2=ld2, H=g, W=g, cin=cin), layout="conv", ldb=ld1)
        for j in reversed(range(nbs)):
            for t, (convs, first, routes) in enumerate(firsts):
                c, d = convs[j][0], dms[t * nbs + j]
                cin, cout = first[1] + first[4], c.out_channels
                T.conv_dgrad(d, W.conv_dg(c.weight), B, g, g, 1, cout, cin, dt, routes=routes)
            self._wg_flush()
            self._ready(cs[j][0].bias)  # every gradient of slices >= i0 + j is final (DP hand-off per slice)

    def _stack_bwd(self, stacks, defer=None):
        """backward of a serial slice's stacks run together, stacks = [(convs, saved, dtop, first, routes)]: one (its
        lrp stack; its mean or scale stack on a stream of its own) or two (mean, scale).  Layers 4..1 by _stacks_bwd;
        then the first layers with their own input splits `first` = (x1, c1, ld1, x2, c2, ld2) and routes, one by one
        in order.  Zero-width routes (no support slices yet) stay in place: their limits still partition the channels"""
        dt, G, B, g, Mp = self.dtype, self.grad, self.batch, self.g, self.Mp
        d0, routed = self._stacks_bwd([s[:3] for s in stacks], routes=[s[4] for s in stacks], defer=defer)
        for (convs, _, _, (x1, c1, ld1, x2, c2, ld2), routes), d in zip(stacks, d0):
            c = convs[0]
            cin, cout = c1 + c2, c.out_channels
            self._wg(d, x1, cout, 9 * cin, Mp, G(c.weight), dt, ldb=ld1,
                     conv=dict(x2=x2, c1=c1, ld2=ld2, H=g, W=g, cin=cin), layout="conv", bias=G(c.bias))
            if not routed:
                T.conv_dgrad(d, self.w.conv_dg(c.weight), B, g, g, 1, cout, cin, dt, routes=routes)
        self._wg_flush()

    def _stacks_bwd(self, stacks, groups=1, routes=None, defer=None):
        """layers 4..1 of P same-shape stacks, stacks = [(convs, saved, dtop)], consecutive stacks of one launch group
        with their dtops and saved activations evenly spaced.  Data gradients: the fused chain (_fused_dgrads) when it
        applies -- with `routes` (one list per problem) and FUSE_FIRST_DGRAD it adds the first layers' input gradients
        too --, else one T.conv_dgrad per layer for the P problems on the group's packed "conv_dg" weights, outputs
        [P][Mp][cin].  Weight gradients per layer through _wg_many, one call for each of `groups` runs of P / groups
        problems, or appended to `defer` (a list) as (items, shape arguments) for the caller to issue.
        -> (the gradients w.r.t. the first layers' pre-activations, one per problem; whether the chain has added the
        first layers' input gradients)"""
        dt, G, B, g, Mp = self.dtype, self.grad, self.batch, self.g, self.Mp
        P, convs = len(stacks), [s[0] for s in stacks]
        routes = routes if self.FUSE_FIRST_DGRAD else None
        fd = self._fused_dgrads(stacks, routes)
        d = [s[2] for s in stacks]

        def even(views, what):
            s = self._stride(views)
            if s is None:
                raise RuntimeError(f"slice stack backward: the problems' {what} are not at a constant stride")
            return s

        for l in range(4, 0, -1):
            cin, cout = convs[0][l].in_channels, convs[0][l].out_channels
            if fd is not None:
                d = fd[l]
            for g0 in range(0, P, P // groups):
                items = [{"a": d[p], "b": stacks[p][1][l - 1][0], "out": G(convs[p][l].weight),
                          "bias": G(convs[p][l].bias)} for p in range(g0, g0 + P // groups)]
                shape = (cout, 9 * cin, Mp, dt, dict(c1=cin, H=g, W=g, cin=cin))
                if defer is not None:
                    defer.append((items, shape))
                else:
                    self._wg_many(items, *shape, layout="conv")
            if fd is not None:
                continue
            wd, sw_ = self._pack(convs, l, "conv_dg")
            pres = [s[1][l - 1][1] for s in stacks]
            dx = self._e(P, Mp, cin)
            T.conv_dgrad(d[0], wd, B, g, g, 1, cout, cin, dt, out=dx[0], pre=pres[0],
                         batch=(P, even(d, "output gradients"), sw_, Mp * cin, even(pres, "pre-activations"))
                         if P > 1 else None)
            d = list(dx.unbind(0))
        if fd is not None:
            return fd[0], routes is not None
        return d, False

    def _fused_dgrads(self, stacks, routes=None):
        """layers 4..1 data gradients of P same-shape stacks (convs, saved, dtop) in ONE tmae_lic_stack backward
        launch (the chain through LDS, TMAE_LIC_STACK_BWD), or None when the operands do not allow it (the per-layer
        launches then run).  Returns d[l] for l = 0..4: the gradient w.r.t. layer l's pre-activation, a list over the
        problems (d[4] = the dtops); d[0..3] are views of one [P][Mp][cout] bf16 buffer per layer.  routes (one list
        per problem, the problems' accumulators disjoint): the first layers' input gradients too, routed like
        T.conv_dgrad's (the caller then skips them)."""
        if not self._fused_bwd:
            return None
        P, Mp = len(stacks), self.Mp
        convs = [s[0] for s in stacks]
        couts = [c.out_channels for c in convs[0]]
        # P > 2: the chain has never run for more than two problems here (the stride check this one replaces compared
        # every problem with the first and refused them); kept, because the chain and the per-layer launches round
        # differently and the kernel is unmeasured there
        if P > 2 or len(convs[0]) != 5 or any(c > ops.LSTK_MAXC for c in couts[:4]):
            return None
        dts = [s[2] for s in stacks]
        pres = [[s[1][l][1] for s in stacks] for l in (3, 2, 1, 0)]
        sx = self._stride(dts)
        if sx is None or any(p_[0].dtype != torch.bfloat16 or (P > 1 and self._stride(p_) != Mp * couts[l])
                             for p_, l in zip(pres, (3, 2, 1, 0))):
            return None
        outs = [self._e(P, Mp, couts[l]) for l in (3, 2, 1, 0)]
        lcouts = [couts[l] for l in (3, 2, 1, 0)]
        ws, st = [], {"x1": (sx, 0)}
        for k, l in enumerate((4, 3, 2, 1, 0) if routes is not None else (4, 3, 2, 1)):
            w, s = self._pack(convs, l, "licT")  # (layer 0: + the first layers' input gradients, routed)
            ws.append(w)
            st[f"w{k}"] = (s if P > 1 else 0, 0)
        for k, c in enumerate(lcouts):
            st[f"s{k}"] = (Mp * c, 0)
        if routes is not None:
            lcouts.append(convs[0][0].in_channels)
        ops.lic_stack_bwd(self.batch, self.g, dts[0], couts[4], couts[4], ws, lcouts, [p_[0] for p_ in pres], outs,
                          nb=(P, 1), strides=st, routes=routes)
        d = [None] * 5
        for k, l in enumerate((3, 2, 1, 0)):
            d[l] = [outs[k][p_] for p_ in range(P)]
        d[4] = dts
        return d


def _hs_layers(seq):
    """h_s layers as (conv, followed_by_pixel_shuffle)"""
    out = []
    for l in seq:
        if isinstance(l, nn.Conv2d):
            out.append((l, False))
        elif isinstance(l, nn.Sequential):
            out.append((l[0], True))
    return out


def _hs_convs(seq):
    return [c for c, _ in _hs_layers(seq)]


class _MCMTrainFn(torch.autograd.Function):
    """MCM.forward as one autograd node: (imgs, scores, *params) -> (x_hat, y likelihood, z likelihood)"""

    @staticmethod
    def forward(ctx, ex, noise, q, qm, imgs, scores, *params):
        x_hat, ylik, zlik = ex.forward(imgs, scores, noise, q, qm)
        ctx.ex = ex
        ctx.params = params
        return x_hat, ylik, zlik

    @staticmethod
    def backward(ctx, dxhat, dylik, dzlik):
        ex = ctx.ex
        params = ctx.params
        # a pre-existing .grad (accumulation across calls, zero_grad(set_to_none=False)) is added to by
        # autograd: write into a fresh buffer then, so the returned views never alias p.grad
        fresh = any(p.grad is not None for p in params if p.requires_grad)
        gflat = ex.grads_buffer(fresh)
        sync = getattr(ex.m, "grad_sync", None)
        ex.backward(dxhat, dylik, dzlik, gflat, sync=sync)
        if sync is not None:
            sync.finish()
        out = []
        for p in params:
            if not p.requires_grad:
                out.append(None)
            else:
                off = ex.offsets[id(p)]
                out.append(gflat[off:off + p.numel()].view(p.shape))
        return (None, None, None, None, None, None, *out)


# ---------------------------------------------------------------------- forward_encoder / forward_decoder alone
# (MCM.py:590-688 as separate nn.Module calls under autograd, like mae_train.py's: each is its own node over its own
# parameters; the executor keeps one set of activations per stage, so a stage's backward must come before that
# stage's next forward -- checked by the executor's forward counters.  No DP hand-offs: sync stays None.)
def enc_params(m):
    out = [m.encoder_norm.weight, m.encoder_norm.bias]
    for blk in m.encoder_blocks:
        out += _block_params(blk)
    return out + [m.encoder_embed.proj.weight, m.encoder_embed.proj.bias, m.cls_token]


def dec_params(m):
    out = [m.decoder_pred.weight, m.decoder_pred.bias, m.decoder_norm.weight, m.decoder_norm.bias,
           m.decoder_embed.weight, m.decoder_embed.bias, m.mask_token]
    for blk in m.decoder_blocks:
        out += _block_params(blk)
    return out


def _param_grads(ex, params, gflat):
    return [gflat[ex.offsets[id(p)]:ex.offsets[id(p)] + p.numel()].view(p.shape) if p.requires_grad else None
            for p in params]


class _MCMEncFn(torch.autograd.Function):
    """MCM.forward_encoder: (imgs, scores, *encoder params) -> (x_remain f32 [B, K, E], ids_restore)"""

    @staticmethod
    def forward(ctx, ex, imgs, scores, *params):
        x = ex.enc_fwd(ex._begin(imgs), scores, out_dtype=torch.float32)
        ctx.ex, ctx.params, ctx.gen = ex, params, ex.enc_gen
        ctx.mark_non_differentiable(ex.rest)
        return x.view(ex.batch, ex.m.num_keep_patches, -1), ex.rest

    @staticmethod
    def backward(ctx, dx, drest):
        ex, params = ctx.ex, ctx.params
        if ex.enc_gen != ctx.gen:
            raise RuntimeError("forward_encoder (or forward) ran again on this model before this backward: its saved "
                               "activations are gone (backward each forward_encoder before the next)")
        gflat = ex.grads_buffer(any(p.grad is not None for p in params if p.requires_grad))
        ex.bwd_begin(gflat)
        ex.enc_bwd(dx.float().contiguous().view(ex.Mp, -1))
        ex._side_join()
        return (None, None, None, *_param_grads(ex, params, gflat))


class _MCMDecFn(torch.autograd.Function):
    """MCM.forward_decoder: (x_remain [B, K, E], *decoder params) -> preds f32 [B, L, p*p*C] (ids_restore fixed)"""

    @staticmethod
    def forward(ctx, ex, ids_restore, x, *params):
        ex.rest = ids_restore
        ex.shuf = ops.invert_permutation(ids_restore)
        ex.w.refresh()  # (a no-op after forward_encoder's)
        preds = ex.dec_fwd(ex._cast(x.float().contiguous().view(ex.Mp, -1)), tokens=True)
        ctx.ex, ctx.params, ctx.gen, ctx.xshape = ex, params, ex.dec_gen, x.shape
        return preds.view(ex.batch, ex.L, -1)

    @staticmethod
    def backward(ctx, dpreds):
        ex, params = ctx.ex, ctx.params
        if ex.dec_gen != ctx.gen:
            raise RuntimeError("forward_decoder (or forward) ran again on this model before this backward: its saved "
                               "activations are gone (backward each forward_decoder before the next)")
        gflat = ex.grads_buffer(any(p.grad is not None for p in params if p.requires_grad))
        ex.bwd_begin(gflat)
        dP = ex._cast(dpreds.float().contiguous().view(ex.batch * ex.L, -1))  # the node starts at dP: no patchify
        dx = ex.dec_bwd(dP, out_f32=True)
        ex._side_join()
        return (None, None, dx.view(ctx.xshape), *_param_grads(ex, params, gflat))


def _exec_for(m, B, device):
    if getattr(m, "grad_sync", None) is not None:
        raise RuntimeError("MCM.forward_encoder / forward_decoder under autograd run without gradient all-reduce: "
                           "bucketed data parallel (grad_sync) covers forward() only")
    dt = m.compute_dtype
    if torch.is_autocast_enabled() and dt == torch.float32:
        dt = torch.bfloat16
    ex = getattr(m, "_train_exec", None)
    if ex is None or ex.batch != B or ex.dtype != dt or ex.device != device:
        ex = m._train_exec = TrainExec(m, B, dt, device)
    return ex


def train_forward_encoder(m, imgs, scores):
    """MCM.forward_encoder with autograd: (x_remain f32 [N, K, E], ids_restore)"""
    ex = _exec_for(m, imgs.shape[0], imgs.device)
    return _MCMEncFn.apply(ex, imgs, scores, *enc_params(m))


def train_forward_decoder(m, x, ids_restore):
    """MCM.forward_decoder with autograd: preds f32 [N, L, p*p*C] (gradients to x and the decoder's parameters)"""
    n, ntok, _ = x.shape
    if ntok != m.num_keep_patches:
        raise ValueError(f"forward_decoder under autograd takes num_keep_patches={m.num_keep_patches} tokens per image "
                         f"(the training workspaces are sized by it), got {ntok}")
    ex = _exec_for(m, n, x.device)
    return _MCMDecFn.apply(ex, ids_restore.to(x.device).to(torch.int64).contiguous(), x, *dec_params(m))


class BppFn(torch.autograd.Function):
    """RateDistortionLoss bpp term (rd_loss.py:19-20) with its HIP backward"""

    @staticmethod
    def forward(ctx, ylik, zlik, num_pixels):
        ctx.save_for_backward(ylik, zlik)
        ctx.num_pixels = num_pixels
        return ops.bpp(ylik, zlik, num_pixels)

    @staticmethod
    def backward(ctx, g):
        ylik, zlik = ctx.saved_tensors
        g = g.float().contiguous().reshape(1)
        dy = T.bpp_bwd(ylik.contiguous(), g, torch.empty_like(ylik), ctx.num_pixels)
        dz = T.bpp_bwd(zlik.contiguous(), g, torch.empty_like(zlik), ctx.num_pixels)
        return dy, dz, None


class AuxLossFn(torch.autograd.Function):
    """EntropyBottleneck.loss (compressai; utils/engine.py:79, 87): gradient only to quantiles"""

    @staticmethod
    def forward(ctx, eb, quantiles):
        ctx.eb = eb
        return ops.eb_aux_loss(eb)

    @staticmethod
    def backward(ctx, g):
        eb = ctx.eb
        dq = torch.empty_like(eb.quantiles)
        T.eb_aux_bwd(ops._eb_params(eb), eb.target, g.float().contiguous().reshape(1), dq, eb.channels)
        return None, dq
