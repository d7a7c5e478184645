"""MCM — drop-in for reference models/Compression/MCM.py:25 (``class MCM(CompressionModel)``).

Same constructor arguments and defaults (MCM.py:34-52), same submodule names, so
``state_dict()`` keys, ``named_parameters()`` (``*.quantiles`` split, model_utils.py:67-90) and
``load_state_dict`` behave as in the reference; same call surface (``forward(imgs, total_scores)``
-> ``{"loss", "likelihoods", "x_hat"}``, the staged ``forward_encoder(imgs, total_scores)`` ->
``(x_remain, ids_restore)``, ``forward_decoder(x_remain, ids_restore)`` -> patch tokens and
``forward_loss(imgs, preds)`` on patch tokens (or on the reconstruction itself), ``aux_loss()``,
``from_state_dict``, ``patchify`` / ``unpatchify``).  The two stages run the same kernels as ``forward``'s
encoder and decoder, without the entropy model; under autograd each is its own node (mcm_train.py).

Underneath, ``forward`` never calls a PyTorch compute op on the hot path: it enqueues the gfx950
kernels of libtmae.so on the current stream through a persistent workspace (``_Executor``), with
the LIC feature maps kept NHWC end to end.  ``compute_dtype`` selects the MFMA
operand type: torch.float32 (exact f32 MFMA; the parity path, default) or torch.bfloat16
(throughput path; f32 accumulate, f32 residual stream / entropy models / likelihoods).
"""
from __future__ import annotations

import collections.abc
import math
import os

from functools import partial
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .entropy import CompressionModel, EntropyBottleneck, GaussianConditional
from .layers import Block, BlockScratch, BlockWeights, PatchEmbed, conv3x3, run_block, subpel_conv3x3
from .pos_embed import get_2d_sincos_pos_embed


class MCM(CompressionModel):
    """Masked-compression model: MAE-ViT encoder -> hyperprior LIC with channel-conditional slices ->
    MAE-ViT decoder (reference MCM.py:25-968)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, encoder_embed_dim=768, encoder_depth=12,
                 encoder_num_heads=12, decoder_embed_dim=512, decoder_depth=8, decoder_num_heads=16, mlp_ratio=4.0,
                 norm_layer=partial(nn.LayerNorm, eps=1e-6), norm_pix_loss=False, latent_depth=384,
                 hyperprior_depth=192, num_slices=12, num_keep_patches=144):
        super().__init__()
        self.frozen_stages = -1
        self.encoder_embed_dim = E = encoder_embed_dim
        self.encoder_depth = encoder_depth
        self.encoder_num_heads = encoder_num_heads
        self.decoder_embed_dim = Dd = decoder_embed_dim
        self.decoder_depth = decoder_depth
        self.decoder_num_heads = decoder_num_heads
        self.latent_depth = M = latent_depth
        self.hyperprior_depth = N = hyperprior_depth
        self.num_slices = S = num_slices
        self.num_keep_patches = num_keep_patches

        # entropy models (MCM.py:71-73)
        self.entropy_bottleneck = EntropyBottleneck(N)
        self.gaussian_conditional = GaussianConditional(None)
        self.max_support_slices = S // 2

        # g_a / g_s: 1x1 convs E -> .. -> M and back (MCM.py:77-112)
        ga = [E, int(Dd + (E - Dd) * 3 / 4), int(Dd + (E - Dd) * 2 / 4), Dd, M]
        self.g_a = nn.Sequential(*_interleave([nn.Conv2d(ga[j], ga[j + 1], 1, 1, 0) for j in range(4)]))
        gs = ga[::-1]
        self.g_s = nn.Sequential(*_interleave([nn.ConvTranspose2d(gs[j], gs[j + 1], 1, 1, 0) for j in range(4)]))

        # h_a / h_s (MCM.py:115-162)
        ha = [M, M, int(N + (M - N) * 3 / 4), int(N + (M - N) * 2 / 4), int(N + (M - N) / 4), N]
        self.h_a = nn.Sequential(*_interleave([conv3x3(ha[j], ha[j + 1], stride=(2 if j in (2, 4) else 1))
                                               for j in range(5)]))
        hs = [N, int(N + (M - N) / 4), int(N + (M - N) * 2 / 4), int(N + (M - N) * 3 / 4), M, M]

        def h_s():
            return nn.Sequential(*_interleave([
                conv3x3(hs[0], hs[1]), subpel_conv3x3(hs[1], hs[2], r=2), conv3x3(hs[2], hs[3]),
                subpel_conv3x3(hs[3], hs[4], r=2), conv3x3(hs[4], hs[5])]))

        self.h_s_mean = h_s()
        self.h_s_scale = h_s()

        # channel-conditional slice transforms (MCM.py:165-293)
        sw = M // S
        mid = [int(sw * (S // 2 + 1)), int(sw * (S // 2 * 3 / 4 + 1)), int(sw * (S // 2 * 2 / 4 + 1)),
               int(sw * (S // 2 * 1 / 4 + 1)), sw]

        def stack(cin):
            ch = [cin] + mid
            return nn.Sequential(*_interleave([nn.Conv2d(ch[j], ch[j + 1], 3, 1, 1) for j in range(5)]))

        self.cc_transform_mean = nn.ModuleList([stack(int(M + sw * min(i, S // 2))) for i in range(S)])
        self.cc_transform_scale = nn.ModuleList([stack(int(M + sw * min(i, S // 2))) for i in range(S)])
        self.lrp_transform = nn.ModuleList([stack(int(M + sw * min(i + 1, S // 2 + 1))) for i in range(S)])

        # MAE encoder / decoder (MCM.py:300-354)
        self.encoder_embed = PatchEmbed(img_size, patch_size, in_chans, E)
        num_patches = self.encoder_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, E))
        self.encoder_pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, E), requires_grad=False)
        self.encoder_blocks = nn.ModuleList([Block(dim=E, num_heads=encoder_num_heads, mlp_ratio=mlp_ratio,
                                                   qkv_bias=True, norm_layer=norm_layer)
                                             for _ in range(encoder_depth)])
        self.encoder_norm = norm_layer(E)
        self.decoder_embed = nn.Linear(E, Dd, bias=True)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, Dd))
        self.decoder_pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, Dd), requires_grad=False)
        self.decoder_blocks = nn.ModuleList([Block(dim=Dd, num_heads=decoder_num_heads, mlp_ratio=mlp_ratio,
                                                   qkv_bias=True, norm_layer=norm_layer)
                                             for _ in range(decoder_depth)])
        self.decoder_norm = norm_layer(Dd)
        self.decoder_pred = nn.Linear(Dd, patch_size ** 2 * in_chans, bias=True)
        self.norm_pix_loss = norm_pix_loss
        self.initialize_weights()

        # MI355X execution settings (not part of the reference surface)
        self.compute_dtype = torch.float32
        self.sum_lanes = 8          # torch CPU float-sum vector width the reference ran with
        self.distortion = "ssim+l1"  # forward_loss terms; "none" skips them (encode/decode/rate only)
        self._exec = None

    # ---------------------------------------------------------------------------------- init
    def initialize_weights(self):
        """MCM.initialize_weights / _init_weights (MCM.py:454-495)."""
        g = int(self.encoder_embed.num_patches ** 0.5)
        self.encoder_pos_embed.data.copy_(
            torch.from_numpy(get_2d_sincos_pos_embed(self.encoder_pos_embed.shape[-1], g, True)).float().unsqueeze(0))
        self.decoder_pos_embed.data.copy_(
            torch.from_numpy(get_2d_sincos_pos_embed(self.decoder_pos_embed.shape[-1], g, True)).float().unsqueeze(0))
        w = self.encoder_embed.proj.weight.data
        torch.nn.init.xavier_uniform_(w.view([w.shape[0], -1]))
        torch.nn.init.normal_(self.cls_token, std=0.02)
        torch.nn.init.normal_(self.mask_token, std=0.02)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            torch.nn.init.xavier_uniform_(m.weight)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def load_state_dict(self, state_dict, strict=True):
        # the reference override drops `strict` (MCM.py:445-446); keep the compressai buffer resizing
        r = super().load_state_dict(state_dict, strict=strict)
        self._exec = None
        self._train_exec = None
        return r

    @classmethod
    def from_state_dict(cls, num_keep_patches, state_dict):
        net = cls(num_keep_patches=num_keep_patches)
        net.load_state_dict(state_dict)
        return net

    # ---------------------------------------------------------------------------------- layout helpers
    def patchify(self, imgs):
        p = self.encoder_embed.patch_size[0]
        assert imgs.shape[2] == imgs.shape[3] and imgs.shape[2] % p == 0
        h = w = imgs.shape[2] // p
        x = imgs.reshape(imgs.shape[0], 3, h, p, w, p)
        return torch.einsum("nchpwq->nhwpqc", x).reshape(imgs.shape[0], h * w, p ** 2 * 3)

    def unpatchify(self, x):
        p = self.encoder_embed.patch_size[0]
        h = w = int(x.shape[1] ** 0.5)
        assert h * w == x.shape[1]
        x = torch.einsum("nhwpqc->nchpwq", x.reshape(x.shape[0], h, w, p, p, 3))
        return x.reshape(x.shape[0], 3, h * p, w * p)

    # ---------------------------------------------------------------------------------- masking
    def get_ids_shuffle(self, total_scores):
        """MCM.get_ids_shuffle (MCM.py:364-423) — one GPU launch for the whole batch."""
        if self.num_keep_patches > total_scores.shape[1]:
            raise ValueError("Number of patches should not be greater than the length of scores")
        return ops.ids_shuffle(total_scores, self.num_keep_patches, self.sum_lanes)[0]

    def random_masking(self, x, total_scores):
        """MCM.random_masking (MCM.py:548-588): (x_remain, ids_restore)."""
        shuf, rest = ops.ids_shuffle(total_scores, self.num_keep_patches, self.sum_lanes)
        D = x.shape[-1]
        x_remain = torch.gather(x, 1, shuf[:, : self.num_keep_patches].unsqueeze(-1).repeat(1, 1, D))
        return x_remain, rest

    # ---------------------------------------------------------------------------------- forward
    def _executor(self, batch, device):
        dt = self.compute_dtype
        if torch.is_autocast_enabled() and dt == torch.float32:
            dt = torch.bfloat16  # val_one_epoch runs under autocast (utils/engine.py:189)
        ex = self._exec
        if ex is None or ex.batch != batch or ex.dtype != dt or ex.device != device:
            ex = self._exec = _Executor(self, batch, dt, device)
        ex.refresh_weights()
        return ex

    def forward(self, imgs, total_scores, noise=None, q=None, qoffsets=None, qlevels=None):
        """MCM.forward (MCM.py:714-803).  `noise=(z_noise, y_noise)` (NCHW, U(-1/2, 1/2)) replaces the
        training-mode quantisation noise — used by parity tests; otherwise drawn on the device.

        q: ladder positions of the y quantiser step, as compress_batch takes them (an int or B ints
        in -32..32), or an int32 [B] tensor on the device.  y is then quantised, reconstructed and modelled at the step
        2^(q/8) with the coder's arithmetic: in eval x_hat is bitwise decompress_batch(compress_batch(q=), q=)'s and
        the y likelihoods are the coded symbols' masses; under autograd the backward is that forward's.  None, or host
        values that are all zero, is the path without q with its kernels and bits.  A device tensor is taken as given
        (not read back, so the call can be captured into a graph) and always runs the kernels with a step.

        qoffsets / qlevels (eval only): compress_batch's table of ladder offsets and source of the
        per-patch levels; y is then quantised at a step per kept patch, q being the base position.  x_hat and the y
        likelihoods are bit for bit what the coder reconstructs and codes with the same arguments.  The slice loop
        runs unchained.  Under autograd or in training mode ValueError: forward_qmap is the differentiable forward."""
        q = self._forward_q(q, imgs.shape[0])
        train = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        qm = self._check_qoffsets(qoffsets, qlevels, imgs.shape[0], self._geometry()[3], "forward")
        if qm is not None and (train or self.training):
            raise ValueError("forward: qoffsets is for evaluation (model.eval() under torch.no_grad()); forward_qmap "
                             "is the differentiable forward at a map of quantiser steps")
        if not imgs.is_cuda:
            raise ValueError("MCM.forward runs on the MI355X kernels: move the model and inputs to the GPU")
        if train:
            return self._forward_train(imgs, total_scores, noise, q)
        with torch.no_grad():
            ex = self._executor(imgs.shape[0], imgs.device)
            out = ex.run(imgs, total_scores, self.training, noise, q=q, qm=qm)
            x_hat = out["x_hat"]
            loss = self.forward_loss(imgs, x_hat) if self.distortion != "none" else (ex.zero_loss,) * 3
        return {"loss": loss, "likelihoods": {"y": out["y"], "z": out["z"]}, "x_hat": x_hat}

    @classmethod
    def _forward_q(cls, q, B):
        """q= of forward -> None, a list of B ladder positions (_check_q) or the caller's device tensor, checked for
        what can be checked without reading it"""
        if torch.is_tensor(q) and q.is_cuda:
            if q.dtype != torch.int32 or q.dim() != 1 or q.numel() != B or not q.is_contiguous():
                raise ValueError(f"forward: a device q must be a contiguous int32 [{B}] tensor, got {q.dtype} "
                                 f"{tuple(q.shape)}")
            return q
        return cls._check_q(q, B, "forward")

    def forward_qmap(self, imgs, total_scores, noise=None, q=None, qoffsets=None, qlevels="scores", _rows=None,
                     _read_status=True):
        """The differentiable forward at a quantiser step per kept patch: forward(q=)'s arithmetic
        and gradients element by element at the step of the element's own patch.  qoffsets (required) and qlevels
        are compress_batch's: a table of 2..16 ladder offsets and the source of the per-patch levels, "scores" or an
        integer map [B, L] in image patch order; q is the base position as forward takes it (an int, B ints or an int32
        [B] device tensor; None: 0).  Levels and offsets are integers derived by comparisons and carry no gradient.

        Under autograd or in training mode: the training node (mcm_train._MCMTrainFn) with the map; y_hat before the
        LRP term is bit for bit what the coder reconstructs with the same arguments, and with all-zero offsets every
        output and gradient is bitwise forward(q=)'s at a non-zero q.  Under eval() and no_grad: forward(qoffsets=)'s
        bits, with the slice loop allowed to run chained.  A device map with an entry outside the table gives that
        image all-zero levels and raises ValueError naming the image after the kernels have been enqueued.

        _rows / _read_status are for captured calls (GraphedTrainStep, a captured eval forward): the offsets' rows as a
        static device buffer (int32 [B, 16]), so that nothing is uploaded, and whether the status of a device map is
        read back here."""
        if qoffsets is None:
            raise ValueError("forward_qmap: qoffsets (the table of ladder offsets) is required; forward(q=) is the "
                             "path without a map")
        B = imgs.shape[0]
        q = self._forward_q(q, B)
        qm = self._check_qoffsets(qoffsets, qlevels, B, self._geometry()[3], "forward_qmap")
        if not imgs.is_cuda:
            raise ValueError("MCM.forward_qmap runs on the MI355X kernels: move the model and inputs to the GPU")
        train = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if train or self.training:
            with torch.set_grad_enabled(train):
                out = self._forward_train(imgs, total_scores, noise, q, (*qm, _rows))
            status = self._train_exec.qm_status
            if status is not None and _read_status:
                _Executor._raise_levels(status.cpu().numpy(), "forward_qmap")
            return out
        with torch.no_grad():
            ex = self._executor(B, imgs.device)
            out = ex.run(imgs, total_scores, False, noise, q=q, qm=(*qm, _rows), qm_chain=True)
            x_hat = out["x_hat"]
            loss = self.forward_loss(imgs, x_hat) if self.distortion != "none" else (ex.zero_loss,) * 3
        return {"loss": loss, "likelihoods": {"y": out["y"], "z": out["z"]}, "x_hat": x_hat}

    def _forward_train(self, imgs, total_scores, noise, q=None, qm=None):
        """MCM.forward under autograd (utils/engine.py:75): one autograd node whose forward keeps the
        activations and whose backward is the HIP reverse pass (mcm_train.py)."""
        from .mcm_train import TrainExec, _MCMTrainFn

        dt = self.compute_dtype
        if torch.is_autocast_enabled() and dt == torch.float32:
            dt = torch.bfloat16
        B = imgs.shape[0]
        ex = getattr(self, "_train_exec", None)
        if ex is None or ex.batch != B or ex.dtype != dt or ex.device != imgs.device:
            ex = self._train_exec = TrainExec(self, B, dt, imgs.device)
        x_hat, ylik, zlik = _MCMTrainFn.apply(ex, noise, q, qm, imgs, total_scores, *self.parameters())
        loss = self.forward_loss(imgs, x_hat) if self.distortion != "none" else (
            torch.zeros((), device=imgs.device),) * 3
        return {"loss": loss, "likelihoods": {"y": ylik, "z": zlik}, "x_hat": x_hat}

    def _stage_trains(self, what, t, params, extra=False):
        """common entry of forward_encoder / forward_decoder: the device check, then whether the stage takes its
        training node (grad enabled and one of its parameters -- or `extra` -- requires grad, the rule of forward)"""
        if not t.is_cuda:
            raise ValueError(f"MCM.{what} runs on the MI355X kernels: move the model and inputs to the GPU")
        return torch.is_grad_enabled() and (extra or any(p.requires_grad for p in params))

    def forward_encoder(self, imgs, total_scores):
        """MCM.forward_encoder (MCM.py:590-634) -> (x_remain f32 [N, K, E], ids_restore int64 [N, L]): ids, kept-patch
        embedding, cls, encoder blocks, encoder_norm without the cls row; g_a / h_a do not run.  Under autograd its
        own node with the HIP encoder backward (mcm_train._MCMEncFn)."""
        from . import mcm_train

        if self._stage_trains("forward_encoder", imgs, mcm_train.enc_params(self)):
            return mcm_train.train_forward_encoder(self, imgs, total_scores)
        with torch.no_grad():
            return self._executor(imgs.shape[0], imgs.device).encode(imgs, total_scores)

    def forward_decoder(self, x_remain, ids_restore):
        """MCM.forward_decoder (MCM.py:636-688) -> preds f32 [N, L, p*p*in_chans], columns (py, px, c) as in the
        reference.  x_remain [N, ntok, E] with 1 <= ntok <= L (mask tokens fill the other L + 1 - ntok rows; the
        first token takes the cls row, the reference's off-by-one).  Under autograd (decoder parameters or x_remain
        requiring gradients) its own node with the HIP decoder backward (mcm_train._MCMDecFn); ntok must then be
        num_keep_patches."""
        from . import mcm_train

        train = self._stage_trains("forward_decoder", x_remain, mcm_train.dec_params(self),
                                     extra=x_remain.requires_grad)
        L, E = self.encoder_embed.num_patches, self.encoder_embed_dim
        if x_remain.dim() != 3 or x_remain.shape[2] != E or not 1 <= x_remain.shape[1] <= L:
            raise ValueError(f"forward_decoder: x_remain must be [N, ntok, E={E}] with 1 <= ntok <= L={L}, got "
                             f"{tuple(x_remain.shape)}")
        if tuple(ids_restore.shape) != (x_remain.shape[0], L):
            raise ValueError(f"forward_decoder: ids_restore must be [N={x_remain.shape[0]}, L={L}], got "
                             f"{tuple(ids_restore.shape)}")
        if train:
            return mcm_train.train_forward_decoder(self, x_remain, ids_restore)
        with torch.no_grad():
            return self._executor(x_remain.shape[0], x_remain.device).decode(x_remain, ids_restore)

    def forward_loss(self, imgs, preds):
        """MCM.forward_loss (MCM.py:690-712): (1 - SSIM, L1, VGG16 feature loss).  `preds` is either the reference's
        argument, patch tokens [N, L, p*p*in_chans] (unpatchified here by tmae_unpatchify, differentiable w.r.t. the
        tokens), or the reconstruction itself [N, in_chans, H, W] (what forward() passes).  The reference downloads
        torchvision's pretrained VGG16 on every call (vgg.py:14, 99); here the feature loss runs once local
        weights are given (load_vgg16, or the TMAE_VGG16_WEIGHTS file) and is 0 (with a one-time warning in
        training) without them."""
        from . import vgg
        from .distortion import UnpatchifyFn, ssim_l1_loss

        p, C = self.encoder_embed.patch_size[0], self.encoder_embed.proj.in_channels
        L = self.encoder_embed.num_patches
        if preds.dim() == 3:
            if tuple(preds.shape[1:]) != (L, p * p * C) or preds.shape[0] != imgs.shape[0]:
                raise ValueError(f"forward_loss: patch tokens must be [N={imgs.shape[0]}, L={L}, "
                                 f"p*p*in_chans={p * p * C}], got {tuple(preds.shape)}")
            if not preds.is_cuda:
                raise ValueError("MCM.forward_loss runs on the MI355X kernels: move the model and inputs to the GPU")
            x_hat = UnpatchifyFn.apply(preds, p, C, imgs.shape[2], imgs.shape[3])
        elif preds.dim() == 4:
            x_hat = preds
        else:
            raise ValueError(f"forward_loss takes patch tokens [N, L={L}, p*p*in_chans={p * p * C}] or images "
                             f"[N, {C}, H, W], got a {preds.dim()}-D tensor {tuple(preds.shape)}")
        s, l1 = ssim_l1_loss(x_hat, imgs)
        net = self._vgg_net(imgs.device)
        if net is None:
            if self.training:
                vgg.warn_missing_once()
            return s, l1, torch.zeros((), device=imgs.device)
        return s, l1, vgg.cal_features_loss(x_hat, imgs, net)

    def load_vgg16(self, weights):
        """local VGG16 weights for the feature loss: a torchvision vgg16 state_dict (or the reference Vgg16
        module's) or a path to one (loaded with weights_only=True).  Not part of MCM's state_dict, as in the
        reference, where the network is frozen and rebuilt inside the loss."""
        from .vgg import load_vgg16_state_dict

        sd = load_vgg16_state_dict(weights) if isinstance(weights, (str, os.PathLike)) else weights
        self.__dict__["_vgg_sd"] = {k: v.detach().cpu() for k, v in sd.items() if torch.is_tensor(v)}
        self.__dict__["_vgg"] = None

    def _vgg_net(self, device):
        from .vgg import Vgg16Features

        if self.__dict__.get("_vgg_sd") is None:
            path = os.environ.get("TMAE_VGG16_WEIGHTS")
            if not path:
                return None
            self.load_vgg16(path)
        dt = self.compute_dtype
        if torch.is_autocast_enabled() and dt == torch.float32:
            dt = torch.bfloat16
        net = self.__dict__.get("_vgg")
        if net is None or net.device != torch.device(device) or net.dtype != dt:
            net = Vgg16Features(self.__dict__["_vgg_sd"], device, dt)
            self.__dict__["_vgg"] = net
        return net

    def aux_loss(self):
        return self.entropy_bottleneck.loss()

    def compress(self, imgs, total_scores):
        """MCM.compress (MCM.py:805-894) -> {"string": [[y_string], z_strings], "shape", "ids_restore"}.
        Needs the CDF tables: call update(force=True) first (testing.py:223), as with compressai."""
        if not imgs.is_cuda:
            raise ValueError("MCM.compress runs on the MI355X kernels: move the model and inputs to the GPU")
        self.entropy_bottleneck._check_cdf()
        self.gaussian_conditional._check_cdf()
        with torch.no_grad():
            ex = self._executor(imgs.shape[0], imgs.device)
            return ex.compress(imgs, total_scores)

    def decompress(self, strings, shape, ids_restore=None):
        """MCM.decompress (MCM.py:896-968) -> {"x_hat"}.  Batch = number of z strings; the reference's
        reshape(1, ...) at MCM.py:944 limits it to one image, this handles any batch the y string holds."""
        assert isinstance(strings, list) and len(strings) == 2
        if ids_restore is None:
            raise ValueError("MCM.decompress needs ids_restore (the decoder unshuffles by it, MCM.py:667-669)")
        self.entropy_bottleneck._check_cdf()
        self.gaussian_conditional._check_cdf()
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise ValueError("MCM.decompress runs on the MI355X kernels: move the model to the GPU")
        with torch.no_grad():
            ex = self._executor(len(strings[1]), dev)
            return {"x_hat": ex.decompress(strings, shape, ids_restore)}

    @staticmethod
    def _check_q(q, B, who):
        """q= of the batch methods -> None (no q, or every entry 0: the plain path) or a list of B ladder positions
        (bitstream.check_q); an int stands for all B images.  ValueError before anything is launched"""
        from .bitstream import check_q

        if q is None:
            return None
        if np.ndim(q) == 0:
            qs = [check_q(q, f"{who}: q")] * B
        else:
            qs = list(q.tolist() if hasattr(q, "tolist") else q)
            if len(qs) != B:
                raise ValueError(f"{who}: {len(qs)} entries of q for {B} images: one per image, or one int for all")
            qs = [check_q(v, f"{who}: q[{b}]") for b, v in enumerate(qs)]
        return qs if any(qs) else None

    @staticmethod
    def _check_rdoq(rdoq, B, who):
        """rdoq= of the encode methods -> None (plain rounding with today's kernels) or a list of B weights >= 0, in
        squared latent units per bit; a float stands for all B images.  ValueError before anything
        is launched"""
        if rdoq is None:
            return None
        if np.ndim(rdoq) == 0:
            ws = [rdoq] * B
        else:
            ws = list(rdoq.tolist() if hasattr(rdoq, "tolist") else rdoq)
            if len(ws) != B:
                raise ValueError(f"{who}: {len(ws)} entries of rdoq for {B} images: one per image, or one float for all")
        out = []
        for b, v in enumerate(ws):
            if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"{who}: rdoq[{b}] = {v!r} is not a number")
            v = float(v)
            if not (math.isfinite(v) and v >= 0.0) or v > float(np.finfo(np.float32).max):
                raise ValueError(f"{who}: rdoq[{b}] = {v!r} must be finite and >= 0")
            out.append(v)
        return out

    @staticmethod
    def _check_qoffsets(qoffsets, qlevels, B, L, who, K=None):
        """qoffsets= / qlevels= of the batch methods -> None (no map) or (the offsets as a tuple, the source of the
        levels): "scores", an int32 numpy array checked here, or the caller's device tensor (checked on the device).
        The array is [B, L] in image patch order; with K (decompress_batch) also [B, K] in kept order.  ValueError
        before anything is launched"""
        from .bitstream import check_offsets

        if qoffsets is None:
            if qlevels is not None:
                raise ValueError(f"{who}: qlevels without qoffsets (the table the levels index)")
            return None
        offs = check_offsets(qoffsets, f"{who}: qoffsets")
        if isinstance(qlevels, str) or qlevels is None:
            if qlevels not in (None, "scores") or K is not None:
                raise ValueError(f"{who}: qlevels = {qlevels!r}: " + ("the levels compress_batch returned, or an int "
                                 f"map [{B}, {L}]" if K is not None else f"'scores' or an int map [{B}, {L}]"))
            return offs, "scores"
        shapes = [(B, L)] + ([(B, K)] if K is not None else [])
        if torch.is_tensor(qlevels) and qlevels.is_cuda:
            if qlevels.dtype != torch.int32 or tuple(qlevels.shape) not in shapes or not qlevels.is_contiguous():
                raise ValueError(f"{who}: a device qlevels must be a contiguous int32 {list(shapes[0])} tensor, got "
                                 f"{qlevels.dtype} {tuple(qlevels.shape)}")
            return offs, qlevels
        a = np.asarray(qlevels.numpy() if torch.is_tensor(qlevels) else qlevels)
        if a.shape not in shapes or a.dtype.kind not in "iu":
            raise ValueError(f"{who}: qlevels must be 'scores' or an integer map {list(shapes[0])} in image patch "
                             f"order, got {a.dtype} {a.shape}")
        bad = np.flatnonzero(((a < 0) | (a >= len(offs))).any(axis=1))
        if bad.size:
            raise ValueError(f"{who}: qlevels of image {int(bad[0])}: a level outside 0..{len(offs) - 1}")
        return offs, np.ascontiguousarray(a, dtype=np.int32)

    def compress_batch(self, imgs, total_scores, lanes=1, z_lanes=None, q=None, qoffsets=None, qlevels=None,
                       rdoq=None):
        """compress with one independent record per image, coded on the device (csrc/rans_device.hip) ->
        {"string": [y_strings, z_strings], "shape", "ids_restore"}, len(y_strings) == len(z_strings) == B.
        Image b's (y_strings[b], z_strings[b]) are the strings MCM.compress (MCM.py:805-894) returns for that image
        alone.  Same preconditions as compress.

        lanes / z_lanes (powers of two in 1..64, z_lanes=None: 1) deal an image's y / z symbols over that many
        interleaved rANS states, which shortens the serial chain of the coder; the strings are then the records of
        coder.encode_record, the result also carries "lanes": (lanes, z_lanes), and decompress_batch needs the same
        values.  (1, 1) is the plain format above.

        q: ladder positions of the y quantiser step, an int or a sequence of B ints in -32..32
        (bitstream.qstep: step 2^(q/8), 1/16 .. 16); image b's y symbols are round((y - mu) / step_b) and its record
        grows as q falls.  None, or all zero, is the path above with its kernels and bytes; decompress_batch needs
        the same q.  z is not scaled.

        qoffsets: a table of 2..16 ladder offsets, integers in -64..64; every kept patch p then
        has a level l[p] into it and its y elements are coded at ladder position clamp(q + qoffsets[l[p]], -32, 32),
        q being the base (None: 0).  qlevels: "scores" (the default: the kept patches ranked by their score, level 0
        the most text-like share) or an integer map [B, L] in image patch order (the layout of total_scores), a numpy
        array or an int32 device tensor; an entry outside the table raises ValueError naming the image.  The result
        then carries "qoffsets" and "qlevels" (int32 [B, K] on the device, kept order), which decompress_batch needs
        together with q.

        rdoq: rate-distortion optimised quantisation of y, a weight >= 0 in squared latent units per
        bit, a float or B floats.  Every non-zero y symbol may then move one step toward zero where the bits that
        saves through its own CDF row, times the weight, exceed the latent error it adds (csrc/gc_rdo.h).  None is
        the path above with its kernels and bytes; 0.0 takes the new kernel and gives the same bytes.  It works with
        q and with qoffsets; the decoder needs nothing, decompress_batch takes the same arguments as without it.  The
        result then carries "rdoq" and last_streams["y_changed"] the moved symbols per image.  z is not touched."""
        from .coder import check_lanes

        lanes, z_lanes = check_lanes(lanes), check_lanes(1 if z_lanes is None else z_lanes)
        q = self._check_q(q, imgs.shape[0], "compress_batch")
        rdoq = self._check_rdoq(rdoq, imgs.shape[0], "compress_batch")
        qm = self._check_qoffsets(qoffsets, qlevels, imgs.shape[0], self._geometry()[3], "compress_batch")
        if not imgs.is_cuda:
            raise ValueError("MCM.compress_batch runs on the MI355X kernels: move the model and inputs to the GPU")
        self.entropy_bottleneck._check_cdf()
        self.gaussian_conditional._check_cdf()
        with torch.no_grad():
            ex = self._executor(imgs.shape[0], imgs.device)
            return ex.compress_batch(imgs, total_scores, lanes, z_lanes, q, qm=qm, rdoq=rdoq)

    def decompress_batch(self, strings, shape, ids_restore=None, lanes=1, z_lanes=None, q=None, qoffsets=None,
                         qlevels=None):
        """inverse of compress_batch -> {"x_hat"}: strings = [y_strings, z_strings], one of each per image.  The
        streams are decoded on the device inside the slice loop; a corrupt stream raises ValueError naming its image
        after the whole batch has been enqueued.  lanes / z_lanes are compress_batch's; a record whose header does
        not fit them raises ValueError naming its image before anything is launched.  q: compress_batch's (an int or
        one per image), checked before anything is launched as well.  qoffsets / qlevels: compress_batch's table and
        the "qlevels" it returned (int [B, K], kept order), or an integer map [B, L] in image patch order (at K = L an
        array is taken to be in kept order)."""
        from .coder import check_lanes

        lanes, z_lanes = check_lanes(lanes), check_lanes(1 if z_lanes is None else z_lanes)
        assert isinstance(strings, list) and len(strings) == 2
        if ids_restore is None:
            raise ValueError("MCM.decompress_batch needs ids_restore (the decoder unshuffles by it, MCM.py:667-669)")
        if len(strings[0]) != len(strings[1]):
            raise ValueError(f"{len(strings[0])} y strings but {len(strings[1])} z strings: one of each per image")
        q = self._check_q(q, len(strings[1]), "decompress_batch")
        _, _, K, L = self._geometry()
        qm = self._check_qoffsets(qoffsets, qlevels, len(strings[1]), L, "decompress_batch", K=K)
        self.entropy_bottleneck._check_cdf()
        self.gaussian_conditional._check_cdf()
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise ValueError("MCM.decompress_batch runs on the MI355X kernels: move the model to the GPU")
        with torch.no_grad():
            ex = self._executor(len(strings[1]), dev)
            if qm is not None:
                qm = ex.decode_map(qm, ids_restore)
            return {"x_hat": ex.decompress_batch(strings, shape, ids_restore, lanes, z_lanes, q=q, qm=qm)}

    def _geometry(self):
        """(img_size, patch_size, num_keep_patches, L) as the container header states them"""
        pe = self.encoder_embed
        return int(pe.img_size[0]), int(pe.patch_size[0]), int(self.num_keep_patches), int(pe.num_patches)

    def encode_bytes(self, imgs, total_scores, lanes=1, z_lanes=None, orig_sizes=None, q=None, target_bytes=None,
                     qoffsets=None, qlevels=None, rdoq=None):
        """compress_batch into self-contained bitstreams -> list of B bytes objects (bitstream.py, container version
        1): header (geometry, lanes, original size), the kept patch ids packed on the device (ops.ids_pack, at
        ceil(log2 L) bits each), then compress_batch's z and y records of the image as they are.  decode_bytes needs
        nothing else, in this process or another.  orig_sizes: optional list of B (width, height) to record.

        q: compress_batch's (an int or B ints); an image coded at q != 0 becomes a TQC blob that records its q, one
        at q = 0 the TMC blob as before.  target_bytes (an int or B ints) instead picks per image the smallest q of
        the ladder whose whole blob (header, ids, z and y) is at most that many bytes: a lower-bound bisection over
        -32..32 for all images at once, at most 7 probes, each of which repeats only the slice loop and the y coder
        (the analysis up to h_s runs once).  The blob kept is the one of the image's smallest successful probe.  The
        size is taken to be non-increasing in q; an image that does not fit at q = 32 gets its q = 32 blob, longer
        than the target.  q together with target_bytes raises ValueError.

        qoffsets / qlevels: compress_batch's; every image then becomes a TPC blob that records its
        base q (0 included), the table and the levels of its kept patches, packed on the device (ops.qlevels_pack).
        With target_bytes the bisection runs over the base q as above, the map being rebuilt per probe, and the size
        counts the TPC header and the level words.

        rdoq: compress_batch's, a float or B floats.  The blobs are of the same kinds and decode
        with decode_bytes as they are: nothing of it is recorded.  With target_bytes the weight is the same in every
        probe and the bisection is unchanged."""
        from . import bitstream

        B = imgs.shape[0]
        rdoq = self._check_rdoq(rdoq, B, "encode_bytes")
        if orig_sizes is not None and len(orig_sizes) != B:
            raise ValueError(f"{len(orig_sizes)} original sizes for {B} images")
        if q is not None and target_bytes is not None:
            raise ValueError("encode_bytes: give q or target_bytes, not both")
        img, patch, K, L = self._geometry()
        qm = self._check_qoffsets(qoffsets, qlevels, B, L, "encode_bytes")
        if target_bytes is not None:
            fixed = 4 * bitstream.id_words(L, K)
            if qm is None:
                size = lambda v: (bitstream.QHEADER_BYTES if v else bitstream.HEADER_BYTES) + fixed  # noqa: E731
            else:
                size = lambda v: bitstream.PHEADER_BYTES + fixed + 4 * bitstream.level_words(K, len(qm[0]))  # noqa: E731
            lanes, z_lanes, ids, z, y, qs, lev = self._encode_sections_target(
                imgs, total_scores, lanes, z_lanes, self._check_targets(target_bytes, B, "encode_bytes"), size, qm,
                rdoq)
        else:
            qs = self._check_q(q, B, "encode_bytes") or [0] * B
            lanes, z_lanes, ids, z, y, lev = self._encode_sections(imgs, total_scores, lanes, z_lanes, qs, qm, rdoq)
        return [bitstream.assemble(img, K, patch, lanes, z_lanes, None if orig_sizes is None else orig_sizes[b],
                                   ids[b], z[b], y[b], qs[b], *(() if qm is None else (qm[0], lev[b])))
                for b in range(B)]

    @staticmethod
    def _check_targets(target_bytes, B, who):
        if isinstance(target_bytes, (int, np.integer)):
            return [int(target_bytes)] * B
        t = [int(v) for v in target_bytes]
        if len(t) != B:
            raise ValueError(f"{who}: {len(t)} entries of target_bytes for {B} images: one per image, or one int")
        return t

    def _side_words(self, qm):
        """the id words and, with a map, the level words of the batch just coded, packed on the device -> (uint32-
        compatible numpy [B, W], [B, W2] or None): one copy for both"""
        K = self._geometry()[2]
        ids = ops.ids_pack(self._exec.last_ids_shuffle, K)
        if qm is None:
            return ids.cpu().numpy(), None  # the one extra copy
        W = ids.shape[1]
        both = torch.cat([ids, ops.qlevels_pack(self._exec.last_levels, len(qm[0]))], dim=1).cpu().numpy()
        return both[:, :W], both[:, W:]

    def _encode_sections(self, imgs, total_scores, lanes, z_lanes, q=None, qm=None, rdoq=None):
        """the sections of encode_bytes' blobs (and of encode_image's tiles) -> (lanes, z_lanes, id words uint32-
        compatible numpy [B, W], z records, y records, level words [B, W2] or None): compress_batch, then the kept ids
        (and with a map qm = _check_qoffsets' pair the levels) packed on the device"""
        out = self.compress_batch(imgs, total_scores, lanes, z_lanes, q, *((None, None) if qm is None else qm),
                                  rdoq=rdoq)
        lanes, z_lanes = out.get("lanes", (1, 1))
        ids, lev = self._side_words(qm)
        y, z = out["string"]
        return lanes, z_lanes, ids, z, y, lev

    def _encode_sections_target(self, imgs, total_scores, lanes, z_lanes, targets, fixed_bytes, qm=None, rdoq=None):
        """_encode_sections with per image the smallest q whose blob fits targets[b] -> (..., y records, q per image,
        level words); fixed_bytes(q): the bytes of a blob at q besides its z and y records"""
        from .coder import check_lanes

        lanes, z_lanes = check_lanes(lanes), check_lanes(1 if z_lanes is None else z_lanes)
        if not imgs.is_cuda:
            raise ValueError("MCM.encode_bytes runs on the MI355X kernels: move the model and inputs to the GPU")
        self.entropy_bottleneck._check_cdf()
        self.gaussian_conditional._check_cdf()
        with torch.no_grad():
            ex = self._executor(imgs.shape[0], imgs.device)
            z, y, qs = ex.compress_batch_target(imgs, total_scores, lanes, z_lanes, targets, fixed_bytes, qm=qm,
                                                rdoq=rdoq)
        ids, lev = self._side_words(qm)
        return lanes, z_lanes, ids, z, y, qs, lev

    def _decode_sections(self, ids, z, y, lanes, z_lanes, who, q=None, maps=None):
        """inverse of _encode_sections -> x_hat [B, 3, S, S]: the id words (B uint32 [W] rows) go up, ops.ids_unpack
        validates and completes them on the device, the records take the decompress_batch path and the ids status
        words are read with the coder's.  who: the calling method's name for the error message; q: the images' ladder
        positions as their containers state them (None: all zero); maps: per image (nlev, offsets, level words) as
        its container states them (nlev = 1: no map), or None when no image has one.  With a map the level words go
        up with their per-image table sizes, ops.qlevels_unpack validates them and an image without a map gets a
        constant one"""
        from . import bitstream

        _, _, K, L = self._geometry()
        B = len(ids)
        if maps is not None and all(m[0] == 1 for m in maps):
            maps = None
        if maps is None:
            q = self._check_q(q, B, who)
        else:
            q = [0] * B if q is None else ([bitstream.check_q(q)] * B if np.ndim(q) == 0 else
                                           [bitstream.check_q(v) for v in q])
        self.entropy_bottleneck._check_cdf()
        self.gaussian_conditional._check_cdf()
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise ValueError(f"MCM.{who} runs on the MI355X kernels: move the model to the GPU")
        strings = [[bytes(s) for s in y], [bytes(s) for s in z]]
        words = torch.from_numpy(np.stack(ids).view(np.int32)).to(dev)
        qm = None
        if maps is not None:
            ldw = max(bitstream.level_words(K, m[0]) for m in maps)
            lw = np.zeros((B, ldw), dtype=np.uint32)
            for b, m in enumerate(maps):
                if m[0] > 1:
                    lw[b, :bitstream.level_words(K, m[0])] = m[2]
            table = np.array([[m[0]] + bitstream.offsets_row(m[1]) for m in maps], dtype=np.int32)
            lw, table = torch.from_numpy(lw.view(np.int32)).to(dev), torch.from_numpy(table).to(dev)
        with torch.no_grad():
            ex = self._executor(len(ids), dev)
            _, rest, status = ops.ids_unpack(words, L, K)
            if maps is not None:
                levels, lstatus = ops.qlevels_unpack(lw, table[:, 0].contiguous(), K)
                qm = dict(levels=levels, status=lstatus, offsets=table[:, 1:].contiguous())
            return ex.decompress_batch(strings, torch.Size([ex.hz, ex.hz]), rest, lanes, z_lanes, ids_status=status,
                                       q=q, qm=qm)

    def decode_bytes(self, blobs):
        """inverse of encode_bytes -> {"x_hat": [B, 3, S, S], "orig_sizes": [(width, height) or None per image]}.
        Every header is parsed on the host first: a malformed blob, one of another geometry (img_size, patch_size,
        num_keep_patches) than this model's, or blobs of one call that disagree in their lanes raise ValueError
        naming the blob's index before anything is launched.  The id words then go up, ops.ids_unpack validates and
        completes them into ids_restore on the device, and the records take the decompress_batch path; the ids
        status words are read with the coder's after everything is enqueued, and an image whose side information is
        corrupt (decoded harmlessly with the identity permutation) raises ValueError("side information of image b").
        Each blob states the quantiser step it was coded at (TMC: 1, TQC: its q; TPC: its base q,
        table and per-patch levels, §3.19); blobs of different steps and kinds decode together in one call, an image
        without a map taking a constant one.  A corrupt level section (decoded harmlessly with all levels zero) raises
        ValueError("side information of image b") like corrupt ids."""
        from . import bitstream

        blobs = list(blobs)
        if not blobs:
            raise ValueError("decode_bytes: no blobs")
        img, patch, K, L = self._geometry()
        parsed = []
        for i, blob in enumerate(blobs):
            try:
                p = bitstream.parse(blob)
            except ValueError as e:
                raise ValueError(f"blob {i}: {e}") from None
            if (p.img_size, p.patch_size, p.num_keep_patches) != (img, patch, K):
                raise ValueError(f"blob {i}: coded for img_size {p.img_size}, patch_size {p.patch_size}, "
                                 f"num_keep_patches {p.num_keep_patches}; this model has {img}, {patch}, {K}")
            if parsed and (p.lanes, p.z_lanes) != (parsed[0].lanes, parsed[0].z_lanes):
                raise ValueError(f"blob {i}: lanes ({p.lanes}, {p.z_lanes}) differ from blob 0's "
                                 f"({parsed[0].lanes}, {parsed[0].z_lanes}): decode them in separate calls")
            parsed.append(p)
        x_hat = self._decode_sections([p.ids for p in parsed], [p.z for p in parsed], [p.y for p in parsed],
                                      parsed[0].lanes, parsed[0].z_lanes, "decode_bytes", [p.q for p in parsed],
                                      [(p.nlev, p.offsets, p.levels) for p in parsed])
        return {"x_hat": x_hat, "orig_sizes": [p.orig_size for p in parsed]}

    def encode_image(self, rgb_u8, overlap=32, lanes=1, z_lanes=None, tile_batch=16, q=None, target_bytes=None,
                     qoffsets=None, rdoq=None):
        """an image at its own resolution -> one TMT file (bitstream.assemble_image).  rgb_u8: uint8
        [H, W, 3], numpy or tensor (a host image is uploaded once).  The image is cut into overlapping model-sized
        tiles (tiling.py; overlap 0..img_size // 2) and every chunk of tile_batch tiles (the last may be smaller)
        goes through ops.tile_cut_u8, scores.image_scores of the tiles' gray and the encode_bytes path, a batch of
        tiles being a batch of images; a tile's bytes in the file are the id / z / y sections of its encode_bytes
        blob.  Same preconditions and ValueErrors as compress_batch.

        q: one ladder position for every tile of the file (compress_batch's q as an int); q != 0 gives a TQT file
        that records it, q = 0 or None the TMT file as before.  target_bytes instead picks the smallest q whose
        whole file is at most that many bytes, by the lower-bound bisection of encode_bytes on the file size (at
        most 7 probes); here every probe codes the image anew, analysis included, and an image that
        does not fit at q = 32 gets its q = 32 file.  q together with target_bytes raises ValueError.

        qoffsets: compress_batch's table of ladder offsets; every tile's kept patches get their
        levels from the tile's own scores and the file becomes a TPT file with that one table, q (or the q that
        target_bytes picks) its base position.

        rdoq: compress_batch's weight as one float for every tile of the file, the same in every
        probe of target_bytes; the file is of the same kind and decode_image / decode_region read it as they are."""
        from . import bitstream, tiling
        from .coder import check_lanes
        from .scores import image_scores

        x = torch.from_numpy(np.ascontiguousarray(rgb_u8)) if isinstance(rgb_u8, np.ndarray) else rgb_u8
        if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() != 3 or x.shape[2] != 3:
            what = f"{tuple(x.shape)} {x.dtype}" if torch.is_tensor(x) else type(rgb_u8).__name__
            raise ValueError(f"encode_image: the image must be uint8 [H, W, 3], got {what}")
        img, patch, K, _ = self._geometry()
        H, W = int(x.shape[0]), int(x.shape[1])
        if H >= 1 << 16 or W >= 1 << 16:
            raise ValueError(f"encode_image: {W}x{H} pixels do not fit the file's u16 size fields")
        g = tiling.grid(H, W, img, overlap)
        tile_batch = int(tile_batch)
        if not 1 <= tile_batch < 1 << 16:
            raise ValueError(f"encode_image: tile_batch {tile_batch} outside 1..65535")
        lanes, z_lanes = check_lanes(lanes), check_lanes(1 if z_lanes is None else z_lanes)
        if q is not None and target_bytes is not None:
            raise ValueError("encode_image: give q or target_bytes, not both")
        q = 0 if q is None else bitstream.check_q(q, "encode_image: q")
        qm = self._check_qoffsets(qoffsets, None, 1, 1, "encode_image")
        if rdoq is not None and np.ndim(rdoq) != 0:
            raise ValueError("encode_image: rdoq is one weight for every tile of the file")
        rdoq = self._check_rdoq(rdoq, 1, "encode_image")
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise ValueError("MCM.encode_image runs on the MI355X kernels: move the model to the GPU")
        x = x.to(dev).contiguous()

        def code(qv):
            ids, zs, ys, lvs = [], [], [], []
            for t0 in range(0, g.T, tile_batch):
                tiles, gray = ops.tile_cut_u8(x, img, g.O, t0, min(tile_batch, g.T - t0))
                _, _, i, z, y, lv = self._encode_sections(tiles, image_scores(gray, img, patch), lanes, z_lanes, qv, qm,
                                                          None if rdoq is None else rdoq[0])
                ids.append(i)
                lvs.append(lv)
                zs += list(z)
                ys += list(y)
            return bitstream.assemble_image(img, K, patch, lanes, z_lanes, g.O, W, H, tile_batch, np.concatenate(ids),
                                            zs, ys, qv, *(() if qm is None else (qm[0], np.concatenate(lvs))))

        if target_bytes is None:
            return code(q)
        target, lo, hi, best, last = int(target_bytes), bitstream.Q_MIN, bitstream.Q_MAX + 1, None, None
        while lo < hi:  # the smallest q that fits; hi = Q_MAX + 1 stands for "none does" and is never probed
            mid = (lo + hi) // 2
            last = code(mid)
            if len(last) <= target:
                best, hi = last, mid
            else:
                lo = mid + 1
        return last if best is None else best  # none fits: the last probe was q = 32

    def decode_image(self, blob, tile_batch=None, out="f32"):
        """inverse of encode_image -> f32 [3, H, W] (out="f32") or uint8 [H, W, 3] (out="u8", the f32 image through
        clamp(0, 1).mul(255).round()).  The file is parsed on the host first (bitstream.parse_image): a malformed
        one, or one of another geometry than this model's, raises ValueError before anything is launched.  The tiles
        are decoded in chunks of tile_batch (None: the file's chunk, the encoder's batching) through the
        decode_bytes path into one [T, 3, S, S] buffer, which one ops.tile_blend turns into the image.  A corrupt
        tile raises ValueError naming its index in the file."""
        import re

        from . import bitstream

        if out not in ("f32", "u8"):
            raise ValueError(f"decode_image: out must be 'f32' or 'u8', got {out!r}")
        p = bitstream.parse_image(blob)
        img, patch, K, _ = self._geometry()
        if (p.img_size, p.patch_size, p.num_keep_patches) != (img, patch, K):
            raise ValueError(f"coded for img_size {p.img_size}, patch_size {p.patch_size}, "
                             f"num_keep_patches {p.num_keep_patches}; this model has {img}, {patch}, {K}")
        n = p.chunk if tile_batch is None else int(tile_batch)
        if n < 1:
            raise ValueError(f"decode_image: tile_batch {n} must be >= 1")
        T, tiles = p.num_tiles, None
        for t0 in range(0, T, n):
            t1 = min(t0 + n, T)
            try:
                x_hat = self._decode_sections(p.ids[t0:t1], p.z[t0:t1], p.y[t0:t1], p.lanes, p.z_lanes,
                                              "decode_image", p.q,
                                              None if p.nlev == 1 else [(p.nlev, p.offsets, lv)
                                                                        for lv in p.levels[t0:t1]])
            except ValueError as e:  # the batch path names the image of its call: that is tile t0 + b of the file
                raise ValueError(re.sub(r"\bimage (\d+)", lambda m: f"tile {t0 + int(m.group(1))}", str(e), count=1)
                                 ) from None
            if tiles is None:
                tiles = torch.empty((T,) + tuple(x_hat.shape[1:]), dtype=torch.float32, device=x_hat.device)
            tiles[t0:t1].copy_(x_hat)
        return ops.tile_blend(tiles, p.height, p.width, p.overlap, out=out)

    def decode_region(self, src, x0, y0, w, h, out="f32", tile_batch=None):
        """the window [x0, x0 + w) x [y0, y0 + h) of decode_image's image, bit for bit, from the tiles that window
        needs alone -> f32 [3, h, w] (out="f32") or uint8 [h, w, 3] ("u8").  src: the TMT file as
        a bytes-like object or a seekable binary file object, of which only the header, the table and those tiles'
        bytes are read (bitstream.read_image_index / read_tiles).  The tiles tiling.region_tiles names are decoded
        in chunks of tile_batch (None: the file's chunk) through the decode_bytes path into a compact buffer and
        blended by one ops.tile_blend_crops.  A malformed file, one of another geometry or a window that is not
        inside the image raises ValueError before anything is launched; a corrupt tile among the needed ones raises
        ValueError naming its index in the file, and one the window does not need is never read."""
        return self._decode_windows([src], [(x0, y0)], (w, h), out, tile_batch, "decode_region")[0]

    def decode_crops(self, srcs, origins, size, out="f32", tile_batch=16):
        """R windows of one size = (w, h) from TMT files, windows r at origins[r] = (x0, y0) of srcs[r] -> f32
        [R, 3, h, w] or uint8 [R, h, w, 3], each window decode_region's.  srcs may hold the same object several
        times: per distinct source the union of the tiles its windows need is read and decoded once.  The tiles of
        all sources are batched together in chunks of tile_batch (sources coded with other lanes in batches of
        their own, files of different quantiser steps, with a per-patch table or without, in one batch) and one
        ops.tile_blend_crops produces all
        windows.  ValueErrors as decode_region, naming the source by its first position in srcs; the sources of one
        call must agree in their overlap."""
        srcs, origins = list(srcs), list(origins)
        if len(srcs) != len(origins):
            raise ValueError(f"decode_crops: {len(srcs)} sources but {len(origins)} origins: one of each per window")
        if not srcs:
            raise ValueError("decode_crops: no windows")
        return self._decode_windows(srcs, origins, size, out, tile_batch, "decode_crops")

    def _decode_windows(self, srcs, origins, size, out, tile_batch, who):
        """decode_region / decode_crops: index every distinct source, list the tiles its windows need, decode them
        grouped by lanes into one compact [N, 3, S, S] buffer (slot = position in that order), blend all windows"""
        import re

        from . import bitstream, tiling

        if out not in ("f32", "u8"):
            raise ValueError(f"{who}: out must be 'f32' or 'u8', got {out!r}")
        many = who == "decode_crops"
        img, patch, K, _ = self._geometry()
        n = None if tile_batch is None else int(tile_batch)
        if n is not None and n < 1:
            raise ValueError(f"{who}: tile_batch {n} must be >= 1")
        # distinct sources by identity, in order of appearance; where: a source's first position in srcs
        first, where, index, grids, need, windows = {}, [], [], [], [], []
        for r, (src, (x0, y0)) in enumerate(zip(srcs, origins)):
            k = first.get(id(src))
            try:
                if k is None:
                    p = bitstream.read_image_index(src)
                    if (p.img_size, p.patch_size, p.num_keep_patches) != (img, patch, K):
                        raise ValueError(f"coded for img_size {p.img_size}, patch_size {p.patch_size}, "
                                         f"num_keep_patches {p.num_keep_patches}; this model has {img}, {patch}, {K}")
                    if index and p.overlap != index[0].overlap:
                        raise ValueError(f"overlap {p.overlap} differs from source 0's {index[0].overlap}: decode "
                                         f"them in separate calls")
                    k = first[id(src)] = len(index)
                    where.append(r)
                    index.append(p)
                    grids.append(tiling.grid(p.height, p.width, p.img_size, p.overlap))
                    need.append(set())
                need[k].update(tiling.region_tiles(grids[k], x0, y0, size[0], size[1]))
            except ValueError as e:
                raise ValueError(f"source {r}: {e}" if many else str(e)) from None
            windows.append((k, int(x0), int(y0)))
        # the jobs: (source, tile) in slot order, sources of equal lanes next to each other
        jobs = []
        for lanes in sorted({(p.lanes, p.z_lanes) for p in index}):
            jobs += [(k, t) for k, p in enumerate(index) if (p.lanes, p.z_lanes) == lanes for t in sorted(need[k])]
        slots = [[-1] * g.T for g in grids]
        for s, (k, t) in enumerate(jobs):
            slots[k][t] = s
        sections = {}
        for k, p in enumerate(index):
            tiles_k = sorted(need[k])
            got = bitstream.read_tiles(srcs[where[k]], p, tiles_k)
            for j, t in enumerate(tiles_k):  # a file with a map has a fourth list, the level words
                sections[k, t] = (got[0][j], got[1][j], got[2][j], got[3][j] if p.nlev > 1 else None)
        n = index[0].chunk if n is None else n
        job_lanes = [(index[k].lanes, index[k].z_lanes) for k, _ in jobs]
        tiles, s0 = None, 0
        while s0 < len(jobs):  # chunks of at most n jobs of equal lanes
            lanes = job_lanes[s0]
            s1 = s0 + 1
            while s1 < min(s0 + n, len(jobs)) and job_lanes[s1] == lanes:
                s1 += 1
            part = [sections[j] for j in jobs[s0:s1]]
            try:
                x_hat = self._decode_sections([a[0] for a in part], [a[1] for a in part], [a[2] for a in part],
                                              lanes[0], lanes[1], who, [index[k].q for k, _ in jobs[s0:s1]],
                                              [(index[k].nlev, index[k].offsets, a[3])
                                               for (k, _), a in zip(jobs[s0:s1], part)])
            except ValueError as e:  # the batch path names the image of its call: that is job s0 + b

                def name(m, s0=s0):
                    k, t = jobs[s0 + int(m.group(1))]
                    return f"tile {t} of source {where[k]}" if many else f"tile {t}"

                raise ValueError(re.sub(r"\bimage (\d+)", name, str(e), count=1)) from None
            if tiles is None:
                tiles = torch.empty((len(jobs),) + tuple(x_hat.shape[1:]), dtype=torch.float32, device=x_hat.device)
            tiles[s0:s1].copy_(x_hat)
            s0 = s1
        images = [(g.H, g.W, slots[k]) for k, g in enumerate(grids)]
        return ops.tile_blend_crops(tiles, images, windows, size, index[0].overlap, out=out)


class _LazyStreams(collections.abc.Mapping):
    """_Executor.last_streams of compress_batch: the keys compress sets, as host arrays copied from the device on
    first use (the batch path itself never copies the symbols to the host)"""

    def __init__(self, **tensors):
        self._t, self._h = tensors, {}

    def __getitem__(self, key):
        if key not in self._h:
            self._h[key] = self._t[key].cpu().numpy()
        return self._h[key]

    def __iter__(self):
        return iter(self._t)

    def __len__(self):
        return len(self._t)


def _interleave(layers):
    out = []
    for j, l in enumerate(layers):
        out.append(l)
        if j < len(layers) - 1:
            out.append(nn.GELU())
    return out


# ====================================================================================== executor
class _Executor:
    """Prepared weights + persistent workspaces for one (batch, dtype, device); `run` enqueues the
    whole forward on the current stream (graph-capturable: no host sync, no allocation-dependent
    control flow).

    LIC slice loop restructure (exact up to f32 summation order):
      * the first conv of every cc_transform_mean/scale and lrp_transform stack sees
        cat(latent_{means,scales}, y_hat slices): its latent-channel part is the same input for all 12
        slices, so it is computed for all slices up front as two big convs (N = 3 * 12 * 224) into the
        partial-sum buffer P; each slice's first conv then only contracts the y_hat channels and adds
        its P block in the epilogue;
      * the mean and scale stacks of a slice run as one batched launch per layer;
      * slices 6..11 all condition on y_hat slices 0..5 (max_support_slices = 6, MCM.py:73, 756-758),
        so their mean/scale stacks, Gaussian likelihoods and lrp stacks run batched (12 / 6 problems).
    """

    # reference paths the tests compare the fused LIC launches against (bitwise / bounded): False selects the
    # per-layer conv launches (the f32 parity path's structure) or the unchained serial slices
    USE_LIC_STACK = True
    USE_LIC_CHAIN = True
    USE_LIC_LATENT = True  # False: the latent partial sums on the halo conv (conv_halo.h)

    def __init__(self, m: MCM, batch, dtype, device):
        self.m, self.batch, self.dtype, self.device = m, batch, dtype, device
        self._sig = None
        B = batch
        E, Dd, M, N, S = m.encoder_embed_dim, m.decoder_embed_dim, m.latent_depth, m.hyperprior_depth, m.num_slices
        K = m.num_keep_patches
        P = m.encoder_embed.patch_size[0]
        self.img = m.encoder_embed.img_size[0]
        self.P, self.L = P, m.encoder_embed.num_patches
        self.g = g = int(round(K ** 0.5))
        if g * g != K:
            raise ValueError(f"num_keep_patches={K} must be a perfect square (MCM.py:729-732 views it as sqrt x sqrt)")
        self.hz = ((g + 1) // 2 + 1) // 2  # two stride-2 convs
        if self.hz * 4 != g:
            raise ValueError(f"sqrt(num_keep_patches)={g} must be a multiple of 4 so h_s returns to the y grid")
        self.sw = M // S
        self.maxsup = S // 2
        # the coder's scale bound, read once here: the forward at a quantiser step must not read the device back
        gc = m.gaussian_conditional
        self.scale_bound = float(gc.scale_bound) if gc.scale_bound is not None else 0.11
        self.nb = S - self.maxsup  # slices sharing the full support (batched)
        f32, dt = torch.float32, dtype
        dev = device

        def z(*shape, dtype=f32):
            return torch.empty(shape, dtype=dtype, device=dev)

        Te, Td = K + 1, self.L + 1
        Mp = B * g * g
        self.Mp = Mp
        hid_e = m.encoder_blocks[0].mlp.fc1.out_features if m.encoder_depth else 4 * E
        hid_d = m.decoder_blocks[0].mlp.fc1.out_features if m.decoder_depth else 4 * Dd
        self.tok = z(B * Te, E)
        self.enc_s = BlockScratch(B * Te, E, hid_e, dt, dev)
        self.enc_out = z(B * K, E, dtype=dt)
        ga = [l.out_channels for l in m.g_a if isinstance(l, nn.Conv2d)]
        self.ga_buf = [z(B * K, c, dtype=dt) for c in ga[:-1]]
        self.Y32 = z(Mp, M)
        self.YT = self.Y32 if dt == f32 else z(Mp, M, dtype=dt)
        ha = [l.out_channels for l in m.h_a if isinstance(l, nn.Conv2d)]
        res = [g, g, (g + 1) // 2, (g + 1) // 2, self.hz]
        self.ha_buf = [z(B * r * r, c, dtype=dt) for c, r in zip(ha[:-1], res[:-1])]
        self.Z = z(B * self.hz * self.hz, N)
        self.ZLIK = z(B, N, self.hz, self.hz)
        self.ZHAT = z(B * self.hz * self.hz, N, dtype=dt)
        self.eb_table = z(N, 59)
        self.zero_loss = torch.zeros((), device=device)  # the loss terms of distortion="none" (never written)
        hs_out = [m.h_s_mean[0].out_channels, m.h_s_mean[2][0].out_channels // 4, m.h_s_mean[4].out_channels,
                  m.h_s_mean[6][0].out_channels // 4]
        hs_res = [self.hz, 2 * self.hz, 2 * self.hz, g]
        # h_s_scale / h_s_mean run as one 2-problem launch per layer: [scale, mean] slabs
        self.hs_buf = [z(2, B * r * r, c, dtype=dt) for c, r in zip(hs_out, hs_res)]
        self.LSM = z(2, Mp, M, dtype=dt)
        self.LS, self.LM = self.LSM[0], self.LSM[1]
        self.mid = [l.out_channels for l in m.cc_transform_mean[0] if isinstance(l, nn.Conv2d)]
        c0 = self.mid[0]
        self.PW = 3 * S * c0  # partial sums: [mean (S*c0) | lrp (S*c0) | scale (S*c0)]
        self.Pbuf = z(Mp, self.PW)
        # side stream for the partial sums under the serial slice steps (_slices)
        self.overlap = torch.device(dev).type == "cuda"
        self.side_stream = torch.cuda.Stream(device=dev) if self.overlap else None
        self.SUPY = z(Mp, M, dtype=dt)    # y_hat slices (post-LRP for i < maxsup; pre-LRP for the batched ones)
        self.YPRE = z(Mp, M)              # f32 pre-LRP y_hat = round(y - mu) + mu
        self.YH = z(Mp, M, dtype=dt)      # final y_hat (g_s input)
        nb = self.nb
        self.CM = [z(2, nb, Mp, c, dtype=dt) for c in self.mid[:-1]]
        self.MUSIG = z(2, nb, Mp, self.sw)
        # chained serial slices (mean stack + lrp stack in one launch): every serial slice's mu / sigma kept
        # for the one deferred likelihood launch after the slice loop
        self.MS_SER = z(2, S, Mp, self.sw)
        self.CL = [z(nb, Mp, c, dtype=dt) for c in self.mid[:-1]]
        self.YLIK = z(B, M, g, g)
        gs = [l.out_channels for l in m.g_s if isinstance(l, nn.ConvTranspose2d)]
        self.gs_buf = [z(B * K, c, dtype=dt) for c in gs]
        self.dec = z(B * Td, Dd)
        self.dec_s = BlockScratch(B * Td, Dd, hid_d, dt, dev)
        self.dn = z(B * self.L, Dd, dtype=dt)

    # ------------------------------------------------------------------ weights
    def refresh_weights(self):
        sig = tuple((p.data_ptr(), p._version) for p in self.m.parameters())
        if sig == self._sig:
            return
        self._sig = sig
        m, dt = self.m, self.dtype
        M, S, sw, ms = m.latent_depth, m.num_slices, self.sw, self.maxsup

        def cast(t):
            t = t.detach()
            return (t if dt == torch.float32 else t.to(dt)).contiguous()

        def cw(w, lo=None, hi=None):  # conv weight [Cout][Cin][3][3] -> [Cout][3][3][Cin slice]
            w = w.detach()
            if lo is not None:
                w = w[:, lo:hi]
            return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)

        self.w_pe = cast(m.encoder_embed.proj.weight.view(m.encoder_embed.proj.weight.shape[0], -1))
        self.enc_w = [BlockWeights.from_block(b, dt) for b in m.encoder_blocks]
        self.dec_w = [BlockWeights.from_block(b, dt) for b in m.decoder_blocks]
        self.ga_w = [(cast(l.weight.view(l.weight.shape[0], -1)), l.bias.detach())
                     for l in m.g_a if isinstance(l, nn.Conv2d)]
        self.gs_w = [(cast(l.weight.view(l.weight.shape[0], -1).t()), l.bias.detach())
                     for l in m.g_s if isinstance(l, nn.ConvTranspose2d)]
        self.ha_w = [(cast(cw(l.weight)), l.bias.detach(), l.stride[0]) for l in m.h_a if isinstance(l, nn.Conv2d)]

        def hs_convs(seq):  # (conv, followed by PixelShuffle) of h_s_mean / h_s_scale
            out = []
            for l in seq:
                if isinstance(l, nn.Conv2d):
                    out.append((l, False))
                elif isinstance(l, nn.Sequential):
                    out.append((l[0], True))
            return out

        # [scale, mean] weights / biases of each layer stacked for the 2-problem launch
        self.hs2_w = [(cast(torch.stack([cw(s.weight), cw(mn.weight)])),
                       torch.stack([s.bias, mn.bias]).detach().contiguous(), ps)
                      for (s, ps), (mn, _) in zip(hs_convs(m.h_s_scale), hs_convs(m.h_s_mean))]

        def convs(seq):
            return [l for l in seq if isinstance(l, nn.Conv2d)]

        mean = [convs(s) for s in m.cc_transform_mean]
        scale = [convs(s) for s in m.cc_transform_scale]
        lrp = [convs(s) for s in m.lrp_transform]
        # latent-channel parts of every first conv: [mean | lrp] from latent_means, scale from latent_scales
        self.w_pre_ml = cast(torch.cat([cw(mean[i][0].weight, 0, M) for i in range(S)]
                                       + [cw(lrp[i][0].weight, 0, M) for i in range(S)]))
        self.w_pre_s = cast(torch.cat([cw(scale[i][0].weight, 0, M) for i in range(S)]))
        # the same latent parts in fragment order, one block per stack [mean | lrp | scale] x slices (tmae_lic_latent)
        c0 = self.mid[0]
        self.w_lat = None
        if dt == torch.bfloat16 and self.USE_LIC_LATENT and ops.lic_latent_fits(self.g, M) and c0 % 32 == 0:
            self.w_lat = torch.stack([ops.pack_lic_stack_weight(t[i][0].weight[:, :M])
                                      for t in (mean, lrp, scale) for i in range(S)]).contiguous()
        # per-slice y_hat-channel parts + the remaining layers, packed for batched launches
        self.ms_first, self.ms_layers, self.lrp_first, self.lrp_layers = [], [], [], []
        for i in range(ms):
            ny = sw * i
            self.ms_first.append((cast(torch.stack([cw(mean[i][0].weight, M, M + ny), cw(scale[i][0].weight, M, M + ny)])),
                                  torch.stack([mean[i][0].bias, scale[i][0].bias]).detach().contiguous()))
            self.ms_layers.append([(cast(torch.stack([cw(mean[i][j].weight), cw(scale[i][j].weight)])),
                                    torch.stack([mean[i][j].bias, scale[i][j].bias]).detach().contiguous())
                                   for j in range(1, 5)])
            self.lrp_first.append((cast(cw(lrp[i][0].weight, M, M + ny + sw)), lrp[i][0].bias.detach()))
            self.lrp_layers.append([(cast(cw(lrp[i][j].weight)), lrp[i][j].bias.detach()) for j in range(1, 5)])
        bs = range(ms, S)
        ny = sw * ms
        self.b_ms_first = (cast(torch.stack([torch.stack([cw(t[i][0].weight, M, M + ny) for i in bs])
                                             for t in (mean, scale)])),
                           torch.stack([torch.stack([t[i][0].bias for i in bs]) for t in (mean, scale)]).detach()
                           .contiguous())
        self.b_ms_layers = [(cast(torch.stack([torch.stack([cw(t[i][j].weight) for i in bs]) for t in (mean, scale)])),
                             torch.stack([torch.stack([t[i][j].bias for i in bs]) for t in (mean, scale)]).detach()
                             .contiguous()) for j in range(1, 5)]
        self.b_lrp_first = (cast(torch.stack([cw(lrp[i][0].weight, M, M + ny + sw) for i in bs])),
                            torch.stack([lrp[i][0].bias for i in bs]).detach().contiguous())
        self.b_lrp_layers = [(cast(torch.stack([cw(lrp[i][j].weight) for i in bs])),
                              torch.stack([lrp[i][j].bias for i in bs]).detach().contiguous()) for j in range(1, 5)]
        # fused slice-transform stacks (lic_stack.hip): every layer packed in MFMA fragment order, problems
        # stacked like the per-layer launches above; bf16 only, shapes that fit one workgroup's LDS
        self.lstk = None
        if (dt == torch.bfloat16 and self.USE_LIC_STACK and sw % 8 == 0
                and ops.lic_stack_fits(self.g, sw * (ms + 1), self.mid)):
            pk = ops.pack_lic_stack_weight

            def packs(convs, lo=None, hi=None):  # [layer] -> packed weights of one stack
                return [pk(c.weight[:, lo:hi] if j == 0 else c.weight) for j, c in enumerate(convs)]

            def stk(ts):  # stack problems' packed weights per layer
                return [torch.stack(list(layer)).contiguous() for layer in zip(*ts)]

            L = {"ms": [], "lrp": []}
            for i in range(ms):
                ny = sw * i
                L["ms"].append(stk([packs(mean[i], M, M + ny), packs(scale[i], M, M + ny)]))
                L["lrp"].append(packs(lrp[i], M, M + ny + sw))
            if S > ms:
                ny = sw * ms
                L["b_ms"] = [torch.stack([a_, b_]).contiguous() for a_, b_ in
                             zip(stk([packs(mean[i], M, M + ny) for i in bs]), stk([packs(scale[i], M, M + ny) for i in bs]))]
                L["b_lrp"] = stk([packs(lrp[i], M, M + ny + sw) for i in bs])
            self.lstk = L
        self.w_de = cast(m.decoder_embed.weight)
        # decoder_pred rows in channel-planar order: the unpatchify epilogue stores whole pixel runs
        pp = m.encoder_embed.patch_size[0]
        perm = ops.pred_channel_planar_perm(pp, m.encoder_embed.proj.in_channels)
        pred_cp = pp % 8 == 0
        self.pred_cp = pred_cp
        self.w_dp = cast(m.decoder_pred.weight[perm.to(m.decoder_pred.weight.device)] if pred_cp
                         else m.decoder_pred.weight)
        self.b_dp = (m.decoder_pred.bias[perm.to(m.decoder_pred.bias.device)] if pred_cp
                     else m.decoder_pred.bias).detach().contiguous()
        # the unpermuted (py, px, c) rows for the token-layout output of the decode stage
        self.w_dp_tok = cast(m.decoder_pred.weight) if pred_cp else self.w_dp

    # ------------------------------------------------------------------ forward
    def _check_imgs(self, imgs):
        imgs = imgs.float().contiguous()
        if imgs.shape[1:] != (self.m.encoder_embed.proj.in_channels, self.img, self.img):
            raise ValueError(f"Input image size {tuple(imgs.shape[2:])} doesn't match model ({self.img})")
        return imgs

    def run(self, imgs, scores, training, noise, q=None, qm=None, qm_chain=False):
        """q: None, B ladder positions (uploaded once, before the first launch) or an int32 [B] device tensor; qm:
        MCM._check_qoffsets' pair (eval only): the slice loop then runs at a step per kept patch, unchained as the
        coders run it, or with qm_chain (forward_qmap) chained with the map in the launches' cqm"""
        m, B = self.m, self.batch
        qd = self._q_dev(q)
        if qm is not None:
            qm = self._map_upload(qm)
        M, N, g, hz = m.latent_depth, m.hyperprior_depth, self.g, self.hz
        imgs = self._check_imgs(imgs)
        if training:
            if noise is not None:
                z_noise, y_noise = (t.float().contiguous() for t in noise)
            else:
                z_noise = torch.empty((B, N, hz, hz), device=self.device).uniform_(-0.5, 0.5)
                y_noise = torch.empty((B, M, g, g), device=self.device).uniform_(-0.5, 0.5)
        else:
            z_noise = y_noise = None

        # the likelihoods are returned to the caller: fresh tensors per forward (no copy of the executor's)
        self.ZLIK = torch.empty_like(self.ZLIK)
        self.YLIK = torch.empty_like(self.YLIK)
        shuf, rest = self._front(imgs, scores)

        # ---- entropy bottleneck + z_hat (MCM.py:741-744)
        ops.eb_likelihood(m.entropy_bottleneck, self.Z, B, N, hz * hz, noise=z_noise, lik=self.ZLIK, zhat=self.ZHAT,
                          table=self.eb_table)

        # ---- h_s (MCM.py:747-748)
        self._h_s()

        # ---- slice loop (MCM.py:751-787)
        if qm is None:
            self._slices(self._gc_forward(y_noise, qd), chain_ok=True, cq=qd)
        else:
            qmap, lstatus = self._encode_map(qm, scores, shuf, qd)
            self._slices(self._gc_forward(y_noise, None, qmap), chain_ok=qm_chain, cqm=qmap)

        x_hat = self._back(shuf, imgs.shape[1])
        if qm is not None and lstatus is not None:
            self._raise_levels(lstatus.cpu().numpy(), "forward")
        return {"x_hat": x_hat, "y": self.YLIK, "z": self.ZLIK, "ids_restore": rest,
                "ids_shuffle": shuf}

    # ------------------------------------------------------------------ compress / decompress
    def compress(self, imgs, scores):
        """MCM.compress (MCM.py:805-894): the eval forward's analysis path with symbol/index outputs, then
        the host rANS coder: one z string per image, ONE y string for the whole batch (slice-major)."""
        from .coder import BufferedRansEncoder

        B, hz = self.batch, self.hz
        eb, gc = self.m.entropy_bottleneck, self.m.gaussian_conditional
        zsym, sym, idx, rest = self._analysis(imgs, scores)
        zsym_h, sym_h, idx_h = zsym.cpu().numpy(), sym.cpu().numpy(), idx.cpu().numpy()
        self.last_streams = {"z_symbols": zsym_h, "y_symbols": sym_h, "y_indexes": idx_h}  # rate diagnostics
        zidx = eb._channel_indexes(hz * hz)
        z_strings = [eb._code(zsym_h[b].reshape(-1), zidx) for b in range(B)]
        enc = BufferedRansEncoder()
        enc.encode_with_indexes(sym_h, idx_h, *gc.host_tables())
        return {"string": [[enc.flush()], z_strings], "shape": torch.Size([hz, hz]), "ids_restore": rest}

    def decompress(self, strings, shape, ids_restore):
        """MCM.decompress (MCM.py:896-968): z strings -> z_hat -> h_s -> slice loop decoding each slice's
        symbols from the y string with indexes built on the device -> g_s -> decoder."""
        from .coder import RansDecoder

        m, B = self.m, self.batch
        N, hz = m.hyperprior_depth, self.hz
        eb = m.entropy_bottleneck
        if tuple(int(v) for v in shape) != (hz, hz):
            raise ValueError(f"shape {tuple(shape)} does not match this model's z grid ({hz}, {hz})")
        zidx = eb._channel_indexes(hz * hz)
        zsym = np.stack([eb._decode(s, zidx) for s in strings[1]]).astype(np.int32)
        ops.eb_dequantize(eb, torch.from_numpy(zsym).to(self.device), B, N, hz * hz, self.ZHAT, table=self.eb_table)
        self._h_s()
        decoder = RansDecoder()
        decoder.set_stream(strings[0][0])
        self._slices(self._gc_decompress(decoder))
        shuf = ops.invert_permutation(ids_restore.to(self.device))
        return self._back(shuf, m.encoder_embed.proj.in_channels)

    def _q_dev(self, q):
        """the per-image ladder positions on the device (int32 [B], one upload) or None for the plain kernels"""
        if q is None or torch.is_tensor(q):
            return q
        return torch.tensor(q, dtype=torch.int32).to(self.device)

    def _rdo_dev(self, rdoq):
        """the per-image weights of the rate-distortion optimised quantisation on the device (float32 [B], one upload)
        with the counters of moved symbols (int32 [B]) and the tables the decision reads, or None for today's kernels"""
        if rdoq is None:
            return None
        gc = self.m.gaussian_conditional
        _, sizes, offsets = gc.device_tables(self.device)
        return SimpleNamespace(w=torch.tensor(rdoq, dtype=torch.float32).to(self.device),
                               rate=gc.device_rate_table(self.device), sizes=sizes, offsets=offsets,
                               changed=torch.zeros(self.batch, dtype=torch.int32, device=self.device))

    # ------------------------------------------------------------------ per-patch quantiser steps
    def _map_upload(self, qm):
        """MCM._check_qoffsets' pair with everything of it that lives on the host uploaded (before the first launch)
        -> (offsets tuple, "scores" | int32 device tensor, device offsets [B, 16], whether the device checks the map)"""
        from .bitstream import offsets_row

        offs, src = qm[0], qm[1]
        rows = qm[2] if len(qm) > 2 else None  # forward_qmap's _rows: already on the device (a captured forward)
        if rows is None:
            rows = torch.tensor([offsets_row(offs)] * self.batch, dtype=torch.int32).to(self.device)
        on_device = torch.is_tensor(src)
        if isinstance(src, np.ndarray):
            src = torch.from_numpy(src).to(self.device)
        return offs, src, rows, on_device

    def _select_levels(self, qm, scores, shuf):
        """the levels of the kept patches -> (levels int32 [B, K], status int32 [B] or None when nothing can be wrong)"""
        offs, src, _, on_device = qm
        K = self.m.num_keep_patches
        if isinstance(src, str):
            levels, _ = ops.qlevels_select(shuf, K, len(offs), scores=scores.float().contiguous())
            return levels, None
        levels, status = ops.qlevels_select(shuf, K, len(offs), level_map=src)
        return levels, status if on_device else None

    def _encode_map(self, qm, scores, shuf, qd):
        """levels from the scores or the caller's map, then the map of clamped ladder positions at the base qd ->
        (qmap int32 [B, K], status or None); the levels stay in self.last_levels for the side information"""
        self.last_levels, status = self._select_levels(qm, scores, shuf)
        return ops.qmap_build(self.last_levels, qd, qm[2]), status

    @staticmethod
    def _raise_levels(status, who):
        for b in np.flatnonzero(status):
            raise ValueError(f"{who}: qlevels of image {int(b)}: a level outside its table of offsets")

    def decode_map(self, qm, ids_restore):
        """decompress_batch's qoffsets / qlevels -> the dict its executor method takes: levels in kept order as they
        are, a map in image patch order gathered by ids_shuffle"""
        offs, src, rows, on_device = self._map_upload(qm)
        K = self.m.num_keep_patches
        status = None
        if src.shape[1] == K:
            levels = src
        else:
            shuf = ops.invert_permutation(ids_restore.to(self.device))
            levels, status = ops.qlevels_select(shuf, K, len(offs), level_map=src)
        return dict(levels=levels, status=status if on_device else None, offsets=rows, who="qlevels")

    def _analysis(self, imgs, scores, qd=None, qm=None, rdo=None):
        """the eval forward's analysis path with symbol / index outputs -> (zsym [B][N][hz*hz], y sym and idx
        [slice][image][channel][pixel], ids_restore), all on the device; qd: _q_dev's positions; qm: _map_upload's
        tuple, the levels' status then in self.last_levels_status"""
        zsym, rest = self._analysis_head(imgs, scores)
        qmap = None
        if qm is not None:
            qmap, self.last_levels_status = self._encode_map(qm, scores, self.last_ids_shuffle, qd)
        sym, idx = self._analysis_slices(qd, qmap, rdo)
        return zsym, sym, idx, rest

    def _analysis_head(self, imgs, scores):
        """everything of _analysis that does not depend on the y quantiser step: encoder, g_a, h_a, z and h_s ->
        (zsym, ids_restore)"""
        m, B = self.m, self.batch
        N, hz = m.hyperprior_depth, self.hz
        eb = m.entropy_bottleneck
        shuf, rest = self._front(self._check_imgs(imgs), scores)
        self.last_ids_shuffle = shuf  # encode_bytes packs its kept ids as the blobs' side information
        # z: symbols round(z - median); z_hat = symbols + median (= EB.decompress of its own strings)
        ops.eb_likelihood(eb, self.Z, B, N, hz * hz, lik=self.ZLIK, zhat=self.ZHAT, table=self.eb_table)
        zsym = ops.eb_symbols(eb, self.Z, B, N, hz * hz, table=self.eb_table)
        self._h_s()
        return zsym, rest

    def _analysis_slices(self, qd=None, qmap=None, rdo=None):
        """the slice loop of _analysis on what _analysis_head left (Y32, the h_s outputs) -> (sym, idx); it may be
        run again at another qd or qmap (int32 [B, K], which takes precedence): nothing it reads is written by it.
        rdo: _rdo_dev's, whose counters of moved symbols are zeroed here and then hold this run's"""
        m, B = self.m, self.batch
        S, sw, HW = m.num_slices, self.sw, self.g * self.g
        sym = torch.empty(S * B * sw * HW, dtype=torch.int32, device=self.device)
        idx = torch.empty_like(sym)
        if rdo is not None:
            rdo.changed.zero_()
        self._slices(self._gc_compress(sym, idx, qd, qmap, rdo))
        return sym, idx

    def _code_z(self, zsym, z_lanes):
        m, B, hz = self.m, self.batch, self.hz
        nz = m.hyperprior_depth * hz * hz
        return self._encoder().encode_records(zsym, (0, nz), self._z_indexes(), (0, 0), B, 1, nz,
                                              m.entropy_bottleneck.device_tables(), z_lanes, what="z stream of image")

    def _code_y(self, sym, idx, lanes):
        m, B, per = self.m, self.batch, self.sw * self.g * self.g
        return self._encoder().encode_records(sym, (B * per, per), idx, (B * per, per), B, m.num_slices, per,
                                              m.gaussian_conditional.device_tables(), lanes, what="y stream of image")

    def _encoder(self):
        from .coder import DeviceRansEncoder

        enc = self.__dict__.get("_dev_encoder")
        if enc is None:
            enc = self._dev_encoder = DeviceRansEncoder()
        return enc

    def compress_batch(self, imgs, scores, lanes=1, z_lanes=1, q=None, qm=None, rdoq=None):
        """compress with the device coder: the same symbol / index buffers, coded as one y and one z record per
        image (image b's y stream = its [slice][channel][pixel] symbols) of lanes / z_lanes lanes
        (coder.encode_record); one lane is the plain stream, the reference's batch-1 format B times.  q: None or B
        ladder positions, uploaded once before the first launch; qm: MCM._check_qoffsets' pair
        (§3.19); rdoq: None or B weights, uploaded with q (§3.21)"""
        hz = self.hz
        qd = self._q_dev(q)
        rdo = self._rdo_dev(rdoq)
        if qm is not None:
            qm = self._map_upload(qm)
        zsym, sym, idx, rest = self._analysis(imgs, scores, qd, qm, rdo)
        z_strings = self._code_z(zsym, z_lanes)
        y_strings = self._code_y(sym, idx, lanes)
        self.last_streams = _LazyStreams(z_symbols=zsym, y_symbols=sym, y_indexes=idx,  # rate diagnostics
                                         **({} if rdo is None else {"y_changed": rdo.changed}))
        out = {"string": [y_strings, z_strings], "shape": torch.Size([hz, hz]), "ids_restore": rest}
        if rdoq is not None:
            out["rdoq"] = list(rdoq)
        if qm is not None:
            if self.last_levels_status is not None:
                self._raise_levels(self.last_levels_status.cpu().numpy(), "compress_batch")
            out["qoffsets"], out["qlevels"] = qm[0], self.last_levels
        if lanes > 1 or z_lanes > 1:
            out["lanes"] = (lanes, z_lanes)
        return out

    def compress_batch_target(self, imgs, scores, lanes, z_lanes, targets, fixed_bytes, qm=None, rdoq=None):
        """compress_batch with per image the smallest q of the ladder at which fixed_bytes(q) + its z record + its y
        record is at most targets[b] -> (z records, y records, q per image).  Lower-bound bisection over Q_MIN..Q_MAX
        for all images at once (hi = Q_MAX + 1 stands for "no q fits" and is never probed): at most 7 probes, each the
        slice loop and the y coder at the images' current midpoints; the analysis head and the z records are done
        once.  An image's record is the one of its smallest successful probe; where none fits, of its last probe,
        which is q = Q_MAX.  The size is taken to be non-increasing in q.  qm (MCM._check_qoffsets' pair): q is the
        base position, the levels are selected once and the map is rebuilt per probe (tmae_qmap_build).  rdoq: None
        or B weights (§3.21), the same in every probe."""
        from .bitstream import Q_MAX, Q_MIN

        B = self.batch
        rdo = self._rdo_dev(rdoq)
        if qm is not None:
            qm = self._map_upload(qm)
        zsym, rest = self._analysis_head(imgs, scores)
        if qm is not None:
            self.last_levels, lstatus = self._select_levels(qm, scores, self.last_ids_shuffle)
        z_strings = self._code_z(zsym, z_lanes)
        lo, hi = [Q_MIN] * B, [Q_MAX + 1] * B
        kept = [None] * B  # (q, y record)
        while any(l < h for l, h in zip(lo, hi)):
            mid = [(l + h) // 2 if l < h else min(l, Q_MAX) for l, h in zip(lo, hi)]  # settled images: any valid q
            qd = self._q_dev(mid)
            sym, idx = self._analysis_slices(qd, None if qm is None else ops.qmap_build(self.last_levels, qd, qm[2]),
                                             rdo)
            y_strings = self._code_y(sym, idx, lanes)
            for b in range(B):
                if lo[b] >= hi[b]:
                    continue
                if fixed_bytes(mid[b]) + len(z_strings[b]) + len(y_strings[b]) <= targets[b]:
                    hi[b], kept[b] = mid[b], (mid[b], y_strings[b])
                else:
                    lo[b] = mid[b] + 1
                    if mid[b] == Q_MAX:
                        kept[b] = (Q_MAX, y_strings[b])
        if qm is not None and lstatus is not None:
            self._raise_levels(lstatus.cpu().numpy(), "encode_bytes")
        self.last_streams = _LazyStreams(z_symbols=zsym, y_symbols=sym, y_indexes=idx,  # of the last probe
                                         **({} if rdo is None else {"y_changed": rdo.changed}))
        return z_strings, [k[1] for k in kept], [k[0] for k in kept]

    def _z_indexes(self):
        """EntropyBottleneck channel indexes of one image's z symbols [C][hz*hz] on the device (shared by all images)"""
        zidx = self.__dict__.get("_zidx")
        if zidx is None:
            zidx = self.m.entropy_bottleneck._channel_indexes(self.hz * self.hz)
            zidx = self._zidx = torch.from_numpy(zidx).to(self.device)
        return zidx

    def decompress_batch(self, strings, shape, ids_restore, lanes=1, z_lanes=1, ids_status=None, q=None, qm=None):
        """decompress of per-image records: every string goes up in one copy, the z and y streams are decoded by
        device kernels (the y streams inside the slice loop, one call per slice step), and nothing synchronises with
        the host until the status words are read after the last kernel of _back has been enqueued.  ids_status
        (decode_bytes): ops.ids_unpack's device status words of ids_restore, read in that same copy.  q: None or B
        ladder positions (compress_batch's), uploaded before the first launch.  qm: dict of levels
        int32 [B, K], their device status words or None (read in the same copy) and offsets int32 [B, 16], all on the
        device; the map is built from them at the base q and the _qm kernels run"""
        from .bitstream import IDS_STATUS, LEVELS_STATUS
        from .coder import DeviceRansDecoder, _raise_status

        m, B = self.m, self.batch
        N, S, hz, sw, HW = m.hyperprior_depth, m.num_slices, self.hz, self.sw, self.g * self.g
        eb, gc = m.entropy_bottleneck, m.gaussian_conditional
        if tuple(int(v) for v in shape) != (hz, hz):
            raise ValueError(f"shape {tuple(shape)} does not match this model's z grid ({hz}, {hz})")
        # everything that touches the host comes first: tables, the scale bound, ids, then the one upload
        etabs, gtabs = eb.device_tables(), gc.device_tables()
        bound = float(gc.scale_bound) if gc.scale_bound is not None else 0.11
        zidx = self._z_indexes()
        rest = ids_restore.to(self.device)
        qd = self._q_dev(q)
        qmap = None if qm is None else ops.qmap_build(qm["levels"], qd, qm["offsets"])
        dec = DeviceRansDecoder()  # records [0, B): y, [B, 2B): z; a bad header raises here, before the first launch
        dec.set_records(list(strings[0]) + list(strings[1]), [lanes] * B + [z_lanes] * B, self.device,
                        what=[f"{c} stream of image {b}" for c in "yz" for b in range(B)])
        decode = dec.decode_records
        nz, per = N * hz * hz, B * sw * HW
        zsym = torch.empty((B, N, hz * hz), dtype=torch.int32, device=self.device)
        decode(B, B, zidx, (0, 0), zsym, (0, nz), 0, 1, nz, etabs)
        ops.eb_dequantize(eb, zsym, B, N, hz * hz, self.ZHAT, table=self.eb_table)
        self._h_s()
        idx = torch.empty(S * per, dtype=torch.int32, device=self.device)
        sym = torch.empty_like(idx)
        M, dt = m.latent_depth, self.dtype

        def step(i0, nbs, mu, sigma, ms_stride):
            if qmap is not None:
                ops.gc_indexes_qm(sigma, ms_stride, sw, B, HW, nbs, sw, gc.scale_table, bound, idx[i0 * per:], qmap)
            elif qd is None:
                ops.gc_indexes(sigma, ms_stride, sw, B, HW, nbs, sw, gc.scale_table, bound, idx[i0 * per:])
            else:
                ops.gc_indexes_q(sigma, ms_stride, sw, B, HW, nbs, sw, gc.scale_table, bound, idx[i0 * per:], qd)
            decode(0, B, idx, (per, sw * HW), sym, (per, sw * HW), i0, nbs, sw * HW, gtabs)
            if qmap is not None:
                ops.gc_dequantize_qm(sym[i0 * per:], mu, ms_stride, sw, B, HW, nbs, sw, i0 * sw, self.SUPY, dt, M,
                                     self.YPRE, M, qmap)
            elif qd is None:
                ops.gc_dequantize(sym[i0 * per:], mu, ms_stride, sw, B, HW, nbs, sw, i0 * sw, self.SUPY, dt, M,
                                  self.YPRE, M)
            else:
                ops.gc_dequantize_q(sym[i0 * per:], mu, ms_stride, sw, B, HW, nbs, sw, i0 * sw, self.SUPY, dt, M,
                                    self.YPRE, M, qd)

        self._slices(step)
        self.last_decoded = _LazyStreams(y_symbols=sym, y_indexes=idx)  # what the decoder saw (diagnostics, tests)
        shuf = ops.invert_permutation(rest)
        x_hat = self._back(shuf, m.encoder_embed.proj.in_channels)
        lstatus = None if qm is None else qm.get("status")
        extra = [t for t in (ids_status, lstatus) if t is not None]
        # the only synchronisation: after everything is enqueued
        status = dec.status(torch.cat([t.reshape(-1) for t in extra]) if extra else None)
        at = 2 * B
        if ids_status is not None:
            for b in np.flatnonzero(status[at:at + B]):
                c = int(status[at + b])
                raise ValueError(f"side information of image {int(b)}: {IDS_STATUS.get(c, f'status {c}')}")
            at += B
        if lstatus is not None:
            for b in np.flatnonzero(status[at:at + B]):
                c = int(status[at + b])
                if qm.get("who"):
                    self._raise_levels(status[at:at + B], "decompress_batch")
                raise ValueError(f"side information of image {int(b)}: {LEVELS_STATUS.get(c, f'status {c}')}")
        _raise_status(status[:B], "y stream of image")
        _raise_status(status[B:2 * B], "z stream of image")
        return x_hat

    def encode(self, imgs, scores):
        """the encoder stage alone (MCM.forward_encoder): -> (x_remain f32 [B, K, E], ids_restore), both fresh;
        encoder_norm writes f32 whatever the operand dtype"""
        m, B, K = self.m, self.batch, self.m.num_keep_patches
        _, rest = self._enc_blocks(self._check_imgs(imgs), scores)
        x = ops.layernorm(self.tok, m.encoder_norm.weight, m.encoder_norm.bias, m.encoder_norm.eps, torch.float32,
                          rows=B * K, row_group=K, group_stride=K + 1, row_offset=1)
        return x.view(B, K, -1), rest

    def decode(self, x_remain, ids_restore):
        """the decoder stage alone (MCM.forward_decoder) of x_remain [B, ntok, E]: -> preds f32 [B, L, p*p*C] (fresh)
        in the reference's (py, px, c) column order, decoder_pred as a plain linear over the norm output"""
        m, dt, B = self.m, self.dtype, self.batch
        shuf = ops.invert_permutation(ids_restore.to(self.device))
        x = x_remain.float().contiguous()
        self._dec_blocks(x.view(-1, x.shape[2]), shuf, x.shape[1])
        preds = ops.linear(self.dn, self.w_dp_tok, m.decoder_pred.bias.detach(), dt, out_dtype=torch.float32)
        return preds.view(B, self.L, -1)

    def _front(self, imgs, scores):
        """encoder + g_a + h_a (MCM.py:590-634, 729-739): tokens -> Y32/YT -> Z; returns (ids_shuffle, ids_restore)"""
        m, dt, B, K = self.m, self.dtype, self.batch, self.m.num_keep_patches
        Te = K + 1
        shuf, rest = self._enc_blocks(imgs, scores)
        ops.layernorm(self.tok, m.encoder_norm.weight, m.encoder_norm.bias, m.encoder_norm.eps, dt, rows=B * K,
                      row_group=K, group_stride=Te, row_offset=1, out=self.enc_out)
        return self._front_lic(shuf, rest)

    def _enc_blocks(self, imgs, scores):
        """ids, kept-patch embedding, cls row and the encoder blocks (MCM.py:590-630) -> self.tok; returns
        (ids_shuffle, ids_restore)"""
        m, dt, B = self.m, self.dtype, self.batch
        E, K, P = m.encoder_embed_dim, m.num_keep_patches, self.P
        Te = K + 1
        # ---- encoder (MCM.py:590-634): ids on device, embed only the kept patches
        shuf, rest = ops.ids_shuffle(scores, K, m.sum_lanes)
        pos_e = m.encoder_pos_embed.detach()
        ops.patch_embed(imgs, shuf, self.w_pe, m.encoder_embed.proj.bias.detach(), pos_e, self.tok, K, P, dt)
        ops.cls_rows(self.tok, m.cls_token.detach(), pos_e, B, Te, E)
        for w in self.enc_w:
            run_block(self.tok, w, B, Te, dt, self.enc_s)
        return shuf, rest

    def _front_lic(self, shuf, rest):
        """g_a + h_a on the encoder output (MCM.py:729-739)"""
        m, dt, B = self.m, self.dtype, self.batch
        M, g = m.latent_depth, self.g
        # ---- g_a: 1x1 convs on the token matrix (tokens in ids_keep order = the g x g grid, MCM.py:729-735)
        x = self.enc_out
        for j, (w, b) in enumerate(self.ga_w):
            last = j == len(self.ga_w) - 1
            if last:
                ops.linear(x, w, b, dt, out=self.YT, out32=None if self.YT is self.Y32 else self.Y32)
            else:
                ops.linear(x, w, b, dt, act=ops.ACT_GELU, out=self.ga_buf[j])
                x = self.ga_buf[j]

        # ---- h_a (MCM.py:739)
        H = g
        x, cin = self.YT, M
        for j, (w, b, stride) in enumerate(self.ha_w):
            last = j == len(self.ha_w) - 1
            out = self.Z if last else self.ha_buf[j]
            cout = w.shape[0]
            ops.conv3x3(x, cin, cin, B, H, H, w, b, out, cout, cout, dt, stride=stride,
                        act=ops.ACT_NONE if last else ops.ACT_GELU)
            H = (H + 2 - 3) // stride + 1
            x, cin = out, cout
        return shuf, rest

    def _back(self, shuf, in_chans):
        """g_s + decoder + unpatchify (MCM.py:636-688, 790-797) from YH; returns x_hat NCHW f32"""
        m, dt, B = self.m, self.dtype, self.batch
        K, L, P = m.num_keep_patches, self.L, self.P
        # ---- g_s (MCM.py:790-792): transposed 1x1 convs back to E-dim tokens
        x = self.YH
        for j, (w, b) in enumerate(self.gs_w):
            last = j == len(self.gs_w) - 1
            ops.linear(x, w, b, dt, act=ops.ACT_NONE if last else ops.ACT_GELU, out=self.gs_buf[j])
            x = self.gs_buf[j]

        # ---- decoder (MCM.py:636-688): embed + unshuffle (+ off-by-one cls), blocks, norm, pred+unpatchify
        self._dec_blocks(x, shuf, K)
        x_hat = torch.empty((B, in_chans, self.img, self.img), dtype=torch.float32, device=self.device)
        ops.decoder_pred(self.dn, self.w_dp, self.b_dp, x_hat, B, L, P, dt, channel_planar=self.pred_cp)
        return x_hat

    def _dec_blocks(self, x, shuf, ntok):
        """decoder_embed of x [B*ntok, E] (f32 or the operand dtype) + unshuffle (+ off-by-one cls), mask rows,
        blocks, decoder_norm without the cls rows (MCM.py:657-682) -> self.dn"""
        m, dt, B = self.m, self.dtype, self.batch
        Dd, L = m.decoder_embed_dim, self.L
        Td = L + 1
        pos_d = m.decoder_pos_embed.detach()
        ops.decoder_embed(x, self.w_de, m.decoder_embed.bias.detach(), pos_d, shuf, self.dec, B, ntok, L, dt)
        ops.mask_rows(self.dec, m.mask_token.detach(), pos_d, shuf, B, L, ntok, Dd)
        for w in self.dec_w:
            run_block(self.dec, w, B, Td, dt, self.dec_s)
        ops.layernorm(self.dec, m.decoder_norm.weight, m.decoder_norm.bias, m.decoder_norm.eps, dt, rows=B * L,
                      row_group=L, group_stride=Td, row_offset=1, out=self.dn)

    # ------------------------------------------------------------------ Gaussian-conditional slice steps
    # Each is called with (i0, nbs, mu, sigma, ms_stride): slices i0..i0+nbs-1, mu/sigma device addresses
    # of rows [Mp][sw] per slice, ms_stride elements apart; it must leave y_hat (pre-LRP) in SUPY (operand
    # dtype) and YPRE (f32) at channels i0*sw.. .
    def _gc_forward(self, y_noise, qd=None, qmap=None):
        """qd: per-image ladder positions on the device (the kernel at a step) or None; qmap: ladder
        positions per kept patch, int32 [B, K] (§3.19), which takes precedence"""
        M, sw, B, HW, dt = self.m.latent_depth, self.sw, self.batch, self.g * self.g, self.dtype
        bound = self.scale_bound

        def step(i0, nbs, mu, sigma, ms_stride):
            if qmap is not None:
                ops.gc_slices_fwd_qm(self.Y32, M, i0 * sw, mu, sigma, ms_stride, sw, y_noise, self.YLIK, M, self.SUPY,
                                     dt, M, self.YPRE, M, B, HW, nbs, sw, bound, qmap)
            elif qd is None:
                ops.gc_slices(self.Y32, M, i0 * sw, mu, sigma, ms_stride, sw, y_noise, self.YLIK, M, self.SUPY, dt, M,
                              self.YPRE, M, B, HW, nbs, sw)
            else:
                ops.gc_slices_fwd_q(self.Y32, M, i0 * sw, mu, sigma, ms_stride, sw, y_noise, self.YLIK, M, self.SUPY,
                                    dt, M, self.YPRE, M, B, HW, nbs, sw, bound, qd)
        return step

    def _gc_compress(self, sym, idx, qd=None, qmap=None, rdo=None):
        """eval step + int32 symbols / scale indexes in the coder's [slice][image][channel][pixel] order; qd: per-image
        ladder positions on the device (the _q kernel, which skips the likelihoods nobody reads here) or None; rdo:
        _rdo_dev's (the _rdo kernel for all three cases of the step) or None"""
        gc = self.m.gaussian_conditional
        M, sw, B, HW, dt = self.m.latent_depth, self.sw, self.batch, self.g * self.g, self.dtype
        table = gc.scale_table
        bound = float(gc.scale_bound) if gc.scale_bound is not None else 0.11
        per = B * sw * HW

        def step(i0, nbs, mu, sigma, ms_stride):
            if rdo is not None:
                ops.gc_slices_code_rdo(self.Y32, M, i0 * sw, mu, sigma, ms_stride, sw, None, M, self.SUPY, dt, M,
                                       self.YPRE, M, B, HW, nbs, sw, sym[i0 * per:], idx[i0 * per:], table, bound, qd,
                                       qmap, rdo.w, rdo.rate, rdo.sizes, rdo.offsets, rdo.changed)
            elif qmap is not None:
                ops.gc_slices_code_qm(self.Y32, M, i0 * sw, mu, sigma, ms_stride, sw, None, M, self.SUPY, dt, M,
                                      self.YPRE, M, B, HW, nbs, sw, sym[i0 * per:], idx[i0 * per:], table, bound, qmap)
            elif qd is None:
                ops.gc_slices_code(self.Y32, M, i0 * sw, mu, sigma, ms_stride, sw, self.YLIK, M, self.SUPY, dt, M,
                                   self.YPRE, M, B, HW, nbs, sw, sym[i0 * per:], idx[i0 * per:], table)
            else:
                ops.gc_slices_code_q(self.Y32, M, i0 * sw, mu, sigma, ms_stride, sw, None, M, self.SUPY, dt, M,
                                     self.YPRE, M, B, HW, nbs, sw, sym[i0 * per:], idx[i0 * per:], table, bound, qd)
        return step

    def _gc_decompress(self, decoder):
        """indexes on the device -> host rANS decode of the next slices' symbols -> y_hat = symbols + mu"""
        gc = self.m.gaussian_conditional
        M, sw, B, HW, dt = self.m.latent_depth, self.sw, self.batch, self.g * self.g, self.dtype
        cdf, sizes, offsets = gc.host_tables()
        bound = float(gc.scale_bound) if gc.scale_bound is not None else 0.11
        per = B * sw * HW
        idx_dev = torch.empty(self.m.num_slices * per, dtype=torch.int32, device=self.device)

        def step(i0, nbs, mu, sigma, ms_stride):
            n = nbs * per
            ops.gc_indexes(sigma, ms_stride, sw, B, HW, nbs, sw, gc.scale_table, bound, idx_dev)
            idx = idx_dev[:n].cpu().numpy()
            vals = decoder.decode_stream_array(idx, cdf, sizes, offsets)
            sym = torch.from_numpy(vals).to(self.device)
            ops.gc_dequantize(sym, mu, ms_stride, sw, B, HW, nbs, sw, i0 * sw, self.SUPY, dt, M, self.YPRE, M)
        return step

    def _h_s(self):
        """h_s_scale -> LS and h_s_mean -> LM (MCM.py:747-748): both stacks have the same shapes and read
        the same z_hat, so every layer is ONE launch of 2 problems ([scale, mean] weight / output slabs)"""
        B, dt = self.batch, self.dtype
        x, xs, cin, H = self.ZHAT, 0, self.m.hyperprior_depth, self.hz
        for j, (w, b, pshuf) in enumerate(self.hs2_w):
            last = j == len(self.hs2_w) - 1
            cout = w.shape[1]
            out = self.LSM if last else self.hs_buf[j]
            ops.conv3x3(x, cin, cin, B, H, H, w, b, out, out.shape[2], cout, dt,
                        act=ops.ACT_NONE if last else ops.ACT_GELU, pixel_shuffle=pshuf, nb=(1, 2),
                        strides={"x1": (0, xs), "w": (0, w[0].numel()), "b": (0, cout), "y": (0, out[0].numel())})
            if pshuf:
                H *= 2
                cin = cout // 4
            else:
                cin = cout
            x, xs = out, out[0].numel()

    def _slices(self, gc_step, chain_ok=False, cq=None, cqm=None):
        m, dt, B, g = self.m, self.dtype, self.batch, self.g
        M, S, sw, ms, nb, Mp = m.latent_depth, m.num_slices, self.sw, self.maxsup, self.nb, self.Mp
        mid = self.mid
        c0 = mid[0]
        Pw = self.PW
        Pb = self.Pbuf
        eP = Pb.element_size()
        pbase = Pb.data_ptr()
        off_mean, off_lrp, off_scale = 0, S * c0, 2 * S * c0
        esz = self.SUPY.element_size()
        supy, ypre, yh = self.SUPY.data_ptr(), self.YPRE.data_ptr(), self.YH.data_ptr()
        e4 = 4
        # latent-channel partial sums of the first convs of slices [i0, i1): mean + lrp (one 2-problem launch
        # on LM, weight / output slabs S*c0 apart) and scale (on LS)
        wrow = self.w_pre_ml[0].numel()

        def pre(i0, i1):
            if self.w_lat is not None:  # every stack's block of slices [i0, i1) in one launch
                nfs = c0 // 16
                ops.lic_latent(B, g, [self.LM, self.LM, self.LS], M, M, self.w_lat, nfs, self.w_lat[0].numel(),
                               [0, S * nfs, 2 * S * nfs], i0 * nfs, i1 * nfs, pbase, Pw)
                return
            n = (i1 - i0) * c0
            ops.conv3x3(self.LM, M, M, B, g, g, self.w_pre_ml[i0 * c0:], None, pbase + (off_mean + i0 * c0) * eP, Pw,
                        n, dt, y_f32=True, nb=(1, 2), strides={"w": (0, S * c0 * wrow), "y": (0, S * c0)})
            ops.conv3x3(self.LS, M, M, B, g, g, self.w_pre_s[i0 * c0:], None, pbase + (off_scale + i0 * c0) * eP,
                        Pw, n, dt, y_f32=True)

        # The serial slice steps run 64-256-workgroup launches that leave most CUs idle: the partial sums of
        # slices 1.. are computed on a side stream under them (fork / join by events, graph-capturable);
        # slice i's first conv waits only for its own group.  Slice 0's group runs first on the main stream.
        ready = {}
        groups = [(i, i + 1) for i in range(1, ms)] + ([(ms, S)] if nb > 0 else [])
        if self.overlap and groups:
            main = torch.cuda.current_stream()
            pre(0, 1)
            fork = torch.cuda.Event()
            fork.record(main)
            side = self.side_stream
            side.wait_event(fork)
            with torch.cuda.stream(side):
                for i0, i1 in groups:
                    pre(i0, i1)
                    ev = torch.cuda.Event()
                    ev.record(side)
                    ready[i0] = ev
        else:
            pre(0, S)

        def wait_pre(i0):
            if i0 in ready:
                torch.cuda.current_stream().wait_event(ready.pop(i0))

        cm = [t.data_ptr() for t in self.CM]
        cl = [t.data_ptr() for t in self.CL]
        musig = self.MUSIG.data_ptr()
        cm_s1 = [nb * Mp * c for c in mid[:-1]]
        ms_s1 = nb * Mp * sw

        def ms_stack(first, layers, x1, c1, i0, nbs):
            """mean+scale stacks for slices i0.. (nbs problems per type) -> MUSIG"""
            w, b = first
            ops.conv3x3(x1, c1, M, B, g, g, w, b, cm[0], c0, c0, dt, act=ops.ACT_GELU,
                        addend=pbase + (off_mean + i0 * c0) * eP, ld_add=Pw, nb=(2, nbs),
                        strides={"w": (w[0].numel(), w[0][0].numel() if nbs > 1 else 0),
                                 "b": (b[0].numel(), c0 if nbs > 1 else 0),
                                 "a": (off_scale - off_mean, c0), "y": (cm_s1[0], Mp * c0)})
            for j, (w, b) in enumerate(layers):
                cin, cout = mid[j], mid[j + 1]
                last = j == len(layers) - 1
                y = musig if last else cm[j + 1]
                ys1 = ms_s1 if last else cm_s1[j + 1]
                ops.conv3x3(cm[j], cin, cin, B, g, g, w, b, y, cout, cout, dt,
                            act=ops.ACT_NONE if last else ops.ACT_GELU, y_f32=last, nb=(2, nbs),
                            strides={"x1": (cm_s1[j], Mp * cin), "w": (w[0].numel(), w[0][0].numel() if nbs > 1 else 0),
                                     "b": (b[0].numel(), cout if nbs > 1 else 0), "y": (ys1, Mp * cout)})

        def ms_fused(i0, nbs):
            """mean+scale stacks of slices i0.. as ONE tmae_lic_stack launch (2 x nbs problems) -> MUSIG"""
            ws = self.lstk["b_ms"] if nbs > 1 else self.lstk["ms"][i0]
            first, layers = (self.b_ms_first, self.b_ms_layers) if nbs > 1 else (self.ms_first[i0], self.ms_layers[i0])
            bs_ = [first[1]] + [b for _, b in layers]
            st = {"a": (off_scale - off_mean, c0), "y": (ms_s1, Mp * sw)}
            for l, (w, b) in enumerate(zip(ws, bs_)):
                st[f"w{l}"] = (w[0].numel(), w[0][0].numel() if nbs > 1 else 0)
                st[f"b{l}"] = (b[0].numel(), b.shape[-1] if nbs > 1 else 0)
            ops.lic_stack(B, g, supy, sw * (ms if nbs > 1 else i0), M, ws, bs_, mid, musig, sw, True,
                          addend=pbase + (off_mean + i0 * c0) * eP, ld_add=Pw, nb=(2, nbs), strides=st)

        def lrp_fused(i0, nbs):
            """lrp stack(s) of slices i0.. as one tmae_lic_stack launch: y_hat = y_hat_pre + 0.5 tanh(lrp) -> YH"""
            ws = self.lstk["b_lrp"] if nbs > 1 else self.lstk["lrp"][i0]
            first, layers = (self.b_lrp_first, self.b_lrp_layers) if nbs > 1 else (self.lrp_first[i0], self.lrp_layers[i0])
            bs_ = [first[1]] + [b for _, b in layers]
            st = {"a": (0, c0), "y": (0, sw), "src": (0, sw), "x2": (0, sw)}
            for l, (w, b) in enumerate(zip(ws, bs_)):
                st[f"w{l}"] = (0, w[0].numel() if nbs > 1 else 0)
                st[f"b{l}"] = (0, b.shape[-1] if nbs > 1 else 0)
            if nbs > 1:  # shared slots 0..ms-1 + own pre-LRP slot
                x = dict(x2=supy + ms * sw * esz, c2=sw, ld2=M)
                c1 = sw * ms
            else:        # y_hat slots 0..i0 (contiguous); also the support slot
                x = dict(y2=supy + i0 * sw * esz, ldy2=M)
                c1 = sw * (i0 + 1)
            ops.lic_stack(B, g, supy, c1, M, ws, bs_, mid, yh + i0 * sw * esz, M, False,
                          addend=pbase + (off_lrp + i0 * c0) * eP, ld_add=Pw, lrp_src=ypre + i0 * sw * e4, ld_src=M,
                          nb=(1, nbs), strides=st, **x)

        def lrp_stack(first, layers, i0, nbs, x2=None):
            w, b = first
            if x2 is None:  # single slice i0: input = y_hat slots 0..i0 (contiguous)
                ops.conv3x3(supy, sw * (i0 + 1), M, B, g, g, w, b, cl[0], c0, c0, dt, act=ops.ACT_GELU,
                            addend=pbase + (off_lrp + i0 * c0) * eP, ld_add=Pw)
            else:           # batched slices: shared slots 0..ms-1 + own pre-LRP slot
                ops.conv3x3(supy, sw * ms, M, B, g, g, w, b, cl[0], c0, c0, dt, act=ops.ACT_GELU,
                            x2=x2, c2=sw, ld2=M, addend=pbase + (off_lrp + i0 * c0) * eP, ld_add=Pw, nb=(1, nbs),
                            strides={"x2": (0, sw), "w": (0, w[0].numel()), "b": (0, c0), "a": (0, c0),
                                     "y": (0, Mp * c0)})
            for j, (w, b) in enumerate(layers):
                cin, cout = mid[j], mid[j + 1]
                if j < len(layers) - 1:
                    ops.conv3x3(cl[j], cin, cin, B, g, g, w, b, cl[j + 1], cout, cout, dt, act=ops.ACT_GELU,
                                nb=(1, nbs), strides={"x1": (0, Mp * cin), "w": (0, w[0].numel() if nbs > 1 else 0),
                                                      "b": (0, cout if nbs > 1 else 0), "y": (0, Mp * cout)})
                else:  # y_hat = y_hat_pre + 0.5 tanh(lrp) -> YH (and the support slot for i < ms)
                    ops.conv3x3(cl[j], cin, cin, B, g, g, w, b, yh + i0 * sw * esz, M, cout, dt,
                                y_f32=(dt == torch.float32), lrp_src=ypre + i0 * sw * e4, ld_src=M,
                                y2=(supy + i0 * sw * esz) if nbs == 1 else None, ldy2=M, nb=(1, nbs),
                                strides={"x1": (0, Mp * cin), "w": (0, w[0].numel() if nbs > 1 else 0),
                                         "b": (0, cout if nbs > 1 else 0), "src": (0, sw), "y": (0, sw),
                                         "y2": (0, sw)})

        # slices 0..ms-1: serial (slice i conditions on y_hat 0..i-1)
        fused = self.lstk is not None
        # serial slices as ONE launch each: the mean stack's workgroups go on with the slice's lrp stack
        # (y_hat_pre = round(y - mu) + mu in between), the scale stacks run beside them; the slices' Gaussian
        # likelihoods follow the loop in one launch (nothing in the chain reads them)
        chain = fused and chain_ok and self.USE_LIC_CHAIN
        ms_ser = self.MS_SER.data_ptr()
        yv = self.Y32.data_ptr()

        def ms_chain(i):
            ws, (first, layers) = self.lstk["ms"][i], (self.ms_first[i], self.ms_layers[i])
            bs_ = [first[1]] + [b for _, b in layers]
            st = {"a": (off_scale - off_mean, c0), "y": (S * Mp * sw, 0)}
            for l, (w, b) in enumerate(zip(ws, bs_)):
                st[f"w{l}"] = (w[0].numel(), 0)
                st[f"b{l}"] = (b[0].numel(), 0)
            lw = self.lstk["lrp"][i]
            lb_ = [self.lrp_first[i][1]] + [b for _, b in self.lrp_layers[i]]
            ch = dict(w=lw, b=lb_, couts=mid, x1=supy, c1=sw * i, ld1=M, y=yv + i * sw * e4, ldy=M,
                      add=pbase + (off_lrp + i * c0) * eP, ld_add=Pw, ypre=ypre + i * sw * e4, ld_ypre=M,
                      out=yh + i * sw * esz, ld_out=M, out2=supy + i * sw * esz, ld_out2=M, q=cq, qm=cqm)
            ops.lic_stack(B, g, supy, sw * i, M, ws, bs_, mid, ms_ser + i * Mp * sw * e4, sw, True,
                          addend=pbase + (off_mean + i * c0) * eP, ld_add=Pw, nb=(2, 1), strides=st, chain=ch)

        for i in range(ms):
            wait_pre(i)
            if chain:
                ms_chain(i)
                continue
            if fused:
                ms_fused(i, 1)
            else:
                ms_stack(self.ms_first[i], self.ms_layers[i], supy, sw * i, i, 1)
            gc_step(i, 1, musig, musig + ms_s1 * e4, Mp * sw)
            if fused:
                lrp_fused(i, 1)
            else:
                lrp_stack(self.lrp_first[i], self.lrp_layers[i], i, 1)
        # slices ms..S-1: batched on the fixed support y_hat 0..ms-1 (chaining them into their lrp stacks as
        # well measured slower, round 3)
        if nb > 0:
            wait_pre(ms)
            if fused:
                ms_fused(ms, nb)
            else:
                ms_stack(self.b_ms_first, self.b_ms_layers, supy, sw * ms, ms, nb)
            gc_step(ms, nb, musig, musig + ms_s1 * e4, Mp * sw)
            if fused:
                lrp_fused(ms, nb)
            else:
                lrp_stack(self.b_lrp_first, self.b_lrp_layers, ms, nb, x2=supy + ms * sw * esz)
        if chain:  # likelihoods of the chained slices (overwrites their dead SUPY / YPRE slots)
            gc_step(0, ms, ms_ser, ms_ser + S * Mp * sw * e4, Mp * sw)
        for k in list(ready):  # join the side stream in every case
            wait_pre(k)
