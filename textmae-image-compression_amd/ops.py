"""Tensor-level wrappers over the C ABI (include/tmae.h).

Each wrapper checks device / dtype / contiguity on the host, then enqueues the HIP kernel on
torch's current stream.  They allocate outputs with torch (the caching allocator owns all memory,
the library never allocates) unless an `out=` buffer is passed.
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import torch

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, TMAE_BF16, TMAE_F32, ConvArgs, EBParams, LicStackArgs

__all__ = [
    "ids_shuffle", "layernorm", "linear", "linear_residual", "patch_embed", "cls_rows", "mha", "decoder_embed",
    "mask_rows", "decoder_pred", "conv3x3", "lic_stack", "pack_lic_stack_weight", "lic_stack_fits", "gc_slices", "eb_likelihood", "eb_aux_loss",
    "gc_likelihood", "nhwc_to_nchw", "bpp", "gemm_plan", "force_gemm_tile", "GEMM_TILES", "mha_plan", "mha_force_stream", "dtype_code", "gc_slices_code", "gc_indexes",
    "gc_dequantize", "gc_slices_fwd_q", "gc_slices_code_q", "gc_indexes_q", "gc_dequantize_q",
    "gc_slices_fwd_qm", "gc_slices_code_qm", "gc_indexes_qm", "gc_dequantize_qm", "gc_slices_code_rdo",
    "qlevels_select", "qlevels_pack", "qlevels_unpack", "qmap_build",
    "gc_pmf", "eb_pmf", "eb_symbols", "eb_dequantize", "invert_permutation", "mae_masking",
    "rans_stream_cap_words", "rans_encode_streams", "rans_pack_streams", "rans_decode_streams",
    "rans_encode_lanes", "rans_decode_lanes", "ids_pack", "ids_unpack",
    "resize_tables", "resize_u8", "rgb_to_gray_u8", "tile_cut_u8", "tile_blend", "tile_blend_crops",
    "mae_loss", "TMAE_F32", "TMAE_BF16", "ACT_NONE", "ACT_GELU",
]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    """device address of a tensor, a raw int address (offset views into a workspace), or None"""
    if t is None or isinstance(t, int):
        return t
    return t.data_ptr()


def _need(t: torch.Tensor, dtype=None, name="tensor"):
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device (HIP) tensor")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return TMAE_F32
    if dt == torch.bfloat16:
        return TMAE_BF16
    raise ValueError(f"unsupported compute dtype {dt}")


def gemm_plan(M: int, N: int, K: int, dtype: torch.dtype, batch: int = 1) -> str:
    """name of the MFMA GEMM variant the library launches for this problem (no device work)"""
    buf = ctypes.create_string_buffer(96)
    _lib.call("tmae_gemm_plan", M, N, K, batch, dtype_code(dtype), buf, len(buf))
    return buf.value.decode()


# tmae_gemm_force_tile's candidate list (gemm_core.h kTileCand): weight rows x token rows of a workgroup's tile
GEMM_TILES = ((256, 256), (128, 128), (64, 128), (32, 128), (64, 64), (32, 64), (256, 192), (128, 160), (128, 192))


@contextlib.contextmanager
def force_gemm_tile(index: int):
    """Test hook: every MFMA GEMM launched inside the block takes tile GEMM_TILES[index] where its path has it
    (tmae_gemm_force_tile); -1 = the chooser.  The previous value is restored on exit."""
    if not -1 <= index < len(GEMM_TILES):
        raise ValueError(f"force_gemm_tile: index {index} outside -1..{len(GEMM_TILES) - 1}")
    prev = _lib.value("tmae_gemm_force_tile", index)
    try:
        yield
    finally:
        _lib.value("tmae_gemm_force_tile", prev)


def mha_plan(T: int, dh: int, dtype: torch.dtype, backward: bool = False) -> str:
    """name of the attention kernel family tmae_mha_fwd / tmae_mha_fwd_lse (or tmae_mha_bwd) launches at this
    sequence length, with the streamed family's block and chunk sizes, e.g. "stream<bf16,dh64,q256,c128>"
    (no device work)"""
    buf = ctypes.create_string_buffer(96)
    _lib.call("tmae_mha_plan", T, dh, dtype_code(dtype), int(bool(backward)), buf, len(buf))
    return buf.value.decode()


@contextlib.contextmanager
def mha_force_stream(on: bool = True):
    """Test hook: every attention launch inside the block takes the streamed kernels (tmae_mha_force_stream),
    whatever the sequence length.  The previous value is restored on exit."""
    prev = _lib.value("tmae_mha_force_stream", int(bool(on)))
    try:
        yield
    finally:
        _lib.value("tmae_mha_force_stream", prev)


# --------------------------------------------------------------------------------------- masking
def ids_shuffle(scores: torch.Tensor, keep: int, sum_lanes: int = 8):
    """MCM.get_ids_shuffle + argsort (MCM.py:364-423, 579-580) -> (ids_shuffle, ids_restore) int64."""
    s = _need(scores.float().contiguous(), name="total_scores")
    n, L = s.shape
    shuf = torch.empty((n, L), dtype=torch.int64, device=s.device)
    rest = torch.empty_like(shuf)
    _lib.call("tmae_ids_shuffle", s.data_ptr(), shuf.data_ptr(), rest.data_ptr(), n, L, keep, sum_lanes, _stream())
    return shuf, rest


# --------------------------------------------------------------------------------------- transformer
def layernorm(x, weight, bias, eps, out_dtype, rows=None, row_group=None, group_stride=0, row_offset=0, out=None):
    _need(x, torch.float32, "x")
    D = x.shape[-1]
    rows = x.numel() // D if rows is None else rows
    row_group = rows if row_group is None else row_group
    if out is None:
        out = torch.empty((rows, D), dtype=out_dtype, device=x.device)
    _lib.call("tmae_layernorm_fwd", x.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(), rows, D,
              max(row_group, 1), group_stride, row_offset, float(eps), dtype_code(out.dtype), _stream())
    return out


def linear(x, w, b, dtype, act=ACT_NONE, out=None, out_dtype=None, M=None, ldx=None, row_group=None, group_stride=0,
           row_offset=0, out32=None):
    """y = act(x W^T + b); x f32 or `dtype`; W [N][K] in `dtype`."""
    N, K = w.shape
    M = x.numel() // x.shape[-1] if M is None else M
    ldx = x.shape[-1] if ldx is None else ldx
    out_dtype = out_dtype or dtype
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=x.device)
    code = dtype_code(dtype)
    x_f32 = int(x.dtype == torch.float32)
    if code == TMAE_BF16 and not x_f32 and x.dtype != torch.bfloat16:
        raise ValueError("x must be f32 or bf16")
    if code == TMAE_F32 and (x.dtype != torch.float32 or out.dtype != torch.float32):
        raise ValueError("f32 path needs f32 tensors")
    _lib.call("tmae_linear_fwd", x.data_ptr(), x_f32, ldx, row_group or M, group_stride, row_offset, w.data_ptr(),
              _p(b), out.data_ptr(), int(out.dtype == torch.float32), out.shape[-1], _p(out32),
              0 if out32 is None else out32.shape[-1], M, N, K, act, code, _stream())
    return out


def linear_residual(x, w, b, resid, dtype):
    N, K = w.shape
    M = x.numel() // K
    _lib.call("tmae_linear_residual_fwd", x.data_ptr(), K, w.data_ptr(), _p(b), resid.data_ptr(), resid.shape[-1], M,
              N, K, dtype_code(dtype), _stream())
    return resid


_PATCH_WORK: dict = {}


def patch_embed(imgs, ids_shuffle, w, b, pos, tokens, keep, patch, dtype, patches=None):
    """kept-patch embedding (+ pos) into tokens rows 1..keep of every image.  Patches whose rows are whole 16-B
    chunks (P % 8 == 0), and every patch size when `patches` is given, are gathered first (into `patches`
    [n*keep][Kw] of dtype -- the training forward keeps them for the weight gradient -- else a cached workspace;
    Kw = C*P*P rounded up to 8, zero tail) and projected by the LDS-DMA GEMM; otherwise (ViT-H's patch 14 at
    inference) they are gathered value by value inside the GEMM."""
    n, C, H, W = imgs.shape
    D = w.shape[0]
    L = ids_shuffle.shape[1]
    if w.dim() != 2 or w.shape[1] != -(-C * patch * patch // 8) * 8 or not w.is_contiguous():
        raise ValueError(f"patch_embed: weight {tuple(w.shape)} must be contiguous [D][C*P*P rounded up to 8]")
    Kw = w.shape[1]  # C*P*P rounded up to 8 (the gathered rows' zero tail: patch 14, 588 -> 592)
    if patch % 8 == 0 or patches is not None:
        if patches is None:
            key = (imgs.device, dtype, n * keep * Kw)
            patches = _PATCH_WORK.get(key)
            if patches is None:
                patches = _PATCH_WORK[key] = torch.empty((n * keep, Kw), dtype=dtype, device=imgs.device)
            _lib.call("tmae_patch_gather", _need(imgs, torch.float32, "imgs").data_ptr(), ids_shuffle.data_ptr(),
                      patches.data_ptr(), n, C, H, W, patch, L, keep, dtype_code(dtype), _stream())
        elif tuple(patches.shape) != (n * keep, Kw):
            raise ValueError(f"patch_embed: gathered patches {tuple(patches.shape)} must be [{n * keep}][{Kw}]")
        _lib.call("tmae_patch_embed_gathered", patches.data_ptr(), ids_shuffle.data_ptr(), w.data_ptr(), b.data_ptr(),
                  pos.data_ptr(), tokens.data_ptr(), n, Kw, D, L, keep, dtype_code(dtype), _stream())
        return tokens
    _lib.call("tmae_patch_embed_fwd", _need(imgs, torch.float32, "imgs").data_ptr(), ids_shuffle.data_ptr(),
              w.data_ptr(), b.data_ptr(), pos.data_ptr(), tokens.data_ptr(), n, C, H, W, patch, D, L, keep,
              dtype_code(dtype), _stream())
    return tokens


def cls_rows(tokens, cls, pos, n, rows_per_img, D):
    _lib.call("tmae_cls_rows", tokens.data_ptr(), cls.data_ptr(), pos.data_ptr(), n, rows_per_img, D, _stream())


def mha(qkv, B, T, H, dh, scale, dtype, out=None):
    if out is None:
        out = torch.empty((B * T, H * dh), dtype=dtype, device=qkv.device)
    _lib.call("tmae_mha_fwd", qkv.data_ptr(), out.data_ptr(), B, T, H, dh, float(scale), dtype_code(dtype), _stream())
    return out


_QKV_ATTN_OK = {}


def qkv_attn_supported(T, H, dh, dtype):
    """a fused qkv + attention kernel exists for this shape (bf16 only)"""
    if dtype != torch.bfloat16:
        return False
    key = (T, H, dh)
    if key not in _QKV_ATTN_OK:
        _QKV_ATTN_OK[key] = bool(_lib.value("tmae_qkv_attn_supported", T, H, dh))
    return _QKV_ATTN_OK[key]


def qkv_attn(x, w, b, B, T, H, dh, scale, dtype, out):
    """out = attention(x W_qkv^T + b_qkv) in one launch, Q / K / V kept on chip (tmae_qkv_attn_fwd)"""
    _lib.call("tmae_qkv_attn_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), B, T, H, dh, float(scale),
              dtype_code(dtype), _stream())
    return out


def decoder_embed(x, w, b, pos, ids_shuffle, out, n, ntok, L, dtype):
    D, Din = w.shape
    _lib.call("tmae_decoder_embed_fwd", x.data_ptr(), int(x.dtype == torch.float32), w.data_ptr(), b.data_ptr(),
              pos.data_ptr(), ids_shuffle.data_ptr(), out.data_ptr(), n, ntok, L, Din, D, dtype_code(dtype),
              _stream())


def mask_rows(out, mask_token, pos, ids_shuffle, n, L, ntok, D):
    _lib.call("tmae_mask_rows", out.data_ptr(), mask_token.data_ptr(), pos.data_ptr(), ids_shuffle.data_ptr(), n, L,
              ntok, D, _stream())


def decoder_pred(x, w, b, imgs, n, L, patch, dtype, channel_planar=False):
    """channel_planar: w / b rows already in (c, py, px) order (see pred_channel_planar_perm)"""
    N, Din = w.shape
    C, H, W = imgs.shape[1:]
    _lib.call("tmae_decoder_pred_cp_fwd" if channel_planar else "tmae_decoder_pred_fwd", x.data_ptr(), w.data_ptr(),
              b.data_ptr(), imgs.data_ptr(), n, L, Din, C, H, W, patch, dtype_code(dtype), _stream())


def pred_channel_planar_perm(patch, chans):
    """row permutation taking decoder_pred rows (py, px, c) (MCM.py:524-546 "nhwpqc") to (c, py, px)"""
    return torch.arange(patch * patch * chans).view(patch, patch, chans).permute(2, 0, 1).reshape(-1)


# --------------------------------------------------------------------------------------- LIC
def conv3x3(x1, c1, ld1, n, H, W, w, b, y, ldy, cout, dtype, stride=1, act=ACT_NONE, pixel_shuffle=False,
            x2=None, c2=0, ld2=0, y_f32=None, y32=None, ld32=0, addend=None, ld_add=0, lrp_src=None, ld_src=0,
            y2=None, ldy2=0, nb=(1, 1), strides=None, pre=None, ldp=0):
    """Batched 3x3 conv (tmae_conv3x3).  Pointer arguments: tensors or raw device addresses.
    `strides` maps operand name (x1, x2, w, b, y, y32, a, src, y2, pre) -> (s1, s2) element strides for the
    nb[0] x nb[1] problems.  `pre` (training): pre-activation copy in the output's dtype / layout (the last
    lrp conv: f32 pre-tanh rows ldp apart)."""
    a = ConvArgs()
    a.x1, a.c1, a.ld1 = _p(x1), c1, ld1
    a.x2, a.c2, a.ld2 = _p(x2), c2, ld2
    a.n, a.H, a.W, a.stride = n, H, W, stride
    a.w, a.bias = _p(w), _p(b)
    a.cout, a.act, a.pixel_shuffle = cout, act, int(pixel_shuffle)
    if dtype == torch.float32:
        y_f32 = True  # the f32 path writes f32 everywhere
    elif y_f32 is None:
        y_f32 = isinstance(y, torch.Tensor) and y.dtype == torch.float32
    a.y, a.y_f32, a.ldy = _p(y), int(y_f32), ldy
    a.y32, a.ld32 = _p(y32), ld32
    a.addend, a.ld_add = _p(addend), ld_add
    a.lrp_src, a.ld_src = _p(lrp_src), ld_src
    a.y2, a.ldy2 = _p(y2), ldy2
    a.pre, a.ldp = _p(pre), ldp
    a.nb1, a.nb2 = nb
    for name, (s1, s2) in (strides or {}).items():
        setattr(a, f"{name}_s1", s1)
        setattr(a, f"{name}_s2", s2)
    _lib.call("tmae_conv3x3", ctypes.byref(a), dtype_code(dtype), _stream())


LSTK_MAXC, LSTK_MAXPIX = 224, 144  # lic_stack.hip: widest resident activation, pixels per workgroup


def _pad(c, m):
    return (c + m - 1) // m * m


def lic_stack_fits(G, cin0, couts):
    """True when tmae_lic_stack takes a stack of this shape (grid G x G, layer-0 input cin0 channels,
    output channels per layer): bf16 operands, activations resident in one workgroup's LDS"""
    return (G * G <= LSTK_MAXPIX and cin0 % 8 == 0 and _pad(cin0, 32) <= LSTK_MAXC and 1 <= len(couts) <= 5
            and all(c % 8 == 0 for c in couts) and all(_pad(c, 32) <= LSTK_MAXC for c in couts[:-1]))


def pack_lic_stack_weight(w: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """Conv weight [Cout][Cin][3][3] -> tmae_lic_stack's MFMA fragment order
    [tap 9][k-step Cin/32][cout fragment Cout/16][lane 64][8] (lane = 16 * k-group + cout row), zero-padded
    to multiples of 32 input / 16 output channels (flat, `dtype`)"""
    w = w.detach()
    co, ci = w.shape[:2]
    cip, cop = _pad(ci, 32), _pad(co, 16)
    t = torch.zeros(9, cop, cip, dtype=torch.float32, device=w.device)
    if ci:
        t[:, :co, :ci] = w.float().permute(2, 3, 0, 1).reshape(9, co, ci)
    nkc, nfr = cip // 32, cop // 16
    t = t.view(9, nfr, 16, nkc, 4, 8).permute(0, 3, 1, 4, 2, 5).contiguous()
    return t.view(-1).to(dtype)


def pack_lic_stack_weight_t(w: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """A 3x3 conv weight [Cout][Cin][3][3] as the weight of its transposed conv (the data gradient: input Cout
    channels, output Cin, taps flipped) in tmae_lic_stack's fragment order (relayout mode 4 builds the same)"""
    return pack_lic_stack_weight(w.detach().transpose(0, 1).flip(2, 3), dtype)


def lic_stack_bwd(n, G, dtop, ldt, c_top, weights, couts, pres, outs, nb=(1, 1), strides=None, routes=None):
    """The data-gradient chain of a slice stack's layers L-1..1 in one launch (tmae_lic_stack, TMAE_LIC_STACK_BWD):
    dtop [rows][c_top] (bf16, rows ldt apart) is the gradient of the stack's output; layer l (the transposed conv
    of forward layer L-1-l, weights[l] from pack_lic_stack_weight_t) writes outs[l] = (its conv) * GELU'(pres[l]),
    bf16 [rows][couts[l]].  `strides` maps x1, w<l>, s<l> (pres[l] / outs[l]) -> per-problem (s1, s2).
    routes (optional, one list per problem of (acc_f32, ld, ncols), <= 3 consecutive channel ranges): the last
    layer is the stack's first conv's input gradient, added into those accumulators (no pres / outs entry)."""
    a = LicStackArgs()
    if routes is not None:
        if nb[1] != 1:
            # the kernel steps routed accumulators by problem index along nb1 only
            raise ValueError("lic_stack_bwd routes: nb2 must be 1")
        if len(routes) > 1 and len(routes) != nb[0]:
            raise ValueError("lic_stack_bwd routes: one route list per problem")
        lim = 0
        for r in range(3):
            if r < len(routes[0]):
                acc, ld, nc = routes[0][r]
                a.racc[r], a.rld[r] = _p(acc), ld
                if len(routes) > 1 and nc:
                    steps = [_p(routes[k + 1][r][0]) - _p(routes[k][r][0]) for k in range(len(routes) - 1)]
                    if len(set(steps)) != 1 or steps[0] % 4:
                        raise ValueError("lic_stack_bwd routes: accumulators not at a constant stride")
                    a.rs[r] = steps[0] // 4  # problem k's accumulator = problem 0's + k * stride (f32 elements)
                lim += nc
            a.rlim[r] = lim
    a.n, a.G, a.nlayers = n, G, len(couts)
    a.nb1, a.nb2 = nb
    a.x1, a.c1, a.ld1 = _p(dtop), c_top, ldt
    a.flags = 2
    for l, (w, c) in enumerate(zip(weights, couts)):
        a.w[l], a.cout[l] = _p(w), c
        if l < len(pres):
            a.sv_pre[l], a.sv_act[l] = _p(pres[l]), _p(outs[l])
    for name, (s1, s2) in (strides or {}).items():
        if name[0] == "w":
            a.w_s[int(name[1:])][:] = (s1, s2)
        elif name[0] == "s":
            a.sv_s[int(name[1:])][:] = (s1, s2)
        else:
            getattr(a, f"{name}_s")[:] = (s1, s2)
    _lib.call("tmae_lic_stack", ctypes.byref(a), _stream())


def lic_latent_fits(G, cin):
    """True when tmae_lic_latent takes the latent partial sums of this shape (bf16, cin a multiple of 32)"""
    return G * G <= LSTK_MAXPIX and cin % 32 == 0 and 32 <= cin <= 384


def lic_latent(n, G, xs, ldx, cin, w, nfr, blk, f_off, f_lo, f_hi, y, ldy, y_s=None, biases=None, act=ACT_NONE,
               y_bf16=False):
    """Stride-1 3x3 conv with the input resident in LDS (tmae_lic_latent): for problem j, relative fragment r in
    [f_lo, f_hi): y + y_s[j] (elements), columns 16 r .. = act(bias_j + the conv of xs[j]'s channels [0, cin) with
    the packed weight fragments f_off[j] + r of w: blocks of nfr fragments blk elements apart (pack_lic_stack_weight,
    stacked)).  y_s defaults to 16 f_off[j] (the latent partial sums' column blocks).  Pointers: tensors or raw
    addresses."""
    a = _lib.LicLatentArgs()
    a.n, a.G, a.cin, a.nb = n, G, cin, len(xs)
    for j, (x, fo) in enumerate(zip(xs, f_off)):
        a.x[j] = _p(x)
        a.f_off[j] = fo
        a.y_s[j] = (16 * fo) if y_s is None else y_s[j]
        a.bias[j] = _p(biases[j]) if biases is not None else None
    a.ldx, a.w, a.nfr, a.blk = ldx, _p(w), nfr, blk
    a.f_lo, a.f_hi = f_lo, f_hi
    a.y, a.ldy = _p(y), ldy
    a.act, a.y_bf16 = act, int(y_bf16)
    _lib.call("tmae_lic_latent", ctypes.byref(a), _stream())


def lic_stack(n, G, x1, c1, ld1, weights, biases, couts, y, ldy, y_f32, x2=None, c2=0, ld2=0, addend=None, ld_add=0,
              lrp_src=None, ld_src=0, y2=None, ldy2=0, nb=(1, 1), strides=None, chain=None, save=None):
    """One slice-transform stack per (problem, image) (tmae_lic_stack).  weights: packed per layer
    (pack_lic_stack_weight, problems stacked); `strides` maps operand (x1, x2, w0..w4, b0..b4, a, y, src, y2)
    -> (s1, s2) element strides of the nb[0] x nb[1] problems.  Pointers: tensors or raw addresses.
    save (training): {"layers": [(pre, act, (s1, s2)) per non-last layer], "t": pre-tanh f32, "t_s": (s1, s2),
    "chain": [(pre, act, s) per lrp layer], "chain_t": ..., "chain_t_s": s} -- what the HIP backward reads."""
    a = LicStackArgs()
    a.n, a.G, a.nlayers = n, G, len(couts)
    a.nb1, a.nb2 = nb
    a.x1, a.c1, a.ld1 = _p(x1), c1, ld1
    a.x2, a.c2, a.ld2 = _p(x2), c2, ld2
    for l, (w, b, c) in enumerate(zip(weights, biases, couts)):
        a.w[l], a.bias[l], a.cout[l] = _p(w), _p(b), c
    a.addend, a.ld_add = _p(addend), ld_add
    a.y, a.y_f32, a.ldy = _p(y), int(y_f32), ldy
    a.lrp_src, a.ld_src = _p(lrp_src), ld_src
    a.y2, a.ldy2 = _p(y2), ldy2
    if chain is not None:  # the mean problem goes on with its slice's lrp stack (TMAE_LIC_STACK_CHAIN)
        a.flags = 1
        a.cn = len(chain["couts"])
        for l, (w, b, c) in enumerate(zip(chain["w"], chain["b"], chain["couts"])):
            a.cw[l], a.cb[l], a.ccout[l] = _p(w), _p(b), c
        a.cx1, a.cc1, a.cld1 = _p(chain["x1"]), chain["c1"], chain["ld1"]
        a.yv, a.ldyv = _p(chain["y"]), chain["ldy"]
        a.cadd, a.cld_add = _p(chain["add"]), chain["ld_add"]
        a.csrc, a.cld_src = _p(chain["ypre"]), chain["ld_ypre"]
        a.cy, a.cldy = _p(chain["out"]), chain["ld_out"]
        a.cy2, a.cldy2 = _p(chain.get("out2")), chain.get("ld_out2", 0)
        a.cq = _q_ptr(chain.get("q"), n)  # per-image quantiser step of y_hat_pre or None
        if chain.get("qm") is not None:  # a step per pixel of the grid: int32 [n, G * G]
            a.cqm = _qmap_ptr(chain["qm"], n, G * G)
        cs = chain.get("strides", {})  # per-slice (b2) element strides of the chain operands
        a.cs_x1, a.cs_yv, a.cs_src = cs.get("x1", 0), cs.get("y", 0), cs.get("ypre", 0)
        a.cs_add, a.cs_y, a.cs_y2 = cs.get("add", 0), cs.get("out", 0), cs.get("out2", 0)
        for l in range(a.cn):
            a.cs_w[l], a.cs_b[l] = cs.get(f"w{l}", 0), cs.get(f"b{l}", 0)
    for name, (s1, s2) in (strides or {}).items():
        if name[0] in "wb" and name[1:].isdigit():
            getattr(a, f"{name[0]}_s")[int(name[1:])][:] = (s1, s2)
        else:
            getattr(a, f"{name}_s")[:] = (s1, s2)
    if save is not None:  # training: per layer (pre, act, (s1, s2)) of the problems, and the lrp pre-tanh t
        for l, (pre, act, st) in enumerate(save.get("layers", [])):
            a.sv_pre[l], a.sv_act[l] = _p(pre), _p(act)
            a.sv_s[l][:] = st
        if save.get("t") is not None:
            a.sv_t = _p(save["t"])
            a.sv_t_s[:] = save.get("t_s", (0, 0))
        for l, (pre, act, st) in enumerate(save.get("chain", [])):
            a.csv_pre[l], a.csv_act[l] = _p(pre), _p(act)
            a.cs_sv[l] = st
        if save.get("chain_t") is not None:
            a.csv_t, a.cs_t = _p(save["chain_t"]), save.get("chain_t_s", 0)
    _lib.call("tmae_lic_stack", ctypes.byref(a), _stream())


def gc_slices(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, noise, lik, Mtot, yhat, yhat_dtype, ld_yhat, yhat32, ld32, n,
              HW, nslices, sw):
    _lib.call("tmae_gc_slices_fwd", _p(y), ldy, yoff, _p(mu), _p(sigma), ms_stride, ld_ms, _p(noise), _p(lik), Mtot,
              _p(yhat), dtype_code(yhat_dtype), ld_yhat, _p(yhat32), ld32, n, HW, nslices, sw, _stream())


def mae_masking(noise: torch.Tensor, len_keep: int):
    """models_mae.random_masking indices: (ids_shuffle, ids_restore) int64 and the binary mask f32 [n, L]"""
    nz = _need(noise.float().contiguous(), name="noise")
    n, L = nz.shape
    shuf = torch.empty((n, L), dtype=torch.int64, device=nz.device)
    rest = torch.empty_like(shuf)
    mask = torch.empty((n, L), dtype=torch.float32, device=nz.device)
    _lib.call("tmae_mae_masking", nz.data_ptr(), shuf.data_ptr(), rest.data_ptr(), mask.data_ptr(), n, L, len_keep,
              _stream())
    return shuf, rest, mask


_MAE_WORK = {}


def mae_loss(pred, imgs, ids_restore, len_keep, patch, norm_pix_loss):
    """models_mae.forward_loss -> 0-d f32 device tensor"""
    p = _need(pred.contiguous(), torch.float32, "pred")
    x = _need(imgs.contiguous(), torch.float32, "imgs")
    n, C, H, W = x.shape
    work = _MAE_WORK.get(x.device)
    if work is None:
        work = _MAE_WORK[x.device] = torch.empty(1024, dtype=torch.float64, device=x.device)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    _lib.call("tmae_mae_loss", p.data_ptr(), x.data_ptr(), _need(ids_restore, torch.int64, "ids_restore").data_ptr(),
              n, C, H, W, patch, len_keep, int(bool(norm_pix_loss)), work.data_ptr(), out.data_ptr(), _stream())
    return out


def gc_slices_code(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, lik, Mtot, yhat, yhat_dtype, ld_yhat, yhat32, ld32, n,
                   HW, nslices, sw, symbols, indexes, scale_table):
    """eval slice step of MCM.compress: gc_slices outputs + int32 symbols / scale indexes in coder order"""
    st = _need(scale_table.contiguous(), torch.float32, "scale_table")
    _lib.call("tmae_gc_slices_code", _p(y), ldy, yoff, _p(mu), _p(sigma), ms_stride, ld_ms, _p(lik), Mtot, _p(yhat),
              dtype_code(yhat_dtype), ld_yhat, _p(yhat32), ld32, n, HW, nslices, sw, _p(symbols), _p(indexes),
              st.data_ptr(), st.numel(), _stream())


def gc_indexes(sigma, ms_stride, ld_ms, n, HW, nslices, sw, scale_table, scale_bound, indexes):
    st = _need(scale_table.contiguous(), torch.float32, "scale_table")
    _lib.call("tmae_gc_indexes", _p(sigma), ms_stride, ld_ms, n, HW, nslices, sw, st.data_ptr(), st.numel(),
              float(scale_bound), _p(indexes), _stream())


def gc_dequantize(symbols, mu, ms_stride, ld_ms, n, HW, nslices, sw, yoff, yhat, yhat_dtype, ld_yhat, yhat32, ld32):
    _lib.call("tmae_gc_dequantize", _p(symbols), _p(mu), ms_stride, ld_ms, n, HW, nslices, sw, yoff, _p(yhat),
              dtype_code(yhat_dtype), ld_yhat, _p(yhat32), ld32, _stream())


def _q_ptr(q, n):
    """device address of the per-image ladder positions (int32 [n]) or None = all zero"""
    if q is None:
        return None
    _need(q, torch.int32, "q")
    if q.numel() != n:
        raise ValueError(f"q holds {q.numel()} entries for {n} images")
    return q.data_ptr()


def gc_slices_code_q(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, lik, Mtot, yhat, yhat_dtype, ld_yhat, yhat32, ld32, n,
                     HW, nslices, sw, symbols, indexes, scale_table, scale_bound, q):
    """gc_slices_code at a per-image quantiser step: q int32 [n] on the device, ladder positions
    in -32..32 (bitstream.qstep), or None = all zero; lik may be None"""
    st = _need(scale_table.contiguous(), torch.float32, "scale_table")
    _lib.call("tmae_gc_slices_code_q", _p(y), ldy, yoff, _p(mu), _p(sigma), ms_stride, ld_ms, _p(lik), Mtot, _p(yhat),
              dtype_code(yhat_dtype), ld_yhat, _p(yhat32), ld32, n, HW, nslices, sw, _p(symbols), _p(indexes),
              st.data_ptr(), st.numel(), float(scale_bound), _q_ptr(q, n), _stream())


def gc_slices_fwd_q(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, noise, lik, Mtot, yhat, yhat_dtype, ld_yhat, yhat32, ld32,
                    n, HW, nslices, sw, scale_bound, q):
    """gc_slices at a per-image quantiser step: q int32 [n] on the device or None = all zero; without
    noise the outputs are bitwise gc_slices_code_q's y_hat and likelihood, with noise the training likelihood at
    |(y - mu) / step + noise|"""
    _lib.call("tmae_gc_slices_fwd_q", _p(y), ldy, yoff, _p(mu), _p(sigma), ms_stride, ld_ms, _p(noise), _p(lik), Mtot,
              _p(yhat), dtype_code(yhat_dtype), ld_yhat, _p(yhat32), ld32, n, HW, nslices, sw, float(scale_bound),
              _q_ptr(q, n), _stream())


def gc_indexes_q(sigma, ms_stride, ld_ms, n, HW, nslices, sw, scale_table, scale_bound, indexes, q):
    st = _need(scale_table.contiguous(), torch.float32, "scale_table")
    _lib.call("tmae_gc_indexes_q", _p(sigma), ms_stride, ld_ms, n, HW, nslices, sw, st.data_ptr(), st.numel(),
              float(scale_bound), _p(indexes), _q_ptr(q, n), _stream())


def gc_dequantize_q(symbols, mu, ms_stride, ld_ms, n, HW, nslices, sw, yoff, yhat, yhat_dtype, ld_yhat, yhat32, ld32,
                    q):
    _lib.call("tmae_gc_dequantize_q", _p(symbols), _p(mu), ms_stride, ld_ms, n, HW, nslices, sw, yoff, _p(yhat),
              dtype_code(yhat_dtype), ld_yhat, _p(yhat32), ld32, _q_ptr(q, n), _stream())


def _qmap_ptr(qmap, n, HW):
    """device address of the per-pixel ladder positions (int32 [n, HW], required)"""
    if qmap is None:
        raise ValueError("qmap is required (int32 [n, HW] on the device)")
    _need(qmap, torch.int32, "qmap")
    if qmap.numel() != n * HW:
        raise ValueError(f"qmap holds {qmap.numel()} entries for {n} images of {HW} pixels")
    return qmap.data_ptr()


def gc_slices_code_qm(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, lik, Mtot, yhat, yhat_dtype, ld_yhat, yhat32, ld32, n,
                      HW, nslices, sw, symbols, indexes, scale_table, scale_bound, qmap):
    """gc_slices_code_q with the quantiser step per pixel of the latent grid, i.e. per kept patch:
    qmap int32 [n, HW] on the device, the clamped ladder positions of qmap_build; lik may be None"""
    st = _need(scale_table.contiguous(), torch.float32, "scale_table")
    _lib.call("tmae_gc_slices_code_qm", _p(y), ldy, yoff, _p(mu), _p(sigma), ms_stride, ld_ms, _p(lik), Mtot, _p(yhat),
              dtype_code(yhat_dtype), ld_yhat, _p(yhat32), ld32, n, HW, nslices, sw, _p(symbols), _p(indexes),
              st.data_ptr(), st.numel(), float(scale_bound), _qmap_ptr(qmap, n, HW), _stream())


def gc_slices_code_rdo(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, lik, Mtot, yhat, yhat_dtype, ld_yhat, yhat32, ld32,
                       n, HW, nslices, sw, symbols, indexes, scale_table, scale_bound, q, qmap, rdo_w, rate_table,
                       cdf_sizes, cdf_offsets, changed=None):
    """gc_slices_code_q / _qm with rate-distortion optimised quantisation: q int32 [n] or None, qmap
    int32 [n, HW] or None (takes precedence), both None = step 1; rdo_w float32 [n] on the device, the weights in
    squared latent units per bit (0 = plain rounding, bit for bit); rate_table float32 [nscale, width], cdf_sizes /
    cdf_offsets int32 [nscale]: GaussianConditional.device_rate_table() and the device_tables() it belongs to;
    changed: int32 [n], zeroed by the caller, to which the elements whose symbol left the rounded one are added"""
    st = _need(scale_table.contiguous(), torch.float32, "scale_table")
    _need(rdo_w, torch.float32, "rdo_w")
    if rdo_w.numel() != n:
        raise ValueError(f"rdo_w holds {rdo_w.numel()} entries for {n} images")
    _need(rate_table, torch.float32, "rate_table")
    _need(cdf_sizes, torch.int32, "cdf_sizes")
    _need(cdf_offsets, torch.int32, "cdf_offsets")
    if rate_table.dim() != 2 or not rate_table.is_contiguous() or rate_table.shape[0] != st.numel() or \
            cdf_sizes.numel() != st.numel() or cdf_offsets.numel() != st.numel():
        raise ValueError(f"rate_table {tuple(rate_table.shape)}, {cdf_sizes.numel()} sizes and {cdf_offsets.numel()} "
                         f"offsets for {st.numel()} scales: one contiguous row, size and offset per scale")
    if changed is not None:
        _need(changed, torch.int32, "changed")
        if changed.numel() < n:
            raise ValueError(f"changed holds {changed.numel()} entries for {n} images")
    _lib.call("tmae_gc_slices_code_rdo", _p(y), ldy, yoff, _p(mu), _p(sigma), ms_stride, ld_ms, _p(lik), Mtot, _p(yhat),
              dtype_code(yhat_dtype), ld_yhat, _p(yhat32), ld32, n, HW, nslices, sw, _p(symbols), _p(indexes),
              st.data_ptr(), st.numel(), float(scale_bound), _q_ptr(q, n),
              None if qmap is None else _qmap_ptr(qmap, n, HW), rdo_w.data_ptr(), rate_table.data_ptr(),
              rate_table.shape[1], cdf_sizes.data_ptr(), cdf_offsets.data_ptr(), _p(changed), _stream())


def gc_slices_fwd_qm(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, noise, lik, Mtot, yhat, yhat_dtype, ld_yhat, yhat32,
                     ld32, n, HW, nslices, sw, scale_bound, qmap):
    """gc_slices_fwd_q at a step per pixel (qmap int32 [n, HW]); without noise bitwise gc_slices_code_qm's y_hat and
    likelihood"""
    _lib.call("tmae_gc_slices_fwd_qm", _p(y), ldy, yoff, _p(mu), _p(sigma), ms_stride, ld_ms, _p(noise), _p(lik), Mtot,
              _p(yhat), dtype_code(yhat_dtype), ld_yhat, _p(yhat32), ld32, n, HW, nslices, sw, float(scale_bound),
              _qmap_ptr(qmap, n, HW), _stream())


def gc_indexes_qm(sigma, ms_stride, ld_ms, n, HW, nslices, sw, scale_table, scale_bound, indexes, qmap):
    st = _need(scale_table.contiguous(), torch.float32, "scale_table")
    _lib.call("tmae_gc_indexes_qm", _p(sigma), ms_stride, ld_ms, n, HW, nslices, sw, st.data_ptr(), st.numel(),
              float(scale_bound), _p(indexes), _qmap_ptr(qmap, n, HW), _stream())


def gc_dequantize_qm(symbols, mu, ms_stride, ld_ms, n, HW, nslices, sw, yoff, yhat, yhat_dtype, ld_yhat, yhat32, ld32,
                     qmap):
    _lib.call("tmae_gc_dequantize_qm", _p(symbols), _p(mu), ms_stride, ld_ms, n, HW, nslices, sw, yoff, _p(yhat),
              dtype_code(yhat_dtype), ld_yhat, _p(yhat32), ld32, _qmap_ptr(qmap, n, HW), _stream())


def _check_nlev(nlev, who):
    nlev = int(nlev)
    if not 2 <= nlev <= 16:
        raise ValueError(f"{who}: nlev = {nlev} outside 2..16")
    return nlev


def qlevels_select(ids_shuffle, K: int, nlev: int, scores=None, level_map=None):
    """the level of every kept patch (bitstream.select_levels_host on the device) -> (levels int32
    [n, K], status int32 [n]).  Exactly one source: scores f32 [n, L] (rank of the kept patch's score among the kept
    patches' scores, level 0 the highest share) or level_map int32 [n, L] in image patch order, gathered by
    ids_shuffle int64 [n, L]; status 1 = a gathered map entry outside 0..nlev-1, that image's levels all zero"""
    s = _need(ids_shuffle, torch.int64, "ids_shuffle")
    n, L = s.shape
    nlev = _check_nlev(nlev, "qlevels_select")
    if not 1 <= K <= L:
        raise ValueError(f"qlevels_select: need 1 <= K={K} <= L={L}")
    if (scores is None) == (level_map is None):
        raise ValueError("qlevels_select: give scores or level_map, exactly one")
    src = _need(scores, torch.float32, "scores") if level_map is None else _need(level_map, torch.int32, "level_map")
    if tuple(src.shape) != (n, L):
        raise ValueError(f"qlevels_select: the source must be [{n}, {L}], got {tuple(src.shape)}")
    levels = torch.empty((n, int(K)), dtype=torch.int32, device=s.device)
    status = torch.empty(n, dtype=torch.int32, device=s.device)
    _lib.call("tmae_qlevels_select", _p(scores), _p(level_map), s.data_ptr(), levels.data_ptr(), status.data_ptr(), n,
              L, int(K), nlev, _stream())
    return levels, status


def qlevels_pack(levels, nlev: int):
    """levels int32 [n, K] -> int32 [n, bitstream.level_words(K, nlev)] holding the container's little-endian words
    (bitstream.pack_levels_host on the device)"""
    from .bitstream import level_words

    lv = _need(levels, torch.int32, "levels")
    nlev = _check_nlev(nlev, "qlevels_pack")
    n, K = lv.shape
    words = torch.empty((n, level_words(K, nlev)), dtype=torch.int32, device=lv.device)
    _lib.call("tmae_qlevels_pack", lv.data_ptr(), words.data_ptr(), n, K, nlev, _stream())
    return words


def qlevels_unpack(words, nlev, K: int):
    """words int32 [n, ldw] (rows padded to a common width) and the table size of every image, nlev int32 [n] on the
    device (1 = the image has no map: nothing is read) -> (levels int32 [n, K], status int32 [n]): 0 ok, 1 a level >=
    nlev, 2 non-zero tail bits; an image with a fault gets all-zero levels.  Nothing synchronises."""
    w = _need(words, torch.int32, "words")
    nl = _need(nlev, torch.int32, "nlev")
    if w.dim() != 2 or nl.dim() != 1 or nl.numel() != w.shape[0]:
        raise ValueError(f"qlevels_unpack: words must be [n, ldw] and nlev [n], got {tuple(w.shape)} and "
                         f"{tuple(nl.shape)}")
    n, ldw = w.shape
    levels = torch.empty((n, int(K)), dtype=torch.int32, device=w.device)
    status = torch.empty(n, dtype=torch.int32, device=w.device)
    _lib.call("tmae_qlevels_unpack", w.data_ptr() if ldw else None, ldw, nl.data_ptr(), levels.data_ptr(),
              status.data_ptr(), n, int(K), _stream())
    return levels, status


def qmap_build(levels, q, offsets):
    """qmap[b][p] = clamp(q[b] + offsets[b][levels[b][p]], -32, 32) -> int32 [n, K] (bitstream.build_qmap_host on the
    device); levels int32 [n, K], q int32 [n] or None (all zero), offsets int32 [n, 16]"""
    lv = _need(levels, torch.int32, "levels")
    off = _need(offsets, torch.int32, "offsets")
    n, K = lv.shape
    if tuple(off.shape) != (n, 16):
        raise ValueError(f"qmap_build: offsets must be [{n}, 16], got {tuple(off.shape)}")
    qmap = torch.empty_like(lv)
    _lib.call("tmae_qmap_build", lv.data_ptr(), _q_ptr(q, n), off.data_ptr(), qmap.data_ptr(), n, K, _stream())
    return qmap


def gc_pmf(scale_table, pmf_center, max_length):
    """GaussianConditional.update pmf rows + tail masses (device tensors)"""
    st = _need(scale_table.contiguous(), torch.float32, "scale_table")
    c = _need(pmf_center.to(torch.int32).contiguous(), torch.int32, "pmf_center")
    pmf = torch.empty((st.numel(), max_length), dtype=torch.float32, device=st.device)
    tail = torch.empty(st.numel(), dtype=torch.float32, device=st.device)
    _lib.call("tmae_gc_pmf", st.data_ptr(), c.data_ptr(), st.numel(), max_length, pmf.data_ptr(), tail.data_ptr(),
              _stream())
    return pmf, tail


def eb_pmf(eb, pmf_start, max_length):
    """EntropyBottleneck.update pmf rows + tail masses (device tensors)"""
    C = eb.channels
    dev = eb.quantiles.device
    start = _need(pmf_start.float().contiguous(), torch.float32, "pmf_start")
    pmf = torch.empty((C, max_length), dtype=torch.float32, device=dev)
    tail = torch.empty(C, dtype=torch.float32, device=dev)
    table = torch.empty((C, 59), dtype=torch.float32, device=dev)
    params = _eb_params(eb)
    _lib.call("tmae_eb_pmf", params, table.data_ptr(), start.data_ptr(), C, max_length, pmf.data_ptr(),
              tail.data_ptr(), _stream())
    return pmf, tail


def eb_symbols(eb, z_nhwc, n, C, HW, out=None, table=None):
    """round(z - median) as int32 NCHW [n, C, HW] from NHWC z"""
    dev = z_nhwc.device
    out = torch.empty((n, C, HW), dtype=torch.int32, device=dev) if out is None else out
    table = torch.empty((C, 59), dtype=torch.float32, device=dev) if table is None else table
    params = _eb_params(eb)
    _lib.call("tmae_eb_symbols", z_nhwc.data_ptr(), params, table.data_ptr(), n, C, HW, _p(out), _stream())
    return out


def eb_dequantize(eb, symbols, n, C, HW, zhat, table=None):
    """z_hat (NHWC, zhat's dtype) = symbols (NCHW int32) + median"""
    dev = zhat.device
    table = torch.empty((C, 59), dtype=torch.float32, device=dev) if table is None else table
    params = _eb_params(eb)
    _lib.call("tmae_eb_dequantize", _p(symbols), params, table.data_ptr(), n, C, HW, _p(zhat), dtype_code(zhat.dtype),
              _stream())
    return zhat


def invert_permutation(perm):
    p = _need(perm.to(torch.int64).contiguous(), torch.int64, "permutation")
    n, L = p.shape
    inv = torch.empty_like(p)
    _lib.call("tmae_invert_permutation", p.data_ptr(), inv.data_ptr(), n, L, _stream())
    return inv


def ids_pack(ids_shuffle, K: int):
    """ids_shuffle int64 [n, L] -> the first K ids of every row packed at max(1, ceil(log2 L)) bits each, LSB first:
    int32 [n, bitstream.id_words(L, K)] holding the container's little-endian words (bitstream.pack_ids_host on the
    device)"""
    from .bitstream import id_words

    s = _need(ids_shuffle, torch.int64, "ids_shuffle")
    n, L = s.shape
    if not 1 <= K <= L:
        raise ValueError(f"ids_pack: need 1 <= K={K} <= L={L}")
    words = torch.empty((n, id_words(L, K)), dtype=torch.int32, device=s.device)
    _lib.call("tmae_ids_pack", s.data_ptr(), words.data_ptr(), n, L, int(K), _stream())
    return words


def ids_unpack(words, L: int, K: int):
    """inverse of ids_pack with validation: words int32 [n, bitstream.id_words(L, K)] -> (ids_shuffle, ids_restore
    int64 [n, L], status int32 [n]).  The kept ids come first, the unused ones follow in ascending order; status 0 ok,
    1 id >= L, 2 duplicate id, 3 non-zero tail bits, and an image with a non-zero status gets the identity in both
    outputs.  Nothing synchronises: the caller reads status when it suits it."""
    from .bitstream import id_words

    w = _need(words, torch.int32, "words")
    if not 1 <= K <= L:
        raise ValueError(f"ids_unpack: need 1 <= K={K} <= L={L}")
    if w.dim() != 2 or w.shape[1] != id_words(L, K):
        raise ValueError(f"ids_unpack: words must be [n, {id_words(L, K)}] for L={L}, K={K}, got {tuple(w.shape)}")
    n = w.shape[0]
    shuf = torch.empty((n, L), dtype=torch.int64, device=w.device)
    rest = torch.empty_like(shuf)
    status = torch.empty(n, dtype=torch.int32, device=w.device)
    _lib.call("tmae_ids_unpack", w.data_ptr(), shuf.data_ptr(), rest.data_ptr(), status.data_ptr(), n, int(L), int(K),
              _stream())
    return shuf, rest, status


def rans_stream_cap_words(nsymbols: int) -> int:
    """words that always hold one stream of nsymbols symbols (no device work)"""
    return int(_lib.value("tmae_rans_stream_cap_words", int(nsymbols)))


def _rans_tables(tables):
    cdf, sizes, offsets = tables
    _need(cdf, torch.int32, "cdf")
    _need(sizes, torch.int32, "cdf_sizes")
    _need(offsets, torch.int32, "offsets")
    if cdf.dim() != 2 or sizes.numel() != cdf.shape[0] or offsets.numel() != cdf.shape[0]:
        raise ValueError("tables must be cdf [ncdf][stride], cdf_sizes [ncdf], offsets [ncdf]")
    return cdf.data_ptr(), cdf.shape[1], sizes.data_ptr(), offsets.data_ptr(), cdf.shape[0]


def _rans_nsub(name, lanes, nstreams):
    """sub-streams of a call; lanes = None is the wave-per-stream entry point: one sub-stream per stream"""
    from .coder import check_lanes

    lanes = 1 if lanes is None else check_lanes(lanes, f"{name}: ")
    if nstreams <= 0:
        raise ValueError(f"{name}: nstreams = {nstreams} must be positive")
    return nstreams * lanes


def _rans_bufs(name, **bufs):
    """bufs = {what: (tensor, dtype, least number of elements)}: dtype, size and contiguity of all, then the device"""
    for what, (t, dtype, numel) in bufs.items():
        if t.dtype != dtype:
            raise ValueError(f"{name}: {what} must be {dtype}, got {t.dtype}")
        if t.numel() < numel:
            raise ValueError(f"{name}: {what} holds {t.numel()} elements, {numel} needed")
        if not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be contiguous")
    for what, (t, _, _) in bufs.items():
        if not t.is_cuda:
            raise ValueError(f"{name}: {what} must be a device (HIP) tensor")


def _rans_encode(name, lanes, symbols, sym_strides, indexes, idx_strides, nstreams, nseg, seg_len, tables, slabs,
                 cap_words, nwords, status):
    """both encode wrappers: the checks, then tmae_<name> (which takes lanes last where lanes is not None)"""
    i32, nsub = torch.int32, _rans_nsub(name, lanes, nstreams)
    if cap_words <= 0:
        raise ValueError(f"{name}: cap_words = {cap_words} must be positive")
    _rans_bufs(name, symbols=(symbols, i32, 1), indexes=(indexes, i32, 1), slabs=(slabs, i32, nsub * cap_words),
               nwords=(nwords, i32, nsub), status=(status, i32, nstreams))
    _lib.call("tmae_" + name, _p(symbols), sym_strides[0], sym_strides[1], _p(indexes), idx_strides[0], idx_strides[1],
              nstreams, nseg, seg_len, *_rans_tables(tables), _p(slabs), cap_words, _p(nwords), _p(status),
              *(() if lanes is None else (lanes,)), _stream())


def _rans_decode(name, lanes, words, total_words, word_offsets, word_counts, indexes, idx_strides, symbols, sym_strides,
                 nstreams, seg0, nseg, seg_len, tables, state, pos, status, first):
    i32, i64, nsub = torch.int32, torch.int64, _rans_nsub(name, lanes, nstreams)
    _rans_bufs(name, words=(words, i32, max(int(total_words), 1)), word_offsets=(word_offsets, i64, nsub),
               word_counts=(word_counts, i32, nsub), indexes=(indexes, i32, 1), symbols=(symbols, i32, 1),
               state=(state, i64, nsub), pos=(pos, i32, nsub), status=(status, i32, nstreams))
    _lib.call("tmae_" + name, _p(words), total_words, _p(word_offsets), _p(word_counts), _p(indexes), idx_strides[0],
              idx_strides[1], _p(symbols), sym_strides[0], sym_strides[1], nstreams, seg0, nseg, seg_len,
              *_rans_tables(tables), _p(state), _p(pos), _p(status), int(bool(first)),
              *(() if lanes is None else (lanes,)), _stream())


def rans_encode_streams(symbols, sym_strides, indexes, idx_strides, nstreams, nseg, seg_len, tables, slabs, cap_words,
                        nwords, status):
    """code nstreams independent rANS streams on the device (csrc/rans_device.hip), one wave each.  Stream b's
    segment j is seg_len int32 at base + j * strides[0] + b * strides[1]; stream b lands in the last nwords[b] words of
    slabs[b] (cap_words words each); status[b] != 0 where a slab was too small"""
    _rans_encode("rans_encode_streams", None, symbols, sym_strides, indexes, idx_strides, nstreams, nseg, seg_len,
                 tables, slabs, cap_words, nwords, status)


def rans_encode_lanes(symbols, sym_strides, indexes, idx_strides, nstreams, nseg, seg_len, tables, slabs, cap_words,
                      nwords, status, lanes):
    """rans_encode_streams with every stream dealt over `lanes` sub-streams, one thread each (sub-stream l of a stream
    codes the symbols k = l mod lanes of each segment): sub-stream b * lanes + l lands in the last
    nwords[b * lanes + l] words of slab b * lanes + l; status is per stream ([nstreams])"""
    _rans_encode("rans_encode_lanes", lanes, symbols, sym_strides, indexes, idx_strides, nstreams, nseg, seg_len, tables,
                 slabs, cap_words, nwords, status)


def rans_pack_streams(slabs, cap_words, nwords, nstreams, dense, dense_cap_words, word_offsets, status):
    """gather the slab tails into one dense word buffer; word_offsets int64 [nstreams + 1]"""
    _lib.call("tmae_rans_pack_streams", _p(slabs), cap_words, _p(nwords), nstreams, _p(dense), dense_cap_words,
              _p(word_offsets), _p(status), _stream())


def rans_decode_streams(words, total_words, word_offsets, word_counts, indexes, idx_strides, symbols, sym_strides,
                        nstreams, seg0, nseg, seg_len, tables, state, pos, status, first):
    """decode segments [seg0, seg0 + nseg) of nstreams device-resident streams; state (int64 storage of the
    uint64 coder state) / pos / status carry each stream from one call to the next"""
    _rans_decode("rans_decode_streams", None, words, total_words, word_offsets, word_counts, indexes, idx_strides,
                 symbols, sym_strides, nstreams, seg0, nseg, seg_len, tables, state, pos, status, first)


def rans_decode_lanes(words, total_words, word_offsets, word_counts, indexes, idx_strides, symbols, sym_strides,
                      nstreams, seg0, nseg, seg_len, tables, state, pos, status, first, lanes):
    """rans_decode_streams of lane-interleaved streams: word_offsets / word_counts / state / pos are per sub-stream
    ([nstreams * lanes], stream-major), status per stream"""
    _rans_decode("rans_decode_lanes", lanes, words, total_words, word_offsets, word_counts, indexes, idx_strides,
                 symbols, sym_strides, nstreams, seg0, nseg, seg_len, tables, state, pos, status, first)


def _eb_params(eb) -> EBParams:
    p = EBParams()
    for i in range(5):
        p.matrix[i] = getattr(eb, f"_matrix{i}").data_ptr()
        p.bias[i] = getattr(eb, f"_bias{i}").data_ptr()
        if i < 4:
            p.factor[i] = getattr(eb, f"_factor{i}").data_ptr()
    p.quantiles = eb.quantiles.data_ptr()
    return p


def eb_likelihood(eb, z_nhwc, n, C, HW, noise=None, lik=None, zhat=None, table=None):
    """EntropyBottleneck forward on NHWC z: returns (lik NCHW, z_hat NHWC in zhat's dtype, default f32)."""
    dev = z_nhwc.device
    if lik is None:
        lik = torch.empty((n, C, HW), dtype=torch.float32, device=dev)
    if zhat is None:
        zhat = torch.empty((n * HW, C), dtype=torch.float32, device=dev)
    if table is None:
        table = torch.empty((C, 59), dtype=torch.float32, device=dev)
    params = _eb_params(eb)
    _lib.call("tmae_eb_likelihood_fwd", z_nhwc.data_ptr(), params, _p(noise), lik.data_ptr(), _p(zhat),
              dtype_code(zhat.dtype), table.data_ptr(), n, C, HW, _stream())
    return lik, zhat


def eb_aux_loss(eb, out=None, table=None):
    C = eb.channels
    dev = eb.quantiles.device
    out = torch.empty((), dtype=torch.float32, device=dev) if out is None else out
    table = torch.empty((C, 59), dtype=torch.float32, device=dev) if table is None else table
    params = _eb_params(eb)
    _lib.call("tmae_eb_aux_loss", params, eb.target.data_ptr(), out.data_ptr(), table.data_ptr(), C, _stream())
    return out


def gc_likelihood(x, scales, means=None, noise=None, scale_bound=0.11):
    x = _need(x.contiguous(), torch.float32, "inputs")
    lik = torch.empty_like(x)
    xt = torch.empty_like(x)
    _lib.call("tmae_gc_likelihood_fwd", x.data_ptr(), _need(scales.contiguous(), torch.float32, "scales").data_ptr(),
              _p(None if means is None else means.contiguous()), _p(noise), xt.data_ptr(), lik.data_ptr(), x.numel(),
              float(scale_bound), _stream())
    return xt, lik


def nhwc_to_nchw(x, ldx, n, C, H, W, out=None):
    out = torch.empty((n, C, H, W), dtype=torch.float32, device=x.device) if out is None else out
    _lib.call("tmae_nhwc_to_nchw", x.data_ptr(), ldx, out.data_ptr(), n, C, H * W, _stream())
    return out


def crop_normalize_u8(src, crops, size, mean, std, out=None):
    """random-crop loader sample: src uint8 [nsrc, H, W, 3] (device), crops int32 [B, 3] = (image, top, left)
    (device) -> (crop / 255 - mean) / std as f32 [B, 3, size, size] (utils/dataloader.py:58-61)"""
    import ctypes

    assert src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3 and src.is_contiguous()
    crops = _need(crops.contiguous(), torch.int32, "crops")
    B = crops.shape[0]
    out = torch.empty((B, 3, size, size), dtype=torch.float32, device=src.device) if out is None else out
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _lib.call("tmae_crop_normalize_u8", src.data_ptr(), src.shape[0], src.shape[1], src.shape[2], crops.data_ptr(), B,
              size, m, s, out.data_ptr(), _stream())
    return out


_BPP_WORK = {}


def bpp(y_lik, z_lik, num_pixels):
    """sum(log y_lik) + sum(log z_lik), / (-ln 2 * num_pixels): a 0-d f32 device tensor (rd_loss.py:19-20)."""
    y = _need(y_lik.contiguous(), torch.float32, "y likelihood")
    z = _need(z_lik.contiguous(), torch.float32, "z likelihood")
    work = _BPP_WORK.get(y.device)
    if work is None:
        work = _BPP_WORK[y.device] = torch.empty(512, dtype=torch.float64, device=y.device)
    out = torch.empty((), dtype=torch.float32, device=y.device)
    _lib.call("tmae_bpp_sum", y.data_ptr(), y.numel(), z.data_ptr(), z.numel(), work.data_ptr(), out.data_ptr(),
              float(num_pixels), _stream())
    return out


# ---------------------------------------------------------------------------------------------- input pipeline
# Pillow's 8-bit resample (ImagingResample, src/libImaging/Resample.c) is integer arithmetic over coefficient
# tables computed in C doubles; the tables are rebuilt here with the same operations in the same order (Python
# floats are C doubles), the device kernels (csrc/resize.hip) apply them.
RESIZE_PRECISION_BITS = 32 - 8 - 2
_RESIZE_FILTERS = {}
_RESIZE_TABLES = {}
_RESIZE_DEVICE_TABLES = {}


def _bicubic_filter(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear_filter(x: float) -> float:
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


_RESIZE_FILTERS.update({"bicubic": (_bicubic_filter, 2.0), "bilinear": (_bilinear_filter, 1.0)})


def resize_tables(in_size: int, out_size: int, filter: str = "bicubic"):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis: (kk int32 [out_size][ksize] 22-bit fixed
    point, bounds int32 [out_size][2] = (xmin, n)) as numpy arrays, cached per (in, out, filter).  Output xx is
    clip8((2^21 + sum_{x < n} px[xmin + x] * kk[xx][x]) >> 22); entries past n are 0."""
    import math

    import numpy as np

    key = (int(in_size), int(out_size), filter)
    hit = _RESIZE_TABLES.get(key)
    if hit is not None:
        return hit
    if filter not in _RESIZE_FILTERS:
        raise ValueError(f"resize_tables: unknown filter {filter!r} (bicubic, bilinear)")
    in_size, out_size = key[0], key[1]
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resize_tables: sizes must be >= 1, got {in_size} -> {out_size}")
    f, fsupport = _RESIZE_FILTERS[filter]
    filterscale = scale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    one = float(1 << RESIZE_PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        n = xmax - xmin
        if not (0 <= xmin and n >= 1 and xmin + n <= in_size and n <= ksize):
            raise ValueError(f"resize_tables: output {xx} of {in_size} -> {out_size} has taps [{xmin}, {xmin + n})")
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        # int() truncates toward zero like the C cast
        kk[xx, :n] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        bounds[xx] = (xmin, n)
    kk.setflags(write=False)
    bounds.setflags(write=False)
    _RESIZE_TABLES[key] = (kk, bounds)
    return kk, bounds


def _resize_device_tables(in_size, out_size, filter, device):
    """device copies of one axis' tables: (kk, bounds, ksize)"""
    key = (int(in_size), int(out_size), filter, torch.device(device))
    hit = _RESIZE_DEVICE_TABLES.get(key)
    if hit is None:
        kk, bounds = resize_tables(in_size, out_size, filter)  # read-only cached arrays: upload writable copies
        hit = (torch.from_numpy(kk.copy()).to(device), torch.from_numpy(bounds.copy()).to(device), kk.shape[1])
        _RESIZE_DEVICE_TABLES[key] = hit
    return hit


_RESIZE_MODES = {"u8": 0, "f32": 1}


def resize_u8(src, size, filter="bicubic", out="u8", mean=None, std=None):
    """PIL.Image.resize of a batch on the device, bit for bit (csrc/resize.hip): src uint8 [n, H, W, 3] (or
    [H, W, 3]), size an int or (h, w).  out="u8": uint8 [n, h, w, 3]; out="f32": f32 [n, 3, h, w] = v / 255
    (ToTensor), or (v / 255 - mean) / std when mean and std are given (Normalize) -- bitwise torch's."""
    single = src.dim() == 3
    s = src.unsqueeze(0) if single else src
    if s.dim() != 4 or s.shape[3] != 3:
        raise ValueError(f"resize_u8: src must be uint8 [n, H, W, 3], got {tuple(src.shape)}")
    s = _need(s.contiguous(), torch.uint8, "src")
    if out not in _RESIZE_MODES:
        raise ValueError(f"resize_u8: out must be 'u8' or 'f32', got {out!r}")
    if (mean is None) != (std is None) or (mean is not None and out != "f32"):
        raise ValueError("resize_u8: mean and std go together, with out='f32'")
    Ho, Wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    n, H, W = int(s.shape[0]), int(s.shape[1]), int(s.shape[2])
    if min(n, H, W, Ho, Wo) < 1:
        raise ValueError(f"resize_u8: sizes must be >= 1, got n={n} {H}x{W} -> {Ho}x{Wo}")
    kh, bh, ksh = _resize_device_tables(W, Wo, filter, s.device)
    kv, bv, ksv = _resize_device_tables(H, Ho, filter, s.device)
    mode = _RESIZE_MODES[out] + (1 if mean is not None else 0)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean]) if mean is not None else None
    sd = (ctypes.c_float * 3)(*[float(v) for v in std]) if std is not None else None
    if out == "u8":
        dst = torch.empty((n, Ho, Wo, 3), dtype=torch.uint8, device=s.device)
    else:
        dst = torch.empty((n, 3, Ho, Wo), dtype=torch.float32, device=s.device)
    nwork = int(_lib.value("tmae_resize_u8_workspace", n, H, W, Ho, Wo))
    work = torch.empty(nwork, dtype=torch.uint8, device=s.device) if nwork else None
    with torch.cuda.device(s.device):
        _lib.call("tmae_resize_u8", s.data_ptr(), n, H, W, Ho, Wo, kh.data_ptr(), bh.data_ptr(), ksh, kv.data_ptr(),
                  bv.data_ptr(), ksv, mode, m, sd, dst.data_ptr(), _p(work), nwork, _stream())
    return dst[0] if single else dst


def rgb_to_gray_u8(src):
    """uint8 [..., 3] (device) -> uint8 [...]: (9798 R + 19235 G + 3735 B + 16384) >> 15, the grayscale
    scores.imread_gray computes on the host for non-JPEG files"""
    if src.dim() < 2 or src.shape[-1] != 3 or src.numel() == 0:
        raise ValueError(f"rgb_to_gray_u8: src must be uint8 [..., 3] and not empty, got {tuple(src.shape)}")
    s = _need(src.contiguous(), torch.uint8, "src")
    out = torch.empty(s.shape[:-1], dtype=torch.uint8, device=s.device)
    with torch.cuda.device(s.device):
        _lib.call("tmae_rgb_to_gray_u8", s.data_ptr(), out.numel(), out.data_ptr(), _stream())
    return out


# --------------------------------------------------------------------------------------- tiled images
def tile_cut_u8(src, S: int, O: int, t0: int = 0, nt=None, tiles=None, gray=None):
    """tiles t0 .. t0 + nt (nt=None: to the last) of the overlapping S x S tile grid of an image (tiling.py,
    csrc/tile.hip): src uint8 [H, W, 3] on the device -> (tiles f32 [nt, 3, S, S] = v / 255, the test transform's
    ToTensor bit for bit, gray uint8 [nt, S, S] = rgb_to_gray_u8 of the tiles).  Samples outside the image are the
    nearest edge pixel.  tiles= / gray= take preallocated outputs."""
    from .tiling import grid

    if src.dim() != 3 or src.shape[2] != 3:
        raise ValueError(f"tile_cut_u8: src must be uint8 [H, W, 3], got {tuple(src.shape)}")
    s = _need(src, torch.uint8, "src")
    H, W = int(s.shape[0]), int(s.shape[1])
    g = grid(H, W, S, O)
    t0 = int(t0)
    nt = g.T - t0 if nt is None else int(nt)
    if t0 < 0 or nt < 1 or t0 + nt > g.T:
        raise ValueError(f"tile_cut_u8: tiles {t0}..{t0 + nt} outside the image's {g.T} ({g.ny} x {g.nx})")
    if tiles is None:
        tiles = torch.empty((nt, 3, g.S, g.S), dtype=torch.float32, device=s.device)
    elif tuple(_need(tiles, torch.float32, "tiles").shape) != (nt, 3, g.S, g.S):
        raise ValueError(f"tile_cut_u8: tiles must be [{nt}, 3, {g.S}, {g.S}], got {tuple(tiles.shape)}")
    if gray is None:
        gray = torch.empty((nt, g.S, g.S), dtype=torch.uint8, device=s.device)
    elif tuple(_need(gray, torch.uint8, "gray").shape) != (nt, g.S, g.S):
        raise ValueError(f"tile_cut_u8: gray must be [{nt}, {g.S}, {g.S}], got {tuple(gray.shape)}")
    with torch.cuda.device(s.device):
        _lib.call("tmae_tile_cut_u8", s.data_ptr(), H, W, g.S, g.O, t0, nt, tiles.data_ptr(), gray.data_ptr(),
                  _stream())
    return tiles, gray


def tile_blend(tiles, H: int, W: int, O: int, out="f32", out_f32=None, out_u8=None):
    """inverse of tile_cut_u8 on decoded tiles: tiles f32 [T, 3, S, S] (all tiles of the H x W image) -> the
    weighted blend, out="f32": f32 [3, H, W]; "u8": uint8 [H, W, 3] = clamp(0, 1).mul(255).round() of it; "both":
    the pair, from one launch.  out_f32= / out_u8= take preallocated outputs."""
    from .tiling import grid

    if out not in ("f32", "u8", "both"):
        raise ValueError(f"tile_blend: out must be 'f32', 'u8' or 'both', got {out!r}")
    t = _need(tiles, torch.float32, "tiles")
    if t.dim() != 4 or t.shape[1] != 3 or t.shape[2] != t.shape[3]:
        raise ValueError(f"tile_blend: tiles must be f32 [T, 3, S, S], got {tuple(t.shape)}")
    g = grid(H, W, int(t.shape[2]), O)
    if t.shape[0] != g.T:
        raise ValueError(f"tile_blend: {t.shape[0]} tiles, but {g.H}x{g.W} at tile size {g.S}, overlap {g.O} has "
                         f"{g.ny} x {g.nx} = {g.T}")
    f32 = u8 = None
    if out in ("f32", "both"):
        f32 = out_f32 if out_f32 is not None else torch.empty((3, g.H, g.W), dtype=torch.float32, device=t.device)
        if tuple(_need(f32, torch.float32, "out_f32").shape) != (3, g.H, g.W):
            raise ValueError(f"tile_blend: out_f32 must be [3, {g.H}, {g.W}], got {tuple(f32.shape)}")
    if out in ("u8", "both"):
        u8 = out_u8 if out_u8 is not None else torch.empty((g.H, g.W, 3), dtype=torch.uint8, device=t.device)
        if tuple(_need(u8, torch.uint8, "out_u8").shape) != (g.H, g.W, 3):
            raise ValueError(f"tile_blend: out_u8 must be [{g.H}, {g.W}, 3], got {tuple(u8.shape)}")
    with torch.cuda.device(t.device):
        _lib.call("tmae_tile_blend", t.data_ptr(), g.H, g.W, g.S, g.O, _p(f32), _p(u8), _stream())
    return (f32, u8) if out == "both" else (f32 if out == "f32" else u8)


TILE_CROP_DESC = 8  # int32 per window descriptor (TL_DESC of csrc/tile.hip): H, W, y0, x0, map_base, three unused


def tile_blend_crops(tiles, images, windows, size, O: int, out="f32", out_f32=None, out_u8=None):
    """R windows of one size out of tile_blend's image without the tiles they do not touch (region decode, DESIGN.md
    §3.16), one launch.  tiles f32 [N, 3, S, S]: a compact buffer of decoded tiles, of any number of images in any
    order; images: per image (H, W, slots), slots[t] = the position of its tile t in tiles, -1 where the tile is
    not there; windows: R triples (image index, x0, y0); size = (w, h).  -> f32 [R, 3, h, w] (out="f32"), uint8
    [R, h, w, 3] ("u8") or the pair ("both"), each window equal to tile_blend(all tiles of its image)[..., y0:y0 + h,
    x0:x0 + w] bit for bit.  Every window is checked against its image and every tile it needs
    (tiling.region_tiles) against the buffer, on the host, before anything is uploaded.  out_f32= / out_u8= take
    preallocated outputs."""
    from .tiling import grid, region_tiles

    if out not in ("f32", "u8", "both"):
        raise ValueError(f"tile_blend_crops: out must be 'f32', 'u8' or 'both', got {out!r}")
    t = _need(tiles, torch.float32, "tiles")
    if t.dim() != 4 or t.shape[0] < 1 or t.shape[1] != 3 or t.shape[2] != t.shape[3]:
        raise ValueError(f"tile_blend_crops: tiles must be f32 [N >= 1, 3, S, S], got {tuple(t.shape)}")
    N, S = int(t.shape[0]), int(t.shape[2])
    w, h = int(size[0]), int(size[1])
    images, windows = list(images), list(windows)
    if not windows:
        raise ValueError("tile_blend_crops: no windows")
    grids, bases, slot_map = [], [], []
    for i, (H, W, slots) in enumerate(images):
        g = grid(H, W, S, O)
        slots = [int(s) for s in slots]
        if len(slots) != g.T:
            raise ValueError(f"tile_blend_crops: image {i}: {len(slots)} slots, but {g.H}x{g.W} at tile size {g.S}, "
                             f"overlap {g.O} has {g.ny} x {g.nx} = {g.T} tiles")
        if any(not -1 <= s < N for s in slots):
            raise ValueError(f"tile_blend_crops: image {i}: slots must be -1 or one of the buffer's {N}")
        grids.append(g)
        bases.append(len(slot_map))
        slot_map += slots
    R = len(windows)
    desc = []
    for r, (i, x0, y0) in enumerate(windows):
        i = int(i)
        if not 0 <= i < len(grids):
            raise ValueError(f"tile_blend_crops: window {r}: image {i} outside 0..{len(grids) - 1}")
        g = grids[i]
        try:
            need = region_tiles(g, x0, y0, w, h)
        except ValueError as e:
            raise ValueError(f"tile_blend_crops: window {r}: {e}") from None
        for k in need:
            if slot_map[bases[i] + k] < 0:
                raise ValueError(f"tile_blend_crops: window {r}: needs tile {k} of image {i}, which has no slot")
        desc += [g.H, g.W, int(y0), int(x0), bases[i]] + [0] * (TILE_CROP_DESC - 5)
    f32 = u8 = None
    if out in ("f32", "both"):
        f32 = out_f32 if out_f32 is not None else torch.empty((R, 3, h, w), dtype=torch.float32, device=t.device)
        if tuple(_need(f32, torch.float32, "out_f32").shape) != (R, 3, h, w):
            raise ValueError(f"tile_blend_crops: out_f32 must be [{R}, 3, {h}, {w}], got {tuple(f32.shape)}")
    if out in ("u8", "both"):
        u8 = out_u8 if out_u8 is not None else torch.empty((R, h, w, 3), dtype=torch.uint8, device=t.device)
        if tuple(_need(u8, torch.uint8, "out_u8").shape) != (R, h, w, 3):
            raise ValueError(f"tile_blend_crops: out_u8 must be [{R}, {h}, {w}, 3], got {tuple(u8.shape)}")
    # the descriptors, then the maps: one upload
    table = torch.tensor(desc + slot_map, dtype=torch.int32).to(t.device)
    with torch.cuda.device(t.device):
        _lib.call("tmae_tile_blend_crops", t.data_ptr(), N, table.data_ptr() + 4 * len(desc), len(slot_map),
                  table.data_ptr(), R, h, w, S, int(O), _p(f32), _p(u8), _stream())
    return (f32, u8) if out == "both" else (f32 if out == "f32" else u8)
