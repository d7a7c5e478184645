"""Element-wise checker of the two backward GEMM families: tmae_wgrad (csrc/gemm_tn.h, the split-K TN GEMM behind every
weight and bias gradient) and tmae_conv_dgrad (ConvTSrc in csrc/train.hip, the transposed-conv row source on the GEMM
core).  tests/test_gpu_wgrad_cases.py and tests/test_gpu_conv_dgrad_cases.py run the cases on the GPU,
tests/test_tn_checker.py proves on the CPU that the checker rejects the faults such kernels can produce.

Two passes per case.

* Exact pass.  Operands are drawn from {+-1, +-2, +-3}: exact in bf16, no product is zero, and every partial sum of
  any of the cases is an integer below 2^24 (|a b| <= 9, reductions of at most 5632 terms), so f32 accumulation is
  exact in ANY order, split count or tile, and every output element must EQUAL the integer reference (formed in
  float64, where the same sums are exact, and held as int64).  A dropped, doubled or misaddressed term fails it at
  every K, also where no rounding bound can see one term.
* Bounded pass.  A ~ N(0, 1), B ~ N(0, 1) / sqrt(K), rounded to the operand dtype, against float64 under
  gemm_check's any-order bound (K + 2) u S with S = sum_k |a b|, u = 2^-23.  The fixed-order fold of the split slabs
  is one more summation tree over the same K products, so it adds no term.  Accumulation into a non-zero f32 buffer
  adds u (|acc0| + |ref| + bound) (gemm_check.dgrad_reference).  The bias gradient sum_k A(k, m) has the same bound
  with S = sum_k |a|.  A store in the operand dtype adds BF16_ROUND (|ref| + bound).  No constant here comes from
  running a kernel.

Buffers.  Dense outputs are gemm_check.Guarded blocks; the conv-layout output, the bias and the workspace are Flat
buffers (NaN-filled, 64 guard floats on each side); operands are packed into NaN-filled buffers whose padding
columns, skipped rows (the cls rows of a remap) and two guard rows on each side are NaN.  An element never written
stays NaN, a write outside shows as a non-NaN guard, a read outside the operand poisons the output.
"""
import collections
import ctypes
import math

import torch

from gemm_check import BF16_ROUND, U, Guarded, check_out, dgrad_reference, ratio  # noqa: F401
from parity_log import check as log_check

BF16, F32 = torch.bfloat16, torch.float32


def dname(dtype):
    return "bf16" if dtype == BF16 else "f32"


def epc(dtype):
    return 8 if dtype == BF16 else 4


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------ the plan, restated
Plan = collections.namedtuple("Plan", "dtype bn bm nw splits kchunk")


def _rule(M, N, K, bf, slot_div, nb):
    K = max(K, 1)
    if not bf:
        bn, bm, nw = 64, 64, 4
    else:
        t256 = cdiv(N, 256) * cdiv(M, 256)
        u256 = (N / (cdiv(N, 256) * 256.0)) * (M / (cdiv(M, 256) * 256.0)) if t256 else 0.0
        bn, bm, nw = (256, 256, 8) if (u256 > 0.7 and t256 * 8 >= 64) else (128, 128, 4)
    tiles = max(1, cdiv(N, bn) * cdiv(M, bm) * max(1, nb))
    slots = (256 if nw == 8 else 512) // max(1, slot_div)
    s = max(1, slots // tiles)
    s = max(1, min(s, max(1, K // (256 if bf else 128))))
    s = min(s, 64)
    step = 64 if bf else 32
    kchunk = cdiv(cdiv(K, s), step) * step
    return Plan("bf16" if bf else "f32", bn, bm, nw, cdiv(K, kchunk), kchunk)


def expected_plan(M, N, K, dtype, slot_div=1, nb=1):
    """tn_plan's documented rule (csrc/gemm_tn.h), restated independently of the library: bf16 takes the
    256 x 256 8-wave tile when it is at least 70 % full and there are at least 8 such tiles, else 128 x 128; f32 one
    64 x 64 tile.  The K range is cut into as many splits as fit one round of the workgroup slots (512, or 256 for
    the 8-wave tile, divided by slot_div and shared by the nb problems), at least 256 (f32: 128) rows each, at most
    64, in chunks of whole K-steps.  The f32 path launches its problems one by one, each planned alone.  K <= 0
    plans as K = 1."""
    bf = dtype == BF16
    return _rule(M, N, K, bf, slot_div, nb if bf else 1)


def plan_str(p):
    return f"tn<{p.dtype},{p.bn}x{p.bm},{p.nw}w,s{p.splits},kc{p.kchunk}>"


def workspace_elems(M, N, K, dtype, slot_div=1, nb=1):
    """what tmae_wgrad_workspace_nb must return: the slabs and bias slabs of nb problems planned together, and never
    less than one problem planned alone (what each launch of the f32 per-problem path can take)"""
    bf, nb = dtype == BF16, max(1, nb)
    return max(nb * _rule(M, N, K, bf, slot_div, nb).splits, _rule(M, N, K, bf, 1, 1).splits) * (M * N + M)


# ------------------------------------------------------------------------------------ case tables
# dense weight gradients: M x N x K and the bf16 plan (tile, splits, K rows per split) worked out from the rule
WCase = collections.namedtuple("WCase", "M N K bf16_plan remap lda_pad ldb_pad")
W_CASES = {
    "W1": WCase(8, 8, 8, (128, 1, 64), None, 0, 0),            # one partial tile, one tail K-step, clamp to column 0
    "W2": WCase(136, 264, 456, (128, 1, 512), None, 0, 0),     # 2 x 3 ragged tiles, 8 K-steps, the last of 8 rows
    "W3": WCase(72, 64, 5632, (128, 22, 256), None, 0, 0),     # the 16-, 4- and 1-split folds of tn_reduce_kernel
    "W4": WCase(512, 1024, 72, (256, 1, 128), None, 0, 0),     # 8-wave tile, K-step 2 a tail
    "W5": WCase(760, 1032, 584, (256, 2, 320), None, 0, 0),    # 8-wave tile, ragged M and N, split 2 ragged
    "W6": WCase(264, 136, 1160, (128, 4, 320), None, 0, 0),    # four splits, the last of 200 rows
    # remap on both operands, padded leading dimensions: groups of 144 of every 145 rows (the encoder's cls rows);
    # groups of 5 of every 7 (a split boundary inside a group); G > K (ungrouped rows, offset 1)
    "W7a": WCase(136, 72, 720, (128, 2, 384), (144, 145, 1), 16, 8),
    "W7b": WCase(136, 72, 720, (128, 2, 384), (5, 7, 2), 16, 8),
    "W7c": WCase(136, 72, 720, (128, 2, 384), (1 << 30, 0, 1), 16, 8),
}

# 3x3 conv weight gradients: M = cout, N = 9 cin, K = n Ho Wo
CCase = collections.namedtuple("CCase", "n H W stride c1 c2 cout cin_total ci_off")
C_CASES = {
    "C1": CCase(64, 3, 3, 1, 48, 0, 40, 48, 0),     # hw = 9: a K-step jumps 7 images; split 2 starts mid-image, mid-row
    "C2": CCase(3, 12, 12, 1, 48, 0, 40, 48, 0),    # hw = 144: K-steps straddle images
    "C3": CCase(70, 2, 2, 2, 16, 0, 24, 16, 0),     # hw = 1: every tap but four is padding; a K-step jumps 64 images
    "C4": CCase(5, 5, 7, 2, 24, 0, 16, 24, 0),      # odd, non-square map at stride 2
    "C5": CCase(2, 6, 10, 1, 16, 8, 24, 32, 8),     # two input tensors, written into a channel slice
    "C6a": CCase(1, 8, 8, 1, 256, 0, 256, 256, 0),  # the 8-wave tile on the conv source, one split
    "C6b": CCase(9, 8, 8, 1, 256, 0, 256, 256, 0),  # ... two splits
}

# conv data gradients: rows = n H W, output columns = cin, K = 9 cout; cout / cin None: EPC / BN + 8
DCase = collections.namedtuple("DCase", "n H W stride cout cin")
D_CASES = {
    "D1": DCase(1, 1, 1, 1, None, None),   # centre tap only; 8 taps per K-step; the second K-step one live chunk
    "D2": DCase(3, 5, 7, 2, 24, 20),       # 2-3 tap crossings per step; parity taps on an odd map; 4-column tail
    "D3": DCase(2, 6, 6, 2, 72, None),     # h_a's geometry; a tap boundary inside a K-step
    "D4": DCase(2, 12, 12, 1, 192, 32),    # 27 K-steps (deep rings on the small tiles); 288 rows, ragged on every BM
    "D5": DCase(5, 2, 2, 2, 40, None),     # the 64-pixel model's h_a
}
D_TILES = {BF16: (5, 1, 7, 0), F32: (5, 1)}  # indices into gemm_check.TILES


def out_hw(H, W, stride):
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def conv_mnk(c):
    Ho, Wo = out_hw(c.H, c.W, c.stride)
    return c.cout, 9 * (c.c1 + c.c2), c.n * Ho * Wo


def dcase(name, bn, dtype):
    """the case with its cout / cin filled in for a tile of bn weight rows"""
    c = D_CASES[name]
    return c._replace(cout=c.cout or epc(dtype), cin=c.cin or bn + 8)


# ------------------------------------------------------------------------------------ operands
def gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v)) % (1 << 31)
    return torch.Generator().manual_seed(seed)


def draw(shape, dtype, exact, scale, g):
    """exact: {+-1, +-2, +-3}; else N(0, scale^2) rounded to dtype"""
    if exact:
        v = torch.randint(1, 4, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)
        return v.to(dtype)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def draw_acc(shape, exact, g):
    """a non-zero f32 buffer to accumulate onto (integers in the exact pass)"""
    if exact:
        return torch.randint(-8, 9, shape, generator=g).float()
    return torch.randn(shape, generator=g)


def wgrad_operands(M, N, K, dtype, exact, seed=0):
    g = gen(M, N, K, exact, seed)
    return draw((K, M), dtype, exact, 1.0, g), draw((K, N), dtype, exact, 1.0 / math.sqrt(K), g)


def conv_operands(c, dtype, exact, seed=0):
    """x NCHW [n][cin][H][W] and dy NCHW [n][cout][Ho][Wo], rounded to dtype"""
    Ho, Wo = out_hw(c.H, c.W, c.stride)
    K = c.n * Ho * Wo
    g = gen(*c, exact, seed)
    dy = draw((c.n, c.cout, Ho, Wo), dtype, exact, 1.0, g)
    x = draw((c.n, c.c1 + c.c2, c.H, c.W), dtype, exact, 1.0 / math.sqrt(K), g)
    return x, dy


def dgrad_operands(c, dtype, exact, seed=0):
    """dy NCHW [n][cout][Ho][Wo] and w [cout][cin][3][3], rounded to dtype"""
    Ho, Wo = out_hw(c.H, c.W, c.stride)
    g = gen(*c, exact, seed, 7)
    dy = draw((c.n, c.cout, Ho, Wo), dtype, exact, 1.0, g)
    w = draw((c.cout, c.cin, 3, 3), dtype, exact, 1.0 / math.sqrt(9 * c.cout), g)
    return dy, w


def nhwc(t):
    """NCHW -> [n H W][C]"""
    return t.permute(0, 2, 3, 1).contiguous().reshape(-1, t.shape[1])


# ------------------------------------------------------------------------------------ float64 terms
def dense_terms(a, b):
    """ref = A^T B [M][N], S = |A|^T |B|, bias = column sums of A, Sb = column sums of |A| (float64)"""
    ad, bd = a.double(), b.double()
    return ad.t() @ bd, ad.abs().t() @ bd.abs(), ad.sum(0), ad.abs().sum(0)


def conv_wgrad_terms(c, x, dy):
    """the same four of a 3x3 conv's weight gradient [cout][cin][3][3], from torch.nn.grad.conv2d_weight"""
    shape = (c.cout, c.c1 + c.c2, 3, 3)
    xd, dd = x.double(), dy.double()
    ref = torch.nn.grad.conv2d_weight(xd, shape, dd, stride=c.stride, padding=1)
    S = torch.nn.grad.conv2d_weight(xd.abs(), shape, dd.abs(), stride=c.stride, padding=1)
    return ref, S, dd.sum((0, 2, 3)), dd.abs().sum((0, 2, 3))


def conv_dgrad_terms(c, dy, w):
    """ref, S [n H W][cin] of a 3x3 conv's data gradient, from torch.nn.grad.conv2d_input"""
    shape = (c.n, c.cin, c.H, c.W)
    ref = torch.nn.grad.conv2d_input(shape, w.double(), dy.double(), stride=c.stride, padding=1)
    S = torch.nn.grad.conv2d_input(shape, w.double().abs(), dy.double().abs(), stride=c.stride, padding=1)
    return nhwc(ref), nhwc(S)


def bounded(ref, S, K, exact, acc0=None, store_bf16=False):
    """(ref, bound) of a K-term reduction stored in f32 (+ acc0), or rounded to bf16; exact: a zero bound"""
    if exact:
        ref = ref if acc0 is None else ref + acc0.double()
        return ref, torch.zeros_like(ref)
    ref, bound = dgrad_reference(ref, S, K, None, acc0)
    if store_bf16:
        bound = bound + BF16_ROUND * (ref.abs() + bound)
    return ref, bound


def to_int64(ref):
    """the exact pass's reference as integers (float64 sums of small integers are exact)"""
    r = ref.round()
    assert torch.equal(r, ref) and float(ref.abs().max()) < 2 ** 24
    return r.to(torch.int64)


# ------------------------------------------------------------------------------------ the kernels' index maps
def im2col(x_nhwc, n, H, W, stride, wrap=False):
    """[n H W][cin] -> [n Ho Wo][9 cin], column tap * cin + ci: KConvSrc's operand as a dense matrix.  wrap: the
    fault of reading the padding pixel ix = -1 from the flat neighbour (the last pixel of the row above)."""
    cin = x_nhwc.shape[1]
    Ho, Wo = out_hw(H, W, stride)
    xz = torch.cat([x_nhwc, torch.zeros(1, cin, dtype=x_nhwc.dtype)])  # the last row: the zero page
    b = torch.arange(n).view(n, 1, 1)
    oy, ox = torch.arange(Ho).view(1, Ho, 1), torch.arange(Wo).view(1, 1, Wo)
    cols = []
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        iy, ix = oy * stride - 1 + ky, ox * stride - 1 + kx
        rows_ok = (iy >= 0) & (iy < H)
        ok = rows_ok & (ix >= 0) & (ix < W)
        pix = b * H * W + iy * W + ix
        if wrap:
            ok = ok | (rows_ok & (ix == -1) & (pix >= 0))
        pix = torch.where(ok, pix, torch.full_like(pix, n * H * W))
        cols.append(xz[pix.reshape(-1)])
    return torch.cat(cols, 1)


def dgrad_cols(dy_nhwc, n, H, W, stride, parity=True):
    """[n Ho Wo][cout] -> [n H W][9 cout], column tap * cout + co: ConvTSrc's operand as a dense matrix.
    parity=False: the fault of letting a stride-2 tap through whose output pixel is not integral."""
    cout = dy_nhwc.shape[1]
    Ho, Wo = out_hw(H, W, stride)
    dz = torch.cat([dy_nhwc, torch.zeros(1, cout, dtype=dy_nhwc.dtype)])
    b = torch.arange(n).view(n, 1, 1)
    iy, ix = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    cols = []
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        ty, tx = iy + 1 - ky, ix + 1 - kx
        ok = (ty >= 0) & (tx >= 0)
        if stride == 2:
            if parity:
                ok = ok & (((ty | tx) & 1) == 0)
            ty, tx = ty // 2, tx // 2
        ok = ok & (ty < Ho) & (tx < Wo)
        pix = (b * Ho + ty) * Wo + tx
        pix = torch.where(ok, pix, torch.full_like(pix, n * Ho * Wo))
        cols.append(dz[pix.reshape(-1)])
    return torch.cat(cols, 1)


def conv_to_columns(w):
    """[cout][cin][3][3] -> [cout][9 cin] with column tap * cin + ci (the TN GEMM's N axis)"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def columns_to_conv(m, cin):
    """the inverse: [cout][9 cin] -> [cout][cin][3][3]"""
    return m.reshape(m.shape[0], 3, 3, cin).permute(0, 3, 1, 2)


def dgrad_weights(w):
    """[cout][cin][3][3] -> wd [cin][9 cout], column tap * cout + co (tmae_conv_dgrad's weight layout)"""
    return w.permute(1, 2, 3, 0).contiguous().reshape(w.shape[1], -1)


# ------------------------------------------------------------------------------------ buffers
class Flat:
    """n f32 elements inside a NaN-filled buffer with G guard floats on each side"""
    G = 64

    def __init__(self, n, device="cpu", init=None):
        self.n = n
        self.buf = torch.full((n + 2 * self.G,), float("nan"), dtype=F32, device=device)
        if init is not None:
            self.inner()[...] = init.reshape(-1).to(F32).to(device)

    def inner(self):
        return self.buf[self.G:self.G + self.n]

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.G

    def poison(self):
        self.buf.fill_(float("nan"))

    def guard_hits(self):
        g = torch.cat([self.buf[:self.G], self.buf[self.G + self.n:]])
        return int((~torch.isnan(g)).sum())

    def result(self):
        return self.inner().detach().double().cpu()


def check_flat(metric, f, ref, bound, mask=None, log=True):
    """guards untouched; with a mask (same shape as ref), the elements outside it still NaN and those inside within
    their bound; returns the largest ratio"""
    hits = f.guard_hits()
    assert hits == 0, f"{metric}: {hits} guard elements outside the buffer were written"
    out = f.result().view(ref.shape)
    if mask is not None:
        stray = int((~torch.isnan(out[~mask])).sum())
        assert stray == 0, f"{metric}: {stray} elements outside the parameter's slice were written"
        out, ref, bound = out[mask], ref[mask], bound[mask]
    r = ratio(out, ref, bound)
    if log:
        log_check(metric, r, 1.0, strict=False)
    assert r <= 1.0, f"{metric}: error / bound = {r:.3g} (an element is off by more than its bound, or never written)"
    return r


def check_workspace(metric, ws):
    hits = ws.guard_hits()
    assert hits == 0, f"{metric}: {hits} elements outside the {ws.n}-float workspace were written"


class Packed:
    """per-problem matrices [rows][cols] packed for the kernels: each in a NaN-filled [2 + src_rows + 2][ld] block
    (two guard rows on each side, padding columns [cols, ld), and with remap = (G, Gs, off) logical row k at source
    row (k // G) Gs + off + k % G, the skipped rows NaN).  ptr: the first problem's source row 0; stride: elements
    from one problem to the next."""
    GR = 2

    def __init__(self, mats, dtype, device, ld=None, remap=None):
        rows, cols = mats[0].shape
        self.ld = ld = ld or cols
        k = torch.arange(rows)
        src = k if remap is None else (k // remap[0]) * remap[1] + remap[2] + k % remap[0]
        nsrc = int(src.max()) + 1 if rows else 0
        blocks = []
        for m in mats:
            blk = torch.full((nsrc + 2 * self.GR, ld), float("nan"), dtype=dtype)
            blk[self.GR + src, :cols] = m.to(dtype)
            blocks.append(blk)
        self.stride = blocks[0].numel()
        self.buf = torch.stack(blocks).to(device)
        self.ptr = self.buf.data_ptr() + self.GR * ld * self.buf.element_size()


# ------------------------------------------------------------------------------------ launches (GPU)
def launch_wgrad(M, N, K, dtype, A, B, out_ptr, layout, *, remap=None, conv=None, B2=None, accumulate=False,
                 bias_ptr=None, bias_accumulate=False, slot_div=1, nb=1, s_b=None, s_out=0, s_bias=0):
    """one tmae_wgrad call with the arguments filled in here, not by train_ops.wgrad: the workspace is exactly
    tmae_wgrad_workspace_nb floats inside a NaN-poisoned Flat whose guards are checked after the launch.
    A, B (B2): Packed operands; layout = (o_base, o_sm, o_sc, o_st, o_cp); conv = dict(c1, H, W, stride, cin)."""
    from textmae_amd import _lib
    from textmae_amd.ops import _stream, dtype_code

    code = dtype_code(dtype)
    need = _lib.value("tmae_wgrad_workspace_nb", M, N, K, code, slot_div, nb)
    assert need == workspace_elems(M, N, K, dtype, slot_div, nb), (need, workspace_elems(M, N, K, dtype, slot_div, nb))
    ws = Flat(need, A.buf.device)
    a = _lib.WgradArgs()
    G, Gs, off = remap or (1 << 30, 0, 0)
    a.a, a.lda, a.a_G, a.a_Gs, a.a_off = A.ptr, A.ld, G, Gs, off
    a.b, a.ldb, a.b_G, a.b_Gs, a.b_off = B.ptr, B.ld, G, Gs, off
    if conv is not None:
        a.b_conv, a.b_c1, a.b_Cin = 1, conv["c1"], conv["cin"]
        a.b_H, a.b_W, a.b_stride = conv["H"], conv["W"], conv["stride"]
        a.b_G, a.b_Gs, a.b_off = 1 << 30, 0, 0
        if B2 is not None:
            a.b2, a.b_ld2 = B2.ptr, B2.ld
    a.M, a.N, a.K = M, N, K
    a.work, a.work_elems = ws.ptr(), need
    a.out = out_ptr
    a.o_base, a.o_sm, a.o_sc, a.o_st, a.o_cp = layout
    a.accumulate = int(accumulate)
    a.bias_out = bias_ptr
    a.bias_accumulate = int(bias_accumulate)
    a.slot_div = slot_div
    if nb > 1:
        a.nb, a.s_a, a.s_b = nb, A.stride, B.stride if s_b is None else s_b
        a.s_b2, a.s_out, a.s_bias = (B2.stride if B2 is not None else 0), s_out, s_bias
    _lib.call("tmae_wgrad", ctypes.byref(a), code, _stream())
    torch.cuda.synchronize()
    check_workspace(f"workspace:{M}x{N}x{K}:{dname(dtype)}", ws)
