"""Element-wise checker of the MFMA GEMM core's outputs (tests/test_gpu_gemm_tiles.py on the GPU, tests/test_gemm_checker.py
for the checker itself on the CPU).

Every output element is bounded on its own against a float64 reference computed from operands already rounded to the
operand dtype.  With u = 2^-23 and S = sum_k |x_k w_k| + |bias| (+ |residual or addend|) in float64, the linear part's
error is at most e = (K + 2) u S for ANY summation order and for truncating as well as rounding accumulation: each of
the K products (exact in f32 for bf16 operands, one rounding for f32 operands) passes through at most K + 1 additions
of relative error <= u, and the bias / residual additions are two more.  The activation and the store add:

    f32 store, no activation / ReLU (1-Lipschitz)   e
    GELU, f32 path (common.h gelu_erf)              1.13 e + 0.5 |z| 3.5e-7 + 4 2^-24 |ref|
    GELU before a bf16 store (gelu_bf16out)         1.13 e + 2.6e-5
    any bf16 store (round to nearest)               + 2^-8 (|ref| + bound so far)

1.13 is the largest slope of GELU (1.1289 at x = 1.41); 3.5e-7 and 2.6e-5 are the approximation errors DESIGN.md §3.2
and common.h state for the two GELUs; 4 2^-24 |ref| covers the f32 evaluation of the final 0.5 x (1 + erf) products.
No constant here comes from running the kernels.

The bf16 store term is 2^-8, not the 2^-9 first written down for it: bf16 keeps 8 significand bits (7 stored), so an
ulp is 2^-7 of the binade's lower end and round-to-nearest is off by up to half of that, 2^-8 |v| for v just above a
power of two.  2^-9 is half an ulp only relative to the binade's UPPER end; the f32 CPU matmul rounded to bf16
(tests/test_gemm_checker.py) already misses a 2^-9 bound by 1.6x on the first case.

Outputs live inside a NaN-filled buffer with guard rows and columns on every side (Guarded): an element the kernel
never wrote stays NaN and fails, and a write outside the M x N block shows up as a non-NaN guard.
"""
import math

import torch

from parity_log import check as log_check

U = 2.0 ** -23
BF16_ROUND = 2.0 ** -8      # unit roundoff of a round-to-nearest bf16 store (8 significand bits)
GELU_MAX_SLOPE = 1.13
GELU_F32_ERR = 3.5e-7    # common.h gelu_erf / DESIGN.md §3.2
GELU_BF16_ERR = 2.6e-5   # common.h gelu_bf16out / DESIGN.md §3.2
ERF_F32_ERR = 4.4e-7     # common.h gelu_erf: the A-S 7.1.26 erf as evaluated in f32

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2

# tmae_gemm_force_tile's candidate list: (BN weight rows, BM token rows), index = position
TILES = ((256, 256), (128, 128), (64, 128), (32, 128), (64, 64), (32, 64), (256, 192), (128, 160), (128, 192))
BF16_ONLY = (0, 6, 7, 8)                                   # the bf16 LDS-DMA path alone instantiates these
F32_TILES = tuple(i for i in range(len(TILES)) if i not in BF16_ONLY)
DEEP_STAGES = {(32, 64): 4, (64, 64): 4, (32, 128): 4, (64, 128): 3}  # bf16 LDS-DMA, from 8 K-steps on


def epc(dtype):
    """elements per 16-B chunk"""
    return 8 if dtype == torch.bfloat16 else 4


def bke(dtype):
    """elements per K-step (128-B LDS rows)"""
    return 8 * epc(dtype)


def expected_stages(dtype, tile, K):
    """LDS stages the LDS-DMA kernel is documented to take, restated independently of the library"""
    if dtype == torch.bfloat16 and tile in DEEP_STAGES and -(-K // 64) >= 8:
        return DEEP_STAGES[tile]
    return 2


def case_shape(case, tile, dtype):
    """(M, N, K) of cases A-E for a tile: A one partial tile, one chunk, an N tail on the 4-column path; B seven
    K-steps (two-stage ring everywhere), ragged last tiles, N % 8 == 0; C nine K-steps, the last one chunk (deep rings,
    checked addresses on the tail step); D the smallest K of the deep ring, no tail; E 11 x 3 tiles of one K-step
    (tile_order's remainder group, a grid of 33 for xcd_remap)"""
    bn, bm = tile
    e, k = epc(dtype), bke(dtype)
    return {"A": (1, bn - 4, e), "B": (2 * bm + 1, bn + 8, 7 * k), "C": (bm - 1, 2 * bn - 4, 8 * k + e),
            "D": (bm + 3, bn, 8 * k), "E": (10 * bm + 5, 2 * bn + 8, k)}[case]


def operands(M, N, K, dtype, seed=0):
    """x [M][K], w [N][K] rounded to dtype, f32 bias [N]; values of order 1 on the output"""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + seed)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype)
    b = torch.randn(N, generator=g)
    return x, w, b


def linear_terms(x, w, bias=None, extra=None):
    """float64 z = x w^T + bias + extra and S = |x| |w|^T + |bias| + |extra| of already rounded operands"""
    xd, wd = x.double(), w.double()
    z, S = xd @ wd.t(), xd.abs() @ wd.abs().t()
    for t in (bias, extra):
        if t is not None:
            z, S = z + t.double(), S + t.double().abs()
    return z, S


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def reference(z, S, K, act=ACT_NONE, gelu="f32", store_bf16=False):
    """(ref, bound) of act(z) for a reduction of length K; gelu = "f32" (gelu_erf, f32 stores) or "bf16"
    (gelu_bf16out, epilogues storing bf16); store_bf16 adds the rounding of a bf16 store"""
    e = (K + 2) * U * S
    if act == ACT_GELU:
        ref = gelu64(z)
        if gelu == "f32":
            bound = GELU_MAX_SLOPE * e + 0.5 * z.abs() * GELU_F32_ERR + 4 * 2.0 ** -24 * ref.abs()
        else:
            bound = GELU_MAX_SLOPE * e + GELU_BF16_ERR
    elif act == ACT_RELU:
        ref, bound = z.clamp_min(0.0), e
    else:
        ref, bound = z, e
    if store_bf16:
        bound = bound + BF16_ROUND * (ref.abs() + bound)
    return ref, bound


def gelu_grad64(p):
    """(GELU'(p), |GELU''(p)|) in float64"""
    phi = torch.exp(-0.5 * p * p) / math.sqrt(2.0 * math.pi)
    return 0.5 * (1.0 + torch.erf(p / math.sqrt(2.0))) + p * phi, (phi * (2.0 - p * p)).abs()


def dgrad_reference(a, S, K, pre=None, acc0=None):
    """(ref, bound) of the data-gradient epilogue out = acc * GELU'(pre) (+ acc0) stored in f32.

    acc has the linear bound e = (K + 2) u S.  common.h gelu_grad is Phi(p) + p phi(p) with the A-S 7.1.26 erf of
    gelu_erf; it states no error of its own, so the factor's bound d is built from that formula: the erf, evaluated
    in f32, is off by at most 4.4e-7 (stated beside gelu_erf), Phi = 0.5 (1 + erf) by half of it; the f32
    evaluation perturbs the argument by at most an f32 ulp, which moves the factor by |GELU''(p)| ulp(p) to first
    order; the closing multiplications and the addition round four times, 4 2^-24 |g|.  Then
        |out - a g| <= |g| e + (|a| + e) d + u |a g|            (the last term: the product's own rounding)
    and an accumulation into a non-zero f32 buffer adds one more rounding, u (|acc0| + |a g| + bound so far)."""
    e = (K + 2) * U * S
    if pre is None:
        ref, bound = a, e
    else:
        p = pre.double()
        g, g2 = gelu_grad64(p)
        d = 0.5 * ERF_F32_ERR + g2 * (U * p.abs()) + 4 * 2.0 ** -24 * g.abs()
        ref = a * g
        bound = g.abs() * e + (a.abs() + e) * d + U * ref.abs()
    if acc0 is not None:
        bound = bound + U * (acc0.double().abs() + ref.abs() + bound)
        ref = ref + acc0.double()
    return ref, bound


class Guarded:
    """An M x N output inside a NaN-filled (M + 2 GR) x (N + 2 GC) buffer.  view() is what the kernel gets: M rows
    of leading dimension N + 2 GC starting at the block (16-B aligned: GC = 8 elements), result() the block."""
    GR, GC = 2, 8

    def __init__(self, M, N, dtype, device="cpu", init=None):
        self.M, self.N, self.ld = M, N, N + 2 * self.GC
        self.buf = torch.full((M + 2 * self.GR, self.ld), float("nan"), dtype=dtype, device=device)
        if init is not None:
            self.block()[...] = init.to(dtype).to(device)

    def block(self):
        return self.buf[self.GR:self.GR + self.M, self.GC:self.GC + self.N]

    def view(self):
        off = self.GR * self.ld + self.GC
        return self.buf.view(-1)[off:off + self.M * self.ld].view(self.M, self.ld)

    def guard_hits(self):
        """number of guard elements that are no longer NaN"""
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        keep[self.GR:self.GR + self.M, self.GC:self.GC + self.N] = False
        return int((~torch.isnan(self.buf[keep].float())).sum())

    def result(self):
        return self.block().detach().double().cpu()


def ratio(out, ref, bound):
    """largest |out - ref| / bound over the elements; inf for a NaN (an element never written) or an error over a
    zero bound"""
    err = (out.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def check_out(metric, g, ref, bound, log=True):
    """the one verdict: guards untouched, every element of the block within its bound; returns the largest ratio"""
    hits = g.guard_hits()
    assert hits == 0, f"{metric}: {hits} guard elements outside the {g.M} x {g.N} block were written"
    r = ratio(g.result(), ref, bound)
    if log:
        log_check(metric, r, 1.0, strict=False)
    assert r <= 1.0, f"{metric}: error / bound = {r:.3g} (an element is off by more than its bound, or never written)"
    return r
