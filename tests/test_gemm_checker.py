"""The GEMM tile tests' checker and tile hook, without a GPU (CPU only).

1. A plain f32 CPU matmul of the rounded operands, and its bf16-rounded copy, stay inside the checker's bounds at every
   case shape of tests/test_gpu_gemm_tiles.py: the reference's own error does not eat the bound.
2. The checker rejects the float64 reference after each fault a tiled kernel can produce: a single element 2 bf16 ulp
   off at a small-magnitude position, a dropped K chunk, swapped column groups, an unwritten row, a row past M.
3. tmae_gemm_force_tile / ops.force_gemm_tile: tmae_gemm_plan names the forced tile and the ring depth actually
   launched for every (dtype, tile, K); no device work, so this runs wherever the library loads.
"""
import pytest
import torch
import torch.nn.functional as F

import gemm_check as gc

BF16, F32 = torch.bfloat16, torch.float32
SMALL, LARGE = (32, 64), (256, 256)


def _written(M, N, dtype, values):
    g = gc.Guarded(M, N, dtype)
    g.view()[:, :N] = values.to(dtype)
    return g


# ------------------------------------------------------------------------------------ the reference fits the bound
@pytest.mark.parametrize("case", "ABCDE")
@pytest.mark.parametrize("tile,dtype", [(SMALL, BF16), (LARGE, BF16), (SMALL, F32), ((128, 128), F32)])
def test_cpu_matmul_within_bound(case, tile, dtype):
    M, N, K = gc.case_shape(case, tile, dtype)
    x, w, b = gc.operands(M, N, K, dtype)
    z, S = gc.linear_terms(x, w, b)
    y = F.linear(x.float(), w.float(), b)  # f32 accumulation in whatever order the CPU BLAS takes
    for act, yy in ((gc.ACT_NONE, y), (gc.ACT_GELU, F.gelu(y)), (gc.ACT_RELU, F.relu(y))):
        ref, bound = gc.reference(z, S, K, act, gelu="f32")
        assert gc.check_out(f"cpu_f32_{act}", _written(M, N, F32, yy), ref, bound, log=False) <= 1.0
        # the bf16 store of the same values (the bf16 GELU's bound is the wider one: the exact erf GELU fits it)
        ref, bound = gc.reference(z, S, K, act, gelu="bf16", store_bf16=True)
        assert gc.check_out(f"cpu_bf16_{act}", _written(M, N, BF16, yy), ref, bound, log=False) <= 1.0


# ------------------------------------------------------------------------------------ faults are rejected
FAULT_CASES = [("B", SMALL), ("C", SMALL), ("B", (128, 160)), ("E", (64, 64))]


def _setup(case, tile, out_dtype):
    M, N, K = gc.case_shape(case, tile, BF16)
    x, w, b = gc.operands(M, N, K, BF16)
    z, S = gc.linear_terms(x, w, b)
    ref, bound = gc.reference(z, S, K, store_bf16=out_dtype == BF16)
    g = _written(M, N, out_dtype, ref)
    assert gc.check_out("clean", g, ref, bound, log=False) <= 1.0  # the rounded reference itself passes
    return (M, N, K), (x, w, b), g, ref, bound


@pytest.mark.parametrize("case,tile", FAULT_CASES)
def test_rejects_two_ulp_at_small_magnitude(case, tile):
    """one element of a bf16 output moved by 2 ulp, at the position whose |ref| is the largest below the median (so a
    max-error / max-magnitude metric would not see it).  bf16 stores only: for an f32 store 2 ulp = 2^-22 |ref| lies
    inside (K + 2) 2^-23 S >= 5 2^-23 |ref| by construction, i.e. it is a legitimate summation-order difference."""
    (M, N, K), _, g, ref, bound = _setup(case, tile, BF16)
    a = ref.abs().flatten()
    order = torch.argsort(a)
    pos = int(order[(a.numel() - 1) // 2 - 1])  # torch's median is the sorted element (n - 1) // 2
    assert a[pos] < a.median()
    blk = g.block()
    q = blk[pos // N, pos % N].clone()
    ulp = 2.0 ** (torch.frexp(q.float().abs())[1].item() - 8)  # bf16: 8 significand bits
    moved = (q.float() + 2 * ulp).to(BF16)
    assert float(moved) - float(q) == 2 * ulp
    blk[pos // N, pos % N] = moved
    assert float((blk.double() - ref).abs().max() / ref.abs().max()) < 7e-3  # the suite's old bf16 metric passes it
    with pytest.raises(AssertionError):
        gc.check_out("two_ulp", g, ref, bound, log=False)


@pytest.mark.parametrize("out_dtype", [F32, BF16])
@pytest.mark.parametrize("case,tile", FAULT_CASES)
def test_rejects_dropped_k_chunk(case, tile, out_dtype):
    (M, N, K), (x, w, b), g, ref, bound = _setup(case, tile, out_dtype)
    r = M - 1
    short = ref[r] - x[r, K - 8:].double() @ w[:, K - 8:].double().t()
    g.block()[r] = short.to(out_dtype)
    with pytest.raises(AssertionError):
        gc.check_out("dropped_chunk", g, ref, bound, log=False)


@pytest.mark.parametrize("out_dtype", [F32, BF16])
@pytest.mark.parametrize("case,tile", FAULT_CASES)
def test_rejects_swapped_column_groups(case, tile, out_dtype):
    (M, N, K), _, g, ref, bound = _setup(case, tile, out_dtype)
    blk, r = g.block(), M // 2
    a, b = blk[r, 8:16].clone(), blk[r, 16:24].clone()
    blk[r, 8:16], blk[r, 16:24] = b, a
    with pytest.raises(AssertionError):
        gc.check_out("swapped_groups", g, ref, bound, log=False)


@pytest.mark.parametrize("out_dtype", [F32, BF16])
@pytest.mark.parametrize("case,tile", FAULT_CASES)
def test_rejects_unwritten_last_row(case, tile, out_dtype):
    (M, N, K), _, g, ref, bound = _setup(case, tile, out_dtype)
    g.block()[M - 1] = float("nan")  # what the pre-fill leaves when the kernel skips the row
    with pytest.raises(AssertionError):
        gc.check_out("unwritten_row", g, ref, bound, log=False)


@pytest.mark.parametrize("out_dtype", [F32, BF16])
@pytest.mark.parametrize("case,tile", FAULT_CASES)
def test_rejects_row_past_m(case, tile, out_dtype):
    (M, N, K), _, g, ref, bound = _setup(case, tile, out_dtype)
    g.buf[g.GR + M, g.GC:g.GC + N] = g.block()[M - 1]  # row M: the first guard row below the block
    with pytest.raises(AssertionError, match="guard"):
        gc.check_out("row_past_m", g, ref, bound, log=False)
    g2 = _setup(case, tile, out_dtype)[2]
    g2.view()[0, N] = 1.0  # one column past N
    with pytest.raises(AssertionError, match="guard"):
        gc.check_out("col_past_n", g2, ref, bound, log=False)


# ------------------------------------------------------------------------------------ the tile hook and the plan
@pytest.fixture(autouse=True)
def _reset_tile(tmae):
    yield
    from textmae_amd import _lib

    _lib.value("tmae_gemm_force_tile", -1)


def test_force_tile_returns_previous_and_restores(tmae):
    from textmae_amd import _lib

    assert tmae.ops.GEMM_TILES == gc.TILES
    assert _lib.value("tmae_gemm_force_tile", 3) == -1
    assert _lib.value("tmae_gemm_force_tile", 99) == 3    # out of range: back to the chooser
    assert _lib.value("tmae_gemm_force_tile", -1) == -1
    free = tmae.ops.gemm_plan(300, 64, 32, BF16)
    with tmae.ops.force_gemm_tile(7):
        with tmae.ops.force_gemm_tile(0):
            assert "256x256,8w" in tmae.ops.gemm_plan(300, 64, 32, BF16)
        assert "128x160,4w" in tmae.ops.gemm_plan(300, 64, 32, BF16)
    assert tmae.ops.gemm_plan(300, 64, 32, BF16) == free
    with pytest.raises(RuntimeError):
        with tmae.ops.force_gemm_tile(2):
            raise RuntimeError("body fails")
    assert tmae.ops.gemm_plan(300, 64, 32, BF16) == free
    with pytest.raises(ValueError):
        with tmae.ops.force_gemm_tile(9):
            pass


def test_unforced_plan_is_the_chooser(tmae):
    """the picks the issue was written from: small problems land on 32 x 64, the 9280 x 2304 x 768 case on
    128 x 128 (f32) / 128 x 192 (bf16); the two-stage ring below 8 K-steps, the four-stage one from 8 on"""
    assert tmae.ops.gemm_plan(300, 64, 32, F32) == "glds<f32,32x64,4w,BK32x2>"
    assert tmae.ops.gemm_plan(77, 32, 96, BF16) == "glds<bf16,32x64,4w,BK64x2>"
    assert tmae.ops.gemm_plan(129, 704, 640, BF16) == "glds<bf16,32x64,4w,BK64x4>"
    assert tmae.ops.gemm_plan(129, 704, 640, F32) == "glds<f32,32x64,4w,BK32x2>"
    assert tmae.ops.gemm_plan(9280, 2304, 768, F32) == "glds<f32,128x128,4w,BK32x2>"
    assert tmae.ops.gemm_plan(9280, 2304, 768, BF16) == "glds<bf16,128x192,4w,BK64x2>"


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("index", range(len(gc.TILES)))
def test_plan_names_forced_tile_and_stages(tmae, dtype, index):
    bn, bm = gc.TILES[index]
    name, k = ("bf16", 64) if dtype == BF16 else ("f32", 32)
    for K in (gc.epc(dtype), 7 * k, 7 * k + gc.epc(dtype), 8 * k, 8 * k + gc.epc(dtype), 40 * k):
        free = tmae.ops.gemm_plan(500, 200, K, dtype)
        with tmae.ops.force_gemm_tile(index):
            plan = tmae.ops.gemm_plan(500, 200, K, dtype)
        if dtype == F32 and index in gc.BF16_ONLY:
            assert plan == free  # the f32 path has no such tile: the chooser still picks
            continue
        nw = 8 if bn == 256 else 4
        assert plan == f"glds<{name},{bn}x{bm},{nw}w,BK{k}x{gc.expected_stages(dtype, (bn, bm), K)}>", (K, plan)
