"""Every tile and ring depth of the MFMA GEMM core (csrc/gemm_core.h launch_gemm), forced one at a time with
ops.force_gemm_tile and compared element by element with a float64 CPU reference of the rounded operands under the
derived per-element bounds of tests/gemm_check.py (read its docstring for the derivation; the bf16 store term there is
2^-8, the unit roundoff of 8 significand bits, not 2^-9).

The chooser sends every small problem to the 32 x 64 tile, so without the hook the other eight tiles, the three- and
four-stage rings at a barely long enough K, the partial DMA round of the 160-row tile, the one-block-behind operand
fetch of the 256 x 256 data-gradient epilogue, tile_order's remainder group and xcd_remap on a grid that is no
multiple of 8 are reached only by whole-model runs under a relative-L2 bound.  Shapes (gemm_check.case_shape), per
tile BN x BM, BKE = 64 bf16 / 32 f32 elements per K-step, EPC = 8 / 4 per 16-B chunk:

    A  1 x (BN - 4) x EPC              one partial tile, one chunk, an N tail on the 4-column path
    B  (2 BM + 1) x (BN + 8) x 7 BKE   two-stage ring on every tile, ragged last tiles, bf16-first epilogue (N % 8 == 0)
    C  (BM - 1) x (2 BN - 4) x (8 BKE + EPC)   nine K-steps, the last one chunk: deep rings, checked tail addresses
    D  (BM + 3) x BN x 8 BKE           the smallest K that takes the deep ring, no tail
    E  (10 BM + 5) x (2 BN + 8) x BKE  11 x 3 tiles: tile_order's remainder group, a grid of 33

Every output sits in a NaN-filled buffer with guard rows and columns (gemm_check.Guarded), every case asserts through
ops.gemm_plan that the forced tile and the expected ring depth are what the library launches, and the last test
asserts that the module exercised every (dtype, tile, stages) the library can instantiate.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_check as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
ALL = tuple(range(len(gc.TILES)))
SEEN = set()  # (dtype name, tile, stages) of the LDS-DMA launches this module made


@pytest.fixture(autouse=True)
def _reset_tile(tmae):
    yield
    from textmae_amd import _lib

    _lib.value("tmae_gemm_force_tile", -1)


def _tid(i):
    return "%dx%d" % gc.TILES[i]


def tiles(idx):
    return pytest.mark.parametrize("ti", idx, ids=[_tid(i) for i in idx])


def cases(names):
    return pytest.mark.parametrize("case", list(names))


def _name(dtype):
    return "bf16" if dtype == BF16 else "f32"


def assert_plan(tmae, ti, M, N, K, dtype, batch=1, glds=True):
    """the plan (which shares choose_tile and the ring rule with every launch) names the forced tile and the ring
    depth this K must get; call inside force_gemm_tile"""
    bn, bm = gc.TILES[ti]
    stages = gc.expected_stages(dtype, (bn, bm), K)
    plan = tmae.ops.gemm_plan(M, N, K, dtype, batch)
    k = 64 if dtype == BF16 else 32
    assert plan == f"glds<{_name(dtype)},{bn}x{bm},{8 if bn == 256 else 4}w,BK{k}x{stages}>", plan
    if glds:
        SEEN.add((_name(dtype), (bn, bm), stages))


@functools.lru_cache(maxsize=4)
def problem(M, N, K, dtype):
    """rounded operands and the float64 terms of x w^T + b, computed once per shape and shared (never modified)"""
    x, w, b = gc.operands(M, N, K, dtype)
    z, S = gc.linear_terms(x, w, b)
    return x, w, b, z, S


def dev(t):
    return t.to(DEV)


# ------------------------------------------------------------------------------------ ops.linear
@tiles(ALL)
@cases("ABCDE")
@pytest.mark.parametrize("act", [0, 1])
def test_linear_bf16(tmae, ti, case, act):
    """bf16 -> bf16: the bf16-first epilogue where N % 8 == 0 (B, D, E), the f32 transpose with 4-column tails else"""
    M, N, K = gc.case_shape(case, gc.TILES[ti], BF16)
    x, w, b, z, S = problem(M, N, K, BF16)
    out = gc.Guarded(M, N, BF16, DEV)
    with tmae.ops.force_gemm_tile(ti):
        assert_plan(tmae, ti, M, N, K, BF16)
        tmae.ops.linear(dev(x), dev(w), dev(b), BF16, act=act, out=out.view(), M=M)
    torch.cuda.synchronize()
    ref, bound = gc.reference(z, S, K, act, gelu="bf16", store_bf16=True)
    gc.check_out(f"ratio:linear_bf16:{_tid(ti)}:{case}:act{act}", out, ref, bound)


@tiles(ALL)
@cases("BC")
@pytest.mark.parametrize("act", [0, 1])
def test_linear_bf16_out32(tmae, ti, case, act):
    """bf16 output plus the f32 copy: the f32 transpose with a second store (the copy holds the unrounded values)"""
    M, N, K = gc.case_shape(case, gc.TILES[ti], BF16)
    x, w, b, z, S = problem(M, N, K, BF16)
    out, out32 = gc.Guarded(M, N, BF16, DEV), gc.Guarded(M, N, F32, DEV)
    with tmae.ops.force_gemm_tile(ti):
        assert_plan(tmae, ti, M, N, K, BF16)
        tmae.ops.linear(dev(x), dev(w), dev(b), BF16, act=act, out=out.view(), M=M, out32=out32.view())
    torch.cuda.synchronize()
    ref, bound = gc.reference(z, S, K, act, gelu="bf16", store_bf16=True)
    gc.check_out(f"ratio:linear_out32_bf16:{_tid(ti)}:{case}:act{act}", out, ref, bound)
    ref, bound = gc.reference(z, S, K, act, gelu="bf16")
    gc.check_out(f"ratio:linear_out32_f32:{_tid(ti)}:{case}:act{act}", out32, ref, bound)


@tiles(ALL)
@cases("BC")
@pytest.mark.parametrize("act", [0, 1])
def test_linear_bf16_f32_output(tmae, ti, case, act):
    """bf16 operands, f32 output (the erf GELU)"""
    M, N, K = gc.case_shape(case, gc.TILES[ti], BF16)
    x, w, b, z, S = problem(M, N, K, BF16)
    out = gc.Guarded(M, N, F32, DEV)
    with tmae.ops.force_gemm_tile(ti):
        assert_plan(tmae, ti, M, N, K, BF16)
        tmae.ops.linear(dev(x), dev(w), dev(b), BF16, act=act, out=out.view(), M=M)
    torch.cuda.synchronize()
    ref, bound = gc.reference(z, S, K, act, gelu="f32")
    gc.check_out(f"ratio:linear_bf16_f32out:{_tid(ti)}:{case}:act{act}", out, ref, bound)


@tiles(gc.F32_TILES)
@cases("ABCDE")
@pytest.mark.parametrize("act", [0, 1])
def test_linear_f32(tmae, ti, case, act):
    """the f32 parity path: five tiles, the two-stage ring only (the deep rings need a 2-byte element)"""
    M, N, K = gc.case_shape(case, gc.TILES[ti], F32)
    x, w, b, z, S = problem(M, N, K, F32)
    out = gc.Guarded(M, N, F32, DEV)
    with tmae.ops.force_gemm_tile(ti):
        assert_plan(tmae, ti, M, N, K, F32)
        tmae.ops.linear(dev(x), dev(w), dev(b), F32, act=act, out=out.view(), M=M)
    torch.cuda.synchronize()
    ref, bound = gc.reference(z, S, K, act, gelu="f32")
    gc.check_out(f"ratio:linear_f32:{_tid(ti)}:{case}:act{act}", out, ref, bound)


@tiles(gc.F32_TILES)
@cases("ABC")
@pytest.mark.parametrize("act", [0, 1])
def test_linear_f32_source_reg_kernel(tmae, ti, case, act):
    """an f32 x into bf16 weights: gemm_reg_kernel (global -> VGPR -> LDS, converting on the way), which takes the
    five tiles of the non-bf16-only set -- the f32 plan's tile choice (choose_tile without the big tiles) -- and
    has a two-buffer ring only.  x is rounded to bf16 by the kernel; the reference rounds it the same way."""
    M, N, K = gc.case_shape(case, gc.TILES[ti], BF16)
    x, w, b, z, S = problem(M, N, K, BF16)
    g = torch.Generator().manual_seed(M + N + K)
    x32 = x.float() + x.float().abs() * (torch.rand(x.shape, generator=g) - 0.5) * 2.0 ** -10  # rounds back to x
    assert torch.equal(x32.to(BF16), x)
    out = gc.Guarded(M, N, BF16, DEV)
    with tmae.ops.force_gemm_tile(ti):
        bn, bm = gc.TILES[ti]
        assert f",{bn}x{bm},4w," in tmae.ops.gemm_plan(M, N, K, F32)
        tmae.ops.linear(dev(x32), dev(w), dev(b), BF16, act=act, out=out.view(), M=M)
    torch.cuda.synchronize()
    ref, bound = gc.reference(z, S, K, act, gelu="bf16", store_bf16=True)
    gc.check_out(f"ratio:linear_reg:{_tid(ti)}:{case}:act{act}", out, ref, bound)


@tiles((7, 0))
def test_linear_strided_rows(tmae, ti):
    """row_group / group_stride / row_offset with the cls row of every group dropped (as the LayerNorm test does),
    case B on the 160-row tile (partial DMA round) and the 256 x 256 tile"""
    M, N, K = gc.case_shape("B", gc.TILES[ti], BF16)
    x, w, b, z, S = problem(M, N, K, BF16)
    groups = 3
    glen = M // groups
    assert groups * glen == M
    g = torch.Generator().manual_seed(7)
    xs = torch.randn(groups, glen + 1, K, generator=g).to(BF16)  # row 0 of every group is not an operand
    xs[:, 1:] = x.view(groups, glen, K)
    out = gc.Guarded(M, N, BF16, DEV)
    with tmae.ops.force_gemm_tile(ti):
        assert_plan(tmae, ti, M, N, K, BF16)
        tmae.ops.linear(dev(xs), dev(w), dev(b), BF16, out=out.view(), M=M, ldx=K, row_group=glen,
                        group_stride=glen + 1, row_offset=1)
    torch.cuda.synchronize()
    ref, bound = gc.reference(z, S, K, store_bf16=True)
    gc.check_out(f"ratio:linear_strided:{_tid(ti)}:B", out, ref, bound)


# ------------------------------------------------------------------------------------ ops.linear_residual
@pytest.mark.parametrize("dtype,ti", [(BF16, i) for i in ALL] + [(F32, i) for i in gc.F32_TILES],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else _tid(v))
@cases("BC")
def test_linear_residual(tmae, dtype, ti, case):
    """resid += x W^T + b in f32 (the residual rows fetched one 16-row block ahead); S includes |resid|"""
    M, N, K = gc.case_shape(case, gc.TILES[ti], dtype)
    x, w, b, _, _ = problem(M, N, K, dtype)
    r0 = torch.randn(M, N, generator=torch.Generator().manual_seed(M * N))
    z, S = gc.linear_terms(x, w, b, r0)
    res = gc.Guarded(M, N, F32, DEV, init=r0)
    with tmae.ops.force_gemm_tile(ti):
        assert_plan(tmae, ti, M, N, K, dtype)
        tmae.ops.linear_residual(dev(x), dev(w), dev(b), res.view(), dtype)
    torch.cuda.synchronize()
    ref, bound = gc.reference(z, S, K)
    gc.check_out(f"ratio:linear_residual_{_name(dtype)}:{_tid(ti)}:{case}", res, ref, bound)


# ------------------------------------------------------------------------------------ train_ops.dgrad_linear
@pytest.mark.parametrize("dtype,ti", [(BF16, i) for i in ALL] + [(F32, i) for i in gc.F32_TILES],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else _tid(v))
@cases("BC")
@pytest.mark.parametrize("accumulate", [False, True])
def test_dgrad_linear(tmae, dtype, ti, case, accumulate):
    """dx = (dy W) * GELU'(pre) into an f32 out, and again with the f32 accumulation into a non-zero buffer; on
    256 x 256 the epilogue's operand sets no longer fit beside the accumulators and are fetched one block behind.
    The output columns are the case's N and the reduction its K (dy [M][K], W^T [N][K]).  The bound of the GELU'
    factor is derived in gemm_check.dgrad_reference."""
    from textmae_amd import train_ops

    M, N, K = gc.case_shape(case, gc.TILES[ti], dtype)
    dy, wt, _, _, _ = problem(M, N, K, dtype)
    a, S = gc.linear_terms(dy, wt)
    g = torch.Generator().manual_seed(M + 3 * N)
    pre = (torch.randn(M, N, generator=g) * 1.5).to(dtype)
    acc0 = torch.randn(M, N, generator=g) if accumulate else None
    out = gc.Guarded(M, N, F32, DEV)
    acc = gc.Guarded(M, N, F32, DEV, init=acc0) if accumulate else None
    with tmae.ops.force_gemm_tile(ti):
        assert_plan(tmae, ti, M, N, K, dtype)
        # the entry point's N is the reduction and its K the output width
        train_ops.dgrad_linear(dev(dy), dev(wt), M, K, N, dtype, out=out.view(), pre=dev(pre), ldo=out.ld,
                               acc32=acc.view() if accumulate else None)
    torch.cuda.synchronize()
    ref, bound = gc.dgrad_reference(a, S, K, pre)
    tag = f"{_name(dtype)}:{_tid(ti)}:{case}"
    gc.check_out(f"ratio:dgrad_out:{tag}:acc{int(accumulate)}", out, ref, bound)
    if accumulate:
        ref, bound = gc.dgrad_reference(a, S, K, pre, acc0)
        gc.check_out(f"ratio:dgrad_acc32:{tag}", acc, ref, bound)


# ------------------------------------------------------------------------------------ ops.conv3x3, implicit GEMM
# Every geometry below is one tmae_conv3x3 sends to the implicit GEMM: conv.hip conv_go takes the halo-staged kernel
# only when   conv_halo_ok(H, W, stride, N, nb) = H == 12 && W == 12 && stride == 1 && N <= 2048 && nb <= 12
# (conv_halo.h) holds, and only for bf16.  A 6 x 6 map fails H == 12; the 12 x 12 map is run at stride 2.
def _conv_problem(n, c1, c2, H, stride, cout, dtype, nprob=1):
    cin = c1 + c2
    g = torch.Generator().manual_seed(cin * 131 + H * 17 + stride + cout + nprob)
    x = torch.randn(n, cin, H, H, generator=g).to(dtype)
    w = (torch.randn(nprob, cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).to(dtype)
    b = torch.randn(nprob, cout, generator=g)
    refs = []
    for p in range(nprob):
        z = F.conv2d(x.double(), w[p].double(), b[p].double(), stride=stride, padding=1)
        S = F.conv2d(x.double().abs(), w[p].double().abs(), b[p].double().abs(), stride=stride, padding=1)
        refs.append((z.permute(0, 2, 3, 1).reshape(-1, cout), S.permute(0, 2, 3, 1).reshape(-1, cout)))
    Ho = (H - 1) // stride + 1
    xa = x[:, :c1].permute(0, 2, 3, 1).contiguous()
    xb = x[:, c1:].permute(0, 2, 3, 1).contiguous() if c2 else None
    wk = w.permute(0, 1, 3, 4, 2).reshape(nprob, cout, 9 * cin).contiguous()  # [Cout][ky][kx][Cin]
    return xa, xb, wk, b, refs, n * Ho * Ho, 9 * cin


CONV1 = [(BF16, i) for i in ALL] + [(F32, i) for i in gc.F32_TILES]


@pytest.mark.parametrize("dtype,ti", CONV1, ids=lambda v: _name(v) if isinstance(v, torch.dtype) else _tid(v))
def test_conv3x3_narrow(tmae, dtype, ti):
    """Cin = 72 (ConvSrc: the tap divided out of k per chunk), 6 x 6, 3 images, cout = BN + 8, GELU"""
    n, cin, H, cout = 3, 72, 6, gc.TILES[ti][0] + 8
    xa, _, wk, b, refs, M, K = _conv_problem(n, cin, 0, H, 1, cout, dtype)
    y = gc.Guarded(M, cout, dtype, DEV)
    with tmae.ops.force_gemm_tile(ti):
        assert_plan(tmae, ti, M, cout, K, dtype)
        tmae.ops.conv3x3(dev(xa), cin, cin, n, H, H, dev(wk[0]), dev(b[0]), y.view(), y.ld, cout, dtype, act=1)
    torch.cuda.synchronize()
    bf = dtype == BF16
    ref, bound = gc.reference(*refs[0], K, gc.ACT_GELU, gelu="bf16" if bf else "f32", store_bf16=bf)
    gc.check_out(f"ratio:conv_narrow_{_name(dtype)}:{_tid(ti)}", y, ref, bound)


@tiles(ALL)
@pytest.mark.parametrize("H,stride", [(6, 1), (12, 2)])
def test_conv3x3_wide_two_segments(tmae, ti, H, stride):
    """Cin = 136 = 96 + 40 (ConvSrcIt: a tap crossing inside a 64-channel K-step and a segment switch), 6 x 6 and
    12 x 12 at stride 2; on 128 x 160 the iterator advances in the lanes of the partial DMA round too"""
    n, c1, c2, cout = 3, 96, 40, gc.TILES[ti][0] + 8
    xa, xb, wk, b, refs, M, K = _conv_problem(n, c1, c2, H, stride, cout, BF16)
    y = gc.Guarded(M, cout, BF16, DEV)
    with tmae.ops.force_gemm_tile(ti):
        assert_plan(tmae, ti, M, cout, K, BF16)
        tmae.ops.conv3x3(dev(xa), c1, c1, n, H, H, dev(wk[0]), dev(b[0]), y.view(), y.ld, cout, BF16, stride=stride,
                         x2=dev(xb), c2=c2, ld2=c2)
    torch.cuda.synchronize()
    ref, bound = gc.reference(*refs[0], K, store_bf16=True)
    gc.check_out(f"ratio:conv_wide:{_tid(ti)}:{H}s{stride}", y, ref, bound)


@tiles((5, 7, 0))
def test_conv3x3_wide_batched(tmae, ti):
    """nb = (2, 3) problems with their own weights, biases and outputs through `strides`, one shared two-segment
    input of 136 channels (the K iterator must start from the batch-adjusted pointers), GELU"""
    n, c1, c2, H, nb1, nb2 = 3, 96, 40, 6, 2, 3
    cout = gc.TILES[ti][0] + 8
    xa, xb, wk, b, refs, M, K = _conv_problem(n, c1, c2, H, 1, cout, BF16, nprob=nb1 * nb2)
    ys = [gc.Guarded(M, cout, BF16) for _ in range(nb1 * nb2)]
    ybuf = torch.stack([g.buf for g in ys]).to(DEV)  # problem p's guarded buffer p * per elements on
    per, ld, off = ys[0].buf.numel(), ys[0].ld, ys[0].GR * ys[0].ld + ys[0].GC
    with tmae.ops.force_gemm_tile(ti):
        assert_plan(tmae, ti, M, cout, K, BF16, batch=nb1 * nb2)
        tmae.ops.conv3x3(dev(xa), c1, c1, n, H, H, dev(wk), dev(b), ybuf.data_ptr() + 2 * off, ld, cout, BF16, act=1,
                         x2=dev(xb), c2=c2, ld2=c2, y_f32=False, nb=(nb1, nb2),
                         strides={"w": (nb2 * cout * K, cout * K), "b": (nb2 * cout, cout), "y": (nb2 * per, per)})
    torch.cuda.synchronize()
    for p, g in enumerate(ys):
        g.buf = ybuf[p]
        ref, bound = gc.reference(*refs[p], K, gc.ACT_GELU, gelu="bf16", store_bf16=True)
        gc.check_out(f"ratio:conv_wide_batched:{_tid(ti)}:p{p}", g, ref, bound)


# ------------------------------------------------------------------------------------ coverage (keep last)
def test_every_instantiation_was_exercised(tmae):
    """the union of (dtype, tile, stages) the cases above launched equals what the library can instantiate, asked
    of the library itself (tmae_gemm_plan shares the ring rule with launch_one): nine bf16 tiles and five f32 tiles
    on the two-stage ring, four deep-ring variants in bf16, none in f32"""
    can = set()
    for dtype in (BF16, F32):
        for ti, (bn, bm) in enumerate(gc.TILES):
            for K in (8, 1 << 20):
                with tmae.ops.force_gemm_tile(ti):
                    plan = tmae.ops.gemm_plan(4096, 4096, K, dtype)
                if f",{bn}x{bm}," in plan:  # the path has the tile
                    can.add((_name(dtype), (bn, bm), int(plan.rsplit("x", 1)[1].rstrip(">"))))
    assert len(can) == 9 + 4 + 5 and sum(1 for d, _, s in can if d == "f32" and s > 2) == 0, sorted(can)
    assert SEEN == can, (sorted(can - SEEN), sorted(SEEN - can))
