"""tmae_conv_dgrad (ConvTSrc in csrc/train.hip: the transposed-conv row source on the GEMM core) element by element.
Rows = n H W input pixels, output columns = cin, K = 9 cout.  Each case (tn_check.D_CASES) is forced onto a tile with
ops.force_gemm_tile and asserted with ops.gemm_plan, in the exact pass (integer operands, bit-equal to the integer
reference) and the bounded pass (float64 torch.nn.grad.conv2d_input, per-element bound): tests/tn_check.py.

    D1  1 x 1 map, cout = one 16-byte chunk   centre tap only; 8 taps per K-step; the second K-step one live chunk
    D2  3 x (5 x 7), stride 2, 24 -> 20       2-3 tap crossings per K-step; parity taps on an odd non-square map
    D3  2 x (6 x 6), stride 2, cout 72        h_a's geometry; a tap boundary inside a K-step
    D4  2 x (12 x 12), stride 1, 192 -> 32    27 K-steps (deep rings on the small tiles); 288 rows
    D5  5 x (2 x 2), stride 2, cout 40        the 64-pixel model's h_a: a 1 x 1 output map

The epilogues run on D2 and D4 with dy rows padded to cout + 8 (NaN) and out / pre inside Guarded buffers: a store in
the operand dtype, an f32 store, out * GELU'(pre), routed accumulation onto f32 buffers, and three problems in one
launch.  Route limits must be multiples of 8 except the last, so D2 (20 channels) is routed 8 / 8 / 4 and only D4
(32 channels) also 16 / 8 / 8 and as a single route.
"""
import functools

import pytest
import torch

import gemm_check as gc
import tn_check as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
PASSES = ((True, "exact"), (False, "bounded"))
TILED = pytest.mark.parametrize("dtype,ti", [(d, t) for d in (BF16, F32) for t in tc.D_TILES[d]],
                                ids=lambda v: tc.dname(v) if isinstance(v, torch.dtype) else "%dx%d" % gc.TILES[v])


@pytest.fixture(autouse=True)
def _reset_tile(tmae):
    yield
    from textmae_amd import _lib

    _lib.value("tmae_gemm_force_tile", -1)


def assert_plan(tmae, ti, M, N, K, dtype, batch=1):
    bn, bm = gc.TILES[ti]
    k = 64 if dtype == BF16 else 32
    want = f"glds<{tc.dname(dtype)},{bn}x{bm},{8 if bn == 256 else 4}w,BK{k}x{gc.expected_stages(dtype, (bn, bm), K)}>"
    plan = tmae.ops.gemm_plan(M, N, K, dtype, batch)
    assert plan == want, (plan, want)


@functools.lru_cache(maxsize=None)
def problem(c, dtype, exact, seed=0):
    """operands and float64 terms of a case, computed once and shared (never modified)"""
    dy, w = tc.dgrad_operands(c, dtype, exact, seed)
    return (tc.nhwc(dy), tc.dgrad_weights(w)) + tc.conv_dgrad_terms(c, dy, w)


def launch(tmae, c, ti, dtype, DY, wd, **kw):
    from textmae_amd import train_ops

    with tmae.ops.force_gemm_tile(ti):
        assert_plan(tmae, ti, c.n * c.H * c.W, c.cin, 9 * c.cout, dtype, kw["batch"][0] if "batch" in kw else 1)
        train_ops.conv_dgrad(DY.ptr, wd, c.n, c.H, c.W, c.stride, c.cout, c.cin, dtype, ldy=DY.ld, **kw)
    torch.cuda.synchronize()


def tag_of(case, ti, dtype, pname):
    return "%s:%s:%dx%d:%s" % (case, tc.dname(dtype), *gc.TILES[ti], pname)


@TILED
@pytest.mark.parametrize("case", list(tc.D_CASES))
def test_conv_dgrad_f32_out(tmae, case, dtype, ti):
    c = tc.dcase(case, gc.TILES[ti][0], dtype)
    rows, K = c.n * c.H * c.W, 9 * c.cout
    for exact, pname in PASSES:
        dy, wd, ref, S = problem(c, dtype, exact)
        DY = tc.Packed([dy], dtype, DEV)
        out = gc.Guarded(rows, c.cin, F32, DEV)
        launch(tmae, c, ti, dtype, DY, wd.to(DEV), out=out.view(), ldo=out.ld)
        gc.check_out(f"ratio:conv_dgrad:{tag_of(case, ti, dtype, pname)}:f32", out, *tc.bounded(ref, S, K, exact))


EPI = pytest.mark.parametrize("case", ["D2", "D4"])


@TILED
@EPI
def test_conv_dgrad_padded_rows_and_gelu(tmae, case, dtype, ti):
    """ldy = cout + 8; an f32 store; out * GELU'(pre) with pre in a Guarded buffer (bounded pass: the factor is not
    an integer); bf16 also the store in the operand dtype"""
    c = tc.dcase(case, gc.TILES[ti][0], dtype)
    rows, K = c.n * c.H * c.W, 9 * c.cout
    for exact, pname in PASSES:
        dy, wd, ref, S = problem(c, dtype, exact)
        DY, wdd = tc.Packed([dy], dtype, DEV, ld=c.cout + 8), wd.to(DEV)
        tag = tag_of(case, ti, dtype, pname)
        out = gc.Guarded(rows, c.cin, F32, DEV)
        launch(tmae, c, ti, dtype, DY, wdd, out=out.view(), ldo=out.ld)
        gc.check_out(f"ratio:conv_dgrad:{tag}:ldy", out, *tc.bounded(ref, S, K, exact))
        if exact:
            continue
        pre = (torch.randn(rows, c.cin, generator=tc.gen(rows, c.cin, ti)) * 1.5).to(dtype)
        gpre = gc.Guarded(rows, c.cin, dtype, DEV, init=pre)
        out = gc.Guarded(rows, c.cin, F32, DEV)
        launch(tmae, c, ti, dtype, DY, wdd, out=out.view(), ldo=out.ld, pre=gpre.view(), ldp=gpre.ld)
        gc.check_out(f"ratio:conv_dgrad:{tag}:gelu", out, *gc.dgrad_reference(ref, S, K, pre))
        assert gpre.guard_hits() == 0 and torch.equal(gpre.block().cpu(), pre)
        if dtype == BF16:
            out = gc.Guarded(rows, c.cin, BF16, DEV)
            launch(tmae, c, ti, dtype, DY, wdd, out=out.view(), ldo=out.ld)
            gc.check_out(f"ratio:conv_dgrad:{tag}:bf16out", out, *tc.bounded(ref, S, K, False, store_bf16=True))


@TILED
@pytest.mark.parametrize("case,widths", [("D2", (8, 8, 4)), ("D4", (16, 8, 8)), ("D4", (32,))],
                         ids=["D2-8_8_4", "D4-16_8_8", "D4-32"])
def test_conv_dgrad_routes(tmae, case, widths, dtype, ti):
    """column ranges += into separate f32 accumulators (the inputs of a torch.cat), random before the launch"""
    c = tc.dcase(case, gc.TILES[ti][0], dtype)
    rows, K = c.n * c.H * c.W, 9 * c.cout
    assert sum(widths) == c.cin
    for exact, pname in PASSES:
        dy, wd, ref, S = problem(c, dtype, exact)
        DY = tc.Packed([dy], dtype, DEV, ld=c.cout + 8)
        g = tc.gen(rows, c.cin, exact, len(widths))
        acc0 = [tc.draw_acc((rows, w), exact, g) for w in widths]
        accs = [gc.Guarded(rows, w, F32, DEV, init=a0) for w, a0 in zip(widths, acc0)]
        launch(tmae, c, ti, dtype, DY, wd.to(DEV), routes=[(a.view(), a.ld, a.N) for a in accs])
        lo = 0
        for i, (a, a0) in enumerate(zip(accs, acc0)):
            hi = lo + a.N
            gc.check_out(f"ratio:conv_dgrad:{tag_of(case, ti, dtype, pname)}:route{i}of{len(widths)}", a,
                         *tc.bounded(ref[:, lo:hi], S[:, lo:hi], K, exact, a0))
            lo = hi


@TILED
@EPI
def test_conv_dgrad_batched(tmae, case, dtype, ti):
    """batch = (3, s_dy, s_wd, s_out, s_pre): three problems with their own dy, weights, output and GELU input (the
    bounded pass; the exact pass runs without the factor)"""
    c = tc.dcase(case, gc.TILES[ti][0], dtype)
    rows, K, nb = c.n * c.H * c.W, 9 * c.cout, 3
    for exact, pname in PASSES:
        probs = [problem(c, dtype, exact, seed=j) for j in range(nb)]
        DY = tc.Packed([p[0] for p in probs], dtype, DEV, ld=c.cout + 8)
        wd = torch.stack([p[1] for p in probs]).to(DEV)
        outs = [gc.Guarded(rows, c.cin, F32) for _ in range(nb)]
        obuf = torch.stack([o.buf for o in outs]).to(DEV)
        per, ld, off = outs[0].buf.numel(), outs[0].ld, outs[0].GR * outs[0].ld + outs[0].GC
        kw, pres, s_pre = {}, [None] * nb, 0
        if not exact:
            g = tc.gen(rows, c.cin, ti, 5)
            pres = [(torch.randn(rows, c.cin, generator=g) * 1.5).to(dtype) for _ in range(nb)]
            gp = [gc.Guarded(rows, c.cin, dtype, init=p) for p in pres]
            pbuf = torch.stack([q.buf for q in gp]).to(DEV)
            s_pre = gp[0].buf.numel()
            kw = dict(pre=pbuf.data_ptr() + off * pbuf.element_size(), ldp=ld)
        launch(tmae, c, ti, dtype, DY, wd, out=obuf.data_ptr() + 4 * off, ldo=ld, out_f32=True,
               batch=(nb, DY.stride, wd[0].numel(), per, s_pre), **kw)
        for j, o in enumerate(outs):
            o.buf = obuf[j]
            _, _, ref, S = probs[j]
            rb = tc.bounded(ref, S, K, True) if exact else gc.dgrad_reference(ref, S, K, pres[j])
            gc.check_out(f"ratio:conv_dgrad:{tag_of(case, ti, dtype, pname)}:batched{j}", o, *rb)
