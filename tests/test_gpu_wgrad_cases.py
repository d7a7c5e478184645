"""tmae_wgrad (csrc/gemm_tn.h: the split-K TN GEMM behind every weight and bias gradient) element by element, at the
shapes where its tiles, splits, sources and scatter layouts take another path (case tables and the two passes:
tests/tn_check.py).  Every case asserts through train_ops.wgrad_plan, against the rule restated in
tn_check.expected_plan, which kernel ran; the last test asserts that the module reached all ten instantiations:
bf16 {128 x 128, 256 x 256} x {bias, no bias} x {dense, conv source} and f32 {dense, conv source}.

The launch helper (tn_check.launch_wgrad) fills tmae_wgrad_args itself: the workspace is exactly
tmae_wgrad_workspace_nb floats between NaN guards, outputs and biases sit in NaN-filled guarded buffers, the conv
layout's channels outside the parameter's slice must stay NaN, and operand padding (columns past M / N, the rows a
remap skips) is NaN.
"""
import functools

import pytest
import torch

import gemm_check as gc
import tn_check as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F32], ids=tc.dname)
BIAS = pytest.mark.parametrize("bias", ["nobias", "bias", "biasacc"])
SEEN = set()  # (dtype name, tile, bias instantiation or None for f32, source) of the launches this module made
PASSES = ((True, "exact"), (False, "bounded"))


def assert_plan(M, N, K, dtype, bias, source, slot_div=1, nb=1):
    """the library names the kernel the restated rule expects; recorded for the coverage test"""
    from textmae_amd import train_ops

    want = tc.expected_plan(M, N, K, dtype, slot_div, nb)
    got = train_ops.wgrad_plan(M, N, K, dtype, slot_div, nb)
    assert got == tc.plan_str(want), (got, tc.plan_str(want))
    SEEN.add((want.dtype, want.bn, bool(bias) if dtype == BF16 else None, source))
    return want


@functools.lru_cache(maxsize=None)
def dense_problem(M, N, K, dtype, exact):
    """operands and float64 terms, computed once per shape and shared (never modified)"""
    a, b = tc.wgrad_operands(M, N, K, dtype, exact)
    return (a, b) + tc.dense_terms(a, b)


def run_dense(case, dtype, bias="nobias", layout="dense", accumulate=False):
    c = tc.W_CASES[case]
    M, N, K = c.M, c.N, c.K
    want = assert_plan(M, N, K, dtype, bias != "nobias", "dense")
    if dtype == BF16:
        assert (want.bn, want.splits, want.kchunk) == c.bf16_plan
    for exact, pname in PASSES:
        a, b, ref, S, bref, Sb = dense_problem(M, N, K, dtype, exact)
        g = tc.gen(M, N, K, exact, 99)
        A = tc.Packed([a], dtype, DEV, ld=M + c.lda_pad, remap=c.remap)
        B = tc.Packed([b], dtype, DEV, ld=N + c.ldb_pad, remap=c.remap)
        if layout == "dense":
            acc0 = tc.draw_acc((M, N), exact, g) if accumulate else None
            out = gc.Guarded(M, N, F32, DEV, init=acc0)
            lay = (0, out.ld, 1, 0, N)
        else:  # out [N][M]
            acc0 = tc.draw_acc((N, M), exact, g) if accumulate else None
            out = gc.Guarded(N, M, F32, DEV, init=acc0)
            lay, ref, S = (0, 1, out.ld, 0, N), ref.t(), S.t()
        bacc0 = tc.draw_acc((M,), exact, g) if bias == "biasacc" else None
        fb = tc.Flat(M, DEV, init=bacc0) if bias != "nobias" else None
        tc.launch_wgrad(M, N, K, dtype, A, B, out.view().data_ptr(), lay, remap=c.remap, accumulate=accumulate,
                        bias_ptr=fb.ptr() if fb else None, bias_accumulate=bias == "biasacc")
        tag = f"{case}:{tc.dname(dtype)}:{pname}:{layout}{':acc' if accumulate else ''}:{bias}"
        gc.check_out(f"ratio:wgrad:{tag}:w", out, *tc.bounded(ref, S, K, exact, acc0))
        if fb:
            tc.check_flat(f"ratio:wgrad:{tag}:b", fb, *tc.bounded(bref, Sb, K, exact, bacc0))


@DTYPES
@BIAS
@pytest.mark.parametrize("case", list(tc.W_CASES))
def test_wgrad_dense(tmae, case, dtype, bias):
    run_dense(case, dtype, bias)


@DTYPES
@BIAS
@pytest.mark.parametrize("case", ["W2", "W7a", "W7b", "W7c"])
def test_wgrad_dense_transposed(tmae, case, dtype, bias):
    """out [N][M]: the strided scatter of tn_reduce_kernel (ConvTranspose2d 1x1 weights)"""
    run_dense(case, dtype, bias, layout="dense_t")


@DTYPES
@BIAS
@pytest.mark.parametrize("layout", ["dense", "dense_t"])
def test_wgrad_dense_accumulate(tmae, dtype, bias, layout):
    """W2 onto a random f32 buffer (integers in the exact pass)"""
    run_dense("W2", dtype, bias, layout=layout, accumulate=True)


# ------------------------------------------------------------------------------------ conv weight gradients
def run_conv(name, c, dtype, bias=True, nb=1, shared=False, slot_div=1):
    M, N, K = tc.conv_mnk(c)
    cin, ct = c.c1 + c.c2, c.cin_total
    assert_plan(M, N, K, dtype, bias, "conv", slot_div, nb)
    for exact, pname in PASSES:
        probs = [tc.conv_operands(c, dtype, exact, seed=j) for j in range(nb)]
        if shared:  # every problem reads the first problem's first input (stride 0)
            probs = [(torch.cat([probs[0][0][:, :c.c1], x[:, c.c1:]], 1), dy) for x, dy in probs]
        A = tc.Packed([tc.nhwc(dy) for _, dy in probs], dtype, DEV)
        B = tc.Packed([tc.nhwc(x[:, :c.c1]) for x, _ in (probs[:1] if shared else probs)], dtype, DEV)
        B2 = tc.Packed([tc.nhwc(x[:, c.c1:]) for x, _ in probs], dtype, DEV) if c.c2 else None
        out = tc.Flat(nb * c.cout * ct * 9, DEV)
        fb = tc.Flat(nb * c.cout, DEV) if bias else None
        tc.launch_wgrad(M, N, K, dtype, A, B, out.ptr(), (c.ci_off * 9, ct * 9, 9, 1, cin), B2=B2,
                        conv=dict(c1=c.c1, H=c.H, W=c.W, stride=c.stride, cin=cin), bias_ptr=fb.ptr() if fb else None,
                        slot_div=slot_div, nb=nb, s_b=0 if shared else None, s_out=c.cout * ct * 9, s_bias=c.cout)
        terms = [tc.conv_wgrad_terms(c, x, dy) for x, dy in probs]
        ref = torch.zeros(nb, c.cout, ct, 3, 3, dtype=torch.float64)
        bound = torch.zeros_like(ref)
        mask = torch.zeros(ref.shape, dtype=torch.bool)
        sl = slice(c.ci_off, c.ci_off + cin)
        mask[:, :, sl] = True
        for j, t in enumerate(terms):
            ref[j, :, sl], bound[j, :, sl] = tc.bounded(t[0], t[1], K, exact)
        tag = f"{name}:{tc.dname(dtype)}:{pname}:{'bias' if bias else 'nobias'}"
        tc.check_flat(f"ratio:wgrad_conv:{tag}:w", out, ref, bound, mask=mask)
        if fb:
            bt = [tc.bounded(t[2], t[3], K, exact) for t in terms]
            tc.check_flat(f"ratio:wgrad_conv:{tag}:b", fb, torch.stack([r for r, _ in bt]),
                          torch.stack([b for _, b in bt]))


@DTYPES
@pytest.mark.parametrize("case", list(tc.C_CASES))
def test_wgrad_conv(tmae, case, dtype):
    run_conv(case, tc.C_CASES[case], dtype)


@DTYPES
@pytest.mark.parametrize("case", ["C2", "C6a"])
def test_wgrad_conv_no_bias(tmae, case, dtype):
    """the conv source without the bias MFMAs, on both bf16 tiles"""
    run_conv(case, tc.C_CASES[case], dtype, bias=False)


@DTYPES
@pytest.mark.parametrize("slot_div", [1, 4])
@pytest.mark.parametrize("shared", [False, True], ids=["own", "shared"])
def test_wgrad_conv_batched(tmae, dtype, shared, slot_div):
    """C7: four problems of C2's shape in one launch (f32: one launch per problem), each against its own reference:
    per-problem inputs, or a shared first input of 32 channels at stride 0 plus a per-problem second of 16"""
    c = tc.C_CASES["C2"]
    if shared:
        c = c._replace(c1=32, c2=16)
    run_conv(f"C7:{'shared' if shared else 'own'}:sd{slot_div}", c, dtype, nb=4, shared=shared, slot_div=slot_div)


# ------------------------------------------------------------------------------------ coverage (keep last)
def test_every_instantiation_was_exercised(tmae):
    can = {("bf16", t, b, s) for t in (128, 256) for b in (False, True) for s in ("dense", "conv")}
    can |= {("f32", 64, None, s) for s in ("dense", "conv")}
    assert len(can) == 10
    assert SEEN == can, (sorted(can - SEEN, key=str), sorted(SEEN - can, key=str))
