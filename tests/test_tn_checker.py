"""The wgrad / conv-dgrad case tests' checker, plan and host validation, without a GPU (CPU only).

1. Plan: tn_check.expected_plan equals tmae_wgrad_plan at every case of tests/test_gpu_wgrad_cases.py and at the ViT-B
   batch-64 shapes; K = 0 plans (it was an integer division by zero in tn_plan) and tmae_wgrad rejects it; the
   workspace queries agree with the plan.
2. The reference fits the bound: a plain f32 CPU a.t() @ b, conv2d_weight and conv2d_input, and the same f32 sums in
   two other orders (reversed K; per-split partial sums, then folded), stay at ratio <= 1 at every case, both dtypes.
   The index maps tn_check restates (im2col, dgrad_cols) reproduce torch's gradients exactly on integers.
3. Faults are rejected by both passes: a dropped / doubled K row, a zeroed 16-byte chunk, a split missing from the
   bias fold, exchanged taps, a wrapped padding pixel, a parity tap let through, an unwritten element, writes into
   a guard, outside the channel slice and past the workspace.  A single dropped K row moves most elements past the
   bounded pass's bound up to K ~ 1000 and none at K = 9280, so the bounded pass is asked to reject it only at the
   cases with K <= 1160; at W3 (K = 5632) its mutation is a whole dropped split and single terms are the exact
   pass's job.
4. Host validation of tmae_wgrad / tmae_conv_dgrad: every rejection happens before any device work.
"""
import ctypes
import functools

import pytest
import torch

import gemm_check as gc
import tn_check as tc

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F32], ids=tc.dname)
PASSES = pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
VITB = {"qkv": (2304, 768, 9216), "fc1": (3072, 768, 9216), "fc2": (768, 3072, 9216), "proj": (768, 768, 9216)}


# ------------------------------------------------------------------------------------ plan
def _wgrad_shapes():
    shapes = {k: (c.M, c.N, c.K) for k, c in tc.W_CASES.items()}
    shapes.update({k: tc.conv_mnk(c) for k, c in tc.C_CASES.items()})
    return shapes


def test_case_table_plans():
    """the bf16 plans written down in the case table follow from the restated rule; so does the f32 example"""
    for k, c in tc.W_CASES.items():
        p = tc.expected_plan(c.M, c.N, c.K, BF16)
        assert (p.bn, p.splits, p.kchunk) == c.bf16_plan and p.nw == (8 if p.bn == 256 else 4), (k, p)
    assert tc.plan_str(tc.expected_plan(136, 264, 456, F32)) == "tn<f32,64x64,4w,s3,kc160>"
    assert tc.plan_str(tc.expected_plan(760, 1032, 584, BF16)) == "tn<bf16,256x256,8w,s2,kc320>"
    for k, want in (("C1", (128, 2, 320)), ("C6a", (256, 1, 64)), ("C6b", (256, 2, 320))):
        p = tc.expected_plan(*tc.conv_mnk(tc.C_CASES[k]), BF16)
        assert (p.bn, p.splits, p.kchunk) == want, (k, p)


@DTYPES
def test_expected_plan_is_the_library_plan(tmae, dtype):
    from textmae_amd import train_ops

    for k, (M, N, K) in {**_wgrad_shapes(), **VITB}.items():
        for slot_div, nb in ((1, 1), (4, 1), (1, 4), (4, 4)):
            want = tc.plan_str(tc.expected_plan(M, N, K, dtype, slot_div, nb))
            assert train_ops.wgrad_plan(M, N, K, dtype, slot_div, nb) == want, (k, slot_div, nb)


def test_vitb_plans_fill_one_round(tmae):
    """the encoder's weight gradients at batch 64 take the 8-wave tile and at most one round of its 256 slots"""
    for k, (M, N, K) in VITB.items():
        p = tc.expected_plan(M, N, K, BF16)
        tiles = tc.cdiv(N, 256) * tc.cdiv(M, 256)
        assert p.bn == 256 and p.splits > 1 and tiles * p.splits <= 256, (k, p)


@DTYPES
def test_workspace_agrees_with_plan(tmae, dtype):
    from textmae_amd import _lib
    from textmae_amd.ops import dtype_code

    code = dtype_code(dtype)
    for k, (M, N, K) in {**_wgrad_shapes(), **VITB}.items():
        p = tc.expected_plan(M, N, K, dtype)
        assert _lib.value("tmae_wgrad_workspace", M, N, K, code) == p.splits * (M * N + M), k
        for slot_div, nb in ((1, 1), (4, 1), (1, 4), (4, 4)):
            got = _lib.value("tmae_wgrad_workspace_nb", M, N, K, code, slot_div, nb)
            assert got == tc.workspace_elems(M, N, K, dtype, slot_div, nb), (k, slot_div, nb)
            if dtype == BF16:  # the plan string's split count is the launch's: nb problems' slabs and bias slabs
                s = int(_lib_plan_splits(M, N, K, dtype, slot_div, nb))
                assert got >= nb * s * (M * N + M)


def _lib_plan_splits(M, N, K, dtype, slot_div, nb):
    from textmae_amd import train_ops

    return train_ops.wgrad_plan(M, N, K, dtype, slot_div, nb).split(",s")[1].split(",")[0]


@DTYPES
@pytest.mark.parametrize("K", [0, -3])
def test_empty_reduction_plans_as_one_row(tmae, dtype, K):
    """tn_plan divided by kchunk = 0 here (SIGFPE in tmae_wgrad_workspace and in tmae_wgrad before any launch)"""
    from textmae_amd import _lib, train_ops
    from textmae_amd.ops import dtype_code

    code = dtype_code(dtype)
    one = train_ops.wgrad_plan(72, 64, 1, dtype)
    assert train_ops.wgrad_plan(72, 64, K, dtype) == one == tc.plan_str(tc.expected_plan(72, 64, K, dtype))
    assert ",s1,kc%d>" % (64 if dtype == BF16 else 32) in one
    assert _lib.value("tmae_wgrad_workspace", 72, 64, K, code) == 72 * 64 + 72
    assert _lib.value("tmae_wgrad_workspace_nb", 72, 64, K, code, 4, 3) == 3 * (72 * 64 + 72)
    # an empty output plans too (tiles = 0 was the second division by zero)
    assert _lib.value("tmae_wgrad_workspace", 0, 64, 300, code) == 0
    assert train_ops.wgrad_plan(0, 0, 300, dtype) == tc.plan_str(tc.expected_plan(0, 0, 300, dtype))
    a = _wargs(72, 64, K)
    with pytest.raises(ValueError, match="K=%d" % K):
        _lib.call("tmae_wgrad", ctypes.byref(a), code, None)


# ------------------------------------------------------------------------------------ the reference fits the bound
def _orders(a, b, kchunk):
    """f32 A^T B three ways: the BLAS order, reversed K, per-split partial sums folded in split order"""
    af, bf = a.float(), b.float()
    yield "blas", af.t() @ bf
    yield "reversed", af.flip(0).t() @ bf.flip(0)
    acc = None
    for k0 in range(0, a.shape[0], kchunk):
        part = af[k0:k0 + kchunk].t() @ bf[k0:k0 + kchunk]
        acc = part if acc is None else acc + part
    yield "splits", acc


def _written(M, N, values):
    g = gc.Guarded(M, N, F32)
    g.view()[:, :N] = values.to(F32)
    return g


@DTYPES
@pytest.mark.parametrize("case", ["W1", "W2", "W3", "W4", "W5", "W6", "W7a"])
def test_cpu_wgrad_within_bound(case, dtype):
    c = tc.W_CASES[case]
    a, b = tc.wgrad_operands(c.M, c.N, c.K, dtype, False)
    ref, S, bias, Sb = tc.dense_terms(a, b)
    ref, bound = tc.bounded(ref, S, c.K, False)
    kc = tc.expected_plan(c.M, c.N, c.K, dtype).kchunk
    for name, y in _orders(a, b, kc):
        assert gc.check_out(f"cpu:{case}:{name}", _written(c.M, c.N, y), ref, bound, log=False) <= 1.0
    bref, bbound = tc.bounded(bias, Sb, c.K, False)
    for y in (a.float().sum(0), a.float().flip(0).sum(0)):
        assert tc.check_flat("cpu:bias", tc.Flat(c.M, init=y), bref, bbound, log=False) <= 1.0
    # the exact pass's premise: f32 sums of the integer operands equal the integer reference
    a, b = tc.wgrad_operands(c.M, c.N, c.K, dtype, True)
    ref, S, bias, _ = tc.dense_terms(a, b)
    for name, y in _orders(a, b, kc):
        assert torch.equal(y.to(torch.int64), tc.to_int64(ref)), name
    assert torch.equal(a.float().sum(0).to(torch.int64), tc.to_int64(bias))


@DTYPES
@pytest.mark.parametrize("case", list(tc.C_CASES))
def test_cpu_conv_wgrad_within_bound(case, dtype):
    c = tc.C_CASES[case]
    M, N, K = tc.conv_mnk(c)
    cin = c.c1 + c.c2
    x, dy = tc.conv_operands(c, dtype, False)
    ref, S, _, _ = tc.conv_wgrad_terms(c, x, dy)
    ref, bound = tc.bounded(ref, S, K, False)
    y = torch.nn.grad.conv2d_weight(x.float(), ref.shape, dy.float(), stride=c.stride, padding=1)
    assert gc.ratio(y, ref, bound) <= 1.0
    a, b = tc.nhwc(dy), tc.im2col(tc.nhwc(x), c.n, c.H, c.W, c.stride)
    for name, y in _orders(a, b, tc.expected_plan(M, N, K, dtype).kchunk):
        assert gc.ratio(tc.columns_to_conv(y, cin), ref, bound) <= 1.0, name
    # the restated im2col is conv2d_weight's: equal on integers
    x, dy = tc.conv_operands(c, dtype, True)
    ref = tc.conv_wgrad_terms(c, x, dy)[0]
    mine = tc.dense_terms(tc.nhwc(dy), tc.im2col(tc.nhwc(x), c.n, c.H, c.W, c.stride))[0]
    assert torch.equal(tc.columns_to_conv(mine, cin), ref) and float(ref.abs().max()) < 2 ** 24


@pytest.mark.parametrize("dtype,ti", [(d, t) for d in (BF16, F32) for t in tc.D_TILES[d]],
                         ids=lambda v: tc.dname(v) if isinstance(v, torch.dtype) else "%dx%d" % gc.TILES[v])
@pytest.mark.parametrize("case", list(tc.D_CASES))
def test_cpu_conv_dgrad_within_bound(case, dtype, ti):
    c = tc.dcase(case, gc.TILES[ti][0], dtype)
    K = 9 * c.cout
    dy, w = tc.dgrad_operands(c, dtype, False)
    ref, S = tc.conv_dgrad_terms(c, dy, w)
    ref, bound = tc.bounded(ref, S, K, False)
    y = torch.nn.grad.conv2d_input((c.n, c.cin, c.H, c.W), w.float(), dy.float(), stride=c.stride, padding=1)
    assert gc.ratio(tc.nhwc(y), ref, bound) <= 1.0
    X, wd = tc.dgrad_cols(tc.nhwc(dy), c.n, c.H, c.W, c.stride), tc.dgrad_weights(w)
    for name, y in _orders(X.t(), wd.t(), 64 if dtype == BF16 else 32):
        assert gc.ratio(y, ref, bound) <= 1.0, name
    assert gc.ratio(y.to(BF16), *tc.bounded(ref, S, K, False, store_bf16=True)) <= 1.0
    dy, w = tc.dgrad_operands(c, dtype, True)
    ref = tc.conv_dgrad_terms(c, dy, w)[0]
    X, wd = tc.dgrad_cols(tc.nhwc(dy), c.n, c.H, c.W, c.stride), tc.dgrad_weights(w)
    assert torch.equal(X.double() @ wd.double().t(), ref) and float(ref.abs().max()) < 2 ** 24


# ------------------------------------------------------------------------------------ faults are rejected
class Problem:
    """a case in its dense form out[m][n] = sum_k A[k][m] B[k][n], with the container the GPU test checks it in:
    a Guarded block (dense weight gradients, conv data gradients) or the conv-layout Flat with eight channels in
    front of the parameter's slice (conv weight gradients)"""

    def __init__(self, case, exact, faults=()):
        self.case, self.exact = case, exact
        self.conv = None
        if case in tc.W_CASES:
            c = tc.W_CASES[case]
            self.A, self.B = tc.wgrad_operands(c.M, c.N, c.K, BF16, exact)
            p = tc.expected_plan(c.M, c.N, c.K, F32)
            self.kc = p.kchunk if p.kchunk < c.K else c.K // 2
        elif case in tc.C_CASES:
            self.conv = c = tc.C_CASES[case]
            x, dy = tc.conv_operands(c, BF16, exact)
            self.A = tc.nhwc(dy)
            self.B = tc.im2col(tc.nhwc(x), c.n, c.H, c.W, c.stride, wrap="wrap" in faults)
            p = tc.expected_plan(*tc.conv_mnk(c), F32)
            self.kc = p.kchunk if p.kchunk < self.A.shape[0] else self.A.shape[0] // 2
            self.taps = c.c1 + c.c2  # columns per tap on the N axis
        else:
            c = tc.dcase(case, 32, BF16)
            dy, w = tc.dgrad_operands(c, BF16, exact)
            self.A = tc.dgrad_cols(tc.nhwc(dy), c.n, c.H, c.W, c.stride, parity="parity" not in faults).t()
            self.B = tc.dgrad_weights(w).t()
            self.kc = 64
            self.taps = c.cout  # rows per tap on the K axis
        if "taps" in faults:  # taps 0 and 8 exchanged in the source's index map
            t = self.taps
            if case in tc.C_CASES:
                self.B = torch.cat([self.B[:, 8 * t:], self.B[:, t:8 * t], self.B[:, :t]], 1)
            else:
                self.A = torch.cat([self.A[8 * t:], self.A[t:8 * t], self.A[:t]], 0)
        self.K, self.M = self.A.shape
        self.N = self.B.shape[1]
        self.out, _, self.bias, _ = tc.dense_terms(self.A, self.B)

    def reference(self):
        ref, S, bias, Sb = tc.dense_terms(self.A, self.B)
        if self.exact:
            tc.to_int64(ref), tc.to_int64(bias)
        return tc.bounded(ref, S, self.K, self.exact), tc.bounded(bias, Sb, self.K, self.exact)

    def verdict(self, values, ref, bound, spoil=None):
        """write `values` [M][N] where the kernel would and check them as the GPU tests do"""
        if self.conv is None:
            g = _written(self.M, self.N, values)
            if spoil:
                spoil(g)
            return gc.check_out("fault", g, ref, bound, log=False)
        c = self.conv
        cin, ct = c.c1 + c.c2, c.c1 + c.c2 + 8
        f = tc.Flat(c.cout * ct * 9)
        mask = torch.zeros(c.cout, ct, 3, 3, dtype=torch.bool)
        mask[:, 8:] = True
        f.inner().view(c.cout, ct, 3, 3)[:, 8:] = tc.columns_to_conv(values, cin).to(F32)
        def full(t):
            return torch.cat([torch.zeros(c.cout, 8, 3, 3, dtype=t.dtype), tc.columns_to_conv(t, cin)], 1)

        if spoil:
            spoil(f)
        return tc.check_flat("fault", f, full(ref), full(bound), mask=mask, log=False)


@functools.lru_cache(maxsize=None)
def clean(case, exact):
    p = Problem(case, exact)
    (ref, bound), (bref, bbound) = p.reference()
    assert p.verdict(ref, ref, bound) <= 1.0  # the reference itself passes
    return p, ref, bound, bref, bbound


FAULT_CASES = ["W2", "W6", "C1", "C4", "D2", "D3"]
CONV_W, CONV_D = ["C1", "C4"], ["D2", "D3"]


def _rejected(p, values, ref, bound, spoil=None, match=None):
    with pytest.raises(AssertionError, match=match):
        p.verdict(values, ref, bound, spoil)


@PASSES
@pytest.mark.parametrize("case", FAULT_CASES)
def test_rejects_dropped_and_doubled_k_row(case, exact):
    p, ref, bound, _, _ = clean(case, exact)
    assert p.K <= 1160
    k = p.kc  # the first row of split 2
    _rejected(p, ref - torch.outer(p.A[k].double(), p.B[k].double()), ref, bound)
    _rejected(p, ref + torch.outer(p.A[k - 1].double(), p.B[k - 1].double()), ref, bound)


@PASSES
@pytest.mark.parametrize("case", FAULT_CASES)
def test_rejects_zeroed_chunk(case, exact):
    """one 16-byte chunk (8 bf16 columns) of one K row of A read as zero: eight output rows lose one term"""
    p, ref, bound, _, _ = clean(case, exact)
    k = 4 * p.taps + 1 if case in CONV_D else p.kc + 3  # conv dgrad: a centre-tap row, live wherever parity allows
    m0 = (p.M // 2) // 8 * 8
    bad = ref.clone()
    bad[m0:m0 + 8] -= torch.outer(p.A[k, m0:m0 + 8].double(), p.B[k].double())
    assert not torch.equal(bad, ref)
    _rejected(p, bad, ref, bound)


@PASSES
@pytest.mark.parametrize("case", ["W2", "W6", "C1", "C4"])
def test_rejects_split_missing_from_bias_fold(case, exact):
    p, _, _, bref, bbound = clean(case, exact)
    assert tc.check_flat("bias", tc.Flat(p.M, init=bref), bref, bbound, log=False) <= 1.0
    short = bref - p.A[p.kc:2 * p.kc].double().sum(0)
    with pytest.raises(AssertionError):
        tc.check_flat("bias", tc.Flat(p.M, init=short), bref, bbound, log=False)


@PASSES
@pytest.mark.parametrize("case", CONV_W + CONV_D)
def test_rejects_exchanged_taps(case, exact):
    p, ref, bound, _, _ = clean(case, exact)
    _rejected(p, Problem(case, exact, ("taps",)).out, ref, bound)


@PASSES
@pytest.mark.parametrize("case", CONV_W)
def test_rejects_wrapped_padding_pixel(case, exact):
    p, ref, bound, _, _ = clean(case, exact)
    _rejected(p, Problem(case, exact, ("wrap",)).out, ref, bound)


@PASSES
@pytest.mark.parametrize("case", CONV_D)
def test_rejects_parity_tap_let_through(case, exact):
    p, ref, bound, _, _ = clean(case, exact)
    _rejected(p, Problem(case, exact, ("parity",)).out, ref, bound)


@PASSES
@pytest.mark.parametrize("case", FAULT_CASES)
def test_rejects_unwritten_element_and_guard_write(case, exact):
    p, ref, bound, _, _ = clean(case, exact)
    hole = ref.clone()
    hole[p.M - 1, p.N - 1] = float("nan")  # what the pre-fill leaves when the kernel skips the element
    _rejected(p, hole, ref, bound)

    def after(c):  # one element past the block (Guarded) / the parameter (Flat)
        if isinstance(c, gc.Guarded):
            c.view()[p.M - 1, p.N] = 1.0
        else:
            c.buf[c.G + c.n] = 1.0
    _rejected(p, ref, ref, bound, spoil=after, match="guard")

    def before(c):  # the element just in front
        if isinstance(c, gc.Guarded):
            c.buf[c.GR, c.GC - 1] = 0.0
        else:
            c.buf[c.G - 1] = 0.0
    _rejected(p, ref, ref, bound, spoil=before, match="guard")


@PASSES
@pytest.mark.parametrize("case", CONV_W)
def test_rejects_write_outside_channel_slice(case, exact):
    p, ref, bound, _, _ = clean(case, exact)

    def stray(f):  # channel 7 of the wider parameter: ci_off = 8 shifted by one channel
        f.inner().view(p.conv.cout, -1, 3, 3)[0, 7, 1, 1] = 0.0
    _rejected(p, ref, ref, bound, spoil=stray, match="slice")


def test_rejects_write_past_workspace():
    ws = tc.Flat(tc.workspace_elems(136, 264, 456, F32))
    ws.inner().fill_(0.0)
    tc.check_workspace("ws", ws)
    ws.buf[ws.G + ws.n] = 0.0  # slab `splits` of a launch that ran one split too many
    with pytest.raises(AssertionError, match="workspace"):
        tc.check_workspace("ws", ws)


def test_w3_single_terms_are_the_exact_pass_job():
    """K = 5632, 22 splits: the exact pass rejects one dropped row of 5632; the bounded pass is asked only to reject
    a whole dropped split (row kchunk onwards for kchunk rows)"""
    c = tc.W_CASES["W3"]
    kc = c.bf16_plan[2]
    for exact in (True, False):
        a, b = tc.wgrad_operands(c.M, c.N, c.K, BF16, exact)
        ref, S, _, _ = tc.dense_terms(a, b)
        ref, bound = tc.bounded(ref, S, c.K, exact)
        assert gc.check_out("w3", _written(c.M, c.N, ref), ref, bound, log=False) <= 1.0
        bad = ref - (torch.outer(a[kc].double(), b[kc].double()) if exact
                     else a[kc:2 * kc].double().t() @ b[kc:2 * kc].double())
        with pytest.raises(AssertionError):
            gc.check_out("w3", _written(c.M, c.N, bad), ref, bound, log=False)


# ------------------------------------------------------------------------------------ host validation
PTR = 1 << 20  # never dereferenced: every case below is rejected before any device work


def _wargs(M, N, K, conv=False, **kw):
    from textmae_amd import _lib

    a = _lib.WgradArgs()
    a.a, a.b, a.work, a.out = PTR, PTR, PTR, PTR
    a.lda, a.ldb, a.a_G, a.b_G = M, N, 1 << 30, 1 << 30
    a.M, a.N, a.K = M, N, K
    a.work_elems = 1 << 40
    a.o_sm, a.o_sc, a.o_cp = N, 1, N
    if conv:
        a.b_conv, a.b_Cin, a.b_c1, a.ldb, a.b_H, a.b_W, a.b_stride = 1, N // 9, N // 9, N // 9, 4, 4, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@DTYPES
def test_wgrad_host_validation(tmae, dtype):
    from textmae_amd import _lib
    from textmae_amd.ops import dtype_code

    code, e = dtype_code(dtype), tc.epc(dtype)

    def rejected(a, match):
        with pytest.raises(ValueError, match=match):
            _lib.call("tmae_wgrad", ctypes.byref(a), code, None)

    rejected(_wargs(64 + e // 2, 64, 256), "multiples of")
    rejected(_wargs(64, 64 + e // 2, 256), "multiples of")
    rejected(_wargs(64, 9 * 16, 32, conv=True, b_Cin=24, b_c1=24), r"9 \* Cin")
    rejected(_wargs(64, 9 * 16, 32, conv=True, b_stride=3), "stride 3")
    need = _lib.value("tmae_wgrad_workspace_nb", 72, 64, 5632, code, 1, 1)
    assert need == tc.workspace_elems(72, 64, 5632, dtype)
    rejected(_wargs(72, 64, 5632, work_elems=need - 1), "workspace too small")
    # 70000 rows of 65536 elements: the last source row starts past 2^32 elements
    rejected(_wargs(8, 8, 70000, lda=65536), "operand A spans 2")
    rejected(_wargs(8, 8, 70000, ldb=65536), "operand B spans 2")
    rejected(_wargs(8, 8, 40000, lda=8, a_G=4, a_Gs=1 << 29, a_off=1), "operand A spans 2")


@DTYPES
def test_conv_dgrad_host_validation(tmae, dtype):
    from textmae_amd import _lib
    from textmae_amd.ops import dtype_code

    code = dtype_code(dtype)

    def args(**kw):
        a = _lib.ConvDgradArgs()
        a.dy, a.wd, a.out, a.out_f32 = PTR, PTR, PTR, 1
        a.ldy, a.n, a.H, a.W, a.stride, a.cout, a.cin, a.ldo = 24, 2, 5, 7, 2, 24, 24, 24
        for k, v in kw.items():
            if isinstance(v, tuple):
                for i, x in enumerate(v):
                    getattr(a, k)[i] = x
            else:
                setattr(a, k, v)
        return a

    def rejected(a, match):
        with pytest.raises(ValueError, match=match):
            _lib.call("tmae_conv_dgrad", ctypes.byref(a), code, None)

    rejected(args(stride=3), "stride 3")
    rejected(args(cout=20 if dtype == BF16 else 22), "channels")
    rejected(args(cin=22), "channels")
    routes = dict(out=None, acc=(PTR, PTR, PTR), ld_acc=(8, 8, 8))
    rejected(args(lim=(4, 16, 24), **routes), "route limits")
    rejected(args(lim=(8, 12, 24), **routes), "route limits")
    rejected(args(lim=(8, 16, 20), **routes), "route limits")
    rejected(args(lim=(8, 16, 24), out=None, acc=(PTR, 0, PTR), ld_acc=(8, 8, 8)), "route destination")
    rejected(args(lim=(8, 16, 24), nb=3, **routes), "take no routes")
    if dtype == F32:
        rejected(args(out_f32=0), "f32 path writes f32")
