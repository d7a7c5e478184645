"""The training path's glue kernels on the MI355X, one kernel per test, every output element bounded on its own
(tests/glue_check.py: float64 references, bounds derived from the kernels' formulas, NaN-filled guarded outputs).

The entropy models' backward kernels, the rate term, the elementwise / gather / reduction kernels of csrc/train.hip and
the training-only outputs of the forward (lse, pre-activations, the out-of-place residual) are reached by the whole-model
gradient tests only in f32, on golden inputs, through a max-error / max-magnitude metric; here each runs alone, in f32
and bf16, at the shapes, layouts and branches named beside the cases.  Every bounded comparison lands in the parity log
with its ratio (error / bound, <= 1 passes).

Largest error / bound per kernel on an MI355X (198 cases, 3.7 s), by the output's dtype; "-" where the kernel has no
such output, 0 where the comparison is bitwise:

    kernel                  f32     bf16        kernel                  f32     bf16
    gc_bwd                  0.492   0.960       ln_bwd                  0.277   0.980
    eb_bwd                  0.768   -           dec_gather              0.120   0.993
    eb_aux_bwd              0.029   -           mha_lse                 0.019   -
    bpp_sum                 0.189   -           patch_gather            0       0
    bpp_bwd                 0.391   -           patchify                -       0
    lrp_bwd                 0.999   0.973       copy2d                  0       0
    unshuffle_bwd           0.476   0.982       add                     0       -
    gelu_bwd                0.537   0.990       linear_pre              0       0
    colsum                  0.035   -           linear_residual_out     0       -
                                                conv3x3_pre             0       0

A bf16 store is rounded to nearest, so its ratio approaches 1 on any large enough output; that is the bound being
exact, not thin.  The f32 ratios above 0.5, with their elements:
  * lrp_bwd gsum 0.999 (g32 + g16, element 592: out -2.0029344559, ref -2.0029345751, bound 1.19e-7), 0.992
    (g32 + g32b, element 752) and eb_bwd dz 0.768 (two_pass, element 1252: out 1.1834946871, ref 1.1834947464, bound
    7.7e-8), 0.594 (one_pass, element 70), 0.508 (sub_wave, element 9): each is ONE correctly rounded f32 addition
    (g32 + g16; gzhat + a likelihood term below f32's resolution), whose bound is half an ulp, and half an ulp is
    reached.  Neither the derivation nor the kernel has room to give there.
  * lrp_bwd dt 0.645 (all three addends, element 380: out 1.45775e-3, ref 1.45776e-3, bound 1.74e-8) and 0.583 (g32,
    element 408): t near +-3, where 1 - tanh(t)^2 cancels to 1e-2 and tanhf's 4 ulp dominate the bound.
  * gelu_bwd 0.537 (element 31: out -0.4920061231, ref -0.4920059150, bound 3.87e-7): the A-S 7.1.26 erf's 4.4e-7
    absolute error, which the bound takes from common.h.
No test of this file found a kernel outside its bound; tmae_gelu_bwd, which had no caller, is correct.
"""
import copy

import pytest
import torch

import gemm_check
import glue_check as gk
from glue_check import BF16, F32, Guarded
from oracle import mcm_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [F32, BF16]
TRIPLES = [(F32, F32), (F32, BF16), (BF16, BF16)]  # (dy dtype, operand dtype): what the entries dispatch


@pytest.fixture(scope="module")
def T():
    import textmae_amd  # noqa: F401
    from textmae_amd import train_ops

    return train_ops


def dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).contiguous().to(DEV)


def G(M, N, dtype=F32, init=None):
    return Guarded(M, N, dtype, device=DEV, init=init)


def G1(n, dtype=F32, init=None):
    """a dense 1-D / NCHW output: one guarded row"""
    return Guarded(1, n, dtype, device=DEV, init=None if init is None else init.reshape(1, -1))


def sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ tmae_gc_bwd
# everything given, at both shapes, forms and dtypes; glik=None and gyp=None once per form (f32, the larger shape)
GC_CASES = [(s, tr, dt, "full") for s in gk.GC_SHAPES for tr in (True, False) for dt in DTYPES]
GC_CASES += [("three_wg", tr, F32, v) for tr in (True, False) for v in ("no_glik", "no_gyp")]


@pytest.mark.parametrize("shape,training,dtype,variant", GC_CASES)
def test_gc_bwd(T, shape, training, dtype, variant):
    """small: 90 elements, one partial workgroup; three_wg: 528 elements, three workgroups, the last ragged.  Seeds
    gk.GC_SEEDS; skipped share (reference alone): small 0 / 90 train and eval; three_wg 9 / 528 = 1.7 % train,
    4 / 528 = 0.8 % eval.  ldy = Mtot + 8, ld_ms = sw + 3, ldg = Mtot + 3, lddy = Mtot + 16, ldd = sw + 16"""
    c = gk.gc_case(shape)
    use_glik, use_gyp = variant != "no_glik", variant != "no_gyp"
    out, skip, a, f = gk.gc_bwd_reference(c, training, dtype, use_glik, use_gyp)
    assert float(skip.any.double().mean()) <= gk.SKIP_CAP
    if shape == "three_wg" and variant == "full":
        for k, v in gk.gc_census(c, a).items():
            assert v >= 4, (k, v)
    dy, dmu, dsig = G(c.M, c.Mtot, init=c.dy0), G(c.M, c.sw, dtype), G(c.M, c.sw, dtype)
    assert len({c.ldy, c.ld_ms, c.ldg, dy.ld, dmu.ld}) == 5
    T.gc_bwd(dev(gk.pad(c.y, c.ldy)), c.ldy, c.yoff, dev(gk.pad(c.mu, c.ld_ms)), dev(gk.pad(c.sigma, c.ld_ms)), c.ld_ms,
             dev(c.noise) if training else None, c.Mtot, dev(c.glik) if use_glik else None,
             dev(gk.pad(c.gyp, c.ldg)) if use_gyp else None, c.ldg, dy.view(), dy.ld, dmu.view(), dsig.view(), dmu.ld,
             c.n, c.HW, c.sw, dtype)
    sync()
    tag = f"gc_bwd:{shape}:{'train' if training else 'eval'}:{variant}"
    gk.check(f"{tag}:dy", dy, *out["dy"])
    gk.check(f"{tag}:dmu", dmu, *out["dmu"])
    gk.check(f"{tag}:dsigma", dsig, *out["dsigma"])
    if not training:  # only the likelihood path feeds dmu, and x~ moves with mu: exactly zero
        assert float(dmu.result().abs().max()) == 0.0


# ------------------------------------------------------------------------------------ tmae_eb_bwd
@pytest.fixture(scope="module")
def eb5(tmae):
    return gk.eb_module(tmae, 5)


def _eb_device(eb, sd):
    m = copy.deepcopy(eb)
    m.load_state_dict({k[len(gk.EB_PRE):]: v for k, v in sd.items()})
    return m.to(DEV)


def _eb_grad_struct(bufs):
    from textmae_amd import _lib

    p = _lib.EBParams()
    for i in range(5):
        p.matrix[i] = bufs[f"_matrix{i}"].view().data_ptr()
        p.bias[i] = bufs[f"_bias{i}"].view().data_ptr()
        if i < 4:
            p.factor[i] = bufs[f"_factor{i}"].view().data_ptr()
    return p


# accumulate 0 and 1 at every size and form; glik=None and gzhat=None once per form
EB_CASES = [(s, tr, v) for s in gk.EB_SIZES for tr in (True, False) for v in ("full", "accumulate")]
EB_CASES += [("one_pass", tr, v) for tr in (True, False) for v in ("no_glik", "no_gzhat")]


@pytest.mark.parametrize("size,training,variant", EB_CASES)
def test_eb_bwd(T, tmae, eb5, size, training, variant):
    """C = 5; n HW = 18 (fewer elements than a wave), 105, 273 (the stride loop's second pass ragged).  Seeds
    gk.EB_SEEDS; clamped share 28 % / 30 % / 30 %, skipped dz elements (likelihood band) 0 / 90, 0 / 525, 1 / 1365
    in training, none in eval.  One raw _matrix entry is 21 (softplus threshold)"""
    c = gk.eb_case(eb5, size)
    acc = variant == "accumulate"
    use_glik, use_gzhat = variant != "no_glik", variant != "no_gzhat"
    out, a, f = gk.eb_bwd_reference(c, training, acc, use_glik, use_gzhat)
    cen = gk.eb_census(a)
    if use_glik:
        assert 0.05 <= cen["share"] <= 0.5 and cen["blocked"] >= 4 and cen["passes"] >= 4, cen
    assert float(out["dz"][2].double().mean()) <= gk.SKIP_CAP
    m = _eb_device(eb5, c.sd)
    bufs = {k: G1(c.sd[gk.EB_PRE + k].numel(), init=c.acc0[k] if acc else None) for k in gk.EB_KEYS}
    dz = G1(c.N * c.C)
    T.eb_bwd(tmae.ops._eb_params(m), dev(c.z), dev(c.noise) if training else None, dev(c.glik) if use_glik else None,
             dev(c.gzhat) if use_gzhat else None, dz.view(), c.n, c.C, c.HW, _eb_grad_struct(bufs), accumulate=acc)
    sync()
    tag = f"eb_bwd:{size}:{'train' if training else 'eval'}:{variant}"
    ref, bound, skip = out["dz"]
    gk.check(f"{tag}:dz", dz, ref.reshape(1, -1), bound.reshape(1, -1), skip.reshape(1, -1))
    for k in gk.EB_KEYS:
        ref, bound, _ = out[k]
        gk.check(f"{tag}:{k}", bufs[k], ref.reshape(1, -1), bound.reshape(1, -1))


# ------------------------------------------------------------------------------------ tmae_eb_aux_bwd
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("gout", [None, -1.75])
@pytest.mark.parametrize("C", [5, 90])
def test_eb_aux_bwd(T, tmae, C, gout, acc):
    """C = 90: 270 work items, past one workgroup.  Every quantile at least 1e-3 from the kink f(q) == target"""
    eb = gk.eb_module(tmae, C)
    sd = {gk.EB_PRE + k: v.detach().clone().float() for k, v in eb.state_dict().items()}
    acc0 = torch.randn(C, 1, 3, generator=gk._gen(C)) if acc else None
    ref, bound, kink, _ = gk.eb_aux_reference(sd, None if gout is None else torch.tensor(gout), acc0)
    assert kink >= 1e-3
    m = eb.to(DEV)
    dq = G1(3 * C, init=acc0)
    T.eb_aux_bwd(tmae.ops._eb_params(m), m.target, None if gout is None else torch.tensor([gout], device=DEV), dq.view(),
                 C, accumulate=acc)
    sync()
    gk.check(f"eb_aux_bwd:C{C}:g{gout}:acc{int(acc)}", dq, ref, bound)


# ------------------------------------------------------------------------------------ tmae_bpp_sum, tmae_bpp_bwd
@pytest.mark.parametrize("ny,nz", [(1000, 37), (131072 + 5, 3)])
def test_bpp_sum_and_bwd(T, ny, nz):
    """(131077, 3) walks the grid stride (512 x 256 threads); both cross the i < na seam; exact 1e-9 and 1.0 on both
    sides of it"""
    from textmae_amd import _lib
    from textmae_amd.ops import _stream

    y, z = gk.bpp_case(ny, nz)
    npx = 3.0 * 64 * 64
    yd, zd = dev(y), dev(z)
    work = torch.empty(512, dtype=torch.float64, device=DEV)
    out = G1(1)
    _lib.call("tmae_bpp_sum", yd.data_ptr(), ny, zd.data_ptr(), nz, work.data_ptr(), out.view().data_ptr(), npx,
              _stream())
    sync()
    gk.check(f"bpp_sum:{ny}", out, *gk.bpp_sum_reference(y, z, npx))
    lik = torch.cat([y, z])
    ref, bound, _ = gk.bpp_bwd_reference(lik, 0.7, npx)
    dlik = G1(ny + nz)
    T.bpp_bwd(dev(lik), torch.tensor([0.7], device=DEV), dlik.view(), npx)
    sync()
    gk.check(f"bpp_bwd:{ny}", dlik, ref, bound)


# ------------------------------------------------------------------------------------ tmae_lrp_bwd
LRP_SUBSETS = [("g32",), ("g32b",), ("g16",), ("g32", "g32b"), ("g32", "g16"), ("g32b", "g16"), ("g32", "g32b", "g16")]


@pytest.mark.parametrize("with_gsum", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use", LRP_SUBSETS)
def test_lrp_bwd(T, use, dtype, with_gsum):
    """rows 37 x C 20 = 740 elements (ragged last workgroup); t up to +-12; every ld wider than C and distinct"""
    c = gk.lrp_case()
    out = gk.lrp_reference(c, dtype, use)
    ld = {"g32": c.C + 1, "g32b": c.C + 2, "g16": c.C + 3, "t": c.C + 5}
    dt, gs = G(c.rows, c.C, dtype), G(c.rows, c.C + 4)  # lddt = C + 16, ldgs = C + 20
    args = {k: dev(gk.pad(getattr(c, k), ld[k]), dtype if k == "g16" else None) if k in use else None for k in ld if k != "t"}
    T.lrp_bwd(dev(gk.pad(c.t, ld["t"])), ld["t"], dt.view(), dt.ld, c.rows, c.C, dtype, g32=args["g32"], ld32=ld["g32"],
              g16=args["g16"], ld16=ld["g16"], gsum=gs.view() if with_gsum else None, ldgs=gs.ld, g32b=args["g32b"],
              ld32b=ld["g32b"])
    sync()
    tag = f"lrp_bwd:{'+'.join(use)}"
    gk.check(f"{tag}:dt", dt, *out["dt"])
    if with_gsum:
        blk = gs.block()
        assert bool(torch.isnan(blk[:, c.C:]).all())  # the block is 4 columns wider than C: those stay untouched
        blk[:, c.C:] = 0.0
        zero = torch.zeros(c.rows, 4, dtype=torch.float64)
        gk.check(f"{tag}:gsum", gs, torch.cat([out["gsum"][0], zero], 1), torch.cat([out["gsum"][1], zero], 1))
    else:
        assert gs.guard_hits() == 0 and bool(torch.isnan(gs.block()).all())


# ------------------------------------------------------------------------------------ tmae_unshuffle_bwd, tmae_gelu_bwd
@pytest.mark.parametrize("use_pre", [True, False])
@pytest.mark.parametrize("dy_dt,dt", TRIPLES)
def test_unshuffle_bwd(T, dy_dt, dt, use_pre):
    """n 2, H 3, W 5 (H != W), C4 12; ldy, ldp wider than C4 / 4 and distinct"""
    c = gk.unshuffle_case()
    _, _, (ref, bound) = gk.unshuffle_reference(c, dy_dt, dt, use_pre)
    cw = c.C4 // 4
    out = G1(ref.numel(), dt)
    T.unshuffle_bwd(dev(gk.pad(c.dy, cw + 5), dy_dt), cw + 5, dev(gk.pad(c.pre, cw + 2), dt) if use_pre else None, cw + 2,
                    out.view(), c.n, c.H, c.W, c.C4, dt, dy_dt == F32)
    sync()
    gk.check(f"unshuffle_bwd:pre{int(use_pre)}", out, ref.reshape(1, -1), bound.reshape(1, -1))


@pytest.mark.parametrize("dy_dt,dt", TRIPLES)
def test_gelu_bwd(T, dy_dt, dt):
    """total 1000 (ragged last workgroup); pre spans +-6 and includes 0"""
    dy, pre = gk.gelu_case()
    dy, pre = dy.to(dy_dt), pre.to(dt)
    ref, bound = gk.gelu_bwd_reference(dy, pre, dt)
    out = G1(1000, dt)
    T.gelu_bwd(dev(dy), dev(pre), out.view(), 1000, dt, dy_dt == F32)
    sync()
    gk.check("gelu_bwd", out, ref.reshape(1, -1), bound.reshape(1, -1))


# ------------------------------------------------------------------------------------ tmae_colsum
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C,ld", [(24, 32), (20, 23)])
@pytest.mark.parametrize("rows,remap", [(18, (6, 7, 1)), (1000, None)])
def test_colsum(T, rows, remap, C, ld, dt, acc):
    """C 24 / ld 32: the 8-wide arm; C 20 / ld 23: the scalar arm.  rows 18 remapped (one row dropped per group of 7);
    rows 1000 dense: 31 splits of 33 rows, the last one short"""
    G_, Gs, off = remap or (None, 0, 0)
    x, acc0 = gk.colsum_case(rows, C, total=22 if remap else rows)
    x = x.to(dt)
    ref, bound = gk.colsum_reference(x, rows, G_, Gs, off, acc0 if acc else None)
    out = G1(C, init=acc0 if acc else None)
    T.colsum(dev(gk.pad(x, ld)), rows, C, out.view(), ld=ld, row_group=G_, group_stride=Gs, row_offset=off,
             accumulate=acc, x_dtype=dt)
    sync()
    gk.check(f"colsum:r{rows}:C{C}:acc{int(acc)}", out, ref, bound)


@pytest.mark.parametrize("C,ld", [(24, 32), (20, 23)])
def test_colsum_small_workspace(C, ld):
    """the C entry with work_elems = 4 C: 31 splits are halved to 3; the workspace itself is guarded"""
    from textmae_amd import _lib
    from textmae_amd.ops import _stream, dtype_code

    rows = 1000
    x, _ = gk.colsum_case(rows, C)
    ref, bound = gk.colsum_reference(x, rows)
    out, ws, xd = G1(C), G1(4 * C), dev(gk.pad(x, ld))
    _lib.call("tmae_colsum", xd.data_ptr(), dtype_code(F32), ld, rows, C, rows, 0, 0, ws.view().data_ptr(),
              4 * C, out.view().data_ptr(), 0, _stream())
    sync()
    assert ws.guard_hits() == 0
    gk.check(f"colsum:small_ws:C{C}", out, ref, bound)


# ------------------------------------------------------------------------------------ tmae_layernorm_bwd
def _ln_run(T, c, use_dres, use_drs, op_dtype, acc, work_elems=None):
    from textmae_amd import _lib
    from textmae_amd.ops import _p, _stream, dtype_code

    D = c.D
    dx = G1(c.total * D)
    dxop = G1(c.total * D, op_dtype) if op_dtype is not None else None
    dg, db = G1(D, init=c.dg0 if acc else None), G1(D, init=c.db0 if acc else None)
    drs = G1(D, init=c.dr0 if acc else None) if use_drs else None
    kw = dict(dres=dev(c.dres) if use_dres else None, dxop=dxop.view() if dxop else None, row_group=c.G,
              group_stride=c.Gs, row_offset=c.off, accumulate=acc, dres_colsum=drs.view() if drs else None)
    xd, gd, dyd = dev(c.x), dev(c.gamma), dev(c.dy)
    if work_elems is None:
        T.layernorm_bwd(xd, gd, dyd, dx.view(), c.rows, D, c.eps, dg.view(), db.view(), **kw)
    else:
        ws = G1(work_elems)
        _lib.call("tmae_layernorm_bwd", xd.data_ptr(), gd.data_ptr(), dyd.data_ptr(), _p(kw["dres"]),
                  dx.view().data_ptr(), _p(kw["dxop"]), dtype_code(op_dtype or F32), c.rows, D, c.G or max(c.rows, 1),
                  c.Gs, c.off, c.eps, ws.view().data_ptr(), work_elems, dg.view().data_ptr(), db.view().data_ptr(),
                  _p(kw["dres_colsum"]), int(acc), _stream())
        sync()
        assert ws.guard_hits() == 0
    sync()
    return dx, dxop, dg, db, drs


def _ln_check(tag, c, out, dx, dxop, dg, db, drs):
    D = c.D
    written = torch.zeros(c.total, dtype=torch.bool)
    written[c.src] = True
    for name, g in (("dx", dx), ("dxop", dxop)):
        if g is None:
            continue
        blk = g.block().reshape(c.total, D)
        nan_rows = torch.isnan(blk.float()).all(1).cpu()
        assert torch.equal(nan_rows, ~written), f"{tag}:{name}: exactly the remapped rows are written"
        blk[~written.to(DEV)] = 0.0  # the dropped rows kept their NaN; the bound check is for the others
        ref, bound = (torch.zeros(c.total, D, dtype=torch.float64) for _ in range(2))
        ref[c.src], bound[c.src] = out[name]
        gk.check(f"{tag}:{name}", g, ref.reshape(1, -1), bound.reshape(1, -1))
    gk.check(f"{tag}:dgamma", dg, *out["dgamma"])
    gk.check(f"{tag}:dbeta", db, *out["dbeta"])
    if drs is not None:
        gk.check(f"{tag}:dres_colsum", drs, *out["dres_colsum"])


# (use_dres, use_dres_colsum, dxop dtype, accumulate): with / without dres and its column sums (RS true / false),
# dxop bf16 / f32 / None, accumulation onto non-zero dgamma / dbeta
LN_VARIANTS = [(True, True, BF16, False), (True, False, F32, True), (False, False, None, False), (True, True, None, True)]


@pytest.mark.parametrize("variant", range(len(LN_VARIANTS)))
@pytest.mark.parametrize("rows,remap", [(18, (6, 7, 1)), (3, None)])
@pytest.mark.parametrize("D", [512, 768, 1024, 1280, 2048])
def test_layernorm_bwd(T, D, rows, remap, variant):
    """D 512 / 768 / 1024 / 1280 / 2048: VPL 2, 3, 4, 8, 8.  rows 18 remapped (cls rows dropped: they keep their NaN);
    rows 3: fewer rows than the workgroup has waves"""
    use_dres, use_drs, op, acc = LN_VARIANTS[variant]
    G_, Gs, off = remap or (None, 0, 0)
    c = gk.ln_case(rows, D, G_, Gs, off)
    out = gk.ln_bwd_reference(c, use_dres, op, acc)
    _ln_check(f"ln_bwd:D{D}:r{rows}:v{variant}", c, out, *_ln_run(T, c, use_dres, use_drs, op, acc))


def test_layernorm_bwd_small_workspace(T):
    """rows 18 would take 3 workgroups; a workspace of 2 x 3 D elements halves them to 1"""
    c = gk.ln_case(18, 768, 6, 7, 1)
    out = gk.ln_bwd_reference(c, True, BF16, False)
    _ln_check("ln_bwd:small_ws", c, out, *_ln_run(T, c, True, True, BF16, False, work_elems=2 * 3 * 768))


# ------------------------------------------------------------------------------------ tmae_decoder_embed_bwd_gather
@pytest.mark.parametrize("mask", ["none", "fresh", "accumulate"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("L,ntok", [(16, 1), (16, 9), (16, 16), (16, 17), (300, 10)])
def test_decoder_embed_bwd_gather(T, L, ntok, dt, mask):
    """n 3, D 72 (past one 64-column block).  ntok 1: nothing kept; 9: MCM's off-by-one; 16: everything kept; 17: MAE's
    K + 1 (no masked position at all); L 300 / ntok 10: 291 masked positions, the staging loop's second pass"""
    c = gk.dec_gather_case(3, L, 72)
    acc = mask == "accumulate"
    out = gk.dec_gather_reference(c, ntok, dt, acc)
    tok = G1(c.n * ntok * c.D, dt)
    dmask = G1(c.D, init=c.dmask0 if acc else None) if mask != "none" else None
    T.decoder_embed_bwd_gather(dev(c.grad), dev(c.ids), tok.view(), c.n, ntok, L, c.D, dt,
                               dmask=dmask.view() if dmask else None, accumulate=acc)
    sync()
    tag = f"dec_gather:L{L}:ntok{ntok}:{mask}"
    ref, bound = out["tok"]
    gk.check(f"{tag}:tok", tok, ref.reshape(1, -1), bound.reshape(1, -1))
    if dmask is not None:
        gk.check(f"{tag}:dmask", dmask, *out["dmask"])


# ------------------------------------------------------------------------------------ gathers and copies (bitwise)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("keep", [1, 9])
@pytest.mark.parametrize("arm", ["vec16", "scalar14", "misaligned16"])
def test_patch_gather(T, arm, keep, dt):
    """patch 16 on 64^2: the 8-wide arm; patch 14 on 56^2: the scalar arm, rows 592 wide with a zero tail of 4; patch 16
    with imgs 4 bytes past a 16-byte boundary: the scalar arm"""
    P, S = (14, 56) if arm == "scalar14" else (16, 64)
    g = gk._gen(17 + keep)
    imgs = torch.rand(3, 3, S, S, generator=g)
    L = (S // P) ** 2
    ids = torch.stack([torch.randperm(L, generator=g) for _ in range(3)])
    val = gk.patch_gather_values(imgs, ids, keep, P)
    if arm == "misaligned16":
        base = torch.empty(imgs.numel() + 4, device=DEV)
        di = base[1:1 + imgs.numel()].view(imgs.shape)
        di.copy_(imgs)
        assert di.data_ptr() % 16 == 4
    else:
        di = dev(imgs)
    out = G1(val.numel(), dt)
    T.patch_gather(di, dev(ids), out.view(), keep, P, dt)
    sync()
    ref, bound = gk.exact_out(val, dt)
    assert gk.check(f"patch_gather:{arm}:keep{keep}", out, ref.reshape(1, -1), bound.reshape(1, -1)) == 0.0


def test_patchify_bf16(T):
    imgs = torch.randn(2, 3, 32, 32, generator=gk._gen(18))
    ref, bound = gk.exact_out(orc.patchify(imgs, 8).to(BF16).reshape(1, -1), BF16)
    out = G1(imgs.numel(), BF16)
    T.patchify(dev(imgs), out.view(), 8, BF16)
    sync()
    assert gk.check("patchify:bf16", out, ref, bound) == 0.0


@pytest.mark.parametrize("dt", DTYPES)
def test_copy2d(T, dt):
    src = torch.randn(37, 21, generator=gk._gen(19)).to(dt)
    out = G(37, 21, dt)
    T.copy2d(dev(gk.pad(src, 29)), 29, out.view(), out.ld, 37, 21, src.element_size())
    sync()
    ref, bound = gk.exact_out(src, dt)
    assert gk.check(f"copy2d:esz{src.element_size()}", out, ref, bound) == 0.0


def test_add(T):
    g = gk._gen(20)
    a, b = torch.randn(1000, generator=g), torch.randn(1000, generator=g) * 100
    out = G1(1000)
    T.add(dev(a), dev(b), out.view()[0, :1000])  # the wrapper takes the length from `out`
    sync()
    ref, bound = gk.exact_out((a + b).reshape(1, -1))
    assert gk.check("add", out, ref, bound) == 0.0


# ------------------------------------------------------------------------------------ forward extras
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,T_,H,dh", [(2, 33, 3, 32), (1, 161, 2, 80), (2, 145, 2, 64)])
def test_mha_fwd_lse(T, B, T_, H, dh, dt):
    """the lse tmae_mha_bwd reads back: base 2, [b][h][t]"""
    qkv = torch.randn(B * T_, 3 * H * dh, generator=gk._gen(T_)).to(dt)
    scale = dh ** -0.5
    ref, bound = gk.lse_reference(qkv, B, T_, H, dh, scale)
    out = torch.empty(B * T_, H * dh, device=DEV, dtype=dt)
    lse = G1(B * H * T_)
    T.mha_lse(dev(qkv), B, T_, H, dh, scale, dt, out, lse.view())
    sync()
    gk.check(f"mha_lse:T{T_}:dh{dh}", lse, ref, bound)


def _bitwise(metric, g, values):
    ref, bound = gk.exact_out(values.cpu(), values.dtype)
    assert gk.check(metric, g, ref, bound) == 0.0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,N,K", [(129, 704, 640), (77, 32, 96)])
def test_linear_fwd_pre(T, tmae, M, N, K, dt):
    """pre is bitwise the act = 0 output of tmae_linear_fwd, out bitwise its act = 1 output"""
    x, w, b = gemm_check.operands(M, N, K, dt)
    xd, wd, bd = dev(x), dev(w), dev(b)
    out, pre = G(M, N, dt), G(M, N, dt)
    T.linear_pre(xd, wd, bd, dt, 1, out.view(), pre.view())
    y0 = tmae.ops.linear(xd, wd, bd, dt, act=0)
    y1 = tmae.ops.linear(xd, wd, bd, dt, act=1)
    sync()
    _bitwise(f"linear_pre:{M}:pre", pre, y0)
    _bitwise(f"linear_pre:{M}:out", out, y1)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,N,K", [(129, 704, 640), (77, 32, 96)])
def test_linear_residual_out(T, tmae, M, N, K, dt):
    """bitwise tmae_linear_residual_fwd applied to a copy of resid; resid itself untouched"""
    x, w, b = gemm_check.operands(M, N, K, dt)
    r0 = torch.randn(M, N, generator=gk._gen(M))
    xd, wd, bd = dev(x), dev(w), dev(b)
    resid, out, inplace = G(M, N, init=r0), G(M, N), G(M, N, init=r0)
    T.linear_residual_out(xd, wd, bd, resid.view(), out.view(), dt)
    tmae.ops.linear_residual(xd, wd, bd, inplace.view(), dt)
    sync()
    assert inplace.guard_hits() == 0
    _bitwise(f"linear_residual_out:{M}:out", out, inplace.block().clone())
    _bitwise(f"linear_residual_out:{M}:resid", resid, r0)


def _nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)


def _wk(w, dtype):
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous().to(dtype).to(DEV)


@pytest.mark.parametrize("dt", DTYPES)
def test_conv3x3_pre_pixel_shuffle(tmae, dt):
    """test_subpel_conv's shape: pre (pixel-shuffled layout, the output's dtype) is bitwise the act = 0 output"""
    torch.manual_seed(5)
    n, H, cin, c = 2, 6, 48, 16
    x = torch.randn(n, cin, H, H)
    w, b = torch.randn(4 * c, cin, 3, 3) / (9 * cin) ** 0.5, torch.randn(4 * c)
    xd, wd, bd = _nhwc(x, dt), _wk(w, dt), b.to(DEV)
    rows = n * 4 * H * H
    y, pre, y0 = G(rows, c, dt), G(rows, c, dt), G(rows, c, dt)
    tmae.ops.conv3x3(xd, cin, cin, n, H, H, wd, bd, y.view(), y.ld, 4 * c, dt, act=1, pixel_shuffle=True,
                     y_f32=dt == F32, pre=pre.view(), ldp=pre.ld)
    tmae.ops.conv3x3(xd, cin, cin, n, H, H, wd, bd, y0.view(), y0.ld, 4 * c, dt, act=0, pixel_shuffle=True,
                     y_f32=dt == F32)
    sync()
    assert y.guard_hits() == 0 and y0.guard_hits() == 0 and not bool(torch.isnan(y.block().float()).any())
    _bitwise("conv3x3_pre:pixel_shuffle", pre, y0.block().clone())


@pytest.mark.parametrize("dt", DTYPES)
def test_conv3x3_pre_lrp_epilogue(tmae, dt):
    """test_conv3x3_lrp_epilogue's shape: the f32 pre-tanh rows (ldp wider than cout) are bitwise the act = 0 f32
    output of the same conv"""
    torch.manual_seed(12)
    n, H, cin, cout = 2, 12, 80, 32
    x = torch.randn(n, cin, H, H)
    w, b = torch.randn(cout, cin, 3, 3) / (9 * cin) ** 0.5, torch.randn(cout)
    src = (torch.randn(n * H * H, 96) * 4).to(DEV)
    xd, wd, bd = _nhwc(x, dt), _wk(w, dt), b.to(DEV)
    rows = n * H * H
    y, pre, y0 = G(rows, cout, dt), G(rows, cout), G(rows, cout)
    tmae.ops.conv3x3(xd, cin, cin, n, H, H, wd, bd, y.view(), y.ld, cout, dt, y_f32=dt == F32,
                     lrp_src=src.data_ptr() + 40 * 4, ld_src=96, pre=pre.view(), ldp=pre.ld)
    tmae.ops.conv3x3(xd, cin, cin, n, H, H, wd, bd, y0.view(), y0.ld, cout, dt, act=0, y_f32=True)
    sync()
    assert y.guard_hits() == 0 and y0.guard_hits() == 0 and not bool(torch.isnan(y.block().float()).any())
    _bitwise("conv3x3_pre:lrp", pre, y0.block().clone())
