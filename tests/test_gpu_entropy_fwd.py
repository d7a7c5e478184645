"""The forward entropy models and the coding kernels on the MI355X, one kernel per test, every output element bounded on
its own (tests/entropy_check.py: float64 references, bounds carried through the kernels' formulas, NaN- or
sentinel-filled guarded outputs, NaN padding, pairwise distinct leading dimensions, nothing skipped).

The whole-model tests compare likelihoods through max|a - b| / max|b| < 1e-5, which sees no element below 1e-4 although
the loss is -log2(lik); the coding kernels were reached through round trips only, which an indexing error made alike
by encoder and decoder passes.  Here the likelihood kernels are bounded per element at the shapes that reach each arm
(sub-pass, ragged second pass, last tiled and first element-kernel shape of tmae_gc_slices_*; ragged 64-channel block
of tmae_eb_likelihood_fwd), the integer and single-rounded outputs are bitwise, and the agreements decoding relies on
are asserted: tiled against element path, tmae_gc_indexes against the indexes of tmae_gc_slices_code,
tmae_gc_dequantize against its yhat, tmae_eb_dequantize(tmae_eb_symbols(z)) against the eval zhat.

Largest error / bound per kernel and output on an MI355X (87 cases, under 4 s); 0 where the comparison is bitwise, no guard
element written, no element skipped:

    kernel                 output            ratio      kernel                 output            ratio
    gc_slices_fwd          lik               0.550      eb_likelihood_fwd      lik               0.237
                           yhat f32 / bf16   0 / 0.996                         zhat f32 / bf16   0 / 0.989
                           yhat32            0          eb_aux_loss                              0.004
    gc_slices_code         lik               0.423      eb_symbols                               0
                           yhat f32 / bf16   0 / 0.996  eb_dequantize          zhat f32 / bf16   0 / 0.989
                           yhat32            0          gc_pmf                 pmf / tail        0.314 / 0.284
                           symbols, indexes  0          eb_pmf                 pmf / tail        0.048 / 0.011
    gc_slices (element     lik               0.545      gc_indexes                               0
      kernel, HW = 290)    all others        as above   gc_dequantize          yhat f32 / bf16   0 / 0.996
    gc_likelihood_fwd      lik               0.354                             yhat32            0
                           x_tilde           0          invert_permutation                       0

A bf16 store is rounded to nearest, so its ratio approaches 1 on any large enough output.  0.237 is |1e-9f - 1e-9|
over u 1e-9: a clamped element; every unclamped EntropyBottleneck likelihood is closer than that.  The f32 ratios above
0.5 are training likelihoods whose sigma is below the bound (s = 0.11f) and whose v = |y + noise - mu| lies just past
0.5, so that 0.5 - v cancels and the roundings of y + noise and of the subtraction of mu, each half an ulp of a number
of order one, are divided by 0.11: gc_slices_fwd 0.550 (first_element, element 3315: v 0.50270, out 0.4902200699, ref
0.4902205377, bound 8.5e-7), 0.545 (last_tiled, element 12066: v 0.50284, out 0.4897152781, ref 0.4897157219, bound
8.1e-7; the same element through the element kernel at HW = 290, bit for bit), 0.513 (ragged_pass, element 3058:
v 0.59968, out 0.1824205220, ref 0.1824202986, bound 4.4e-7).  The torch f32 restatement reaches 0.515, 0.545 and
0.513 at the same shapes.
No test of this file found a kernel outside its bound, and both bitwise promises hold: tiled against element path, the
encode-side against the decode-side kernels.
"""
import copy
import functools

import pytest
import torch

import entropy_check as ek
import glue_check as gk
from glue_check import BF16, F32, Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [F32, BF16]
TABLES = {"model": ek.model_table, "low": ek.low_table}


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def G1(n, dtype=F32, init=None):
    return Guarded(1, n, dtype, device=DEV, init=None if init is None else init.reshape(1, -1))


def I1(n, dtype=ek.I32):
    return ek.GuardedInt(1, n, dtype, device=DEV)


def sync():
    torch.cuda.synchronize()


def tname(dt):
    return "bf16" if dt == BF16 else "f32"


# ------------------------------------------------------------------------------------ tmae_gc_slices_fwd / _code
@functools.lru_cache(None)
def gcf_case(shape, table="model", n=None, HW=None):
    return ek.gcf_case(shape, TABLES[table](), n, HW)


@functools.lru_cache(None)
def gcf_reference(shape, training, yt, code, table="model", n=None, HW=None):
    """computed once per case and shared; never written to"""
    return ek.gcf_reference(gcf_case(shape, table, n, HW), training, yt, code)


def gcf_launch(tmae, c, training, yt, code, yhat32=True):
    inp = ek.gcf_inputs(c, training, DEV)
    o = ek.gcf_outputs(c, yt, code, DEV, yhat32)  # asserts the leading dimensions pairwise distinct
    y32, ld32 = (o.yhat32.view(), o.yhat32.ld) if yhat32 else (None, 0)
    if code:
        tmae.ops.gc_slices_code(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, o.lik.view(), c.Mtot,
                                o.yhat.view(), yt, o.yhat.ld, y32, ld32, c.n, c.HW, c.nsl, c.sw, o.sym.view(),
                                o.idx.view(), dev(c.table))
    else:
        tmae.ops.gc_slices(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, inp.noise, o.lik.view(),
                           c.Mtot, o.yhat.view(), yt, o.yhat.ld, y32, ld32, c.n, c.HW, c.nsl, c.sw)
    sync()
    return inp, o


@pytest.mark.parametrize("yhat32", [True, False])
@pytest.mark.parametrize("yt", DTYPES)
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", list(ek.GCF_SHAPES))
def test_gc_slices_fwd(tmae, shape, training, yt, yhat32):
    """nslices = 2, yoff = 3, Mtot = yoff + 2 sw + 4; ldy = Mtot + 8, ld_ms = sw + 3, ms_stride = M ld_ms + 5,
    ld_yhat = Mtot + 16, ld32 = Mtot + 19.  Seeds and class counts: ek.GCF_SEEDS"""
    c = gcf_case(shape)
    out, p = gcf_reference(shape, training, yt, False)
    assert p.skipped == 0
    _, o = gcf_launch(tmae, c, training, yt, False, yhat32)
    ek.gcf_check(f"gc_slices_fwd:{shape}:{'train' if training else 'eval'}:{tname(yt)}", o, out)


@pytest.mark.parametrize("yt", DTYPES)
@pytest.mark.parametrize("shape,table", [(s, "model") for s in ek.GCF_SHAPES] + [("sub_pass", "low")])
def test_gc_slices_code(tmae, shape, table, yt):
    """symbols and indexes bitwise in the coder's order; the same indexes from tmae_gc_indexes; the same yhat / yhat32
    from tmae_gc_dequantize(symbols, mu).  The 24-entry table with entries below 0.11 is there because against the
    model's table (table[0] == 0.11f) indexes from the unbounded sigma are the same numbers"""
    c = gcf_case(shape, table)
    out, p = gcf_reference(shape, False, yt, True, table)
    inp, o = gcf_launch(tmae, c, False, yt, True)
    tag = f"gc_slices_code:{shape}:{table}:{tname(yt)}"
    ek.gcf_check(tag, o, out)
    total = c.nsl * c.M * c.sw
    idx = I1(total)
    tmae.ops.gc_indexes(inp.sigma, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, dev(c.table), 0.11, idx.view())
    sync()
    ek.check_exact(f"gc_indexes:{shape}:{table}", idx, out["idx"])
    assert torch.equal(idx.result(), o.idx.result())
    d = ek.gcf_outputs(c, yt, False, DEV)
    tmae.ops.gc_dequantize(o.sym.view(), inp.mu, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, c.yoff, d.yhat.view(), yt,
                           d.yhat.ld, d.yhat32.view(), d.yhat32.ld)
    sync()
    gk.check(f"gc_dequantize:{shape}:yhat:{tname(yt)}", d.yhat, *out["yhat"])
    gk.check(f"gc_dequantize:{shape}:yhat32", d.yhat32, *out["yhat32"])
    assert torch.equal(d.yhat.block().cpu(), o.yhat.block().cpu())  # bitwise, bf16 included
    assert torch.equal(d.yhat32.block().cpu(), o.yhat32.block().cpu())


def test_gc_indexes_other_bound(tmae):
    """scale_bound = 0.25: the bound is the kernel's argument, not a constant"""
    c = gcf_case("sub_pass")
    inp = ek.gcf_inputs(c, False, DEV)
    idx = I1(c.nsl * c.M * c.sw)
    tmae.ops.gc_indexes(inp.sigma, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, dev(c.table), 0.25, idx.view())
    sync()
    ref = ek.coder_order(ek.build_indexes32(c.sigma, c.table, 0.25), c.n, c.HW)
    assert int((ref != ek.coder_order(ek.build_indexes32(c.sigma, c.table), c.n, c.HW)).sum()) >= 4
    ek.check_exact("gc_indexes:sub_pass:bound0.25", idx, ref)


def _rows(c, g):
    """a dense NCHW likelihood buffer -> [M][Mtot]"""
    return g.block().cpu().reshape(c.n, c.Mtot, c.HW).permute(0, 2, 1).reshape(c.M, c.Mtot)


def _slices(c, g):
    """coder order -> [slice][M][sw]"""
    return g.result().reshape(c.nsl, c.n, c.sw, c.HW).permute(0, 1, 3, 2).reshape(c.nsl, c.M, c.sw)


@pytest.mark.parametrize("yt", DTYPES)
@pytest.mark.parametrize("form", ["train", "eval", "code"])
def test_gc_slices_tiled_equals_element(tmae, form, yt):
    """csrc/conv.hip promises 'bitwise the same outputs': the same 290 x 64 element values as (n = 2, HW = 145), the
    last tiled shape, and as (n = 1, HW = 290), which takes the element kernel"""
    training, code = form == "train", form == "code"
    a, b = gcf_case("last_tiled"), gcf_case("last_tiled", "model", 1, 290)
    assert a.HW * (a.sw + 1) <= 4800 < b.HW * (b.sw + 1) and torch.equal(a.y, b.y) and torch.equal(a.sigma, b.sigma)
    _, oa = gcf_launch(tmae, a, training, yt, code)
    _, ob = gcf_launch(tmae, b, training, yt, code)
    ek.gcf_check(f"gc_slices_element:{form}:{tname(yt)}", ob, gcf_reference("last_tiled", training, yt, code, "model", 1, 290)[0])
    assert torch.equal(_rows(a, oa.lik), _rows(b, ob.lik))
    assert torch.equal(oa.yhat.block().cpu(), ob.yhat.block().cpu())
    assert torch.equal(oa.yhat32.block().cpu(), ob.yhat32.block().cpu())
    if code:
        assert torch.equal(_slices(a, oa.sym), _slices(b, ob.sym)) and torch.equal(_slices(a, oa.idx), _slices(b, ob.idx))


# ------------------------------------------------------------------------------------ tmae_gc_likelihood_fwd
@pytest.mark.parametrize("bound", [0.11, 0.25])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("means", [True, False])
def test_gc_likelihood_fwd(tmae, means, training, bound):
    """total = 528: three workgroups, the last ragged.  x~ is rounded once: bitwise"""
    from textmae_amd import _lib
    from textmae_amd.ops import _stream

    el = ek.flat_case(ek.model_table())
    (ref, b), xt, r = ek.flat_reference(el, training, means, bound)
    n = el.y.numel()
    lik, xto = G1(n), G1(n)
    x, sg, mu, nz = dev(el.y), dev(el.sigma), dev(el.mu) if means else None, dev(el.noise) if training else None
    _lib.call("tmae_gc_likelihood_fwd", x.data_ptr(), sg.data_ptr(), None if mu is None else mu.data_ptr(),
              None if nz is None else nz.data_ptr(), xto.view().data_ptr(), lik.view().data_ptr(), n, float(bound), _stream())
    sync()
    tag = f"gc_likelihood_fwd:{'means' if means else 'nomeans'}:{'train' if training else 'eval'}:b{bound}"
    gk.check(f"{tag}:lik", lik, ref, b)
    ek.check_bits(f"{tag}:x_tilde", xto, xt.reshape(1, -1))


# ------------------------------------------------------------------------------------ EntropyBottleneck
@pytest.fixture(scope="module")
def ebs(tmae):
    return {C: gk.eb_module(tmae, C) for C in (5, 70, 90)}


_EBF = {}


def ebf(ebs, C, HW, training, zt):
    """the case and its reference, computed once and shared; never written to"""
    key = (C, HW, training, zt)
    if key not in _EBF:
        c = ek.ebf_case(ebs[C], HW)
        _EBF[key] = (c, ek.ebf_reference(c, training, zt))
    return _EBF[key]


def _eb_device(eb, sd):
    m = copy.deepcopy(eb)
    m.load_state_dict({k[len(gk.EB_PRE):]: v for k, v in sd.items()})
    return m.to(DEV)


@pytest.mark.parametrize("zt", DTYPES)
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("C,HW", list(ek.EBF_SEEDS))
def test_eb_likelihood_fwd(tmae, ebs, C, HW, training, zt):
    """n = 2; C = 70: two 64-channel blocks, the second with 6 channels (the c >= C arm); parameters of
    gk.eb_module, one raw _matrix2 entry at 21 (softplus threshold).  zhat bitwise (bf16: its rounding)"""
    c, (out, p) = ebf(ebs, C, HW, training, zt)
    assert p.skipped == 0
    m = _eb_device(ebs[C], c.sd)
    lik, zhat = G1(c.n * C * HW), G1(c.N * C, zt)
    tmae.ops.eb_likelihood(m, dev(c.z), c.n, C, HW, dev(c.noise) if training else None, lik.view(), zhat.view())
    sync()
    tag = f"eb_likelihood_fwd:C{C}:HW{HW}:{'train' if training else 'eval'}"
    gk.check(f"{tag}:lik", lik, *out["lik"])
    gk.check(f"{tag}:zhat", zhat, out["zhat"][0].reshape(1, -1), out["zhat"][1].reshape(1, -1))


@pytest.mark.parametrize("C", [5, 90])
def test_eb_aux_loss(tmae, ebs, C):
    """C = 90: 270 terms, past one pass of the 256 threads"""
    sd = {gk.EB_PRE + k: v.detach().clone().float() for k, v in ebs[C].state_dict().items()}
    ref, bound = ek.eb_aux_loss_reference(sd)
    m = copy.deepcopy(ebs[C]).to(DEV)
    out = G1(1)
    tmae.ops.eb_aux_loss(m, out.view())
    sync()
    gk.check(f"eb_aux_loss:C{C}", out, ref, bound)


@pytest.mark.parametrize("zt", DTYPES)
@pytest.mark.parametrize("C,HW", list(ek.EBF_SEEDS))
def test_eb_symbols_dequantize(tmae, ebs, C, HW, zt):
    """symbols bitwise (NCHW); dequantised symbols bitwise the eval zhat of tmae_eb_likelihood_fwd"""
    c, (out, p) = ebf(ebs, C, HW, False, zt)
    m = _eb_device(ebs[C], c.sd)
    sym = I1(c.n * C * HW)
    tmae.ops.eb_symbols(m, dev(c.z), c.n, C, HW, sym.view())
    sync()
    ek.check_exact(f"eb_symbols:C{C}:HW{HW}", sym, out["sym"])
    zq, zhat, lik = G1(c.N * C, zt), G1(c.N * C, zt), G1(c.n * C * HW)
    tmae.ops.eb_dequantize(m, sym.view(), c.n, C, HW, zq.view())
    tmae.ops.eb_likelihood(m, dev(c.z), c.n, C, HW, None, lik.view(), zhat.view())
    sync()
    gk.check(f"eb_dequantize:C{C}:HW{HW}", zq, out["zhat"][0].reshape(1, -1), out["zhat"][1].reshape(1, -1))
    assert zhat.guard_hits() == 0 and torch.equal(zq.block().cpu(), zhat.block().cpu())


# ------------------------------------------------------------------------------------ pmf rows and tail masses
def test_gc_pmf(tmae):
    """the model's 64-entry table; centres and the padded length from oracle/coding_oracle.py"""
    from textmae_amd import _lib
    from textmae_amd.ops import _stream

    t = ek.model_table()
    _, _, center, L = ek.co.gc_pmf(t)
    (ref, b), (tref, tb) = ek.gc_pmf_reference(t, center, L)
    pmf, tail = G1(64 * L), G1(64)
    td, cd = dev(t), dev(center.to(torch.int32))
    _lib.call("tmae_gc_pmf", td.data_ptr(), cd.data_ptr(), 64, L, pmf.view().data_ptr(), tail.view().data_ptr(), _stream())
    sync()
    gk.check("gc_pmf:pmf", pmf, ref.reshape(1, -1), b.reshape(1, -1))
    gk.check("gc_pmf:tail", tail, tref, tb)


@pytest.mark.parametrize("quantiles", ["module", "narrow"])
def test_eb_pmf(tmae, ebs, quantiles):
    """C = 5; starts and the padded length from oracle/coding_oracle.py; the tail takes upstream's last sample of the
    PADDED range.  "narrow": quantiles 1 .. 3 samples from the median, so the lengths differ and the tails are masses
    f32 holds (the module's own lie below 1e-40)"""
    from textmae_amd import _lib
    from textmae_amd.ops import _stream

    C = 5
    sd = {gk.EB_PRE + k: v.detach().clone().float() for k, v in ebs[C].state_dict().items()}
    if quantiles == "narrow":
        sd = ek.narrow_quantiles(sd)
    _, _, start, L = ek.co.eb_pmf(sd, gk.EB_PRE)
    (ref, b), (tref, tb) = ek.eb_pmf_reference(sd, start, L)
    m = _eb_device(ebs[C], sd)
    pmf, tail = G1(C * L), G1(C)
    table = torch.empty(C, 59, device=DEV)
    sd_ = dev(start.float())
    _lib.call("tmae_eb_pmf", tmae.ops._eb_params(m), table.data_ptr(), sd_.data_ptr(), C, L, pmf.view().data_ptr(),
              tail.view().data_ptr(), _stream())
    sync()
    gk.check(f"eb_pmf:{quantiles}:pmf", pmf, ref.reshape(1, -1), b.reshape(1, -1))
    gk.check(f"eb_pmf:{quantiles}:tail", tail, tref, tb)


# ------------------------------------------------------------------------------------ tmae_invert_permutation
def test_invert_permutation(tmae):
    """n = 3, L = 100: seeded permutations invert exactly; an out-of-range entry and a -1 leave the two slots they
    would have named at the sentinel, and the rest of the row is correct"""
    from textmae_amd import _lib
    from textmae_amd.ops import _stream

    p = ek.perm_case()
    bad = p.clone()
    bad[1, 3], bad[1, 50] = 100, -1
    for name, perm in (("valid", p), ("out_of_range", bad)):
        ref = ek.invert_reference(perm)
        inv = ek.GuardedInt(1, perm.numel(), ek.I64, device=DEV)
        pd = dev(perm)
        _lib.call("tmae_invert_permutation", pd.data_ptr(), inv.view().data_ptr(), 3, 100, _stream())
        sync()
        ek.check_exact(f"invert_permutation:{name}", inv, ref)
        assert int((ref == ek.SENTINEL).sum()) == (0 if name == "valid" else 2)
