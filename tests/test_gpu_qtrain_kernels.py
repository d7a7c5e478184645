"""The kernels of the forward and backward at a per-image quantiser step element by element:
tmae_gc_slices_fwd_q (csrc/coding.hip), tmae_gc_bwd_q (csrc/train.hip) and tmae_lic_stack's chain with cq
(csrc/lic_stack_q.hip), against tests/qtrain_check.py (checked on the CPU by tests/test_qtrain_host.py).

Three images at q = (-32, 0, 11): steps 1/16, 1 and 2^(11/8).  qstep_check.SHAPES: HW = 16, sw = 16 with 1, 2 and 6
slices runs the LDS-tiled kernel, HW = 324 the element kernel.
* eval forward: yhat, yhat32 and lik bit for bit what tmae_gc_slices_code_q writes into the same buffers;
* training forward: yhat / yhat32 bit for bit the numpy f32 restatement, lik inside the E bound of the float64
  definition, no element skipped; the tiled form bit for bit the element form on the same values;
* backward: both forms, both dtypes, with and without glik / gyp, against float64 autograd with the kernel's formula
  carried through E (skip share under glue_check.SKIP_CAP; census in test_qtrain_host.py);
* chain with cq: y_hat_pre bit for bit the restatement of the launch's own f32 mu, cy / cy2 bit for bit the unchained
  sequence mean stack, tmae_gc_slices_fwd_q, lrp stack."""
import numpy as np
import pytest
import torch

import conv_check as cc
import entropy_check as ek
import glue_check as gk
import qstep_check as qk
import qtrain_check as tk
from glue_check import BF16, F32, Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [F32, BF16]


@pytest.fixture(scope="module")
def T():
    import textmae_amd  # noqa: F401
    from textmae_amd import train_ops

    return train_ops


def dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).contiguous().to(DEV)


def qdev(q):
    return None if q is None else torch.tensor(q, dtype=torch.int32, device=DEV)


def tname(dt):
    return "bf16" if dt == BF16 else "f32"


def sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ tmae_gc_slices_fwd_q
def launch_fwd(tmae, c, training, yt, q, yhat32=True, bound=0.11):
    inp = ek.gcf_inputs(c, training, DEV)
    o = ek.gcf_outputs(c, yt, False, DEV, yhat32)
    y32, ld32 = (o.yhat32.view(), o.yhat32.ld) if yhat32 else (None, 0)
    tmae.ops.gc_slices_fwd_q(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, inp.noise, o.lik.view(),
                             c.Mtot, o.yhat.view(), yt, o.yhat.ld, y32, ld32, c.n, c.HW, c.nsl, c.sw, bound, qdev(q))
    sync()
    return inp, o


def _same(a, b, name):
    assert a.guard_hits() == 0 and b.guard_hits() == 0, name
    x, y = a.buf.cpu(), b.buf.cpu()
    it = torch.int32 if x.element_size() == 4 else torch.int16
    assert torch.equal(x.view(it), y.view(it)), f"{name}: not bit for bit (guards included)"


@pytest.mark.parametrize("yt", DTYPES)
@pytest.mark.parametrize("shape", list(qk.SHAPES))
def test_fwd_q_eval_is_the_coders_kernel(tmae, shape, yt):
    """eval: yhat, yhat32 and lik bit for bit tmae_gc_slices_code_q's, and (through it) the restatement's"""
    c = tk.fwd_case(shape)
    out, _ = qk.reference(shape)
    inp, o = launch_fwd(tmae, c, False, yt, c.q)
    code = ek.gcf_outputs(c, yt, True, DEV, True)
    tmae.ops.gc_slices_code_q(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, code.lik.view(), c.Mtot,
                              code.yhat.view(), yt, code.yhat.ld, code.yhat32.view(), code.yhat32.ld, c.n, c.HW, c.nsl,
                              c.sw, code.sym.view(), code.idx.view(), dev(c.table), 0.11, qdev(c.q))
    sync()
    for name in ("yhat", "yhat32", "lik"):
        _same(getattr(o, name), getattr(code, name), f"gc_slices_fwd_q:eval:{shape}:{name}")
    tag = f"gc_slices_fwd_q:{shape}:eval:{tname(yt)}"
    ek.check_bits(f"{tag}:yhat", o.yhat, qk.yhat_values(c, out, yt))
    ek.check_bits(f"{tag}:yhat32", o.yhat32, out["yhat32"])
    gk.check(f"{tag}:lik", o.lik, *out["lik"])


@pytest.mark.parametrize("yhat32", [True, False])
@pytest.mark.parametrize("yt", DTYPES)
@pytest.mark.parametrize("shape", list(qk.SHAPES))
def test_fwd_q_training(tmae, shape, yt, yhat32):
    c = tk.fwd_case(shape)
    out, _ = tk.fwd_reference(shape)
    _, o = launch_fwd(tmae, c, True, yt, c.q, yhat32)
    tag = f"gc_slices_fwd_q:{shape}:train:{tname(yt)}"
    ek.check_bits(f"{tag}:yhat", o.yhat, qk.yhat_values(c, out, yt))
    if yhat32:
        ek.check_bits(f"{tag}:yhat32", o.yhat32, out["yhat32"])
    gk.check(f"{tag}:lik", o.lik, *out["lik"])


@pytest.mark.parametrize("q", [None, (0, 0, 0)], ids=["null", "zeros"])
def test_fwd_q_step_one(tmae, q):
    """q = NULL and q = 0: y_hat bit for bit tmae_gc_slices_fwd's; the likelihoods are other roundings of the same
    numbers (|y + noise - mu| there, |(y - mu) / 1 + noise| here), so they are held to their own bounds"""
    c = NS_with_noise(qk.case("tiled2", None), 2062)
    for training in (True, False):
        inp, o = launch_fwd(tmae, c, training, F32, q)
        old = ek.gcf_outputs(c, F32, False, DEV, True)
        tmae.ops.gc_slices(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, inp.noise, old.lik.view(),
                           c.Mtot, old.yhat.view(), F32, old.yhat.ld, old.yhat32.view(), old.yhat32.ld, c.n, c.HW, c.nsl,
                           c.sw)
        sync()
        _same(o.yhat, old.yhat, "yhat")
        _same(o.yhat32, old.yhat32, "yhat32")
        if training:  # this kernel's own formula at delta = 1
            ys, nz = ek.gcf_slices(c, c.y).contiguous().numpy(), ek.gcf_slices(c, c.noise).contiguous().numpy()
            lik, lb = tk.lik_train_reference(ys, c.mu.numpy(), c.sigma.numpy(), nz, np.ones_like(ys))
            ref, b = c.lik0.double().clone(), torch.zeros(c.M, c.Mtot, dtype=torch.float64)
            ref[:, c.sl], b[:, c.sl] = ek.gcf_rows(c, lik), ek.gcf_rows(c, lb)
            gk.check("gc_slices_fwd_q:q0:train:lik", o.lik, ek.to_nchw(ref, c.n, c.HW).reshape(1, -1),
                     ek.to_nchw(b, c.n, c.HW).reshape(1, -1), log=False)
        else:  # |qi| is exact where the existing kernel takes |fl(qi + mu) - mu|: inside that kernel's own bound
            ref, _ = ek.gcf_reference(c, False, F32)
            gk.check("gc_slices_fwd_q:q0:eval:lik", o.lik, *ref["lik"], log=False)


def NS_with_noise(c, seed):
    from types import SimpleNamespace as NS

    c = NS(**vars(c))
    c.noise = torch.rand(c.M, c.Mtot, generator=gk._gen(seed)) - 0.5
    return c


def _rows(c, g):
    """a dense NCHW likelihood buffer -> [M][Mtot]"""
    return g.block().cpu().reshape(c.n, c.Mtot, c.HW).permute(0, 2, 1).reshape(c.M, c.Mtot)


@pytest.mark.parametrize("yt", DTYPES)
@pytest.mark.parametrize("training", [True, False])
def test_fwd_q_tiled_equals_element(tmae, training, yt):
    """the same 288 x 32 element values as three images of 96 pixels (the LDS tile) and as one image of 288 pixels
    (288 x 17 floats > 4800: one element per thread), one step for all: bit for bit the same outputs"""
    a, b = tk.tile_cases()
    _, oa = launch_fwd(tmae, a, training, yt, a.q)
    _, ob = launch_fwd(tmae, b, training, yt, b.q)
    assert oa.lik.guard_hits() == 0 and ob.lik.guard_hits() == 0
    la, lb = _rows(a, oa.lik), _rows(b, ob.lik)
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert not bool(torch.equal(la[:, a.sl], a.lik0[:, a.sl]))  # written
    _same(oa.yhat, ob.yhat, "yhat")
    _same(oa.yhat32, ob.yhat32, "yhat32")


def test_fwd_q_other_bound_and_bad_q(tmae):
    """the bound is the kernel's argument, applied to sigma / delta; q of the wrong length or type launches nothing"""
    c = tk.fwd_case("tiled2")
    inp, o = launch_fwd(tmae, c, False, F32, c.q, bound=0.25)
    out, _ = qk.reference("tiled2", qk.Q3, 0.25)
    gk.check("gc_slices_fwd_q:bound0.25:lik", o.lik, *out["lik"])
    o2 = ek.gcf_outputs(c, F32, False, DEV, True)
    args = (inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, None, o2.lik.view(), c.Mtot, o2.yhat.view(),
            F32, o2.yhat.ld, o2.yhat32.view(), o2.yhat32.ld, c.n, c.HW, c.nsl, c.sw, 0.11)
    with pytest.raises(ValueError, match=r"q holds 2 entries for 3 images"):
        tmae.ops.gc_slices_fwd_q(*args, qdev((0, 1)))
    with pytest.raises(ValueError, match=r"q must be torch.int32"):
        tmae.ops.gc_slices_fwd_q(*args, torch.zeros(3, dtype=torch.int64, device=DEV))
    sync()
    ek.check_bits("untouched", o2.yhat, c.yh0)


# ------------------------------------------------------------------------------------ tmae_gc_bwd_q
GCQ_CASES = [(s, tr, dt, "full") for s in tk.GCQ_SHAPES for tr in (True, False) for dt in DTYPES]
GCQ_CASES += [("three_wg", tr, F32, v) for tr in (True, False) for v in ("no_glik", "no_gyp")]


@pytest.mark.parametrize("shape,training,dtype,variant", GCQ_CASES)
def test_gc_bwd_q(T, shape, training, dtype, variant):
    """small: 135 elements, part of one workgroup; three_wg: 528 elements, three workgroups, the last ragged; three
    images at q = (-32, 0, 11), sigma planted on both sides of bound x delta in each.  ldy = Mtot + 8, ld_ms = sw + 3,
    ldg = Mtot + 3, lddy = Mtot + 16, ldd = sw + 16"""
    c = tk.gcq_case(shape)
    use_glik, use_gyp = variant != "no_glik", variant != "no_gyp"
    out, skip, a, f = tk.gcq_bwd_reference(c, training, dtype, use_glik, use_gyp)
    assert float(skip.any.double().mean()) <= gk.SKIP_CAP
    dy, dmu, dsig = (Guarded(c.M, c.Mtot, F32, device=DEV, init=c.dy0), Guarded(c.M, c.sw, dtype, device=DEV),
                     Guarded(c.M, c.sw, dtype, device=DEV))
    assert len({c.ldy, c.ld_ms, c.ldg, dy.ld, dmu.ld}) == 5
    T.gc_bwd_q(dev(gk.pad(c.y, c.ldy)), c.ldy, c.yoff, dev(gk.pad(c.mu, c.ld_ms)), dev(gk.pad(c.sigma, c.ld_ms)), c.ld_ms,
               dev(c.noise) if training else None, c.Mtot, dev(c.glik) if use_glik else None,
               dev(gk.pad(c.gyp, c.ldg)) if use_gyp else None, c.ldg, dy.view(), dy.ld, dmu.view(), dsig.view(), dmu.ld,
               c.n, c.HW, c.sw, dtype, tk.BOUND, qdev(c.q))
    sync()
    tag = f"gc_bwd_q:{shape}:{'train' if training else 'eval'}:{variant}"
    gk.check(f"{tag}:dy", dy, *out["dy"])
    gk.check(f"{tag}:dmu", dmu, *out["dmu"])
    gk.check(f"{tag}:dsigma", dsig, *out["dsigma"])
    if not training:  # the eval likelihood moves neither y nor mu
        assert float(dmu.result().abs().max()) == 0.0


# ------------------------------------------------------------------------------------ tmae_lic_stack's chain with cq
def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_slab(a, b):
    return bool((_bits(a.buf) == _bits(b.buf)).all())


def _st(nb2, per):
    return (nb2 * per, per)


@pytest.mark.parametrize("case", cc.CHAIN, ids=lambda c: c.name)
def test_lic_stack_chain_at_a_step(tmae, case):
    """test_gpu_lic_conv.test_lic_stack_chain_bitwise's chained cases (12 x 12 and 9 x 9 grids, two slices batched
    through the cs_* strides) with three images at q = (-32, 0, 11): csrc (y_hat_pre) bit for bit the restatement of
    the launch's own f32 mu; y, cy and cy2 bit for bit the unchained sequence mean / scale stacks,
    tmae_gc_slices_fwd_q, lrp stacks"""
    ops = tmae.ops
    assert cc.N_IMG == 3
    g = torch.Generator().manual_seed(case.G * 100 + case.c1 + 7)
    G, nb2, sw, rows = case.G, case.nb2, case.couts[-1], cc.N_IMG * case.G * case.G
    HW = G * G
    P = 2 * nb2
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    q = qdev(tk.Q3)
    delta = np.repeat(np.array(tk.deltas(tk.Q3), dtype=np.float32), HW).reshape(rows, 1)

    def layers(nprob, chans):
        ws = [(rn(nprob, co, ci, 3, 3) / (3.0 * ci ** 0.5)).to(BF16) for ci, co in zip(chans[:-1], chans[1:])]
        pk = [torch.stack([ops.pack_lic_stack_weight(w[p]) for p in range(nprob)]).to(DEV) for w in ws]
        return pk, [dev(rn(nprob, co) * 0.5) for co in chans[1:]]

    x1 = dev(rn(P, rows, case.c1).to(BF16))
    pk, bs = layers(P, (case.c1,) + case.couts)
    cpk, cbs = layers(nb2, (case.cc1 + sw,) + case.ccouts)
    cx1 = dev(rn(nb2, rows, case.cc1).to(BF16))
    ldyv, ld_cadd = sw + 8, case.ccouts[0] + 12
    # y in units of each image's step, so that every image has symbols other than 0
    yv = dev(rn(nb2, rows, ldyv) * 3.0 * torch.from_numpy(delta))
    cadd = dev(rn(nb2, rows, ld_cadd) * 0.5)
    st = {"x1": _st(nb2, rows * case.c1)}
    for l, co in enumerate(case.couts):
        st[f"w{l}"], st[f"b{l}"] = _st(nb2, pk[l][0].numel()), _st(nb2, co)

    def slabs():
        return (cc.Slab(P, rows, sw, torch.float32, device=DEV), cc.Slab(nb2, rows, sw, torch.float32, device=DEV),
                cc.Slab(nb2, rows, sw, BF16, device=DEV), cc.Slab(nb2, rows, sw, BF16, device=DEV))

    def mean_scale(y, chain=None):
        ops.lic_stack(cc.N_IMG, G, x1, case.c1, case.c1, pk, bs, list(case.couts), y.ptr(), y.ld, True, nb=(2, nb2),
                      strides=dict(st, y=y.strides(nb2)), chain=chain)
        sync()

    def chain_args(ypre, cy, cy2, **extra):
        cs = {"x1": rows * case.cc1, "y": rows * ldyv, "ypre": ypre.per, "add": rows * ld_cadd, "out": cy.per,
              "out2": cy2.per}
        for l, co in enumerate(case.ccouts):
            cs[f"w{l}"], cs[f"b{l}"] = cpk[l][0].numel(), co
        return dict({"couts": list(case.ccouts), "w": cpk, "b": cbs, "x1": cx1, "c1": case.cc1, "ld1": case.cc1,
                     "y": yv, "ldy": ldyv, "add": cadd, "ld_add": ld_cadd, "ypre": ypre.ptr(), "ld_ypre": ypre.ld,
                     "out": cy.ptr(), "ld_out": cy.ld, "out2": cy2.ptr(), "ld_out2": cy2.ld, "strides": cs}, **extra)

    # chained, at the step
    y, ypre, cy, cy2 = slabs()
    mean_scale(y, chain=chain_args(ypre, cy, cy2, q=q))
    # 1. y_hat_pre is the restatement of the kernel's own mu
    nonzero = 0
    for b2 in range(nb2):
        mu = y.block(b2).cpu().numpy()
        r = tk.restate_fwd(yv[b2, :, :sw].cpu().numpy(), mu, np.ones_like(mu), None, delta)
        got = ypre.block(b2).cpu()
        assert torch.equal(got.view(torch.int32), torch.from_numpy(r.yhat).view(torch.int32)), f"y_hat_pre of slice {b2}"
        nonzero += int((r.qi != 0).sum())
        for b in range(cc.N_IMG):  # every image rounds to something other than zero somewhere
            assert int((r.qi[b * HW:(b + 1) * HW] != 0).sum()) > 0
    assert ypre.guard_hits() == 0
    # 2. the unchained sequence: mean / scale stacks, tmae_gc_slices_fwd_q (y_hat_pre in bf16 and f32), lrp stacks
    y_u, ypre_u, cy_u, cy2_u = slabs()
    mean_scale(y_u)
    assert _same_slab(y, y_u), "the chain's mean / scale outputs differ from the plain launch's"
    x2 = torch.full((nb2, rows, sw), float("nan"), dtype=BF16, device=DEV)
    lik = torch.empty(cc.N_IMG * sw * HW, device=DEV)
    sigma1 = torch.ones(rows, y_u.ld, device=DEV)  # read through mu's leading dimension; only the likelihood uses it
    for b2 in range(nb2):
        ops.gc_slices_fwd_q(yv[b2], ldyv, 0, y_u.ptr(b2), sigma1, 0, y_u.ld, None, lik, sw, x2[b2], BF16, sw,
                            ypre_u.ptr(b2), ypre_u.ld, cc.N_IMG, HW, 1, sw, 0.11, q)
    sync()
    assert _same_slab(ypre, ypre_u), "y_hat_pre differs from tmae_gc_slices_fwd_q's"
    st2 = {"x1": _st(nb2, rows * case.cc1), "x2": _st(nb2, rows * sw), "a": _st(nb2, rows * ld_cadd),
           "src": ypre_u.strides(nb2), "y": cy_u.strides(nb2), "y2": cy2_u.strides(nb2)}
    for l, co in enumerate(case.ccouts):
        st2[f"w{l}"], st2[f"b{l}"] = _st(nb2, cpk[l][0].numel()), _st(nb2, co)
    ops.lic_stack(cc.N_IMG, G, cx1, case.cc1, case.cc1, cpk, cbs, list(case.ccouts), cy_u.ptr(), cy_u.ld, False, x2=x2,
                  c2=sw, ld2=sw, addend=cadd, ld_add=ld_cadd, lrp_src=ypre_u.ptr(), ld_src=ypre_u.ld, y2=cy2_u.ptr(),
                  ldy2=cy2_u.ld, nb=(1, nb2), strides=st2)
    sync()
    for name, a, b in (("cy", cy, cy_u), ("cy2", cy2, cy2_u)):
        assert not torch.isnan(a.block(0).float()).any(), f"chain: {name} was not written"
        assert _same_slab(a, b), f"chain: {name} differs from the unchained launches (or a guard was written)"
        assert a.guard_hits() == 0 and b.guard_hits() == 0
    # 3. the step matters: the plain chain on the same operands gives another y_hat_pre
    y0, ypre0, cy0, cy20 = slabs()
    mean_scale(y0, chain=chain_args(ypre0, cy0, cy20))
    assert _same_slab(y, y0) and not _same_slab(ypre, ypre0)


def test_lic_stack_rejects_cq_without_chain(tmae):
    """cq needs TMAE_LIC_STACK_CHAIN, and the backward launch takes none"""
    from textmae_amd import _lib

    ops = tmae.ops
    G, n, c1 = 4, 3, 32
    rows = n * G * G
    w = ops.pack_lic_stack_weight(torch.randn(32, c1, 3, 3).to(BF16)).to(DEV)
    x = torch.zeros(rows, c1, dtype=BF16, device=DEV)
    y = torch.full((rows, 32), 7.0, device=DEV)
    a = _lib.LicStackArgs()
    a.n, a.G, a.nb1, a.nb2, a.nlayers = n, G, 1, 1, 1
    a.x1, a.c1, a.ld1 = x.data_ptr(), c1, c1
    a.w[0], a.bias[0], a.cout[0] = w.data_ptr(), torch.zeros(32, device=DEV).data_ptr(), 32
    a.y, a.y_f32, a.ldy = y.data_ptr(), 1, 32
    a.cq = qdev((0, 1, 2)).data_ptr()
    import ctypes

    for flags in (0, 2):
        a.flags = flags
        with pytest.raises(ValueError, match=r"cq \(the chain's quantiser step\) needs TMAE_LIC_STACK_CHAIN"):
            _lib.call("tmae_lic_stack", ctypes.byref(a), ops._stream())
    sync()
    assert float((y - 7.0).abs().max()) == 0.0  # nothing was launched
