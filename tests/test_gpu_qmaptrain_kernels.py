"""The kernels of training at a quantiser step per kept patch element by element: tmae_gc_bwd_qm
(csrc/gc_bwd_qm.hip) and tmae_lic_stack's chain with cqm (csrc/lic_stack_qm.hip), against tests/qmaptrain_check.py
(checked on the CPU by tests/test_qmaptrain_host.py).  On the parent commit the symbol tmae_gc_bwd_qm and the field cqm
do not exist: every test here fails there.

Three images whose pixels cycle through qmap_check.CYCLES = (-32, 32, 0, 11, -5), (-13, 3, 26, 0), (7).
* tmae_gc_bwd_qm: qtrain_check.GCQ_SHAPES (135 elements, part of one workgroup; 528, three workgroups, the last
  ragged: the launch shapes tmae_gc_bwd_q is tested in; like it the kernel has one launch form, one element per
  thread), both output dtypes, training and eval, with and without glik / gyp, against float64 autograd with the
  kernel's formula carried through E; a map constant over each image bit for bit tmae_gc_bwd_q at q = that constant.
* the chain with cqm: test_gpu_qtrain_kernels' chained cases (12 x 12 and 9 x 9 grids): y_hat_pre bit for bit the
  restatement of the launch's own f32 mu at each element's own step, cy / cy2 bit for bit the unchained sequence mean
  stack, tmae_gc_slices_fwd_qm, lrp stack; a constant map bit for bit the cq launch; the three rejections."""
import ctypes

import numpy as np
import pytest
import torch

import conv_check as cc
import glue_check as gk
import qmap_check as mk
import qmaptrain_check as mt
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


def idev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(DEV)


def sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ tmae_gc_bwd_qm
def _launch_bwd(fn, c, training, dtype, use_glik, use_gyp, *tail):
    dy, dmu, dsig = (Guarded(c.M, c.Mtot, F32, device=DEV, init=c.dy0), Guarded(c.M, c.sw, dtype, device=DEV),
                     Guarded(c.M, c.sw, dtype, device=DEV))
    assert len({c.ldy, c.ld_ms, c.ldg, dy.ld, dmu.ld}) == 5
    fn(dev(gk.pad(c.y, c.ldy)), c.ldy, c.yoff, dev(gk.pad(c.mu, c.ld_ms)), dev(gk.pad(c.sigma, c.ld_ms)), c.ld_ms,
       dev(c.noise) if training else None, c.Mtot, dev(c.glik) if use_glik else None,
       dev(gk.pad(c.gyp, c.ldg)) if use_gyp else None, c.ldg, dy.view(), dy.ld, dmu.view(), dsig.view(), dmu.ld,
       c.n, c.HW, c.sw, dtype, tk.BOUND, *tail)
    sync()
    return dy, dmu, dsig


GCQM_CASES = [(s, tr, dt, "full") for s in mt.GCQ_SHAPES for tr in (True, False) for dt in DTYPES]
GCQM_CASES += [("three_wg", tr, F32, v) for tr in (True, False) for v in ("no_glik", "no_gyp")]


@pytest.mark.parametrize("shape,training,dtype,variant", GCQM_CASES)
def test_gc_bwd_qm(T, shape, training, dtype, variant):
    """ldy = Mtot + 8, ld_ms = sw + 3, ldg = Mtot + 3, lddy = Mtot + 16, ldd = sw + 16; the largest error / bound of
    every output goes to the parity log (glue_check.check -> parity_log)"""
    c = mt.gcqm_case(shape)
    use_glik, use_gyp = variant != "no_glik", variant != "no_gyp"
    out, skip, a, f = tk.gcq_bwd_reference(c, training, dtype, use_glik, use_gyp)
    assert float(skip.any.double().mean()) <= gk.SKIP_CAP
    dy, dmu, dsig = _launch_bwd(T.gc_bwd_qm, c, training, dtype, use_glik, use_gyp, idev(c.qmap))
    tag = f"gc_bwd_qm:{shape}:{'train' if training else 'eval'}:{variant}"
    gk.check(f"{tag}:dy", dy, *out["dy"])
    gk.check(f"{tag}:dmu", dmu, *out["dmu"])
    gk.check(f"{tag}:dsigma", dsig, *out["dsigma"])
    if not training:  # the eval likelihood moves neither y nor mu
        assert float(dmu.result().abs().max()) == 0.0


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", list(mt.GCQ_SHAPES))
def test_gc_bwd_qm_constant_map_is_gc_bwd_q(T, shape, training, dtype):
    """qmap[b][.] = q[b]: every output buffer, guards included, bit for bit tmae_gc_bwd_q's"""
    c = mt.gcqm_case(shape, constant=tk.Q3)
    got = _launch_bwd(T.gc_bwd_qm, c, training, dtype, True, True, idev(c.qmap))
    want = _launch_bwd(T.gc_bwd_q, c, training, dtype, True, True, idev(np.array(tk.Q3)))
    for name, g, w in zip(("dy", "dmu", "dsigma"), got, want):
        assert g.guard_hits() == 0 and w.guard_hits() == 0, name
        assert torch.equal(_bits(g.buf.cpu()), _bits(w.buf.cpu())), name
    assert not torch.equal(got[0].result(), c.dy0.double())  # written


def test_gc_bwd_qm_needs_its_map(T):
    c = mt.gcqm_case("small")
    with pytest.raises(ValueError, match=r"qmap is required"):
        _launch_bwd(T.gc_bwd_qm, c, True, F32, True, True, None)
    with pytest.raises(ValueError, match=r"qmap holds 3 entries for 3 images of 9 pixels"):
        _launch_bwd(T.gc_bwd_qm, c, True, F32, True, True, idev(np.zeros(3)))


# ------------------------------------------------------------------------------------ tmae_lic_stack's chain with cqm
def _same_slab(a, b):
    return bool((_bits(a.buf) == _bits(b.buf)).all())


def _st(nb2, per):
    return (nb2 * per, per)


@pytest.mark.parametrize("case", cc.CHAIN, ids=lambda c: c.name)
def test_lic_stack_chain_at_a_map(tmae, case):
    """test_gpu_qtrain_kernels.test_lic_stack_chain_at_a_step with the step per pixel: csrc (y_hat_pre) bit for bit the
    restatement of the launch's own f32 mu at each element's own step; y, cy and cy2 bit for bit the unchained sequence
    mean / scale stacks, tmae_gc_slices_fwd_qm, lrp stacks; a constant map bit for bit the cq launch"""
    ops = tmae.ops
    assert cc.N_IMG == 3
    g = torch.Generator().manual_seed(case.G * 100 + case.c1 + 7)
    G, nb2, sw, rows = case.G, case.nb2, case.couts[-1], cc.N_IMG * case.G * case.G
    HW = G * G
    P = 2 * nb2
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    qmap_h = mk.qmap_of(HW)
    assert len(set(qmap_h[0].tolist())) == 5 and HW % 5 and G % 5  # image 0's step follows neither row nor column
    qmap = idev(qmap_h)
    delta = mk.steps(qmap_h).reshape(rows, 1)

    def layers(nprob, chans):
        ws = [(rn(nprob, co, ci, 3, 3) / (3.0 * ci ** 0.5)).to(BF16) for ci, co in zip(chans[:-1], chans[1:])]
        pk = [torch.stack([ops.pack_lic_stack_weight(w[p]) for p in range(nprob)]).to(DEV) for w in ws]
        return pk, [dev(rn(nprob, co) * 0.5) for co in chans[1:]]

    x1 = dev(rn(P, rows, case.c1).to(BF16))
    pk, bs = layers(P, (case.c1,) + case.couts)
    cpk, cbs = layers(nb2, (case.cc1 + sw,) + case.ccouts)
    cx1 = dev(rn(nb2, rows, case.cc1).to(BF16))
    ldyv, ld_cadd = sw + 8, case.ccouts[0] + 12
    # y in units of each pixel's step, so that every step has symbols other than 0
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

    # chained, at the map
    y, ypre, cy, cy2 = slabs()
    mean_scale(y, chain=chain_args(ypre, cy, cy2, qm=qmap))
    # 1. y_hat_pre is the restatement of the kernel's own mu, every element at its own pixel's step
    for b2 in range(nb2):
        mu = y.block(b2).cpu().numpy()
        r = tk.restate_fwd(yv[b2, :, :sw].cpu().numpy(), mu, np.ones_like(mu), None, delta)
        got = ypre.block(b2).cpu()
        assert torch.equal(got.view(torch.int32), torch.from_numpy(r.yhat).view(torch.int32)), f"y_hat_pre of slice {b2}"
        for b in range(cc.N_IMG):  # every position of every image's cycle rounds to something other than zero
            for v in set(qmap_h[b].tolist()):
                at = b * HW + np.flatnonzero(qmap_h[b] == v)
                assert int((r.qi[at] != 0).sum()) > 0, (b, v)
    assert ypre.guard_hits() == 0
    # 2. the unchained sequence: mean / scale stacks, tmae_gc_slices_fwd_qm (y_hat_pre in bf16 and f32), lrp stacks
    y_u, ypre_u, cy_u, cy2_u = slabs()
    mean_scale(y_u)
    assert _same_slab(y, y_u), "the chain's mean / scale outputs differ from the plain launch's"
    x2 = torch.full((nb2, rows, sw), float("nan"), dtype=BF16, device=DEV)
    lik = torch.empty(cc.N_IMG * sw * HW, device=DEV)
    sigma1 = torch.ones(rows, y_u.ld, device=DEV)  # read through mu's leading dimension; only the likelihood uses it
    for b2 in range(nb2):
        ops.gc_slices_fwd_qm(yv[b2], ldyv, 0, y_u.ptr(b2), sigma1, 0, y_u.ld, None, lik, sw, x2[b2], BF16, sw,
                             ypre_u.ptr(b2), ypre_u.ld, cc.N_IMG, HW, 1, sw, 0.11, qmap)
    sync()
    assert _same_slab(ypre, ypre_u), "y_hat_pre differs from tmae_gc_slices_fwd_qm's"
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
    # 3. a map constant over each image is the cq launch, bit for bit; and the varying map is not
    q3 = np.array(tk.Q3, dtype=np.int32)
    a4, b4 = slabs(), slabs()
    mean_scale(a4[0], chain=chain_args(*a4[1:], qm=idev(np.repeat(q3[:, None], HW, axis=1))))
    mean_scale(b4[0], chain=chain_args(*b4[1:], q=idev(q3)))
    for u, v in zip(a4, b4):
        assert _same_slab(u, v)
    assert _same_slab(y, a4[0]) and not _same_slab(ypre, a4[1])


def test_lic_stack_rejects_cqm_combinations(tmae):
    """cqm with cq, with TMAE_LIC_STACK_BWD and without TMAE_LIC_STACK_CHAIN: each its own message, nothing launched"""
    from textmae_amd import _lib

    ops = tmae.ops
    G, n, c1 = 4, 3, 32
    rows = n * G * G
    w = ops.pack_lic_stack_weight(torch.randn(32, c1, 3, 3).to(BF16)).to(DEV)
    x = torch.zeros(rows, c1, dtype=BF16, device=DEV)
    y = torch.full((rows, 32), 7.0, device=DEV)
    bias = torch.zeros(32, device=DEV)
    qm, q = idev(np.zeros((n, G * G))), idev(np.zeros(n))

    def args(flags, cq):
        a = _lib.LicStackArgs()
        a.n, a.G, a.nb1, a.nb2, a.nlayers = n, G, 1, 1, 1
        a.x1, a.c1, a.ld1 = x.data_ptr(), c1, c1
        a.w[0], a.bias[0], a.cout[0] = w.data_ptr(), bias.data_ptr(), 32
        a.y, a.y_f32, a.ldy = y.data_ptr(), 1, 32
        a.cqm = qm.data_ptr()
        a.cq = q.data_ptr() if cq else None
        a.flags = flags
        return a

    for a, msg in ((args(1, True), r"cqm \(a step per pixel\) and cq \(a step per image\) exclude each other"),
                   (args(2, False), r"cqm \(the chain's quantiser steps per pixel\) takes no TMAE_LIC_STACK_BWD"),
                   (args(0, False), r"cqm \(the chain's quantiser steps per pixel\) needs TMAE_LIC_STACK_CHAIN")):
        with pytest.raises(ValueError, match=msg):
            _lib.call("tmae_lic_stack", ctypes.byref(a), ops._stream())
    sync()
    assert float((y - 7.0).abs().max()) == 0.0  # nothing was launched
