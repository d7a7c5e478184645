"""The LDS-resident LIC convolutions, element by element: tmae_lic_stack (forward layer by layer, chained, backward),
tmae_lic_latent (csrc/lic_stack.hip) and conv_halo_kernel (csrc/conv_halo.h through ops.conv3x3) against the float64
references and derived per-element bounds of tests/conv_check.py (read its docstring for the derivation; the cases
are its shared table, which tests/test_conv_checker.py also runs through an f32 restatement on the CPU).

* lic_stack forward: the training launch (save=) writes every hidden layer's pre-activation and GELU output; layer l
  is checked against the float64 conv of the launch's OWN sv_act[l - 1], so no error compounds and no element of any
  layer is skipped.  The inference launch (no save) must give bit-identical y / y2.
* lic_stack chained: y, the y_hat_pre copy, cy and cy2 bitwise equal to two unchained launches with
  y_hat_pre = round(y - mu) + mu computed by torch in f32 from the first launch's mu.
* lic_stack backward: the reversed channel lists, layer by layer through outs, with and without the routed f32
  accumulators (three ranges with limits that are multiples of 4 but not of 16, three problems at one stride, prior
  contents kept, padding bit-identical).
* lic_latent: every cin = 32 k, fragments [2, 5) of two 3-fragment blocks (a pair straddling the blocks, a lone last
  fragment), two problems; the bias / GELU / bf16 forms and the 12 x 12 and 7 x 7 grids at k = 3, 7, 12.
* halo conv: ops.conv3x3 on bf16 12 x 12 stride-1 problems, which conv.hip conv_go sends to conv_halo_kernel when
  conv_halo_ok(H, W, stride, N, nb) = H == 12 && W == 12 && stride == 1 && N <= 2048 && nb <= 12 holds (restated as
  conv_check.conv_halo_ok; asserted per case), one pass per epilogue over Cin in {8, 64, 40 + 32, 200},
  N in {4, 36, 64, 72, 224}, n in {1, 3}.
Every output sits in NaN-filled slabs with guard rows and columns; the weights carry non-zero values in the padded
input channels, so the kernels' zeroing of the activation padding is part of what is checked.

Measured on an MI355X (largest error / bound per kernel and epilogue over all cases, problems and elements; the
assertion is <= 1 against the derived bound, never against these):

    kernel / epilogue                                   f32 outputs                  bf16 outputs
    lic_stack forward, hidden layer l = 0 / 1 / 2 / 3                               sv_pre 0.996 / 0.871 / 0.818 / 0.842
                                                                                    sv_act 0.991 / 0.824 / 0.841 / 0.824
    lic_stack forward, last layer                       y 0.002, sv_t 0.003          plain y 0.611, lrp y = y2 0.967
    lic_stack chained                                   bitwise                      bitwise
    lic_stack backward, layer k = 0 / 1 / 2 / 3         routes 0.001 / 0.001 / 0.001 outs 0.977 / 0.952 / 0.837 / 0.770
    lic_latent                                          plain 0.002, bias 0.001      bias + GELU 0.811
    halo conv                                           f32 0.006, GELU 0.001,       store 0.940, pre 0.940, GELU 0.946,
                                                        y32 0.009, lrp pre 0.007     addend 0.964, shuffle 0.937 (pre
                                                                                     0.911), lrp y = y2 0.974

Every f32 output uses under 1 % of its bound: e = (K + 2) u S is an any-order worst case and the kernels' sums behave
far better.  Every figure above 0.9 is a bf16 store, and there the bf16 store term 2^-8 |ref| dominates the bound
(the linear and GELU terms are one hundredth of it): a value just above a power of two rounds by up to half an ulp,
which is exactly that term, so over 10^5 elements the ratio approaches 1 for a CORRECT kernel (the f32 CPU
restatement of tests/test_conv_checker.py reaches 0.996 on the same case).  The largest, 0.996, is sv_pre of layer 0
with an empty input: bf16(bias + addend), nothing but the store's rounding.

75 cases (conv_check.all_case_names: 10 forward, 2 chained, 8 backward, 24 lic_latent, 31 halo) in 76 tests, 273
per-problem ratios; 3.2 s for the module.  No kernel was found wrong.
"""
import pytest
import torch

import conv_check as cc
from conv_check import BF16, N_IMG

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAUNCHED = set()  # names of the shared table's cases this module launched


def dev(t):
    return t.to(DEV)


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return bool((_bits(a.buf) == _bits(b.buf)).all())


def _st(nb2, per):
    return (nb2 * per, per)


# ------------------------------------------------------------------------------------ lic_stack forward
def _launch_stack(ops, pr, o, packed, save):
    c, nb2, rows = pr.case, pr.case.nb[1], pr.rows
    st = {"x1": _st(nb2, rows * pr.ld1), "x2": _st(nb2, rows * pr.ld2), "y": o.y.strides(nb2)}
    for l, co in enumerate(c.couts):
        st[f"w{l}"] = _st(nb2, packed[l][0].numel())
        st[f"b{l}"] = _st(nb2, co)
    kw = {}
    if pr.add is not None:
        st["a"] = _st(nb2, rows * pr.ld_add)
        kw.update(addend=dev(pr.add), ld_add=pr.ld_add)
    if c.epi == "lrp":
        st["src"], st["y2"] = _st(nb2, rows * pr.ld_src), o.y2.strides(nb2)
        kw.update(lrp_src=dev(pr.src), ld_src=pr.ld_src, y2=o.y2.ptr(), ldy2=o.y2.ld)
    if save:
        sv = {"layers": [(p.ptr(), a.ptr(), p.strides(nb2)) for p, a in zip(o.pre, o.act)]}
        if o.t is not None:
            sv.update(t=o.t.ptr(), t_s=o.t.strides(nb2))
        kw["save"] = sv
    ops.lic_stack(N_IMG, c.G, dev(pr.x1), c.c1, pr.ld1, packed, [dev(b) for b in pr.b], list(c.couts), o.y.ptr(),
                  o.y.ld, c.epi == "f32", x2=dev(pr.x2) if c.c2 else None, c2=c.c2, ld2=pr.ld2, nb=c.nb, strides=st,
                  **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", cc.STACK_FWD, ids=lambda c: c.name)
def test_lic_stack_forward_layers(tmae, case):
    ops = tmae.ops
    assert ops.lic_stack_fits(case.G, case.c1 + case.c2, list(case.couts))
    pr = cc.stack_problem(case)
    packed = [torch.stack([ops.pack_lic_stack_weight(torch.cat([w[p], t[p]], dim=1)) for p in range(pr.P)]).to(DEV)
              for w, t in zip(pr.w, pr.wtail)]
    o = cc.stack_outputs(pr, DEV)
    _launch_stack(ops, pr, o, packed, save=True)
    LAUNCHED.add("fwd:" + case.name)
    cc.check_stack_fwd(pr, o, log=True).ok()
    # the inference launch: the same y (and y2), bit for bit, guards included
    oi = cc.stack_outputs(pr, DEV, save=False)
    _launch_stack(ops, pr, oi, packed, save=False)
    assert _same_bits(o.y, oi.y), "inference y differs from the training launch's"
    if o.y2 is not None:
        assert _same_bits(o.y2, oi.y2), "inference y2 differs from the training launch's"


# ------------------------------------------------------------------------------------ lic_stack chained
@pytest.mark.parametrize("case", cc.CHAIN, ids=lambda c: c.name)
def test_lic_stack_chain_bitwise(tmae, case):
    """TMAE_LIC_STACK_CHAIN (the mean problem's workgroups go on with the slice's lrp stack) against the mean / scale
    launch, torch's round(y - mu) + mu in f32, and the lrp launch on it.  Those unchained launches are the ones
    test_lic_stack_forward_layers checks per element."""
    ops = tmae.ops
    g = torch.Generator().manual_seed(case.G * 100 + case.c1)
    G, nb2, sw, rows = case.G, case.nb2, case.couts[-1], N_IMG * case.G * case.G
    P = 2 * nb2
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731

    def layers(nprob, chans):
        ws = [(rn(nprob, co, ci, 3, 3) / (3.0 * ci ** 0.5)).to(BF16) for ci, co in zip(chans[:-1], chans[1:])]
        pk = [torch.stack([ops.pack_lic_stack_weight(w[p]) for p in range(nprob)]).to(DEV) for w in ws]
        return pk, [dev(rn(nprob, co) * 0.5) for co in chans[1:]]

    x1 = dev(rn(P, rows, case.c1).to(BF16))
    pk, bs = layers(P, (case.c1,) + case.couts)
    cpk, cbs = layers(nb2, (case.cc1 + sw,) + case.ccouts)
    cx1 = dev(rn(nb2, rows, case.cc1).to(BF16))
    ldyv, ld_cadd = sw + 8, case.ccouts[0] + 12
    yv, cadd = dev(rn(nb2, rows, ldyv) * 3.0), dev(rn(nb2, rows, ld_cadd) * 0.5)
    st = {"x1": _st(nb2, rows * case.c1)}
    for l, co in enumerate(case.couts):
        st[f"w{l}"], st[f"b{l}"] = _st(nb2, pk[l][0].numel()), _st(nb2, co)

    def slabs():
        return (cc.Slab(P, rows, sw, torch.float32, device=DEV), cc.Slab(nb2, rows, sw, torch.float32, device=DEV),
                cc.Slab(nb2, rows, sw, BF16, device=DEV), cc.Slab(nb2, rows, sw, BF16, device=DEV))

    def mean_scale(y, chain=None):
        ops.lic_stack(N_IMG, G, x1, case.c1, case.c1, pk, bs, list(case.couts), y.ptr(), y.ld, True, nb=(2, nb2),
                      strides=dict(st, y=y.strides(nb2)), chain=chain)
        torch.cuda.synchronize()

    # chained
    y, ypre, cy, cy2 = slabs()
    cs = {"x1": rows * case.cc1, "y": rows * ldyv, "ypre": ypre.per, "add": rows * ld_cadd, "out": cy.per,
          "out2": cy2.per}
    for l, co in enumerate(case.ccouts):
        cs[f"w{l}"], cs[f"b{l}"] = cpk[l][0].numel(), co
    mean_scale(y, chain={"couts": list(case.ccouts), "w": cpk, "b": cbs, "x1": cx1, "c1": case.cc1, "ld1": case.cc1,
                         "y": yv, "ldy": ldyv, "add": cadd, "ld_add": ld_cadd, "ypre": ypre.ptr(), "ld_ypre": ypre.ld,
                         "out": cy.ptr(), "ld_out": cy.ld, "out2": cy2.ptr(), "ld_out2": cy2.ld, "strides": cs})
    LAUNCHED.add("chain:" + case.name)
    # unchained: mean / scale, torch's y_hat_pre, lrp
    y_u, ypre_u, cy_u, cy2_u = slabs()
    mean_scale(y_u)
    for b2 in range(nb2):
        mu = y_u.block(b2)  # problem (0, b2): the slice's mean stack
        ypre_u.block(b2)[...] = torch.round(yv[b2, :, :sw] - mu) + mu
    x2 = torch.stack([ypre_u.block(b2).to(BF16) for b2 in range(nb2)]).contiguous()
    st2 = {"x1": _st(nb2, rows * case.cc1), "x2": _st(nb2, rows * sw), "a": _st(nb2, rows * ld_cadd),
           "src": ypre_u.strides(nb2), "y": cy_u.strides(nb2), "y2": cy2_u.strides(nb2)}
    for l, co in enumerate(case.ccouts):
        st2[f"w{l}"], st2[f"b{l}"] = _st(nb2, cpk[l][0].numel()), _st(nb2, co)
    ops.lic_stack(N_IMG, G, cx1, case.cc1, case.cc1, cpk, cbs, list(case.ccouts), cy_u.ptr(), cy_u.ld, False, x2=x2,
                  c2=sw, ld2=sw, addend=cadd, ld_add=ld_cadd, lrp_src=ypre_u.ptr(), ld_src=ypre_u.ld, y2=cy2_u.ptr(),
                  ldy2=cy2_u.ld, nb=(1, nb2), strides=st2)
    torch.cuda.synchronize()
    for name, a, b in (("y", y, y_u), ("y_hat_pre", ypre, ypre_u), ("cy", cy, cy_u), ("cy2", cy2, cy2_u)):
        assert not torch.isnan(a.block(0).float()).any(), f"chain: {name} was not written"
        assert _same_bits(a, b), f"chain: {name} differs from the unchained launches (or a guard was written)"
        assert a.guard_hits() == 0 and b.guard_hits() == 0


# ------------------------------------------------------------------------------------ lic_stack backward
@pytest.mark.parametrize("case", cc.STACK_BWD, ids=lambda c: c.name)
def test_lic_stack_backward_layers(tmae, case):
    ops = tmae.ops
    pr = cc.bwd_problem(case)
    ch, nb2, rows, R = case.chans, case.nb[1], pr.rows, cc.Slab.GR
    o = cc.bwd_outputs(pr, DEV)
    wpk, couts, pres, st = [], [], [], {"x1": _st(nb2, rows * ch[pr.L])}
    keep = []
    for k in range(pr.nk):
        fw = pr.L - 1 - k
        wpk.append(torch.stack([ops.pack_lic_stack_weight_t(torch.cat([pr.w[fw][p], pr.wtail[fw][p]], dim=0))
                                for p in range(pr.P)]).to(DEV))
        couts.append(ch[fw])
        st[f"w{k}"] = _st(nb2, wpk[k][0].numel())
        if k < pr.L - 1:
            pre = dev(pr.pres[fw - 1])
            keep.append(pre)
            pres.append(pre.data_ptr() + 2 * R * ch[fw])  # rows R .. of problem 0: the same stride as outs[k]
            st[f"s{k}"] = o.outs[k].strides(nb2)
            assert o.outs[k].per == pre[0].numel()
    routes = [[(s.ptr(p), s.ld, nc) for s, nc in zip(o.acc, case.routes)] for p in range(pr.P)] if case.routes else None
    ops.lic_stack_bwd(N_IMG, case.G, dev(pr.dtop), ch[pr.L], ch[pr.L], wpk, couts, pres, [s.ptr() for s in o.outs],
                      nb=case.nb, strides=st, routes=routes)
    torch.cuda.synchronize()
    LAUNCHED.add("bwd:" + case.name)
    cc.check_stack_bwd(pr, o, log=True).ok()


# ------------------------------------------------------------------------------------ lic_latent
@pytest.mark.parametrize("case", cc.LATENT, ids=lambda c: c.name)
def test_lic_latent(tmae, case):
    ops = tmae.ops
    pr = cc.latent_problem(case)
    assert ops.lic_latent_fits(case.G, pr.cin)
    wpk = torch.stack([ops.pack_lic_stack_weight(pr.w[b]) for b in range(4)]).contiguous().to(DEV)
    y = cc.latent_outputs(pr, DEV)
    xs = [dev(pr.x[p]) for p in range(2)]
    ops.lic_latent(cc.LAT_N, case.G, xs, pr.ldx, pr.cin, wpk, cc.LAT_NFR, wpk[0].numel(), pr.f_off, cc.LAT_FLO,
                   cc.LAT_FHI, y.ptr(), y.ld, y_s=[0, y.per],
                   biases=[dev(pr.bias[p]) for p in range(2)] if pr.bias is not None else None,
                   act=ops.ACT_GELU if case.form == "gelu_bf16" else ops.ACT_NONE, y_bf16=case.form == "gelu_bf16")
    torch.cuda.synchronize()
    LAUNCHED.add("latent:" + case.name)
    cc.check_latent(pr, y, log=True).ok()


# ------------------------------------------------------------------------------------ halo conv
@pytest.mark.parametrize("case", cc.HALO, ids=lambda c: c.name)
def test_conv_halo(tmae, case):
    ops = tmae.ops
    assert cc.conv_halo_ok(12, 12, 1, case.N, case.nb[0] * case.nb[1])
    pr = cc.halo_problem(case)
    o = cc.halo_outputs(pr, DEV)
    nb2, N, K = case.nb[1], case.N, 9 * pr.cin
    st = {"w": _st(nb2, N * K), "b": _st(nb2, N), "y": o.y.strides(nb2)}
    kw = {}
    e = case.epi
    if e == "bf16_y32_pre":
        kw.update(y32=o.y32.ptr(), ld32=o.y32.ld, pre=o.pre.ptr(), ldp=o.pre.ld)
    elif e in ("gelu", "gelu_f32"):
        kw.update(act=ops.ACT_GELU)
    elif e == "addend":
        st["a"] = _st(nb2, pr.rows * pr.ld_add)
        kw.update(addend=dev(pr.add), ld_add=pr.ld_add)
    elif e == "shuffle":
        assert o.pre.ld == o.y.ld
        kw.update(act=ops.ACT_GELU, pixel_shuffle=True, pre=o.pre.ptr(), ldp=o.pre.ld)
    elif e == "lrp":
        kw.update(lrp_src=dev(pr.src), ld_src=pr.ld_src, y2=o.y2.ptr(), ldy2=o.y2.ld, pre=o.pre.ptr(), ldp=o.pre.ld)
    ops.conv3x3(dev(pr.x1), case.c1, pr.ld1, case.n, 12, 12, dev(cc.halo_packed_weight(pr)), dev(pr.b), o.y.ptr(),
                o.y.ld, N, BF16, y_f32=e in ("f32", "gelu_f32"), x2=dev(pr.x2) if case.c2 else None, c2=case.c2,
                ld2=pr.ld2, nb=case.nb, strides=st, **kw)
    torch.cuda.synchronize()
    LAUNCHED.add("halo:" + case.name)
    cc.check_halo(pr, o, log=True).ok()


# ------------------------------------------------------------------------------------ coverage (keep last)
def test_every_case_was_launched(tmae):
    """the module launched every case of the shared table (whose reach over the kernels' instantiations
    tests/test_conv_checker.py::test_census asserts on the CPU)"""
    want = set(cc.all_case_names())
    assert LAUNCHED == want, (sorted(want - LAUNCHED), sorted(LAUNCHED - want))
