"""tests/conv_check.py checked on the CPU.

* A plain torch f32 restatement of every operation (bf16-rounded operands, f32 arithmetic, round-to-nearest bf16
  stores) must fit its bound on EVERY case of the shared table, the ones tests/test_gpu_lic_conv.py launches: that
  is what makes the bounds usable.  The restatement keeps the kernels' padded layout: activations padded to 32
  channels, weights with non-zero values in the padded input channels (conv_check's wtail).
* Ten faults, each injected into that restatement at the small 9 x 9 case (halo faults at a 36-channel case), must be
  rejected: a ratio above 1 or a guard hit.
* The old verdict (max |a - b| / max |b| of the last output against 6e-3) is evaluated for every fault and printed;
  conv_check's docstring records the figures.  The old verdict lets through fault 1 (5.4e-3 <= 6e-3), fault 3 (with the
  zero-padded weights the old tests packed it changes no output at all) and fault 10 (no guards); fault 7 sits at the
  limit (6.2e-3: over 6e-3, under the 7e-3 of the old lds-conv test).  A record, not an assertion.
* The census: the restated dispatch of lic_stack / lic_latent reaches every instantiation over the shared table.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_check as cc
from conv_check import BF16, pad32

OLD_MAXREL = 6e-3
FAULTS = {
    1: "one 8-channel piece of one tap dropped at one border pixel (hidden layer)",
    2: "a tap outside the grid reads the wrapped neighbour: pixel (y, G-1), dx = +1 reads (y+1, 0)",
    3: "the channel padding [cout, pad32(cout)) of a hidden layer holds the previous layer's values",
    4: "the x1 | x2 segment boundary is off by 8 channels",
    5: "a lone last fragment (odd fragment count) takes its neighbour's bias",
    6: "the layer-0 addend is skipped for the last pixel fragment",
    7: "a hidden activation is truncated to bf16 instead of rounded",
    8: "GELU' is taken from pre of the neighbouring problem",
    9: "the last image of an odd batch is never written",
    10: "four columns are written past cout",
}


def bf(t):
    return t.to(BF16).float()


def conv_f32(xp, wp, G, fault=None):
    """tap by tap in f32: xp [rows][cp], wp [cout][cp][3][3]"""
    rows, cp = xp.shape
    n = rows // (G * G)
    hp = F.pad(xp.view(n, G, G, cp), (0, 0, 1, 1, 1, 1))
    acc = torch.zeros(n, G, G, wp.shape[0])
    for t in range(9):
        acc = acc + hp[:, t // 3:t // 3 + G, t % 3:t % 3 + G] @ wp[:, :, t // 3, t % 3].t()
    if fault == 1 and G > 1:   # pixel (0, G-1) of image 0 loses channels 8..15 of tap (dy, dx) = (+1, 0)
        acc[0, 0, G - 1] -= hp[0, 2, G, 8:16] @ wp[:, 8:16, 2, 1].t()
    if fault == 2 and G > 1:   # pixel (0, G-1), tap (0, +1): (1, 0) instead of the zero outside the grid
        acc[0, 0, G - 1] += hp[0, 2, 1] @ wp[:, :, 1, 2].t()
    return acc.view(rows, -1)


def trunc_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def restate_stack_fwd(pr, fault=None, fault_layer=None):
    c, o = pr.case, cc.stack_outputs(pr)
    nl, G = len(c.couts), c.G
    for p in range(pr.P):
        xin = torch.zeros(pr.rows, pad32(pr.cin0))
        c1 = c.c1 - 8 if fault == 4 else c.c1
        xin[:, :c1] = pr.x1[p, :, :c1].float()
        xin[:, c1:pr.cin0] = pr.x2[p, :, :pr.cin0 - c1].float()
        for l in range(nl):
            cout, here = c.couts[l], fault_layer == l
            wp = torch.cat([pr.w[l][p], pr.wtail[l][p]], dim=1).float()
            v = conv_f32(xin, wp, G, fault if here else None) if wp.shape[1] else torch.zeros(pr.rows, cout)
            if l == 0 and pr.add is not None:
                add = pr.add[p, :, :cout].clone()
                if fault == 6:
                    add.view(cc.N_IMG, G * G, cout)[:, 16 * ((G * G - 1) // 16):] = 0.0
                v = v + add
            b = pr.b[l][p].clone()
            if fault == 5 and here:
                nfr = -(-cout // 16)
                assert nfr % 2 == 1 and nfr >= 9
                b[16 * (nfr - 1):] = b[16 * (nfr - 2):16 * (nfr - 2) + cout - 16 * (nfr - 1)]
            v = v + b
            if l + 1 < nl:
                act = F.gelu(v)
                o.pre[l].block(p)[...] = v.to(BF16)
                o.act[l].block(p)[...] = trunc_bf16(act).to(BF16) if fault == 7 and here else act.to(BF16)
                nxt = torch.zeros(pr.rows, pad32(cout))
                if fault == 3 and here:
                    nxt[:, cout:] = xin[:, cout:pad32(cout)]  # what the buffer held before
                nxt[:, :cout] = o.act[l].block(p).float()
                xin = nxt
            else:
                rows = slice(0, pr.rows - G * G) if fault == 9 else slice(None)
                if c.epi == "lrp":
                    r = pr.src[p, :, :cout] + 0.5 * torch.tanh(v)
                    o.t.block(p)[rows] = v[rows]
                    o.y.block(p)[rows] = r.to(BF16)[rows]
                    o.y2.block(p)[rows] = r.to(BF16)[rows]
                else:
                    o.y.block(p)[rows] = v.to(o.y.buf.dtype)[rows]
                if fault == 10:
                    R, C = o.y.GR, o.y.GC
                    o.y.buf[p, R:R + pr.rows, C + cout:C + cout + 4] = 1.0
    return o


def gelu_grad_f32(x):
    return 0.5 * (1.0 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5


def restate_stack_bwd(pr, fault=None):
    c, o, R = pr.case, cc.bwd_outputs(pr), cc.Slab.GR
    n, G = cc.N_IMG, c.G
    for p in range(pr.P):
        d = pr.dtop[p].float()
        for k in range(pr.nk):
            fw = pr.L - 1 - k
            wext = torch.cat([pr.w[fw][p], pr.wtail[fw][p]], dim=0).float()
            dp = torch.zeros(pr.rows, wext.shape[0])
            dp[:, :d.shape[1]] = d
            h = dp.view(n, G, G, -1).permute(0, 3, 1, 2)
            a = F.conv_transpose2d(h, wext, padding=1).permute(0, 2, 3, 1).reshape(pr.rows, -1)
            if k < pr.L - 1:
                q = (p ^ 1) % pr.P if fault == 8 and k == 0 else p
                out = (a * gelu_grad_f32(pr.pres[fw - 1][q, R:R + pr.rows].float())).to(BF16)
                o.outs[k].block(p)[...] = out
                d = out.float()
            else:
                c0 = 0
                for r, nc in enumerate(c.routes):
                    o.acc[r].block(p)[...] += a[:, c0:c0 + nc]
                    c0 += nc
    return o


def restate_latent(pr):
    c, y = pr.case, cc.latent_outputs(pr)
    lo, hi = 16 * cc.LAT_FLO, 16 * cc.LAT_FHI
    for p in range(2):
        w = torch.cat([pr.w[2 * p], pr.w[2 * p + 1]], dim=0)[lo:hi].float()
        v = conv_f32(pr.x[p, :, :pr.cin].float(), w, c.G)
        if pr.bias is not None:
            v = v + pr.bias[p, lo:hi]
        if c.form == "gelu_bf16":
            v = F.gelu(v)
        y.block(p)[:, lo:hi] = v.to(y.buf.dtype)
    return y


def restate_halo(pr, fault=None):
    c, o = pr.case, cc.halo_outputs(pr)
    x = torch.cat([pr.x1[:, :c.c1], pr.x2[:, :c.c2]], dim=1).float()
    keep = slice(0, pr.rows - 144) if fault == 9 else slice(None)

    def put(slab, p, t):
        slab.block(p)[keep] = t.to(slab.buf.dtype)[keep]

    for p in range(pr.P):
        v = conv_f32(x, pr.w[p].float(), 12) + pr.b[p]
        if pr.add is not None:
            v = v + pr.add[p, :, :c.N]
        if c.epi == "bf16_y32_pre":
            put(o.y, p, v), put(o.y32, p, v), put(o.pre, p, v)
        elif c.epi in ("f32", "addend"):
            put(o.y, p, v)
        elif c.epi in ("gelu", "gelu_f32"):
            put(o.y, p, F.gelu(v))
        elif c.epi == "shuffle":
            vs = cc.shuffle2(v, c.n, 12)
            put(o.pre, p, vs), put(o.y, p, F.gelu(vs))
        else:
            r = pr.src[p, :, :c.N] + 0.5 * torch.tanh(v)
            put(o.y, p, r), put(o.y2, p, r), put(o.pre, p, v)
        if fault == 10:
            R, C = o.y.GR, o.y.GC
            o.y.buf[p, R:R + pr.rows, C + c.N:C + c.N + 4] = 1.0
    return o


# ------------------------------------------------------------------------------------ the restatement fits
@pytest.mark.parametrize("case", cc.STACK_FWD, ids=lambda c: c.name)
def test_stack_fwd_restatement_fits(case):
    pr = cc.stack_problem(case)
    v = cc.check_stack_fwd(pr, restate_stack_fwd(pr))
    print(case.name, v.by_kind())
    v.ok()


@pytest.mark.parametrize("case", cc.STACK_BWD, ids=lambda c: c.name)
def test_stack_bwd_restatement_fits(case):
    pr = cc.bwd_problem(case)
    v = cc.check_stack_bwd(pr, restate_stack_bwd(pr))
    print(case.name, v.by_kind())
    v.ok()


@pytest.mark.parametrize("case", cc.LATENT, ids=lambda c: c.name)
def test_latent_restatement_fits(case):
    pr = cc.latent_problem(case)
    cc.check_latent(pr, restate_latent(pr)).ok()


@pytest.mark.parametrize("case", cc.HALO, ids=lambda c: c.name)
def test_halo_restatement_fits(case):
    pr = cc.halo_problem(case)
    cc.check_halo(pr, restate_halo(pr)).ok()


def test_chain_cases_are_stack_cases():
    """the chained launch is compared bitwise with unchained launches of the same kernel; its shapes must be ones the
    stack accepts (multiples of 8, resident widths)"""
    for c in cc.CHAIN:
        assert c.couts[-1] == c.ccouts[-1] and all(x % 8 == 0 for x in c.couts + c.ccouts + (c.c1, c.cc1))
        assert pad32(c.cc1 + c.ccouts[-1]) <= 224 and c.G * c.G <= 144


# ------------------------------------------------------------------------------------ the faults
G9 = next(c for c in cc.STACK_FWD if c.name == "g9")
G9_BWD = next(c for c in cc.STACK_BWD if c.name == "g9")
HALO36 = next(c for c in cc.HALO if c.name == "f32_64_36_3")
FAULT_LAYER = {1: 1, 2: 1, 3: 1, 5: 0, 7: 0}  # g9 is 64 -> 136 -> 40 -> 8: 136 = 9 fragments (odd), pad32(40) = 64


def _maxrel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _run_fault(k):
    """(conv_check's verdict, the old metric's value) of fault k"""
    if k == 8:
        pr = cc.bwd_problem(G9_BWD)
        good, bad = restate_stack_bwd(pr), restate_stack_bwd(pr, fault=8)
        old = max(_maxrel(b.result(p), g.result(p)) for g, b in zip(good.outs, bad.outs) for p in range(pr.P))
        return cc.check_stack_bwd(pr, bad), old
    if k in (9, 10):
        pr = cc.halo_problem(HALO36)
        good, bad = restate_halo(pr), restate_halo(pr, fault=k)
        return cc.check_halo(pr, bad), _maxrel(bad.y.result(0), good.y.result(0))
    pr = cc.stack_problem(G9)
    good, bad = restate_stack_fwd(pr), restate_stack_fwd(pr, fault=k, fault_layer=FAULT_LAYER.get(k))
    return cc.check_stack_fwd(pr, bad), _maxrel(bad.y.result(0), good.y.result(0))


@pytest.mark.parametrize("k", sorted(FAULTS))
def test_fault_is_rejected(k):
    v, old = _run_fault(k)
    print(f"fault {k:2d}: worst ratio {v.worst():.3g}, guard hits {v.hits()}; old max-rel {old:.2e} "
          f"({'passes' if old <= OLD_MAXREL else 'fails'} {OLD_MAXREL:g})  -- {FAULTS[k]}")
    assert v.rejected(), FAULTS[k]


def test_stale_padding_needs_nonzero_tail_weights():
    """fault 3 with the library's zero-padded weights changes no output at all: only the non-zero tail weights of the
    shared problems make it visible"""
    pr = cc.stack_problem(G9)
    saved = pr.wtail
    try:
        pr.wtail = [torch.zeros_like(t) for t in saved]
        assert not cc.check_stack_fwd(pr, restate_stack_fwd(pr, fault=3, fault_layer=1)).rejected()
    finally:
        pr.wtail = saved


# ------------------------------------------------------------------------------------ census
def test_census():
    every = {(2, 9), (2, 5), (2, 4), (1, 5), (1, 4)}
    fwd_pairs, fwd_nkc, bwd_pairs, bwd_nkc = set(), set(), set(), set()
    odd_nf2 = cout8 = ragged_halves = ragged_whole = False
    for c in cc.STACK_FWD:
        chans = (c.c1 + c.c2,) + tuple(c.couts)
        npix = c.G * c.G
        for ci, co in zip(chans[:-1], chans[1:]):
            pairs, nkc, nfr = cc.stack_items(c.G, ci, co)
            fwd_pairs |= pairs
            fwd_nkc.add(nkc)
            odd_nf2 |= nfr % 2 == 1 and (2, 9) in pairs or nfr % 2 == 1 and (2, 5) in pairs
            cout8 |= co % 16 == 8
        ragged_halves |= npix % 16 != 0 and -(-npix // 16) > 5
        ragged_whole |= npix % 16 != 0 and -(-npix // 16) <= 5
    for c in cc.STACK_BWD:
        L = len(c.chans) - 1
        for k in range(L - 1 + (1 if c.routes else 0)):
            fw = L - 1 - k
            pairs, nkc, _ = cc.stack_items(c.G, c.chans[fw + 1], c.chans[fw])
            bwd_pairs |= pairs
            bwd_nkc.add(nkc)
    assert fwd_pairs == every and bwd_pairs == every
    assert fwd_nkc == set(range(0, 8)) and bwd_nkc == set(range(1, 8))
    assert odd_nf2 and cout8 and ragged_halves and ragged_whole
    assert {len(c.couts) for c in cc.STACK_FWD} >= {1, 2, 5}
    assert {c.epi for c in cc.STACK_FWD if len(c.couts) == 1} == {"f32", "bf16", "lrp"}
    assert {c.k for c in cc.LATENT} == set(range(1, 13))
    assert {cc.latent_ring(c.k) for c in cc.LATENT} == {1, 2, 3, 4, 5, 7}
    assert [cc.latent_ring(k) for k in range(1, 13)] == [1, 2, 3, 4, 5, 3, 7, 4, 3, 2, 1, 4]
    for c in cc.HALO:
        assert cc.conv_halo_ok(12, 12, 1, c.N, c.nb[0] * c.nb[1])
    assert {c.N % 8 for c in cc.HALO} == {0, 4} and min(c.N for c in cc.HALO) < 64
    assert {c.c1 + c.c2 for c in cc.HALO} == {8, 64, 72, 200} and {c.n for c in cc.HALO} == {1, 3}
    names = cc.all_case_names()
    assert len(names) == len(set(names))
