"""The kernels of the per-patch quantiser steps against tests/qmap_check.py and the numpy
restatements of bitstream.py.

tmae_qlevels_select / pack / unpack and tmae_qmap_build (csrc/qlevels.hip): integers and comparisons only, so equality.
(K, L) = (16, 64), (144, 256), (5, 64) for tail bits, (1024, 1024); nlev = 2 / 3 / 4 / 16; planted equal and non-finite
scores, the invalid level 3 at nlev = 3, non-zero tail bits, mixed per-image nlev with nlev = 1 among them.

tmae_gc_slices_code_qm / indexes_qm / dequantize_qm / slices_fwd_qm (csrc/coding_qmap.hip) on qstep_check.SHAPES with
three images whose pixels cycle through the ladder positions of qmap_check.CYCLES: symbols, indexes and both y_hat
outputs bit for bit the restatement's, the likelihood within entropy_check's E bound, no element skipped; the LDS form
against the element form on the same elements; a map that is constant per image against the _q kernels, bitwise."""
import numpy as np
import pytest
import torch

import entropy_check as ek
import glue_check as gk
import qmap_check as mk
import qstep_check as qk
from glue_check import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEOMETRIES = [(16, 64), (144, 256), (5, 64), (1024, 1024)]
NLEVS = [2, 3, 4, 16]


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def tname(dt):
    return "bf16" if dt == BF16 else "f32"


def perms(n, L, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(L) for _ in range(n)]).astype(np.int64)


@pytest.fixture(scope="module")
def bs(tmae):
    from textmae_amd import bitstream

    return bitstream


# ------------------------------------------------------------------------------------------------ csrc/qlevels.hip
def planted_scores(n, L, seed):
    rng = np.random.default_rng(seed)
    s = rng.random((n, L)).astype(np.float32)
    s[1] = np.round(s[1] * 4) / 4  # ties
    s[2] = 0.5                     # all equal
    s[3, ::3] = np.nan
    s[3, 1::7] = np.inf
    s[3, 2::11] = -np.inf
    s[3, 5::13] = -0.0
    return s


@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("K,L", GEOMETRIES)
def test_select_from_scores(tmae, bs, K, L, nlev):
    ids, s = perms(5, L, K + nlev), planted_scores(5, L, K * 7 + nlev)
    want, _ = bs.select_levels_host(ids, K, nlev, scores=s)
    got, st = tmae.ops.qlevels_select(torch.from_numpy(ids).to(DEV), K, nlev, scores=torch.from_numpy(s).to(DEV))
    assert got.dtype == torch.int32 and tuple(got.shape) == (5, K)
    assert np.array_equal(got.cpu().numpy(), want)
    assert not st.cpu().numpy().any()
    assert int(got.min()) >= 0 and int(got.max()) <= nlev - 1  # the non-finite rows included


@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("K,L", GEOMETRIES)
def test_select_from_a_map(tmae, bs, K, L, nlev):
    ids = perms(4, L, K + 3 * nlev)
    m = np.random.default_rng(K + nlev).integers(0, nlev, (4, L)).astype(np.int32)
    m[1, ids[1, K // 2]] = nlev          # at nlev = 3: the invalid level 3, in a kept patch of image 1
    m[2, ids[2, K - 1]] = -1
    if K < L:
        m[3, ids[3, K]] = 99             # not kept: never read
    want, wst = bs.select_levels_host(ids, K, nlev, level_map=m)
    assert wst.tolist() == [0, 1, 1, 0]
    got, st = tmae.ops.qlevels_select(torch.from_numpy(ids).to(DEV), K, nlev, level_map=torch.from_numpy(m).to(DEV))
    assert np.array_equal(st.cpu().numpy(), wst)
    got = got.cpu().numpy()
    assert np.array_equal(got, want)
    assert not got[1].any() and not got[2].any()  # a faulted image: zero levels; the others untouched
    assert np.array_equal(got[0], m[0][ids[0, :K]]) and np.array_equal(got[3], m[3][ids[3, :K]])


@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("K,L", GEOMETRIES)
def test_pack_unpack_build(tmae, bs, K, L, nlev):
    n = 6
    rng = np.random.default_rng(K * 3 + nlev)
    lv = rng.integers(0, nlev, (n, K)).astype(np.int32)
    lv[0, -1] = nlev - 1
    want = bs.pack_levels_host(lv, nlev)
    words = tmae.ops.qlevels_pack(torch.from_numpy(lv).to(DEV), nlev)
    assert tuple(words.shape) == (n, bs.level_words(K, nlev))
    assert np.array_equal(words.cpu().numpy().view(np.uint32), want)
    # unpack: rows padded to a wider common ldw, per-image tables, faults planted
    lbits, W2 = bs.level_bits(nlev), bs.level_words(K, nlev)
    ldw = W2 + 1
    w = np.full((n, ldw), 0xDEADBEEF, dtype=np.uint32)  # the padding past an image's own words is never read
    w[:, :W2] = want
    nl = np.array([nlev, 1, nlev, nlev, 2, nlev], dtype=np.int32)
    w[1] = 0xFFFFFFFF                                   # nlev = 1: no map, nothing read
    lv2 = rng.integers(0, 2, K).astype(np.int32)        # image 4 has a table of its own
    w[4] = 0xDEADBEEF
    w[4, :bs.level_words(K, 2)] = bs.pack_levels_host(lv2, 2)
    tail = (K * lbits) % 32
    if nlev < (1 << lbits):                             # a level >= nlev can be written: image 2
        k = K // 2
        bit = k * lbits
        w[2, bit // 32] |= np.uint32(((1 << lbits) - 1) << (bit % 32) & 0xFFFFFFFF)
        if bit % 32 + lbits > 32:
            w[2, bit // 32 + 1] |= np.uint32(((1 << lbits) - 1) >> (32 - bit % 32))
    if tail:                                            # non-zero tail bits: image 3
        w[3, W2 - 1] |= np.uint32(1 << 31)
    want_lv, want_st = bs.unpack_levels_host(w, nl, K)
    assert want_st[2] == (1 if nlev < (1 << lbits) else 0) and want_st[3] == (2 if tail else 0)
    assert want_st[[0, 1, 4, 5]].tolist() == [0, 0, 0, 0]
    got, st = tmae.ops.qlevels_unpack(torch.from_numpy(w.view(np.int32)).to(DEV), torch.from_numpy(nl).to(DEV), K)
    got, st = got.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(st, want_st) and np.array_equal(got, want_lv)
    assert np.array_equal(got[0], lv[0]) and np.array_equal(got[5], lv[5]) and np.array_equal(got[4], lv2)
    assert not got[1].any()
    for b in (2, 3):
        assert (not got[b].any()) if want_st[b] else np.array_equal(got[b], lv[b])
    # build: saturation at both ends
    offs = rng.integers(-64, 65, (n, 16)).astype(np.int32)
    offs[0, :2] = (-64, 64)
    q = np.array([30, -30, 0, 32, -32, 5], dtype=np.int32)
    qm = tmae.ops.qmap_build(torch.from_numpy(lv).to(DEV), torch.from_numpy(q).to(DEV), torch.from_numpy(offs).to(DEV))
    wantq = bs.build_qmap_host(lv, q, offs)
    assert np.array_equal(qm.cpu().numpy(), wantq) and wantq.min() == -32 and wantq.max() == 32
    qm0 = tmae.ops.qmap_build(torch.from_numpy(lv).to(DEV), None, torch.from_numpy(offs).to(DEV))
    assert np.array_equal(qm0.cpu().numpy(), bs.build_qmap_host(lv, None, offs))


def test_unpack_both_faults_lowest_wins(tmae, bs):
    K, nlev = 5, 3
    lv = np.array([[0, 1, 2, 1, 0]] * 3, dtype=np.int32)
    w = bs.pack_levels_host(lv, nlev).copy()
    w[1, 0] |= np.uint32((3 << 0) | (1 << 31))
    w[2, 0] |= np.uint32(1 << 10)  # the first tail bit
    got, st = tmae.ops.qlevels_unpack(torch.from_numpy(w.view(np.int32)).to(DEV),
                                      torch.full((3,), nlev, dtype=torch.int32, device=DEV), K)
    assert st.cpu().tolist() == [0, 1, 2]
    assert np.array_equal(got.cpu().numpy(), bs.unpack_levels_host(w, nlev, K)[0])
    # a row narrower than the image's table needs: a fault, and nothing is read
    got, st = tmae.ops.qlevels_unpack(torch.zeros((1, 1), dtype=torch.int32, device=DEV),
                                      torch.tensor([16], dtype=torch.int32, device=DEV), 16)
    assert st.cpu().tolist() == [1] and not got.cpu().numpy().any()


def test_wrapper_errors_before_any_launch(tmae):
    ids = torch.from_numpy(perms(2, 64, 1)).to(DEV)
    s = torch.rand(2, 64, device=DEV)
    with pytest.raises(ValueError, match=r"nlev = 17 outside 2\.\.16"):
        tmae.ops.qlevels_select(ids, 16, 17, scores=s)
    with pytest.raises(ValueError, match=r"exactly one"):
        tmae.ops.qlevels_select(ids, 16, 4)
    with pytest.raises(ValueError, match=r"exactly one"):
        tmae.ops.qlevels_select(ids, 16, 4, scores=s, level_map=torch.zeros(2, 64, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match=r"need 1 <= K=65 <= L=64"):
        tmae.ops.qlevels_select(ids, 65, 4, scores=s)
    with pytest.raises(ValueError, match=r"offsets must be \[2, 16\]"):
        tmae.ops.qmap_build(torch.zeros(2, 16, dtype=torch.int32, device=DEV), None,
                            torch.zeros(2, 4, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------------------------------------ csrc/coding_qmap.hip
def launch(tmae, c, yt, qmap, yhat32=True, lik=True, fwd=False):
    inp = ek.gcf_inputs(c, False, DEV)
    o = ek.gcf_outputs(c, yt, True, DEV, yhat32)
    y32, ld32 = (o.yhat32.view(), o.yhat32.ld) if yhat32 else (None, 0)
    qm = torch.from_numpy(np.ascontiguousarray(qmap, dtype=np.int32)).to(DEV)
    if fwd:
        tmae.ops.gc_slices_fwd_qm(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, None, o.lik.view(),
                                  c.Mtot, o.yhat.view(), yt, o.yhat.ld, y32, ld32, c.n, c.HW, c.nsl, c.sw, 0.11, qm)
    else:
        tmae.ops.gc_slices_code_qm(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms,
                                   o.lik.view() if lik else None, c.Mtot, o.yhat.view(), yt, o.yhat.ld, y32, ld32, c.n,
                                   c.HW, c.nsl, c.sw, o.sym.view(), o.idx.view(), dev(c.table), 0.11, qm)
    torch.cuda.synchronize()
    return inp, o, qm


def check_outputs(tag, c, o, out, yt, yhat32, lik, code=True):
    if code:
        ek.check_exact(f"{tag}:symbols", o.sym, out["sym"])
        ek.check_exact(f"{tag}:indexes", o.idx, out["idx"])
    ek.check_bits(f"{tag}:yhat", o.yhat, qk.yhat_values(c, out, yt))
    if yhat32:
        ek.check_bits(f"{tag}:yhat32", o.yhat32, out["yhat32"])
    if lik:
        gk.check(f"{tag}:lik", o.lik, *out["lik"])  # every element, entropy_check's E bound
    else:  # NULL: nothing of the buffer the test holds was written
        ek.check_bits(f"{tag}:lik_untouched", o.lik, ek.to_nchw(c.lik0, c.n, c.HW).reshape(1, -1))


@pytest.mark.parametrize("lik", [True, False])
@pytest.mark.parametrize("yhat32", [True, False])
@pytest.mark.parametrize("yt", [F32, BF16])
@pytest.mark.parametrize("shape", list(mk.SHAPES))
def test_code_qm_against_restatement(tmae, shape, yt, yhat32, lik):
    c = mk.case(shape)
    out, _ = mk.reference(shape)
    inp, o, qm = launch(tmae, c, yt, c.qmap, yhat32, lik)
    check_outputs(f"gc_slices_code_qm:{shape}:{tname(yt)}", c, o, out, yt, yhat32, lik)
    total = c.nsl * c.M * c.sw
    # the decoder's two kernels: the same indexes from sigma, the same y_hat from the symbols
    idx = ek.GuardedInt(1, total, device=DEV)
    tmae.ops.gc_indexes_qm(inp.sigma, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, dev(c.table), 0.11, idx.view(), qm)
    d = ek.gcf_outputs(c, yt, False, DEV, yhat32)
    y32, ld32 = (d.yhat32.view(), d.yhat32.ld) if yhat32 else (None, 0)
    tmae.ops.gc_dequantize_qm(o.sym.view(), inp.mu, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, c.yoff,
                              d.yhat.view(), yt, d.yhat.ld, y32, ld32, qm)
    torch.cuda.synchronize()
    ek.check_exact(f"gc_indexes_qm:{shape}", idx, out["idx"])
    ek.check_bits(f"gc_dequantize_qm:{shape}:yhat:{tname(yt)}", d.yhat, qk.yhat_values(c, out, yt))
    assert torch.equal(d.yhat.block().cpu(), o.yhat.block().cpu())  # bitwise, bf16 included
    if yhat32:
        ek.check_bits(f"gc_dequantize_qm:{shape}:yhat32", d.yhat32, out["yhat32"])
        assert torch.equal(d.yhat32.block().cpu(), o.yhat32.block().cpu())


@pytest.mark.parametrize("yhat32", [True, False])
@pytest.mark.parametrize("yt", [F32, BF16])
@pytest.mark.parametrize("shape", list(mk.SHAPES))
def test_fwd_qm_is_the_coders_arithmetic(tmae, shape, yt, yhat32):
    """eval forward: y_hat the restatement's, the likelihood within the E bound and bit for bit the coding kernel's"""
    c = mk.case(shape)
    out, _ = mk.reference(shape)
    _, f, _ = launch(tmae, c, yt, c.qmap, yhat32, True, fwd=True)
    check_outputs(f"gc_slices_fwd_qm:{shape}:{tname(yt)}", c, f, out, yt, yhat32, True, code=False)
    _, o, _ = launch(tmae, c, yt, c.qmap, yhat32, True)
    assert torch.equal(f.lik.block().cpu(), o.lik.block().cpu())
    assert torch.equal(f.yhat.block().cpu(), o.yhat.block().cpu())


@pytest.mark.parametrize("yt", [F32, BF16])
def test_lds_form_against_element_form(tmae, yt):
    """the rows of element2 (3 images of HW = 324: past the LDS bound, one element per thread) coded again as 9 images of
    HW = 108 (the LDS form): inputs, map and row-major outputs are indexed by the row alone, the coder order and the
    NCHW likelihood are put back into rows; everything equal bit for bit"""
    c = mk.case("element2")
    d = mk.regrouped(c, 9, 108)
    assert d.HW * (d.sw + 1) <= 4800 < c.HW * (c.sw + 1)
    for fwd in (False, True):
        _, a, _ = launch(tmae, c, yt, c.qmap, fwd=fwd)
        _, b, _ = launch(tmae, d, yt, c.qmap.reshape(9, 108), fwd=fwd)
        for name in ("yhat", "yhat32"):
            x, y = getattr(a, name), getattr(b, name)
            assert x.guard_hits() == 0 and y.guard_hits() == 0, name
            assert torch.equal(x.block().cpu().view(torch.int32 if name == "yhat32" or yt == F32 else torch.int16),
                               y.block().cpu().view(torch.int32 if name == "yhat32" or yt == F32 else torch.int16)), name
        la = mk.lik_by_row(c, a.lik.block().cpu().reshape(-1))
        lb = mk.lik_by_row(d, b.lik.block().cpu().reshape(-1))
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
        if not fwd:
            for name in ("sym", "idx"):
                assert torch.equal(mk.by_row(c, getattr(a, name).result().reshape(-1)),
                                   mk.by_row(d, getattr(b, name).result().reshape(-1))), name


@pytest.mark.parametrize("yt", [F32, BF16])
@pytest.mark.parametrize("shape", ["tiled2", "tiled6", "element2"])
def test_constant_map_is_the_q_kernels(tmae, shape, yt):
    """qmap[b][.] = q[b]: every output of the four kernels bitwise the _q namesake's at q (the likelihood included)"""
    c = qk.case(shape)  # per-image steps q = (-32, 0, 11)
    qmap = np.repeat(np.array(c.q, dtype=np.int32)[:, None], c.HW, axis=1)
    qd = torch.tensor(c.q, dtype=torch.int32, device=DEV)
    inp, new, qm = launch(tmae, c, yt, qmap)
    _, fnew, _ = launch(tmae, c, yt, qmap, fwd=True)
    old, fold = ek.gcf_outputs(c, yt, True, DEV, True), ek.gcf_outputs(c, yt, True, DEV, True)
    tmae.ops.gc_slices_code_q(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, old.lik.view(), c.Mtot,
                              old.yhat.view(), yt, old.yhat.ld, old.yhat32.view(), old.yhat32.ld, c.n, c.HW, c.nsl,
                              c.sw, old.sym.view(), old.idx.view(), dev(c.table), 0.11, qd)
    tmae.ops.gc_slices_fwd_q(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, None, fold.lik.view(),
                             c.Mtot, fold.yhat.view(), yt, fold.yhat.ld, fold.yhat32.view(), fold.yhat32.ld, c.n, c.HW,
                             c.nsl, c.sw, 0.11, qd)
    total = c.nsl * c.M * c.sw
    idx_old, idx_new = ek.GuardedInt(1, total, device=DEV), ek.GuardedInt(1, total, device=DEV)
    tmae.ops.gc_indexes_q(inp.sigma, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, dev(c.table), 0.11, idx_old.view(),
                          qd)
    tmae.ops.gc_indexes_qm(inp.sigma, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, dev(c.table), 0.11, idx_new.view(),
                           qm)
    d_old, d_new = ek.gcf_outputs(c, yt, False, DEV), ek.gcf_outputs(c, yt, False, DEV)
    tmae.ops.gc_dequantize_q(old.sym.view(), inp.mu, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, c.yoff,
                             d_old.yhat.view(), yt, d_old.yhat.ld, d_old.yhat32.view(), d_old.yhat32.ld, qd)
    tmae.ops.gc_dequantize_qm(new.sym.view(), inp.mu, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, c.yoff,
                              d_new.yhat.view(), yt, d_new.yhat.ld, d_new.yhat32.view(), d_new.yhat32.ld, qm)
    torch.cuda.synchronize()
    for name, a, b in (("symbols", new.sym, old.sym), ("indexes", new.idx, old.idx), ("yhat", new.yhat, old.yhat),
                       ("yhat32", new.yhat32, old.yhat32), ("lik", new.lik, old.lik), ("fwd yhat", fnew.yhat, fold.yhat),
                       ("fwd yhat32", fnew.yhat32, fold.yhat32), ("fwd lik", fnew.lik, fold.lik),
                       ("gc_indexes", idx_new, idx_old), ("dequantize yhat", d_new.yhat, d_old.yhat),
                       ("dequantize yhat32", d_new.yhat32, d_old.yhat32)):
        assert a.guard_hits() == 0 and b.guard_hits() == 0, name
        assert torch.equal(a.block().cpu(), b.block().cpu()), name


def test_qmap_required_and_checked(tmae):
    c = mk.case("tiled1")
    inp = ek.gcf_inputs(c, False, DEV)
    idx = ek.GuardedInt(1, c.nsl * c.M * c.sw, device=DEV)
    args = (inp.sigma, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, dev(c.table), 0.11, idx.view())
    with pytest.raises(ValueError, match=r"qmap is required"):
        tmae.ops.gc_indexes_qm(*args, None)
    with pytest.raises(ValueError, match=r"qmap holds 32 entries for 3 images of 16 pixels"):
        tmae.ops.gc_indexes_qm(*args, torch.zeros(2, 16, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match=r"qmap must be torch.int32"):
        tmae.ops.gc_indexes_qm(*args, torch.zeros(3, 16, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    assert idx.guard_hits() == 0 and int((idx.block() != ek.SENTINEL).sum()) == 0  # nothing was launched
