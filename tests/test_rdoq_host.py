"""Host side of the rate-distortion optimised quantisation of y: the numpy f32 restatement of the rule
(tests/rdoq_check.py) that the GPU tests compare against, the rate table and coder.table_bits."""
import math

import numpy as np
import pytest
import torch

import entropy_check as ek
import qstep_check as qk
import rdoq_check as rk

CASES = [(s, m) for s in rk.SHAPES for m in rk.MODES]


# ------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("shape,mode", CASES)
def test_census(shape, mode):
    """every class the kernel can get wrong is there, counted on the restatement alone, and at every weight > 0 some
    symbols move and some stay"""
    c = rk.case(shape, mode)
    classes, per_image = rk.census(c, rk.reference(shape, mode)[1])
    print(shape, mode, classes, per_image)
    empty = [k for k, v in classes.items() if v == 0]
    assert not empty, empty
    for b, (flips, keeps) in enumerate(per_image):
        if c.w[b] > 0:
            assert flips > 0 and keeps > 0, (b, flips, keeps)
        else:
            assert flips == 0
    if mode == "qmap":
        assert max(len(set(c.qmap[b].tolist())) for b in range(c.n)) >= 3
    if mode == "q":
        assert c.q == (-32, 0, 11)
    assert 0 in c.w and sorted(c.w)[1] < 1 < sorted(c.w)[2]


def test_launch_forms():
    """tiled2 takes the LDS form, element2 the element form (HW (sw + 1) against the 4800 of the tile)"""
    for shape, tiled in (("tiled2", True), ("element2", False)):
        HW, sw, nsl = qk.SHAPES[shape]
        assert (HW * (sw + 1) <= 4800) == tiled and nsl == 2


@pytest.mark.parametrize("shape,mode", CASES)
def test_weight_zero_is_plain_rounding(shape, mode):
    c = rk.case(shape, mode)
    _, r = rk.reference(shape, mode, (0.0, 0.0, 0.0))
    ys = ek.gcf_slices(c, c.y).contiguous().numpy()
    r0 = qk.restate(ys, c.mu.numpy(), c.sigma.numpy(), c.delta, c.table.numpy())
    assert not r.flipped.any()
    for name in ("qi", "sym", "yhat", "s", "idx"):
        a, b = getattr(r, name), getattr(r0, name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                                     b.view(np.int32) if b.dtype == np.float32 else b), name


@pytest.mark.parametrize("shape,mode", CASES)
def test_toward_zero_and_never_dearer(shape, mode):
    from textmae_amd import coder

    tb = rk.tables()
    _, r = rk.reference(shape, mode)
    assert (np.abs(r.qi) <= np.abs(r.qi0)).all() and (np.abs(r.qi0) - np.abs(r.qi) <= 1).all()
    assert (r.dd >= 0).all()
    bits = lambda q: coder.symbol_bits(q.astype(np.int64).reshape(-1), r.idx.reshape(-1), tb.rate, tb.sizes,  # noqa: E731
                                       tb.offsets)
    assert (bits(r.qi) <= bits(r.qi0)).all()
    assert (bits(r.qi)[r.flipped.reshape(-1)] < bits(r.qi0)[r.flipped.reshape(-1)]).all()


@pytest.mark.parametrize("shape,mode", [("tiled2", "q"), ("tiled2", "qmap"), ("element2", "none")])
def test_flips_monotone_in_the_weight(shape, mode):
    prev = None
    for w in (0.0, 0.01, 0.5, 3.0, 1000.0):
        f = rk.reference(shape, mode, (w, w, w))[1].flipped
        if prev is not None:
            assert not (prev & ~f).any(), w
            assert f.sum() > prev.sum(), w
        prev = f


# ------------------------------------------------------------------------------------ the rate table
def _model():
    from textmae_amd.entropy import GaussianConditional

    tb = rk.tables()
    gc = GaussianConditional(None)
    gc._quantized_cdf, gc._cdf_length, gc._offset = (torch.from_numpy(a.copy()) for a in (tb.cdf, tb.sizes, tb.offsets))
    return gc, tb


def test_rate_table_against_float64():
    gc, tb = _model()
    B = gc.rate_table()
    assert B.dtype == np.float32 and B.shape == (tb.cdf.shape[0], tb.cdf.shape[1] - 1) and B.flags.c_contiguous
    assert gc.rate_table() is B  # cached with the host tables
    assert np.array_equal(B, tb.rate)
    ref = np.zeros(B.shape, dtype=np.float64)
    for r in range(B.shape[0]):
        for k in range(int(tb.sizes[r]) - 1):
            ref[r, k] = 16.0 - math.log2(int(tb.cdf[r, k + 1]) - int(tb.cdf[r, k]))
    assert np.array_equal(ref, rk.rate_table64(tb.cdf, tb.sizes))
    # one rounding to f32 of a float64 value whose own error is a few 2^-53
    assert (np.abs(B.astype(np.float64) - ref) <= 2.0 ** -24 * np.abs(ref) + 1e-13).all()
    inside = np.arange(B.shape[1])[None, :] < (tb.sizes.astype(np.int64) - 1)[:, None]
    assert (B[~inside] == 0).all() and (B[inside] > 0).all() and (B[inside] <= 16).all()
    # a frequency that is a power of two costs a whole number of bits, exactly
    freq = np.diff(tb.cdf.astype(np.int64), axis=1)
    pow2 = inside & (freq > 0) & ((freq & (freq - 1)) == 0)
    assert pow2.sum() > 64 and np.array_equal(B[pow2], (16 - np.log2(freq[pow2])).astype(np.float32))
    # a row sums to 2^16: the Kraft sum of its costs is one
    for r in (0, 9, 63):
        assert abs(float(np.exp2(-B[r, :tb.sizes[r] - 1].astype(np.float64)).sum()) - 1.0) < 1e-5


def test_rate_table_rejects_a_flat_row():
    from textmae_amd import coder

    tb = rk.tables()
    bad = tb.cdf.copy()
    bad[3, 2] = bad[3, 1]
    with pytest.raises(ValueError, match="not strictly increasing"):
        coder.rate_table(bad, tb.sizes)


def test_symbol_bits_by_hand():
    """the escape rule one symbol at a time: row 0 is the narrowest (size 5, offset -1: symbols -1, 0, 1 in support)"""
    from textmae_amd import coder

    tb = rk.tables()
    assert int(tb.sizes[0]) == 5 and int(tb.offsets[0]) == -1
    B = tb.rate[0].astype(np.float64)
    want = {-1: B[0], 0: B[1], 1: B[2], 2: B[3] + 4, 3: B[3] + 8, 9: B[3] + 8, 10: B[3] + 12, -2: B[3] + 8,
            -9: B[3] + 8, -10: B[3] + 12, 129: B[3] + 12, 130: B[3] + 16}
    for v, w in want.items():
        got = coder.symbol_bits([v], [0], tb.rate, tb.sizes, tb.offsets)
        assert got.dtype == np.float32 and float(got[0]) == float(np.float32(w)), (v, float(got[0]), w)
    with pytest.raises(ValueError, match="outside the tables"):
        coder.symbol_bits([0], [64], tb.rate, tb.sizes, tb.offsets)


@pytest.mark.parametrize("shape,mode", [("tiled2", "q"), ("tiled2", "qmap"), ("element2", "q")])
def test_table_bits_against_the_record(shape, mode):
    """the host coder codes image b's symbols (the restatement's, in the coder's order); its record of R bits satisfies
    table_bits - 64 <= R <= 1.001 table_bits + 96: 0.1 % is DESIGN.md §3.5's figure for this coder, 64 bits the state
    flush, 32 one spare word, and the lower slack the state's initial content"""
    from textmae_amd import coder

    tb = rk.tables()
    c = rk.case(shape, mode)
    out, _ = rk.reference(shape, mode)
    sym = out["sym"].reshape(c.nsl, c.n, c.sw * c.HW).numpy()
    idx = out["idx"].reshape(c.nsl, c.n, c.sw * c.HW).numpy()
    for b in range(c.n):
        s, i = sym[:, b].reshape(-1), idx[:, b].reshape(-1)
        record = coder.RansEncoder().encode_with_indexes(s, i, tb.cdf, tb.sizes, tb.offsets)
        back = coder.RansDecoder().decode_with_indexes(record, i, tb.cdf, tb.sizes, tb.offsets)
        assert np.array_equal(np.asarray(back), s)
        R, T = 8 * len(record), coder.table_bits(s, i, tb.cdf, tb.sizes, tb.offsets)
        print(shape, mode, b, "record bits", R, "table_bits", T)
        assert T - 64 <= R <= 1.001 * T + 96, (b, R, T)
