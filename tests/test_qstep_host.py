"""Host side of the per-image quantiser step: the step ladder, the TQC / TQT containers, and the
numpy f32 restatement of the three kernels (tests/qstep_check.py) that the GPU tests compare against."""
import io
import struct

import numpy as np
import pytest

import entropy_check as ek
import qstep_check as qk
from textmae_amd import bitstream as bs
from textmae_amd import tiling


# ------------------------------------------------------------------------------------ the ladder
def test_ladder_literals():
    assert len(bs.QSTEP_F) == 8
    for k in range(8):
        assert np.float32(bs.QSTEP_F[k]) == np.float32(2.0 ** (k / 8)), k
    assert bs.QSTEP_F[0] == 1.0


def test_ladder_all_65():
    assert (bs.Q_MIN, bs.Q_MAX) == (-32, 32)
    for q in range(-32, 33):
        want = np.float32(2.0 ** ((q % 8) / 8)) * np.float32(2.0 ** (q // 8))  # a power of two: the product is exact
        got = bs.qstep(q)
        assert isinstance(got, np.float32) and got == want, q
        assert abs(float(got) / 2.0 ** (q / 8) - 1) < 2.0 ** -24
    assert bs.qstep(0) == 1.0 and bs.qstep(-32) == 0.0625 and bs.qstep(32) == 16.0
    assert all(bs.qstep(q) < bs.qstep(q + 1) for q in range(-32, 32))
    for bad in (-33, 33, 0.5, 1000):
        with pytest.raises(ValueError, match=r"outside -32\.\.32"):
            bs.qstep(bad)


def test_ladder_in_the_kernel_source():
    """the literals of tmae_qstep (csrc/common.h) are the Python mirror's"""
    import os
    import re

    import textmae_amd

    src = open(os.path.join(os.path.dirname(textmae_amd.__file__), "csrc", "common.h")).read()
    body = src[src.index("tmae_qstep(int q)"):]
    lits = re.search(r"F\[8\] = \{([^}]*)\}", body).group(1)
    vals = [float(v.strip().rstrip("f")) for v in lits.split(",")]
    assert vals == list(bs.QSTEP_F)


# ------------------------------------------------------------------------------------ TQC
def _parts(seed=3, L=64, K=16):
    rng = np.random.default_rng(seed)
    ids = bs.pack_ids_host(rng.permutation(L)[:K], L)
    z = rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
    y = rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
    return ids, z, y


def test_tqc_round_trip():
    ids, z, y = _parts()
    plain = bs.assemble(128, 16, 16, 2, 1, (300, 200), ids, z, y)
    assert bs.assemble(128, 16, 16, 2, 1, (300, 200), ids, z, y, q=0) == plain and plain[:4] == b"TMC\x01"
    assert bs.parse(plain).q == 0
    for q in (-32, -1, 5, 32):
        blob = bs.assemble(128, 16, 16, 2, 1, (300, 200), ids, z, y, q=q)
        assert blob[:4] == b"TQC\x01" and len(blob) == len(plain) + 4
        assert blob[4:16] == plain[4:16] and blob[20:] == plain[16:]
        assert struct.unpack_from("<b", blob, 16)[0] == q and blob[17:20] == b"\0\0\0"
        p, p0 = bs.parse(blob), bs.parse(plain)
        assert p.q == q and p[:6] == p0[:6]
        np.testing.assert_array_equal(p.ids, ids)
        assert bytes(p.z) == z and bytes(p.y) == y
    for bad in (33, -33, 1.5):
        with pytest.raises(ValueError, match=r"outside -32\.\.32"):
            bs.assemble(128, 16, 16, 1, 1, None, ids, z, y, q=bad)


def test_tqc_rejections():
    ids, z, y = _parts()
    blob = bytearray(bs.assemble(128, 16, 16, 1, 1, None, ids, z, y, q=7))

    def with_(at, byte):
        b = bytearray(blob)
        b[at] = byte
        return bytes(b)

    with pytest.raises(ValueError, match=r"TQC stream with q = 0: a step of 1 is written as TMC"):
        bs.parse(with_(16, 0))
    for byte, q in ((33, 33), (256 - 33, -33), (127, 127), (128, -128)):
        with pytest.raises(ValueError, match=rf"TQC stream with q = {q}: the ladder is -32\.\.32"):
            bs.parse(with_(16, byte))
    for at in (17, 18, 19):
        with pytest.raises(ValueError, match=r"TQC stream: padding bytes 17-19 hold .*must be zero"):
            bs.parse(with_(at, 1))
    with pytest.raises(ValueError, match=r"container version 2, this reader knows version 1"):
        bs.parse(with_(3, 2))
    with pytest.raises(ValueError, match=r"shorter than the 20-byte TQC header"):
        bs.parse(bytes(blob[:16]))
    # 16 ids of 6 bits = 3 words, 3 z words: the 20-byte header counts
    with pytest.raises(ValueError, match=r"header \+ 3 id words \+ 3 z words \+ at least 2 y words take 52"):
        bs.parse(bytes(blob[:40]))
    assert bs.parse(with_(16, 256 - 32)).q == -32 and bs.parse(with_(16, 32)).q == 32


# ------------------------------------------------------------------------------------ TQT
def _image_parts(seed=4, W=200, H=150, S=128, O=16, L=64, K=16):
    rng = np.random.default_rng(seed)
    T = tiling.grid(H, W, S, O).T
    ids = np.stack([bs.pack_ids_host(rng.permutation(L)[:K], L) for _ in range(T)])
    zs = [rng.integers(0, 256, 4 * int(rng.integers(2, 5)), dtype=np.uint8).tobytes() for _ in range(T)]
    ys = [rng.integers(0, 256, 4 * int(rng.integers(2, 30)), dtype=np.uint8).tobytes() for _ in range(T)]
    return (S, K, 16, 2, 1, O, W, H, 3, ids, zs, ys), T


def test_tqt_round_trip_and_readers():
    args, T = _image_parts()
    assert T >= 4
    plain = bs.assemble_image(*args)
    assert bs.assemble_image(*args, q=0) == plain and plain[:4] == b"TMT\x01"
    assert bs.parse_image(plain).q == 0 and bs.read_image_index(plain).q == 0
    for q in (-32, -3, 11, 32):
        blob = bs.assemble_image(*args, q=q)
        assert blob[:4] == b"TQT\x01" and len(blob) == len(plain)
        assert blob[4:18] == plain[4:18] and blob[20:] == plain[20:]
        assert struct.unpack_from("<b", blob, 18)[0] == q and blob[19] == 0
        p, p0 = bs.parse_image(blob), bs.parse_image(plain)
        assert p.q == q and p[:9] == p0[:9] and p.num_tiles == T
        for src in (blob, io.BytesIO(blob)):
            idx = bs.read_image_index(src)
            assert idx.q == q and idx[:9] == p[:9] and idx.nbytes == len(blob)
            i, zz, yy = bs.read_tiles(src, idx, [T - 1, 0])
            for k, t in enumerate((T - 1, 0)):
                np.testing.assert_array_equal(i[k], args[9][t])
                assert bytes(zz[k]) == args[10][t] and bytes(yy[k]) == args[11][t]
        for t in (0, T - 1):
            one = bs.tile_blob(p, t)
            assert one[:4] == b"TQC\x01"
            assert one == bs.assemble(args[0], args[1], args[2], args[3], args[4], None, args[9][t], args[10][t],
                                      args[11][t], q=q)
            assert bs.parse(one).q == q
            assert bs.tile_blob(p0, t)[:4] == b"TMC\x01"
    with pytest.raises(ValueError, match=r"outside -32\.\.32"):
        bs.assemble_image(*args, q=40)


@pytest.mark.parametrize("reader", [bs.parse_image, bs.read_image_index])
def test_tqt_rejections(reader):
    args, _ = _image_parts()
    blob = bs.assemble_image(*args, q=-5)

    def with_(at, byte):
        b = bytearray(blob)
        b[at] = byte
        return bytes(b)

    with pytest.raises(ValueError, match=r"TQT stream with q = 0: a step of 1 is written as TMT"):
        reader(with_(18, 0))
    for byte, q in ((33, 33), (256 - 33, -33)):
        with pytest.raises(ValueError, match=rf"TQT stream with q = {q}: the ladder is -32\.\.32"):
            reader(with_(18, byte))
    with pytest.raises(ValueError, match=r"TQT stream: padding byte 19 holds 0x01, must be zero"):
        reader(with_(19, 1))
    with pytest.raises(ValueError, match=r"container version 2, this reader knows version 1"):
        reader(with_(3, 2))
    # the TMT reader's own rule is as before: a TMT file with anything in bytes 18-19 is rejected as reserved
    plain = bytearray(bs.assemble_image(*args))
    plain[18] = 5
    with pytest.raises(ValueError, match=r"reserved bytes 18-19 hold 0x0005, must be zero"):
        reader(bytes(plain))


# ------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("shape", list(qk.SHAPES))
def test_cases_hold_every_class(shape):
    """counted on the restatement alone, per image: every tie, sigma / delta on the table, one ulp either side, at and
    below the bound, past the table"""
    c = qk.case(shape)
    assert c.q == qk.Q3
    ys = ek.gcf_slices(c, c.y).contiguous().numpy()
    for b in range(c.n):
        rows = slice(b * c.HW, (b + 1) * c.HW)
        got = qk.census(ys[:, rows], c.mu.numpy()[:, rows], c.sigma.numpy()[:, rows], qk.qstep(c.q[b]),
                        c.table.numpy())
        print(shape, c.q[b], got, c.planted[b])
        for d in qk.TIES:
            assert got[f"tie_{d}"] >= 2, (b, d, got)
        for k in ("on_table", "ulp_above", "ulp_below"):
            assert got[k] >= 3, (b, k, got)
        assert got["below_bound"] >= 4 and got["past_table"] >= 4, (b, got)
        # sigma / delta == 0.11f exactly: always there at a power of two; at another step only if some f32 sigma has
        # that quotient (solve_quotient), which at q = 11 none has
        assert got["at_bound"] >= (1 if c.q[b] % 8 == 0 else c.planted[b]["at_bound"]), (b, got)


def test_restatement_against_float64():
    """on inputs with no near-ties the f32 restatement is the float64 evaluation: the same symbols, the same indexes
    wherever sigma / delta is not within 2^-20 of a table entry or of the bound, y_hat within 2 ulp"""
    rng = np.random.default_rng(17)
    table = ek.model_table().numpy()
    for q in (-32, -7, 0, 11, 32):
        delta = qk.qstep(q)
        n = 20000
        mu = (rng.standard_normal(n) * delta).astype(np.float32)
        y = (mu + 3 * delta * rng.standard_normal(n)).astype(np.float32)
        sigma = (delta * np.exp(rng.uniform(np.log(0.03), np.log(400.0), n))).astype(np.float32)
        r32 = qk.restate(y, mu, sigma, delta, table)
        r64 = qk.restate64(y, mu, sigma, delta, table)
        clear = np.abs(np.abs(r64.t - np.floor(r64.t)) - 0.5) >= 1e-4
        assert clear.mean() > 0.99
        np.testing.assert_array_equal(r32.qi[clear], r64.qi[clear])
        knots = np.concatenate([table.astype(np.float64), [float(np.float32(0.11))]])
        sdiv = sigma.astype(np.float64) / float(delta)  # the unbounded quotient: that is what may cross a knot
        off = np.abs(sdiv[:, None] / knots[None, :] - 1).min(1) > 2.0 ** -20
        assert off.mean() > 0.99
        np.testing.assert_array_equal(r32.idx[off], r64.idx[off])
        err = np.abs(r32.yhat.astype(np.float64) - r64.yhat)[clear]
        ulp = np.spacing(np.maximum(np.abs(r64.yhat), np.abs(r64.qi * delta)).astype(np.float32))[clear]
        assert (err <= 2 * ulp).all()
        np.testing.assert_array_equal(qk.dequantize(r32.sym, mu, delta), r32.yhat)
        assert r32.idx.min() == 0 and r32.idx.max() == table.size - 1


def test_restatement_at_step_one_is_the_existing_arithmetic():
    """delta = 1: rint(y - mu), rint(y - mu) + mu and build_indexes(sigma), the existing kernels' formulas"""
    c = qk.case("tiled2", None)
    assert c.q == (0, 0, 0)
    out, r = qk.reference("tiled2", None)
    ys = ek.gcf_slices(c, c.y)
    qi = ek.rint32(ys, c.mu)
    assert np.array_equal(r.qi, qi.numpy()) and np.array_equal(r.yhat, (qi + c.mu).numpy())
    assert np.array_equal(r.idx, ek.build_indexes32(c.sigma, c.table).numpy())


def test_likelihood_reference_is_the_checkers():
    """the likelihood reference is gc_raw's form without means at x = qi, sigma = fl(sigma / delta): its float64 value
    is the oracle's Gaussian mass of the symbol, and the torch f32 evaluation of the kernel's formula fits the bound"""
    import torch

    out, r = qk.reference("tiled2")
    ref, bound = qk.likelihood_reference(r)
    s = torch.from_numpy(r.s)
    v = torch.from_numpy(np.abs(r.qi))
    k = torch.tensor(ek.K_ERFC, dtype=torch.float32)
    f32 = torch.maximum(0.5 * torch.erfc(k * ((0.5 - v) / s)) - 0.5 * torch.erfc(k * ((-0.5 - v) / s)),
                        torch.tensor(1e-9, dtype=torch.float32))
    assert float(((f32.double() - ref).abs() / bound).max()) <= 1.0
    want = ek.gc_oracle64(torch.from_numpy(r.qi), torch.from_numpy(r.sdiv), None, None)
    assert float((ref - want).abs().max()) <= 1e-13
