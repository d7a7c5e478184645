"""Per-patch quantiser steps on the CPU: the numpy restatements of the side-information kernels
(bitstream.select_levels_host / pack_levels_host / unpack_levels_host / build_qmap_host) against brute-force
definitions, the rule on ties, equal and non-finite scores and at awkward K / nlev, saturation at both ends of the
ladder, the two containers b"TPC" / b"TPT" (round trips, every rejection with its own message, an encode without a map
byte-equal to today's, a TPT tile as a TPC blob) and the cases of qmap_check.py that the GPU tests run."""
import io
import struct

import numpy as np
import pytest

import qmap_check as mk
import qstep_check as qk


@pytest.fixture(scope="module")
def bs(tmae):
    from textmae_amd import bitstream

    return bitstream


def perms(n, L, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(L) for _ in range(n)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("K,L", [(16, 64), (144, 256), (5, 64), (1, 64), (37, 37)])
@pytest.mark.parametrize("nlev", [2, 3, 4, 16])
def test_select_against_brute_force(bs, K, L, nlev):
    rng = np.random.default_rng(K * 100 + nlev)
    ids = perms(4, L, K + nlev)
    scores = rng.random((4, L)).astype(np.float32)
    scores[1] = np.round(scores[1] * 4) / 4       # many ties
    scores[2] = 0.5                               # all equal
    scores[3, ::3] = np.nan
    scores[3, 1::7] = np.inf
    scores[3, 2::11] = -np.inf
    got, status = bs.select_levels_host(ids, K, nlev, scores=scores)
    assert got.dtype == np.int32 and got.shape == (4, K) and not status.any()
    assert np.array_equal(got, mk.brute_select(ids, K, nlev, scores))
    assert got.min() >= 0 and got.max() <= nlev - 1
    if K == 1:
        assert not got.any()


def test_rule_on_ties_and_shares(bs):
    """distinct scores: level l holds the patches of rank [ceil(l K / nlev), ceil((l + 1) K / nlev)); equal scores: the
    earlier kept position ranks first; level 0 is the highest-scoring share"""
    L, K = 64, 16
    ids = perms(1, L, 3)
    scores = np.random.default_rng(4).random((1, L)).astype(np.float32)
    for nlev in (2, 3, 4, 16):
        lv, _ = bs.select_levels_host(ids, K, nlev, scores=scores)
        kept = scores[0][ids[0, :K]]
        order = np.argsort(-kept, kind="stable")
        assert np.array_equal(lv[0][order], (np.arange(K) * nlev) // K)
        counts = np.bincount(lv[0], minlength=nlev)
        assert counts.sum() == K and counts.max() - counts.min() <= 1, (nlev, counts)
    assert np.array_equal(np.bincount(bs.select_levels_host(ids, K, 4, scores=scores)[0][0]), [4, 4, 4, 4])
    # K not divisible by nlev
    lv, _ = bs.select_levels_host(ids, 5, 3, scores=scores)
    assert sorted(lv[0].tolist()) == [0, 0, 1, 1, 2]
    # all equal: the rank is the kept position
    flat = np.full((1, L), 0.25, dtype=np.float32)
    lv, _ = bs.select_levels_host(ids, K, 4, scores=flat)
    assert np.array_equal(lv[0], np.arange(K) // 4)
    # one tie across a level boundary: the earlier position takes the lower level
    s = np.zeros((1, L), dtype=np.float32)
    s[0, ids[0, :4]] = (3.0, 1.0, 1.0, 0.0)
    lv, _ = bs.select_levels_host(ids, 4, 4, scores=s)
    assert lv[0].tolist() == [0, 1, 2, 3]
    # -0.0 equals 0.0; NaN ranks first and stays in range
    s[0, ids[0, :4]] = (0.0, -0.0, np.nan, np.nan)
    lv, _ = bs.select_levels_host(ids, 4, 2, scores=s)
    assert lv[0].tolist() == [0, 0, 0, 0]


def test_select_from_a_map(bs):
    L, K, nlev = 64, 16, 3
    ids = perms(3, L, 5)
    m = np.random.default_rng(6).integers(0, nlev, (3, L))
    lv, st = bs.select_levels_host(ids, K, nlev, level_map=m)
    assert not st.any() and np.array_equal(lv, np.take_along_axis(m, ids[:, :K], 1))
    m[1, ids[1, 7]] = 3          # a kept patch with the invalid level 3
    m[2, ids[2, K + 2]] = 9      # a patch that is not kept: never read
    lv2, st = bs.select_levels_host(ids, K, nlev, level_map=m)
    assert st.tolist() == [0, 1, 0] and not lv2[1].any()
    assert np.array_equal(lv2[0], lv[0]) and np.array_equal(lv2[2], lv[2])
    with pytest.raises(ValueError):
        bs.select_levels_host(ids, K, nlev)
    with pytest.raises(ValueError):
        bs.select_levels_host(ids, K, 17, level_map=m)


@pytest.mark.parametrize("K", [1, 5, 16, 144, 1024])
@pytest.mark.parametrize("nlev", [2, 3, 4, 5, 16])
def test_pack_unpack_against_brute_force(bs, K, nlev):
    lv = np.random.default_rng(K + nlev).integers(0, nlev, (3, K))
    lv[0, -1] = nlev - 1
    words = bs.pack_levels_host(lv, nlev)
    assert words.dtype == np.uint32 and words.shape == (3, bs.level_words(K, nlev))
    assert bs.level_bits(nlev) == max(1, int(np.ceil(np.log2(nlev))))
    for b in range(3):
        assert np.array_equal(words[b], mk.brute_pack(lv[b], nlev))
    assert np.array_equal(bs.pack_levels_host(lv[0], nlev), words[0])
    got, st = bs.unpack_levels_host(words, nlev, K)
    assert not st.any() and np.array_equal(got, lv)
    # padded rows, mixed tables, an image without a map
    wide = np.zeros((3, words.shape[1] + 2), dtype=np.uint32)
    wide[:, :words.shape[1]] = words
    wide[1] = 0xFFFFFFFF
    got, st = bs.unpack_levels_host(wide, [nlev, 1, nlev], K)
    assert st.tolist() == [0, 0, 0] and np.array_equal(got[0], lv[0]) and not got[1].any()
    assert np.array_equal(got[2], lv[2])


def test_unpack_faults(bs):
    K, nlev = 5, 3  # 10 bits of 32 used
    lv = np.array([[0, 1, 2, 1, 0]] * 4)
    w = bs.pack_levels_host(lv, nlev).copy()
    w[1, 0] |= 3 << 4           # level 2 of image 1 -> the invalid level 3
    w[2, 0] |= 1 << 20          # a tail bit
    w[3, 0] |= (3 << 0) | (1 << 31)  # both: the lowest code wins
    got, st = bs.unpack_levels_host(w, nlev, K)
    assert st.tolist() == [0, 1, 2, 1]
    assert np.array_equal(got[0], lv[0]) and not got[1:].any()
    # a row too narrow for the image's table counts as a fault and is not read
    got, st = bs.unpack_levels_host(np.zeros((1, 1), dtype=np.uint32), [16], 16)
    assert st.tolist() == [1] and not got.any()


def test_build_and_saturation(bs):
    lv = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [0, 0, 3, 3]])
    offs = (-8, -3, 0, 5)
    rows = [bs.offsets_row(offs)] * 3
    for q in ((30, -30, 0), (0, 0, 0), (-32, 32, 5)):
        got = bs.build_qmap_host(lv, q, rows)
        assert got.dtype == np.int32 and np.array_equal(got, mk.brute_qmap(lv, q, rows))
    got = bs.build_qmap_host(lv, (30, -30, 0), rows)
    assert got[0].tolist() == [22, 27, 30, 32]      # 35 saturates at the top, 30 does not
    assert got[1].tolist() == [-25, -30, -32, -32]  # -33 and -38 saturate at the bottom
    # both ends in one image, offsets at their own limits
    wide = bs.build_qmap_host([[0, 1]], [0], [bs.offsets_row((-64, 64))])
    assert wide.tolist() == [[-32, 32]]
    assert np.array_equal(bs.build_qmap_host(lv, None, rows), bs.build_qmap_host(lv, (0, 0, 0), rows))
    assert float(bs.qstep(-32)) == 1 / 16 and float(bs.qstep(32)) == 16.0


def test_check_offsets(bs):
    assert bs.check_offsets([-8, 0, 5]) == (-8, 0, 5)
    assert bs.check_offsets(np.array([-64, 64])) == (-64, 64)
    for bad, msg in (([1], r"nlev = 1 outside 2\.\.16"), ([0] * 17, r"nlev = 17 outside 2\.\.16"),
                     ([0, 65], r"offset outside -64\.\.64"), ([0, -65], r"offset outside -64\.\.64"),
                     ([0, 1.5], r"offset outside -64\.\.64"), (3, r"a sequence of 2\.\.16 integers")):
        with pytest.raises(ValueError, match=msg):
            bs.check_offsets(bad)


# ------------------------------------------------------------------------------------------------ b"TPC"
GEO = dict(img=128, K=16, patch=16, L=64)


def parts(bs, nlev=4, seed=1):
    rng = np.random.default_rng(seed)
    ids = bs.pack_ids_host(rng.permutation(GEO["L"])[:GEO["K"]], GEO["L"])
    lv = bs.pack_levels_host(rng.integers(0, nlev, GEO["K"]), nlev)
    z = rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
    y = rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
    return ids, lv, z, y


def tpc(bs, q=3, offs=(-8, -3, 0, 5), lanes=1, orig=(300, 200), seed=1):
    ids, lv, z, y = parts(bs, len(offs), seed)
    return bs.assemble(GEO["img"], GEO["K"], GEO["patch"], lanes, 1, orig, ids, z, y, q, offs, lv), (ids, lv, z, y)


@pytest.mark.parametrize("offs", [(-8, -3, 0, 5), (0, 0), (-64, 64, 1), tuple(range(-8, 8))])
@pytest.mark.parametrize("q", [0, 7, -32, 32])
def test_tpc_round_trip(bs, q, offs):
    blob, (ids, lv, z, y) = tpc(bs, q, offs, lanes=8)
    assert blob[:4] == b"TPC\x01" and len(blob) % 4 == 0
    assert len(blob) == bs.PHEADER_BYTES + 4 * (len(ids) + bs.level_words(GEO["K"], len(offs))) + len(z) + len(y)
    assert blob[16] == q & 0xFF and blob[17] == len(offs) and blob[18:20] == b"\0\0"
    assert blob[20:36] == struct.pack("<16b", *bs.offsets_row(offs))
    p = bs.parse(blob)
    assert (p.img_size, p.num_keep_patches, p.patch_size, p.lanes, p.z_lanes) == (128, 16, 16, 8, 1)
    assert p.orig_size == (300, 200) and p.q == q and p.nlev == len(offs) and p.offsets == tuple(offs)
    assert np.array_equal(p.ids, ids) and np.array_equal(p.levels, lv)
    assert bytes(p.z) == z and bytes(p.y) == y


def test_without_a_map_todays_bytes(bs):
    ids, _, z, y = parts(bs)
    for q, magic in ((0, b"TMC"), (5, b"TQC")):
        head = struct.pack("<3sBHHBBHHH", magic, 1, 128, 16, 16, 1, len(z) // 4, 9, 9)  # the layout written out
        old = head + (struct.pack("<bxxx", q) if q else b"") + ids.tobytes() + z + y
        new = bs.assemble(128, 16, 16, 2, 1, (9, 9), ids, z, y, q)
        assert new == old
        p = bs.parse(new)
        assert p.q == q and p.nlev == 1 and p.offsets == () and p.levels is None
        assert len(p) == 13 and p[:6] == (128, 16, 16, 2, 1, (9, 9)) and np.array_equal(p.ids, ids)
    assert len(bs.pack_header(128, 16, 16)) == 16 and len(bs.pack_header(128, 16, 16, q=1)) == 20
    assert len(bs.pack_header(128, 16, 16, offsets=(0, 1))) == 36


def test_tpc_rejections(bs):
    blob, _ = tpc(bs)

    def patched(at, byte):
        b = bytearray(blob)
        b[at] = byte
        return bytes(b)

    for bad, msg in ((patched(17, 1), r"TPC stream with nlev = 1: outside 2\.\.16"),
                     (patched(17, 17), r"TPC stream with nlev = 17: outside 2\.\.16"),
                     (patched(21, 65), r"TPC stream: offset 1 = 65 outside -64\.\.64"),
                     (patched(20, 0x80), r"TPC stream: offset 0 = -128 outside -64\.\.64"),
                     (patched(24, 1), r"TPC stream: unused offsets .* past nlev = 4 must be zero"),
                     (patched(18, 1), r"TPC stream: padding bytes 18-19 hold 0100, must be zero"),
                     (patched(19, 7), r"TPC stream: padding bytes 18-19 hold 0007, must be zero"),
                     (patched(16, 33), r"TPC stream with q = 33: the ladder is -32\.\.32"),
                     (patched(16, 0xDF), r"TPC stream with q = -33: the ladder is -32\.\.32"),
                     (blob[:32], r"32 bytes: shorter than the 36-byte TPC header"),
                     (blob[:60], r"60 bytes: header \+ 3 id words \+ 1 level words \+ 3 z words \+ at least 2 y")):
        with pytest.raises(ValueError, match=msg):
            bs.parse(bad)
    ids, lv, z, y = parts(bs)
    with pytest.raises(ValueError, match=r"2 level words, 1 expected"):
        bs.assemble(128, 16, 16, 1, 1, None, ids, z, y, 0, (0, 1, 2, 3), np.zeros(2, dtype=np.uint32))
    with pytest.raises(ValueError, match=r"offsets and level words go together"):
        bs.assemble(128, 16, 16, 1, 1, None, ids, z, y, 0, (0, 1, 2, 3))
    with pytest.raises(ValueError, match=r"nlev = 1 outside 2\.\.16"):
        bs.assemble(128, 16, 16, 1, 1, None, ids, z, y, 0, (0,), lv)
    with pytest.raises(ValueError, match=r"offset outside -64\.\.64"):
        bs.assemble(128, 16, 16, 1, 1, None, ids, z, y, 0, (0, 99), lv)
    with pytest.raises(ValueError, match=r"outside -32\.\.32"):
        bs.assemble(128, 16, 16, 1, 1, None, ids, z, y, 40, (0, 1, 2, 3), lv)


# ------------------------------------------------------------------------------------------------ b"TPT"
def tpt(bs, q=-4, offs=(-8, 0, 5), W=200, H=150, O=16):
    from textmae_amd import tiling

    T = tiling.grid(H, W, 128, O).T
    rng = np.random.default_rng(9)
    ids = np.stack([bs.pack_ids_host(rng.permutation(64)[:16], 64) for _ in range(T)])
    lv = None if offs is None else np.stack([bs.pack_levels_host(rng.integers(0, len(offs), 16), len(offs))
                                             for _ in range(T)])
    zs = [rng.integers(0, 256, 8 + 4 * t, dtype=np.uint8).tobytes() for t in range(T)]
    ys = [rng.integers(0, 256, 16 + 8 * t, dtype=np.uint8).tobytes() for t in range(T)]
    extra = () if offs is None else (offs, lv)
    return bs.assemble_image(128, 16, 16, 1, 1, O, W, H, 3, ids, zs, ys, q, *extra), (ids, lv, zs, ys, T)


def test_tpt_round_trip_and_tiles(bs):
    offs = (-8, 0, 5)
    blob, (ids, lv, zs, ys, T) = tpt(bs, -4, offs)
    assert T == 4 and blob[:4] == b"TPT\x01" and blob[18] == (-4) & 0xFF and blob[19] == 3
    assert blob[24:40] == struct.pack("<16b", *bs.offsets_row(offs))
    p = bs.parse_image(blob)
    assert (p.q, p.nlev, p.offsets, p.num_tiles, p.chunk) == (-4, 3, offs, 4, 3)
    idx = bs.read_image_index(blob)
    assert (idx.q, idx.nlev, idx.offsets, idx.nbytes) == (-4, 3, offs, len(blob))
    for t in range(T):
        assert np.array_equal(p.ids[t], ids[t]) and np.array_equal(p.levels[t], lv[t])
        assert bytes(p.z[t]) == zs[t] and bytes(p.y[t]) == ys[t]
        tb = bs.tile_blob(p, t)  # a tile of a TPT file is a TPC blob
        assert tb[:4] == b"TPC\x01"
        q = bs.parse(tb)
        assert (q.q, q.nlev, q.offsets, q.orig_size) == (-4, 3, offs, None)
        assert np.array_equal(q.ids, ids[t]) and np.array_equal(q.levels, lv[t])
        assert bytes(q.z) == zs[t] and bytes(q.y) == ys[t]
        assert tb == bs.assemble(128, 16, 16, 1, 1, None, ids[t], zs[t], ys[t], -4, offs, lv[t])
    for src in (blob, io.BytesIO(blob)):
        i, z, y, l = bs.read_tiles(src, idx, [3, 0])
        assert np.array_equal(i[0], ids[3]) and np.array_equal(l[0], lv[3]) and np.array_equal(l[1], lv[0])
        assert bytes(z[1]) == zs[0] and bytes(y[0]) == ys[3]
    # base q = 0 with a table is still a TPT file
    zero, _ = tpt(bs, 0, offs)
    assert zero[:3] == b"TPT" and bs.parse_image(zero).q == 0


def test_tiled_without_a_map_todays_bytes(bs):
    for q, magic in ((0, b"TMT"), (6, b"TQT")):
        blob, (ids, _, zs, ys, T) = tpt(bs, q, None)
        assert blob[:3] == magic
        p = bs.parse_image(blob)
        assert (p.q, p.nlev, p.offsets, p.levels) == (q, 1, (), None)
        idx = bs.read_image_index(blob)
        assert (idx.q, idx.nlev, idx.offsets) == (q, 1, ())
        assert len(bs.read_tiles(blob, idx, [0])) == 3
        head = 24 + 8 * T
        assert len(blob) == head + sum(4 * 3 + len(z) + len(y) for z, y in zip(zs, ys))
        assert bs.tile_blob(p, 1) == bs.assemble(128, 16, 16, 1, 1, None, ids[1], zs[1], ys[1], q)


def test_tpt_rejections(bs):
    blob, _ = tpt(bs)

    def patched(at, byte):
        b = bytearray(blob)
        b[at] = byte
        return bytes(b)

    for bad, msg in ((patched(19, 0), r"TPT stream with nlev = 0: outside 2\.\.16"),
                     (patched(19, 17), r"TPT stream with nlev = 17: outside 2\.\.16"),
                     (patched(25, 0x7F), r"TPT stream: offset 1 = 127 outside -64\.\.64"),
                     (patched(30, 2), r"TPT stream: unused offsets .* past nlev = 3 must be zero"),
                     (patched(18, 0x40), r"TPT stream with q = 64: the ladder is -32\.\.32"),
                     (blob[:36], r"36 bytes: shorter than the 40-byte TPT header"),
                     (blob[:48], r"48 bytes: the header and the table of 4 tiles take 72"),
                     (blob[:-4], r"bytes: the header, the table and the 4 tiles it lists take")):
        for reader in (bs.parse_image, bs.read_image_index):
            with pytest.raises(ValueError, match=msg):
                reader(bad)
    # the old magics keep their own checks of bytes 18-19
    plain, _ = tpt(bs, 0, None)
    b = bytearray(plain)
    b[19] = 3
    with pytest.raises(ValueError, match=r"reserved bytes 18-19"):
        bs.parse_image(bytes(b))


# ------------------------------------------------------------------------------------------------ the GPU tests' cases
@pytest.mark.parametrize("shape", list(mk.SHAPES))
def test_cases_plant_every_class_at_the_elements_own_step(tmae, shape):
    c = mk.case(shape)
    HW, sw, nsl = mk.SHAPES[shape]
    assert c.qmap.shape == (3, HW) and c.delta.shape == (nsl, 3 * HW, sw)
    q0 = set(c.qmap[0].tolist())
    assert {-32, 32, 0} <= q0 and sum(1 for v in q0 if v % 8) >= 2  # both ends, one, two steps off the powers of two
    assert len(set(c.qmap[1].tolist())) == 4 and set(c.qmap[2].tolist()) == {7}
    assert np.array_equal(c.delta[0, :, 0], mk.steps(c.qmap).reshape(-1))
    assert (HW * (sw + 1) <= 4800) == (shape != "element2")
    _, r = mk.reference(shape)
    ys = __import__("entropy_check").gcf_slices(c, c.y).contiguous().numpy()
    exact = (ys.astype(np.float64) - c.mu.numpy().astype(np.float64)) == (ys - c.mu.numpy()).astype(np.float64)
    tab = c.table.numpy()
    for b, v, planted in c.planted:  # per image and ladder position: what was planted is there, at that step
        rows = b * HW + np.flatnonzero(c.qmap[b] == v)
        t, sd = r.t[:, rows, :], r.sdiv[:, rows, :]
        for d in qk.TIES:
            assert int(((t == np.float32(d)) & exact[:, rows, :]).sum()) >= planted[f"tie_{d}"] >= 1, (b, v, d)
        assert int(np.isin(sd, tab).sum()) >= planted["on_table"] >= 1, (b, v)
        assert int((sd == np.float32(0.11)).sum()) >= planted["at_bound"], (b, v)
        assert int((sd < np.float32(0.11)).sum()) >= 4 and int((sd > tab[-1]).sum()) >= 4, (b, v)


def test_regrouping_is_a_relabelling(tmae):
    """qmap_check.regrouped / by_row / lik_by_row: the same elements under another (n, HW)"""
    import entropy_check as ek
    import torch

    c = mk.case("element2")
    d = mk.regrouped(c, 9, 108)
    assert d.M == c.M and d.HW * (d.sw + 1) <= 4800 < c.HW * (c.sw + 1)
    out_c, _ = mk.reference_of(c)
    out_d, _ = mk.reference_of(d)
    assert torch.equal(out_c["yhat32"], out_d["yhat32"])
    assert torch.equal(mk.by_row(c, out_c["sym"]), mk.by_row(d, out_d["sym"]))
    assert torch.equal(mk.by_row(c, out_c["idx"]), mk.by_row(d, out_d["idx"]))
    assert torch.equal(mk.lik_by_row(c, out_c["lik"][0].reshape(-1)), mk.lik_by_row(d, out_d["lik"][0].reshape(-1)))
    assert not torch.equal(out_c["sym"], out_d["sym"])
    assert torch.equal(ek.coder_order(mk.by_row(c, out_c["sym"]), c.n, c.HW), out_c["sym"])
