"""Container version 1 of the per-image bitstream (textmae_amd.bitstream): the host part.  CPU only.

The numpy id packer / unpacker are the oracle of the two device kernels (tests/test_gpu_bitstream.py), so they are
checked here against the format's definition itself: a bit-by-bit Python restatement and a hand-written vector.
"""
import numpy as np
import pytest

LK = [(64, 16), (196, 144), (100, 64), (1024, 400), (576, 16), (65, 16), (16, 16), (1, 1)]


def random_keep(rng, n, L, K):
    """n random K-subsets of range(L), each in random order"""
    return np.stack([rng.permutation(L)[:K] for _ in range(n)]).astype(np.int64)


def bits_of(L):
    b = 0
    while (1 << b) < L:
        b += 1
    return max(1, b)


def pack_by_definition(ids, L):
    """id k occupies bits [k*bits, (k+1)*bits) of the string, LSB first; bit i is bit i % 32 of word i // 32"""
    bits = bits_of(L)
    words = [0] * ((len(ids) * bits + 31) // 32)
    for k, v in enumerate(ids):
        for j in range(bits):
            if (int(v) >> j) & 1:
                i = k * bits + j
                words[i // 32] |= 1 << (i % 32)
    return np.array(words, dtype=np.uint32)


@pytest.mark.parametrize("L,K", LK)
def test_ids_oracle_round_trip(tmae, L, K):
    from textmae_amd import bitstream as bs

    rng = np.random.default_rng(1000 * L + K)
    keep = random_keep(rng, 3, L, K)
    words = bs.pack_ids_host(keep, L)
    bits = bits_of(L)
    W = (K * bits + 31) // 32
    assert bs.id_bits(L) == bits and bs.id_words(L, K) == W
    assert words.dtype == np.uint32 and words.shape == (3, W)
    for b in range(3):
        np.testing.assert_array_equal(words[b], pack_by_definition(keep[b], L))
        np.testing.assert_array_equal(bs.pack_ids_host(keep[b], L), words[b])  # one image, 1-D
    tail = 32 * W - K * bits
    if tail:  # unused tail bits are zero
        assert not (words[:, -1] >> np.uint32(32 - tail)).any()
    shuf, rest, status = bs.unpack_ids_host(words, L, K)
    assert shuf.dtype == np.int64 and rest.dtype == np.int64 and not status.any()
    np.testing.assert_array_equal(shuf[:, :K], keep)
    for b in range(3):
        unused = sorted(set(range(L)) - set(keep[b].tolist()))
        np.testing.assert_array_equal(shuf[b, K:], unused)  # the completed tail: unused ids ascending
        np.testing.assert_array_equal(rest[b], np.argsort(shuf[b]))
        np.testing.assert_array_equal(shuf[b][rest[b]], np.arange(L))


def test_ids_hand_vector(tmae):
    """L = 64: 6 bits per id.  [5, 63, 0] -> 5 | 63 << 6 | 0 << 12 = 0xFC5: id 0 sits at bit 0 of word 0"""
    from textmae_amd import bitstream as bs

    words = bs.pack_ids_host([5, 63, 0], 64)
    assert words.tolist() == [0x00000FC5]
    # an id that straddles two words: 6 ids of 6 bits fill bits 0..35, the last, 42 = 0b101010, lies in bits 30..35:
    # 1 | 2 << 6 | 3 << 12 | 4 << 18 | 6 << 24 | (42 & 3) << 30, then 42 >> 2
    words = bs.pack_ids_host([1, 2, 3, 4, 6, 42], 64)
    assert words.tolist() == [0x86103081, 0x0000000A]
    shuf, rest, status = bs.unpack_ids_host(words, 64, 6)
    assert status == 0 and shuf[:6].tolist() == [1, 2, 3, 4, 6, 42] and shuf[6:9].tolist() == [0, 5, 7]


def test_ids_oracle_rejections(tmae):
    """status 1 id >= L, 2 duplicate, 3 tail bits; the identity in both outputs for a rejected image"""
    from textmae_amd import bitstream as bs

    rng = np.random.default_rng(3)
    L, K = 100, 64
    keep = random_keep(rng, 3, L, K)
    bad = keep.copy()
    bad[1, 10] = bad[1, 40]
    words = bs.pack_ids_host(bad, L)
    w2 = pack_by_definition([*keep[2, :7], 127, *keep[2, 8:]], L)  # 127 fits the 7 bits but not L
    words[2] = w2
    shuf, rest, status = bs.unpack_ids_host(words, L, K)
    assert status.tolist() == [0, 2, 1]
    np.testing.assert_array_equal(shuf[0, :K], keep[0])
    for b in (1, 2):
        np.testing.assert_array_equal(shuf[b], np.arange(L))
        np.testing.assert_array_equal(rest[b], np.arange(L))
    L, K = 65, 16  # 7 bits: 112 bits, the last word half used
    w = bs.pack_ids_host(random_keep(rng, 1, L, K)[0], L)
    w[-1] |= np.uint32(1 << 20)
    shuf, rest, status = bs.unpack_ids_host(w, L, K)
    assert status == 3
    np.testing.assert_array_equal(shuf, np.arange(L))
    np.testing.assert_array_equal(rest, np.arange(L))


def make_blob(bs, img=224, K=144, patch=16, lanes=8, z_lanes=2, orig=(768, 512), z_words=5, y_words=9, seed=0):
    rng = np.random.default_rng(seed)
    L = (img // patch) ** 2
    ids = bs.pack_ids_host(rng.permutation(L)[:K], L)
    z = rng.integers(0, 256, 4 * z_words, dtype=np.uint8).tobytes()
    y = rng.integers(0, 256, 4 * y_words, dtype=np.uint8).tobytes()
    return bs.assemble(img, K, patch, lanes, z_lanes, orig, ids, z, y), ids, z, y


def test_header_round_trip(tmae):
    from textmae_amd import bitstream as bs

    cases = [dict(img=224, K=144, patch=16, lanes=8, z_lanes=2, orig=(768, 512), z_words=5, y_words=9),
             dict(img=128, K=16, patch=16, lanes=1, z_lanes=1, orig=None, z_words=2, y_words=2),
             dict(img=160, K=100, patch=16, lanes=64, z_lanes=64, orig=(65535, 1), z_words=300, y_words=4),
             dict(img=512, K=1, patch=16, lanes=2, z_lanes=32, orig=(1, 65535), z_words=2, y_words=1000)]
    for c in cases:
        blob, ids, z, y = make_blob(bs, **c)
        assert isinstance(blob, bytes) and len(blob) % 4 == 0
        assert blob[:4] == b"TMC\x01"
        p = bs.parse(blob)
        assert (p.img_size, p.num_keep_patches, p.patch_size) == (c["img"], c["K"], c["patch"])
        assert (p.lanes, p.z_lanes) == (c["lanes"], c["z_lanes"])
        assert p.orig_size == c["orig"]
        assert p.num_patches == (c["img"] // c["patch"]) ** 2
        np.testing.assert_array_equal(p.ids, ids)
        assert bytes(p.z) == z and bytes(p.y) == y
        hdr = bs.pack_header(c["img"], c["K"], c["patch"], c["lanes"], c["z_lanes"], c["z_words"], c["orig"])
        assert hdr == blob[:16] and len(hdr) == bs.HEADER_BYTES
        # the byte layout of the table in DESIGN.md
        assert int.from_bytes(blob[4:6], "little") == c["img"] and int.from_bytes(blob[6:8], "little") == c["K"]
        assert blob[8] == c["patch"]
        assert blob[9] == (c["lanes"].bit_length() - 1) | (c["z_lanes"].bit_length() - 1) << 4
        assert int.from_bytes(blob[10:12], "little") == c["z_words"]
        w, h = c["orig"] or (0, 0)
        assert int.from_bytes(blob[12:14], "little") == w and int.from_bytes(blob[14:16], "little") == h
        assert bs.parse(bytearray(blob)).lanes == c["lanes"] and bs.parse(memoryview(blob)).lanes == c["lanes"]


def changed(blob, at, value):
    b = bytearray(blob)
    b[at] = value
    return bytes(b)


def test_parse_rejections(tmae):
    """each on a valid blob with one byte changed or one word removed"""
    from textmae_amd import bitstream as bs

    blob, *_ = make_blob(bs, z_words=5, y_words=2)  # the shortest valid blob of its header
    bs.parse(blob)
    bad = {
        "magic": changed(blob, 0, ord("X")),
        "version": changed(blob, 3, 2),
        "not whole words": blob[:-1],
        "one word short": blob[:-4],
        "y lane nibble": changed(blob, 9, 0x07),
        "z lane nibble": changed(blob, 9, 0x70),
        "patch does not divide": changed(blob, 8, 15),
        "patch zero": changed(blob, 8, 0),
        "K > L": changed(blob, 6, 197),
        "L > 1024": changed(blob, 8, 4),  # 224 / 4 = 56, L = 3136
    }
    for what, b in bad.items():
        with pytest.raises(ValueError):
            print("rejecting:", what)
            bs.parse(b)
    # a longer z length than the blob holds; a header alone
    with pytest.raises(ValueError):
        bs.parse(changed(blob, 10, 6))
    with pytest.raises(ValueError):
        bs.parse(blob[:16])
    with pytest.raises(ValueError):
        bs.parse(b"")
    # L = 1024 itself is accepted
    ok, *_ = make_blob(bs, img=512, K=400, patch=16)
    assert bs.parse(ok).num_patches == 1024


def test_pack_header_rejections(tmae):
    from textmae_amd import bitstream as bs

    for kw in (dict(lanes=3), dict(lanes=128), dict(z_lanes=0), dict(z_words=1 << 16), dict(orig_size=(70000, 1)),
               dict(img_size=225), dict(num_keep_patches=197), dict(num_keep_patches=0), dict(patch_size=4)):
        args = dict(img_size=224, num_keep_patches=144, patch_size=16)
        args.update(kw)
        with pytest.raises(ValueError):
            bs.pack_header(**args)


def test_side_information_arithmetic(tmae):
    """224^2, K = 144: L = 196 ids of 8 bits -> 144 bytes of ids and a 16-byte header (1152 bits against the 1508 of
    the reference's Huffman code, which also needs a table it does not send)"""
    from textmae_amd import bitstream as bs

    assert bs.HEADER_BYTES == 16 and len(bs.pack_header(224, 144, 16)) == 16
    assert bs.id_bits(196) == 8 and 4 * bs.id_words(196, 144) == 144
    blob, ids, z, y = make_blob(bs)
    assert len(blob) == 16 + 144 + len(z) + len(y)
    assert 60 * 7 + 136 * 8 == 1508 and 144 * 8 == 1152
