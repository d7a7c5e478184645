"""Tiled full-resolution codec, host part (CPU only): the tile grid and blend weights of textmae_amd.tiling by brute
force, the numpy cut / blend oracle on itself, and the TMT container of textmae_amd.bitstream."""
import struct

import numpy as np
import pytest

SIZES = (1, 15, 16, 17, 28, 29, 41)
OVERLAPS = (0, 1, 4, 8)
S = 16


@pytest.mark.parametrize("O", OVERLAPS)
def test_grid_and_weights_brute_force(tmae, O):
    from textmae_amd import tiling

    stride = S - O
    for H in SIZES:
        for W in SIZES:
            g = tiling.grid(H, W, S, O)
            assert (g.stride, g.T) == (stride, g.ny * g.nx)
            for n, extent in ((g.nx, W), (g.ny, H)):
                assert n * stride + O >= extent
                assert n == 1 or (n - 1) * stride + O < extent
            # per axis: the tiles that geometrically hold a coordinate are the ones covering() names, one or two,
            # and their weights sum to O + 1
            for n, extent in ((g.nx, W), (g.ny, H)):
                w = [tiling.axis_weights(k, n, S, O) for k in range(n)]
                for c in range(extent):
                    geo = [k for k in range(n) if k * stride <= c < k * stride + S]
                    assert geo == tiling.covering(c, n, stride, O), (H, W, O, c)
                    assert 1 <= len(geo) <= 2
                    assert sum(int(w[k][c - k * stride]) for k in geo) == O + 1
            # 2-D: every pixel covered, the product weights sum to (O + 1)^2
            total = np.zeros((H, W), dtype=np.int64)
            for t in range(g.T):
                ty, tx = divmod(t, g.nx)
                y0, x0 = g.origin(t)
                assert (y0, x0) == (ty * stride, tx * stride)
                w2 = np.outer(tiling.axis_weights(ty, g.ny, S, O), tiling.axis_weights(tx, g.nx, S, O))
                h, w_ = min(S, H - y0), min(S, W - x0)
                assert h > 0 and w_ > 0
                total[y0:y0 + h, x0:x0 + w_] += w2[:h, :w_]
            assert (total == (O + 1) ** 2).all(), (H, W, O)


def test_grid_rejects(tmae):
    from textmae_amd import tiling

    with pytest.raises(ValueError, match="overlap 9 outside"):
        tiling.grid(20, 20, 16, 9)
    with pytest.raises(ValueError, match="overlap -1 outside"):
        tiling.grid(20, 20, 16, -1)
    with pytest.raises(ValueError, match="both sizes must be >= 1"):
        tiling.grid(0, 20, 16, 4)
    with pytest.raises(ValueError, match="at most 4096"):
        tiling.grid(16 * 65, 16 * 64, 16, 0)
    assert tiling.grid(16 * 64, 16 * 64, 16, 0).T == 4096


@pytest.mark.parametrize("O", OVERLAPS)
def test_blend_of_cut_is_identity(tmae, O):
    from textmae_amd import tiling

    rng = np.random.default_rng(3 + O)
    for H in SIZES:
        for W in SIZES:
            img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            tiles = tiling.tile_cut_host(img, S, O)
            g = tiling.grid(H, W, S, O)
            assert tiles.shape == (g.T, S, S, 3) and tiles.dtype == np.uint8
            # the samples: clamped coordinates
            t = g.T - 1
            y0, x0 = g.origin(t)
            assert (tiles[t, S - 1, S - 1] == img[min(y0 + S - 1, H - 1), min(x0 + S - 1, W - 1)]).all()
            assert (tiles[0, 0, 0] == img[0, 0]).all()
            f = tiles.astype(np.float64).transpose(0, 3, 1, 2) / 255.0
            back = tiling.tile_blend_host(f, H, W, O)
            assert back.shape == (3, H, W) and back.dtype == np.float64
            assert np.abs(back - img.astype(np.float64).transpose(2, 0, 1) / 255.0).max() <= 1e-12


def test_library_validates_before_launch(tmae):
    """tmae_tile_cut_u8 / tmae_tile_blend check their arguments on the host, so this needs no GPU: every call here
    returns before a launch"""
    from textmae_amd import _lib

    def cut(H, W, S, O, t0, nt, ptr=None):
        return _lib.call("tmae_tile_cut_u8", ptr, H, W, S, O, t0, nt, ptr, ptr, None)

    def blend(H, W, S, O, ptr=None, f32=None, u8=None):
        return _lib.call("tmae_tile_blend", ptr, H, W, S, O, f32, u8, None)

    with pytest.raises(ValueError, match="overlap 9 outside"):
        cut(20, 20, 16, 9, 0, 1)
    with pytest.raises(ValueError, match="overlap 9 outside"):
        blend(20, 20, 16, 9)
    with pytest.raises(ValueError, match="both sizes must be >= 1"):
        cut(0, 20, 16, 4, 0, 1)
    with pytest.raises(ValueError, match="both sizes must be >= 1"):
        blend(20, 0, 16, 4)
    with pytest.raises(ValueError, match="65 x 64 tiles, at most 4096"):
        cut(16 * 65, 16 * 64, 16, 0, 0, 1)
    with pytest.raises(ValueError, match="64 x 65 tiles, at most 4096"):
        blend(16 * 64, 16 * 65, 16, 0)
    with pytest.raises(ValueError, match=r"tiles 1\.\.5 outside the image's 4"):
        cut(20, 20, 16, 4, 1, 4)
    with pytest.raises(ValueError, match=r"tiles -1\.\.0 outside"):
        cut(20, 20, 16, 4, -1, 1)
    with pytest.raises(ValueError, match=r"tiles 0\.\.0 outside"):
        cut(20, 20, 16, 4, 0, 0)
    with pytest.raises(ValueError, match="src / tiles / gray are NULL"):
        cut(20, 20, 16, 4, 0, 4)
    with pytest.raises(ValueError, match="tiles is NULL"):
        blend(20, 20, 16, 4)
    with pytest.raises(ValueError, match="out_f32 and out_u8 are both NULL"):
        blend(20, 20, 16, 4, ptr=4096)


# ------------------------------------------------------------------------------------------------ container
GEO =dict(img_size=32, K=3, patch=16, lanes=4, z_lanes=2, overlap=8, width=70, height=40, chunk=5)


def make_file(tmae):
    """a valid file of 2 x 3 tiles (32 px tiles, overlap 8, 70 x 40 image) with records of different lengths"""
    from textmae_amd import bitstream as bs
    from textmae_amd import tiling

    g = tiling.grid(GEO["height"], GEO["width"], GEO["img_size"], GEO["overlap"])
    assert (g.ny, g.nx) == (2, 3)
    rng = np.random.default_rng(5)
    L = (GEO["img_size"] // GEO["patch"]) ** 2
    W = bs.id_words(L, GEO["K"])
    ids = rng.integers(0, 1 << 32, (g.T, W), dtype=np.uint64).astype(np.uint32)
    z = [rng.integers(0, 256, 4 * (2 + t), dtype=np.uint8).tobytes() for t in range(g.T)]
    y = [rng.integers(0, 256, 4 * (7 - t), dtype=np.uint8).tobytes() for t in range(g.T)]
    blob = bs.assemble_image(GEO["img_size"], GEO["K"], GEO["patch"], GEO["lanes"], GEO["z_lanes"], GEO["overlap"],
                             GEO["width"], GEO["height"], GEO["chunk"], ids, z, y)
    return blob, ids, z, y


def test_container_round_trip(tmae):
    from textmae_amd import bitstream as bs

    blob, ids, z, y = make_file(tmae)
    assert isinstance(blob, bytes) and len(blob) % 4 == 0 and blob[:4] == b"TMT\x01"
    assert len(blob) == 24 + 8 * 6 + sum(4 * ids.shape[1] + len(z[t]) + len(y[t]) for t in range(6))
    p = bs.parse_image(blob)
    assert (p.img_size, p.num_keep_patches, p.patch_size, p.lanes, p.z_lanes) == (32, 3, 16, 4, 2)
    assert (p.overlap, p.width, p.height, p.chunk, p.num_tiles, p.num_patches) == (8, 70, 40, 5, 6, 4)
    for t in range(6):
        np.testing.assert_array_equal(p.ids[t], ids[t])
        assert bytes(p.z[t]) == z[t] and bytes(p.y[t]) == y[t]
        one = bs.tile_blob(p, t)
        q = bs.parse(one)
        assert (q.img_size, q.num_keep_patches, q.patch_size, q.lanes, q.z_lanes, q.orig_size) == \
            (32, 3, 16, 4, 2, None)
        np.testing.assert_array_equal(q.ids, ids[t])
        assert bytes(q.z) == z[t] and bytes(q.y) == y[t]
        assert one == bs.assemble(32, 3, 16, 4, 2, None, ids[t], z[t], y[t])
    with pytest.raises(ValueError, match="tile 6 outside"):
        bs.tile_blob(p, 6)
    with pytest.raises(ValueError, match=r"not a TMC bitstream \(magic b'TMT'\)"):
        bs.parse(blob)
    with pytest.raises(ValueError, match="not a TMT bitstream"):
        bs.parse_image(bs.tile_blob(p, 0) + b"\0" * 16)


def patched(blob, offset, fmt, value):
    b = bytearray(blob)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def test_container_rejections(tmae):
    """each from a one-field corruption of a valid file, each with its own message"""
    from textmae_amd import bitstream as bs

    blob, ids, z, y = make_file(tmae)
    cases = [
        (patched(blob, 0, "<3s", b"TMX"), r"not a TMT bitstream \(magic b'TMX'\)"),
        (patched(blob, 3, "<B", 2), r"container version 2, this reader knows version 1"),
        (blob[:-2], r"not a whole number of 32-bit words"),
        (patched(blob, 8, "<B", 5), r"patch_size 5 does not divide img_size 32"),
        (patched(blob, 6, "<H", 5), r"num_keep_patches 5 outside 1\.\.4"),
        (patched(blob, 9, "<B", 0x27), r"lane fields 2\^7 / 2\^2: at most 2\^6 lanes"),
        (patched(blob, 9, "<B", 0x72), r"lane fields 2\^2 / 2\^7: at most 2\^6 lanes"),
        (patched(blob, 10, "<H", 17), r"overlap 17 above half the tile size 32"),
        (patched(blob, 12, "<H", 0), r"image size 0x40: width and height must be >= 1"),
        (patched(blob, 14, "<H", 0), r"image size 70x0: width and height must be >= 1"),
        (patched(blob, 16, "<H", 0), r"chunk 0"),
        (patched(blob, 18, "<H", 1), r"reserved bytes 18-19 hold 0x0001"),
        (patched(blob, 20, "<I", 5), r"5 tiles, but 70x40 at tile size 32, overlap 8 has 2 x 3 = 6"),
        (patched(blob, 20, "<I", 4097), r"4097 tiles: at most 4096"),
        (patched(blob, 12, "<H", 90), r"6 tiles, but 90x40 at tile size 32, overlap 8 has 2 x 4 = 8"),
        (blob[:24 + 8 * 6 - 4], r"68 bytes: the header and the table of 6 tiles take 72"),
        (blob[:20], r"20 bytes: shorter than the 24-byte header"),
        (patched(blob, 24 + 8 * 2, "<I", 1), r"tile 2: z record of 1 and y record of 5 words"),
        (patched(blob, 24 + 8 * 3 + 4, "<I", 0), r"tile 3: z record of 5 and y record of 0 words"),
        (patched(blob, 24 + 8 * 4 + 4, "<I", 4), r"the header, the table and the 6 tiles it lists take"),
        (blob + b"\0\0\0\0", r"the header, the table and the 6 tiles it lists take"),
        (blob[:-4], r"the header, the table and the 6 tiles it lists take"),
    ]
    seen = set()
    for bad, pattern in cases:
        with pytest.raises(ValueError, match=pattern) as e:
            bs.parse_image(bad)
        seen.add(str(e.value))
    assert len(seen) == len(cases)
    bs.parse_image(blob)  # and the file they came from is fine


def test_assemble_image_rejects(tmae):
    from textmae_amd import bitstream as bs

    blob, ids, z, y = make_file(tmae)
    args = [32, 3, 16, 4, 2, 8, 70, 40, 5, ids, z, y]

    def call(i, v):
        a = list(args)
        a[i] = v
        return bs.assemble_image(*a)

    assert call(0, 32) == blob
    with pytest.raises(ValueError, match="overlap 17 outside"):
        call(5, 17)
    with pytest.raises(ValueError, match="chunk 0"):
        call(8, 0)
    with pytest.raises(ValueError, match="for 6 tiles"):
        call(10, z[:5])
    with pytest.raises(ValueError, match="tile 0: records are whole 32-bit words"):
        call(11, [b"\0" * 6] + y[1:])
    with pytest.raises(ValueError, match="does not fit the header"):
        call(6, 0)
    with pytest.raises(ValueError, match="lanes = 3"):
        call(3, 3)
