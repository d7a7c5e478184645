"""Region decode, host part (CPU only): tiling.region_tiles against brute force and against the
numpy blend with every unlisted tile poisoned, and bitstream.read_image_index / read_tiles against parse_image,
with the bytes they read counted."""
import io
import struct

import numpy as np
import pytest

IMAGES = [(16, 16), (1, 1), (17, 16), (16, 17), (29, 41), (41, 29), (15, 50)]  # (H, W): test_gpu_tiled.py's
OVERLAPS = (0, 1, 4, 8)
S = 16


def windows_of(H, W, rng, n=50):
    """(x0, y0, w, h): the full image, the four corner pixels, n seeded windows"""
    out = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)]
    for _ in range(n):
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        out.append((x0, y0, int(rng.integers(1, W - x0 + 1)), int(rng.integers(1, H - y0 + 1))))
    return out


@pytest.mark.parametrize("O", OVERLAPS)
def test_region_tiles_brute_force(tmae, O):
    """the list is the union of the covering() products over every pixel of the window, and the blend of the listed
    tiles alone (every other tile NaN) is the window of the full blend bit for bit"""
    from textmae_amd import tiling

    rng = np.random.default_rng(700 + O)
    for H, W in IMAGES:
        g = tiling.grid(H, W, S, O)
        tiles = rng.uniform(-0.5, 1.5, (g.T, 3, S, S)).astype(np.float32)
        full = tiling.tile_blend_host(tiles, H, W, O)
        assert np.isfinite(full).all()
        for x0, y0, w, h in windows_of(H, W, rng):
            got = tiling.region_tiles(g, x0, y0, w, h)
            brute = set()
            for y in range(y0, y0 + h):
                for x in range(x0, x0 + w):
                    brute |= {ty * g.nx + tx for ty in tiling.covering(y, g.ny, g.stride, O)
                              for tx in tiling.covering(x, g.nx, g.stride, O)}
            assert got == sorted(brute), (H, W, O, x0, y0, w, h)
            poisoned = np.full_like(tiles, np.nan)
            poisoned[got] = tiles[got]
            part = tiling.tile_blend_host(poisoned, H, W, O)[:, y0:y0 + h, x0:x0 + w]
            assert np.array_equal(part, full[:, y0:y0 + h, x0:x0 + w]), (H, W, O, x0, y0, w, h)


def test_region_tiles_rejects(tmae):
    from textmae_amd import tiling

    g = tiling.grid(29, 41, S, 4)
    assert tiling.region_tiles(g, 0, 0, 41, 29) == list(range(g.T))
    for x0, y0, w, h in [(0, 0, 0, 5), (0, 0, 5, 0), (0, 0, 5, -1)]:
        with pytest.raises(ValueError, match="both sizes must be >= 1"):
            tiling.region_tiles(g, x0, y0, w, h)
    for x0, y0, w, h in [(-1, 0, 5, 5), (0, -1, 5, 5), (37, 0, 5, 5), (0, 25, 5, 5), (41, 0, 1, 1), (0, 0, 42, 29)]:
        with pytest.raises(ValueError, match="is not inside the image of 41x29"):
            tiling.region_tiles(g, x0, y0, w, h)


# ------------------------------------------------------------------------------------------------ container
GEO = dict(img_size=32, K=3, patch=16, lanes=4, z_lanes=2, overlap=8, width=70, height=40, chunk=5)


def make_file():
    """test_tiled_host.py's file: 2 x 3 tiles (32 px tiles, overlap 8, 70 x 40 image), records of different lengths"""
    from textmae_amd import bitstream as bs
    from textmae_amd import tiling

    g = tiling.grid(GEO["height"], GEO["width"], GEO["img_size"], GEO["overlap"])
    assert (g.ny, g.nx) == (2, 3)
    rng = np.random.default_rng(5)
    W = bs.id_words((GEO["img_size"] // GEO["patch"]) ** 2, GEO["K"])
    ids = rng.integers(0, 1 << 32, (g.T, W), dtype=np.uint64).astype(np.uint32)
    z = [rng.integers(0, 256, 4 * (2 + t), dtype=np.uint8).tobytes() for t in range(g.T)]
    y = [rng.integers(0, 256, 4 * (7 - t), dtype=np.uint8).tobytes() for t in range(g.T)]
    return bs.assemble_image(GEO["img_size"], GEO["K"], GEO["patch"], GEO["lanes"], GEO["z_lanes"], GEO["overlap"],
                             GEO["width"], GEO["height"], GEO["chunk"], ids, z, y)


class CountingFile(io.BytesIO):
    """a file object that counts the bytes its read() returns"""
    nread = 0

    def read(self, size=-1):
        b = super().read(size)
        self.nread += len(b)
        return b


def test_index_and_tiles_equal_parse_image(tmae):
    from textmae_amd import bitstream as bs

    blob = make_file()
    p = bs.parse_image(blob)
    for src in (blob, bytearray(blob), memoryview(blob), io.BytesIO(blob)):
        idx = bs.read_image_index(src)
        assert (idx.img_size, idx.num_keep_patches, idx.patch_size, idx.lanes, idx.z_lanes, idx.overlap, idx.width,
                idx.height, idx.chunk) == tuple(p[:9])
        assert (idx.num_tiles, idx.nbytes) == (6, len(blob))
        at = 24 + 8 * 6
        for t in range(6):  # the offsets are the prefix sums of the table
            assert (idx.ids_at[t], idx.z_at[t], idx.y_at[t]) == (at, at + 4 * p.ids[t].size,
                                                                  at + 4 * p.ids[t].size + len(p.z[t]))
            at = idx.y_at[t] + len(p.y[t])
            assert idx.end_at[t] == at
        for tiles in (range(6), [4], [5, 0, 3], [2, 2]):
            ids, z, y = bs.read_tiles(src, idx, tiles)
            assert len(ids) == len(z) == len(y) == len(tiles)
            for k, t in enumerate(tiles):
                assert ids[k].dtype == np.uint32 and np.array_equal(ids[k], p.ids[t])
                assert bytes(z[k]) == bytes(p.z[t]) and bytes(y[k]) == bytes(p.y[t])
        for t in (-1, 6):
            with pytest.raises(ValueError, match=f"tile {t} outside 0..5"):
                bs.read_tiles(src, idx, [t])
    with pytest.raises(ValueError, match="but the index is of a file of"):
        bs.read_tiles(blob + b"\0" * 4, bs.read_image_index(blob), [0])


def test_only_the_needed_bytes_are_read(tmae):
    from textmae_amd import bitstream as bs

    blob = make_file()
    p = bs.parse_image(blob)
    f = CountingFile(blob)
    idx = bs.read_image_index(f)
    assert f.nread == 24 + 8 * 6  # the header and the table
    ids, z, y = bs.read_tiles(f, idx, [4])
    tile4 = 4 * p.ids[4].size + len(p.z[4]) + len(p.y[4])
    assert f.nread <= 24 + 8 * 6 + tile4 < len(blob)
    assert np.array_equal(ids[0], p.ids[4]) and bytes(z[0]) == bytes(p.z[4]) and bytes(y[0]) == bytes(p.y[4])


def patched(blob, offset, fmt, value):
    b = bytearray(blob)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def test_index_rejections(tmae):
    """every malformed field raises from read_image_index what it raises from parse_image, from bytes and from a file
    object, and never by reading a tile"""
    from textmae_amd import bitstream as bs

    blob = make_file()
    cases = [
        (patched(blob, 0, "<3s", b"TMX"), r"not a TMT bitstream \(magic b'TMX'\)"),
        (patched(blob, 0, "<3s", b"TMC"), r"not a TMT bitstream \(magic b'TMC'\)"),
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
        with pytest.raises(ValueError, match=pattern) as want:
            bs.parse_image(bad)
        with pytest.raises(ValueError, match=pattern) as e:
            bs.read_image_index(bad)
        assert str(e.value) == str(want.value)
        f = CountingFile(bad)
        with pytest.raises(ValueError, match=pattern) as e:
            bs.read_image_index(f)
        assert str(e.value) == str(want.value)
        assert f.nread <= 24 + 8 * 6
        seen.add(str(e.value))
    assert len(seen) == len(cases)
    assert bs.read_image_index(blob).num_tiles == 6  # and the file they came from is fine


def test_library_validates_before_launch(tmae):
    """tmae_tile_blend_crops checks what it can see on the host, so this needs no GPU: every call returns before a
    launch"""
    from textmae_amd import _lib

    def crops(N=1, map_len=1, R=1, h=4, w=4, S=16, O=4, ptr=4096, f32=4096, u8=None):
        return _lib.call("tmae_tile_blend_crops", ptr, N, ptr, map_len, ptr, R, h, w, S, O, f32, u8, None)

    with pytest.raises(ValueError, match="overlap 9 outside"):
        crops(O=9)
    with pytest.raises(ValueError, match="tile size 0 outside"):
        crops(S=0, O=0)
    with pytest.raises(ValueError, match=r"0 windows of 4x4 pixels, all three must be >= 1"):
        crops(R=0)
    with pytest.raises(ValueError, match=r"1 windows of 0x4 pixels"):
        crops(h=0)
    with pytest.raises(ValueError, match=r"1 windows of 4x0 pixels"):
        crops(w=0)
    with pytest.raises(ValueError, match=r"0 tile slots and 1 map entries"):
        crops(N=0)
    with pytest.raises(ValueError, match=r"1 tile slots and 0 map entries"):
        crops(map_len=0)
    with pytest.raises(ValueError, match="tiles / map / desc are NULL"):
        crops(ptr=None)
    with pytest.raises(ValueError, match="out_f32 and out_u8 are both NULL"):
        crops(f32=None)
    with pytest.raises(ValueError, match="exceed the launch grid"):
        crops(h=1 << 16, w=1 << 16)
    with pytest.raises(ValueError, match="exceed the launch grid"):
        crops(R=1 << 30, h=1 << 10, w=1 << 10)
