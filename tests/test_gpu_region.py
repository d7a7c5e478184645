"""Region decode on the GPU: the crops blend kernel against crops of the whole-image blend, and
MCM.decode_region / decode_crops / codec decode --region against crops of MCM.decode_image.  Every comparison is an
equality: a window runs the same per-pixel arithmetic on the same decoded tiles."""
import numpy as np
import pytest
import torch

from oracle.mcm_oracle import MCMConfig, make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the cases, the guard and the model of test_gpu_tiled.py
IMAGES = [(16, 16), (1, 1), (17, 16), (16, 17), (29, 41), (41, 29), (15, 50)]  # (H, W)
KERNEL_CASES = [(16, O, IMAGES) for O in (0, 1, 4, 8)] + [(128, 32, [(200, 300)])]
GUARD = 256
SMALL12 = dict(img_size=128, patch_size=16, encoder_embed_dim=128, encoder_depth=1, encoder_num_heads=2,
               decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2, latent_depth=192, hyperprior_depth=96,
               num_slices=12, num_keep_patches=16)


def guarded(shape, dtype):
    """(buffer, view): a tensor of this shape inside a byte buffer with GUARD bytes of 0xA5 on either side"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((2 * GUARD + n,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(shape)


def intact(buf):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())


def compact(tiles, g, windows, size, rng):
    """(buffer, slots): only the tiles the windows (x0, y0) of one size need, in a shuffled slot order, plus one slot
    of NaN that no tile maps to"""
    from textmae_amd import tiling

    need = sorted({t for x0, y0 in windows for t in tiling.region_tiles(g, x0, y0, size[0], size[1])})
    order = rng.permutation(len(need) + 1)
    buf = torch.full((len(need) + 1,) + tuple(tiles.shape[1:]), float("nan"), dtype=torch.float32, device=DEV)
    slots = [-1] * g.T
    for t, s in zip(need, order[:-1]):
        slots[t] = int(s)
        buf[int(s)] = tiles[t]
    return buf, slots


def origins_of(H, W, w, h, rng, n=3):
    """n seeded origins of a w x h window, and the one that touches the image's last row and column"""
    return [(int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))) for _ in range(n)] + [(W - w, H - h)]


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("S,O,sizes", KERNEL_CASES, ids=[f"S{S}-O{O}" for S, O, _ in KERNEL_CASES])
def test_crops_are_crops_of_the_blend(tmae, S, O, sizes):
    from textmae_amd import ops, tiling

    rng = np.random.default_rng(300 * S + O)
    for H, W in sizes:
        g = tiling.grid(H, W, S, O)
        tiles = torch.from_numpy(rng.uniform(-0.5, 1.5, (g.T, 3, S, S)).astype(np.float32)).to(DEV)
        full, full_u8 = ops.tile_blend(tiles, H, W, O, out="both")
        shapes = [(W, H), (1, 1), (min(W, 5), min(H, 7))] + \
            [(int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))) for _ in range(2)]
        for w, h in shapes:
            windows = origins_of(H, W, w, h, rng)
            buf, slots = compact(tiles, g, windows, (w, h), rng)
            want = torch.stack([full[:, y0:y0 + h, x0:x0 + w] for x0, y0 in windows])
            want_u8 = torch.stack([full_u8[y0:y0 + h, x0:x0 + w] for x0, y0 in windows])
            args = (buf, [(H, W, slots)], [(0, x0, y0) for x0, y0 in windows], (w, h), O)
            got = ops.tile_blend_crops(*args)
            assert got.dtype == torch.float32 and tuple(got.shape) == (len(windows), 3, h, w)
            assert torch.equal(got, want), (H, W, w, h)  # no NaN: no unlisted tile was read
            u8 = ops.tile_blend_crops(*args, out="u8")
            assert u8.dtype == torch.uint8 and tuple(u8.shape) == (len(windows), h, w, 3)
            assert torch.equal(u8, want_u8), (H, W, w, h)
            fbuf, fview = guarded(tuple(want.shape), torch.float32)
            ubuf, uview = guarded(tuple(want_u8.shape), torch.uint8)
            both = ops.tile_blend_crops(*args, out="both", out_f32=fview, out_u8=uview)
            assert both[0].data_ptr() == fview.data_ptr() and both[1].data_ptr() == uview.data_ptr()
            assert torch.equal(both[0], want) and torch.equal(both[1], want_u8), (H, W, w, h)
            assert intact(fbuf) and intact(ubuf), (H, W, w, h)


@pytest.mark.parametrize("O", [0, 1, 4, 8])
def test_windows_of_several_images_in_one_launch(tmae, O):
    """windows of 5 rows x 7 columns from three images whose tiles share one compact buffer"""
    from textmae_amd import ops, tiling

    S, w, h = 16, 7, 5
    rng = np.random.default_rng(900 + O)
    images, windows, want, want_u8, parts, base = [], [], [], [], [], 0
    for k, (H, W) in enumerate([(29, 41), (41, 29), (15, 50)]):
        g = tiling.grid(H, W, S, O)
        tiles = torch.from_numpy(rng.uniform(-0.5, 1.5, (g.T, 3, S, S)).astype(np.float32)).to(DEV)
        full, full_u8 = ops.tile_blend(tiles, H, W, O, out="both")
        mine = origins_of(H, W, w, h, rng, n=2) + [(W - w, 0), (0, H - h)]
        buf, slots = compact(tiles, g, mine, (w, h), rng)
        images.append((H, W, [s + base if s >= 0 else -1 for s in slots]))
        parts.append(buf)
        base += buf.shape[0]
        for x0, y0 in mine:
            windows.append((k, x0, y0))
            want.append(full[:, y0:y0 + h, x0:x0 + w])
            want_u8.append(full_u8[y0:y0 + h, x0:x0 + w])
    order = rng.permutation(len(windows))  # the windows of the images interleaved
    windows = [windows[i] for i in order]
    got, u8 = ops.tile_blend_crops(torch.cat(parts), images, windows, (w, h), O, out="both")
    assert torch.equal(got, torch.stack([want[i] for i in order]))
    assert torch.equal(u8, torch.stack([want_u8[i] for i in order]))


def test_one_pixel_image(tmae):
    from textmae_amd import ops

    for O in (0, 8):
        tiles = torch.from_numpy(np.random.default_rng(O).uniform(-0.5, 1.5, (1, 3, 16, 16)).astype(np.float32)).to(DEV)
        got, u8 = ops.tile_blend_crops(tiles, [(1, 1, [0])], [(0, 0, 0)], (1, 1), O, out="both")
        full, full_u8 = ops.tile_blend(tiles, 1, 1, O, out="both")
        assert torch.equal(got, full[None]) and torch.equal(u8, full_u8[None])
        assert torch.equal(got[0, :, 0, 0], tiles[0, :, 0, 0])


def test_argument_errors(tmae):
    """each raises on the host, before anything is uploaded or launched"""
    from textmae_amd import ops

    tiles = torch.zeros((6, 3, 16, 16), dtype=torch.float32, device=DEV)  # 20 x 30 at S 16, O 4: 2 x 3 tiles
    img = (20, 30, [0, 1, 2, 3, 4, 5])

    def call(images=(img,), windows=((0, 0, 0),), size=(8, 8), O=4, t=tiles, **kw):
        return ops.tile_blend_crops(t, list(images), list(windows), size, O, **kw)

    for win in [(0, 23, 0), (0, 0, 13), (0, -1, 0), (0, 30, 20)]:
        with pytest.raises(ValueError, match=r"window 0: window 8x8 at .* is not inside the image of 30x20"):
            call(windows=[win])
    with pytest.raises(ValueError, match=r"window 1: window 8x8 at \(25, 0\)"):
        call(windows=[(0, 0, 0), (0, 25, 0)])
    with pytest.raises(ValueError, match="both sizes must be >= 1"):
        call(size=(0, 8))
    with pytest.raises(ValueError, match="window 0: needs tile 1 of image 0, which has no slot"):
        call(images=[(20, 30, [0, -1, 2, 3, 4, 5])], windows=[(0, 8, 0)])  # columns 8..15 reach into tile 1
    assert call(images=[(20, 30, [0, -1, 2, 3, 4, 5])], windows=[(0, 0, 0)], size=(8, 8)).shape == (1, 3, 8, 8)
    with pytest.raises(ValueError, match="slots must be -1 or one of the buffer's 6"):
        call(images=[(20, 30, [0, 1, 2, 3, 4, 6])])
    with pytest.raises(ValueError, match="image 0: 5 slots, but 20x30"):
        call(images=[(20, 30, [0, 1, 2, 3, 4])])
    with pytest.raises(ValueError, match="window 0: image 1 outside 0..0"):
        call(windows=[(1, 0, 0)])
    with pytest.raises(ValueError, match="no windows"):
        call(windows=[])
    with pytest.raises(ValueError, match="overlap 9 outside"):
        call(O=9)
    with pytest.raises(ValueError, match="out must be"):
        call(out="bf16")
    with pytest.raises(ValueError, match=r"out_f32 must be \[1, 3, 8, 8\]"):
        call(out_f32=torch.zeros((3, 8, 8), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match=r"out_u8 must be \[1, 8, 8, 3\]"):
        call(out="u8", out_u8=torch.zeros((1, 3, 8, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="must be torch.float32"):
        call(t=tiles.half())
    with pytest.raises(ValueError, match=r"f32 \[N >= 1, 3, S, S\]"):
        call(t=tiles[:, :, :8].contiguous())


# ------------------------------------------------------------------------------------------------ model
H0, W0, O0 = 200, 300, 32  # 2 x 3 tiles of 128 at overlap 32
H1, W1 = 150, 140          # 2 x 2 tiles
WINDOWS = [  # (x0, y0, w, h) and the tiles tiling.region_tiles must name
    ((0, 0, 96, 96), [0]),
    ((100, 10, 50, 40), [0, 1]),
    ((90, 90, 20, 20), [0, 1, 3, 4]),
    ((230, 130, 70, 70), [5]),
    ((0, 0, W0, H0), [0, 1, 2, 3, 4, 5]),
    ((299, 199, 1, 1), [5]),
]


@pytest.fixture(scope="module")
def small(tmae):
    cfg = MCMConfig(**SMALL12)
    m = tmae.MCM(**cfg.kwargs())
    sd = m.state_dict()
    sd.update(make_state_dict(cfg, 11))
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.update(force=True)
    return m


@pytest.fixture(scope="module")
def coded(small):
    """per lanes (1, 4): (the file of the seeded 200 x 300 image, its decode_image); computed once, left unchanged"""
    image = np.random.default_rng(41).integers(0, 256, (H0, W0, 3), dtype=np.uint8)
    out = {}
    for lanes in (1, 4):
        blob = small.encode_image(image, overlap=O0, lanes=lanes, tile_batch=6)
        out[lanes] = (blob, small.decode_image(blob).clone())
    return out


@pytest.fixture(scope="module")
def coded_second(small):
    """(the file of a seeded 150 x 140 image coded at lanes 4, its decode_image)"""
    image = np.random.default_rng(42).integers(0, 256, (H1, W1, 3), dtype=np.uint8)
    blob = small.encode_image(image, overlap=O0, lanes=4, tile_batch=4)
    return blob, small.decode_image(blob).clone()


@pytest.fixture
def spy(small, monkeypatch):
    """the numbers of tiles the calls of _decode_sections were given"""
    seen, real = [], small._decode_sections

    def counted(ids, *args, **kw):
        seen.append(len(ids))
        return real(ids, *args, **kw)

    monkeypatch.setattr(small, "_decode_sections", counted)
    return seen


def with_duplicate_id(blob, t):
    """the file rebuilt with a repeated patch id in tile t, as test_gpu_tiled.py's test_corrupt_tiles_are_named"""
    from textmae_amd import bitstream as bs

    p = bs.parse_image(blob)
    keep = bs.unpack_ids_host(p.ids[t], 64, 16)[0][:16].copy()
    keep[3] = keep[12]
    ids = list(p.ids)
    ids[t] = bs.pack_ids_host(keep, 64)
    dup = bs.assemble_image(p.img_size, p.num_keep_patches, p.patch_size, p.lanes, p.z_lanes, p.overlap, p.width,
                            p.height, p.chunk, np.stack(ids), p.z, p.y)
    assert len(dup) == len(blob) and dup != blob
    return dup


class CountingFile:
    """a binary file object that counts the bytes read from it"""

    def __init__(self, path):
        self.f, self.nread = open(path, "rb"), 0

    def seek(self, *args):
        return self.f.seek(*args)

    def read(self, size=-1):
        b = self.f.read(size)
        self.nread += len(b)
        return b

    def close(self):
        self.f.close()


@pytest.mark.parametrize("lanes", [1, 4])
def test_region_is_the_crop_of_the_image(tmae, small, coded, spy, lanes):
    from textmae_amd import tiling

    blob, full = coded[lanes]
    g = tiling.grid(H0, W0, 128, O0)
    for (x0, y0, w, h), tiles in WINDOWS:
        assert tiling.region_tiles(g, x0, y0, w, h) == tiles
        del spy[:]
        got = small.decode_region(blob, x0, y0, w, h)
        assert sum(spy) == len(tiles), (x0, y0, w, h)  # only the needed tiles went through the model
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, h, w)
        assert torch.equal(got, full[:, y0:y0 + h, x0:x0 + w]), (x0, y0, w, h)
        u8 = small.decode_region(blob, x0, y0, w, h, out="u8")
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (h, w, 3)
        assert torch.equal(u8, got.clamp(0, 1).mul(255).round().byte().permute(1, 2, 0)), (x0, y0, w, h)
    # chunks of 1 and of 3 (the four tiles as 3 + 1) decode the same
    x0, y0, w, h = WINDOWS[2][0]
    for n, calls in ((1, [1, 1, 1, 1]), (3, [3, 1])):
        del spy[:]
        assert torch.equal(small.decode_region(blob, x0, y0, w, h, tile_batch=n), full[:, y0:y0 + h, x0:x0 + w])
        assert spy == calls


def test_a_corrupt_tile_matters_only_where_it_is_needed(tmae, small, coded):
    blob, full = coded[1]
    dup = with_duplicate_id(blob, 5)
    with pytest.raises(ValueError, match=r"side information of tile 5: duplicate"):
        small.decode_image(dup)
    for (x0, y0, w, h), tiles in WINDOWS[:2]:  # tiles 0 / 1: tile 5 is never read
        assert torch.equal(small.decode_region(dup, x0, y0, w, h), full[:, y0:y0 + h, x0:x0 + w])
    with pytest.raises(ValueError, match=r"side information of tile 5: duplicate"):
        small.decode_region(dup, 230, 130, 70, 70)
    with pytest.raises(ValueError, match=r"side information of tile 5: duplicate"):
        small.decode_region(dup, 90, 90, 200, 100, tile_batch=2)  # tiles 0 1 2 3 4 5: image 1 of the third call
    assert torch.equal(small.decode_region(blob, 230, 130, 70, 70), full[:, 130:200, 230:300])


def test_region_errors(tmae, small, coded):
    from textmae_amd import bitstream as bs
    from textmae_amd import tiling

    blob, _ = coded[1]
    for x0, y0, w, h in [(231, 130, 70, 70), (0, 131, 70, 70), (-1, 0, 5, 5), (300, 0, 1, 1)]:
        with pytest.raises(ValueError, match="is not inside the image of 300x200"):
            small.decode_region(blob, x0, y0, w, h)
    with pytest.raises(ValueError, match="both sizes must be >= 1"):
        small.decode_region(blob, 0, 0, 0, 5)
    with pytest.raises(ValueError, match="decode_region: out must be 'f32' or 'u8'"):
        small.decode_region(blob, 0, 0, 5, 5, out="both")
    with pytest.raises(ValueError, match="decode_region: tile_batch 0 must be >= 1"):
        small.decode_region(blob, 0, 0, 5, 5, tile_batch=0)
    with pytest.raises(ValueError, match="not a TMT bitstream"):
        small.decode_region(b"TMC\x01" + b"\0" * 28, 0, 0, 5, 5)
    g = tiling.grid(H0, W0, 160, O0)
    rec = [b"\0" * 8] * g.T
    other = bs.assemble_image(160, 16, 16, 1, 1, O0, W0, H0, 6, np.zeros((g.T, bs.id_words(100, 16)), np.uint32), rec,
                              rec)
    with pytest.raises(ValueError, match=r"^coded for img_size 160, patch_size 16, num_keep_patches 16; this model "
                                         r"has 128, 16, 16$"):
        small.decode_region(other, 0, 0, 5, 5)


def test_region_from_a_file_object(tmae, small, coded, tmp_path):
    blob, full = coded[4]
    path = tmp_path / "image.tmt"
    path.write_bytes(blob)
    with open(path, "rb") as f:
        assert torch.equal(small.decode_region(f, 100, 10, 50, 40), small.decode_region(blob, 100, 10, 50, 40))
    f = CountingFile(path)
    try:
        got = small.decode_region(f, 230, 130, 70, 70)  # tile 5 alone
    finally:
        f.close()
    assert torch.equal(got, full[:, 130:200, 230:300])
    from textmae_amd import bitstream as bs

    idx = bs.read_image_index(blob)
    print(f"one-tile window: {f.nread} of {len(blob)} bytes read")
    assert f.nread == 24 + 8 * 6 + int(idx.end_at[5] - idx.ids_at[5]) < len(blob)


CROPS = [(0, (0, 0)), (1, (0, 0)), (0, (50, 40)), (0, (150, 100)), (1, (100, 120))]  # (file, (x0, y0)), 40 x 30 each


def test_crops_of_two_files(tmae, small, coded, coded_second, spy):
    """five windows of 40 x 30 from a lanes-1 and a lanes-4 file, two of them inside tile 0 of the first"""
    from textmae_amd import tiling

    files = [coded[1], coded_second]
    grids = [tiling.grid(H0, W0, 128, O0), tiling.grid(H1, W1, 128, O0)]
    assert (grids[1].ny, grids[1].nx) == (2, 2)
    w, h = 40, 30
    assert tiling.region_tiles(grids[0], 0, 0, w, h) == tiling.region_tiles(grids[0], 50, 40, w, h) == [0]
    union = [set(), set()]
    for k, (x0, y0) in CROPS:
        union[k] |= set(tiling.region_tiles(grids[k], x0, y0, w, h))
    assert [sorted(u) for u in union] == [[0, 1, 4], [0, 1, 2, 3]]
    srcs = [files[k][0] for k, _ in CROPS]
    origins = [o for _, o in CROPS]
    want = torch.stack([files[k][1][:, y0:y0 + h, x0:x0 + w] for k, (x0, y0) in CROPS])
    del spy[:]
    got = small.decode_crops(srcs, origins, (w, h))
    assert spy == [3, 4]  # per file the union of its windows' tiles, once; the lanes in calls of their own
    assert got.dtype == torch.float32 and tuple(got.shape) == (5, 3, h, w)
    assert torch.equal(got, want)
    u8 = small.decode_crops(srcs, origins, (w, h), out="u8")
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (5, h, w, 3)
    assert torch.equal(u8, want.clamp(0, 1).mul(255).round().byte().permute(0, 2, 3, 1))
    del spy[:]
    assert torch.equal(small.decode_crops(srcs, origins, (w, h), tile_batch=2), want)
    assert spy == [2, 1, 2, 2]
    # two files of equal lanes share a batch
    both4 = [coded[4], coded_second]
    del spy[:]
    got = small.decode_crops([both4[k][0] for k, _ in CROPS], origins, (w, h))
    assert spy == [7]
    assert torch.equal(got, torch.stack([both4[k][1][:, y0:y0 + h, x0:x0 + w] for k, (x0, y0) in CROPS]))


def test_crops_errors(tmae, small, coded, coded_second):
    blob, full = coded[1]
    with pytest.raises(ValueError, match="2 sources but 1 origins"):
        small.decode_crops([blob, blob], [(0, 0)], (40, 30))
    with pytest.raises(ValueError, match="decode_crops: no windows"):
        small.decode_crops([], [], (40, 30))
    with pytest.raises(ValueError, match="source 1: not a TMT bitstream"):
        small.decode_crops([blob, b"TMC\x01" + b"\0" * 28], [(0, 0), (0, 0)], (40, 30))
    with pytest.raises(ValueError, match="source 2: window 40x30 at .* is not inside the image of 140x150"):
        small.decode_crops([blob, blob, coded_second[0]], [(0, 0), (260, 170), (101, 120)], (40, 30))
    with pytest.raises(ValueError, match="decode_crops: out must be"):
        small.decode_crops([blob], [(0, 0)], (40, 30), out="both")
    dup = with_duplicate_id(blob, 5)
    with pytest.raises(ValueError, match=r"side information of tile 5 of source 1: duplicate"):
        small.decode_crops([blob, dup, blob], [(0, 0), (260, 170), (10, 10)], (40, 30))
    # the same file where no window needs tile 5
    got = small.decode_crops([blob, dup], [(0, 0), (10, 10)], (40, 30))
    assert torch.equal(got, torch.stack([full[:, 0:30, 0:40], full[:, 10:40, 10:50]]))


# ------------------------------------------------------------------------------------------------ command line
def test_codec_cli_region(tmae, tmp_path, monkeypatch):
    """decode --region writes the crop of the PNG the plain decode writes.  The command lines of this test share one
    model (each would load the same checkpoint again), which keeps it to a few seconds."""
    from PIL import Image

    from textmae_amd import codec

    load, models = codec._model, {}

    def loaded_once(*key):
        if key not in models:
            models[key] = load(*key)
        return models[key]

    monkeypatch.setattr(codec, "_model", loaded_once)
    rng = np.random.default_rng(31)
    ds = tmp_path / "one"
    ds.mkdir()
    yy, xx = np.mgrid[0:200, 0:300]
    a = np.stack([127 + 120 * np.sin(xx / (7.0 + 3 * c)) * np.cos(yy / 5.0 + c) for c in range(3)], -1)
    Image.fromarray(np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)).save(ds / "img0.png")
    cfg = MCMConfig(img_size=224, num_keep_patches=144)
    sd = tmae.MCM(**cfg.kwargs()).state_dict()
    sd.update(make_state_dict(cfg, 17))
    ck = tmp_path / "best_model.pth"
    torch.save({"model": sd}, ck)
    tmt, png, crop = tmp_path / "tmt", tmp_path / "png", tmp_path / "crop"
    assert codec.main(["encode", "-c", str(ck), "-d", str(ds), "-o", str(tmt), "--tiled"]) == 1
    assert [f.name for f in tmt.iterdir()] == ["img0.tmt"]
    assert codec.main(["decode", "-c", str(ck), "-d", str(tmt), "-o", str(png)]) == 1
    assert codec.main(["decode", "-c", str(ck), "-d", str(tmt), "-o", str(crop), "--region", "100,10,50,40"]) == 1
    whole, part = Image.open(png / "img0.png"), Image.open(crop / "img0.png")
    assert whole.size == (300, 200) and part.size == (50, 40)
    assert np.array_equal(np.array(part), np.array(whole)[10:50, 100:150])
    with pytest.raises(ValueError, match=r"img0\.tmt: window 50x40 at \(260, 10\) is not inside the image of 300x200"):
        codec.main(["decode", "-c", str(ck), "-d", str(tmt), "-o", str(crop), "--region", "260,10,50,40"])
    assert len(models) == 1
