"""Tiled full-resolution codec on the GPU: the cut / blend kernels (csrc/tile.hip) against the numpy oracle of
textmae_amd.tiling, MCM.encode_image / decode_image against encode_bytes / decode_bytes of the same tiles (every
comparison an equality: the file carries the same sections and the decoder runs the same path), and the command
lines (codec encode --tiled / decode, testing.main --tiled)."""
import json

import numpy as np
import pytest
import torch

from oracle.mcm_oracle import MCMConfig, make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"

IMAGES = [(16, 16), (1, 1), (17, 16), (16, 17), (29, 41), (41, 29), (15, 50)]  # (H, W)
KERNEL_CASES = [(16, O, IMAGES) for O in (0, 1, 4, 8)] + [(128, 32, [(200, 300)])]
GUARD = 256
# SMALL12 of test_gpu_bitstream.py
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


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("S,O,sizes", KERNEL_CASES, ids=[f"S{S}-O{O}" for S, O, _ in KERNEL_CASES])
def test_cut_against_host_oracle(tmae, S, O, sizes):
    from textmae_amd import ops, tiling

    rng = np.random.default_rng(100 * S + O)
    for H, W in sizes:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        src = torch.from_numpy(img).to(DEV)
        want_u8 = torch.from_numpy(tiling.tile_cut_host(img, S, O))  # [T, S, S, 3]
        T = want_u8.shape[0]
        assert T == tiling.grid(H, W, S, O).T
        tbuf, tview = guarded((T, 3, S, S), torch.float32)
        gbuf, gview = guarded((T, S, S), torch.uint8)
        tiles, gray = ops.tile_cut_u8(src, S, O, tiles=tview, gray=gview)
        assert tiles.dtype == torch.float32 and tuple(tiles.shape) == (T, 3, S, S)
        assert gray.dtype == torch.uint8 and tuple(gray.shape) == (T, S, S)
        assert torch.equal(tiles.cpu(), want_u8.permute(0, 3, 1, 2).float().div(255)), (H, W)
        assert torch.equal(gray, ops.rgb_to_gray_u8(want_u8.to(DEV))), (H, W)
        assert intact(tbuf) and intact(gbuf), (H, W)
        fresh_t, fresh_g = ops.tile_cut_u8(src, S, O)
        assert torch.equal(fresh_t, tiles) and torch.equal(fresh_g, gray)
        if T > 1:
            sub_t, sub_g = ops.tile_cut_u8(src, S, O, t0=1, nt=T - 1)
            assert torch.equal(sub_t, tiles[1:]) and torch.equal(sub_g, gray[1:]), (H, W)


@pytest.mark.parametrize("S,O,sizes", KERNEL_CASES, ids=[f"S{S}-O{O}" for S, O, _ in KERNEL_CASES])
def test_blend_against_host_oracle(tmae, S, O, sizes):
    """tiles that do not agree in their overlaps.  The f32 bound is derived: at most 4 products, 3 adds and 1 divide,
    under 8 roundings of 2^-24 = 4.8e-7 relative to the largest tile value"""
    from textmae_amd import ops, tiling

    rng = np.random.default_rng(200 * S + O)
    for H, W in sizes:
        g = tiling.grid(H, W, S, O)
        tiles_h = rng.uniform(-0.5, 1.5, (g.T, 3, S, S)).astype(np.float32)
        want = tiling.tile_blend_host(tiles_h, H, W, O)
        tiles = torch.from_numpy(tiles_h).to(DEV)
        got = ops.tile_blend(tiles, H, W, O)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, H, W)
        got_h = got.cpu().numpy()
        err = float(np.abs(got_h.astype(np.float64) - want).max())
        bound = 1e-6 * max(1.0, float(np.abs(tiles_h).max()))
        print(f"blend S={S} O={O} {H}x{W}: max err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (H, W)
        ny = np.array([len(tiling.covering(y, g.ny, g.stride, O)) for y in range(H)])
        nx = np.array([len(tiling.covering(x, g.nx, g.stride, O)) for x in range(W)])
        single = np.outer(ny, nx) == 1
        assert single.any()
        assert np.array_equal(got_h[:, single].astype(np.float64), want[:, single]), (H, W)  # the tile's own bits
        u8 = ops.tile_blend(tiles, H, W, O, out="u8")
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (H, W, 3)
        assert torch.equal(u8, got.clamp(0, 1).mul(255).round().byte().permute(1, 2, 0)), (H, W)
        fbuf, fview = guarded((3, H, W), torch.float32)
        ubuf, uview = guarded((H, W, 3), torch.uint8)
        both = ops.tile_blend(tiles, H, W, O, out="both", out_f32=fview, out_u8=uview)
        assert torch.equal(both[0], got) and torch.equal(both[1], u8), (H, W)
        assert intact(fbuf) and intact(ubuf), (H, W)


def test_argument_errors(tmae):
    """each raises on the host, before anything is launched"""
    from textmae_amd import ops

    src = torch.zeros((20, 30, 3), dtype=torch.uint8, device=DEV)
    tiles = torch.zeros((6, 3, 16, 16), dtype=torch.float32, device=DEV)  # 20 x 30 at S 16, O 4: 2 x 3 tiles
    with pytest.raises(ValueError, match="overlap 9 outside"):
        ops.tile_cut_u8(src, 16, 9)
    with pytest.raises(ValueError, match="overlap 9 outside"):
        ops.tile_blend(tiles, 20, 30, 9)
    with pytest.raises(ValueError, match=r"tiles 1\.\.7 outside the image's 6"):
        ops.tile_cut_u8(src, 16, 4, t0=1, nt=6)
    with pytest.raises(ValueError, match=r"tiles 6\.\.6 outside"):
        ops.tile_cut_u8(src, 16, 4, t0=6)
    with pytest.raises(ValueError, match="contiguous"):
        ops.tile_cut_u8(src[:, ::2], 16, 4)
    with pytest.raises(ValueError, match="must be torch.uint8"):
        ops.tile_cut_u8(src.int(), 16, 4)
    with pytest.raises(ValueError, match=r"uint8 \[H, W, 3\]"):
        ops.tile_cut_u8(src.permute(2, 0, 1).contiguous(), 16, 4)
    with pytest.raises(ValueError, match="5 tiles, but 20x30"):
        ops.tile_blend(tiles[:5], 20, 30, 4)
    with pytest.raises(ValueError, match="out must be"):
        ops.tile_blend(tiles, 20, 30, 4, out="bf16")
    assert ops.tile_cut_u8(src, 16, 4)[0].shape[0] == 6  # and the valid call goes through


# ------------------------------------------------------------------------------------------------ model
H0, W0, O0 = 200, 300, 32  # 2 x 3 tiles of 128 at overlap 32


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
def image():
    return np.random.default_rng(41).integers(0, 256, (H0, W0, 3), dtype=np.uint8)


@pytest.mark.parametrize("lanes", [1, 4])
def test_file_is_encode_bytes_of_the_tiles(tmae, small, image, lanes):
    from textmae_amd import bitstream as bs
    from textmae_amd import ops
    from textmae_amd.scores import image_scores

    blob = small.encode_image(image, overlap=O0, lanes=lanes, tile_batch=6)
    assert isinstance(blob, bytes)
    p = bs.parse_image(blob)
    assert (p.img_size, p.num_keep_patches, p.patch_size, p.lanes, p.z_lanes) == (128, 16, 16, lanes, 1)
    assert (p.overlap, p.width, p.height, p.chunk, p.num_tiles) == (O0, W0, H0, 6, 6)
    tiles, gray = ops.tile_cut_u8(torch.from_numpy(image).to(DEV), 128, O0)
    blobs = small.encode_bytes(tiles, image_scores(gray, 128, 16), lanes=lanes)
    for t in range(6):
        assert bs.tile_blob(p, t) == blobs[t], t
    want = ops.tile_blend(small.decode_bytes(blobs)["x_hat"], H0, W0, O0)
    got = small.decode_image(blob)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, H0, W0)
    assert torch.equal(got, want)
    u8 = small.decode_image(blob, out="u8")
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (H0, W0, 3)
    assert torch.equal(u8, got.clamp(0, 1).mul(255).round().byte().permute(1, 2, 0))
    # a device tensor is the same image
    assert small.encode_image(torch.from_numpy(image).to(DEV), overlap=O0, lanes=lanes, tile_batch=6) == blob


def test_chunked_file(tmae, small, image):
    """tile_batch 4: chunks of 4 + 2, recorded, and repeated by the decoder by default"""
    from textmae_amd import bitstream as bs

    blob = small.encode_image(image, overlap=O0, tile_batch=4)
    assert bs.parse_image(blob).chunk == 4
    got = small.decode_image(blob)
    assert tuple(got.shape) == (3, H0, W0) and bool(torch.isfinite(got).all())
    assert torch.equal(small.decode_image(blob, tile_batch=4), got)


def test_decode_does_not_depend_on_the_batch(tmae, small, image):
    """the file coded in chunks of 4 + 2 decoded in one batch of 6: per-image results that do not depend on the
    batch size, which the command lines assume of decode_bytes already"""
    blob = small.encode_image(image, overlap=O0, tile_batch=4)
    a = small.decode_image(blob, tile_batch=4).clone()
    b = small.decode_image(blob, tile_batch=6)
    print(f"batch 4+2 against 6: max abs difference {float((a - b).abs().max()):.3e}")
    assert torch.equal(a, b)


def test_corrupt_tiles_are_named(tmae, small, image):
    from textmae_amd import bitstream as bs

    blob = small.encode_image(image, overlap=O0, tile_batch=6)
    good = small.decode_image(blob).clone()
    p = bs.parse_image(blob)

    def rebuilt(ids=None, y=None):
        return bs.assemble_image(p.img_size, p.num_keep_patches, p.patch_size, p.lanes, p.z_lanes, p.overlap, p.width,
                                 p.height, p.chunk, np.stack(p.ids if ids is None else ids), p.z,
                                 p.y if y is None else y)

    assert rebuilt() == blob
    keep = bs.unpack_ids_host(p.ids[1], 64, 16)[0][:16].copy()
    keep[3] = keep[12]
    ids = list(p.ids)
    ids[1] = bs.pack_ids_host(keep, 64)
    dup = rebuilt(ids=ids)
    assert len(dup) == len(blob)
    with pytest.raises(ValueError, match=r"side information of tile 1: duplicate"):
        small.decode_image(dup)
    assert torch.equal(small.decode_image(blob), good)
    with pytest.raises(ValueError, match=r"side information of tile 1: duplicate"):
        small.decode_image(dup, tile_batch=1)  # tile 1 is image 0 of its call
    y = list(p.y)
    y[2] = bytes(y[2])[:-4]
    short = rebuilt(y=y)
    assert len(short) == len(blob) - 4
    with pytest.raises(ValueError, match=r"y stream of tile 2\b"):
        small.decode_image(short)
    assert torch.equal(small.decode_image(blob), good)
    with pytest.raises(ValueError, match=r"y stream of tile 2\b"):
        small.decode_image(short, tile_batch=2)  # tile 2 is image 0 of the second call
    assert torch.equal(small.decode_image(blob), good)


def test_other_geometry_and_bad_arguments(tmae, small, image):
    from textmae_amd import bitstream as bs
    from textmae_amd import tiling

    g = tiling.grid(H0, W0, 160, O0)
    rec = [b"\0" * 8] * g.T
    other = bs.assemble_image(160, 16, 16, 1, 1, O0, W0, H0, 6, np.zeros((g.T, bs.id_words(100, 16)), np.uint32), rec,
                              rec)
    with pytest.raises(ValueError, match=r"coded for img_size 160, patch_size 16, num_keep_patches 16; this model "
                                         r"has 128, 16, 16"):
        small.decode_image(other)
    with pytest.raises(ValueError, match="not a TMT bitstream"):
        small.decode_image(b"TMC\x01" + b"\0" * 28)
    with pytest.raises(ValueError, match="overlap 65 outside"):
        small.encode_image(image, overlap=65)
    with pytest.raises(ValueError, match=r"uint8 \[H, W, 3\]"):
        small.encode_image(image.astype(np.float32))
    with pytest.raises(ValueError, match=r"uint8 \[H, W, 3\]"):
        small.encode_image(image[:, :, 0])
    with pytest.raises(ValueError, match="power of two"):
        small.encode_image(image, lanes=3)
    with pytest.raises(ValueError, match="tile_batch 0"):
        small.encode_image(image, tile_batch=0)


def test_image_smaller_than_a_tile(tmae, small):
    from textmae_amd import bitstream as bs

    img = np.random.default_rng(43).integers(0, 256, (40, 50, 3), dtype=np.uint8)
    blob = small.encode_image(img)
    p = bs.parse_image(blob)
    assert (p.width, p.height, p.num_tiles, p.overlap, p.chunk) == (50, 40, 1, 32, 16)
    got = small.decode_image(blob)
    assert tuple(got.shape) == (3, 40, 50) and bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------ command lines
SIZES = [(300, 200), (224, 224), (190, 257)]  # PIL (W, H) of the synthetic images


@pytest.fixture(scope="module")
def synth(tmae, tmp_path_factory):
    """the three synthetic PNGs and the seeded checkpoint (224^2, K = 144) of test_gpu_bitstream.py"""
    from PIL import Image

    root = tmp_path_factory.mktemp("tiled_cli")
    rng = np.random.default_rng(31)
    ds = root / "synth3"
    ds.mkdir()
    for i, (w, h) in enumerate(SIZES):
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([127 + 120 * np.sin(xx / (7.0 + 3 * c) + i) * np.cos(yy / (5.0 + 2 * i) + c) for c in range(3)],
                     -1)
        a = np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(ds / f"img{i}.png")
    cfg = MCMConfig(img_size=224, num_keep_patches=144)
    sd = tmae.MCM(**cfg.kwargs()).state_dict()
    sd.update(make_state_dict(cfg, 17))
    ck = root / "best_model.pth"
    torch.save({"model": sd}, ck)
    return ds, ck


def test_codec_cli_tiled(tmae, synth, tmp_path):
    from PIL import Image

    from textmae_amd import bitstream as bs
    from textmae_amd import codec

    ds, ck = synth
    tmt, out = tmp_path / "tmt", tmp_path / "png"
    assert codec.main(["encode", "-c", str(ck), "-d", str(ds), "-o", str(tmt), "--tiled", "--overlap", "32",
                       "--lanes", "2"]) == 3
    files = sorted(tmt.glob("*.tmt"))
    assert [f.name for f in files] == ["img0.tmt", "img1.tmt", "img2.tmt"]
    for f, (w, h), T in zip(files, SIZES, (2, 1, 2)):
        p = bs.parse_image(f.read_bytes())
        assert (p.width, p.height, p.num_tiles) == (w, h, T)
        assert (p.img_size, p.num_keep_patches, p.lanes, p.z_lanes, p.overlap, p.chunk) == (224, 144, 2, 1, 32, 16)
    assert codec.main(["decode", "-c", str(ck), "-d", str(tmt), "-o", str(out)]) == 3
    for f, size in zip(files, SIZES):
        assert Image.open(out / (f.stem + ".png")).size == size


def test_testing_main_tiled(tmae, synth, tmp_path):
    from textmae_amd import testing

    ds, ck = synth
    common = ["-d", str(ds), "--cuda", "-c", str(ck), "--num_keep_patches", "144", "--input_size", "224",
              "--lanes", "1"]
    tmt = tmp_path / "tmt"
    rep = testing.main(common + ["-o", str(tmp_path / "rec"), "--tiled", "--overlap", "32", "--bitstream", str(tmt)])
    files = sorted(tmt.glob("*.tmt"))
    assert [f.name for f in files] == ["img0.tmt", "img1.tmt", "img2.tmt"]
    bpp = 0.0
    for f, (w, h) in zip(files, SIZES):  # averaged as the report averages: sum of the images' values / count
        bpp += 8.0 * f.stat().st_size / (w * h)
    assert rep["results"]["bpp"][0] == pytest.approx(bpp / 3, rel=1e-12, abs=0)
    assert np.isfinite(rep["results"]["psnr"][0]) and rep["results"]["psnr"][0] > 0
    assert 0 < rep["results"]["ms-ssim"][0] <= 1  # every image's smaller side exceeds 160
    assert "MS-SSIM over the 3 of 3 images" in rep["description"] and "tiled" in rep["description"]
    saved = json.load(open(tmp_path / "rec" / "report.txt"))
    assert saved["results"]["bpp"] == rep["results"]["bpp"]
    # without --tiled nothing of this shows
    plain = testing.main(common + ["-o", str(tmp_path / "rec_plain")])
    assert plain["description"] == "Inference (ans)"
    assert sorted(plain["results"]) == ["bpp", "decoding_time", "encoding_time", "ms-ssim", "psnr"]


def test_small_images_report_psnr_only(tmae, synth, tmp_path):
    """an image whose smaller side is at most 160 is too small for MS-SSIM's five scales"""
    from PIL import Image

    from textmae_amd import testing

    ds, ck = synth
    small_ds = tmp_path / "small"
    small_ds.mkdir()
    Image.open(ds / "img0.png").crop((0, 0, 240, 160)).save(small_ds / "a.png")
    rep = testing.main(["-d", str(small_ds), "--cuda", "-c", str(ck), "--num_keep_patches", "144", "--input_size",
                        "224", "-o", str(tmp_path / "rec"), "--tiled"])
    assert "ms-ssim" not in rep["results"] and np.isfinite(rep["results"]["psnr"][0])
    assert "MS-SSIM over the 0 of 1 images" in rep["description"] and "PSNR only" in rep["description"]
    assert Image.open(tmp_path / "rec" / "a.png").size == (240, 160)
