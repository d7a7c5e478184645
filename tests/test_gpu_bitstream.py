"""Self-contained per-image bitstreams on the GPU: the id pack / unpack kernels (csrc/ids_pack.hip) against the numpy
oracle of textmae_amd.bitstream, MCM.encode_bytes / decode_bytes against compress_batch / decompress_batch (every
comparison an equality: the blobs carry the same records and the decoder runs the same path), and testing.main's
--bitstream mode."""
import json

import numpy as np
import pytest
import torch

from oracle.mcm_oracle import MCMConfig, make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"

LK = [(64, 16), (196, 144), (100, 64), (1024, 400), (576, 16), (65, 16), (16, 16), (1, 1)]
# SMALL12 of test_gpu_device_coder.py, and the same model at 160 px: L = 100 ids of 7 bits, K = 16 -> 112 bits
SMALL12 = dict(img_size=128, patch_size=16, encoder_embed_dim=128, encoder_depth=1, encoder_num_heads=2,
               decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2, latent_depth=192, hyperprior_depth=96,
               num_slices=12, num_keep_patches=16)
RAGGED = dict(SMALL12, img_size=160)


def state_dict(tmae, cfgd, seed):
    cfg = MCMConfig(**cfgd)
    full = tmae.MCM(**cfg.kwargs()).state_dict()
    full.update(make_state_dict(cfg, seed))
    return full


def build(tmae, cfgd, sd):
    m = tmae.MCM(**MCMConfig(**cfgd).kwargs())
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.update(force=True)
    return m


def inputs(n, img, L, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = (torch.rand(n, 3, img, img, generator=g) - 0.45) / 0.225
    return imgs.to(DEV), torch.rand(n, L, generator=g).to(DEV)


def random_shuffles(rng, n, L):
    return np.stack([rng.permutation(L) for _ in range(n)]).astype(np.int64)


@pytest.fixture(scope="module")
def small_sd(tmae):
    return state_dict(tmae, SMALL12, 11)


@pytest.fixture(scope="module")
def small(tmae, small_sd):
    return build(tmae, SMALL12, small_sd)


@pytest.fixture(scope="module")
def ragged(tmae):
    return build(tmae, RAGGED, state_dict(tmae, RAGGED, 12))


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n,L,K", [(3, L, K) for L, K in LK] + [(1, 196, 144), (70, 196, 144)])
def test_kernels_against_host_oracle(tmae, n, L, K):
    from textmae_amd import bitstream as bs
    from textmae_amd import ops

    rng = np.random.default_rng(7 * L + K + n)
    shuf_h = random_shuffles(rng, n, L)
    want = bs.pack_ids_host(shuf_h[:, :K], L)
    words = ops.ids_pack(torch.from_numpy(shuf_h).to(DEV), K)
    assert words.dtype == torch.int32 and tuple(words.shape) == (n, bs.id_words(L, K))
    np.testing.assert_array_equal(words.cpu().numpy().view(np.uint32), want)
    shuf, rest, status = ops.ids_unpack(words, L, K)
    ws, wr, wst = bs.unpack_ids_host(want, L, K)
    assert not wst.any()
    assert status.cpu().tolist() == [0] * n
    np.testing.assert_array_equal(shuf.cpu().numpy(), ws)
    np.testing.assert_array_equal(rest.cpu().numpy(), wr)
    # what the oracle gives is the kept ids, then the others ascending (tests/test_bitstream_host.py): spot-check
    np.testing.assert_array_equal(ws[:, :K], shuf_h[:, :K])
    assert (np.diff(ws[:, K:], axis=1) > 0).all()


def test_pack_of_ids_shuffle_kernel(tmae):
    """tmae_ids_shuffle's own output on random scores, L = 256 (8 bits exactly filled), K = 144"""
    from textmae_amd import bitstream as bs
    from textmae_amd import ops

    g = torch.Generator().manual_seed(4)
    shuf, rest = ops.ids_shuffle(torch.rand(5, 256, generator=g).to(DEV), 144)
    words = ops.ids_pack(shuf, 144)
    np.testing.assert_array_equal(words.cpu().numpy().view(np.uint32),
                                  bs.pack_ids_host(shuf[:, :144].cpu().numpy(), 256))
    s2, r2, status = ops.ids_unpack(words, 256, 144)
    assert not status.cpu().any()
    assert torch.equal(s2[:, :144], shuf[:, :144])
    assert torch.equal(torch.gather(s2, 1, r2), torch.arange(256, device=DEV).expand(5, 256))


def test_unpack_rejects_without_harm(tmae):
    """only ops.ids_unpack: a duplicate, an id >= L and a set tail bit are reported, their images get the identity
    in both outputs, and the valid image beside them is untouched"""
    from textmae_amd import bitstream as bs
    from textmae_amd import ops

    rng = np.random.default_rng(21)
    L, K = 100, 64
    keep = random_shuffles(rng, 3, L)[:, :K]
    bits = bs.id_bits(L)
    assert bits == 7
    bad = keep.copy()
    bad[1, 10] = bad[1, 40]                       # image 1: a duplicate
    words = bs.pack_ids_host(bad, L)
    k = 9                                         # image 2: id 9 becomes 127 (all 7 bits set) >= L
    for i in range(k * bits, (k + 1) * bits):
        words[2, i // 32] |= np.uint32(1 << (i % 32))
    shuf, rest, status = ops.ids_unpack(torch.from_numpy(words.view(np.int32)).to(DEV), L, K)
    ws, wr, wst = bs.unpack_ids_host(words, L, K)
    assert wst.tolist() == [0, 2, 1]
    assert status.cpu().tolist() == [0, 2, 1]
    np.testing.assert_array_equal(shuf.cpu().numpy(), ws)
    np.testing.assert_array_equal(rest.cpu().numpy(), wr)
    np.testing.assert_array_equal(shuf[0, :K].cpu().numpy(), keep[0])
    for b in (1, 2):
        np.testing.assert_array_equal(shuf[b].cpu().numpy(), np.arange(L))
        np.testing.assert_array_equal(rest[b].cpu().numpy(), np.arange(L))

    L, K = 65, 16                                 # 112 bits: one tail bit of the half-used last word set
    w = bs.pack_ids_host(random_shuffles(rng, 1, L)[:, :K], L)
    w[0, -1] |= np.uint32(1 << 16)
    shuf, rest, status = ops.ids_unpack(torch.from_numpy(w.view(np.int32)).to(DEV), L, K)
    assert status.cpu().tolist() == [3]
    np.testing.assert_array_equal(shuf[0].cpu().numpy(), np.arange(L))
    np.testing.assert_array_equal(rest[0].cpu().numpy(), np.arange(L))


# ------------------------------------------------------------------------------------------------ model
def check_blobs(m, cfgd, lanes, z_lanes, seed):
    """encode_bytes against compress_batch on the same inputs, decode_bytes against decompress_batch"""
    from textmae_amd import bitstream as bs

    img, K = cfgd["img_size"], cfgd["num_keep_patches"]
    L = (img // 16) ** 2
    imgs, scores = inputs(3, img, L, seed)
    sizes = [(300, 200), (img, img), (65535, 1)]
    out = m.compress_batch(imgs, scores, lanes=lanes, z_lanes=z_lanes)
    blobs = m.encode_bytes(imgs, scores, lanes=lanes, z_lanes=z_lanes, orig_sizes=sizes)
    assert len(blobs) == 3 and all(isinstance(b, bytes) for b in blobs)
    keep = np.argsort(out["ids_restore"].cpu().numpy(), axis=1)[:, :K]
    for b, blob in enumerate(blobs):
        p = bs.parse(blob)
        assert (p.img_size, p.patch_size, p.num_keep_patches, p.num_patches) == (img, 16, K, L)
        assert (p.lanes, p.z_lanes) == (lanes, z_lanes) and p.orig_size == sizes[b]
        assert bytes(p.y) == out["string"][0][b] and bytes(p.z) == out["string"][1][b]
        np.testing.assert_array_equal(p.ids, bs.pack_ids_host(keep[b], L))
        assert len(blob) == 16 + 4 * bs.id_words(L, K) + len(out["string"][0][b]) + len(out["string"][1][b])
    want = m.decompress_batch(out["string"], out["shape"], out["ids_restore"], lanes=lanes, z_lanes=z_lanes)["x_hat"]
    got = m.decode_bytes(blobs)
    assert got["orig_sizes"] == sizes
    assert got["x_hat"].shape == (3, 3, img, img) and torch.equal(got["x_hat"], want)
    return blobs, want


@pytest.mark.parametrize("lanes,z_lanes", [(1, 1), (4, 2)])
def test_blobs_are_compress_batch_records(tmae, small, lanes, z_lanes):
    check_blobs(small, SMALL12, lanes, z_lanes, 5)


def test_ragged_id_section(tmae, ragged):
    """160 px: 100 patches at 7 bits, 16 kept -> 112 bits, the fourth word half used"""
    from textmae_amd import bitstream as bs

    assert bs.id_bits(100) == 7 and bs.id_words(100, 16) == 4
    blobs, _ = check_blobs(ragged, RAGGED, 1, 1, 6)
    assert all(bs.parse(b).ids[-1] >> 16 == 0 for b in blobs)


def test_decode_in_another_model_object(tmae, small, small_sd, tmp_path):
    """the files alone: written here, read back and decoded by a second model built from the same state dict"""
    imgs, scores = inputs(3, 128, 64, 8)
    sizes = [(640, 480), (1, 2), (500, 333)]
    blobs = small.encode_bytes(imgs, scores, lanes=2, orig_sizes=sizes)
    want = small.decode_bytes(blobs)["x_hat"].clone()
    for b, blob in enumerate(blobs):
        (tmp_path / f"{b}.tmc").write_bytes(blob)
    other = build(tmae, SMALL12, small_sd)
    got = other.decode_bytes([(tmp_path / f"{b}.tmc").read_bytes() for b in range(3)])
    assert got["orig_sizes"] == sizes
    assert torch.equal(got["x_hat"], want)
    # no sizes given: none recorded
    assert other.decode_bytes(small.encode_bytes(imgs, scores))["orig_sizes"] == [None] * 3


def test_errors_name_the_blob(tmae, small, ragged):
    from textmae_amd import bitstream as bs

    imgs, scores = inputs(3, 128, 64, 9)
    blobs = small.encode_bytes(imgs, scores)
    want = small.decode_bytes(blobs)["x_hat"].clone()
    other = ragged.encode_bytes(*inputs(1, 160, 100, 9))
    with pytest.raises(ValueError, match=r"blob 2: coded for img_size 160"):
        small.decode_bytes([blobs[0], blobs[1], other[0]])
    with pytest.raises(ValueError, match=r"blob 0: coded for img_size 128"):
        ragged.decode_bytes(blobs[:1])
    lanes4 = small.encode_bytes(imgs, scores, lanes=4)
    with pytest.raises(ValueError, match=r"blob 1: lanes \(4, 1\) differ from blob 0's \(1, 1\)"):
        small.decode_bytes([blobs[0], lanes4[1], blobs[2]])
    with pytest.raises(ValueError, match=r"blob 1: .*whole number of 32-bit words"):
        small.decode_bytes([blobs[0], blobs[1][:-3], blobs[2]])
    p = bs.parse(blobs[2])
    with pytest.raises(ValueError, match=r"blob 2: "):
        small.decode_bytes([blobs[0], blobs[1], blobs[2][:16 + 4 * p.ids.size + len(p.z) + 4]])
    with pytest.raises(ValueError, match=r"no blobs"):
        small.decode_bytes([])
    # a duplicate id in blob 1's id section: found on the device, raised after the call
    p = bs.parse(blobs[1])
    keep = bs.unpack_ids_host(p.ids, 64, 16)[0][:16].copy()
    keep[3] = keep[12]
    dup = bs.assemble(128, 16, 16, 1, 1, None, bs.pack_ids_host(keep, 64), p.z, p.y)
    assert len(dup) == len(blobs[1])
    with pytest.raises(ValueError, match=r"side information of image 1: duplicate"):
        small.decode_bytes([blobs[0], dup, blobs[2]])
    # and the model decodes the good blobs as before afterwards
    assert torch.equal(small.decode_bytes(blobs)["x_hat"], want)


# ------------------------------------------------------------------------------------------------ command lines
SIZES = [(300, 200), (224, 224), (190, 257)]  # PIL (W, H) of the synthetic images


@pytest.fixture(scope="module")
def synth(tmae, tmp_path_factory):
    """three synthetic PNGs of different sizes and a seeded checkpoint (224^2, K = 144) -> (folder, checkpoint)"""
    from PIL import Image

    root = tmp_path_factory.mktemp("bitstream_cli")
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


def test_testing_main_bitstream(tmae, synth, tmp_path):
    """testing.main --bitstream: one .tmc per image, bpp = 8 * mean file size / pixels, PSNR / MS-SSIM those of the
    --lanes 1 run without --bitstream"""
    from PIL import Image

    from textmae_amd import bitstream as bs
    from textmae_amd import testing

    ds, ck = synth
    common = ["-d", str(ds), "--cuda", "-c", str(ck), "--num_keep_patches", "144", "--input_size", "224",
              "--lanes", "1"]
    plain = testing.main(common + ["-o", str(tmp_path / "rec_plain")])
    tmc = tmp_path / "tmc"
    rep = testing.main(common + ["-o", str(tmp_path / "rec"), "--bitstream", str(tmc), "--original_size"])
    files = sorted(tmc.glob("*.tmc"))
    assert [f.name for f in files] == ["img0.tmc", "img1.tmc", "img2.tmc"]
    mean_size = sum(f.stat().st_size for f in files) / 3
    assert rep["results"]["bpp"][0] == pytest.approx(8.0 * mean_size / (224 * 224), rel=1e-12, abs=0)
    assert rep["results"]["psnr"] == plain["results"]["psnr"]
    assert rep["results"]["ms-ssim"] == plain["results"]["ms-ssim"]
    assert "side information" in rep["description"] and "side information" not in plain["description"]
    saved = json.load(open(tmp_path / "rec" / "report.txt"))
    assert saved["results"]["bpp"] == rep["results"]["bpp"]
    for f, size in zip(files, SIZES):  # each file records its image's size; --original_size saved at that size
        p = bs.parse(f.read_bytes())
        assert p.orig_size == size and (p.img_size, p.num_keep_patches, p.lanes) == (224, 144, 1)
        assert p.ids.size * 4 == 144
        assert Image.open(tmp_path / "rec" / (f.stem + ".png")).size == size


def test_codec_cli(tmae, synth, tmp_path):
    """codec encode (batches of 2, so a last batch of 1) then codec decode, which takes the geometry from the files"""
    from PIL import Image

    from textmae_amd import bitstream as bs
    from textmae_amd import codec

    ds, ck = synth
    tmc, out = tmp_path / "tmc", tmp_path / "png"
    assert codec.main(["encode", "-c", str(ck), "-d", str(ds), "-o", str(tmc), "--lanes", "2", "--batch", "2"]) == 3
    files = sorted(tmc.glob("*.tmc"))
    assert [f.name for f in files] == ["img0.tmc", "img1.tmc", "img2.tmc"]
    for f, size in zip(files, SIZES):
        p = bs.parse(f.read_bytes())
        assert p.orig_size == size and (p.img_size, p.num_keep_patches, p.lanes, p.z_lanes) == (224, 144, 2, 1)
    assert codec.main(["decode", "-c", str(ck), "-d", str(tmc), "-o", str(out), "--original_size"]) == 3
    for f, size in zip(files, SIZES):
        assert Image.open(out / (f.stem + ".png")).size == size
