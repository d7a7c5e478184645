"""Variable rate from one checkpoint through the model: MCM.encode_bytes / decode_bytes with q= and
target_bytes=, the tiled files (encode_image / decode_image / decode_region / decode_crops) and the command lines.

SMALL12 of test_gpu_bitstream.py (128 px, K = 16, weights make_state_dict(cfg, 11)), batch 3, input seed 47: chosen on
the CPU so that the oracle restatement of the coded path (qstep_check.oracle_coded) rounds no (y - mu) / delta within
1e-4 of a half-integer at q = (-16, 0, 5), nor at q = -16, 0, 16 for all images, nor any z - median; the tests assert
that on the reference alone.  There the images hold 1713 / 1649 / 1781 non-zero y symbols at q = -16, 88 / 84 / 126 at
q = 0 and none at q = 16."""
import numpy as np
import pytest
import torch

import qstep_check as qk
from oracle.mcm_oracle import MCMConfig, make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"

SMALL12 = dict(img_size=128, patch_size=16, encoder_embed_dim=128, encoder_depth=1, encoder_num_heads=2,
               decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2, latent_depth=192, hyperprior_depth=96,
               num_slices=12, num_keep_patches=16)
SEED_W, SEED_X = 11, 47
QMIX = (-16, 0, 5)


def maxrel(a, b):
    """tests/test_gpu_mcm.py's metric for x_hat against the oracle at f32, bound 1e-3"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def inputs(n, img, L, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = (torch.rand(n, 3, img, img, generator=g) - 0.45) / 0.225
    return imgs, torch.rand(n, L, generator=g)


@pytest.fixture(scope="module")
def small(tmae):
    cfg = MCMConfig(**SMALL12)
    m = tmae.MCM(**cfg.kwargs())
    sd = m.state_dict()
    sd.update(make_state_dict(cfg, SEED_W))
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.update(force=True)
    return m


@pytest.fixture(scope="module")
def xs():
    imgs, scores = inputs(3, 128, 64, SEED_X)
    return imgs.to(DEV), scores.to(DEV)


@pytest.fixture(scope="module")
def plain(small, xs):
    return small.encode_bytes(*xs)


@pytest.fixture(scope="module")
def oracle():
    """the CPU reference, computed once: the coded path at QMIX and at -16 / 0 / 16 for all images"""
    cfg = MCMConfig(**SMALL12)
    sd = make_state_dict(cfg, SEED_W)
    imgs, scores = inputs(3, 128, 64, SEED_X)
    return {q: qk.oracle_coded(sd, cfg, imgs, scores, q) for q in (QMIX, (-16,) * 3, (0,) * 3, (16,) * 3)}


# ------------------------------------------------------------------------------------------------ encode_bytes(q=)
@pytest.mark.parametrize("lanes", [1, 8])
def test_q_zero_is_todays_bytes(tmae, small, xs, lanes):
    from textmae_amd import bitstream as bs

    want = small.encode_bytes(*xs, lanes=lanes)
    assert all(b[:4] == b"TMC\x01" for b in want)
    for q in (None, 0, [0, 0, 0], np.zeros(3, dtype=np.int64)):
        assert small.encode_bytes(*xs, lanes=lanes, q=q) == want
    out = small.compress_batch(*xs, lanes=lanes)
    for q in (0, (0, 0, 0)):
        assert small.compress_batch(*xs, lanes=lanes, q=q)["string"] == out["string"]
    assert [bs.parse(b).q for b in want] == [0, 0, 0]


@pytest.mark.parametrize("lanes", [1, 8])
def test_mixed_batch_round_trip(tmae, small, xs, lanes):
    from textmae_amd import bitstream as bs

    want = small.encode_bytes(*xs, lanes=lanes)
    blobs = small.encode_bytes(*xs, lanes=lanes, q=QMIX, orig_sizes=None)
    ex = small._exec
    enc = {k: getattr(ex, k).clone() for k in ("YH", "SUPY", "YPRE")}
    sym = torch.from_numpy(np.array(ex.last_streams["y_symbols"])).clone()
    idx = torch.from_numpy(np.array(ex.last_streams["y_indexes"])).clone()
    assert [b[:3] for b in blobs] == [b"TQC", b"TMC", b"TQC"]
    assert [bs.parse(b).q for b in blobs] == list(QMIX)
    assert blobs[1] == want[1]  # the q = 0 image of a mixed batch: the plain call's blob, byte for byte
    for b in (0, 2):  # the other images' side information and z records are the plain ones
        p, w = bs.parse(blobs[b]), bs.parse(want[b])
        assert bytes(p.z) == bytes(w.z) and np.array_equal(p.ids, w.ids)
    assert len(bs.parse(blobs[0]).y) > len(bs.parse(want[0]).y)
    got = small.decode_bytes(blobs)
    x_all = got["x_hat"].clone()
    assert small._exec is ex
    for k, v in enc.items():  # the decoder's slice loop left what the encoder's left, bit for bit
        assert torch.equal(getattr(ex, k), v), k
    assert np.array_equal(np.array(ex.last_decoded["y_symbols"]), sym.numpy())
    assert np.array_equal(np.array(ex.last_decoded["y_indexes"]), idx.numpy())
    for b in range(3):  # one blob per call: the same rows
        assert torch.equal(small.decode_bytes([blobs[b]])["x_hat"][0], x_all[b]), b
    # and through compress_batch / decompress_batch with the same q
    out = small.compress_batch(*xs, lanes=lanes, q=QMIX)
    assert [bytes(bs.parse(b).y) for b in blobs] == list(out["string"][0])
    rec = small.decompress_batch(out["string"], out["shape"], out["ids_restore"], lanes=lanes, q=QMIX)["x_hat"]
    assert torch.equal(rec, x_all)
    # the plain path is untouched afterwards
    assert small.encode_bytes(*xs, lanes=lanes) == want


def test_against_the_oracle(tmae, small, xs, oracle):
    """f32 against the CPU restatement of the coded path: symbols equal, x_hat within test_gpu_mcm.py's 1e-3"""
    ref = oracle[QMIX]
    assert qk.near_ties(ref.t) == 0 and qk.near_ties(ref.z_t) == 0  # on the reference alone
    assert small.compute_dtype == torch.float32
    blobs = small.encode_bytes(*xs, q=QMIX)
    sym = np.array(small._exec.last_streams["y_symbols"]).reshape(-1)
    bad = int((torch.from_numpy(sym).long() != ref.sym).sum())
    x_hat = small.decode_bytes(blobs)["x_hat"]
    err = maxrel(x_hat, ref.x_hat)
    print(f"q = {QMIX}: {bad} of {sym.size} symbols differ from the oracle's, x_hat maxrel {err:.3e}")
    assert bad == 0
    assert err <= 1e-3


def test_rate_falls_with_q(tmae, small, xs, oracle):
    from textmae_amd import bitstream as bs

    nz = {}
    for q in (-16, 0, 16):
        ref = oracle[(q,) * 3]
        assert qk.near_ties(ref.t) == 0
        nz[q] = [int((ref.sym.reshape(12, 3, -1)[:, b] != 0).sum()) for b in range(3)]
    ylen = {q: [len(bs.parse(b).y) for b in small.encode_bytes(*xs, q=q)] for q in (-16, 0, 16)}
    print("non-zero symbols on the reference", nz, "y record bytes", ylen)
    for b in range(3):
        assert nz[16][b] < nz[0][b] < nz[-16][b], b  # the reference already shows it
        assert ylen[16][b] < ylen[0][b] < ylen[-16][b], b


# ------------------------------------------------------------------------------------------------ target_bytes
@pytest.mark.parametrize("lanes", [1, 8])
def test_target_bytes(tmae, small, xs, lanes):
    from textmae_amd import bitstream as bs

    s0 = [len(b) for b in small.encode_bytes(*xs, lanes=lanes, q=0)]
    s8 = [len(b) for b in small.encode_bytes(*xs, lanes=lanes, q=8)]
    target = [(a + b) // 2 for a, b in zip(s0, s8)]
    blobs = small.encode_bytes(*xs, lanes=lanes, target_bytes=target)
    qs = [bs.parse(b).q for b in blobs]
    print(f"lanes {lanes}: sizes at q = 0 {s0}, at q = 8 {s8}, targets {target} -> q {qs}, "
          f"sizes {[len(b) for b in blobs]}")
    assert all(len(b) <= t for b, t in zip(blobs, target))
    assert all(0 < q <= 8 for q in qs)
    assert small.encode_bytes(*xs, lanes=lanes, q=qs) == blobs  # the q in the header is the q used
    below = small.encode_bytes(*xs, lanes=lanes, q=[q - 1 for q in qs])
    assert all(len(b) > t for b, t in zip(below, target))
    assert torch.equal(small.decode_bytes(blobs)["x_hat"], small.decode_bytes(small.encode_bytes(
        *xs, lanes=lanes, q=qs))["x_hat"])
    # one int for all images; an unreachable target gives the q = 32 blobs
    one = small.encode_bytes(*xs, lanes=lanes, target_bytes=max(target))
    assert all(len(b) <= max(target) for b in one)
    tiny = small.encode_bytes(*xs, lanes=lanes, target_bytes=1)
    assert [bs.parse(b).q for b in tiny] == [32, 32, 32]
    assert tiny == small.encode_bytes(*xs, lanes=lanes, q=32)
    # a target everything fits: the finest step
    huge = small.encode_bytes(*xs, lanes=lanes, target_bytes=1 << 20)
    assert [bs.parse(b).q for b in huge] == [-32, -32, -32]


def test_errors_before_any_launch(tmae, small, xs, plain, monkeypatch):
    """every one of these is raised on the host: the library is not called at all"""
    from textmae_amd import _lib

    out = small.compress_batch(*xs)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for bad in (33, -33, [0, 40, 0], 1.5):
        with pytest.raises(ValueError, match=r"outside -32\.\.32"):
            small.encode_bytes(*xs, q=bad)
    with pytest.raises(ValueError, match=r"2 entries of q for 3 images"):
        small.encode_bytes(*xs, q=[1, 2])
    with pytest.raises(ValueError, match=r"2 entries of q for 3 images"):
        small.compress_batch(*xs, q=[1, 2])
    with pytest.raises(ValueError, match=r"give q or target_bytes, not both"):
        small.encode_bytes(*xs, q=3, target_bytes=500)
    with pytest.raises(ValueError, match=r"2 entries of target_bytes for 3 images"):
        small.encode_bytes(*xs, target_bytes=[500, 500])
    with pytest.raises(ValueError, match=r"decompress_batch: 4 entries of q for 3 images"):
        small.decompress_batch(out["string"], out["shape"], out["ids_restore"], q=[1, 2, 3, 4])
    with pytest.raises(ValueError, match=r"outside -32\.\.32"):
        small.decompress_batch(out["string"], out["shape"], out["ids_restore"], q=-40)
    assert calls == []
    monkeypatch.undo()
    assert small.encode_bytes(*xs) == plain


def test_decode_bytes_reads_q_from_each_blob(tmae, small, xs, plain):
    """plain and quantised blobs of different steps in one call, in another order than they were coded in"""
    a = small.encode_bytes(*xs, q=7)
    xa = small.decode_bytes(a)["x_hat"].clone()
    xp = small.decode_bytes(plain)["x_hat"].clone()
    got = small.decode_bytes([a[2], plain[0], a[1]])["x_hat"]
    assert torch.equal(got[0], xa[2]) and torch.equal(got[1], xp[0]) and torch.equal(got[2], xa[1])
    assert not torch.equal(xa[0], xp[0])
    bad = bytearray(a[1])
    bad[16] = 0
    with pytest.raises(ValueError, match=r"blob 1: TQC stream with q = 0"):
        small.decode_bytes([a[0], bytes(bad), a[2]])


# ------------------------------------------------------------------------------------------------ tiled files
H0, W0, O0 = 150, 200, 16  # 200 x 150: 2 x 2 tiles of 128 at overlap 16


@pytest.fixture(scope="module")
def image():
    yy, xx = np.mgrid[0:H0, 0:W0]
    a = np.stack([127 + 120 * np.sin(xx / (7.0 + 3 * c)) * np.cos(yy / 5.0 + c) for c in range(3)], -1)
    return np.clip(a + np.random.default_rng(43).normal(0, 6, a.shape), 0, 255).astype(np.uint8)


def test_tiled_files(tmae, small, image):
    from textmae_amd import bitstream as bs
    from textmae_amd import ops

    plain = small.encode_image(image, overlap=O0)
    assert plain[:4] == b"TMT\x01"
    assert small.encode_image(image, overlap=O0, q=0) == plain
    blob = small.encode_image(image, overlap=O0, q=5)
    assert blob[:4] == b"TQT\x01" and len(blob) < len(plain)
    p = bs.parse_image(blob)
    assert p.q == 5 and p.num_tiles == 4 and (p.width, p.height, p.overlap) == (W0, H0, O0)
    tiles = [bs.tile_blob(p, t) for t in range(4)]
    assert all(t[:4] == b"TQC\x01" and bs.parse(t).q == 5 for t in tiles)
    want = ops.tile_blend(small.decode_bytes(tiles)["x_hat"], H0, W0, O0)
    full = small.decode_image(blob)
    assert torch.equal(full, want)
    assert not torch.equal(full, small.decode_image(plain))
    win = (100, 20, 40, 30)  # x0, y0, w, h: columns 100..139 lie in both tile columns (stride 112, overlap 16)
    assert torch.equal(small.decode_region(blob, *win), full[:, 20:50, 100:140])
    both = small.decode_crops([blob, plain, blob], [(100, 20), (5, 110), (0, 0)], (40, 30))
    assert torch.equal(both[0], small.decode_crops([blob], [(100, 20)], (40, 30))[0])
    assert torch.equal(both[1], small.decode_crops([plain], [(5, 110)], (40, 30))[0])
    assert torch.equal(both[2], full[:, 0:30, 0:40])
    with pytest.raises(ValueError, match=r"give q or target_bytes, not both"):
        small.encode_image(image, overlap=O0, q=1, target_bytes=4000)
    with pytest.raises(ValueError, match=r"outside -32\.\.32"):
        small.encode_image(image, overlap=O0, q=64)


def test_tiled_target_bytes(tmae, small, image):
    from textmae_amd import bitstream as bs

    s0 = len(small.encode_image(image, overlap=O0, q=0))
    s8 = len(small.encode_image(image, overlap=O0, q=8))
    target = (s0 + s8) // 2
    blob = small.encode_image(image, overlap=O0, target_bytes=target)
    q = bs.parse_image(blob).q
    print(f"file sizes at q = 0 {s0}, at q = 8 {s8}, target {target} -> q {q}, {len(blob)} bytes")
    assert len(blob) <= target and 0 < q <= 8
    assert blob == small.encode_image(image, overlap=O0, q=q)
    assert len(small.encode_image(image, overlap=O0, q=q - 1)) > target
    tiny = small.encode_image(image, overlap=O0, target_bytes=1)
    assert bs.parse_image(tiny).q == 32 and tiny == small.encode_image(image, overlap=O0, q=32)


# ------------------------------------------------------------------------------------------------ command lines
@pytest.fixture(scope="module")
def synth(tmae, tmp_path_factory, image):
    """two synthetic PNGs and a seeded checkpoint of the command lines' model (224^2, K = 144)"""
    from PIL import Image

    root = tmp_path_factory.mktemp("qstep_cli")
    ds = root / "synth2"
    ds.mkdir()
    Image.fromarray(image).save(ds / "img0.png")
    Image.fromarray(np.ascontiguousarray(image[::-1, ::-1])).save(ds / "img1.png")
    cfg = MCMConfig(img_size=224, num_keep_patches=144)
    sd = tmae.MCM(**cfg.kwargs()).state_dict()
    sd.update(make_state_dict(cfg, 17))
    ck = root / "best_model.pth"
    torch.save({"model": sd}, ck)
    return ds, ck


def test_codec_cli(tmae, synth, tmp_path, capsys):
    from PIL import Image

    from textmae_amd import bitstream as bs
    from textmae_amd import codec

    ds, ck = synth
    enc = ["encode", "-c", str(ck), "-d", str(ds)]
    a, out = tmp_path / "coded", tmp_path / "png"
    with pytest.raises(SystemExit):  # argparse: the two exclude each other
        codec.main(enc + ["-o", str(a), "--q", "1", "--target-bytes", "100"])
    capsys.readouterr()
    assert codec.main(enc + ["-o", str(a), "--q", "6"]) == 2
    assert [bs.parse(f.read_bytes()).q for f in sorted(a.glob("*.tmc"))] == [6, 6]
    assert "Warning" not in capsys.readouterr().err
    # a target nothing reaches: the coarsest step, and a warning per file
    assert codec.main(enc + ["-o", str(a), "--tiled", "--overlap", "16", "--target-bytes", "1"]) == 2
    assert capsys.readouterr().err.count("above --target-bytes 1") == 2
    assert [bs.parse_image(f.read_bytes()).q for f in sorted(a.glob("*.tmt"))] == [32, 32]
    # decode takes no flag: the files say how they were coded (the .tmc of a name is saved after its .tmt)
    assert codec.main(["decode", "-c", str(ck), "-d", str(a), "-o", str(out)]) == 4
    assert Image.open(out / "img0.png").size == (224, 224) and Image.open(out / "img1.png").size == (224, 224)


def test_testing_main_q(tmae, synth, tmp_path):
    from textmae_amd import bitstream as bs
    from textmae_amd import testing

    ds, ck = synth
    common = ["-d", str(ds), "--cuda", "-c", str(ck), "--num_keep_patches", "144", "--input_size", "224"]
    rep = testing.main(common + ["-o", str(tmp_path / "rec"), "--bitstream", str(tmp_path / "tmc"), "--q", "8"])
    files = sorted((tmp_path / "tmc").glob("*.tmc"))
    assert [bs.parse(f.read_bytes()).q for f in files] == [8, 8]
    assert rep["results"]["bpp"][0] == pytest.approx(8.0 * sum(f.stat().st_size for f in files) / 2 / 224 ** 2)
    assert "quantiser step 2^(8/8)" in rep["description"]
    rep = testing.main(common + ["-o", str(tmp_path / "rec2"), "--bitstream", str(tmp_path / "tmt"), "--tiled",
                                 "--overlap", "16", "--q", "-8"])
    files = sorted((tmp_path / "tmt").glob("*.tmt"))
    assert [bs.parse_image(f.read_bytes()).q for f in files] == [-8, -8]
    with pytest.raises(SystemExit):  # --q codes real files
        testing.main(common + ["-o", str(tmp_path / "rec3"), "--q", "8"])
