"""Rate-distortion optimised quantisation of y through the model: MCM.compress_batch / encode_bytes /
encode_image with rdoq=, decoded by today's decode_bytes / decompress_batch / decode_image / decode_region, and the
command lines.

SMALL12 of test_gpu_qstep_model.py (128 px, K = 16, weights make_state_dict(cfg, 11)), batch 3, input seed 47, f32.  At
q = -16 the plain run holds 1713 / 1649 / 1781 non-zero y symbols; W = 0.004 was chosen on the CPU so that the restated
coded path (rdoq_check.oracle_coded) moves about 1000 of them per image, rounds no (y - mu) / delta within 1e-4 of a
half-integer and takes no decision with |lhs - rhs| below 1e-4 of max(|lhs|, |rhs|, 1e-6); the test asserts both on the
reference alone."""
import numpy as np
import pytest
import torch

import qstep_check as qk
import rdoq_check as rk
from oracle.mcm_oracle import MCMConfig, make_state_dict
from test_gpu_qstep_model import H0, O0, SEED_W, SEED_X, SMALL12, W0, image, inputs, maxrel, synth  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
W = 0.004
Q = -16
QMIX = (-16, 0, 5)
OFFS = (-8, 0, 4)


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


def streams(small):
    ls = small._exec.last_streams
    return {k: np.array(ls[k]).copy() for k in ls}


def per_image(a, b):
    """image b's y symbols or indexes in its record's order, from the flat [slice][image][channel][pixel] buffer"""
    return a.reshape(12, 3, -1)[:, b].reshape(-1)


# ------------------------------------------------------------------------------------------------ identity
@pytest.mark.parametrize("kw", [dict(), dict(q=QMIX), dict(qoffsets=OFFS), dict(q=QMIX, qoffsets=OFFS, lanes=8)],
                         ids=["q0", "qmix", "qoffsets", "qmix_qoffsets_lanes8"])
def test_weight_zero_is_todays_bytes(tmae, small, xs, kw):
    want = small.encode_bytes(*xs, **kw)
    assert "y_changed" not in small._exec.last_streams
    plain = streams(small)
    for w in (0.0, [0.0, 0.0, 0.0], np.zeros(3)):
        assert small.encode_bytes(*xs, rdoq=w, **kw) == want
        got = streams(small)
        assert np.array_equal(got["y_changed"], np.zeros(3, dtype=np.int32))
        for k in plain:
            assert np.array_equal(got[k], plain[k]), k
    out = small.compress_batch(*xs, rdoq=0.0, **kw)
    assert out["rdoq"] == [0.0, 0.0, 0.0] and "rdoq" not in small.compress_batch(*xs, **kw)
    assert small.encode_bytes(*xs, **kw) == want  # the plain path is untouched afterwards


# ------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("lanes", [1, 8])
def test_round_trip(tmae, small, xs, lanes):
    from textmae_amd import bitstream as bs

    plain = small.encode_bytes(*xs, lanes=lanes, q=Q)
    blobs = small.encode_bytes(*xs, lanes=lanes, q=Q, rdoq=W)
    ex = small._exec
    enc = {k: getattr(ex, k).clone() for k in ("YH", "SUPY", "YPRE")}
    st = streams(small)
    assert (st["y_changed"] > 0).all()
    assert all(b[:4] == b"TQC\x01" for b in blobs) and [bs.parse(b).q for b in blobs] == [Q] * 3
    for b in range(3):  # the side information and the z records are the plain ones, the y records are not
        p, w = bs.parse(blobs[b]), bs.parse(plain[b])
        assert bytes(p.z) == bytes(w.z) and np.array_equal(p.ids, w.ids) and bytes(p.y) != bytes(w.y)
    x_all = small.decode_bytes(blobs)["x_hat"].clone()
    assert small._exec is ex
    for k, v in enc.items():  # the decoder's slice loop left what the encoder's left, bit for bit
        assert torch.equal(getattr(ex, k), v), k
    assert np.array_equal(np.array(ex.last_decoded["y_symbols"]), st["y_symbols"])
    assert np.array_equal(np.array(ex.last_decoded["y_indexes"]), st["y_indexes"])
    # the same records through compress_batch / decompress_batch, which takes no rdoq
    out = small.compress_batch(*xs, lanes=lanes, q=Q, rdoq=W)
    assert out["rdoq"] == [W] * 3
    assert [bytes(bs.parse(b).y) for b in blobs] == list(out["string"][0])
    rec = small.decompress_batch(out["string"], out["shape"], out["ids_restore"], lanes=lanes, q=Q)["x_hat"]
    assert torch.equal(rec, x_all)
    assert not torch.equal(x_all, small.decode_bytes(plain)["x_hat"])
    for b in range(3):  # per-image weights: image b alone at its weight is image b of the batch
        one = small.encode_bytes(*xs, lanes=lanes, q=Q, rdoq=[W if i == b else 0.0 for i in range(3)])
        assert one[b] == blobs[b] and all(one[i] == plain[i] for i in range(3) if i != b)
    assert small.encode_bytes(*xs, lanes=lanes, q=Q) == plain


# ------------------------------------------------------------------------------------------------ rate
def test_rate(tmae, small, xs):
    """the moved symbols cost fewer bits under the tables than the plain run's.  Record bytes are not compared across
    the two runs: the later slices see other contexts"""
    from textmae_amd import coder

    tabs = small.gaussian_conditional.host_tables()
    small.encode_bytes(*xs, q=Q)
    plain = streams(small)
    small.encode_bytes(*xs, q=Q, rdoq=W)
    got = streams(small)
    for b in range(3):
        tp = coder.table_bits(per_image(plain["y_symbols"], b), per_image(plain["y_indexes"], b), *tabs)
        tg = coder.table_bits(per_image(got["y_symbols"], b), per_image(got["y_indexes"], b), *tabs)
        nzp, nzg = (int((per_image(s["y_symbols"], b) != 0).sum()) for s in (plain, got))
        print(f"image {b}: table_bits {tp:.1f} -> {tg:.1f}, non-zero symbols {nzp} -> {nzg}, "
              f"y_changed {int(got['y_changed'][b])}")
        assert got["y_changed"][b] > 0
        assert tg < tp


# ------------------------------------------------------------------------------------------------ CPU restatement
def test_against_the_oracle(tmae, small, xs):
    """f32 against the CPU restatement of the coded path with the rule in its slice loop and the model's own tables:
    symbols and the counts of moved symbols equal, x_hat within test_gpu_mcm.py's 1e-3"""
    from types import SimpleNamespace as NS

    gc = small.gaussian_conditional
    _, sizes, offsets = gc.host_tables()
    tb = NS(sizes=sizes, offsets=offsets, rate=gc.rate_table())
    cfg = MCMConfig(**SMALL12)
    imgs, scores = inputs(3, 128, 64, SEED_X)
    ref = rk.oracle_coded(make_state_dict(cfg, SEED_W), cfg, imgs, scores, (Q,) * 3, (W,) * 3, tb,
                          gc.scale_table.cpu().numpy())
    ties, near = qk.near_ties(ref.t), rk.near_decisions(ref.lhs, ref.rhs)
    print(f"reference: {ties} near ties, {near} near decisions of {ref.lhs.size}, moved {ref.changed.tolist()}")
    assert ties == 0 and near == 0  # on the reference alone
    assert (ref.changed > 0).all() and (ref.changed < np.array([1713, 1649, 1781])).all()
    assert small.compute_dtype == torch.float32
    blobs = small.encode_bytes(*xs, q=Q, rdoq=W)
    st = streams(small)
    bad = int((torch.from_numpy(st["y_symbols"].reshape(-1)).long() != ref.sym).sum())
    err = maxrel(small.decode_bytes(blobs)["x_hat"], ref.x_hat)
    print(f"q = {Q}, rdoq = {W}: {bad} of {ref.sym.numel()} symbols differ from the oracle's, y_changed "
          f"{st['y_changed'].tolist()}, x_hat maxrel {err:.3e}")
    assert bad == 0
    assert st["y_changed"].tolist() == ref.changed.tolist()
    assert err <= 1e-3


# ------------------------------------------------------------------------------------------------ target_bytes
@pytest.mark.parametrize("kw", [dict(), dict(qoffsets=OFFS)], ids=["q", "qoffsets"])
def test_target_bytes(tmae, small, xs, kw):
    from textmae_amd import bitstream as bs

    s0 = [len(b) for b in small.encode_bytes(*xs, q=-16, rdoq=W, **kw)]
    s8 = [len(b) for b in small.encode_bytes(*xs, q=-8, rdoq=W, **kw)]
    target = [(a + b) // 2 for a, b in zip(s0, s8)]
    blobs = small.encode_bytes(*xs, target_bytes=target, rdoq=W, **kw)
    assert (streams(small)["y_changed"] >= 0).all()
    qs = [bs.parse(b).q for b in blobs]
    print(f"sizes at q = -16 {s0}, at q = -8 {s8}, targets {target} -> q {qs}, sizes {[len(b) for b in blobs]}")
    assert all(len(b) <= t for b, t in zip(blobs, target))
    assert all(-16 < q <= -8 for q in qs)
    assert small.encode_bytes(*xs, q=qs, rdoq=W, **kw) == blobs
    assert small.encode_bytes(*xs, q=qs, **kw) != blobs
    assert torch.equal(small.decode_bytes(blobs)["x_hat"],
                       small.decode_bytes(small.encode_bytes(*xs, q=qs, rdoq=W, **kw))["x_hat"])


# ------------------------------------------------------------------------------------------------ tiled files
@pytest.mark.parametrize("kw", [dict(q=Q), dict(q=Q, qoffsets=OFFS)], ids=["tqt", "tpt"])
def test_tiled_files(tmae, small, image, kw):  # noqa: F811
    from textmae_amd import bitstream as bs
    from textmae_amd import ops

    plain = small.encode_image(image, overlap=O0, **kw)
    assert small.encode_image(image, overlap=O0, rdoq=0.0, **kw) == plain
    blob = small.encode_image(image, overlap=O0, rdoq=W, **kw)
    assert blob[:4] == plain[:4] and blob != plain
    p = bs.parse_image(blob)
    assert p.q == Q and p.num_tiles == 4 and (p.width, p.height, p.overlap) == (W0, H0, O0)
    tiles = [bs.tile_blob(p, t) for t in range(4)]
    want = ops.tile_blend(small.decode_bytes(tiles)["x_hat"], H0, W0, O0)
    full = small.decode_image(blob)
    assert torch.equal(full, want)
    assert not torch.equal(full, small.decode_image(plain))
    assert torch.equal(small.decode_region(blob, 100, 20, 40, 30), full[:, 20:50, 100:140])
    # with target_bytes the weight is the same in every probe
    target = (len(blob) + len(small.encode_image(image, overlap=O0, rdoq=W, **dict(kw, q=Q + 8)))) // 2
    kw2 = {k: v for k, v in kw.items() if k != "q"}
    fit = small.encode_image(image, overlap=O0, rdoq=W, target_bytes=target, **kw2)
    qf = bs.parse_image(fit).q
    assert len(fit) <= target and Q < qf <= Q + 8
    assert fit == small.encode_image(image, overlap=O0, rdoq=W, **dict(kw, q=qf))
    with pytest.raises(ValueError, match=r"one weight for every tile"):
        small.encode_image(image, overlap=O0, rdoq=[W, W])


# ------------------------------------------------------------------------------------------------ command lines
def test_codec_cli(tmae, synth, tmp_path, capsys):  # noqa: F811
    from PIL import Image

    from textmae_amd import bitstream as bs
    from textmae_amd import codec

    ds, ck = synth
    enc = ["encode", "-c", str(ck), "-d", str(ds)]
    a, b, out = tmp_path / "plain", tmp_path / "rdoq", tmp_path / "png"
    for bad in ("-1", "nan", "inf", "x"):
        with pytest.raises(SystemExit):
            codec.main(enc + ["-o", str(b), "--rdoq", bad])
    capsys.readouterr()
    assert codec.main(enc + ["-o", str(a), "--q", "-16"]) == 2
    assert codec.main(enc + ["-o", str(b), "--q", "-16", "--rdoq", "0.01"]) == 2
    fa, fb = sorted(a.glob("*.tmc")), sorted(b.glob("*.tmc"))
    assert [bs.parse(f.read_bytes()).q for f in fb] == [-16, -16]
    assert all(x.read_bytes() != y.read_bytes() and x.read_bytes()[:4] == y.read_bytes()[:4] for x, y in zip(fa, fb))
    assert codec.main(enc + ["-o", str(b), "--tiled", "--overlap", "16", "--target-bytes", "1", "--rdoq", "0.01",
                             "--q-offsets", "-8,0,4"]) == 2
    assert [bs.parse_image(f.read_bytes()).q for f in sorted(b.glob("*.tmt"))] == [32, 32]
    capsys.readouterr()
    # decode takes no flag: nothing of the weight is in the files
    assert codec.main(["decode", "-c", str(ck), "-d", str(b), "-o", str(out)]) == 4
    assert Image.open(out / "img0.png").size == (224, 224) and Image.open(out / "img1.png").size == (224, 224)


def test_testing_main_rdoq(tmae, synth, tmp_path):  # noqa: F811
    from textmae_amd import bitstream as bs
    from textmae_amd import testing

    ds, ck = synth
    common = ["-d", str(ds), "--cuda", "-c", str(ck), "--num_keep_patches", "144", "--input_size", "224"]
    rep = testing.main(common + ["-o", str(tmp_path / "rec"), "--bitstream", str(tmp_path / "tmc"), "--q", "-16",
                                 "--rdoq", "0.01"])
    files = sorted((tmp_path / "tmc").glob("*.tmc"))
    assert [bs.parse(f.read_bytes()).q for f in files] == [-16, -16]
    assert rep["results"]["bpp"][0] == pytest.approx(8.0 * sum(f.stat().st_size for f in files) / 2 / 224 ** 2)
    assert "weight 0.01 per bit" in rep["description"] and "quantiser step 2^(-16/8)" in rep["description"]
    rep = testing.main(common + ["-o", str(tmp_path / "rec2"), "--bitstream", str(tmp_path / "tmt"), "--tiled",
                                 "--overlap", "16", "--rdoq", "0.5"])
    assert len(sorted((tmp_path / "tmt").glob("*.tmt"))) == 2 and "weight 0.5 per bit" in rep["description"]
    with pytest.raises(SystemExit):  # an encoder decision: it needs real files
        testing.main(common + ["-o", str(tmp_path / "rec3"), "--rdoq", "0.5"])
    with pytest.raises(SystemExit):
        testing.main(common + ["-o", str(tmp_path / "rec4"), "--entropy-estimation", "--rdoq", "0.5"])


# ------------------------------------------------------------------------------------------------ errors
def test_errors_before_any_launch(tmae, small, xs, image, monkeypatch):  # noqa: F811
    """every one of these is raised on the host: the library is not called at all"""
    from textmae_amd import _lib

    plain = small.encode_bytes(*xs)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for bad in (-0.5, float("nan"), float("inf"), -float("inf"), [0.1, -1.0, 0.1], [0.1, float("nan"), 0.1], 1e39):
        for f in (small.encode_bytes, small.compress_batch):
            with pytest.raises(ValueError, match=r"must be finite and >= 0"):
                f(*xs, rdoq=bad)
        with pytest.raises(ValueError, match=r"must be finite and >= 0"):
            small.encode_bytes(*xs, rdoq=bad, target_bytes=500)
    for bad in ("0.1", [0.1, None, 0.1], True):
        with pytest.raises(ValueError, match=r"is not a number"):
            small.encode_bytes(*xs, rdoq=bad)
    for f in (small.encode_bytes, small.compress_batch):
        with pytest.raises(ValueError, match=r"2 entries of rdoq for 3 images"):
            f(*xs, rdoq=[0.1, 0.2])
    with pytest.raises(ValueError, match=r"4 entries of rdoq for 3 images"):
        small.encode_bytes(*xs, rdoq=np.ones(4), q=3)
    with pytest.raises(ValueError, match=r"must be finite and >= 0"):
        small.encode_image(image, overlap=O0, rdoq=-1.0)
    with pytest.raises(ValueError, match=r"one weight for every tile"):
        small.encode_image(image, overlap=O0, rdoq=[0.1])
    assert calls == []
    monkeypatch.undo()
    assert small.encode_bytes(*xs) == plain
