"""Per-patch quantiser steps through the model: MCM.encode_bytes / decode_bytes / compress_batch /
decompress_batch / forward with qoffsets= and qlevels=, the tiled files and the command lines.  It extends
test_gpu_qstep_model.py, whose SMALL12 model (128 px, K = 16, weights make_state_dict(cfg, 11)), metric and 1e-3 bound it
uses.

Batch 3, input seed 54, qoffsets = (-8, -3, 0, 5), levels from the scores: chosen on the CPU so that the oracle
restatement of the coded path with the per-patch step (qmap_check.oracle_coded) rounds no (y - mu) / delta and no
z - median within 1e-4 of a half-integer at base q = (-16, 0, 5), (0, 0, 0) and (30, -30, 0).  There the images hold
1787 / 267 / 100, 286 / 267 / 307 and 0 / 2618 / 307 non-zero y symbols, every level holds 4 of the 16 kept patches, and
at (30, -30, 0) level 3 of the first image (position 35) saturates at 32 while its levels 0-2 (22, 27, 30) do not, and
levels 0-1 of the second image (-38, -33) saturate at -32.  The tests assert all of that on the reference alone."""
import numpy as np
import pytest
import torch

import qmap_check as mk
import qstep_check as qk
from oracle.mcm_oracle import MCMConfig, make_state_dict
from test_gpu_qstep_model import SMALL12, inputs, maxrel

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED_W, SEED_X = 11, 54
OFFS = (-8, -3, 0, 5)
BASES = ((-16, 0, 5), (0, 0, 0), (30, -30, 0))
NONZERO = {(-16, 0, 5): [1787, 267, 100], (0, 0, 0): [286, 267, 307], (30, -30, 0): [0, 2618, 307]}


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
def oracle():
    """the CPU reference, computed once: the coded path with the per-patch step at the three base positions"""
    cfg = MCMConfig(**SMALL12)
    sd = make_state_dict(cfg, SEED_W)
    imgs, scores = inputs(3, 128, 64, SEED_X)
    return {q: mk.oracle_coded(sd, cfg, imgs, scores, q, OFFS) for q in BASES}


@pytest.fixture(params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def dtyped(request, small):
    small.compute_dtype = request.param
    yield small
    small.compute_dtype = torch.float32


def level_map(ref, L=64):
    """a caller's map [B, L] in image patch order that reproduces the reference's levels of the kept patches"""
    m = np.zeros((ref.n, L), dtype=np.int32)
    K = ref.levels.shape[1]
    for b in range(ref.n):
        m[b, ref.ids_shuffle[b, :K].numpy()] = ref.levels[b]
    return m


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("q", BASES, ids=[",".join(map(str, q)) for q in BASES])
def test_against_the_oracle(tmae, small, xs, oracle, q):
    """f32 against the CPU restatement of the coded path with the per-patch step: symbols equal, x_hat within
    test_gpu_mcm.py's 1e-3"""
    from textmae_amd import bitstream as bs

    ref = oracle[q]
    assert qk.near_ties(ref.t) == 0 and qk.near_ties(ref.z_t) == 0  # on the reference alone
    nz = [int((ref.sym.reshape(12, 3, -1)[:, b] != 0).sum()) for b in range(3)]
    assert nz == NONZERO[q]
    assert all(np.bincount(l, minlength=4).tolist() == [4, 4, 4, 4] for l in ref.levels)
    if q == (30, -30, 0):  # saturation at both ends of the ladder is part of the definition
        lv = ref.levels
        assert set(ref.qmap[0][lv[0] == 3]) == {32} and set(ref.qmap[0][lv[0] == 2]) == {30}
        assert set(ref.qmap[0][lv[0] == 1]) == {27} and set(ref.qmap[0][lv[0] == 0]) == {22}
        assert set(ref.qmap[1][lv[1] <= 1]) == {-32} and set(ref.qmap[1][lv[1] == 2]) == {-30}
    assert small.compute_dtype == torch.float32
    blobs = small.encode_bytes(*xs, q=q, qoffsets=OFFS)
    assert all(b[:4] == b"TPC\x01" for b in blobs)
    parsed = [bs.parse(b) for b in blobs]
    assert [p.q for p in parsed] == list(q) and all(p.offsets == OFFS and p.nlev == 4 for p in parsed)
    lv, st = bs.unpack_levels_host(np.stack([p.levels for p in parsed]), 4, 16)
    assert not st.any() and np.array_equal(lv, ref.levels)
    sym = np.array(small._exec.last_streams["y_symbols"]).reshape(-1)
    bad = int((torch.from_numpy(sym).long() != ref.sym).sum())
    x_hat = small.decode_bytes(blobs)["x_hat"]
    err = maxrel(x_hat, ref.x_hat)
    print(f"base q = {q}, offsets {OFFS}: {bad} of {sym.size} symbols differ from the oracle's, x_hat maxrel {err:.3e}")
    assert bad == 0
    assert err <= 1e-3


# ------------------------------------------------------------------------------------------------ encoder = decoder
@pytest.mark.parametrize("lanes", [1, 8])
def test_decoder_buffers_are_the_encoders(tmae, dtyped, xs, lanes):
    from textmae_amd import bitstream as bs

    m, q = dtyped, BASES[0]
    blobs = m.encode_bytes(*xs, lanes=lanes, q=q, qoffsets=OFFS)
    ex = m._exec
    assert ex.dtype == m.compute_dtype
    enc = {k: getattr(ex, k).clone() for k in ("YH", "SUPY", "YPRE")}
    sym = torch.from_numpy(np.array(ex.last_streams["y_symbols"])).clone()
    idx = torch.from_numpy(np.array(ex.last_streams["y_indexes"])).clone()
    got = m.decode_bytes(blobs)
    x_all = got["x_hat"].clone()
    assert m._exec is ex
    for k, v in enc.items():  # the decoder's slice loop left what the encoder's left, bit for bit
        assert torch.equal(getattr(ex, k), v), k
    assert np.array_equal(np.array(ex.last_decoded["y_symbols"]), sym.numpy())
    assert np.array_equal(np.array(ex.last_decoded["y_indexes"]), idx.numpy())
    for b in range(3):  # one blob per call: the same rows
        assert torch.equal(m.decode_bytes([blobs[b]])["x_hat"][0], x_all[b]), b
    # and through compress_batch / decompress_batch with what compress_batch returned
    out = m.compress_batch(*xs, lanes=lanes, q=q, qoffsets=OFFS)
    assert out["qoffsets"] == OFFS and tuple(out["qlevels"].shape) == (3, 16)
    assert [bytes(bs.parse(b).y) for b in blobs] == list(out["string"][0])
    rec = m.decompress_batch(out["string"], out["shape"], out["ids_restore"], lanes=lanes, q=q, qoffsets=OFFS,
                             qlevels=out["qlevels"])["x_hat"]
    assert torch.equal(rec, x_all)
    rec = m.decompress_batch(out["string"], out["shape"], out["ids_restore"], lanes=lanes, q=q, qoffsets=OFFS,
                             qlevels=out["qlevels"].cpu().numpy())["x_hat"]
    assert torch.equal(rec, x_all)


def test_forward_is_what_the_coder_does(tmae, dtyped, xs, monkeypatch):
    """x_hat of forward(qoffsets=) is the round trip's bit for bit; every launch of tmae_gc_slices_fwd_qm is followed
    by tmae_gc_slices_code_qm on the same operands into a second likelihood buffer: bit for bit the forward's"""
    m, ops, q = dtyped, tmae.ops, BASES[0]
    lik2, n_calls = {}, [0]
    real = ops.gc_slices_fwd_qm

    def both(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, noise, lik, Mtot, yhat, yt, ld_yhat, yhat32, ld32, n, HW, nsl, sw,
             bound, qmap):
        real(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, noise, lik, Mtot, yhat, yt, ld_yhat, yhat32, ld32, n, HW, nsl, sw,
             bound, qmap)
        assert noise is None
        if "lik" not in lik2:
            lik2["lik"] = torch.full((n, Mtot, HW), float("nan"), device=DEV)
            lik2["yh"] = torch.full((n * HW, Mtot), float("nan"), device=DEV)
        sym = torch.empty(nsl * n * sw * HW, dtype=torch.int32, device=DEV)
        ops.gc_slices_code_qm(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, lik2["lik"], Mtot, None, yt, ld_yhat, lik2["yh"],
                              Mtot, n, HW, nsl, sw, sym, torch.empty_like(sym), m.gaussian_conditional.scale_table, bound,
                              qmap)
        n_calls[0] += 1

    monkeypatch.setattr(ops, "gc_slices_fwd_qm", both)
    with torch.no_grad():
        out = m(*xs, q=q, qoffsets=OFFS)
    torch.cuda.synchronize()
    monkeypatch.undo()
    x, ylik = out["x_hat"].clone(), out["likelihoods"]["y"].clone()
    assert n_calls[0] >= 2 and m._exec.dtype == m.compute_dtype  # unchained: the serial slices one launch each
    assert torch.equal(ylik.reshape(lik2["lik"].shape).view(torch.int32), lik2["lik"].view(torch.int32))
    rec = m.decode_bytes(m.encode_bytes(*xs, q=q, qoffsets=OFFS))["x_hat"]
    assert torch.equal(x, rec)
    with torch.no_grad():
        assert not torch.equal(x, m(*xs, q=q)["x_hat"])  # and the offsets change it
        same = m(*xs, q=q, qoffsets=OFFS, qlevels="scores")["x_hat"]
    assert torch.equal(same, x)


def test_forward_is_eval_only(tmae, small, xs):
    with pytest.raises(ValueError, match=r"forward: qoffsets is for evaluation"):
        small(*xs, qoffsets=OFFS)  # autograd on, parameters require grad
    small.train()
    try:
        with torch.no_grad(), pytest.raises(ValueError, match=r"forward: qoffsets is for evaluation"):
            small(*xs, qoffsets=OFFS)
    finally:
        small.eval()


# ------------------------------------------------------------------------------------------------ sources of levels
def test_caller_map_gives_the_same_bytes(tmae, small, xs, oracle):
    q = BASES[0]
    want = small.encode_bytes(*xs, q=q, qoffsets=OFFS)
    m = level_map(oracle[q])
    assert small.encode_bytes(*xs, q=q, qoffsets=OFFS, qlevels=m) == want
    assert small.encode_bytes(*xs, q=q, qoffsets=OFFS, qlevels=torch.from_numpy(m).to(DEV)) == want
    assert small.encode_bytes(*xs, q=q, qoffsets=OFFS, qlevels="scores") == want
    other = (m + 1) % 4
    assert small.encode_bytes(*xs, q=q, qoffsets=OFFS, qlevels=other) != want
    with torch.no_grad():
        a = small(*xs, q=q, qoffsets=OFFS)["x_hat"]
        b = small(*xs, q=q, qoffsets=OFFS, qlevels=torch.from_numpy(m).to(DEV))["x_hat"]
    assert torch.equal(a, b)
    # a device map with an entry outside the table is found on the device and names the image
    bad = torch.from_numpy(m).to(DEV).clone()
    bad[1, int(oracle[q].ids_shuffle[1, 3])] = 4
    with pytest.raises(ValueError, match=r"qlevels of image 1"):
        small.encode_bytes(*xs, q=q, qoffsets=OFFS, qlevels=bad)
    with pytest.raises(ValueError, match=r"qlevels of image 1"), torch.no_grad():
        small(*xs, q=q, qoffsets=OFFS, qlevels=bad)
    assert small.encode_bytes(*xs, q=q, qoffsets=OFFS) == want


def test_zero_offsets_decode_to_the_plain_path(tmae, small, xs):
    from textmae_amd import bitstream as bs

    plain = small.encode_bytes(*xs)
    xp = small.decode_bytes(plain)["x_hat"].clone()
    blobs = small.encode_bytes(*xs, q=0, qoffsets=(0, 0, 0, 0))
    assert all(b[:3] == b"TPC" for b in blobs)
    assert [bytes(bs.parse(b).y) for b in blobs] == [bytes(bs.parse(b).y) for b in plain]
    assert torch.equal(small.decode_bytes(blobs)["x_hat"], xp)
    assert small.encode_bytes(*xs) == plain  # an encode without a map: today's bytes, before and after


def test_record_grows_when_offsets_fall(tmae, small, xs):
    from textmae_amd import bitstream as bs

    a = [len(bs.parse(b).y) for b in small.encode_bytes(*xs, q=0, qoffsets=OFFS)]
    lower = tuple(o - 12 for o in OFFS)
    b = [len(bs.parse(b).y) for b in small.encode_bytes(*xs, q=0, qoffsets=lower)]
    print("y record bytes", a, "with every offset 12 lower", b)
    assert all(y > x for x, y in zip(a, b))
    # only image 1's offsets fall: a caller map that sends its patches to levels 4..7, the same offsets 12 lower
    offs2 = (-8, -3, 0, 5, -20, -15, -12, -7)  # levels 4..7: the same offsets 12 lower
    m = level_map(NS_levels(small, xs))
    m2 = m.copy()
    m2[1] += 4
    c = [len(bs.parse(b).y) for b in small.encode_bytes(*xs, q=0, qoffsets=offs2, qlevels=m)]
    d = [len(bs.parse(b).y) for b in small.encode_bytes(*xs, q=0, qoffsets=offs2, qlevels=m2)]
    print("y record bytes", c, "with the offsets of image 1 alone 12 lower", d)
    assert c == a and d[0] == c[0] and d[2] == c[2] and d[1] > c[1]


def NS_levels(small, xs):
    """the levels the device selected from the scores and its ids_shuffle, in qmap_check.oracle_coded's fields"""
    from types import SimpleNamespace as NS

    out = small.compress_batch(*xs, qoffsets=OFFS)
    shuf = torch.argsort(out["ids_restore"], dim=1).cpu()
    return NS(n=3, levels=out["qlevels"].cpu().numpy(), ids_shuffle=shuf)


# ------------------------------------------------------------------------------------------------ target_bytes
@pytest.mark.parametrize("lanes", [1, 8])
def test_target_bytes_with_offsets(tmae, small, xs, lanes):
    from textmae_amd import bitstream as bs

    s0 = [len(b) for b in small.encode_bytes(*xs, lanes=lanes, q=0, qoffsets=OFFS)]
    s8 = [len(b) for b in small.encode_bytes(*xs, lanes=lanes, q=8, qoffsets=OFFS)]
    target = [(a + b) // 2 for a, b in zip(s0, s8)]
    blobs = small.encode_bytes(*xs, lanes=lanes, target_bytes=target, qoffsets=OFFS)
    qs = [bs.parse(b).q for b in blobs]
    print(f"lanes {lanes}: sizes at base q = 0 {s0}, at 8 {s8}, targets {target} -> q {qs}, "
          f"sizes {[len(b) for b in blobs]}")
    assert all(b[:3] == b"TPC" for b in blobs)
    assert all(len(b) <= t for b, t in zip(blobs, target))  # header, table and level words counted
    assert all(0 < q <= 8 for q in qs)
    assert small.encode_bytes(*xs, lanes=lanes, q=qs, qoffsets=OFFS) == blobs  # the q in the header is the q used
    below = small.encode_bytes(*xs, lanes=lanes, q=[q - 1 for q in qs], qoffsets=OFFS)
    assert all(len(b) > t for b, t in zip(below, target))
    tiny = small.encode_bytes(*xs, lanes=lanes, target_bytes=1, qoffsets=OFFS)
    assert [bs.parse(b).q for b in tiny] == [32, 32, 32]
    with pytest.raises(ValueError, match=r"give q or target_bytes, not both"):
        small.encode_bytes(*xs, q=3, target_bytes=500, qoffsets=OFFS)


# ------------------------------------------------------------------------------------------------ decode_bytes
def test_mixed_kinds_decode_in_one_call(tmae, small, xs):
    plain = small.encode_bytes(*xs)
    a = small.encode_bytes(*xs, q=7)
    p = small.encode_bytes(*xs, q=-3, qoffsets=OFFS)
    p2 = small.encode_bytes(*xs, q=2, qoffsets=(4, -4))  # another table size in the same call
    assert (plain[0][:3], a[0][:3], p[0][:3]) == (b"TMC", b"TQC", b"TPC")
    xp, xa, xq, x2 = (small.decode_bytes(v)["x_hat"].clone() for v in (plain, a, p, p2))
    got = small.decode_bytes([p[2], plain[0], a[1], p2[0], p[1]])["x_hat"]
    for g, w in zip(got, (xq[2], xp[0], xa[1], x2[0], xq[1])):
        assert torch.equal(g, w)
    assert not torch.equal(xq[0], xp[0])


def test_errors_before_any_launch(tmae, small, xs, monkeypatch):
    """every one of these is raised on the host: the library is not called at all"""
    from textmae_amd import _lib

    plain = small.encode_bytes(*xs)
    out = small.compress_batch(*xs, qoffsets=OFFS)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for bad, msg in (((1,), r"nlev = 1 outside 2\.\.16"), ((0,) * 17, r"nlev = 17 outside 2\.\.16"),
                     ((0, 65), r"offset outside -64\.\.64"), ((0, 0.5), r"offset outside -64\.\.64")):
        with pytest.raises(ValueError, match=msg):
            small.encode_bytes(*xs, qoffsets=bad)
        with pytest.raises(ValueError, match=msg):
            small.compress_batch(*xs, qoffsets=bad)
        with pytest.raises(ValueError, match=msg), torch.no_grad():
            small(*xs, qoffsets=bad)
    with pytest.raises(ValueError, match=r"qlevels without qoffsets"):
        small.encode_bytes(*xs, qlevels="scores")
    with pytest.raises(ValueError, match=r"qlevels of image 2: a level outside 0\.\.3"):
        m = np.zeros((3, 64), dtype=np.int64)
        m[2, 5] = 4
        small.encode_bytes(*xs, qoffsets=OFFS, qlevels=m)
    with pytest.raises(ValueError, match=r"qlevels must be 'scores' or an integer map \[3, 64\]"):
        small.encode_bytes(*xs, qoffsets=OFFS, qlevels=np.zeros((3, 16), dtype=np.int32))
    with pytest.raises(ValueError, match=r"qlevels must be 'scores' or an integer map"):
        small.encode_bytes(*xs, qoffsets=OFFS, qlevels=np.zeros((3, 64), dtype=np.float32))
    with pytest.raises(ValueError, match=r"a device qlevels must be a contiguous int32"):
        small.encode_bytes(*xs, qoffsets=OFFS, qlevels=torch.zeros(3, 64, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match=r"outside -32\.\.32"):
        small.encode_bytes(*xs, q=40, qoffsets=OFFS)
    with pytest.raises(ValueError, match=r"decompress_batch: qlevels"):
        small.decompress_batch(out["string"], out["shape"], out["ids_restore"], qoffsets=OFFS)
    with pytest.raises(ValueError, match=r"decompress_batch: qlevels of image 0"):
        small.decompress_batch(out["string"], out["shape"], out["ids_restore"], qoffsets=OFFS,
                               qlevels=np.full((3, 16), 7))
    assert calls == []
    monkeypatch.undo()
    assert small.encode_bytes(*xs) == plain


def test_corrupt_level_section_names_the_image(tmae, small, xs):
    from textmae_amd import bitstream as bs

    # nlev = 3: two bits a level, so the level 3 can be written; K = 16 levels fill one word exactly
    blobs = small.encode_bytes(*xs, q=1, qoffsets=(-4, 0, 4))
    want = small.decode_bytes(blobs)["x_hat"].clone()
    at = bs.PHEADER_BYTES + 4 * bs.id_words(64, 16)  # the level word
    lv, _ = bs.unpack_levels_host(np.stack([bs.parse(b).levels for b in blobs]), 3, 16)
    k = int(np.flatnonzero(lv[1] == 2)[0])           # flip the low bit of a level 2 -> 3
    bad = bytearray(blobs[1])
    bad[at + (2 * k) // 8] ^= 1 << ((2 * k) % 8)
    with pytest.raises(ValueError, match=r"side information of image 1: quantiser level outside its table"):
        small.decode_bytes([blobs[0], bytes(bad), blobs[2]])
    got = small.decode_bytes([blobs[0], blobs[2]])["x_hat"]  # the others are untouched
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[2])
    # nlev = 5: three bits a level, 48 of 64 bits used: a tail bit
    blobs = small.encode_bytes(*xs, qoffsets=(-4, -2, 0, 2, 4))
    at2 = at + 4 * bs.level_words(16, 5) - 1
    bad = bytearray(blobs[2])
    bad[at2] |= 0x80
    with pytest.raises(ValueError, match=r"side information of image 2: non-zero padding bits of the level section"):
        small.decode_bytes([blobs[0], blobs[1], bytes(bad)])
    with pytest.raises(ValueError, match=r"blob 1: TPC stream with nlev = 1"):
        b = bytearray(blobs[1])
        b[17] = 1
        small.decode_bytes([blobs[0], bytes(b)])
    assert torch.equal(small.decode_bytes(small.encode_bytes(*xs, q=1, qoffsets=(-4, 0, 4)))["x_hat"], want)


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
    assert plain[:4] == b"TMT\x01" and small.encode_image(image, overlap=O0, qoffsets=None) == plain
    tq = small.encode_image(image, overlap=O0, q=5)
    blob = small.encode_image(image, overlap=O0, q=2, qoffsets=OFFS)
    assert blob[:4] == b"TPT\x01"
    p = bs.parse_image(blob)
    assert (p.q, p.nlev, p.offsets, p.num_tiles) == (2, 4, OFFS, 4) and (p.width, p.height, p.overlap) == (W0, H0, O0)
    tiles = [bs.tile_blob(p, t) for t in range(4)]
    assert all(t[:4] == b"TPC\x01" and bs.parse(t).q == 2 for t in tiles)
    for t in range(4):  # every tile: 4 kept patches per level, from the tile's own scores
        lv, st = bs.unpack_levels_host(p.levels[t][None], 4, 16)
        assert not st.any() and np.bincount(lv[0], minlength=4).tolist() == [4, 4, 4, 4]
    want = ops.tile_blend(small.decode_bytes(tiles)["x_hat"], H0, W0, O0)
    full = small.decode_image(blob)
    assert torch.equal(full, want)
    assert not torch.equal(full, small.decode_image(small.encode_image(image, overlap=O0, q=2)))
    win = (100, 20, 40, 30)  # x0, y0, w, h: columns 100..139 lie in both tile columns (stride 112, overlap 16)
    assert torch.equal(small.decode_region(blob, *win), full[:, 20:50, 100:140])
    assert torch.equal(small.decode_crops([blob], [(100, 20)], (40, 30))[0], full[:, 20:50, 100:140])
    # a TPT, a TQT and a TMT file, and a TPT file with another table, in one call
    other = small.encode_image(image, overlap=O0, qoffsets=(6, -6))
    both = small.decode_crops([blob, tq, plain, other, blob], [(100, 20), (5, 110), (60, 60), (90, 90), (0, 0)], (40, 30))
    assert torch.equal(both[0], full[:, 20:50, 100:140]) and torch.equal(both[4], full[:, 0:30, 0:40])
    assert torch.equal(both[1], small.decode_image(tq)[:, 110:140, 5:45])
    assert torch.equal(both[2], small.decode_image(plain)[:, 60:90, 60:100])
    assert torch.equal(both[3], small.decode_image(other)[:, 90:120, 90:130])
    # target_bytes with a table: within budget, the file says which base q
    s0, s8 = len(small.encode_image(image, overlap=O0, q=0, qoffsets=OFFS)), len(
        small.encode_image(image, overlap=O0, q=8, qoffsets=OFFS))
    fit = small.encode_image(image, overlap=O0, target_bytes=(s0 + s8) // 2, qoffsets=OFFS)
    qf = bs.parse_image(fit).q
    assert len(fit) <= (s0 + s8) // 2 and 0 < qf <= 8 and fit == small.encode_image(image, overlap=O0, q=qf, qoffsets=OFFS)
    # a corrupt level section of a tile names the tile
    blob3 = small.encode_image(image, overlap=O0, qoffsets=(-4, 0, 4))
    bad = bytearray(blob3)
    at = int(bs.read_image_index(blob3).ids_at[2]) + 4 * bs.id_words(64, 16)
    bad[at:at + 4] = b"\xff\xff\xff\xff"  # nlev = 3: the invalid level 3
    with pytest.raises(ValueError, match=r"side information of tile 2: quantiser level outside its table"):
        small.decode_image(bytes(bad))
    with pytest.raises(ValueError, match=r"encode_image: qoffsets: nlev = 1 outside 2\.\.16"):
        small.encode_image(image, overlap=O0, qoffsets=(3,))


# ------------------------------------------------------------------------------------------------ command lines
@pytest.fixture(scope="module")
def synth(tmae, tmp_path_factory, image):
    """two synthetic PNGs and a seeded checkpoint of the command lines' model (224^2, K = 144)"""
    from PIL import Image

    root = tmp_path_factory.mktemp("qmap_cli")
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
    with pytest.raises(SystemExit):
        codec.main(enc + ["-o", str(a), "--q-offsets", "5"])  # one offset is no table
    capsys.readouterr()
    assert codec.main(enc + ["-o", str(a), "--q", "6", "--q-offsets", "-8,-3,0,5"]) == 2
    got = [bs.parse(f.read_bytes()) for f in sorted(a.glob("*.tmc"))]
    assert [(p.q, p.offsets) for p in got] == [(6, OFFS)] * 2
    assert codec.main(enc + ["-o", str(a), "--tiled", "--overlap", "16", "--target-bytes", "1",
                             "--q-offsets=-2,2"]) == 2
    assert capsys.readouterr().err.count("above --target-bytes 1") == 2
    assert [(p.q, p.offsets) for p in (bs.parse_image(f.read_bytes()) for f in sorted(a.glob("*.tmt")))] == [
        (32, (-2, 2))] * 2
    # decode takes no flag: the files say how they were coded
    assert codec.main(["decode", "-c", str(ck), "-d", str(a), "-o", str(out)]) == 4
    assert Image.open(out / "img0.png").size == (224, 224) and Image.open(out / "img1.png").size == (224, 224)


def test_testing_main(tmae, synth, tmp_path):
    from textmae_amd import bitstream as bs
    from textmae_amd import testing

    ds, ck = synth
    common = ["-d", str(ds), "--cuda", "-c", str(ck), "--num_keep_patches", "144", "--input_size", "224"]
    rep = testing.main(common + ["-o", str(tmp_path / "rec"), "--bitstream", str(tmp_path / "tmc"), "--q", "8",
                                 "--q-offsets", "-8,-3,0,5"])
    files = sorted((tmp_path / "tmc").glob("*.tmc"))
    assert [(bs.parse(f.read_bytes()).q, bs.parse(f.read_bytes()).offsets) for f in files] == [(8, OFFS)] * 2
    assert rep["results"]["bpp"][0] == pytest.approx(8.0 * sum(f.stat().st_size for f in files) / 2 / 224 ** 2)
    assert "per-patch ladder offsets -8,-3,0,5" in rep["description"]
    rep = testing.main(common + ["-o", str(tmp_path / "rec2"), "--bitstream", str(tmp_path / "tmt"), "--tiled",
                                 "--overlap", "16", "--q-offsets", "-4,4"])
    files = sorted((tmp_path / "tmt").glob("*.tmt"))
    assert [(p.q, p.offsets) for p in (bs.parse_image(f.read_bytes()) for f in files)] == [(0, (-4, 4))] * 2
    est = testing.main(common + ["-o", str(tmp_path / "rec3"), "--entropy-estimation", "--q-offsets", "-8,-3,0,5"])
    base = testing.main(common + ["-o", str(tmp_path / "rec4"), "--entropy-estimation"])
    assert est["results"]["bpp"][0] != base["results"]["bpp"][0]
    with pytest.raises(SystemExit):  # --q-offsets codes real files or estimates
        testing.main(common + ["-o", str(tmp_path / "rec5"), "--q-offsets", "-4,4"])
