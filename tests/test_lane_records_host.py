"""Lane-interleaved rANS records, host side (textmae_amd.coder.encode_record / decode_record / parse_record) and the
host-side validation of ops.rans_encode_lanes / rans_decode_lanes.  CPU only.

A record deals a stream's symbols ([nseg][seg_len]) round-robin over `lanes` sub-streams, each an ordinary stream
of the host coder; for lanes >= 2 a header of lanes + 1 words (lanes, then the word count of every sub-stream)
precedes them, lanes = 1 is the plain stream.  The oracle is the host coder itself (csrc/rans.cpp through
RansEncoder) and, for one sub-stream, the pure-Python restatement oracle/rans_oracle.py."""
import numpy as np
import pytest
import torch

from oracle import rans_oracle as ro

NSEG, SEG_LEN = 3, 111
EMPTY = bytes([0, 0, 0, 0x80, 0, 0, 0, 0])


@pytest.fixture(scope="module")
def coder(tmae):
    from textmae_amd import coder as c

    return c


def make_tables(rng, widths, to_cdf):
    """one CDF row per width (pmf entries incl. the tail bin), sizes = entries of the row, offsets = -centre"""
    cdfs, sizes, offsets = [], [], []
    for n in widths:
        p = rng.random(n).astype(np.float64) ** 3 + 1e-4
        cdf = to_cdf((p / p.sum()).astype(np.float32))
        cdfs.append(cdf)
        sizes.append(len(cdf))
        offsets.append(-(n // 2))
    t = np.zeros((len(cdfs), max(sizes)), dtype=np.int32)
    for i, c in enumerate(cdfs):
        t[i, :len(c)] = c
    return t, np.array(sizes, dtype=np.int32), np.array(offsets, dtype=np.int32)


def make_symbols(rng, idx, sizes, offsets, extremes=True, far_frac=0.05):
    """~90 % inside the row's support, ~5 % 1..3 outside on either side, ~5 % (far_frac) |v| up to 2^20, two values
    at +-2^27"""
    maxv = sizes[idx].astype(np.int64) - 2  # values [0, maxv) are coded directly
    off = offsets[idx].astype(np.int64)
    v = off + (rng.random(idx.shape) * maxv).astype(np.int64)
    u = rng.random(idx.shape)
    k = rng.integers(1, 4, idx.shape)
    side = rng.random(idx.shape) < 0.5
    near = np.where(side, off - k, off + maxv - 1 + k)
    far = rng.integers(-(1 << 20), (1 << 20) + 1, idx.shape)
    v = np.where(u < 0.05, near, v)
    v = np.where(u >= 1.0 - far_frac, far, v)
    if extremes and v.size >= 8:
        flat = v.reshape(-1)
        flat[flat.size // 3] = 1 << 27
        flat[2 * flat.size // 3] = -(1 << 27)
    return v.astype(np.int32)


@pytest.fixture(scope="module")
def data(coder):
    rng = np.random.default_rng(3)
    tabs = make_tables(rng, [3, 5, 8, 21, 64, 65, 300, 2500], coder.pmf_to_quantized_cdf)
    idx = rng.integers(0, tabs[1].size, NSEG * SEG_LEN).astype(np.int32)
    sym = make_symbols(rng, idx, tabs[1], tabs[2])
    assert np.abs(sym.astype(np.int64)).max() == 1 << 27
    return sym, idx, tabs


@pytest.mark.parametrize("lanes", [1, 2, 16, 64])
def test_record_round_trip(coder, data, lanes):
    sym, idx, tabs = data
    rec = coder.encode_record(sym, idx, NSEG, SEG_LEN, lanes, tabs)
    assert np.array_equal(coder.decode_record(rec, idx, NSEG, SEG_LEN, lanes, tabs), sym)
    # the record is its sub-streams behind the header: the sizes add up, and every sub-stream is the host coder's
    subs = [coder.RansEncoder().encode_with_indexes(s, i, *tabs)
            for s, i in zip(coder.lane_split(sym, NSEG, SEG_LEN, lanes), coder.lane_split(idx, NSEG, SEG_LEN, lanes))]
    if lanes == 1:
        assert rec == subs[0]
        return
    assert len(rec) == sum(len(s) for s in subs) + 4 * (lanes + 1)
    offsets, counts = coder.parse_record(rec, lanes)
    assert offsets.dtype == np.int64 and counts.dtype == np.int32 and offsets[0] == lanes + 1
    for l in range(lanes):
        assert rec[4 * offsets[l]:4 * (offsets[l] + counts[l])] == subs[l], f"lane {l}"
    assert np.frombuffer(rec, dtype="<u4", count=lanes + 1).tolist() == [lanes] + [len(s) // 4 for s in subs]


def test_lane_split_is_the_numpy_slice(coder, data):
    sym = data[0]
    for lanes in (1, 4, 64):
        got = coder.lane_split(sym, NSEG, SEG_LEN, lanes)
        assert len(got) == lanes
        for l in range(lanes):
            assert np.array_equal(got[l], sym.reshape(NSEG, SEG_LEN)[:, l::lanes].reshape(-1))
    with pytest.raises(ValueError, match="nseg \\* seg_len"):
        coder.lane_split(sym, NSEG, SEG_LEN + 1, 4)
    with pytest.raises(ValueError, match="power of two"):
        coder.lane_split(sym, NSEG, SEG_LEN, 3)


def test_lanes_one_is_the_plain_stream(coder, data):
    sym, idx, tabs = data
    plain = coder.RansEncoder().encode_with_indexes(sym, idx, *tabs)
    assert coder.encode_record(sym, idx, NSEG, SEG_LEN, 1, tabs) == plain
    offsets, counts = coder.parse_record(plain, 1)
    assert offsets.tolist() == [0] and counts.tolist() == [len(plain) // 4]


def test_empty_lanes_are_the_empty_stream(coder, data):
    """seg_len 5 over 8 lanes: lanes 5..7 code nothing, which is the 8-byte flush of state 2^31"""
    _, _, tabs = data
    rng = np.random.default_rng(8)
    idx = rng.integers(0, tabs[1].size, 2 * 5).astype(np.int32)
    sym = make_symbols(rng, idx, tabs[1], tabs[2])
    rec = coder.encode_record(sym, idx, 2, 5, 8, tabs)
    offsets, counts = coder.parse_record(rec, 8)
    assert coder.EMPTY_STREAM == EMPTY
    for l in range(8):
        sub = rec[4 * offsets[l]:4 * (offsets[l] + counts[l])]
        assert (sub == EMPTY) == (l >= 5), f"lane {l}"
    assert np.array_equal(coder.decode_record(rec, idx, 2, 5, 8, tabs), sym)


def test_sub_stream_equals_python_restatement(coder, data):
    sym, idx, tabs = data
    lanes, l = 16, 5
    rec = coder.encode_record(sym, idx, NSEG, SEG_LEN, lanes, tabs)
    offsets, counts = coder.parse_record(rec, lanes)
    s = sym.reshape(NSEG, SEG_LEN)[:, l::lanes].reshape(-1).tolist()
    i = idx.reshape(NSEG, SEG_LEN)[:, l::lanes].reshape(-1).tolist()
    want = ro.encode(s, i, *[t.tolist() for t in tabs])
    assert rec[4 * offsets[l]:4 * (offsets[l] + counts[l])] == want


def test_parse_record_rejects_malformed_headers(coder, data):
    sym, idx, tabs = data
    lanes = 4
    rec = coder.encode_record(sym, idx, NSEG, SEG_LEN, lanes, tabs)
    words = np.frombuffer(rec, dtype="<u4").copy()
    with pytest.raises(ValueError, match="whole number of 32-bit words"):
        coder.parse_record(rec[:-1], lanes)
    with pytest.raises(ValueError, match="4 lanes, 8 expected"):
        coder.parse_record(rec, 8)
    bad = words.copy()
    bad[0] = 2
    with pytest.raises(ValueError, match="2 lanes, 4 expected"):
        coder.parse_record(bad.tobytes(), lanes)
    bad = words.copy()
    bad[1], bad[2] = 1, bad[2] + bad[1] - 1  # the sum still fits: only the short count is wrong
    with pytest.raises(ValueError, match="< 2"):
        coder.parse_record(bad.tobytes(), lanes)
    bad = words.copy()
    bad[3] += 1
    with pytest.raises(ValueError, match="sum to"):
        coder.parse_record(bad.tobytes(), lanes)
    with pytest.raises(ValueError, match="sum to"):
        coder.parse_record(rec + b"\0\0\0\0", lanes)
    with pytest.raises(ValueError, match="shorter than the header"):
        coder.parse_record(rec[:8], lanes)
    with pytest.raises(ValueError, match="power of two"):
        coder.parse_record(rec, 3)
    with pytest.raises(ValueError, match="lanes, 4 expected"):
        coder.decode_record(words[1:].tobytes(), idx, NSEG, SEG_LEN, lanes, tabs)


def test_set_records_tables_on_the_host(coder, data):
    """DeviceRansDecoder.set_records with device="cpu": records of one lane are their own sub-streams (offsets 0, 2, 5
    and counts 2, 3, 5 for 8, 12 and 20 bytes, the words concatenated), a record with lanes points past its header,
    and a bad header is reported in the caller's words"""
    rng = np.random.default_rng(5)
    strings = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (8, 12, 20)]
    dec = coder.DeviceRansDecoder()
    dec.set_records(strings, 1, "cpu")
    assert dec._woff.dtype == torch.int64 and dec._woff.tolist() == [0, 2, 5]
    assert dec._wlen.dtype == torch.int32 and dec._wlen.tolist() == [2, 3, 5]
    assert dec._words.dtype == torch.int32 and dec._words.numpy().tobytes() == b"".join(strings)
    assert dec._total == 10 and dec._state.numel() == dec._pos.numel() == dec._status.numel() == 3

    sym, idx, tabs = data
    rec = coder.encode_record(sym, idx, NSEG, SEG_LEN, 4, tabs)
    o4, c4 = coder.parse_record(rec, 4)
    assert o4[0] == 5
    dec.set_records([strings[1], rec], [1, 4], "cpu")
    assert dec._woff.tolist() == [0] + (3 + o4).tolist() and dec._woff[1] == 3 + 5  # past the 5-word header
    assert dec._wlen.tolist() == [3] + c4.tolist()
    assert dec._words.numpy().tobytes() == strings[1] + rec
    assert dec._state.numel() == dec._pos.numel() == 5 and dec._status.numel() == 2

    names = ["y stream of image 0", "z stream of image 0"]
    w = np.frombuffer(rec, dtype="<u4").copy()
    w[0] = 2
    with pytest.raises(ValueError, match="^z stream of image 0: record header says 2 lanes, 4 expected"):
        dec.set_records([strings[1], w.tobytes()], [1, 4], "cpu", what=names)
    with pytest.raises(ValueError, match="^record 1: record header says 2 lanes, 4 expected"):
        dec.set_records([strings[1], w.tobytes()], [1, 4], "cpu")
    with pytest.raises(ValueError, match="^y stream of image 0: a stream is at least 8 bytes"):
        dec.set_records([strings[0][:4], rec], [1, 4], "cpu", what=names)
    with pytest.raises(ValueError, match="set_records\\(\\) first"):
        coder.DeviceRansDecoder().decode_records(0, 1, None, (0, 0), None, (0, 0), 0, 1, 1, None)


def enc_call(ops, lanes=4, nstreams=2, cap=16, slabs=None, nwords=None, status=None):
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731  (host tensors: validation comes first)
    tabs = (i32(8).view(2, 4), i32(2), i32(2))
    ops.rans_encode_lanes(i32(16), (0, 8), i32(16), (0, 8), nstreams, 1, 8, tabs,
                          i32(nstreams * 4 * cap) if slabs is None else slabs, cap,
                          i32(nstreams * 4) if nwords is None else nwords, i32(nstreams) if status is None else status,
                          lanes)


def dec_call(ops, lanes=4, nstreams=2, **kw):
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)  # noqa: E731
    nsub = nstreams * 4
    a = dict(words=i32(64), total_words=64, word_offsets=i64(nsub), word_counts=i32(nsub), state=i64(nsub),
             pos=i32(nsub), status=i32(nstreams))
    a.update(kw)
    tabs = (i32(8).view(2, 4), i32(2), i32(2))
    ops.rans_decode_lanes(a["words"], a["total_words"], a["word_offsets"], a["word_counts"], i32(16), (0, 8), i32(16),
                          (0, 8), nstreams, 0, 1, 8, tabs, a["state"], a["pos"], a["status"], True, lanes)


@pytest.mark.parametrize("lanes", [0, 3, 128])
def test_ops_reject_bad_lanes(tmae, lanes):
    from textmae_amd import ops

    with pytest.raises(ValueError, match="rans_encode_lanes: lanes = .+ power of two in 1..64"):
        enc_call(ops, lanes=lanes)
    with pytest.raises(ValueError, match="rans_decode_lanes: lanes = .+ power of two in 1..64"):
        dec_call(ops, lanes=lanes)


def test_ops_reject_mismatched_buffers(tmae):
    from textmae_amd import ops

    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    with pytest.raises(ValueError, match="nwords holds 7 elements, 8 needed"):
        enc_call(ops, nwords=i32(7))
    with pytest.raises(ValueError, match="slabs holds 127 elements, 128 needed"):
        enc_call(ops, slabs=i32(127))
    with pytest.raises(ValueError, match="status holds 1 elements, 2 needed"):
        enc_call(ops, status=i32(1))
    with pytest.raises(ValueError, match="nwords must be torch.int32"):
        enc_call(ops, nwords=torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match="word_offsets holds 7 elements, 8 needed"):
        dec_call(ops, word_offsets=torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ValueError, match="word_offsets must be torch.int64"):
        dec_call(ops, word_offsets=i32(8))
    with pytest.raises(ValueError, match="word_counts holds 2 elements, 8 needed"):
        dec_call(ops, word_counts=i32(2))  # per stream, not per sub-stream
    with pytest.raises(ValueError, match="state holds 2 elements, 8 needed"):
        dec_call(ops, state=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="pos holds 2 elements, 8 needed"):
        dec_call(ops, pos=i32(2))
    with pytest.raises(ValueError, match="words holds 64 elements, 65 needed"):
        dec_call(ops, total_words=65)
    # well-formed host tensors get as far as the device check, never to a launch
    with pytest.raises(ValueError, match="must be a device"):
        enc_call(ops)
    with pytest.raises(ValueError, match="must be a device"):
        dec_call(ops)


@pytest.mark.parametrize("entry,nargs,lanes_at", [("tmae_rans_encode_lanes", 20, 18), ("tmae_rans_decode_lanes", 25, 23)])
def test_c_entry_rejects_bad_lanes(tmae, entry, nargs, lanes_at):
    """the C entry validates lanes itself, before any launch (addresses are never dereferenced)"""
    from textmae_amd import _lib

    D = 0x1000
    if entry == "tmae_rans_encode_lanes":
        base = [D, 0, 8, D, 0, 8, 2, 1, 8, D, 4, D, D, 2, D, 16, D, D, 4, None]
    else:
        base = [D, 8, D, D, D, 0, 8, D, 0, 8, 2, 0, 1, 8, D, 4, D, D, 2, D, D, D, 1, 4, None]
    assert len(base) == nargs
    for lanes in (0, 3, 128, -2):
        args = list(base)
        args[lanes_at] = lanes
        with pytest.raises(ValueError, match=f"{entry}: lanes = "):
            _lib.call(entry, *args)
    args = list(base)
    args[0] = None
    with pytest.raises(ValueError, match=f"{entry}: NULL buffer"):
        _lib.call(entry, *args)
