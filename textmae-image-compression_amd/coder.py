"""compressai's entropy-coder classes (``compressai.ans``) over the C ABI (csrc/rans.cpp).

Same names and call signatures as the objects the reference uses: ``BufferedRansEncoder``
(MCM.py:845, 882-887, 890), ``RansDecoder`` (MCM.py:917-918, 941-943), ``RansEncoder`` (used by
EntropyModel.compress) and ``pmf_to_quantized_cdf`` (EntropyModel._pmf_to_cdf).  Arguments may be
Python lists (the reference passes ``.tolist()`` results), numpy arrays or CPU tensors; symbol
arrays are handed to the coder without per-element Python work.

``encode_record`` / ``decode_record`` / ``parse_record`` are the host side of the lane-interleaved records
(``compress_batch(lanes=L)``): a record is ``lanes`` ordinary streams behind a small header, each stream what
``RansEncoder`` writes for that lane's share of the symbols; one lane is the plain stream without a header.

``DeviceRansEncoder.encode_records`` / ``DeviceRansDecoder.set_records`` + ``decode_records`` code those records on
the GPU (csrc/rans_device.hip), many at once from and to device tensors: the coder of ``MCM.compress_batch`` /
``decompress_batch``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

__all__ = ["BufferedRansEncoder", "RansEncoder", "RansDecoder", "pmf_to_quantized_cdf", "DeviceRansEncoder",
           "DeviceRansDecoder", "lane_split", "encode_record", "decode_record", "parse_record", "rate_table",
           "symbol_bits", "table_bits"]


def _i32(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.int32))


def _tables(cdfs, cdf_sizes, offsets):
    if isinstance(cdfs, (list, tuple)) and cdfs and isinstance(cdfs[0], (list, tuple)):
        width = max(len(r) for r in cdfs)
        t = np.zeros((len(cdfs), width), dtype=np.int32)
        for i, r in enumerate(cdfs):
            t[i, :len(r)] = r
    else:
        t = _i32(cdfs)
    if t.ndim != 2:
        raise ValueError("cdfs must be a 2-D table [num_cdfs][cdf_length]")
    sizes, offs = _i32(cdf_sizes).reshape(-1), _i32(offsets).reshape(-1)
    if sizes.size != t.shape[0] or offs.size != t.shape[0]:
        raise ValueError(f"{t.shape[0]} cdfs but {sizes.size} sizes and {offs.size} offsets")
    return t, sizes, offs


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def pmf_to_quantized_cdf(pmf, precision: int = 16):
    p = np.ascontiguousarray(np.asarray(pmf.detach().cpu() if isinstance(pmf, torch.Tensor) else pmf,
                                        dtype=np.float32).reshape(-1))
    out = np.empty(p.size + 1, dtype=np.int32)
    _lib.call("tmae_pmf_to_quantized_cdf", _ptr(p), p.size, int(precision), _ptr(out))
    return out.tolist()


class BufferedRansEncoder:
    def __init__(self):
        h = ctypes.c_void_p()
        _lib.call("tmae_rans_encoder_create", ctypes.byref(h))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib._lib is not None:
            _lib._lib.tmae_rans_encoder_destroy(h)
            self._h = None

    def encode_with_indexes(self, symbols, indexes, cdfs, cdf_sizes, offsets):
        sym, idx = _i32(symbols).reshape(-1), _i32(indexes).reshape(-1)
        if sym.size != idx.size:
            raise ValueError(f"{sym.size} symbols but {idx.size} indexes")
        t, sizes, offs = _tables(cdfs, cdf_sizes, offsets)
        _lib.call("tmae_rans_encode_with_indexes", self._h, _ptr(sym), _ptr(idx), sym.size, _ptr(t), t.shape[1],
                  _ptr(sizes), _ptr(offs), t.shape[0])

    def flush(self) -> bytes:
        n = ctypes.c_longlong()
        _lib.call("tmae_rans_encoder_flush", self._h, ctypes.byref(n))
        buf = (ctypes.c_uint8 * n.value)()
        _lib.call("tmae_rans_encoder_take", self._h, buf, n.value)
        return bytes(buf)


class RansEncoder:
    """one-shot encoder (compressai RansEncoder.encode_with_indexes -> bytes)"""

    def encode_with_indexes(self, symbols, indexes, cdfs, cdf_sizes, offsets) -> bytes:
        enc = BufferedRansEncoder()
        enc.encode_with_indexes(symbols, indexes, cdfs, cdf_sizes, offsets)
        return enc.flush()


class RansDecoder:
    def __init__(self):
        self._h = None

    def _close(self):
        if self._h is not None and self._h.value and _lib._lib is not None:
            _lib._lib.tmae_rans_decoder_destroy(self._h)
        self._h = None

    def __del__(self):
        self._close()

    def set_stream(self, stream: bytes):
        self._close()
        data = bytes(stream)
        h = ctypes.c_void_p()
        _lib.call("tmae_rans_decoder_create", data, len(data), ctypes.byref(h))
        self._h = h

    def decode_stream_array(self, indexes, cdfs, cdf_sizes, offsets) -> np.ndarray:
        if self._h is None:
            raise ValueError("RansDecoder: set_stream() first")
        idx = _i32(indexes).reshape(-1)
        t, sizes, offs = _tables(cdfs, cdf_sizes, offsets)
        out = np.empty(idx.size, dtype=np.int32)
        _lib.call("tmae_rans_decode_with_indexes", self._h, _ptr(idx), idx.size, _ptr(t), t.shape[1], _ptr(sizes),
                  _ptr(offs), t.shape[0], _ptr(out))
        return out

    def decode_stream(self, indexes, cdfs, cdf_sizes, offsets):
        return self.decode_stream_array(indexes, cdfs, cdf_sizes, offsets).tolist()

    def decode_with_indexes(self, stream, indexes, cdfs, cdf_sizes, offsets):
        self.set_stream(stream)
        try:
            return self.decode_stream(indexes, cdfs, cdf_sizes, offsets)
        finally:
            self._close()


# ------------------------------------------------------------------ what a symbol costs
def rate_table(cdf, cdf_sizes, precision: int = 16) -> np.ndarray:
    """float32 [n][len - 1]: B[r][k] = float32(precision - log2(float64(cdf[r][k + 1] - cdf[r][k]))) for
    k < cdf_sizes[r] - 1 (the last of them is the row's escape symbol), 0 past the row"""
    cdf, sizes = np.asarray(cdf, dtype=np.int64), np.asarray(cdf_sizes, dtype=np.int64).reshape(-1)
    if cdf.ndim != 2 or sizes.size != cdf.shape[0] or (sizes < 2).any() or (sizes > cdf.shape[1]).any():
        raise ValueError(f"rate_table: cdf {cdf.shape} with {sizes.size} sizes: one size in 2..{cdf.shape[-1]} per row")
    freq = np.diff(cdf, axis=1)
    inside = np.arange(freq.shape[1])[None, :] < (sizes - 1)[:, None]
    if (freq[inside] <= 0).any():
        raise ValueError("rate_table: a CDF row is not strictly increasing inside its length")
    bits = float(precision) - np.log2(np.where(inside, freq, 1).astype(np.float64))
    return np.ascontiguousarray(np.where(inside, bits, 0.0).astype(np.float32))


def symbol_bits(symbols, indexes, rate, cdf_sizes, offsets) -> np.ndarray:
    """float32 per symbol: what the coder spends on symbols[i] through row indexes[i] of `rate` (rate_table), by the
    coder's clamp and escape rule: value = symbol - offset; inside [0, size - 2) it is rate[row][value], otherwise the
    escape symbol rate[row][size - 2] plus 4 (1 + ndig) bits, ndig the 4-bit digits of raw = -2 value - 1 below the
    support and 2 (value - (size - 2)) above it"""
    sym, idx = np.asarray(symbols, dtype=np.int64).reshape(-1), np.asarray(indexes, dtype=np.int64).reshape(-1)
    if sym.size != idx.size:
        raise ValueError(f"{sym.size} symbols but {idx.size} indexes")
    rate = np.asarray(rate, dtype=np.float32)
    if idx.size and (idx.min() < 0 or idx.max() >= rate.shape[0]):
        raise ValueError("symbol_bits: a CDF index outside the tables")
    maxv = np.asarray(cdf_sizes, dtype=np.int64).reshape(-1)[idx] - 2
    value = sym - np.asarray(offsets, dtype=np.int64).reshape(-1)[idx]
    esc = (value < 0) | (value >= maxv)
    raw = np.where(value < 0, -2 * value - 1, 2 * (value - maxv))
    raw = np.where(esc, raw, 0)
    ndig = np.zeros(sym.size, dtype=np.int64)
    for d in range(1, 9):
        ndig[raw >= (1 << (4 * (d - 1)))] = d
    base = rate[idx, np.where(esc, maxv, value)]
    return np.where(esc, base + (4 * (1 + ndig)).astype(np.float32), base).astype(np.float32)


def table_bits(symbols, indexes, cdf, cdf_sizes, offsets) -> float:
    """the bits the coder spends on the symbols under the tables' own frequencies (the float64 sum of symbol_bits):
    the length of their record up to the coder's flush and its 0.1 %"""
    t, sizes, offs = _tables(cdf, cdf_sizes, offsets)
    return float(symbol_bits(symbols, indexes, rate_table(t, sizes), sizes, offs).astype(np.float64).sum())


# ------------------------------------------------------------------ lane-interleaved records (host side)
# A stream's symbols ([nseg][seg_len]) are dealt round-robin over L = lanes sub-streams: sub-stream l codes, segment
# after segment, the symbols k = l (mod L) of each segment, k ascending, with their own indexes.  Record, L >= 2
# (little-endian 32-bit words): L, the L word counts (each >= 2), then the sub-streams in lane order.  L = 1 is
# the plain stream without a header.
EMPTY_STREAM = bytes([0, 0, 0, 0x80, 0, 0, 0, 0])  # the coder's flush of state 2^31: a sub-stream without symbols


def check_lanes(lanes, who="") -> int:
    if isinstance(lanes, bool) or not isinstance(lanes, (int, np.integer)) or int(lanes) not in (1, 2, 4, 8, 16, 32, 64):
        raise ValueError(f"{who}lanes = {lanes!r} must be a power of two in 1..64")
    return int(lanes)


def lane_split(a, nseg: int, seg_len: int, lanes: int) -> list:
    """the lanes subsequences of a ([nseg * seg_len] values): lane l = a.reshape(nseg, seg_len)[:, l::lanes]"""
    lanes = check_lanes(lanes)
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a).reshape(-1)
    if a.size != nseg * seg_len:
        raise ValueError(f"{a.size} values but nseg * seg_len = {nseg} * {seg_len}")
    a = a.reshape(nseg, seg_len)
    return [np.ascontiguousarray(a[:, l::lanes]).reshape(-1) for l in range(lanes)]


def _assemble_record(subs) -> bytes:
    if len(subs) == 1:
        return bytes(subs[0])
    head = np.array([len(subs)] + [len(s) // 4 for s in subs], dtype="<u4")
    return head.tobytes() + b"".join(bytes(s) for s in subs)


def encode_record(symbols, indexes, nseg: int, seg_len: int, lanes: int, tables) -> bytes:
    """the record of one stream, coded on the host (the oracle of the device coder); tables = (cdfs, sizes, offsets)"""
    subs = [RansEncoder().encode_with_indexes(s, i, *tables)
            for s, i in zip(lane_split(symbols, nseg, seg_len, lanes), lane_split(indexes, nseg, seg_len, lanes))]
    return _assemble_record(subs)


def parse_record(record, lanes: int):
    """-> (offsets, counts): int64 word offsets into the record and int32 word counts of its lanes sub-streams"""
    lanes = check_lanes(lanes)
    n = len(record)
    if n % 4:
        raise ValueError(f"a record is a whole number of 32-bit words (got {n} bytes)")
    if lanes == 1:
        if n < 8:
            raise ValueError(f"a stream is at least 8 bytes (got {n})")
        return np.zeros(1, dtype=np.int64), np.array([n // 4], dtype=np.int32)
    if n < 4 * (lanes + 1):
        raise ValueError(f"record of {n} bytes is shorter than the header of {lanes} lanes")
    head = np.frombuffer(record, dtype="<u4", count=lanes + 1).astype(np.int64)
    if head[0] != lanes:
        raise ValueError(f"record header says {int(head[0])} lanes, {lanes} expected")
    counts = head[1:]
    if (counts < 2).any():
        raise ValueError(f"sub-stream {int(np.argmax(counts < 2))} of the record has {int(counts.min())} words (< 2)")
    if lanes + 1 + int(counts.sum()) != n // 4:
        raise ValueError(f"sub-stream lengths sum to {int(counts.sum())} words, the record holds {n // 4 - lanes - 1}")
    offsets = lanes + 1 + np.concatenate([[0], np.cumsum(counts[:-1])])
    return offsets.astype(np.int64), counts.astype(np.int32)


def decode_record(record, indexes, nseg: int, seg_len: int, lanes: int, tables) -> np.ndarray:
    """the nseg * seg_len symbols of a record, decoded on the host"""
    record = bytes(record)
    offsets, counts = parse_record(record, lanes)
    out = np.empty((nseg, seg_len), dtype=np.int32)
    dec = RansDecoder()
    for l, idx in enumerate(lane_split(indexes, nseg, seg_len, lanes)):
        dec.set_stream(record[4 * int(offsets[l]):4 * (int(offsets[l]) + int(counts[l]))])
        out[:, l::lanes] = dec.decode_stream_array(idx, *tables).reshape(nseg, -1)
    dec._close()
    return out.reshape(-1)


# ------------------------------------------------------------------ records coded on the device
# (csrc/rans_device.hip): the same format as the classes above, one independent record per image.  A record of one
# lane is the plain stream and takes the wave-per-stream kernels; more lanes take the thread-per-sub-stream kernels.
STREAM_STATUS = {1: "output buffer too small", 2: "corrupt stream (symbol outside its CDF row)",
                 3: "corrupt stream (escape longer than 8 digits)", 4: "stream exhausted",
                 5: "CDF index outside the tables", 6: "stream outside the word buffer"}


def _raise_status(status, what):
    bad = np.flatnonzero(status)
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"{what} {b}: {STREAM_STATUS.get(int(status[b]), f'status {int(status[b])}')}"
                         + (f" (and {bad.size - 1} more)" if bad.size > 1 else ""))


class DeviceRansEncoder:
    """Device symbols and indexes plus a layout in, one record per stream out: record b is what encode_record
    returns for stream b's symbols in coding order (at one lane, RansEncoder.encode_with_indexes' string)."""

    def __init__(self):
        self._bufs = {}

    def _buffers(self, device, nstreams, lanes, cap):
        key = (device, nstreams, lanes, cap)
        bufs = self._bufs.get(key)
        if bufs is None:
            nsub = nstreams * lanes
            slabs = torch.empty((nsub, cap), dtype=torch.int32, device=device)
            dense = torch.empty(nsub * cap, dtype=torch.int32, device=device)
            # one small D2H: int64 word offsets [nsub + 1] | int32 nwords [nsub] | status [nstreams] | pack status
            # [nsub], the last only for lanes > 1 (at one lane pack reports into the streams' own status words)
            meta = torch.empty(3 * nsub + 2 + nstreams + (nsub if lanes > 1 else 0), dtype=torch.int32, device=device)
            bufs = self._bufs[key] = (slabs, dense, meta)
        return bufs

    def encode_records(self, symbols, sym_strides, indexes, idx_strides, nstreams, nseg, seg_len, tables, lanes=1,
                       what="stream") -> list:
        """stream b codes segments j = 0..nseg-1, each seg_len int32 at base + j * strides[0] + b * strides[1]
        (elements), dealt over `lanes` sub-streams; tables = EntropyModel.device_tables().  The sub-streams are packed
        stream-major, lane-minor, so a record's payload is one slice of the dense buffer; its header (none at one
        lane) comes from the word counts on the host.  Synchronises: the records are host bytes."""
        from . import ops

        lanes = check_lanes(lanes)
        nsub = nstreams * lanes
        cap = ops.rans_stream_cap_words(nseg * ((seg_len + lanes - 1) // lanes))
        slabs, dense, meta = self._buffers(symbols.device, nstreams, lanes, cap)
        o, s = 2 * nsub + 2, 3 * nsub + 2
        offs, nwords, status, pstatus = meta[:o].view(torch.int64), meta[o:s], meta[s:s + nstreams], meta[s + nstreams:]
        args = (symbols, sym_strides, indexes, idx_strides, nstreams, nseg, seg_len, tables, slabs, cap, nwords, status)
        if lanes == 1:
            ops.rans_encode_streams(*args)
            pstatus = status
        else:
            pstatus.zero_()
            ops.rans_encode_lanes(*args, lanes)
        ops.rans_pack_streams(slabs, cap, nwords, nsub, dense, dense.numel(), offs, pstatus)
        meta_h = meta.cpu().numpy()
        offs_h, nw_h = meta_h[:o].view(np.int64), meta_h[o:s].reshape(nstreams, lanes)
        st_h = meta_h[s:s + nstreams]
        if lanes > 1:
            st_h = np.maximum(st_h, meta_h[s + nstreams:].reshape(nstreams, lanes).max(axis=1))
        _raise_status(st_h, what)
        raw = dense[:int(offs_h[nsub])].cpu().numpy().tobytes()  # payload-sized copy
        cut = (4 * offs_h[::lanes]).tolist()  # a status-free record's sub-streams are contiguous in the dense buffer
        if lanes == 1:
            return [raw[cut[b]:cut[b + 1]] for b in range(nstreams)]
        head = np.concatenate([np.full((nstreams, 1), lanes, dtype=np.int32), nw_h], axis=1).astype("<u4")
        return [head[b].tobytes() + raw[cut[b]:cut[b + 1]] for b in range(nstreams)]


class DeviceRansDecoder:
    """set_records uploads every record with ONE H2D copy; decode_records then maps device indexes to device
    symbols, any number of times per record (each call carries on where the last one stopped), without touching
    the host; status() reads the status words, one per record (the only synchronisation)."""

    def __init__(self):
        self._n = 0

    def set_records(self, strings, lanes=1, device="cuda", what="record"):
        """lanes is one lane count for every record or one per record; what names record i in an error, as
        f"{what} {i}" or, given a sequence, as what[i].  The headers are parsed on the host, the records go up whole in
        ONE copy, and the sub-stream table points past the headers (a record of one lane is its own sub-stream)."""
        n = len(strings)
        if n == 0:
            raise ValueError("DeviceRansDecoder: no records")
        if isinstance(lanes, (int, np.integer)):
            lanes = np.full(n, check_lanes(lanes), dtype=np.int64)
        else:
            lanes = np.array([check_lanes(v) for v in lanes], dtype=np.int64)
        if lanes.size != n:
            raise ValueError(f"{n} records but {lanes.size} lane counts")
        nbytes = np.fromiter(map(len, strings), dtype=np.int64, count=n)
        base = np.zeros(n + 1, dtype=np.int64)  # first word of every record, then the total
        np.cumsum(nbytes // 4, out=base[1:])
        sub0 = np.zeros(n + 1, dtype=np.int64)  # first sub-stream of every record
        np.cumsum(lanes, out=sub0[1:])
        nsub, total = int(sub0[n]), int(base[n])
        offs, lens = np.empty(nsub, dtype=np.int64), np.empty(nsub, dtype=np.int32)
        offs[sub0[:n]], lens[sub0[:n]] = base[:n], nbytes // 4  # right as it stands for the records of one lane
        for i in np.flatnonzero((lanes > 1) | (nbytes < 8) | (nbytes % 4 != 0)):  # the others have a header to parse
            try:
                o, c = parse_record(strings[i], int(lanes[i]))
            except ValueError as e:
                name = f"{what} {i}" if isinstance(what, str) else what[i]
                raise ValueError(f"{name}: {e}") from None
            offs[sub0[i]:sub0[i + 1]], lens[sub0[i]:sub0[i + 1]] = o + base[i], c
        hdr = (12 * nsub + 7) // 8 * 8
        buf = np.zeros(hdr + 4 * total, dtype=np.uint8)
        buf[:8 * nsub] = offs.view(np.uint8)
        buf[8 * nsub:12 * nsub] = lens.view(np.uint8)
        buf[hdr:] = np.frombuffer(b"".join(bytes(s) for s in strings), dtype=np.uint8)
        dev = torch.from_numpy(buf).to(device)  # the one upload
        self._woff = dev[:8 * nsub].view(torch.int64)
        self._wlen = dev[8 * nsub:12 * nsub].view(torch.int32)
        self._words = dev[hdr:].view(torch.int32)
        self._total = total
        self._state = torch.zeros(nsub, dtype=torch.int64, device=device)
        self._pos = torch.zeros(nsub, dtype=torch.int32, device=device)
        self._status = torch.zeros(n, dtype=torch.int32, device=device)
        self._started = np.zeros(n, dtype=bool)
        self._lanes, self._sub0 = lanes, sub0
        self._n = n

    def decode_records(self, first_record, nrecords, indexes, idx_strides, symbols, sym_strides, seg0, nseg, seg_len,
                       tables):
        """the next nseg segments of records [first_record, first_record + nrecords), which must share one lane count:
        segment seg0 + j of record b is seg_len int32 at base + (seg0 + j) * strides[0] + b * strides[1]; symbols are
        written, indexes read"""
        from . import ops

        r0, r1 = int(first_record), int(first_record) + int(nrecords)
        if self._n == 0:
            raise ValueError("DeviceRansDecoder: set_records() first")
        if not (0 <= r0 < r1 <= self._n):
            raise ValueError(f"records [{r0}, {r1}) outside the {self._n} set")
        L = int(self._lanes[r0])
        if (self._lanes[r0:r1] != L).any():
            raise ValueError("DeviceRansDecoder: records of one call must have one lane count")
        started = self._started[r0:r1]
        if started.any() != started.all():
            raise ValueError("DeviceRansDecoder: records of one call must have been decoded equally far")
        s0, s1 = int(self._sub0[r0]), int(self._sub0[r1])
        args = (self._words, self._total, self._woff[s0:s1], self._wlen[s0:s1], indexes, idx_strides, symbols,
                sym_strides, r1 - r0, seg0, nseg, seg_len, tables, self._state[s0:s1], self._pos[s0:s1],
                self._status[r0:r1], not started.any())
        if L == 1:
            ops.rans_decode_streams(*args)
        else:
            ops.rans_decode_lanes(*args, L)
        self._started[r0:r1] = True

    def status(self, extra=None) -> np.ndarray:
        """per-record status words (synchronises); extra: a device int32 vector of further status words to bring
        down in the same copy, appended to the records'"""
        if extra is None:
            return self._status.cpu().numpy()
        return torch.cat([self._status, extra.reshape(-1)]).cpu().numpy()
