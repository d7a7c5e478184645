"""compressai's entropy-coder classes (``compressai.ans``) over the C ABI (csrc/rans.cpp).

Same names and call signatures as the objects the reference uses: ``BufferedRansEncoder``
(MCM.py:845, 882-887, 890), ``RansDecoder`` (MCM.py:917-918, 941-943), ``RansEncoder`` (used by
EntropyModel.compress) and ``pmf_to_quantized_cdf`` (EntropyModel._pmf_to_cdf).  Arguments may be
Python lists (the reference passes ``.tolist()`` results), numpy arrays or CPU tensors; symbol
arrays are handed to the coder without per-element Python work.

``DeviceRansEncoder`` / ``DeviceRansDecoder`` code the same format on the GPU (csrc/rans_device.hip), many
independent streams at once from and to device tensors: the coder of ``MCM.compress_batch`` / ``decompress_batch``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

__all__ = ["BufferedRansEncoder", "RansEncoder", "RansDecoder", "pmf_to_quantized_cdf", "DeviceRansEncoder",
           "DeviceRansDecoder"]


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


# ------------------------------------------------------------------ per-image streams coded on the device
# (csrc/rans_device.hip): the same format as the classes above, one independent stream per image, one wave each.
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
    """Device symbols and indexes plus a layout in, one rANS string per stream out.  Stream b is what
    RansEncoder.encode_with_indexes returns for stream b's symbols in coding order."""

    def __init__(self):
        self._bufs = {}

    def _buffers(self, device, nstreams, cap):
        key = (device, nstreams, cap)
        bufs = self._bufs.get(key)
        if bufs is None:
            slabs = torch.empty((nstreams, cap), dtype=torch.int32, device=device)
            dense = torch.empty(nstreams * cap, dtype=torch.int32, device=device)
            # one small D2H: int64 word offsets [nstreams + 1] | int32 nwords [nstreams] | int32 status [nstreams]
            meta = torch.empty(4 * nstreams + 2, dtype=torch.int32, device=device)
            bufs = self._bufs[key] = (slabs, dense, meta)
        return bufs

    def encode_streams(self, symbols, sym_strides, indexes, idx_strides, nstreams, nseg, seg_len, tables,
                       what="stream") -> list:
        """stream b codes segments j = 0..nseg-1, each seg_len int32 at base + j * strides[0] + b * strides[1]
        (elements); tables = EntropyModel.device_tables().  Synchronises: the strings are host bytes."""
        from . import ops

        cap = ops.rans_stream_cap_words(nseg * seg_len)
        slabs, dense, meta = self._buffers(symbols.device, nstreams, cap)
        offs = meta[:2 * nstreams + 2].view(torch.int64)
        nwords, status = meta[2 * nstreams + 2:3 * nstreams + 2], meta[3 * nstreams + 2:]
        ops.rans_encode_streams(symbols, sym_strides, indexes, idx_strides, nstreams, nseg, seg_len, tables, slabs, cap,
                                nwords, status)
        ops.rans_pack_streams(slabs, cap, nwords, nstreams, dense, dense.numel(), offs, status)
        meta_h = meta.cpu().numpy()
        offs_h = meta_h[:2 * nstreams + 2].view(np.int64)
        nw_h, st_h = meta_h[2 * nstreams + 2:3 * nstreams + 2], meta_h[3 * nstreams + 2:]
        _raise_status(st_h, what)
        raw = dense[:int(offs_h[nstreams])].cpu().numpy().tobytes()  # payload-sized copy
        return [raw[4 * int(offs_h[b]):4 * (int(offs_h[b]) + int(nw_h[b]))] for b in range(nstreams)]


class DeviceRansDecoder:
    """set_streams uploads every string with ONE H2D copy; decode_streams then maps device indexes to device
    symbols, any number of times per stream (each call carries on where the last one stopped), without touching
    the host; check() reads the status words (the only synchronisation)."""

    def __init__(self):
        self._n = 0

    def set_streams(self, strings, device):
        n = len(strings)
        if n == 0:
            raise ValueError("DeviceRansDecoder: no streams")
        lens = np.empty(n, dtype=np.int32)
        for i, s in enumerate(strings):
            if len(s) < 8 or len(s) % 4:
                raise ValueError(f"stream {i}: a stream is a whole number of 32-bit words, >= 8 bytes (got {len(s)})")
            lens[i] = len(s) // 4
        offs = np.zeros(n, dtype=np.int64)
        np.cumsum(lens[:-1], out=offs[1:])
        total = int(offs[-1]) + int(lens[-1])
        hdr = (12 * n + 7) // 8 * 8
        buf = np.zeros(hdr + 4 * total, dtype=np.uint8)
        buf[:8 * n] = offs.view(np.uint8)
        buf[8 * n:12 * n] = lens.view(np.uint8)
        buf[hdr:] = np.frombuffer(b"".join(bytes(s) for s in strings), dtype=np.uint8)
        dev = torch.from_numpy(buf).to(device)  # the one upload
        self._woff = dev[:8 * n].view(torch.int64)
        self._wlen = dev[8 * n:12 * n].view(torch.int32)
        self._words = dev[hdr:].view(torch.int32)
        self._total = total
        self._state = torch.zeros(n, dtype=torch.int64, device=device)
        self._pos = torch.zeros(n, dtype=torch.int32, device=device)
        self._status = torch.zeros(n, dtype=torch.int32, device=device)
        self._started = np.zeros(n, dtype=bool)
        self._n = n

    def decode_streams(self, first_stream, nstreams, indexes, idx_strides, symbols, sym_strides, seg0, nseg, seg_len,
                       tables):
        """the next nseg segments of streams [first_stream, first_stream + nstreams): segment seg0 + j of stream b
        is seg_len int32 at base + (seg0 + j) * strides[0] + b * strides[1]; symbols are written, indexes read"""
        from . import ops

        s0, s1 = int(first_stream), int(first_stream) + int(nstreams)
        if self._n == 0:
            raise ValueError("DeviceRansDecoder: set_streams() first")
        if not (0 <= s0 < s1 <= self._n):
            raise ValueError(f"streams [{s0}, {s1}) outside the {self._n} set")
        started = self._started[s0:s1]
        if started.any() != started.all():
            raise ValueError("DeviceRansDecoder: streams of one call must have been decoded equally far")
        ops.rans_decode_streams(self._words, self._total, self._woff[s0:s1], self._wlen[s0:s1], indexes, idx_strides,
                                symbols, sym_strides, s1 - s0, seg0, nseg, seg_len, tables, self._state[s0:s1],
                                self._pos[s0:s1], self._status[s0:s1], not started.any())
        self._started[s0:s1] = True

    def status(self) -> np.ndarray:
        """per-stream status words (synchronises)"""
        return self._status.cpu().numpy()
