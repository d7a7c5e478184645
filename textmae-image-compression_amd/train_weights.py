"""The training executors' weight cache: kernel-layout copies of the f32 parameters (mcm_train.TrainExec,
mae_train.MAETrainExec)."""
from __future__ import annotations

import torch

from . import _lib, ops
from . import train_ops as T
from .optim import device_table, table_usable


def _frag_elems(cin, cout):
    """elements of a [cout][cin][3][3] weight in tmae_lic_stack's fragment order (ops.pack_lic_stack_weight)"""
    return 9 * (-(-cin // 32)) * (-(-cout // 16)) * 512


class _Weights:
    """Kernel-layout copies of the f32 parameters, rebuilt when a parameter's version changes (once per
    optimizer step).  The first build of each (parameter, layout) is lazy; afterwards ``refresh()`` re-lays
    out every stale copy in ONE multi-tensor launch (tmae_relayout_multi): plain casts as vectors, 2-D
    transposes (W^T, the conv data-gradient layout) as 64 x 64 LDS tiles, conv weights [Cout][Cin][3][3] ->
    [Cout][3][3][Cin] one row per block through LDS."""

    def __init__(self, dtype):
        self.dtype = dtype
        self.cache = {}   # (id(p), kind) -> [sig, tensor, p, job]; job = (dims, strides) or None (a view)
        self.packs = {}   # (param ids, kind) -> packed buffer whose rows are those params' cache entries
        self.owner = {}   # (id(p), kind) -> key of the one pack that cache entry is a row of
        self._tab = None
        self.builds = 0   # copies built or re-laid out outside refresh(), on the stream current at the time

    def _get(self, p, kind, make):
        key = (id(p), kind)
        sig = (p.data_ptr(), p._version)
        hit = self.cache.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        w = p.detach()
        self.builds += 1
        if hit is not None and hit[3] is not None and hit[0] is not None and hit[0][0] == sig[0]:
            dst, job = hit[1], hit[3]  # same parameter storage, newer values: re-lay out in place (keeps packing)
        elif hit is not None and hit[0] is None:
            dst, job = hit[1], hit[3]  # a packed row registered by packed(), first build
        else:
            dst, job = make(w)
        if job is not None:
            if job[0] == "lic":  # first build of a fragment-order pack (later ones: relayout_multi mode 3)
                _, co, ci, lo, n = job
                dst.copy_(ops.pack_lic_stack_weight(w[:, lo:lo + n], self.dtype))
            elif job[0] == "licT":  # the transposed, tap-flipped pack (relayout mode 4)
                dst.copy_(ops.pack_lic_stack_weight_t(w, self.dtype))
            else:
                T.relayout(w, dst, *job)
        self.cache[key] = [sig, dst, p, job]
        return dst

    def _row(self, p, kind):
        """(shape, dtype, job) of parameter p's row in a `kind` pack"""
        dt = self.dtype
        if kind == "bias":
            return (p.numel(),), torch.float32, ((p.numel(),), (1,))
        co, ci = p.shape[:2]
        if kind == "conv":
            return (co, 9 * ci), dt, ((co, 3, 3, ci), (ci * 9, 3, 1, 9))
        if kind == "conv_dg":  # the transposed-conv data-gradient layout of conv_dg()
            return (ci, 9 * co), dt, ((ci * 9, 1, 1, co), (1, 0, 0, ci * 9))
        if kind == "licT":  # the transposed conv's weight in fragment order (the fused stack backward)
            return (_frag_elems(co, ci),), dt, ("licT", co, ci)
        if isinstance(kind, tuple) and kind[0] == "lic":  # ("lic", lo, n): input channels [lo, lo + n), fragment order
            return (_frag_elems(kind[2], co),), dt, ("lic", co, ci, kind[1], kind[2])
        if isinstance(kind, tuple) and kind[0] == "conv_lat":  # ("conv_lat", n): input channels [0, n), conv layout
            return (co, 9 * kind[1]), dt, ((co, 3, 3, kind[1]), (ci * 9, 3, 1, 9))
        raise ValueError(f"unknown pack kind {kind!r}")

    def packed(self, params, kind):
        """one buffer holding the `kind` layouts of `params` back to back, so a batched launch reaches problem j at a
        constant stride (a shape product); each row is also that parameter's cache entry.  A row belongs to ONE pack:
        refresh() re-lays out cache entries, so a parameter packed in two groupings would leave the older one stale."""
        key = (tuple(id(p) for p in params), kind)
        buf = self.packs.get(key)
        if buf is None:
            for p in params:
                other = self.owner.get((id(p), kind))
                if other is not None:
                    raise RuntimeError(f"weight pack {kind!r}: parameter {id(p):#x} of grouping {key[0]} is already "
                                       f"a row of grouping {other[0]}")
            shape, dtype, _ = self._row(params[0], kind)
            buf = torch.empty((len(params), *shape), dtype=dtype, device=params[0].device)
            for j, p in enumerate(params):  # (an unpacked single entry of p is adopted: later lookups get the row)
                self.cache[(id(p), kind)] = [None, buf[j], p, self._row(p, kind)[2]]
                self.owner[(id(p), kind)] = key
            self.packs[key] = buf
        for p in params:
            self._get(p, kind, None)
        return buf

    @staticmethod
    def _is_transpose(dims, strides):
        d = list(dims) + [1] * (4 - len(dims))
        st = list(strides) + [0] * (4 - len(strides))
        return d[1] == 1 and d[2] == 1 and st[0] == 1 and st[3] >= d[0]

    def refresh(self):
        """re-lay out every cached copy whose parameter moved since it was built"""
        stale = [e for e in self.cache.values() if e[0] != (e[2].data_ptr(), e[2]._version)]
        if not stale:
            return
        rows, chunk, ptrs = [], 0, []
        # a parameter whose plain cast and transpose are both stale: the transpose row writes the cast too (mode 1
        # with a second destination), so the f32 weight is read once
        casts = {id(e[2]): e for e in stale if e[3] is not None and e[3][0] != "lic" and e[3][0] != "licT"
                 and tuple(e[3][0]) == (e[2].numel(),) and tuple(e[3][1]) == (1,)}
        fused = {}
        for e in stale:
            job = e[3]
            if job is None or job[0] in ("lic", "licT") or id(e[2]) not in casts:
                continue
            d = list(job[0]) + [1] * (4 - len(job[0]))
            st = list(job[1]) + [0] * (4 - len(job[1]))
            # the transpose of the parameter's own contiguous [R][C] storage
            if self._is_transpose(job[0], job[1]) and st[3] * d[3] == e[2].numel() and st[3] == d[0]:
                fused[id(e[2])] = (e, casts[id(e[2])])
        skip = {id(c) for _, c in fused.values()}
        for e in stale:
            sig, dst, p, job = e
            e[0] = (p.data_ptr(), p._version)
            if job is None or id(e) in skip:
                continue
            if job[0] == "licT":  # the transposed fragment order (relayout mode 4)
                _, co, ci = job
                total = _frag_elems(co, ci)
                rows.append([p.data_ptr(), dst.data_ptr(), ops.dtype_code(dst.dtype) | (4 << 8), co, ci, 0, 0, 0, 0, 0,
                             total, chunk])
                ptrs.append((p.data_ptr(), dst.data_ptr()))
                chunk += -(-(total // 72) // 256)  # 256 units of 9 taps x 8 elements per chunk
                continue
            if job[0] == "lic":  # tmae_lic_stack fragment order (relayout mode 3)
                _, co, ci, lo, n = job
                total = _frag_elems(n, co)
                rows.append([p.data_ptr(), dst.data_ptr(), ops.dtype_code(dst.dtype) | (3 << 8), co, ci, lo, n, 0, 0, 0,
                             total, chunk])
                ptrs.append((p.data_ptr(), dst.data_ptr()))
                chunk += -(-(total // 72) // 256)
                continue
            dims, strides = job
            d = list(dims) + [1] * (4 - len(dims))
            st = list(strides) + [0] * (4 - len(strides))
            total = d[0] * d[1] * d[2] * d[3]
            if total >= 1 << 31:
                raise ValueError(f"weight relayout of {total} elements exceeds the 32-bit index range")
            if self._is_transpose(dims, strides):  # dst [C][R] of src [R][C] (C = d0, R = d3, ld = s3)
                mode, n = 1, -(-d[3] // 64) * -(-d[0] // 64)
                st[1] = 0  # mode 1 reads s1 as the second destination (none unless fused below)
                f = fused.get(id(p))
                if f is not None and f[0] is e:  # + the plain cast into the "nt" copy (s1 = its address)
                    if f[1][1].dtype != dst.dtype:
                        raise ValueError("relayout: a fused cast copy must have the transpose's dtype")
                    st[1] = f[1][1].data_ptr()
                    ptrs.append((p.data_ptr(), st[1]))
            elif (d[1] * d[2] * d[3] <= 8192 and st[2] == 1 and st[1] == d[2] and st[3] == d[1] * d[2]
                  and st[0] == d[1] * d[2] * d[3]):  # per-row [A][B] -> [B][A]
                mode, n = 2, d[0]
            else:
                mode, n = 0, (total + 32767) // 32768
            rows.append([p.data_ptr(), dst.data_ptr(), ops.dtype_code(dst.dtype) | (mode << 8), d[1], d[2], d[3], *st,
                         total, chunk])
            ptrs.append((p.data_ptr(), dst.data_ptr()))
            chunk += n
        if not rows:
            return
        key = tuple(ptrs)
        if self._tab is None or self._tab[0] != key or not table_usable(self._tab[3]):
            dev = stale[0][1].device
            owner = [t for t in range(len(rows)) for _ in range(rows[t + 1][11] - rows[t][11] if t + 1 < len(rows)
                                                                else chunk - rows[t][11])]
            flat = [v for r in rows for v in r] + owner  # the rows, then each chunk's row (tmae.h)
            tab, epoch = device_table(flat, dev)
            self._tab = (key, tab, chunk, epoch)
        _lib.call("tmae_relayout_multi", self._tab[1].data_ptr(), len(rows), self._tab[2],
                  torch.cuda.current_stream().cuda_stream)

    def _cast_same(self, w2):
        if self.dtype == torch.float32:
            return w2.contiguous(), None
        return torch.empty(w2.shape, dtype=self.dtype, device=w2.device), ((w2.numel(),), (1,))

    def nt(self, p, rows=None):
        """nn.Linear / 1x1 conv weight as [N][K] in the operand dtype"""
        return self._get(p, "nt", lambda w: self._cast_same(w.reshape(w.shape[0], -1) if rows is None
                                                            else w.reshape(rows, -1)))

    def t(self, p, rows=None):
        """transposed [K][N] (the data-gradient operand of y = x W^T)"""
        def b(w):
            w2 = w.reshape(w.shape[0], -1) if rows is None else w.reshape(rows, -1)
            N, K = w2.shape
            return torch.empty((K, N), dtype=self.dtype, device=w.device), ((K, 1, 1, N), (1, 0, 0, K))
        return self._get(p, "t", b)

    def raw(self, p):
        """the weight as stored ([cin][cout] for ConvTranspose2d 1x1), cast"""
        return self._get(p, "raw", lambda w: self._cast_same(w.reshape(w.shape[0], -1)))

    def _single(self, p, kind):
        """a pack row's layout on its own (or the row, once a pack holds this parameter)"""
        def b(w):
            shape, dtype, job = self._row(w, kind)
            return torch.empty(shape, dtype=dtype, device=w.device), job
        return self._get(p, kind, b)

    def conv(self, p):
        """Conv2d 3x3 weight [Cout][Cin][3][3] -> [Cout][3][3][Cin] (forward implicit GEMM)"""
        return self._single(p, "conv")

    def conv_dg(self, p):
        """-> [Cin][3][3][Cout] (transposed-conv data gradient): dst[ci][tap][co] = w[co][ci][tap], the transpose of w
        seen as [Cout][Cin * 9]"""
        return self._single(p, "conv_dg")
