"""Training path of the MCM drop-in: MCM.forward under autograd (utils/engine.py:75-91 calls
``model(samples, total_scores)``, ``criterion(out_net, samples)``, ``loss.backward()``).

One ``torch.autograd.Function`` covers the whole model: its forward enqueues the same gfx950 kernels
as inference but keeps every activation the backward needs (GELU inputs, attention log-sum-exp,
per-slice stack activations, ...); its backward is the full reverse pass on HIP kernels (split-K
TN weight gradients, transposed-weight data gradients, LayerNorm / attention / entropy-model
backward) writing every parameter gradient into one flat f32 buffer, whose views are returned to
autograd (AccumulateGrad adopts them as ``p.grad``).  A ``GradSync`` attached to the model all-reduces
that buffer in buckets over RCCL while the backward is still running (data parallel).

Reference semantics reproduced (compressai 1.2.4 / timm 0.4.5 restated):
  * training mode: EntropyBottleneck / GaussianConditional likelihoods of x + U(-1/2, 1/2);
    z_hat, y_hat through quantize_ste (pass-through gradient, MCM.py:742-744, 776);
  * LowerBound backward (gradient passes where x >= bound or grad < 0);
  * the main loss's gradient on ``*.quantiles`` is exactly zero (d z_hat / d median = -1 + 1) and is
    returned as zeros, so clip_grad_norm_ / aux_loss.backward() see what they see in the reference.
The slice loop runs slice by slice (no batching of slices 6-11 in training).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, ops
from . import train_ops as T
from .ops import ACT_GELU, ACT_NONE
from .optim import device_table, table_usable


# side-stream weight gradients size their split-K for half the chip's CU slots (the data-gradient chain holds the
# rest): graphed step 31.49 -> 31.24 ms; a quarter made the side stream the critical path (40.2 ms)
_SIDE_SLOT_DIV = 2


def _convs(seq):
    return [l for l in seq if isinstance(l, nn.Conv2d)]


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
        self._tab = None

    def _get(self, p, kind, make):
        key = (id(p), kind)
        sig = (p.data_ptr(), p._version)
        hit = self.cache.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        w = p.detach()
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

    def packed(self, params, kind):
        """one buffer holding the `kind` layouts ("conv", "conv_dg" or "bias") of `params` back to back, so a batched
        launch reaches problem j at a constant stride; each row is also that parameter's cache entry"""
        key = (tuple(id(p) for p in params), kind)
        buf = self.packs.get(key)
        if buf is None:
            p0 = params[0]
            if kind == "conv":
                co, ci = p0.shape[:2]
                buf = torch.empty((len(params), co, 9 * ci), dtype=self.dtype, device=p0.device)
                job = ((co, 3, 3, ci), (ci * 9, 3, 1, 9))
            elif kind == "conv_dg":  # the transposed-conv data-gradient layout of conv_dg(), problems back to back
                co, ci = p0.shape[:2]
                buf = torch.empty((len(params), ci, 9 * co), dtype=self.dtype, device=p0.device)
                job = ((ci * 9, 1, 1, co), (1, 0, 0, ci * 9))
            elif isinstance(kind, tuple) and kind[0] == "lic":  # ("lic", lo, n): input channels [lo, lo + n) packed
                co = p0.shape[0]
                lo, n = kind[1], kind[2]
                total = 9 * (-(-n // 32)) * (-(-co // 16)) * 512
                buf = torch.empty((len(params), total), dtype=self.dtype, device=p0.device)
                for j, p in enumerate(params):
                    self.cache[(id(p), kind)] = [None, buf[j], p, ("lic", co, p.shape[1], lo, n)]
                self.packs[key] = buf
                for p in params:
                    self._get(p, kind, None)
                return buf
            elif kind == "licT":  # the transposed conv's weight in fragment order (the fused stack backward)
                co, ci = p0.shape[:2]
                total = 9 * (-(-co // 32)) * (-(-ci // 16)) * 512
                buf = torch.empty((len(params), total), dtype=self.dtype, device=p0.device)
                for j, p in enumerate(params):
                    self.cache[(id(p), kind)] = [None, buf[j], p, ("licT", co, ci)]
                self.packs[key] = buf
                for p in params:
                    self._get(p, kind, None)
                return buf
            elif isinstance(kind, tuple) and kind[0] == "conv_lat":  # ("conv_lat", n): input channels [0, n), conv layout
                co, n = p0.shape[0], kind[1]
                buf = torch.empty((len(params), co, 9 * n), dtype=self.dtype, device=p0.device)
                for j, p in enumerate(params):
                    ci = p.shape[1]
                    self.cache[(id(p), kind)] = [None, buf[j], p, ((co, 3, 3, n), (ci * 9, 3, 1, 9))]
                self.packs[key] = buf
                for p in params:
                    self._get(p, kind, None)
                return buf
            else:
                buf = torch.empty((len(params), p0.numel()), dtype=torch.float32, device=p0.device)
                job = ((p0.numel(),), (1,))
            for j, p in enumerate(params):
                self.cache[(id(p), kind)] = [None, buf[j], p, job]
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
                total = 9 * (-(-co // 32)) * (-(-ci // 16)) * 512
                rows.append([p.data_ptr(), dst.data_ptr(), ops.dtype_code(dst.dtype) | (4 << 8), co, ci, 0, 0, 0, 0, 0,
                             total, chunk])
                ptrs.append((p.data_ptr(), dst.data_ptr()))
                chunk += -(-(total // 72) // 256)  # 256 units of 9 taps x 8 elements per chunk
                continue
            if job[0] == "lic":  # tmae_lic_stack fragment order (relayout mode 3)
                _, co, ci, lo, n = job
                total = 9 * (-(-n // 32)) * (-(-co // 16)) * 512
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

    def conv(self, p):
        """Conv2d 3x3 weight [Cout][Cin][3][3] -> [Cout][3][3][Cin] (forward implicit GEMM)"""
        def b(w):
            co, ci = w.shape[:2]
            return torch.empty((co, 9 * ci), dtype=self.dtype, device=w.device), ((co, 3, 3, ci), (ci * 9, 3, 1, 9))
        return self._get(p, "conv", b)

    def conv_dg(self, p):
        """-> [Cin][3][3][Cout] (transposed-conv data gradient)"""
        def b(w):
            co, ci = w.shape[:2]
            # dst[ci][tap][co] = w[co][ci][tap]: the transpose of w seen as [Cout][Cin * 9]
            return torch.empty((ci, 9 * co), dtype=self.dtype, device=w.device), ((ci * 9, 1, 1, co), (1, 0, 0, ci * 9))
        return self._get(p, "conv_dg", b)


class _BlockSaved:
    __slots__ = ("x", "a1", "qkv", "att", "lse", "xmid", "a2", "hpre", "h")


class _VitTrainBase:
    """What the MCM and MAE training executors share: workspaces, the flat gradient buffer laid out in the order
    the backward finishes the parameters (DP buckets), and the timm Block forward (keeping what its backward
    needs) / backward."""

    _side = None          # side stream of the weight gradients (_wg), made by _side_begin
    # split-K of the ViT blocks' weight gradients sized for 1 / VIT_WG_SLOT_DIV of the CU slots (test / A-B hook;
    # the side stream shares the chip with the data-gradient chain)
    VIT_WG_SLOT_DIV = _SIDE_SLOT_DIV
    SIDE_SLOT_DIV = _SIDE_SLOT_DIV  # the other side-stream weight gradients' (LIC convs) split-K slot divisor
    _side_used = False
    _pending = ()
    _queued = ()
    _groups = ()

    def _layout(self):
        """parameter gradient layout: the order in which the backward finishes them (DP buckets)"""
        self.params = [p for p in self._grad_order() if p.requires_grad]
        self.offsets = {}
        off = 0
        for p in self.params:
            self.offsets[id(p)] = off
            off += p.numel()
        self.numel = off
        self._gflat = None

    # ------------------------------------------------------------------ helpers
    def _e(self, *shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.dtype, device=self.device)

    def _z(self, *shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def _cast(self, src):
        """f32 -> operand dtype (identity for the f32 path)"""
        if self.dtype == torch.float32:
            return src
        return T.relayout(src, torch.empty(src.shape, dtype=self.dtype, device=self.device), (src.numel(),), (1,))

    def grads_buffer(self, fresh):
        if fresh or self._gflat is None:
            buf = torch.empty(self.numel, dtype=torch.float32, device=self.device)
            if fresh:
                return buf
            self._gflat = buf
        return self._gflat

    def grad(self, p):
        off = self.offsets[id(p)]
        return self.gflat[off:off + p.numel()].view(p.shape)

    def _ready(self, p):
        """every gradient up to and including p's is final (DP bucket hand-off).  With weight gradients on the
        side stream the hand-off lags one call: the compute stream waits for the side stream's work up to the
        PREVIOUS hand-off point and issues that bucket's collective.
        Round 6 (profiles/r06/c2_*, c5-c7): in a captured one-rank DP step these waits are what costs the +4 ms
        over the plain graphed step (31.8-32.9 vs 27.8-28.6 ms): the side stream runs far behind the data-gradient
        chain, so the chain stalls at some hand-offs (a kernel trace: 24 HIP-queue hops of the compute chain, 3.75 ms
        of gaps at them, the largest 1.76 ms), and RCCL's one-rank reduce kernels (32 workgroups, ~110 us per 64 MB
        bucket) share the chip with the backward.  Issuing each collective from the side stream instead (it then
        waits for the compute stream's hand-off point, the compute stream never waits inside the backward), or from a
        third stream joined to both, measured 36.7-37.6 ms; a lag of 2 / 4 hand-offs 31.8 / 33.2 ms; HIP graph
        queue counts (DEBUG_HIP_FORCE_GRAPH_QUEUES 2 / 3) changed nothing."""
        if self.sync is None:
            self._wg_flush()
            return
        if self._side is not None:
            self._wg_flush(last=True)  # the event below must follow every group up to p
        upto = self.offsets[id(p)] + p.numel()
        if not self._side_used:
            self.sync.ready(upto)
            return
        ev = torch.cuda.Event()
        ev.record(self._side)
        self._pending.append((ev, upto))
        main = torch.cuda.current_stream(self.device)
        while len(self._pending) > 1:
            e, u = self._pending.pop(0)
            main.wait_event(e)
            self.sync.ready(u)

    # ------------------------------------------------------------------ side-stream weight gradients
    def _side_begin(self):
        """called at the top of a backward: a side stream for the weight gradients when on a GPU"""
        if "_side" not in self.__dict__:  # the class default is None
            self._side = torch.cuda.Stream(device=self.device) if torch.device(self.device).type == "cuda" else None
        self._side_used = False
        self._side_calls = 0  # weight gradients the side stream ran in this backward (tests)
        self._pending, self._keep, self._queued, self._groups = [], [], [], []

    TIMING_SKIP_WG = False  # diagnostics: drop every queued weight gradient (wrong gradients; timing A/B only)

    def _wg(self, a, *args, **kw):
        """T.wgrad for the side stream: a weight gradient has no consumer inside the backward, so it runs under
        the serial data-gradient chain.  Queued here and enqueued by _wg_flush behind ONE fork per group (a stack,
        a block): a captured graph pays a cross-queue dependency per fork.  `a` (this layer's output gradient, a
        fresh tensor of the chain) is kept alive until the join; every other operand is a saved activation."""
        if self.TIMING_SKIP_WG:  # timing diagnostics only (tools/train_ab.py): the step without weight gradients
            return
        if self._side is None:  # same split plan as the side stream's, so both modes sum in the same order
            kw.setdefault("slot_div", self.SIDE_SLOT_DIV)
            return T.wgrad(a, *args, **kw)
        self._queued.append((a, args, kw))

    def _wg_many(self, items, M, N, K, dt, conv=None, **kw):
        """the weight gradients of several problems of one shape (the same layer of several slices' stacks): ONE
        batched launch (tmae_wgrad_args.nb) when every operand and output sits at a constant element stride from
        the previous problem's, else one launch each.  items: dicts a (output gradient), b (layer input), out / bias
        (the parameter's gradient views), x2 (conv second input pointer or None)."""
        P = len(items)

        def ptr(v):
            return v if isinstance(v, int) else v.data_ptr()

        def stride(key, esz):
            vals = [it.get(key) for it in items]
            if vals[0] is None:
                return 0 if all(v is None for v in vals) else None
            d = {ptr(b) - ptr(a) for a, b in zip(vals, vals[1:])}
            if P == 1:
                return 0
            if len(d) != 1 or next(iter(d)) % esz:
                return None
            return next(iter(d)) // esz

        eb = items[0]["b"].element_size()
        st = [stride("a", items[0]["a"].element_size()), stride("b", eb), stride("x2", eb), stride("out", 4),
              stride("bias", 4)]
        if P > 1 and None not in st:
            # the launch reads problems 1.. through pointer strides: keep their output gradients (fresh tensors of the
            # chain, unlike the saved activations) alive until the join, as _wg_flush does for the first one's
            self._keep.extend(it["a"] for it in items[1:] if not isinstance(it["a"], int))
            it = items[0]
            cv = dict(conv, x2=it.get("x2")) if conv is not None else None
            self._wg(it["a"], it["b"], M, N, K, it["out"], dt, bias=it.get("bias"), conv=cv, batch=(P, *st), **kw)
            return
        for it in items:
            cv = dict(conv, x2=it.get("x2")) if conv is not None else None
            self._wg(it["a"], it["b"], M, N, K, it["out"], dt, bias=it.get("bias"), conv=cv, **kw)

    def _wg_flush(self, last=False):
        """close the queued group: record its fork point on the compute stream now, but enqueue the group on the
        side stream only at the NEXT flush (or the join), after the compute stream's next kernels -- in a captured
        graph the fork node's first child is then the compute chain's next kernel, which keeps the compute
        chain on its own queue (the side branch takes the cross-queue dependency instead)"""
        if self._queued:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._groups.append((ev, self._queued))
            self._queued = []
        while len(self._groups) > (0 if last else 1):
            ev, group = self._groups.pop(0)
            self._side.wait_event(ev)
            with torch.cuda.stream(self._side):
                for a, args, kw in group:
                    kw.setdefault("slot_div", self.SIDE_SLOT_DIV)
                    T.wgrad(a, *args, ws_slot=4, **kw)
                    self._keep.append(a)
                    self._side_calls += 1
            self._side_used = True

    def _side_join(self):
        """order the compute stream after every side-stream weight gradient and hand off what is left"""
        if self._side is not None:
            self._wg_flush(last=True)
        if self._side is not None and self._side_used:
            torch.cuda.current_stream(self.device).wait_stream(self._side)
            for _, u in self._pending:
                self.sync.ready(u)
        self._pending, self._keep, self._side_used = [], [], False

    def _block_fwd(self, blk, x, B, Tn, store=None):
        dt, W = self.dtype, self.w
        rows, D = x.shape
        s = _BlockSaved()
        s.x = x
        s.a1 = ops.layernorm(x, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, dt)
        s.qkv = ops.linear(s.a1, W.nt(blk.attn.qkv.weight), _bias(blk.attn.qkv.bias), dt)
        H = blk.attn.num_heads
        s.att = self._e(rows, D)
        s.lse = torch.empty((B * H * Tn,), dtype=torch.float32, device=self.device)
        T.mha_lse(s.qkv, B, Tn, H, D // H, blk.attn.scale, dt, s.att, s.lse)
        s.xmid = torch.empty_like(x)
        T.linear_residual_out(s.att, W.nt(blk.attn.proj.weight), _bias(blk.attn.proj.bias), x, s.xmid, dt)
        s.a2 = ops.layernorm(s.xmid, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps, dt)
        hid = blk.mlp.fc1.out_features
        s.h, s.hpre = self._e(rows, hid), self._e(rows, hid)
        T.linear_pre(s.a2, W.nt(blk.mlp.fc1.weight), _bias(blk.mlp.fc1.bias), dt, ACT_GELU, s.h, s.hpre)
        out = torch.empty_like(x)
        T.linear_residual_out(s.h, W.nt(blk.mlp.fc2.weight), _bias(blk.mlp.fc2.bias), s.xmid, out, dt)
        (self.enc if store is None else store).append(s)
        return out

    def _block_bwd(self, blk, s, dres, dres_op, B, Tn):
        """timm Block backward: (dres f32, dres in the operand dtype) -> the same for the block input"""
        dt, W, G = self.dtype, self.w, self.grad
        rows, D = dres.shape
        hid = blk.mlp.fc1.out_features
        H = blk.attn.num_heads
        f32 = dt == torch.float32
        # fc2 (+ GELU of fc1 in the data-gradient epilogue)
        sd = self.VIT_WG_SLOT_DIV
        self._wg(dres_op, s.h, D, hid, rows, G(blk.mlp.fc2.weight), dt, slot_div=sd)  # fc2.bias: in norm2's backward
        dh = self._e(rows, hid)
        T.dgrad_linear(dres_op, W.t(blk.mlp.fc2.weight), rows, D, hid, dt, out=dh, pre=s.hpre)
        # fc1
        self._wg(dh, s.a2, hid, D, rows, G(blk.mlp.fc1.weight), dt, bias=G(blk.mlp.fc1.bias), slot_div=sd)
        da2 = torch.empty((rows, D), dtype=torch.float32, device=self.device)
        T.dgrad_linear(dh, W.t(blk.mlp.fc1.weight), rows, hid, D, dt, out=da2)
        # norm2 + residual
        dmid = torch.empty((rows, D), dtype=torch.float32, device=self.device)
        dmid_op = dmid if f32 else self._e(rows, D)
        T.layernorm_bwd(s.xmid, blk.norm2.weight, da2, dmid, rows, D, blk.norm2.eps, G(blk.norm2.weight),
                        G(blk.norm2.bias), dres=dres, dxop=None if f32 else dmid_op, dres_colsum=G(blk.mlp.fc2.bias))
        # proj
        self._wg(dmid_op, s.att, D, D, rows, G(blk.attn.proj.weight), dt, slot_div=sd)  # proj.bias: in norm1's bwd
        datt = self._e(rows, D)
        T.dgrad_linear(dmid_op, W.t(blk.attn.proj.weight), rows, D, D, dt, out=datt)
        # attention core
        dqkv = self._e(rows, 3 * D)
        T.mha_bwd(s.qkv, s.att, datt, s.lse, dqkv, B, Tn, H, D // H, blk.attn.scale, dt)
        # qkv
        self._wg(dqkv, s.a1, 3 * D, D, rows, G(blk.attn.qkv.weight), dt,
                 bias=G(blk.attn.qkv.bias) if blk.attn.qkv.bias is not None else None, slot_div=sd)
        da1 = torch.empty((rows, D), dtype=torch.float32, device=self.device)
        T.dgrad_linear(dqkv, W.t(blk.attn.qkv.weight), rows, 3 * D, D, dt, out=da1)
        # norm1 + residual
        dx = torch.empty((rows, D), dtype=torch.float32, device=self.device)
        dx_op = dx if f32 else self._e(rows, D)
        T.layernorm_bwd(s.x, blk.norm1.weight, da1, dx, rows, D, blk.norm1.eps, G(blk.norm1.weight),
                        G(blk.norm1.bias), dres=dmid, dxop=None if f32 else dx_op, dres_colsum=G(blk.attn.proj.bias))
        return dx, dx_op


class TrainExec(_VitTrainBase):
    """Workspaces + saved activations of one training forward for (batch, dtype, device)."""

    def __init__(self, m, batch, dtype, device):
        self.m, self.batch, self.dtype, self.device = m, batch, dtype, device
        self.w = _Weights(dtype)
        K = m.num_keep_patches
        self.P = m.encoder_embed.patch_size[0]
        self.img = m.encoder_embed.img_size[0]
        self.L = m.encoder_embed.num_patches
        self.g = int(round(K ** 0.5))
        if self.g * self.g != K:
            raise ValueError(f"num_keep_patches={K} must be a perfect square (MCM.py:729-732)")
        self.hz = ((self.g + 1) // 2 + 1) // 2
        if self.hz * 4 != self.g:
            raise ValueError(f"sqrt(num_keep_patches)={self.g} must be a multiple of 4 so h_s returns to the y grid")
        self.Mp = batch * K
        self.sw = m.latent_depth // m.num_slices
        self.ms = m.num_slices // 2
        self.mid = [l.out_channels for l in _convs(m.cc_transform_mean[0])]
        # forward counters of the two ViT stages: a staged backward (_MCMEncFn / _MCMDecFn) refuses activations a later
        # forward of that stage -- or a whole forward -- replaced
        self.enc_gen = self.dec_gen = 0
        self._layout()

    def _grad_order(self):
        m = self.m
        out = [m.decoder_pred.weight, m.decoder_pred.bias, m.decoder_norm.weight, m.decoder_norm.bias]
        for blk in reversed(m.decoder_blocks):
            out += _block_params(blk)
        out += [m.decoder_embed.weight, m.decoder_embed.bias, m.mask_token]
        for l in reversed([l for l in m.g_s if isinstance(l, nn.ConvTranspose2d)]):
            out += [l.weight, l.bias]
        for i in reversed(range(m.num_slices)):
            for seq in (m.lrp_transform[i], m.cc_transform_mean[i], m.cc_transform_scale[i]):
                for c in reversed(_convs(seq)):
                    out += [c.weight, c.bias]
        for seq in (m.h_s_mean, m.h_s_scale):
            for c in reversed(_hs_convs(seq)):
                out += [c.weight, c.bias]
        eb = m.entropy_bottleneck
        out += [getattr(eb, f"_matrix{i}") for i in range(5)] + [getattr(eb, f"_bias{i}") for i in range(5)]
        out += [getattr(eb, f"_factor{i}") for i in range(4)] + [eb.quantiles]
        for c in reversed(_convs(m.h_a)):
            out += [c.weight, c.bias]
        for l in reversed([l for l in m.g_a if isinstance(l, nn.Conv2d)]):
            out += [l.weight, l.bias]
        out += [m.encoder_norm.weight, m.encoder_norm.bias]
        for blk in reversed(m.encoder_blocks):
            out += _block_params(blk)
        out += [m.encoder_embed.proj.weight, m.encoder_embed.proj.bias, m.cls_token]
        seen, uniq = set(), []
        for p in out:
            if id(p) not in seen:
                seen.add(id(p))
                uniq.append(p)
        missing = [n for n, p in m.named_parameters() if p.requires_grad and id(p) not in seen]
        if missing:
            raise RuntimeError(f"training executor does not cover parameters {missing}")
        return uniq

    # ------------------------------------------------------------------ forward
    def forward(self, imgs, scores, noise):
        m, B, g = self.m, self.batch, self.g
        M, N, hz = m.latent_depth, m.hyperprior_depth, self.hz
        imgs = self._begin(imgs)
        if noise is not None:
            self.z_noise, self.y_noise = (t.float().contiguous() for t in noise)
        elif not m.training:  # eval semantics: round(x - median) + median / round(y - mu) + mu
            self.z_noise = self.y_noise = None
        else:
            self.z_noise = torch.empty((B, N, hz, hz), device=self.device).uniform_(-0.5, 0.5)
            self.y_noise = torch.empty((B, M, g, g), device=self.device).uniform_(-0.5, 0.5)
        self.enc_out = self.enc_fwd(imgs, scores)
        self._lic_fwd(self.enc_out)
        x_hat = self.dec_fwd(self.gs_out)
        return x_hat, self.YLIK, self.ZLIK

    def _begin(self, imgs):
        """what every forward entry starts with: the image check and the weight copies' refresh"""
        m = self.m
        imgs = imgs.float().contiguous()
        if imgs.shape[1:] != (m.encoder_embed.proj.in_channels, self.img, self.img):
            raise ValueError(f"Input image size {tuple(imgs.shape[2:])} doesn't match model ({self.img})")
        self.imgs = imgs
        self.w.refresh()  # one launch for every weight copy the last optimizer step made stale
        return imgs

    def enc_fwd(self, imgs, scores, out_dtype=None):
        """forward_encoder (MCM.py:590-634) of imgs (after _begin): masking ids, kept-patch embedding, cls, blocks,
        encoder_norm without the cls rows -> [B*K, E] in out_dtype (the compute dtype by default); keeps the
        encoder's activations and the shuffle for the backward"""
        m, dt, B, W = self.m, self.dtype, self.batch, self.w
        E, K, P = m.encoder_embed_dim, m.num_keep_patches, self.P
        Te = K + 1
        self.enc_gen += 1
        shuf, rest = ops.ids_shuffle(scores, K, m.sum_lanes)
        self.shuf, self.rest = shuf, rest
        pos_e = m.encoder_pos_embed.detach()
        tok = torch.empty((B * Te, E), dtype=torch.float32, device=self.device)
        self.patches = T.patch_gather(imgs, shuf, self._e(B * K, m.encoder_embed.proj.weight[0].numel()), K, P, dt)
        ops.patch_embed(imgs, shuf, W.nt(m.encoder_embed.proj.weight), m.encoder_embed.proj.bias.detach(), pos_e, tok,
                        K, P, dt, patches=self.patches)
        ops.cls_rows(tok, m.cls_token.detach(), pos_e, B, Te, E)
        self.enc = []
        for blk in m.encoder_blocks:
            tok = self._block_fwd(blk, tok, B, Te)
        self.tok_last = tok
        return ops.layernorm(tok, m.encoder_norm.weight, m.encoder_norm.bias, m.encoder_norm.eps, out_dtype or dt,
                             rows=B * K, row_group=K, group_stride=Te, row_offset=1)

    def _lic_fwd(self, enc_out):
        """g_a, h_a, the entropy models, h_s, the slice loop and g_s (MCM.py:729-792) -> self.gs_out"""
        m, dt, B, W = self.m, self.dtype, self.batch, self.w
        g = self.g
        M, N, hz = m.latent_depth, m.hyperprior_depth, self.hz

        # ---- g_a (MCM.py:735)
        x = enc_out
        self.ga = []  # (input, pre) per GELU layer
        ga = [l for l in m.g_a if isinstance(l, nn.Conv2d)]
        for j, l in enumerate(ga):
            if j < len(ga) - 1:
                h, pre = self._e(self.Mp, l.out_channels), self._e(self.Mp, l.out_channels)
                T.linear_pre(x, W.nt(l.weight), l.bias.detach(), dt, ACT_GELU, h, pre)
                self.ga.append((x, pre))
                x = h
            else:
                self.ga.append((x, None))
                self.Y32 = torch.empty((self.Mp, M), dtype=torch.float32, device=self.device)
                if dt == torch.float32:
                    ops.linear(x, W.nt(l.weight), l.bias.detach(), dt, out=self.Y32)
                    self.YT = self.Y32
                else:
                    self.YT = self._e(self.Mp, M)
                    ops.linear(x, W.nt(l.weight), l.bias.detach(), dt, out=self.YT, out32=self.Y32)

        # ---- h_a (MCM.py:739)
        self.ha = []
        x, cin, H = self.YT, M, g
        convs = _convs(m.h_a)
        for j, c in enumerate(convs):
            last = j == len(convs) - 1
            s = c.stride[0]
            Ho = (H + 2 - 3) // s + 1
            if last:
                out, pre = torch.empty((B * Ho * Ho, c.out_channels), dtype=torch.float32, device=self.device), None
            else:
                out, pre = self._e(B * Ho * Ho, c.out_channels), self._e(B * Ho * Ho, c.out_channels)
            ops.conv3x3(x, cin, cin, B, H, H, W.conv(c.weight), c.bias.detach(), out, c.out_channels, c.out_channels,
                        dt, stride=s, act=ACT_NONE if last else ACT_GELU, pre=pre, ldp=c.out_channels,
                        y_f32=last)
            self.ha.append((x, cin, H, s, pre))
            x, cin, H = out, c.out_channels, Ho
        self.Z = x

        # ---- entropy bottleneck + z_hat (MCM.py:741-744)
        eb = m.entropy_bottleneck
        self.ZLIK = torch.empty((B, N, hz, hz), dtype=torch.float32, device=self.device)
        self.ZHAT = self._e(B * hz * hz, N)
        ops.eb_likelihood(eb, self.Z, B, N, hz * hz, noise=self.z_noise, lik=self.ZLIK, zhat=self.ZHAT,
                          table=torch.empty((N, 59), dtype=torch.float32, device=self.device))

        # ---- h_s (MCM.py:747-748): mean straight into the first M columns of LMS = [latent_means | y_hat slots]
        # h_s_scale into the first M columns of LS, rows 2M apart like LMS: the mean and scale stacks of a slice
        # then read their inputs with one layout and run as one 2-problem launch per layer (_slices_fwd)
        self.LMS = self._z(self.Mp, 2 * M, dtype=dt)
        self.LS = self._e(self.Mp, 2 * M)
        self.hs_mean = self._h_s_fwd(m.h_s_mean, self.LMS, 2 * M)
        self.hs_scale = self._h_s_fwd(m.h_s_scale, self.LS, 2 * M)

        # ---- slice loop (MCM.py:751-787)
        self._slices_fwd()

        # ---- g_s (MCM.py:790-792)
        x = self.YH
        self.gs = []
        gs = [l for l in m.g_s if isinstance(l, nn.ConvTranspose2d)]
        for j, l in enumerate(gs):
            cout = l.out_channels
            h = self._e(self.Mp, cout)
            if j < len(gs) - 1:
                pre = self._e(self.Mp, cout)
                T.linear_pre(x, W.t(l.weight), l.bias.detach(), dt, ACT_GELU, h, pre)
            else:
                pre = None
                ops.linear(x, W.t(l.weight), l.bias.detach(), dt, out=h)
            self.gs.append((x, pre))
            x = h
        self.gs_out = x

    def dec_fwd(self, x, tokens=False):
        """forward_decoder (MCM.py:636-688) of x [B*K, E] (compute dtype) under self.shuf: embed + unshuffle (+ the
        off-by-one cls), blocks, norm, then decoder_pred fused with unpatchify -> x_hat f32 [B, C, H, W], or
        (tokens) as a plain linear -> preds f32 [B*L, p*p*C] in the reference's (py, px, c) column order"""
        m, dt, B, W = self.m, self.dtype, self.batch, self.w
        K, P, shuf = m.num_keep_patches, self.P, self.shuf
        Td = self.L + 1
        self.dec_gen += 1
        self.gs_out = x
        Dd, L = m.decoder_embed_dim, self.L
        pos_d = m.decoder_pos_embed.detach()
        dec = torch.empty((B * Td, Dd), dtype=torch.float32, device=self.device)
        ops.decoder_embed(x, W.nt(m.decoder_embed.weight), m.decoder_embed.bias.detach(), pos_d, shuf, dec, B, K, L,
                          dt)
        ops.mask_rows(dec, m.mask_token.detach(), pos_d, shuf, B, L, K, Dd)
        self.dec = []
        for blk in m.decoder_blocks:
            dec = self._block_fwd(blk, dec, B, Td, store=self.dec)
        self.dec_last = dec
        self.dn = ops.layernorm(dec, m.decoder_norm.weight, m.decoder_norm.bias, m.decoder_norm.eps, dt, rows=B * L,
                                row_group=L, group_stride=Td, row_offset=1)
        if tokens:
            return ops.linear(self.dn, W.nt(m.decoder_pred.weight), m.decoder_pred.bias.detach(), dt,
                              out_dtype=torch.float32)
        x_hat = torch.empty((B, m.encoder_embed.proj.in_channels, self.img, self.img), dtype=torch.float32,
                            device=self.device)
        ops.decoder_pred(self.dn, W.nt(m.decoder_pred.weight), m.decoder_pred.bias.detach(), x_hat, B, L, P, dt)
        return x_hat

    def _h_s_fwd(self, seq, out_final, ld_final):
        dt, W, B = self.dtype, self.w, self.batch
        x, cin, H = self.ZHAT, self.m.hyperprior_depth, self.hz
        saved = []
        layers = _hs_layers(seq)
        for j, (c, pshuf) in enumerate(layers):
            last = j == len(layers) - 1
            cout = c.out_channels
            if last:
                out, pre, ldo = out_final, None, ld_final
            else:
                Ho = 2 * H if pshuf else H
                co = cout // 4 if pshuf else cout
                out, pre, ldo = self._e(B * Ho * Ho, co), self._e(B * Ho * Ho, co), co
            ops.conv3x3(x, cin, cin, B, H, H, W.conv(c.weight), c.bias.detach(), out, ldo, cout, dt,
                        act=ACT_NONE if last else ACT_GELU, pixel_shuffle=pshuf, pre=pre, ldp=ldo)
            saved.append((x, cin, H, pshuf, pre))
            if pshuf:
                H, cin = 2 * H, cout // 4
            else:
                cin = cout
            x = out
        return saved

    USE_LIC_STACK = True  # test hook: False runs the per-layer conv launches in the bf16 training forward too
    USE_LIC_LATENT = True  # False: the latent partial sums as two implicit-GEMM conv launches
    USE_LIC_STACK_BWD = True  # False: the slice stacks' data gradients as one conv launch per layer
    FUSE_FIRST_DGRAD = True   # the serial slices' first-layer input gradients inside the fused chain (routed)
    _fused_bwd = False

    def _fused_ok(self):
        m = self.m
        return (self.dtype == torch.bfloat16 and self.USE_LIC_STACK and self.sw % 8 == 0 and m.num_slices > self.ms
                and ops.lic_stack_fits(self.g, self.sw * (self.ms + 1), self.mid))

    def _slices_fwd_fused(self):
        """the slice loop on the fused stacks (lic_stack.hip), as the inference forward runs it (mcm.py _slices), with
        every layer's pre-activation and GELU output kept for the backward (tmae_lic_stack_args.sv_*):
          * the latent-channel parts of every slice's first convs (mean + lrp on latent_means, scale on latent_scales)
            as two conv launches into the partial-sum buffer P, added by each stack's layer-0 epilogue;
          * slices 0..ms-1: ONE launch each -- the mean stack's workgroups go on with the slice's lrp stack, the scale
            stack beside them; their Gaussian likelihoods in one launch after the loop;
          * slices ms..S-1 batched: one launch for their 2 x nbs mean / scale stacks, the likelihoods, one for their
            lrp stacks.
        Weights are packed in fragment order by the per-step relayout (relayout mode 3).  Returns nothing; fills
        self.sl with the records _slices_bwd reads (same shapes as _slices_fwd's)."""
        m, dt, W, B, g = self.m, self.dtype, self.w, self.batch, self.g
        M, S, sw, ms, Mp, HW = m.latent_depth, m.num_slices, self.sw, self.ms, self.Mp, g * g
        mid = self.mid
        c0, nl = mid[0], len(mid)
        esz, e4 = self.LMS.element_size(), 4
        lms = self.LMS.data_ptr()
        cm = [_convs(m.cc_transform_mean[i]) for i in range(S)]
        cs = [_convs(m.cc_transform_scale[i]) for i in range(S)]
        cl = [_convs(m.lrp_transform[i]) for i in range(S)]
        self.YPT = self._e(Mp, M)
        self.YPRE = torch.empty((Mp, M), dtype=torch.float32, device=self.device)
        self.YH = self._e(Mp, M)
        self.YLIK = torch.empty((B, M, g, g), dtype=torch.float32, device=self.device)
        # ---- latent-channel partial sums P = [mean (S c0) | lrp (S c0) | scale (S c0)] (no bias: layer 0 adds it)
        Pw = 3 * S * c0
        off_mean, off_lrp, off_scale = 0, S * c0, 2 * S * c0
        P = torch.empty((Mp, Pw), dtype=torch.float32, device=self.device)
        self._P = P
        pb = P.data_ptr()
        if self.USE_LIC_LATENT and ops.lic_latent_fits(g, M) and c0 % 32 == 0:
            # one tmae_lic_latent launch: a block per stack's latent part, [mean | lrp | scale] x slices
            w_lat = W.packed([c[0].weight for c in cm] + [c[0].weight for c in cl] + [c[0].weight for c in cs],
                             ("lic", 0, M))
            nfs = c0 // 16
            ops.lic_latent(B, g, [self.LMS, self.LMS, self.LS], 2 * M, M, w_lat, nfs, w_lat[0].numel(),
                           [0, S * nfs, 2 * S * nfs], 0, S * nfs, pb, Pw)
        else:
            w_ml = W.packed([c[0].weight for c in cm] + [c[0].weight for c in cl], ("conv_lat", M))
            w_s = W.packed([c[0].weight for c in cs], ("conv_lat", M))
            ops.conv3x3(self.LMS, M, 2 * M, B, g, g, w_ml, None, pb, Pw, S * c0, dt, y_f32=True, nb=(1, 2),
                        strides={"w": (0, S * w_ml[0].numel()), "y": (0, S * c0)})
            ops.conv3x3(self.LS, M, 2 * M, B, g, g, w_s, None, pb + off_scale * 4, Pw, S * c0, dt, y_f32=True)

        def stack_weights(convs_per_problem, lo, n0):
            """per layer: packed weights of the problems (layer 0: input channels [lo, lo + n0)) and biases"""
            ws, bs = [], []
            for l in range(nl):
                kind = ("lic", lo, n0) if l == 0 else ("lic", 0, mid[l - 1])
                ws.append(W.packed([c[l].weight for c in convs_per_problem], kind))
                bs.append(W.packed([c[l].bias for c in convs_per_problem], "bias"))
            return ws, bs

        def save_bufs(lead):
            """pre / act per non-last layer, [*lead][Mp][cout] bf16"""
            return [(self._e(*lead, Mp, c), self._e(*lead, Mp, c)) for c in mid[:-1]]

        self.sl = [None] * S
        # ---- slices 0..ms-1: chained launches
        MS = torch.empty((2, ms, Mp, sw), dtype=torch.float32, device=self.device)
        for i in range(ms):
            ny = sw * i
            ws, bs = stack_weights([cm[i], cs[i]], M, ny)
            lw, lb = stack_weights([cl[i]], M, ny + sw)
            st = {"a": (off_scale - off_mean, c0), "y": (ms * Mp * sw, 0)}
            for l in range(nl):
                st[f"w{l}"] = (ws[l][0].numel(), 0)
                st[f"b{l}"] = (bs[l][0].numel(), 0)
            sv_ms = save_bufs((2,))
            sv_l = save_bufs(())
            t = torch.empty((Mp, sw), dtype=torch.float32, device=self.device)
            ch = dict(w=[w[0] for w in lw], b=[b[0] for b in lb], couts=mid, x1=lms + M * esz, c1=ny, ld1=2 * M,
                      y=self.Y32.data_ptr() + i * sw * e4, ldy=M, add=pb + (off_lrp + i * c0) * e4, ld_add=Pw,
                      ypre=self.YPRE.data_ptr() + i * sw * e4, ld_ypre=M, out=self.YH.data_ptr() + i * sw * esz,
                      ld_out=M, out2=lms + (M + i * sw) * esz, ld_out2=2 * M)
            save = {"layers": [(pre, act, (Mp * c, 0)) for (act, pre), c in zip(sv_ms, mid)],
                    "chain": [(pre, act, 0) for act, pre in sv_l], "chain_t": t}
            ops.lic_stack(B, g, lms + M * esz, ny, 2 * M, [w[0] for w in ws], [b[0] for b in bs], mid, MS[0, i], sw,
                          True, addend=pb + (off_mean + i * c0) * e4, ld_add=Pw, nb=(2, 1), strides=st, chain=ch,
                          save=save)
            self.sl[i] = {"mean": [(a[0], p_[0]) for a, p_ in sv_ms] + [MS[0, i]],
                          "scale": [(a[1], p_[1]) for a, p_ in sv_ms] + [MS[1, i]],
                          "lrp": list(sv_l) + [t]}
        # Gaussian likelihoods + y_hat_pre (YPT, the backward's lrp input; YPRE) of the chained slices
        ops.gc_slices(self.Y32, M, 0, MS[0], MS[1], Mp * sw, sw, self.y_noise, self.YLIK, M, self.YPT, dt, M,
                      self.YPRE, M, B, HW, ms, sw)
        # ---- slices ms..S-1 batched on the support slots 0..ms-1
        i0, nbs = ms, S - ms
        bs_ = range(i0, S)
        ws, bsb = stack_weights([cm[i] for i in bs_] + [cs[i] for i in bs_], M, sw * ms)
        st = {"a": (off_scale - off_mean, c0), "y": (nbs * Mp * sw, Mp * sw)}
        for l in range(nl):
            st[f"w{l}"] = (nbs * ws[l][0].numel(), ws[l][0].numel())
            st[f"b{l}"] = (nbs * bsb[l][0].numel(), bsb[l][0].numel())
        MSB = torch.empty((2, nbs, Mp, sw), dtype=torch.float32, device=self.device)
        sv_b = save_bufs((2, nbs))
        ops.lic_stack(B, g, lms + M * esz, sw * ms, 2 * M, [w[0] for w in ws], [b[0] for b in bsb], mid, MSB, sw, True,
                      addend=pb + (off_mean + i0 * c0) * e4, ld_add=Pw, nb=(2, nbs), strides=st,
                      save={"layers": [(pre, act, (nbs * Mp * c, Mp * c)) for (act, pre), c in zip(sv_b, mid)]})
        ops.gc_slices(self.Y32, M, i0 * sw, MSB[0], MSB[1], Mp * sw, sw, self.y_noise, self.YLIK, M, self.YPT, dt, M,
                      self.YPRE, M, B, HW, nbs, sw)
        lw, lb = stack_weights([cl[i] for i in bs_], M, sw * ms + sw)
        st = {"a": (0, c0), "y": (0, sw), "src": (0, sw), "x2": (0, sw)}
        for l in range(nl):
            st[f"w{l}"] = (0, lw[l][0].numel())
            st[f"b{l}"] = (0, lb[l][0].numel())
        sv_lb = save_bufs((nbs,))
        tb = torch.empty((nbs, Mp, sw), dtype=torch.float32, device=self.device)
        ops.lic_stack(B, g, lms + M * esz, sw * ms, 2 * M, [w[0] for w in lw], [b[0] for b in lb], mid,
                      self.YH.data_ptr() + i0 * sw * esz, M, False, x2=self.YPT.data_ptr() + i0 * sw * esz, c2=sw,
                      ld2=M, addend=pb + (off_lrp + i0 * c0) * e4, ld_add=Pw,
                      lrp_src=self.YPRE.data_ptr() + i0 * sw * e4, ld_src=M, nb=(1, nbs), strides=st,
                      save={"layers": [(pre, act, (0, Mp * c)) for (act, pre), c in zip(sv_lb, mid)], "t": tb,
                            "t_s": (0, Mp * sw)})
        for j, i in enumerate(bs_):
            self.sl[i] = {"mean": [(a[0, j], p_[0, j]) for a, p_ in sv_b] + [MSB[0, j]],
                          "scale": [(a[1, j], p_[1, j]) for a, p_ in sv_b] + [MSB[1, j]],
                          "lrp": [(a[j], p_[j]) for a, p_ in sv_lb] + [tb[j]]}

    def _slices_fwd(self):
        # the fused stack backward reads what the fused forward saved (bf16 pre-activations, [problems][Mp][c])
        self._fused_bwd = self._fused_ok() and self.USE_LIC_STACK_BWD
        if self._fused_ok():
            return self._slices_fwd_fused()
        m, dt, W, B, g = self.m, self.dtype, self.w, self.batch, self.g
        M, S, sw, ms, Mp, HW = m.latent_depth, m.num_slices, self.sw, self.ms, self.Mp, self.g * self.g
        esz = self.LMS.element_size()
        lms = self.LMS.data_ptr()
        self.YPT = self._e(Mp, M)
        self.YPRE = torch.empty((Mp, M), dtype=torch.float32, device=self.device)
        self.YH = self._e(Mp, M)
        self.YLIK = torch.empty((B, M, g, g), dtype=torch.float32, device=self.device)
        self.sl = []
        # slices 0..ms-1 in order (each conditions on the ones before); slices ms..S-1 all condition on y_hat
        # slots 0..ms-1 only (max_support_slices, MCM.py:73, 756-758), so they run batched (_batched_fwd)
        nser = ms if S - ms > 1 else S
        for i in range(nser):
            k = min(i, ms)
            cin_m = M + sw * k
            rec = {}
            rec["mean"], rec["scale"] = self._ms_fwd(i, k)
            mu, sig = rec["mean"][-1], rec["scale"][-1]
            ops.gc_slices(self.Y32, M, i * sw, mu, sig, 0, sw, self.y_noise, self.YLIK, M, self.YPT, dt, M,
                          self.YPRE, M, B, HW, 1, sw)
            ypt = self.YPT.data_ptr() + i * sw * esz
            rec["lrp"] = self._stack_fwd(_convs(m.lrp_transform[i]), (self.LMS, cin_m, 2 * M, ypt, sw, M), lrp=i)
            self.sl.append(rec)
        if nser < S:
            self.sl += self._batched_fwd(nser, S - nser)

    def _batched_fwd(self, i0, nbs):
        """slices i0..i0+nbs-1 together: their mean / scale stacks as one 2 x nbs-problem launch per layer, the
        Gaussian likelihoods of all nbs slices in one launch, their lrp stacks as one nbs-problem launch per layer
        (weights / biases of each group packed so problem j sits at a constant stride).  Same arithmetic per
        slice as the serial form; returns one saved-activation record per slice"""
        m, dt, W, B, g, Mp = self.m, self.dtype, self.w, self.batch, self.g, self.Mp
        M, sw, HW = m.latent_depth, self.sw, g * g
        k = self.ms  # support slots of every batched slice
        esz = self.LMS.element_size()
        sl = range(i0, i0 + nbs)
        cm = [_convs(m.cc_transform_mean[i]) for i in sl]
        cs = [_convs(m.cc_transform_scale[i]) for i in sl]
        cl = [_convs(m.lrp_transform[i]) for i in sl]
        recs = [{"mean": [], "scale": [], "lrp": []} for _ in sl]
        x1, c1, ld1 = self.LMS, M, 2 * M
        x1s = ((self.LS.data_ptr() - self.LMS.data_ptr()) // esz, 0)
        x2, c2 = self.LMS.data_ptr() + M * esz, sw * k
        nl = len(cm[0])
        for l in range(nl):
            cout = cm[0][l].out_channels
            wm_, ws_ = W.packed([c[l].weight for c in cm], "conv"), W.packed([c[l].weight for c in cs], "conv")
            bm_, bs_ = W.packed([c[l].bias for c in cm], "bias"), W.packed([c[l].bias for c in cs], "bias")
            st = {"x1": x1s, "w": ((ws_.data_ptr() - wm_.data_ptr()) // wm_.element_size(), wm_[0].numel()),
                  "b": ((bs_.data_ptr() - bm_.data_ptr()) // 4, cout), "y": (nbs * Mp * cout, Mp * cout)}
            if l < nl - 1:
                act, pre = self._e(2, nbs, Mp, cout), self._e(2, nbs, Mp, cout)
                st["pre"] = st["y"]
                ops.conv3x3(x1, c1, ld1, B, g, g, wm_, bm_, act, cout, cout, dt, act=ACT_GELU, x2=x2, c2=c2, ld2=2 * M,
                            pre=pre, ldp=cout, nb=(2, nbs), strides=st)
                for j in range(nbs):
                    recs[j]["mean"].append((act[0, j], pre[0, j]))
                    recs[j]["scale"].append((act[1, j], pre[1, j]))
                x1, c1, ld1, x1s, x2, c2 = act, cout, cout, (nbs * Mp * cout, Mp * cout), None, 0
            else:
                out = torch.empty((2, nbs, Mp, cout), dtype=torch.float32, device=self.device)
                ops.conv3x3(x1, c1, ld1, B, g, g, wm_, bm_, out, cout, cout, dt, y_f32=True, x2=x2, c2=c2, ld2=2 * M,
                            nb=(2, nbs), strides=st)
                for j in range(nbs):
                    recs[j]["mean"].append(out[0, j])
                    recs[j]["scale"].append(out[1, j])
                mus = out
        # GaussianConditional + quantize_ste of all nbs slices (mu / sigma blocks Mp * sw apart)
        ops.gc_slices(self.Y32, M, i0 * sw, mus[0], mus[1], Mp * sw, sw, self.y_noise, self.YLIK, M, self.YPT, dt, M,
                      self.YPRE, M, B, HW, nbs, sw)
        # lrp stacks: input [latent_means | slots 0..k-1] (shared) + this slice's y_hat_pre (x2, sw apart)
        x1, c1, ld1, x1s = self.LMS, M + sw * k, 2 * M, (0, 0)
        x2, c2, ld2, x2s = self.YPT.data_ptr() + i0 * sw * esz, sw, M, (0, sw)
        for l in range(nl):
            cout = cl[0][l].out_channels
            wl_, bl_ = W.packed([c[l].weight for c in cl], "conv"), W.packed([c[l].bias for c in cl], "bias")
            st = {"x1": x1s, "x2": x2s, "w": (0, wl_[0].numel()), "b": (0, cout)}
            if l < nl - 1:
                act, pre = self._e(nbs, Mp, cout), self._e(nbs, Mp, cout)
                st["y"] = st["pre"] = (0, Mp * cout)
                ops.conv3x3(x1, c1, ld1, B, g, g, wl_, bl_, act, cout, cout, dt, act=ACT_GELU, x2=x2, c2=c2, ld2=ld2,
                            pre=pre, ldp=cout, nb=(1, nbs), strides=st)
                for j in range(nbs):
                    recs[j]["lrp"].append((act[j], pre[j]))
                x1, c1, ld1, x1s, x2, c2, ld2, x2s = act, cout, cout, (0, Mp * cout), None, 0, 0, (0, 0)
            else:
                # y_hat = y_hat_pre + 0.5 tanh(t) into YH (slice j at channels (i0 + j) sw), t kept in f32
                t = torch.empty((nbs, Mp, cout), dtype=torch.float32, device=self.device)
                st.update({"y": (0, sw), "src": (0, sw), "pre": (0, Mp * cout)})
                ops.conv3x3(x1, c1, ld1, B, g, g, wl_, bl_, self.YH.data_ptr() + i0 * sw * esz, M, cout, dt,
                            y_f32=(dt == torch.float32), lrp_src=self.YPRE.data_ptr() + i0 * sw * 4, ld_src=M,
                            pre=t, ldp=cout, nb=(1, nbs), strides=st)
                for j in range(nbs):
                    recs[j]["lrp"].append(t[j])
        return recs

    def _ms_fwd(self, i, k):
        """cc_transform_mean[i] and cc_transform_scale[i] (MCM.py:761-768) as one 2-problem conv launch per layer:
        problem 0 reads [latent_means | y_hat slots 0..k-1] from LMS, problem 1 [latent_scales | the same slots]
        (LS and LMS share the 2M row pitch; per-problem weight / bias / input offsets are pointer differences).
        Returns the saved activations of each stack as _stack_fwd does."""
        m, dt, W, B, g, Mp = self.m, self.dtype, self.w, self.batch, self.g, self.Mp
        M, sw = m.latent_depth, self.sw
        cm, cs = _convs(m.cc_transform_mean[i]), _convs(m.cc_transform_scale[i])
        esz = self.LMS.element_size()

        def diff(a, b, e):
            d = b.data_ptr() - a.data_ptr()
            assert d % e == 0
            return d // e

        sv_m, sv_s = [], []
        x1, ld1, xs = self.LMS, 2 * M, diff(self.LMS, self.LS, esz)
        c1, c2 = M, sw * k
        x2 = self.LMS.data_ptr() + M * esz if k else None
        for l, (a, b) in enumerate(zip(cm, cs)):
            cout = a.out_channels
            wa, wb = W.conv(a.weight), W.conv(b.weight)
            st = {"x1": (xs, 0), "w": (diff(wa, wb, wa.element_size()), 0),
                  "b": (diff(a.bias, b.bias, 4), 0), "y": (Mp * cout, 0)}
            if l < 4:
                act, pre = self._e(2, Mp, cout), self._e(2, Mp, cout)
                st["pre"] = (Mp * cout, 0)
                ops.conv3x3(x1, c1, ld1, B, g, g, wa, a.bias.detach(), act, cout, cout, dt, act=ACT_GELU, x2=x2, c2=c2,
                            ld2=2 * M, pre=pre, ldp=cout, nb=(2, 1), strides=st)
                sv_m.append((act[0], pre[0]))
                sv_s.append((act[1], pre[1]))
                x1, c1, ld1, xs, x2, c2 = act, cout, cout, Mp * cout, None, 0
            else:
                out = torch.empty((2, Mp, cout), dtype=torch.float32, device=self.device)
                ops.conv3x3(x1, c1, ld1, B, g, g, wa, a.bias.detach(), out, cout, cout, dt, y_f32=True, x2=x2, c2=c2,
                            ld2=2 * M, nb=(2, 1), strides=st)
                sv_m.append(out[0])
                sv_s.append(out[1])
        return sv_m, sv_s

    def _stack_fwd(self, convs, first, lrp=None):
        """5-conv stack (cc_transform / lrp_transform): returns [(act_l, pre_l) for l < 4] + [out]"""
        dt, W, B, g, Mp = self.dtype, self.w, self.batch, self.g, self.Mp
        m = self.m
        M, sw = m.latent_depth, self.sw
        x1, c1, ld1, x2, c2, ld2 = first
        saved = []
        for l, c in enumerate(convs):
            cout = c.out_channels
            if l < 4:
                act, pre = self._e(Mp, cout), self._e(Mp, cout)
                ops.conv3x3(x1, c1, ld1, B, g, g, W.conv(c.weight), c.bias.detach(), act, cout, cout, dt, act=ACT_GELU,
                            x2=x2, c2=c2, ld2=ld2, pre=pre, ldp=cout)
                saved.append((act, pre))
                x1, c1, ld1, x2, c2, ld2 = act, cout, cout, None, 0, 0
            elif lrp is None:
                out = torch.empty((Mp, cout), dtype=torch.float32, device=self.device)
                ops.conv3x3(x1, c1, ld1, B, g, g, W.conv(c.weight), c.bias.detach(), out, cout, cout, dt, y_f32=True)
                saved.append(out)
            else:
                i = lrp
                esz = self.YH.element_size()
                t = torch.empty((Mp, cout), dtype=torch.float32, device=self.device)
                ops.conv3x3(x1, c1, ld1, B, g, g, W.conv(c.weight), c.bias.detach(), self.YH.data_ptr() + i * sw * esz,
                            M, cout, dt, y_f32=(dt == torch.float32), lrp_src=self.YPRE.data_ptr() + i * sw * 4,
                            ld_src=M, y2=(self.LMS.data_ptr() + (M + i * sw) * esz) if i < self.ms else None,
                            ldy2=2 * M, pre=t, ldp=cout)
                saved.append(t)
        return saved

    # ------------------------------------------------------------------ backward
    def backward(self, dxhat, dylik, dzlik, gflat, sync=None):
        """full reverse pass; every parameter's gradient lands in gflat (views per self.offsets)"""
        m, dt, W, B = self.m, self.dtype, self.w, self.batch
        P, M, N, hz, L = self.P, m.latent_depth, m.hyperprior_depth, self.hz, self.L
        Mp = self.Mp
        self.bwd_begin(gflat, sync)
        G = self.grad
        dxhat = dxhat.float().contiguous() if dxhat is not None else torch.zeros_like(self.imgs)
        dylik = dylik.float().contiguous() if dylik is not None else None
        dzlik = dzlik.float().contiguous() if dzlik is not None else None

        # ---- unpatchify (MCM.py:797), decoder
        dP = T.patchify(dxhat, self._e(B * L, dxhat.shape[1] * P * P), P, dt)
        d = self.dec_bwd(dP)

        # ---- g_s
        gs = [l for l in m.g_s if isinstance(l, nn.ConvTranspose2d)]
        for j in reversed(range(len(gs))):
            l = gs[j]
            x, _ = self.gs[j]
            pre_prev = self.gs[j - 1][1] if j > 0 else None
            cin, cout = l.in_channels, l.out_channels
            self._wg(d, x, cout, cin, Mp, G(l.weight), dt, layout="dense_t", bias=G(l.bias))
            dx = self._e(Mp, cin)
            T.dgrad_linear(d, W.raw(l.weight), Mp, cout, cin, dt, out=dx, pre=pre_prev)
            d = dx
        dYH = d
        self._ready(gs[0].bias)

        # ---- slice loop
        DY, dLM, dLS = self._slices_bwd(dYH, dylik)

        # ---- h_s
        dZH = self._z(B * hz * hz, N)
        self._h_s_bwd(m.h_s_mean, self.hs_mean, dLM, dZH)
        self._h_s_bwd(m.h_s_scale, self.hs_scale, dLS, dZH)
        self._ready(_hs_convs(m.h_s_scale)[0].bias)

        # ---- entropy bottleneck (MCM.py:741-744)
        eb = m.entropy_bottleneck
        dZ = torch.empty((B * hz * hz, N), dtype=torch.float32, device=self.device)
        T.eb_bwd(ops._eb_params(eb), self.Z, self.z_noise, dzlik, dZH, dZ, B, N, hz * hz, self._eb_grads(eb))
        G(eb.quantiles).zero_()
        self._ready(eb.quantiles)

        # ---- h_a (MCM.py:739): dZ -> DY (accumulated with the slice loop's y gradient)
        d = self._cast(dZ)
        convs = _convs(m.h_a)
        for j in reversed(range(len(convs))):
            c = convs[j]
            x, cin, H, s, _ = self.ha[j]
            pre_prev = self.ha[j - 1][4] if j > 0 else None
            cout = c.out_channels
            Ho = (H + 2 - 3) // s + 1
            self._wg(d, x, cout, 9 * cin, B * Ho * Ho, G(c.weight), dt,
                    conv=dict(c1=cin, H=H, W=H, stride=s, cin=cin), layout="conv", bias=G(c.bias))
            if j > 0:
                dx = self._e(B * H * H, cin)
                T.conv_dgrad(d, W.conv_dg(c.weight), B, H, H, s, cout, cin, dt, out=dx, pre=pre_prev)
                d = dx
            else:
                T.conv_dgrad(d, W.conv_dg(c.weight), B, H, H, s, cout, cin, dt, routes=[(DY, M, M)])
        self._ready(convs[0].bias)

        # ---- g_a (MCM.py:735)
        d = self._cast(DY)
        ga = [l for l in m.g_a if isinstance(l, nn.Conv2d)]
        for j in reversed(range(len(ga))):
            l = ga[j]
            x, _ = self.ga[j]
            pre_prev = self.ga[j - 1][1] if j > 0 else None
            cin, cout = l.in_channels, l.out_channels
            self._wg(d, x, cout, cin, Mp, G(l.weight), dt, bias=G(l.bias))
            if j > 0:
                dx = self._e(Mp, cin)
                T.dgrad_linear(d, W.t(l.weight), Mp, cout, cin, dt, out=dx, pre=pre_prev)
            else:
                dx = torch.empty((Mp, cin), dtype=torch.float32, device=self.device)
                T.dgrad_linear(d, W.t(l.weight), Mp, cout, cin, dt, out=dx)
            d = dx
        self._ready(ga[0].bias)
        self.enc_bwd(d)
        self._side_join()

    def enc_bwd(self, denc):
        """encoder backward (MCM.py:590-634) from denc f32 [B*K, E], the gradient of encoder_norm's output without
        the cls rows: every encoder parameter's gradient"""
        m, dt, B = self.m, self.dtype, self.batch
        E, K = m.encoder_embed_dim, m.num_keep_patches
        Te = K + 1
        G = self.grad
        # ---- encoder norm (drops cls, MCM.py:631-632) + blocks
        dt_tok = self._z(B * Te, E)
        dt_op = dt_tok if dt == torch.float32 else self._z(B * Te, E, dtype=dt)
        T.layernorm_bwd(self.tok_last, m.encoder_norm.weight, denc, dt_tok, B * K, E, m.encoder_norm.eps,
                        G(m.encoder_norm.weight), G(m.encoder_norm.bias), dxop=None if dt == torch.float32 else dt_op,
                        row_group=K, group_stride=Te, row_offset=1)
        self._ready(m.encoder_norm.bias)
        for blk, s in zip(reversed(m.encoder_blocks), reversed(self.enc)):
            dt_tok, dt_op = self._block_bwd(blk, s, dt_tok, dt_op, B, Te)
            self._ready(_block_params(blk)[-1])

        # ---- patch embed + cls token (MCM.py:615-626)
        pw = m.encoder_embed.proj.weight
        self._wg(dt_op, self.patches, E, pw[0].numel(), B * K, G(pw), dt, lda=E, a_remap=(K, Te, 1))
        T.colsum(dt_tok, B * K, E, G(m.encoder_embed.proj.bias), row_group=K, group_stride=Te, row_offset=1)
        T.colsum(dt_tok, B, E, G(m.cls_token).view(-1), row_group=1, group_stride=Te, row_offset=0)
        self._ready(m.cls_token)

    def bwd_begin(self, gflat, sync=None):
        self.gflat, self.sync = gflat, sync
        if sync is not None:
            sync.attach(gflat)
        self._side_begin()

    def dec_bwd(self, dP, out_f32=False):
        """decoder backward (MCM.py:636-688) from dP [B*L, p*p*C] (compute dtype), the gradient of decoder_pred's
        token-layout output: every decoder parameter's gradient; -> the gradient of the decoder's input tokens
        [B*K, E] in the compute dtype (g_s goes on with it) or, out_f32, in f32"""
        m, dt, W, B = self.m, self.dtype, self.w, self.batch
        E, K, L, Dd = m.encoder_embed_dim, m.num_keep_patches, self.L, m.decoder_embed_dim
        Td, Mp = L + 1, self.Mp
        G = self.grad
        # ---- decoder_pred (MCM.py:683-686)
        npred = dP.shape[1]
        self._wg(dP, self.dn, npred, Dd, B * L, G(m.decoder_pred.weight), dt, bias=G(m.decoder_pred.bias))
        ddn = torch.empty((B * L, Dd), dtype=torch.float32, device=self.device)
        T.dgrad_linear(dP, W.t(m.decoder_pred.weight), B * L, npred, Dd, dt, out=ddn)
        ddec = self._z(B * Td, Dd)
        ddec_op = ddec if dt == torch.float32 else self._z(B * Td, Dd, dtype=dt)
        T.layernorm_bwd(self.dec_last, m.decoder_norm.weight, ddn, ddec, B * L, Dd, m.decoder_norm.eps,
                        G(m.decoder_norm.weight), G(m.decoder_norm.bias), dxop=None if dt == torch.float32 else ddec_op,
                        row_group=L, group_stride=Td, row_offset=1)
        self._ready(m.decoder_norm.bias)
        for blk, s in zip(reversed(m.decoder_blocks), reversed(self.dec)):
            ddec, ddec_op = self._block_bwd(blk, s, ddec, ddec_op, B, Td)
            self._ready(_block_params(blk)[-1])

        # ---- decoder_embed + mask tokens (MCM.py:657-675)
        dtok = self._e(Mp, Dd)
        T.decoder_embed_bwd_gather(ddec, self.shuf, dtok, B, K, L, Dd, dt, dmask=G(m.mask_token).view(-1))
        self._wg(dtok, self.gs_out, Dd, E, Mp, G(m.decoder_embed.weight), dt, bias=G(m.decoder_embed.bias))
        d = torch.empty((Mp, E), dtype=torch.float32, device=self.device) if out_f32 else self._e(Mp, E)
        T.dgrad_linear(dtok, W.t(m.decoder_embed.weight), Mp, Dd, E, dt, out=d)
        self._ready(m.mask_token)
        return d

    def _eb_grads(self, eb):
        from ._lib import EBParams

        g = EBParams()
        for i in range(5):
            g.matrix[i] = self.grad(getattr(eb, f"_matrix{i}")).data_ptr()
            g.bias[i] = self.grad(getattr(eb, f"_bias{i}")).data_ptr()
            if i < 4:
                g.factor[i] = self.grad(getattr(eb, f"_factor{i}")).data_ptr()
        g.quantiles = self.grad(eb.quantiles).data_ptr()
        return g

    def _h_s_bwd(self, seq, saved, dout32, dZH):
        dt, W, G, B = self.dtype, self.w, self.grad, self.batch
        layers = _hs_layers(seq)
        d = self._cast(dout32)
        for j in reversed(range(len(layers))):
            c, pshuf = layers[j]
            x, cin, H, _, _ = saved[j]
            cout = c.out_channels
            self._wg(d, x, cout, 9 * cin, B * H * H, G(c.weight), dt, conv=dict(c1=cin, H=H, W=H, cin=cin),
                    layout="conv", bias=G(c.bias))
            if j == 0:
                T.conv_dgrad(d, W.conv_dg(c.weight), B, H, H, 1, cout, cin, dt, routes=[(dZH, cin, cin)])
                break
            _, _, Hp, pshuf_prev, pre_prev = saved[j - 1]
            dx = self._e(B * H * H, cin)
            if pshuf_prev:
                # input of this conv = GELU(PixelShuffle(conv_{j-1})): plain data gradient, then unshuffle * gelu'
                T.conv_dgrad(d, W.conv_dg(c.weight), B, H, H, 1, cout, cin, dt, out=dx)
                c4 = cin * 4
                dpre = self._e(B * Hp * Hp, c4)
                T.unshuffle_bwd(dx, cin, pre_prev, cin, dpre, B, Hp, Hp, c4, dt, dy_f32=(dt == torch.float32))
                d = dpre
            else:
                T.conv_dgrad(d, W.conv_dg(c.weight), B, H, H, 1, cout, cin, dt, out=dx, pre=pre_prev)
                d = dx

    def _slices_bwd(self, dYH, dylik):
        m, dt, W, G, B, g = self.m, self.dtype, self.w, self.grad, self.batch, self.g
        M, S, sw, ms, Mp, HW = m.latent_depth, m.num_slices, self.sw, self.ms, self.Mp, g * g
        esz = self.LMS.element_size()
        lms = self.LMS.data_ptr()
        DY = self._z(Mp, M)
        dLM = self._z(Mp, M)
        dLS = self._z(Mp, M)
        dSUP = self._z(Mp, M)
        # The scale stack of a slice depends on nothing the mean stack writes: eager on a GPU it runs on its own
        # stream beside the mean stack, its support-channel gradients in their own buffer (dSUP2, added where slice
        # j's lrp backward reads column block j), so the two data-gradient chains never touch the same accumulator.
        # Not under graph capture: HIP's graph executor ran that topology 3.4 ms slower per step (31.4 -> 34.8 ms;
        # eager 31.9 -> 31.4), and 6.5 ms slower with joins only where slices <= 5 read dSUP2 (31.9 -> 38.4), so a
        # captured step keeps both stacks on the compute stream, their layers 4..1 as 2-problem data-gradient
        # launches (_stack_bwd_pair; same sums either way).
        conc = self._side is not None and not torch.cuda.is_current_stream_capturing()
        if conc and "_scale_stream" not in self.__dict__:
            self._scale_stream = torch.cuda.Stream(device=self.device)
        dSUP2 = self._z(Mp, M)  # also without the stream: the same sums in the same order either way
        main = torch.cuda.current_stream(self.device) if conc else None
        joined = None
        deferred = []  # eager only: (slice, mean stack's, scale stack's layer 4..1 weight gradients)
        GS = torch.empty((Mp, M), dtype=torch.float32, device=self.device)
        # slices ms..S-1 were run batched in the forward (they condition on the fixed support slots 0..ms-1): their
        # backward is batched too, every data gradient of layers 4..1 one launch for all of them
        nser = ms if S - ms > 1 else S
        if nser < S:
            self._batched_bwd(nser, S - nser, dYH, dylik, DY, dLM, dLS, dSUP, dSUP2, GS)
        for i in reversed(range(nser)):
            # fresh per slice: the side stream's weight gradients of slice i + 1 may still read the last ones
            dT = self._e(Mp, sw)
            dMU, dSG = self._e(Mp, sw), self._e(Mp, sw)
            k = min(i, ms)
            cin_m = M + sw * k
            rec = self.sl[i]
            gs_i = GS.data_ptr() + i * sw * 4
            if joined is not None and i < ms:  # later slices' scale stacks wrote dSUP2's block i (read below)
                main.wait_event(joined)
                joined = None
            # y_hat = y_hat_pre + 0.5 tanh(t)   (MCM.py:782-783)
            T.lrp_bwd(rec["lrp"][-1], sw, dT, sw, Mp, sw, dt, g32=(dSUP.data_ptr() + i * sw * 4) if i < ms else None,
                      ld32=M, g16=dYH.data_ptr() + i * sw * esz, ld16=M, gsum=gs_i, ldgs=M,
                      g32b=(dSUP2.data_ptr() + i * sw * 4) if i < ms else None, ld32b=M)
            self._stack_bwd(_convs(m.lrp_transform[i]), rec["lrp"], dT,
                            (self.LMS, cin_m, 2 * M, self.YPT.data_ptr() + i * sw * esz, sw, M),
                            [(dLM, M, M), (dSUP, M, sw * k), (gs_i, M, sw)])
            # GaussianConditional + quantize_ste (MCM.py:771-776)
            T.gc_bwd(self.Y32, M, i * sw, rec["mean"][-1], rec["scale"][-1], sw, self.y_noise, M, dylik, GS, M, DY, M,
                     dMU, dSG, sw, B, HW, sw, dt)
            scale_args = (_convs(m.cc_transform_scale[i]), rec["scale"], dSG,
                          (self.LS, M, 2 * M, lms + M * esz if k else None, sw * k, 2 * M),
                          [(dLS, M, M), (dSUP2, M, sw * k)])
            mean_args = (_convs(m.cc_transform_mean[i]), rec["mean"], dMU, (self.LMS, cin_m, 2 * M, None, 0, 0),
                         [(dLM, M, M), (dSUP, M, sw * k)])
            if not conc:
                # one stream: layers 4..1 of both stacks as 2-problem data-gradient launches
                self._stack_bwd_pair(mean_args, scale_args)
                self._ready(_convs(m.cc_transform_scale[i])[0].bias)
                continue
            # eager: the scale stack on its own stream, the mean stack first on the compute stream.  Their layers
            # 4..1 weight gradients wait for the final join and then run as the same 2-problem launches a captured
            # step issues (_stack_bwd_pair), so eager and graphed steps sum them with one split plan; the DP
            # hand-offs of these slices follow them.
            fork = torch.cuda.Event()
            fork.record(main)
            im, is_ = [], []
            self._stack_bwd(*mean_args, defer=im)
            ss = self._scale_stream
            ss.wait_event(fork)
            with torch.cuda.stream(ss):
                self._stack_bwd(*scale_args, defer=is_)
            joined = torch.cuda.Event()
            joined.record(ss)
            self._keep.append(dSG)  # read on the scale stream; freed after the backward's join
            deferred.append((i, im, is_))
        if joined is not None:
            main.wait_event(joined)
        for i, im, is_ in deferred:
            for (ia, shp), (ib, _) in zip(im, is_):
                self._wg_many([ia, ib], *shp, layout="conv")
            self._wg_flush()
            self._ready(_convs(m.cc_transform_scale[i])[0].bias)
        return DY, dLM, dLS

    def _batched_bwd(self, i0, nbs, dYH, dylik, DY, dLM, dLS, dSUP, dSUP2, GS):
        """backward of the batched slices i0..i0+nbs-1 (_batched_fwd): per slice the lrp backward, then the lrp stacks'
        layers 4..1 as ONE nbs-problem data-gradient launch each, their first layers one by one (routes into the
        shared latent / support gradients, slices in descending order), the Gaussian backward per slice, then the
        mean and scale stacks' layers 4..1 as ONE 2 nbs-problem launch each and their first layers one by one (mean
        before scale per slice).  Weight gradients per problem on the side stream, as for the serial slices."""
        m, dt, W, G, B, g = self.m, self.dtype, self.w, self.grad, self.batch, self.g
        M, sw, ms, Mp, HW = m.latent_depth, self.sw, self.ms, self.Mp, g * g
        esz = self.LMS.element_size()
        lms = self.LMS.data_ptr()
        k = ms
        sl = list(range(i0, i0 + nbs))
        recs = [self.sl[i] for i in sl]
        cl = [_convs(m.lrp_transform[i]) for i in sl]
        cm = [_convs(m.cc_transform_mean[i]) for i in sl]
        cs = [_convs(m.cc_transform_scale[i]) for i in sl]

        def stride(views, what):
            """constant element stride between consecutive problems' views (the batched forward's buffers)"""
            d = {(b.data_ptr() - a.data_ptr()) for a, b in zip(views, views[1:])}
            e = views[0].element_size()
            if len(d) > 1 or (d and next(iter(d)) % e):
                raise RuntimeError(f"batched slice backward: {what} not at a constant stride")
            return (next(iter(d)) // e) if d else 0

        def stacks(convs, saved, dtop, what, groups=1):
            """layers 4..1 of len(convs) same-shape stacks, problem p's saved activations saved[p]; dtop [P][Mp][cout];
            the weight gradients of each of `groups` consecutive problem groups (lrp / mean / scale) as one batched
            launch per layer"""
            P = len(convs)
            fd = self._fused_dgrads([(convs[p_], saved[p_], dtop[p_]) for p_ in range(P)])
            if fd is not None:  # the data gradients in one launch, then the weight gradients per layer
                for l in range(4, 0, -1):
                    cin, cout = convs[0][l].in_channels, convs[0][l].out_channels
                    q = P // groups
                    for g0 in range(0, P, q):
                        self._wg_many([{"a": fd[l][p_], "b": saved[p_][l - 1][0], "out": G(convs[p_][l].weight),
                                        "bias": G(convs[p_][l].bias)} for p_ in range(g0, g0 + q)],
                                      cout, 9 * cin, Mp, dt, conv=dict(c1=cin, H=g, W=g, cin=cin), layout="conv")
                return fd[0]
            d = dtop
            for l in range(4, 0, -1):
                cin, cout = convs[0][l].in_channels, convs[0][l].out_channels
                q = P // groups
                for g0 in range(0, P, q):
                    self._wg_many([{"a": d[p_], "b": saved[p_][l - 1][0], "out": G(convs[p_][l].weight),
                                    "bias": G(convs[p_][l].bias)} for p_ in range(g0, g0 + q)],
                                  cout, 9 * cin, Mp, dt, conv=dict(c1=cin, H=g, W=g, cin=cin), layout="conv")
                wd = W.packed([c[l].weight for c in convs], "conv_dg")
                pres = [saved[p_][l - 1][1] for p_ in range(P)]
                dx = self._e(P, Mp, cin)
                T.conv_dgrad(d[0], wd[0], B, g, g, 1, cout, cin, dt, out=dx[0], pre=pres[0],
                             batch=(P, Mp * cout, wd[0].numel(), Mp * cin, stride(pres, what + " pre")))
                d = dx
            return d

        # ---- lrp: y_hat = y_hat_pre + 0.5 tanh(t) backward, per slice (no support gradients beyond slot ms - 1)
        dT = self._e(nbs, Mp, sw)
        for j, i in enumerate(sl):
            T.lrp_bwd(recs[j]["lrp"][-1], sw, dT[j], sw, Mp, sw, dt, g16=dYH.data_ptr() + i * sw * esz, ld16=M,
                      gsum=GS.data_ptr() + i * sw * 4, ldgs=M)
        dl = stacks(cl, [r["lrp"] for r in recs], dT, "lrp")
        cin, cout = M + sw * k + sw, cl[0][0].out_channels
        self._wg_many([{"a": dl[j], "b": self.LMS, "x2": self.YPT.data_ptr() + i * sw * esz, "out": G(cl[j][0].weight),
                        "bias": G(cl[j][0].bias)} for j, i in enumerate(sl)],
                      cout, 9 * cin, Mp, dt, conv=dict(c1=M + sw * k, ld2=M, H=g, W=g, cin=cin), layout="conv",
                      ldb=2 * M)
        for j in reversed(range(nbs)):
            i, c = sl[j], cl[j][0]
            T.conv_dgrad(dl[j], W.conv_dg(c.weight), B, g, g, 1, cout, cin, dt,
                         routes=[(dLM, M, M), (dSUP, M, sw * k), (GS.data_ptr() + i * sw * 4, M, sw)])
        self._wg_flush()
        # ---- GaussianConditional + quantize_ste per slice -> d mu, d sigma of every problem ([mean | scale][slice])
        dMS = self._e(2, nbs, Mp, sw)
        for j, i in enumerate(sl):
            T.gc_bwd(self.Y32, M, i * sw, recs[j]["mean"][-1], recs[j]["scale"][-1], sw, self.y_noise, M, dylik, GS, M,
                     DY, M, dMS[0, j], dMS[1, j], sw, B, HW, sw, dt)
        dms = stacks(cm + cs, [r["mean"] for r in recs] + [r["scale"] for r in recs], dMS.view(2 * nbs, Mp, sw),
                     "mean/scale", groups=2)
        firsts = ((cm, (self.LMS, M + sw * k, 2 * M, None, 0, 0), lambda j: [(dLM, M, M), (dSUP, M, sw * k)]),
                  (cs, (self.LS, M, 2 * M, lms + M * esz, sw * k, 2 * M), lambda j: [(dLS, M, M), (dSUP2, M, sw * k)]))
        for t, (convs, first, _) in enumerate(firsts):
            x1, c1, ld1, x2, c2, ld2 = first
            cin, cout = c1 + c2, convs[0][0].out_channels
            self._wg_many([{"a": dms[t * nbs + j], "b": x1, "x2": x2, "out": G(convs[j][0].weight),
                            "bias": G(convs[j][0].bias)} for j in range(nbs)],
                          cout, 9 * cin, Mp, dt, conv=dict(c1=c1, ld2=ld2, H=g, W=g, cin=cin), layout="conv", ldb=ld1)
        for j in reversed(range(nbs)):
            for t, (convs, first, routes) in enumerate(firsts):
                c, d = convs[j][0], dms[t * nbs + j]
                cin, cout = first[1] + first[4], c.out_channels
                T.conv_dgrad(d, W.conv_dg(c.weight), B, g, g, 1, cout, cin, dt, routes=routes(j))
            self._wg_flush()
            self._ready(cs[j][0].bias)  # every gradient of slices >= i0 + j is final (DP hand-off per slice)

    def _fused_dgrads(self, stacks, routes=None):
        """layers 4..1 data gradients of P same-shape stacks (convs, saved, dtop) in ONE tmae_lic_stack backward
        launch (the chain through LDS, TMAE_LIC_STACK_BWD), or None when the operands do not allow it (the per-layer
        launches then run).  Returns d[l] for l = 0..4: the gradient w.r.t. layer l's pre-activation, a list over the
        problems (d[4] = the dtops); d[0..3] are views of one [P][Mp][cout] bf16 buffer per layer.  routes (one list
        per problem, the problems' accumulators disjoint): the first layers' input gradients too, routed like
        T.conv_dgrad's (the caller then skips them)."""
        if not self._fused_bwd:
            return None
        P, Mp = len(stacks), self.Mp
        convs0 = stacks[0][0]
        couts = [c.out_channels for c in convs0]
        if len(convs0) != 5 or any(c > ops.LSTK_MAXC for c in couts[:4]):
            return None

        def delta(ts):
            d = {t.data_ptr() - ts[0].data_ptr() for t in ts[1:]}
            return 0 if not d else (next(iter(d)) // ts[0].element_size() if len(d) == 1 else None)

        dts = [s[2] for s in stacks]
        pres = [[s[1][l][1] for s in stacks] for l in (3, 2, 1, 0)]
        sx = delta(dts)
        if sx is None or any(p_[0].dtype != torch.bfloat16 or (P > 1 and delta(p_) != Mp * couts[l])
                             for p_, l in zip(pres, (3, 2, 1, 0))):
            return None
        ws = [self.w.packed([s[0][l].weight for s in stacks], "licT") for l in (4, 3, 2, 1)]
        outs = [self._e(P, Mp, couts[l]) for l in (3, 2, 1, 0)]
        st = {"x1": (sx, 0)}
        for k, l in enumerate((3, 2, 1, 0)):
            st[f"w{k}"] = (ws[k][0].numel() if P > 1 else 0, 0)
            st[f"s{k}"] = (Mp * couts[l], 0)
        lcouts = [couts[l] for l in (3, 2, 1, 0)]
        if routes is not None:  # + the first layers' input gradients, routed
            ws.append(self.w.packed([s[0][0].weight for s in stacks], "licT"))
            st["w4"] = (ws[4][0].numel() if P > 1 else 0, 0)
            lcouts.append(convs0[0].in_channels)
        ops.lic_stack_bwd(self.batch, self.g, dts[0], couts[4], couts[4], ws, lcouts, [p_[0] for p_ in pres], outs,
                          nb=(P, 1), strides=st, routes=routes)
        d = [None] * 5
        for k, l in enumerate((3, 2, 1, 0)):
            d[l] = [outs[k][p_] for p_ in range(P)]
        d[4] = dts
        return d

    def _stack_bwd_pair(self, a, b):
        """_stack_bwd of two stacks with the same layer shapes (a slice's mean and scale stacks): the data gradients
        of layers 4..1 as one 2-problem launch (the fused chain, or one 2-problem conv launch per layer); the weight
        gradients of layers 4..1 as 2-problem launches; the first layers (their own input splits / routes) one by one,
        a's before b's"""
        dt, W, G, B, g, Mp = self.dtype, self.w, self.grad, self.batch, self.g, self.Mp
        (ca, sa, da, fa, ra), (cb, sb, db, fb, rb) = a, b
        fd = self._fused_dgrads([(ca, sa, da), (cb, sb, db)], routes=[ra, rb] if self.FUSE_FIRST_DGRAD else None)
        for l in range(4, 0, -1):
            cin = ca[l].in_channels
            dl = (fd[l][0], fd[l][1]) if fd is not None else (da, db)
            self._wg_many([{"a": d, "b": saved[l - 1][0], "out": G(c.weight), "bias": G(c.bias)}
                           for c, saved, d in ((ca[l], sa, dl[0]), (cb[l], sb, dl[1]))],
                          ca[l].out_channels, 9 * cin, Mp, dt, conv=dict(c1=cin, H=g, W=g, cin=cin), layout="conv")
            if fd is not None:
                continue
            cin, cout = ca[l].in_channels, ca[l].out_channels
            assert (cb[l].in_channels, cb[l].out_channels) == (cin, cout)
            dxa, dxb = self._e(Mp, cin), self._e(Mp, cin)
            T.conv_dgrad(da, W.conv_dg(ca[l].weight), B, g, g, 1, cout, cin, dt, out=dxa, pre=sa[l - 1][1],
                         second=(db, W.conv_dg(cb[l].weight), dxb, sb[l - 1][1]))
            da, db = dxa, dxb
        if fd is not None:
            da, db = fd[0]
        for c, d, first, routes in ((ca[0], da, fa, ra), (cb[0], db, fb, rb)):
            x1, c1, ld1, x2, c2, ld2 = first
            cin, cout = c1 + c2, c.out_channels
            self._wg(d, x1, cout, 9 * cin, Mp, G(c.weight), dt, ldb=ld1,
                     conv=dict(x2=x2, c1=c1, ld2=ld2, H=g, W=g, cin=cin), layout="conv", bias=G(c.bias))
            if fd is None or not self.FUSE_FIRST_DGRAD:
                T.conv_dgrad(d, W.conv_dg(c.weight), B, g, g, 1, cout, cin, dt, routes=routes)
        self._wg_flush()

    def _stack_bwd(self, convs, saved, dtop, first, routes, defer=None):
        """backward of one 5-layer slice stack; with `defer` (a list) the weight gradients of layers 4..1 are
        appended to it as (_wg_many item, shape args) instead of being queued"""
        dt, W, G, B, g, Mp = self.dtype, self.w, self.grad, self.batch, self.g, self.Mp
        fd = self._fused_dgrads([(convs, saved, dtop)], routes=[routes] if self.FUSE_FIRST_DGRAD else None)
        d = dtop
        for l in range(4, 0, -1):
            c = convs[l]
            cin, cout = c.in_channels, c.out_channels
            act_prev, pre_prev = saved[l - 1]
            if fd is not None:
                d = fd[l][0]
            if defer is not None:
                defer.append(({"a": d, "b": act_prev, "out": G(c.weight), "bias": G(c.bias)},
                              (cout, 9 * cin, Mp, dt, dict(c1=cin, H=g, W=g, cin=cin))))
            else:
                self._wg(d, act_prev, cout, 9 * cin, Mp, G(c.weight), dt, conv=dict(c1=cin, H=g, W=g, cin=cin),
                         layout="conv", bias=G(c.bias))
            if fd is not None:
                continue
            dx = self._e(Mp, cin)
            T.conv_dgrad(d, W.conv_dg(c.weight), B, g, g, 1, cout, cin, dt, out=dx, pre=pre_prev)
            d = dx
        if fd is not None:
            d = fd[0][0]
        c = convs[0]
        x1, c1, ld1, x2, c2, ld2 = first
        cin, cout = c1 + c2, c.out_channels
        self._wg(d, x1, cout, 9 * cin, Mp, G(c.weight), dt, ldb=ld1,
                 conv=dict(x2=x2, c1=c1, ld2=ld2, H=g, W=g, cin=cin), layout="conv", bias=G(c.bias))
        # zero-width routes (no support slices yet) stay in place: their limits still partition the channels
        if fd is None or not self.FUSE_FIRST_DGRAD:
            T.conv_dgrad(d, W.conv_dg(c.weight), B, g, g, 1, cout, cin, dt, routes=routes)
        self._wg_flush()

def _bias(b):
    return None if b is None else b.detach()


def _block_params(blk):
    ps = [blk.mlp.fc2.weight, blk.mlp.fc2.bias, blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.norm2.weight, blk.norm2.bias,
          blk.attn.proj.weight, blk.attn.proj.bias, blk.attn.qkv.weight]
    if blk.attn.qkv.bias is not None:
        ps.append(blk.attn.qkv.bias)
    ps += [blk.norm1.weight, blk.norm1.bias]
    return ps


def _hs_layers(seq):
    """h_s layers as (conv, followed_by_pixel_shuffle)"""
    out = []
    for l in seq:
        if isinstance(l, nn.Conv2d):
            out.append((l, False))
        elif isinstance(l, nn.Sequential):
            out.append((l[0], True))
    return out


def _hs_convs(seq):
    return [c for c, _ in _hs_layers(seq)]


class _MCMTrainFn(torch.autograd.Function):
    """MCM.forward as one autograd node: (imgs, scores, *params) -> (x_hat, y likelihood, z likelihood)"""

    @staticmethod
    def forward(ctx, ex, noise, imgs, scores, *params):
        x_hat, ylik, zlik = ex.forward(imgs, scores, noise)
        ctx.ex = ex
        ctx.params = params
        return x_hat, ylik, zlik

    @staticmethod
    def backward(ctx, dxhat, dylik, dzlik):
        ex = ctx.ex
        params = ctx.params
        # a pre-existing .grad (accumulation across calls, zero_grad(set_to_none=False)) is added to by
        # autograd: write into a fresh buffer then, so the returned views never alias p.grad
        fresh = any(p.grad is not None for p in params if p.requires_grad)
        gflat = ex.grads_buffer(fresh)
        sync = getattr(ex.m, "grad_sync", None)
        ex.backward(dxhat, dylik, dzlik, gflat, sync=sync)
        if sync is not None:
            sync.finish()
        out = []
        for p in params:
            if not p.requires_grad:
                out.append(None)
            else:
                off = ex.offsets[id(p)]
                out.append(gflat[off:off + p.numel()].view(p.shape))
        return (None, None, None, None, *out)


# ---------------------------------------------------------------------- forward_encoder / forward_decoder alone
# (MCM.py:590-688 as separate nn.Module calls under autograd, like mae_train.py's: each is its own node over its own
# parameters; the executor keeps one set of activations per stage, so a stage's backward must come before that
# stage's next forward -- checked by the executor's forward counters.  No DP hand-offs: sync stays None.)
def enc_params(m):
    out = [m.encoder_norm.weight, m.encoder_norm.bias]
    for blk in m.encoder_blocks:
        out += _block_params(blk)
    return out + [m.encoder_embed.proj.weight, m.encoder_embed.proj.bias, m.cls_token]


def dec_params(m):
    out = [m.decoder_pred.weight, m.decoder_pred.bias, m.decoder_norm.weight, m.decoder_norm.bias,
           m.decoder_embed.weight, m.decoder_embed.bias, m.mask_token]
    for blk in m.decoder_blocks:
        out += _block_params(blk)
    return out


def _param_grads(ex, params, gflat):
    return [gflat[ex.offsets[id(p)]:ex.offsets[id(p)] + p.numel()].view(p.shape) if p.requires_grad else None
            for p in params]


class _MCMEncFn(torch.autograd.Function):
    """MCM.forward_encoder: (imgs, scores, *encoder params) -> (x_remain f32 [B, K, E], ids_restore)"""

    @staticmethod
    def forward(ctx, ex, imgs, scores, *params):
        x = ex.enc_fwd(ex._begin(imgs), scores, out_dtype=torch.float32)
        ctx.ex, ctx.params, ctx.gen = ex, params, ex.enc_gen
        ctx.mark_non_differentiable(ex.rest)
        return x.view(ex.batch, ex.m.num_keep_patches, -1), ex.rest

    @staticmethod
    def backward(ctx, dx, drest):
        ex, params = ctx.ex, ctx.params
        if ex.enc_gen != ctx.gen:
            raise RuntimeError("forward_encoder (or forward) ran again on this model before this backward: its saved "
                               "activations are gone (backward each forward_encoder before the next)")
        gflat = ex.grads_buffer(any(p.grad is not None for p in params if p.requires_grad))
        ex.bwd_begin(gflat)
        ex.enc_bwd(dx.float().contiguous().view(ex.Mp, -1))
        ex._side_join()
        return (None, None, None, *_param_grads(ex, params, gflat))


class _MCMDecFn(torch.autograd.Function):
    """MCM.forward_decoder: (x_remain [B, K, E], *decoder params) -> preds f32 [B, L, p*p*C] (ids_restore fixed)"""

    @staticmethod
    def forward(ctx, ex, ids_restore, x, *params):
        ex.rest = ids_restore
        ex.shuf = ops.invert_permutation(ids_restore)
        ex.w.refresh()  # (a no-op after forward_encoder's)
        preds = ex.dec_fwd(ex._cast(x.float().contiguous().view(ex.Mp, -1)), tokens=True)
        ctx.ex, ctx.params, ctx.gen, ctx.xshape = ex, params, ex.dec_gen, x.shape
        return preds.view(ex.batch, ex.L, -1)

    @staticmethod
    def backward(ctx, dpreds):
        ex, params = ctx.ex, ctx.params
        if ex.dec_gen != ctx.gen:
            raise RuntimeError("forward_decoder (or forward) ran again on this model before this backward: its saved "
                               "activations are gone (backward each forward_decoder before the next)")
        gflat = ex.grads_buffer(any(p.grad is not None for p in params if p.requires_grad))
        ex.bwd_begin(gflat)
        dP = ex._cast(dpreds.float().contiguous().view(ex.batch * ex.L, -1))  # the node starts at dP: no patchify
        dx = ex.dec_bwd(dP, out_f32=True)
        ex._side_join()
        return (None, None, dx.view(ctx.xshape), *_param_grads(ex, params, gflat))


def _exec_for(m, B, device):
    if getattr(m, "grad_sync", None) is not None:
        raise RuntimeError("MCM.forward_encoder / forward_decoder under autograd run without gradient all-reduce: "
                           "bucketed data parallel (grad_sync) covers forward() only")
    dt = m.compute_dtype
    if torch.is_autocast_enabled() and dt == torch.float32:
        dt = torch.bfloat16
    ex = getattr(m, "_train_exec", None)
    if ex is None or ex.batch != B or ex.dtype != dt or ex.device != device:
        ex = m._train_exec = TrainExec(m, B, dt, device)
    return ex


def train_forward_encoder(m, imgs, scores):
    """MCM.forward_encoder with autograd: (x_remain f32 [N, K, E], ids_restore)"""
    ex = _exec_for(m, imgs.shape[0], imgs.device)
    return _MCMEncFn.apply(ex, imgs, scores, *enc_params(m))


def train_forward_decoder(m, x, ids_restore):
    """MCM.forward_decoder with autograd: preds f32 [N, L, p*p*C] (gradients to x and the decoder's parameters)"""
    n, ntok, _ = x.shape
    if ntok != m.num_keep_patches:
        raise ValueError(f"forward_decoder under autograd takes num_keep_patches={m.num_keep_patches} tokens per image "
                         f"(the training workspaces are sized by it), got {ntok}")
    ex = _exec_for(m, n, x.device)
    return _MCMDecFn.apply(ex, ids_restore.to(x.device).to(torch.int64).contiguous(), x, *dec_params(m))


class BppFn(torch.autograd.Function):
    """RateDistortionLoss bpp term (rd_loss.py:19-20) with its HIP backward"""

    @staticmethod
    def forward(ctx, ylik, zlik, num_pixels):
        ctx.save_for_backward(ylik, zlik)
        ctx.num_pixels = num_pixels
        return ops.bpp(ylik, zlik, num_pixels)

    @staticmethod
    def backward(ctx, g):
        ylik, zlik = ctx.saved_tensors
        g = g.float().contiguous().reshape(1)
        dy = T.bpp_bwd(ylik.contiguous(), g, torch.empty_like(ylik), ctx.num_pixels)
        dz = T.bpp_bwd(zlik.contiguous(), g, torch.empty_like(zlik), ctx.num_pixels)
        return dy, dz, None


class AuxLossFn(torch.autograd.Function):
    """EntropyBottleneck.loss (compressai; utils/engine.py:79, 87): gradient only to quantiles"""

    @staticmethod
    def forward(ctx, eb, quantiles):
        ctx.eb = eb
        return ops.eb_aux_loss(eb)

    @staticmethod
    def backward(ctx, g):
        eb = ctx.eb
        dq = torch.empty_like(eb.quantiles)
        T.eb_aux_bwd(ops._eb_params(eb), eb.target, g.float().contiguous().reshape(1), dq, eb.channels)
        return None, dq
