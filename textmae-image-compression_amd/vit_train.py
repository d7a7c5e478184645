"""What the MCM and MAE training executors share (mcm_train.TrainExec, mae_train.MAETrainExec): workspaces, the flat
gradient buffer, the side-stream weight gradients and the timm Block forward / backward."""
from __future__ import annotations

import torch

from . import ops
from . import train_ops as T
from .ops import ACT_GELU

# side-stream weight gradients size their split-K for half the chip's CU slots (the data-gradient chain holds the
# rest): graphed step 31.49 -> 31.24 ms; a quarter made the side stream the critical path (40.2 ms)
_SIDE_SLOT_DIV = 2


def _bias(b):
    return None if b is None else b.detach()


def _block_params(blk):
    ps = [blk.mlp.fc2.weight, blk.mlp.fc2.bias, blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.norm2.weight, blk.norm2.bias,
          blk.attn.proj.weight, blk.attn.proj.bias, blk.attn.qkv.weight]
    if blk.attn.qkv.bias is not None:
        ps.append(blk.attn.qkv.bias)
    ps += [blk.norm1.weight, blk.norm1.bias]
    return ps


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

    @staticmethod
    def _stride(vals, esz=None):
        """the constant element stride between consecutive problems' operands -- views of one buffer, or raw addresses
        inside one (then with esz, the element size): 0 for a single problem or when every operand is None, None when
        the problems are not evenly spaced"""
        if vals[0] is None:
            return 0 if all(v is None for v in vals) else None
        ptrs = [v if isinstance(v, int) else v.data_ptr() for v in vals]
        esz = esz or vals[0].element_size()
        d = {b - a for a, b in zip(ptrs, ptrs[1:])}
        if not d:
            return 0
        if len(d) != 1 or next(iter(d)) % esz:
            return None
        return next(iter(d)) // esz

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
        third stream joined to both, measured 36.7-37.6 ms; a lag of 2 / 4 hand-offs 31.8 / 33.2 ms; other HIP graph
        queue counts (2 / 3) changed nothing."""
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
        eb = items[0]["b"].element_size()
        st = [self._stride([it.get(key) for it in items], esz)
              for key, esz in (("a", items[0]["a"].element_size()), ("b", eb), ("x2", eb), ("out", 4), ("bias", 4))]
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
