"""Train / validation loops — counterparts of reference utils/engine.py:30-219 with the same call
pattern on the model (``model(samples, total_scores)``, ``criterion(out_net, samples)``,
``model.aux_loss()``, loss.backward(), clip_grad_norm_(model.parameters(), clip), optimizer.step(),
aux_loss.backward(), aux_optimizer.step(), zero_grad x2) and the same metric names.

What differs (MI355X-side, not semantics):
  * the six per-step metric all-reduces of the reference (engine.py:117-122, each behind a blocking
    ``.item()``) are ONE 6-element all-reduce, read back once per step;
  * the gradient all-reduce of data parallelism runs inside the backward (parallel.GradSync);
  * with ``fused=True`` clip_grad_norm_ / Adam are the flat-buffer HIP kernels (optim.py).
Logging (MetricLogger / TensorBoard) is out of scope.
"""
from __future__ import annotations

import numpy as np
import torch

from . import distributed
from .optim import FusedAdam, clip_grad_norm_, clip_norm_deferred


def _clip_buffer(optimizer):
    """the persistent [norm, factor] f32 pair of this optimizer's deferred clip (allocated outside any capture)"""
    buf = getattr(optimizer, "_clip_buf", None)
    if buf is None:
        dev = next(p.device for g in optimizer.param_groups for p in g["params"])
        buf = optimizer._clip_buf = torch.empty(2, dtype=torch.float32, device=dev)
    return buf

def _drain_watchdog(group):
    """Return once the process group's watchdog holds no pending work: ``_wait_for_pending_works`` blocks until
    its work list is empty (the GPU must have finished them, so the device is synchronised first)."""
    import torch.distributed as dist

    torch.cuda.synchronize()
    pg = group if group is not None else dist.group.WORLD
    pg._wait_for_pending_works()


METRICS = ("loss", "L1_loss", "ssim_loss", "vgg_loss", "bpp_loss", "aux_loss")


def train_step(model, criterion, samples, total_scores, optimizer, aux_optimizer, clip_max_norm=1.0, accum_iter=1,
               step_now=True, noise=None, q=None, lmbda=None, qoffsets=None, qlevels=None, _qmap_kw=None):
    """one iteration of the reference loop body (utils/engine.py:72-91); returns the device losses.  q: the y
    quantiser step of this iteration (MCM.forward's q: an int, one per image, or an int32 device tensor), lmbda: the
    criterion's weight for it (RateDistortionLoss.forward's lmbda, e.g. rd_loss.lmbda_for_q).  qoffsets / qlevels
    (DESIGN.md §3.20): a table of ladder offsets and the source of the per-patch levels ("scores", the default, or a
    map); the step then runs MCM.forward_qmap, q being the base position"""
    kw = {}
    if noise is not None:
        kw["noise"] = noise
    if q is not None:
        kw["q"] = q
    if qoffsets is None:
        if qlevels is not None:
            raise ValueError("train_step: qlevels without qoffsets (the table the levels index)")
        out_net = model(samples, total_scores, **kw)
    else:
        out_net = model.forward_qmap(samples, total_scores, qoffsets=qoffsets,
                                     qlevels="scores" if qlevels is None else qlevels, **kw, **(_qmap_kw or {}))
    out_criterion = criterion(out_net, samples) if lmbda is None else criterion(out_net, samples, lmbda=lmbda)
    out_criterion["loss"] = out_criterion["loss"] / accum_iter
    aux_loss = model.aux_loss() / accum_iter
    if step_now:
        out_criterion["loss"].backward()
        scale = None
        if clip_max_norm > 0:
            if isinstance(optimizer, FusedAdam):
                # the clip factor goes into the Adam update (g * s, the product the in-place scale would store):
                # one pass over the 805 MB gradient buffer less; the gradients are zeroed below either way
                buf = _clip_buffer(optimizer)
                if clip_norm_deferred(model.parameters(), clip_max_norm, buf):
                    scale = buf[1:]
            else:
                clip_grad_norm_(model.parameters(), clip_max_norm)
        if scale is not None:
            optimizer.step(grad_scale=scale)
        else:
            optimizer.step()
        aux_loss.backward()
        aux_optimizer.step()
        optimizer.zero_grad()
        aux_optimizer.zero_grad()
    out_criterion["aux_loss"] = aux_loss
    return out_criterion


class GraphedTrainStep:
    """The loop body of utils/engine.py:72-91 (``train_step``) captured ONCE into a HIP graph and replayed per
    batch: forward (HIP kernels, device noise from torch's graph-safe generator), RateDistortionLoss, aux loss,
    the HIP backward, clip_grad_norm_, both FusedAdam steps and zero_grad are one ``graph.replay()``, so the host
    enqueues one launch per step instead of ~2500.

    What makes the step capturable: the library never allocates or synchronises; the optimizer's step counts
    and bias corrections live on the device (optim.FusedAdam); launch tables built during capture come from
    pinned memory (optim.device_table); the gradient buffer is persistent.  Construction runs ``warmup`` eager
    training steps on the first batch (ordinary optimizer steps: lazy workspaces and tables are created outside
    the capture), then captures one more step without running it.

    Each call copies the batch into the graph's static input tensors, replays, and advances the parameters'
    version counters (the update kernel writes through raw pointers; the executors' weight caches are keyed on
    the versions, so an eager forward after replays re-lays out the new weights).  The learning rates, betas,
    eps and weight decays are baked into the graph: when any of them changes, the step is captured again.
    Data parallelism over RCCL is captured too: GradSync's bucketed all-reduces are issued from inside the captured
    backward, so every replay runs them on the process group's stream under the remaining backward kernels, joined
    before clip / Adam (one ``graph.replay()`` per step at any world size, like the reference's one loop body,
    utils/engine.py:75-91).  The RCCL communicator exists before the capture (the eager warm-up step's
    collectives).  A gloo group (host-staged all-reduce) is refused: use ``train_step`` there.

    q / lmbda, given at capture: the y quantiser step of the captured step (an int or one per
    image) and the criterion's weight live in a static int32 [B] and a static 0-d f32 device buffer that every call
    refreshes, so both may change from replay to replay without a new capture: the captured forward and backward
    always run the kernels with a step, at q = 0 too.

    qoffsets / qlevels, given at capture: the step runs MCM.forward_qmap.  The table lives in a
    static int32 [B, 16] device buffer that every call refreshes, so its values may change from replay to replay; its
    size is fixed at capture (the level rule depends on it) and a table of another size raises.  With qlevels =
    "scores" (the default) the selection and the map's construction are kernels of the captured step.  With a device
    map of levels (int32 [B, L], image patch order) the step keeps a static [B, L] buffer refreshed per call; the
    map's status is not read during a replay: ``step.qlevels_status`` (int32 [B], 1 = an entry outside the table) is
    the caller's to read, and an image with such an entry trains at all-zero levels, as the kernel defines."""

    def __init__(self, model, criterion, optimizer, aux_optimizer, samples, total_scores, clip_max_norm=1.0,
                 warmup=1, noise=None, q=None, lmbda=None, qoffsets=None, qlevels=None):
        sync = getattr(model, "grad_sync", None)
        if sync is not None and not sync.capturable():
            raise ValueError("GraphedTrainStep: a gloo gradient all-reduce (host-staged) is not capturable; use "
                             "engine.train_step, or the nccl (RCCL) backend whose collectives the graph holds")
        if not samples.is_cuda:
            raise ValueError("GraphedTrainStep needs device inputs")
        self.model, self.criterion = model, criterion
        self.optimizer, self.aux_optimizer = optimizer, aux_optimizer
        self.clip_max_norm = clip_max_norm
        self.samples = samples.detach().clone()
        self.total_scores = total_scores.detach().clone()
        # injected quantisation noise (parity tests): static tensors refreshed per call like the batch
        self.noise = tuple(t.detach().clone() for t in noise) if noise is not None else None
        dev = samples.device
        self.q = None if q is None else torch.empty(samples.shape[0], dtype=torch.int32, device=dev)
        self.lmbda = None if lmbda is None else torch.empty((), dtype=torch.float32, device=dev)
        self._refresh_q(q, lmbda)
        B = samples.shape[0]
        self.qoffsets = self.qlevels = self.nlev = None
        if qoffsets is None:
            if qlevels is not None:
                raise ValueError("GraphedTrainStep: qlevels without qoffsets (the table the levels index)")
        else:
            from .bitstream import check_offsets

            self.nlev = len(check_offsets(qoffsets, "GraphedTrainStep: qoffsets"))
            self.qoffsets = torch.zeros((B, 16), dtype=torch.int32, device=dev)
            if qlevels is not None and not isinstance(qlevels, str):
                if not (torch.is_tensor(qlevels) and qlevels.is_cuda and qlevels.dtype == torch.int32
                        and qlevels.dim() == 2 and qlevels.shape[0] == B):
                    raise ValueError("GraphedTrainStep: qlevels must be 'scores' or an int32 [B, L] device tensor")
                self.qlevels = torch.empty_like(qlevels, memory_format=torch.contiguous_format)
            elif qlevels not in (None, "scores"):
                raise ValueError(f"GraphedTrainStep: qlevels = {qlevels!r}: 'scores' or an int32 [B, L] device tensor")
        self._refresh_qmap(qoffsets, qlevels)
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.graph, self.out = None, None
        self._capture(warmup)

    @property
    def qlevels_status(self):
        """the last step's status of a device map of levels (int32 [B] on the device; None without such a map)"""
        ex = getattr(self.model, "_train_exec", None)
        return None if self.qlevels is None or ex is None else ex.qm_status

    def _refresh_qmap(self, qoffsets, qlevels):
        """copy this call's table (and device map of levels) into the static buffers"""
        if (qoffsets is None) != (self.qoffsets is None):
            raise ValueError("GraphedTrainStep: qoffsets must be given at every call iff it was given at capture")
        if qoffsets is None:
            if qlevels is not None:
                raise ValueError("GraphedTrainStep: qlevels without qoffsets (the table the levels index)")
            return
        from .bitstream import check_offsets, offsets_row

        offs = check_offsets(qoffsets, "GraphedTrainStep: qoffsets")
        if len(offs) != self.nlev:
            raise ValueError(f"GraphedTrainStep: a table of {len(offs)} offsets at a step captured with {self.nlev}: "
                             "the table size is fixed at capture")
        self._offs = offs
        self.qoffsets.copy_(torch.tensor([offsets_row(offs)] * self.qoffsets.shape[0], dtype=torch.int32),
                            non_blocking=True)
        given = qlevels is not None and not isinstance(qlevels, str)
        if given != (self.qlevels is not None):
            raise ValueError("GraphedTrainStep: a map of levels must be given at every call iff it was given at capture")
        if given:
            if not torch.is_tensor(qlevels) or qlevels.dtype != torch.int32 or qlevels.shape != self.qlevels.shape:
                raise ValueError(f"GraphedTrainStep: qlevels must be int32 {tuple(self.qlevels.shape)}")
            self.qlevels.copy_(qlevels, non_blocking=True)

    def _hyper(self):
        return tuple((g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"])
                     for o in (self.optimizer, self.aux_optimizer) for g in o.param_groups)

    def _refresh_q(self, q, lmbda):
        """copy this call's q / lmbda into the static buffers (copy_ on the current stream, ahead of the replay)"""
        if (q is None) != (self.q is None):
            raise ValueError("GraphedTrainStep: q must be given at every call iff it was given at capture")
        if (lmbda is None) != (self.lmbda is None):
            raise ValueError("GraphedTrainStep: lmbda must be given at every call iff it was given at capture")
        if q is not None:
            if not (torch.is_tensor(q) and q.is_cuda):
                from .mcm import MCM

                qs = MCM._check_q(q, self.q.numel(), "GraphedTrainStep") or [0] * self.q.numel()
                q = torch.tensor(qs, dtype=torch.int32)
            elif q.dtype != torch.int32 or q.shape != self.q.shape:
                raise ValueError(f"GraphedTrainStep: a device q must be int32 {tuple(self.q.shape)}, got {q.dtype} "
                                 f"{tuple(q.shape)}")
            self.q.copy_(q, non_blocking=True)
        if lmbda is not None:
            if torch.is_tensor(lmbda):
                self.lmbda.copy_(lmbda.detach().reshape(()), non_blocking=True)
            else:
                self.lmbda.fill_(float(lmbda))

    def _step(self):
        return train_step(self.model, self.criterion, self.samples, self.total_scores, self.optimizer,
                          self.aux_optimizer, self.clip_max_norm, noise=self.noise, q=self.q, lmbda=self.lmbda,
                          **self._qmap_args())

    def _qmap_args(self):
        """train_step's arguments of the map: the captured table stands for its size only, the values come from the
        static rows; a device map's status is left on the device"""
        if self.qoffsets is None:
            return {}
        return dict(qoffsets=self._offs, qlevels="scores" if self.qlevels is None else self.qlevels,
                    _qmap_kw=dict(_rows=self.qoffsets, _read_status=False))

    def _capture(self, warmup):
        self.graph, self.out = None, None
        cur = torch.cuda.current_stream(self.samples.device)
        side = torch.cuda.Stream(device=self.samples.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._step()
        cur.wait_stream(side)
        self.optimizer.zero_grad()
        self.aux_optimizer.zero_grad()
        # every weight cache stale at capture time, so the graph always carries the per-step weight re-layout
        from .optim import bump_versions, reserve_capture_staging

        bump_versions(self.params)
        self._staging = reserve_capture_staging()  # the graph's copy nodes read it at every replay
        sync = getattr(self.model, "grad_sync", None)
        mode = "global"
        if sync is not None and (sync.world() > 1 or sync.always_collective):
            # the warm-up step's RCCL works sit in the process group's watchdog until it sees them complete; it
            # queries their end events, recorded on the process group's stream -- which the capture below turns
            # into a capturing stream, where such a query fails (hipErrorCapturedEvent) and takes the watchdog
            # down.  By construction: block until the watchdog has retired every pending work (collectives issued
            # during the capture are never handed to it), and capture in thread-local mode so that a query from
            # the watchdog's thread cannot invalidate the capture either.
            _drain_watchdog(sync.group)
            mode = "thread_local"
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode=mode):
            out = self._step()
        self.graph, self.out = g, out
        self._hyper_at_capture = self._hyper()

    def __call__(self, samples, total_scores, noise=None, q=None, lmbda=None, qoffsets=None, qlevels=None):
        """one training step on (samples, total_scores); returns the step's device losses (static tensors,
        overwritten by the next call)"""
        if (noise is None) != (self.noise is None):
            raise ValueError("GraphedTrainStep: noise must be given at every call iff it was given at capture")
        self._refresh_q(q, lmbda)
        self._refresh_qmap(qoffsets, qlevels)
        if self._hyper() != self._hyper_at_capture:
            self._capture(0)
        self.samples.copy_(samples, non_blocking=True)
        self.total_scores.copy_(total_scores, non_blocking=True)
        if noise is not None:
            for dst, src in zip(self.noise, noise):
                dst.copy_(src, non_blocking=True)
        self.graph.replay()
        from .optim import bump_versions

        bump_versions(self.params)
        return self.out


class GraphedMAEStep:
    """MaskedAutoencoderViT pre-training step (models_mae.py:216-220 under autograd + an optimizer step) captured
    once into a HIP graph, replayed per batch: zero_grad, forward (masking noise from torch's graph-safe generator,
    or a static noise tensor refreshed per call), masked-MSE loss, the HIP backward (mae_train.py) and the FusedAdam
    update.  Same capture rules as GraphedTrainStep (device step counts, pinned launch tables, persistent gradient
    buffer); a changed learning rate re-captures.  Returns the step's loss (a static device tensor)."""

    def __init__(self, model, optimizer, imgs, mask_ratio=0.75, warmup=1, noise=None):
        if not imgs.is_cuda:
            raise ValueError("GraphedMAEStep needs device inputs")
        self.model, self.optimizer, self.mask_ratio = model, optimizer, mask_ratio
        self.imgs = imgs.detach().float().clone()
        self.noise = noise.detach().float().clone() if noise is not None else None
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.graph, self.loss = None, None
        self._capture(warmup)

    def _hyper(self):
        return tuple((g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) for g in self.optimizer.param_groups)

    def _step(self):
        self.optimizer.zero_grad()
        loss, _, _ = self.model(self.imgs, self.mask_ratio, noise=self.noise)
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    def _capture(self, warmup):
        from .optim import bump_versions, reserve_capture_staging

        self.graph, self.loss = None, None
        cur = torch.cuda.current_stream(self.imgs.device)
        side = torch.cuda.Stream(device=self.imgs.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._step()
        cur.wait_stream(side)
        self.optimizer.zero_grad()
        bump_versions(self.params)
        self._staging = reserve_capture_staging()  # the graph's copy nodes read it at every replay
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            loss = self._step()
        self.graph, self.loss = g, loss
        self._hyper_at_capture = self._hyper()

    def __call__(self, imgs, noise=None):
        if (noise is None) != (self.noise is None):
            raise ValueError("GraphedMAEStep: noise must be given at every call iff it was given at capture")
        if self._hyper() != self._hyper_at_capture:
            self._capture(0)
        self.imgs.copy_(imgs, non_blocking=True)
        if noise is not None:
            self.noise.copy_(noise, non_blocking=True)
        self.graph.replay()
        from .optim import bump_versions

        bump_versions(self.params)
        return self.loss


def q_schedule(q_range, q_seed, epoch):
    """the seeded host generator train_one_epoch draws its per-step ladder positions from: next(gen) is uniform over
    q_range = (lo, hi), both ends included; the same (q_seed, epoch) gives the same sequence"""
    from .bitstream import check_q

    lo, hi = (check_q(v, f"q_range[{i}]") for i, v in enumerate(q_range))
    if lo > hi:
        raise ValueError(f"q_range = {tuple(q_range)!r}: lo must not exceed hi")
    rng = np.random.default_rng([int(q_seed), int(epoch)])

    def draw():
        while True:
            yield int(rng.integers(lo, hi + 1))
    return draw()  # the checks above run at the call, not at the first draw


def train_one_epoch(model, criterion, train_dataloader, optimizer, aux_optimizer, epoch, clip_max_norm=1.0,
                    accum_iter=1, log=None, q_range=None, q_seed=0, qoffsets=None):
    """utils/engine.py:30-156 (without MetricLogger / TensorBoard); returns the per-metric averages.

    q_range = (lo, hi): every step draws one ladder position q from a host generator seeded with
    (q_seed, epoch) and runs at the y quantiser step 2^(q/8) with the criterion's weight lmbda_for_q(criterion.lmbda,
    q).  The whole batch shares the step's q: the distortion terms are batch means, so one weight per step is what the
    loss can honour (per-image q stays available through model.forward / train_step).

    qoffsets, with or without q_range: every step runs MCM.forward_qmap with this table and levels
    from the scores, the drawn q (0 without q_range) being the base position of the whole batch.  The criterion's
    weight stays lmbda_for_q(criterion.lmbda, base q): which weight suits a map of steps is not measured."""
    from .rd_loss import lmbda_for_q

    draw = q_schedule(q_range, q_seed, epoch) if q_range is not None else None
    model.train()
    device = next(model.parameters()).device
    optimizer.zero_grad()
    aux_optimizer.zero_grad()
    sums = torch.zeros(len(METRICS), dtype=torch.float64)
    n = 0
    for i, (samples, _ori_shape, total_scores) in enumerate(train_dataloader):
        samples = samples.to(device, non_blocking=True)
        total_scores = total_scores.to(device, non_blocking=True)
        q = next(draw) if draw is not None else None
        out = train_step(model, criterion, samples, total_scores, optimizer, aux_optimizer, clip_max_norm, accum_iter,
                         step_now=(i + 1) % accum_iter == 0, q=q,
                         lmbda=None if q is None else lmbda_for_q(criterion.lmbda, q), qoffsets=qoffsets)
        vals = torch.stack([out[k].detach().float().reshape(()) for k in METRICS]).cpu().double()
        reduced = distributed.all_reduce_mean_many(vals.tolist())
        sums += torch.tensor(reduced, dtype=torch.float64)
        n += 1
        if log is not None:
            log(epoch, i, dict(zip(METRICS, reduced)))
    return {k: round(float(v) / max(n, 1), 7) for k, v in zip(METRICS, sums)}


@torch.no_grad()
def val_one_epoch(epoch, val_dataloader, model, criterion, q=None, qoffsets=None):
    """utils/engine.py:159-219: eval mode, no_grad, autocast (bf16 operands on MI355X).  q: the y quantiser step the
    estimate is taken at (MCM.forward's q); qoffsets: the table of ladder offsets of an estimate at a
    step per kept patch, levels from the scores (MCM.forward's qoffsets; §3.19)"""
    model.eval()
    device = next(model.parameters()).device
    sums = torch.zeros(len(METRICS), dtype=torch.float64)
    n = 0
    for samples, _ori_shape, total_scores in val_dataloader:
        samples = samples.to(device)
        total_scores = total_scores.to(device)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            kw = {} if q is None else {"q": q}
            if qoffsets is not None:
                kw["qoffsets"] = qoffsets
            out_net = model(samples, total_scores, **kw)
            out = criterion(out_net, samples)
            out["aux_loss"] = model.aux_loss()
        sums += torch.tensor([float(out[k]) for k in METRICS], dtype=torch.float64)
        n += 1
    avg = distributed.all_reduce_mean_many((sums / max(n, 1)).tolist())
    return {k: round(v, 2) for k, v in zip(METRICS, avg)}
