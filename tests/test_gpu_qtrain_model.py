"""MCM.forward(q=) in eval and under autograd, RateDistortionLoss(lmbda=), engine.train_step / GraphedTrainStep /
train_one_epoch / val_one_epoch with a quantiser step.

Eval, test_gpu_qstep_model.py's SMALL12 (128 px, K = 16, weight seed 11, input seed 47), batch 3, q = (-16, 0, 5): what
forward(q=) estimates is what the coder does: x_hat bit for bit decompress_batch(compress_batch(q=), q=)'s, the y
likelihoods bit for bit tmae_gc_slices_code_q's on the same buffers; in bf16 the chained launches (cq) bit for bit the
unchained ones.  On the parent commit forward() takes no q: these tests fail there with TypeError.

Training, test_gpu_train.py's SMALL (64 px, weight seed 3, batch 2, injected noise), q = (-9, 6): f32 gradients of every
parameter, the loss and x_hat against float64 autograd through qtrain_check.mcm_forward_q with that file's metrics and
bounds (1e-4 on x_hat and the loss, 2e-3 on gradients); bf16 against f32 and the fused against the per-layer path at the
bounds of the tests they extend; the captured step with q and lambda buffers bit for bit eager steps."""
import numpy as np
import pytest
import torch

import qstep_check as qk
import qtrain_check as tk
from oracle.mcm_oracle import MCMConfig, make_state_dict
from parity_log import check
from test_gpu_qstep_model import SEED_W, SEED_X, SMALL12, inputs
from test_gpu_train import SMALL, _model_and_oracle, _rel, _rel2

pytestmark = pytest.mark.gpu
DEV = "cuda"
QMIX = (-16, 0, 5)
QTRAIN = (-9, 6)


# ------------------------------------------------------------------------------------------------ eval
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


@pytest.fixture(params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def dtyped(request, small):
    small.compute_dtype = request.param
    yield small
    small.compute_dtype = torch.float32


def _fwd(m, xs, **kw):
    with torch.no_grad():
        out = m(*xs, **kw)
    torch.cuda.synchronize()
    return out["x_hat"].clone(), out["likelihoods"]["y"].clone(), out["likelihoods"]["z"].clone()


def test_forward_q_is_what_the_coder_does(tmae, dtyped, xs, monkeypatch):
    """x_hat of forward(q=) is the decoded x_hat bit for bit; every launch of tmae_gc_slices_fwd_q is followed by
    tmae_gc_slices_code_q on the same operands into a second likelihood buffer: bit for bit the forward's"""
    m = dtyped
    ops = tmae.ops
    lik2, n_calls = {}, [0]
    real = ops.gc_slices_fwd_q

    def both(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, noise, lik, Mtot, yhat, yt, ld_yhat, yhat32, ld32, n, HW, nsl, sw,
             bound, q):
        real(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, noise, lik, Mtot, yhat, yt, ld_yhat, yhat32, ld32, n, HW, nsl, sw,
             bound, q)
        assert noise is None
        if "lik" not in lik2:
            lik2["lik"] = torch.full((n, Mtot, HW), float("nan"), device=DEV)
            lik2["yh"] = torch.full((n * HW, Mtot), float("nan"), device=DEV)
        sym = torch.empty(nsl * n * sw * HW, dtype=torch.int32, device=DEV)
        ops.gc_slices_code_q(y, ldy, yoff, mu, sigma, ms_stride, ld_ms, lik2["lik"], Mtot, None, yt, ld_yhat, lik2["yh"],
                             Mtot, n, HW, nsl, sw, sym, torch.empty_like(sym), m.gaussian_conditional.scale_table, bound, q)
        n_calls[0] += 1

    monkeypatch.setattr(ops, "gc_slices_fwd_q", both)
    x, ylik, _ = _fwd(m, xs, q=QMIX)
    monkeypatch.undo()
    assert n_calls[0] >= 1 and m._exec.dtype == m.compute_dtype
    assert torch.equal(ylik.reshape(lik2["lik"].shape).view(torch.int32), lik2["lik"].view(torch.int32))
    out = m.compress_batch(*xs, q=QMIX)
    rec = m.decompress_batch(out["string"], out["shape"], out["ids_restore"], q=QMIX)["x_hat"]
    assert torch.equal(x, rec)
    assert not torch.equal(x, _fwd(m, xs)[0])  # and the step changes it


def test_chain_on_and_off_bitwise(tmae, small, xs):
    """bf16: the chained serial slices (tmae_lic_stack with cq) against the unchained launches"""
    from textmae_amd.mcm import _Executor

    small.compute_dtype = torch.bfloat16
    try:
        a = _fwd(small, xs, q=QMIX)
        assert small._exec.lstk is not None and _Executor.USE_LIC_CHAIN
        _Executor.USE_LIC_CHAIN = False
        try:
            b = _fwd(small, xs, q=QMIX)
        finally:
            _Executor.USE_LIC_CHAIN = True
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    finally:
        small.compute_dtype = torch.float32


def test_q_zero_is_forward(dtyped, xs):
    want = _fwd(dtyped, xs)
    for q in (0, None, [0, 0, 0], np.zeros(3, dtype=np.int64)):
        got = _fwd(dtyped, xs, q=q)
        for u, v in zip(got, want):
            assert torch.equal(u, v), q


def test_device_q_gives_the_lists_bits(dtyped, xs):
    want = _fwd(dtyped, xs, q=list(QMIX))
    got = _fwd(dtyped, xs, q=torch.tensor(QMIX, dtype=torch.int32, device=DEV))
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    # a device tensor always takes the kernels with a step: at zero y_hat, hence x_hat, is still the plain forward's
    zero = _fwd(dtyped, xs, q=torch.zeros(3, dtype=torch.int32, device=DEV))
    assert torch.equal(zero[0], _fwd(dtyped, xs)[0])
    with pytest.raises(ValueError, match=r"a device q must be a contiguous int32 \[3\] tensor"):
        dtyped(*xs, q=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match=r"a device q must be a contiguous int32 \[3\] tensor"):
        dtyped(*xs, q=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match=r"outside -32\.\.32"):
        dtyped(*xs, q=40)


def test_rate_falls_along_the_ladder(small, xs):
    bits = []
    for q in (-16, 0, 16):
        _, ylik, zlik = _fwd(small, xs, q=q)
        bits.append((-torch.log2(ylik.double())).sum(dim=(1, 2, 3)).cpu())
        assert torch.equal(zlik, _fwd(small, xs)[2])  # there is no z step
    assert bool((bits[0] > bits[1]).all()) and bool((bits[1] > bits[2]).all()), bits


def test_estimate_path_of_testing_takes_q(tmae, small, xs, monkeypatch):
    """testing.py --q on the estimated-rate path (inference_entropy_estimation -> forward(q=)), and val_one_epoch(q=).
    MS-SSIM needs sides above 160 pixels and is not what is tested: the 128-pixel model's metrics are stubbed"""
    from textmae_amd import engine, testing
    from textmae_amd.rd_loss import RateDistortionLoss

    monkeypatch.setattr(testing, "compute_metrics", lambda org, rec, max_val=255: {"psnr": 0.0, "ms-ssim": 0.0})
    imgs, scores = xs
    x01 = imgs[:1].clamp(0, 1)
    r = {q: testing.inference_entropy_estimation(small, x01, scores[:1], q=q) for q in (-8, None, 8)}
    assert r[-8]["bpp"] > r[None]["bpp"] > r[8]["bpp"]
    assert r[None]["bpp"] == testing.inference_entropy_estimation(small, x01, scores[:1])["bpp"]
    ev = testing.eval_model(small, None, [(x01, (128, 128))], scores[:1], entropy_estimation=True, q=8)
    assert ev["bpp"] == r[8]["bpp"]
    was = small.distortion
    small.distortion = "none"
    try:
        loader = [(imgs, None, scores)]
        v = {q: engine.val_one_epoch(0, loader, small, RateDistortionLoss(1e-2), q=q)["bpp_loss"] for q in (-16, None, 16)}
    finally:
        small.distortion = was
        small.compute_dtype = torch.float32
    assert v[-16] > v[None] > v[16], v


# ------------------------------------------------------------------------------------------------ training
def _hip_grads_q(m, imgs, scores, zn, yn, R, q):
    from textmae_amd.rd_loss import RateDistortionLoss

    m.zero_grad(set_to_none=True)
    out = m(imgs.cuda(), scores.cuda(), noise=(zn.cuda(), yn.cuda()), q=q)
    crit = RateDistortionLoss(lmbda=1e-2)
    loss = crit(out, imgs.cuda())["bpp_loss"] + (out["x_hat"] * R.cuda()).sum()
    loss.backward()
    aux = m.aux_loss()
    aux.backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.requires_grad}, out, loss, aux


def _oracle_grads_q(cfg, sd, imgs, scores, zn, yn, R, q):
    from oracle.train_oracle import aux_loss, rate_bpp

    leaf = {k: (v.clone().double().requires_grad_(True) if torch.is_floating_point(v) and not k.endswith("pos_embed")
                and k != "entropy_bottleneck.target" else (v.double() if torch.is_floating_point(v) else v))
            for k, v in sd.items()}
    r = tk.mcm_forward_q(leaf, cfg, imgs.double(), scores, zn.double(), yn.double(), q)
    n, _, H, W = imgs.shape
    loss = rate_bpp(r.y_lik, r.z_lik, n * H * W) + (r.x_hat * R.double()).sum()
    loss.backward()
    aux = aux_loss(leaf, "entropy_bottleneck.")
    aux.backward()
    grads = {k: v.grad for k, v in leaf.items() if isinstance(v, torch.Tensor) and v.requires_grad}
    return grads, r, loss, aux


def test_train_grads_f32_vs_float64_at_a_step():
    """every parameter's gradient, the loss and x_hat against float64 autograd of the restatement.  The reference has
    no (y - mu) / delta within 1e-4 of a half-integer (asserted first, on the reference alone), so f32 rounds every
    symbol as float64 does.  At these seeded weights nearly every sigma / delta is below the bound (the scale gate
    closed); tmae_gc_bwd_q's kernel test covers the open side"""
    m, cfg, sd, imgs, scores, zn, yn, R = _model_and_oracle(SMALL, 3, 2, torch.float32)
    ref, r, loss_ref, aux_ref = _oracle_grads_q(cfg, sd, imgs, scores, zn, yn, R, QTRAIN)
    assert qk.near_ties(r.t) == 0
    print(f"reference: {r.t.numel()} symbols, {int((r.sym != 0).sum())} non-zero, scale gate open at {int(r.gate.sum())}")
    assert int((r.sym != 0).sum()) > 100
    hip, out, loss, aux = _hip_grads_q(m, imgs, scores, zn, yn, R, list(QTRAIN))
    check("_rel:qtrain_x_hat", _rel(out["x_hat"], r.x_hat), 1e-4)
    assert abs(loss.item() - loss_ref.item()) < 1e-4 * max(1.0, abs(loss_ref.item()))
    assert abs(aux.item() - aux_ref.item()) < 1e-4 * abs(aux_ref.item())
    bad, worst = [], 0.0
    for name, g in hip.items():
        rg = ref[name].float()
        if rg.abs().max() == 0:
            if g.abs().max() > 1e-6:
                bad.append((name, "nonzero", g.abs().max().item()))
            continue
        e = _rel(g, rg)
        worst = max(worst, e)
        if e > 2e-3:
            bad.append((name, e))
    check("grad_maxrel_worst_tensor_qtrain_f32", worst, 2e-3, strict=False, tensors=len(hip))
    assert not bad, bad[:20]
    # the step is in the gradients: the same model without q gives other ones
    plain, *_ = _hip_grads_q(m, imgs, scores, zn, yn, R, None)
    assert _rel2(torch.cat([plain[k].reshape(-1) for k in hip]), torch.cat([hip[k].reshape(-1) for k in hip])) > 1e-2


def test_train_bf16_close_to_f32_at_a_step():
    """test_gpu_train.test_mcm_train_bf16_close_to_f32's metric and bound at q = (-9, 6), on this file's model (weight
    seed 3).  Measured on an MI355X: 1.64e-3 (that test, at q = 0: 1.61e-3 on its weight seed 4, 0.97e-3 on seed 3).
    What the figure measures at a fine step is mostly how many symbols the bf16 forward rounds the other way: a bf16
    error in mu is a larger share of a step of 0.46 than of a step of 1.  On this input bf16 rounds 10 of image 0's 3072
    symbols differently from f32 (2 at q = 0, 1 at q = 6); on weight seed 4 the 5 symbols it rounds differently at
    q = -9 put the same metric at 5.9e-3 (q = (-9, -9): 6.1e-3, q = 6: 1.1e-3, q = -16: 3.0e-3), while a device q of zeros
    through the same kernels gives 1.614e-3 against 1.611e-3 without q.  The f32 path is held to float64 above."""
    m, cfg, sd, imgs, scores, zn, yn, R = _model_and_oracle(SMALL, 3, 2, torch.float32)
    g32, *_ = _hip_grads_q(m, imgs, scores, zn, yn, R, list(QTRAIN))
    m.compute_dtype = torch.bfloat16
    g16, *_ = _hip_grads_q(m, imgs, scores, zn, yn, R, list(QTRAIN))
    assert m._train_exec._fused_ok()
    flat32 = torch.cat([g32[k].reshape(-1) for k in g32])
    flat16 = torch.cat([g16[k].reshape(-1) for k in g32])
    assert torch.isfinite(flat16).all()
    check("_rel2:qtrain_flat16", _rel2(flat16, flat32), 3e-3)


def test_train_fused_vs_per_layer_at_a_step():
    """test_gpu_train.test_train_fused_stacks_vs_per_layer (small) at q = (-9, 6): the chained launches with cq and
    the batched stacks against the per-layer conv launches, the same bounds"""
    from textmae_amd.mcm_train import TrainExec

    m, cfg, sd, imgs, scores, zn, yn, R = _model_and_oracle(SMALL, 3, 2, torch.bfloat16)
    res = {}
    for fused in (True, False):
        TrainExec.USE_LIC_STACK = fused
        try:
            m._train_exec = None
            g, out, loss, aux = _hip_grads_q(m, imgs, scores, zn, yn, R, list(QTRAIN))
            assert m._train_exec._fused_ok() == fused
        finally:
            TrainExec.USE_LIC_STACK = True
        res[fused] = (g, out["x_hat"].float().cpu(), out["likelihoods"]["y"].float().cpu())
    (ga, xa, ya), (gb, xb, yb) = res[True], res[False]
    check("_rel2:qtrain_fused_x_hat", _rel2(xa, xb), 2e-2)
    check("_rel2:qtrain_fused_ylik", _rel2(ya, yb), 2e-2)
    fa = torch.cat([ga[k].reshape(-1) for k in ga])
    fb = torch.cat([gb[k].reshape(-1) for k in ga])
    assert torch.isfinite(fa).all()
    check("_rel2:qtrain_fused_grads", _rel2(fa, fb), 3e-2)


def _qdev(q):
    return torch.tensor(q, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_graphed_step_with_q_and_lambda_buffers(dt):
    """one capture, replays at a different q and lambda each (one of them q = (0, 0)): losses and weights bit for bit
    those of eager engine.train_step calls with the same q (a device tensor, so the kernels with a step run at zero
    too), lambda and noise"""
    from test_gpu_optim_dp import _inputs, _model
    from textmae_amd import engine
    from textmae_amd.optim import configure_optimizers
    from textmae_amd.rd_loss import RateDistortionLoss, lmbda_for_q

    crit = RateDistortionLoss(lmbda=1e-2)
    m1, cfg = _model(SMALL, 3, dt)
    m2, _ = _model(SMALL, 3, dt)
    m1.distortion = m2.distortion = "ssim+l1"
    batches = [_inputs(cfg, 2, 300 + i) for i in range(4)]
    qs = [(-9, 6), (4, 4), (0, 0), (12, -5)]
    lms = [lmbda_for_q(1e-2, q[0]) for q in qs]
    o1 = configure_optimizers(m1, lr=3e-3, aux_lr=1e-3, fused=True)
    o2 = configure_optimizers(m2, lr=3e-3, aux_lr=1e-3, fused=True)
    cu = lambda b: tuple(t.cuda() for t in b)  # noqa: E731
    imgs, scores, zn, yn = cu(batches[0])
    g = engine.GraphedTrainStep(m1, crit, *o1, imgs, scores, clip_max_norm=1.0, warmup=1, noise=(zn, yn), q=qs[0],
                                lmbda=lms[0])
    la = []
    for b, q, lm in zip(batches[1:], qs[1:], lms[1:]):
        imgs, scores, zn, yn = cu(b)
        la.append(float(g(imgs, scores, noise=(zn, yn), q=list(q), lmbda=lm)["loss"]))
    lb = []
    for b, q, lm in zip(batches, qs, lms):
        imgs, scores, zn, yn = cu(b)
        out = engine.train_step(m2, crit, imgs, scores, *o2, clip_max_norm=1.0, noise=(zn, yn), q=_qdev(q),
                                lmbda=torch.tensor(lm, dtype=torch.float32, device=DEV))
        lb.append(float(out["loss"].detach()))
    torch.cuda.synchronize()
    assert la == lb[1:], (la, lb)
    assert all(np.isfinite(la))
    for (n, p), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, p2), n
    # the rule of the noise argument
    imgs, scores, zn, yn = cu(batches[0])
    with pytest.raises(ValueError, match=r"q must be given at every call iff it was given at capture"):
        g(imgs, scores, noise=(zn, yn), lmbda=lms[0])
    with pytest.raises(ValueError, match=r"lmbda must be given at every call iff it was given at capture"):
        g(imgs, scores, noise=(zn, yn), q=0)


def test_graphed_step_without_q_refuses_one():
    from test_gpu_optim_dp import _inputs, _model
    from textmae_amd import engine
    from textmae_amd.optim import configure_optimizers
    from textmae_amd.rd_loss import RateDistortionLoss

    m, cfg = _model(SMALL, 3, torch.bfloat16)
    m.distortion = "ssim+l1"
    opt = configure_optimizers(m, lr=3e-3, aux_lr=1e-3, fused=True)
    imgs, scores, zn, yn = (t.cuda() for t in _inputs(cfg, 2, 300))
    g = engine.GraphedTrainStep(m, RateDistortionLoss(1e-2), *opt, imgs, scores, warmup=1, noise=(zn, yn))
    with pytest.raises(ValueError, match=r"q must be given at every call iff it was given at capture"):
        g(imgs, scores, noise=(zn, yn), q=3)
    with pytest.raises(ValueError, match=r"lmbda must be given at every call iff it was given at capture"):
        g(imgs, scores, noise=(zn, yn), lmbda=0.1)


def test_train_one_epoch_draws_a_seeded_q_per_step():
    """q_range = (-8, 8), q_seed = 1 on a two-batch loader: the forward sees engine.q_schedule's draws, one q for the
    whole batch, the same sequence in a second run, and the losses are finite"""
    from test_gpu_optim_dp import _inputs, _model
    from textmae_amd import engine
    from textmae_amd.optim import configure_optimizers
    from textmae_amd.rd_loss import RateDistortionLoss, lmbda_for_q

    runs = []
    for _ in range(2):
        m, cfg = _model(SMALL, 3, torch.bfloat16)
        m.distortion = "ssim+l1"
        opt = configure_optimizers(m, lr=1e-3, aux_lr=1e-3, fused=True)
        loader = [(b[0], None, b[1]) for b in (_inputs(cfg, 2, 500 + i) for i in range(2))]
        seen, lam = [], []
        crit = RateDistortionLoss(1e-2)
        real = crit.forward
        crit.forward = lambda o, t, lmbda=None: (lam.append(lmbda), real(o, t, lmbda))[1]
        h = m.register_forward_pre_hook(lambda mod, args, kwargs: seen.append(kwargs.get("q")), with_kwargs=True)
        torch.manual_seed(5)  # the quantisation noise
        res = engine.train_one_epoch(m, crit, loader, *opt, epoch=3, q_range=(-8, 8), q_seed=1)
        h.remove()
        assert all(np.isfinite(v) for v in res.values()), res
        runs.append((seen, lam, res))
    draw = engine.q_schedule((-8, 8), 1, 3)
    want = [next(draw) for _ in range(2)]
    assert runs[0][0] == want and runs[1][0] == want
    assert runs[0][1] == [lmbda_for_q(1e-2, q) for q in want]
    assert runs[0][2] == runs[1][2]
