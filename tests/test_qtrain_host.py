"""The quantiser ladder in training and evaluation without a GPU: rd_loss.lmbda_for_q, the f32
restatement of the forward at a step against float64, the checker of tmae_gc_bwd_q (tests/qtrain_check.py) on its own
reference (census, skip cap, a correct f32 evaluation fits, faults are rejected), the seeded q schedule and the argument
errors that need no device."""
import numpy as np
import pytest
import torch

import glue_check as gk
import qstep_check as qk
import qtrain_check as tk
from glue_check import BF16, F32, U

DTYPES = [F32, BF16]


# ------------------------------------------------------------------------------------ lmbda_for_q
def test_lmbda_for_q_ladder_pins():
    from textmae_amd import bitstream
    from textmae_amd.rd_loss import lmbda_for_q

    assert lmbda_for_q(0.01, 0) == 0.01
    # whole octaves of the ladder are exact powers of two: step 2^(q/8)
    for q, step in ((8, 2.0), (-8, 0.5), (16, 4.0), (32, 16.0), (-32, 1 / 16)):
        assert float(bitstream.qstep(q)) == step
        assert lmbda_for_q(0.01, q) == 0.01 * step ** -2.0
        assert lmbda_for_q(3.0, q, exponent=1.0) == 3.0 / step
        assert lmbda_for_q(3.0, q, exponent=0.0) == 3.0
    # in between it is the ladder's own f32 step, not 2^(q/8) in double
    for q in (-31, -3, 1, 5, 11, 27):
        d = float(bitstream.qstep(q))
        assert lmbda_for_q(0.01, q) == 0.01 * d ** -2.0
        assert lmbda_for_q(0.01, q) == pytest.approx(0.01 * 2.0 ** (-q / 4), rel=1e-6)
    vals = [lmbda_for_q(1.0, q) for q in range(-32, 33)]
    assert all(a > b for a, b in zip(vals, vals[1:]))  # a coarser step, a smaller weight on the distortion
    for bad in (33, -33, 1.5):
        with pytest.raises(ValueError, match=r"outside -32\.\.32"):
            lmbda_for_q(0.01, bad)


def test_rd_loss_lmbda_argument():
    """the per-call weight replaces self.lmbda (float or 0-d tensor), None keeps it; a vector is refused"""
    from textmae_amd.rd_loss import RateDistortionLoss

    crit = RateDistortionLoss(lmbda=0.5)
    lik = {"y": torch.full((1, 2, 2, 2), 0.5), "z": torch.full((1, 1, 1, 1), 0.25)}
    out = {"likelihoods": lik, "loss": (torch.tensor(0.2), torch.tensor(0.03), torch.tensor(0.1))}
    tgt = torch.zeros(1, 3, 4, 4)
    with pytest.raises(ValueError, match=r"lmbda must be a float or a 0-d tensor"):
        crit(out, tgt, lmbda=torch.ones(2))


# ------------------------------------------------------------------------------------ the restatement against float64
@pytest.mark.parametrize("shape", list(qk.SHAPES))
def test_restatement_against_float64(shape):
    """y_hat, s and the training likelihood of the f32 restatement against the same definition in float64: the rounded
    integer agrees wherever float64 is not within 1e-6 of a tie, y_hat and s to their roundings, the likelihood inside
    the E bound the GPU test applies; and that bound's reference is the plain float64 definition"""
    c = tk.fwd_case(shape)
    out, r = tk.fwd_reference(shape)
    import entropy_check as ek

    ys, nz = ek.gcf_slices(c, c.y).contiguous().numpy(), ek.gcf_slices(c, c.noise).contiguous().numpy()
    mu, sg = c.mu.numpy(), c.sigma.numpy()
    r64 = qk.restate64(ys, mu, sg, c.delta, c.table.numpy())
    far = np.abs(r64.t - np.floor(r64.t) - 0.5) > 1e-6
    assert far.mean() > 0.9 and np.array_equal(r.qi[far].astype(np.float64), r64.qi[far])
    # y_hat: two roundings (the product, the sum); s: one division
    err = np.abs(r.yhat.astype(np.float64) - r64.yhat)[far]
    assert float((err / (np.abs(r64.qi * c.delta) + np.abs(r64.yhat) + 1e-30)[far]).max()) <= U
    assert float(np.abs(r.s.astype(np.float64) - r64.s).max() / r64.s.max()) <= U
    # the training likelihood
    ref, bound = tk.lik_train_reference(ys, mu, sg, nz, c.delta)
    assert float((ref - tk.lik64(ys, mu, sg, nz, c.delta)).abs().max()) <= 1e-13
    l32 = tk.lik32(r.v, r.s).double()
    ratio = ((l32 - ref).abs() / bound).max()
    print(shape, "f32 restatement of the training likelihood: error / bound", float(ratio))
    assert float(ratio) <= 1.0
    floor = int((ref == 1e-9).sum())
    assert floor >= 4 and int((ref > 1e-4).sum()) >= 4, floor  # both ends of the range are there
    # eval: |qi| is what the coder's kernel takes, so the reference is qstep_check's
    e = tk.restate_fwd(ys, mu, sg, None, c.delta)
    assert np.array_equal(e.v, np.abs(r.qi)) and np.array_equal(e.yhat, r.yhat)
    assert np.array_equal(r.yhat, qk.reference(shape)[1].yhat)  # the coder tests' y_hat, bit for bit


def test_tile_cases_share_their_values():
    a, b = tk.tile_cases()
    assert (a.n, a.HW, b.n, b.HW) == (3, 96, 1, 288) and a.M == b.M
    assert torch.equal(a.y, b.y) and torch.equal(a.sigma, b.sigma) and torch.equal(a.noise, b.noise)
    assert set(a.q) == set(b.q) == {tk.TILE_Q}


# ------------------------------------------------------------------------------------ tmae_gc_bwd_q's checker
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", list(tk.GCQ_SHAPES))
def test_gcq_census_and_skip(shape, training):
    """on the reference alone: every branch class of the kernel in every image (each has its own step), sigma planted
    on both sides of bound x delta, and the skipped share under glue_check's cap.  Measured (seeds tk.GCQ_SEEDS), all
    of it in the likelihood band: small 1 / 135 (train) and 2 / 135 (eval), three_wg 5 / 528 = 0.9 % (train and eval);
    three_wg per image: likelihood clamped 24-33 blocked / 18-29 passing, sigma / delta below the bound 15-26 passing /
    6-14 blocked, t + noise 89-98 positive / 78-87 negative"""
    c = tk.gcq_case(shape)
    assert c.q == (-32, 0, 11) and c.n == 3
    _, skip, a, f = tk.gcq_bwd_reference(c, training, F32)
    share = float(skip.any.double().mean())
    census = tk.gcq_census(c, a, f)
    print(shape, "train" if training else "eval", "skipped", int(skip.any.sum()), "of", skip.any.numel(),
          dict(band=int(skip.band.sum()), sig=int(skip.sig.sum()), near0=int(skip.near0.sum())), census)
    assert share <= gk.SKIP_CAP
    for b in range(c.n):  # the planted sigmas: two below, two above the gate, none skipped
        r = slice(b * c.HW, (b + 1) * c.HW)
        sr = a.sr[r]
        for mult in tk.PLANT:
            hit = ((sr / tk.BOUND - mult).abs() < 1e-5)
            assert int(hit.sum()) >= 1 and not bool((hit & skip.any[r]).any()), (b, mult)
    need = ("lik_blocked", "lik_passes", "lik_open", "sigma_open", "sigma_passes", "sigma_blocked")
    need += ("positive", "negative") if training else ()
    for b, cen in enumerate(census):
        floor = 2 if shape == "small" else 4
        for k in need:
            if shape == "three_wg" or k in ("lik_open", "sigma_open"):
                assert cen[k] >= floor, (b, k, cen)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("variant", ["both", "lik", "gyp"])
@pytest.mark.parametrize("shape", list(tk.GCQ_SHAPES))
def test_gcq_reference_fits(shape, training, dtype, variant):
    """the E evaluation of the kernel's formula agrees with float64 autograd, and the kernel's formula in plain f32
    torch (gcq_bwd_emulate) stays inside the bound"""
    c = tk.gcq_case(shape)
    use_glik, use_gyp = variant != "gyp", variant != "lik"
    out, skip, a, f = tk.gcq_bwd_reference(c, training, dtype, use_glik, use_gyp)
    for k, fe in (("dmu", f.dmu), ("dsigma", f.dsigma)):
        d = (fe.v - out[k][0]).abs()
        assert float(d[~skip.any].max()) <= 1e-12 * (1 + float(out[k][0].abs().max())), k
    dy, dmu, ds = tk.gcq_bwd_emulate(c, training, dtype, use_glik, use_gyp)
    for k, v, dt in (("dy", dy, F32), ("dmu", dmu, dtype), ("dsigma", ds, dtype)):
        g = gk.written(v.float(), dt)
        r = gk.check(f"gcq:{k}", g, *out[k], log=False)
        assert r <= 1.0, (k, r)
    if not training:  # the eval likelihood moves neither y nor mu
        assert float(out["dmu"][0].abs().max()) == 0.0 and float(out["dmu"][1].max()) == 0.0
        sl = slice(c.yoff, c.yoff + c.sw)
        gyp = c.gyp[:, sl].double() if use_gyp else 0.0
        assert torch.equal(out["dy"][0][:, sl], c.dy0[:, sl].double() + gyp)


@pytest.mark.parametrize("mutant", tk.GCQ_MUTANTS)
def test_gcq_rejects_mutants(mutant):
    """one fault each: the scale gate tested on sigma instead of sigma / delta, dsigma without its 1 / delta, an eval
    likelihood that moves mu, the straight-through gradient also given to mu, the sign of t + noise dropped"""
    c = tk.gcq_case("three_wg")
    training = mutant != "eval_moves_mu"
    out, skip, a, f = tk.gcq_bwd_reference(c, training, F32)
    dy, dmu, ds = tk.gcq_bwd_emulate(c, training, F32, mutant=mutant)
    bad = 0
    for k, v in (("dy", dy), ("dmu", dmu), ("dsigma", ds)):
        try:
            gk.check(f"gcq:{mutant}:{k}", gk.written(v.float(), F32), *out[k], log=False)
        except AssertionError:
            bad += 1
    assert bad >= 1


# ------------------------------------------------------------------------------------ host-side arguments
def test_q_schedule_is_seeded_and_checked():
    from textmae_amd.engine import q_schedule

    a, b = q_schedule((-8, 8), 1, 0), q_schedule((-8, 8), 1, 0)
    sa = [next(a) for _ in range(64)]
    assert sa == [next(b) for _ in range(64)] and min(sa) >= -8 and max(sa) <= 8 and len(set(sa)) > 8
    other = q_schedule((-8, 8), 2, 0)
    assert sa != [next(other) for _ in range(64)]
    later = q_schedule((-8, 8), 1, 1)
    assert sa != [next(later) for _ in range(64)]
    one = q_schedule((5, 5), 0, 0)
    assert [next(one) for _ in range(4)] == [5] * 4
    with pytest.raises(ValueError, match=r"lo must not exceed hi"):
        q_schedule((3, 1), 0, 0)
    with pytest.raises(ValueError, match=r"outside -32\.\.32"):
        q_schedule((-40, 1), 0, 0)


def test_forward_q_argument_errors():
    """MCM.forward(q=) validates before it looks at the device or launches anything"""
    from textmae_amd.mcm import MCM

    assert MCM._forward_q(None, 3) is None and MCM._forward_q(0, 3) is None and MCM._forward_q([0, 0, 0], 3) is None
    assert MCM._forward_q(5, 3) == [5, 5, 5] and MCM._forward_q((-16, 0, 5), 3) == [-16, 0, 5]
    assert MCM._forward_q(torch.tensor([1, 0, 2]), 3) == [1, 0, 2]  # a host tensor is read like a list
    with pytest.raises(ValueError, match=r"2 entries of q for 3 images"):
        MCM._forward_q([1, 2], 3)
    with pytest.raises(ValueError, match=r"outside -32\.\.32"):
        MCM._forward_q(33, 3)
    with pytest.raises(ValueError, match=r"outside -32\.\.32"):
        MCM._forward_q([0, 1.5, 0], 3)


def test_train_one_epoch_checks_q_range_first():
    from textmae_amd import engine

    class Never:
        def train(self):
            raise AssertionError("the range is checked before the model is touched")

    with pytest.raises(ValueError, match=r"lo must not exceed hi"):
        engine.train_one_epoch(Never(), None, [], None, None, 0, q_range=(4, -4))
