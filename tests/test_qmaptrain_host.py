"""Training at per-patch quantiser steps without a GPU: the checker of tmae_gc_bwd_qm
(tests/qmaptrain_check.py) on its own reference, float64 autograd of §3.18's definition with the step a function of
(image, pixel): census of the branch classes per image, the skipped share under glue_check's cap, a plain f32
evaluation inside the bound, the five faults of §3.18 and three faults of the map's indexing rejected; the model's
restatement at a constant map against qtrain_check.mcm_forward_q; the argument errors that need no device."""
import numpy as np
import pytest
import torch

import glue_check as gk
import qmap_check as mk
import qmaptrain_check as mt
import qtrain_check as tk
from glue_check import BF16, F32

DTYPES = [F32, BF16]


def test_the_map_is_indexed_by_pixel_alone():
    """the cycles' lengths 5 and 4 divide neither HW = 9 nor 16 nor sw = 5 / 11: every other way to index the step
    gives other values; image 2 holds one position"""
    assert mk.CYCLES == ((-32, 32, 0, 11, -5), (-13, 3, 26, 0), (7,))
    for shape, d in mt.GCQ_SHAPES.items():
        c = mt.gcqm_case(shape)
        assert c.qmap.shape == (3, d["HW"]) and c.delta.shape == (c.M, 1)
        for b, cyc in enumerate(mk.CYCLES):
            assert c.qmap[b].tolist() == [cyc[p % len(cyc)] for p in range(d["HW"])]
            assert len(set(c.qmap[b].tolist())) == len(cyc)
        for mutant in mt.MAP_MUTANTS:
            mt.mutant_case(c, mutant)  # asserts that the fault changes some element's step


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", list(mt.GCQ_SHAPES))
def test_gcqm_census_and_skip(shape, training):
    """on the reference alone: every branch class of §3.18 in every image, sigma planted on both sides of bound x the
    step of the element's own pixel, the skipped share under glue_check.SKIP_CAP.  Counted (seeds mt.GCQM_SEEDS), all in
    the likelihood band: small 1 / 135 (train) and 2 / 135 (eval), three_wg 6 / 528 (train) and 5 / 528 (eval)"""
    c = mt.gcqm_case(shape)
    _, skip, a, f = tk.gcq_bwd_reference(c, training, F32)
    share = float(skip.any.double().mean())
    census = tk.gcq_census(c, a, f)
    print(shape, "train" if training else "eval", "skipped", int(skip.any.sum()), "of", skip.any.numel(),
          dict(band=int(skip.band.sum()), sig=int(skip.sig.sum()), near0=int(skip.near0.sum())), census)
    assert share <= gk.SKIP_CAP
    for b in range(c.n):  # the planted sigmas: two below, two above the gate of their own pixel's step, none skipped
        r = slice(b * c.HW, (b + 1) * c.HW)
        for mult in tk.PLANT:
            hit = ((a.sr[r] / tk.BOUND - mult).abs() < 1e-5)
            assert int(hit.sum()) >= 1 and not bool((hit & skip.any[r]).any()), (b, mult)
    for k, mult in enumerate(tk.PLANT):  # and they sit on pixels of different steps in image 0
        m = (2 * k + 1) % c.HW
        assert float(c.sigma[m, (3 * k) % c.sw]) == float(torch.tensor(tk.BOUND * mult) * c.delta[m, 0])
    assert len({float(c.delta[(2 * k + 1) % c.HW, 0]) for k in range(4)}) >= 3
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
@pytest.mark.parametrize("shape", list(mt.GCQ_SHAPES))
def test_gcqm_reference_fits(shape, training, dtype, variant):
    """the E evaluation of the kernel's formula agrees with float64 autograd, and the formula in plain f32 torch
    (qtrain_check.gcq_bwd_emulate on the per-pixel delta) stays inside the bound"""
    c = mt.gcqm_case(shape)
    use_glik, use_gyp = variant != "gyp", variant != "lik"
    out, skip, a, f = tk.gcq_bwd_reference(c, training, dtype, use_glik, use_gyp)
    for k, fe in (("dmu", f.dmu), ("dsigma", f.dsigma)):
        d = (fe.v - out[k][0]).abs()
        assert float(d[~skip.any].max()) <= 1e-12 * (1 + float(out[k][0].abs().max())), k
    dy, dmu, ds = tk.gcq_bwd_emulate(c, training, dtype, use_glik, use_gyp)
    for k, v, dt in (("dy", dy, F32), ("dmu", dmu, dtype), ("dsigma", ds, dtype)):
        r = gk.check(f"gcqm:{k}", gk.written(v.float(), dt), *out[k], log=False)
        assert r <= 1.0, (k, r)
    if not training:  # the eval likelihood moves neither y nor mu
        assert float(out["dmu"][0].abs().max()) == 0.0 and float(out["dmu"][1].max()) == 0.0


@pytest.mark.parametrize("mutant", tk.GCQ_MUTANTS)
def test_gcqm_rejects_the_mutants_of_a_step(mutant):
    c = mt.gcqm_case("three_wg")
    training = mutant != "eval_moves_mu"
    out, *_ = tk.gcq_bwd_reference(c, training, F32)
    assert mt.rejected(out, *tk.gcq_bwd_emulate(c, training, F32, mutant=mutant), f"gcqm:{mutant}") >= 1


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", list(mt.GCQ_SHAPES))
@pytest.mark.parametrize("mutant", mt.MAP_MUTANTS)
def test_gcqm_rejects_the_mutants_of_the_map(mutant, shape, training):
    """the step of pixel 0 for the whole image, image 0's row for every image, the map indexed by the channel: a
    correct evaluation at the wrong step is refused in both shapes, in training and in eval"""
    c = mt.gcqm_case(shape)
    out, *_ = tk.gcq_bwd_reference(c, training, F32)
    assert mt.rejected(out, *tk.gcq_bwd_emulate(c, training, F32), "gcqm:correct") == 0
    assert mt.rejected(out, *tk.gcq_bwd_emulate(mt.mutant_case(c, mutant), training, F32), f"gcqm:{mutant}") >= 1


def test_constant_map_is_the_per_image_case():
    """a map constant over each image: the same rows, steps and reference as a per-image q"""
    c = mt.gcqm_case("three_wg", constant=tk.Q3)
    assert c.q == tk.Q3 and (c.qmap == np.array(tk.Q3)[:, None]).all()
    want = torch.tensor([float(v) for v in tk.deltas(tk.Q3)], dtype=F32).repeat_interleave(c.HW).reshape(c.M, 1)
    assert torch.equal(c.delta, want)


# ------------------------------------------------------------------------------------ the model's restatement
def test_restatement_at_a_constant_map_is_mcm_forward_q():
    """float64, test_gpu_train.SMALL's geometry at one block per stage: mcm_forward_qm with qmap[b][.] = q[b] equals
    qtrain_check.mcm_forward_q to the last bit, values and gradients; a map that varies gives other values"""
    from oracle.mcm_oracle import MCMConfig, make_state_dict

    cfg = MCMConfig(img_size=64, patch_size=16, encoder_embed_dim=64, encoder_depth=1, encoder_num_heads=2,
                    decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2, latent_depth=192, hyperprior_depth=96,
                    num_slices=12, num_keep_patches=16)
    sd = make_state_dict(cfg, 3)
    rng = np.random.default_rng(4)
    B, q = 2, (-16, 5)
    imgs = torch.from_numpy(rng.random((B, 3, 64, 64))).double()
    scores = torch.from_numpy(rng.random((B, 16), dtype=np.float32))
    zn = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 96, 1, 1)))
    yn = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 192, 4, 4)))

    def run(fn, arg):
        leaf = {k: (v.clone().double().requires_grad_(True) if k.startswith(("g_a.", "cc_transform_scale.0."))
                    else (v.double() if torch.is_floating_point(v) else v)) for k, v in sd.items()}
        r = fn(leaf, cfg, imgs, scores, zn, yn, arg)
        (r.y_lik.log().sum() + r.x_hat.sum()).backward()
        return r, {k: v.grad for k, v in leaf.items() if torch.is_tensor(v) and v.requires_grad}

    a, ga = run(tk.mcm_forward_q, q)
    b, gb = run(mt.mcm_forward_qm, np.repeat(np.array(q)[:, None], 16, axis=1))
    for k in ("x_hat", "y_lik", "z_lik", "t", "sym"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert len(ga) > 4 and all(torch.equal(ga[k], gb[k]) for k in ga)
    levels, qmap = mt.score_map(cfg, scores, q, (-8, -3, 0, 5))
    assert all(np.bincount(l, minlength=4).tolist() == [4, 4, 4, 4] for l in levels)
    c, _ = run(mt.mcm_forward_qm, qmap)
    assert not torch.equal(c.sym, a.sym) and not torch.equal(c.x_hat, a.x_hat)


# ------------------------------------------------------------------------------------ host-side arguments
def test_forward_qmap_argument_errors():
    """validated before the device is looked at"""
    from textmae_amd.mcm import MCM

    m = MCM.__new__(MCM)
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(ValueError, match=r"forward_qmap: qoffsets \(the table of ladder offsets\) is required"):
        MCM.forward_qmap(m, x, None)
    with pytest.raises(ValueError, match=r"forward_qmap: 3 entries of q for 2 images|forward: 3 entries of q"):
        MCM.forward_qmap(m, x, None, q=[1, 2, 3], qoffsets=(0, 1))


def test_train_step_checks_the_map_arguments_first():
    from textmae_amd import engine

    class Never:
        def __call__(self, *a, **k):
            raise AssertionError("the arguments are checked before the model is called")

    with pytest.raises(ValueError, match=r"train_step: qlevels without qoffsets"):
        engine.train_step(Never(), None, None, None, None, None, qlevels="scores")
