"""MCM's staged surface on the GPU (reference MCM.py:590-712): forward_encoder, forward_decoder and the token-input
forward_loss, eval and under autograd, against references composed here from the oracle's public helpers
(oracle.mcm_oracle: block, layer_norm, linear, unpatchify, forward_loss, mcm_forward's "enc_out").

Tolerances are the project's own: f32 max|a-b| / max|b| <= 1e-3 (north_star, tests/test_gpu_mcm.py); bf16 relative
L2 < 3e-2 (test_mcm_vitb_bf16_close_to_oracle); gradients worst per-parameter maxrel <= 1e-3
(test_split_encoder_decoder_grads_f32_vs_oracle).  No element is excluded: the two ViT stages contain no rounding
step.  tmae_unpatchify is a pure permutation and is compared bitwise.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from parity_log import check  # noqa: E402

from oracle import ids as ids_oracle
from oracle import mcm_oracle as O
from oracle.mcm_oracle import MCMConfig, make_state_dict, mcm_forward

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the configurations of tests/test_gpu_mcm.py
TINY = dict(img_size=128, patch_size=16, encoder_embed_dim=64, encoder_depth=2, encoder_num_heads=2,
            decoder_embed_dim=32, decoder_depth=2, decoder_num_heads=1, latent_depth=64, hyperprior_depth=32,
            num_slices=4, num_keep_patches=16)
SMALL12 = dict(img_size=128, patch_size=16, encoder_embed_dim=128, encoder_depth=1, encoder_num_heads=2,
               decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2, latent_depth=192, hyperprior_depth=96,
               num_slices=12, num_keep_patches=16)
ENC = ("encoder_norm.", "encoder_blocks.", "encoder_embed.", "cls_token")
DEC = ("decoder_pred.", "decoder_norm.", "decoder_blocks.", "decoder_embed.", "mask_token")


def build(tmae, cfgd, seed, dtype=torch.float32):
    cfg = MCMConfig(**cfgd)
    m = tmae.MCM(**cfg.kwargs())
    full = m.state_dict()
    sd = make_state_dict(cfg, seed)
    full.update(sd)
    m.load_state_dict(full)
    m.compute_dtype = dtype
    return m.to(DEV), cfg, sd


def maxrel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------ composed references (CPU, f32)
def ref_encoder(sd, cfg, imgs, scores):
    """forward_encoder (MCM.py:590-634), the lines of mcm_forward up to "enc_out" -> (x_remain, ids_restore)"""
    p, K, D = cfg.patch_size, cfg.num_keep_patches, cfg.encoder_embed_dim
    shuf, rest = ids_oracle.ids_shuffle(scores.float().cpu().numpy(), K, 8)
    shuf, rest = torch.from_numpy(shuf), torch.from_numpy(rest)
    x = F.conv2d(imgs, sd["encoder_embed.proj.weight"], sd["encoder_embed.proj.bias"], stride=p)
    x = x.flatten(2).transpose(1, 2) + sd["encoder_pos_embed"][:, 1:, :]
    x = torch.gather(x, 1, shuf[:, :K].unsqueeze(-1).repeat(1, 1, D))
    cls = (sd["cls_token"] + sd["encoder_pos_embed"][:, :1, :]).expand(imgs.shape[0], -1, -1)
    x = torch.cat((cls, x), dim=1)
    for i in range(cfg.encoder_depth):
        x = O.block(x, sd, f"encoder_blocks.{i}.", cfg.encoder_num_heads, cfg.norm_eps)
    return O.layer_norm(x, sd, "encoder_norm.", cfg.norm_eps)[:, 1:, :], rest


def ref_decoder(sd, cfg, t, rest):
    """forward_decoder (MCM.py:636-688) with the reference's off-by-one cls: mcm_oracle.py:234-244"""
    n = t.shape[0]
    xd = O.linear(t, sd, "decoder_embed.")
    L = rest.shape[1]
    mask = sd["mask_token"].repeat(n, L + 1 - xd.shape[1], 1)
    x_ = torch.cat([xd[:, 1:, :], mask], dim=1)
    x_ = torch.gather(x_, 1, rest.unsqueeze(-1).repeat(1, 1, xd.shape[2]))
    x = torch.cat([xd[:, :1, :], x_], dim=1) + sd["decoder_pos_embed"]
    for i in range(cfg.decoder_depth):
        x = O.block(x, sd, f"decoder_blocks.{i}.", cfg.decoder_num_heads, cfg.norm_eps)
    x = O.layer_norm(x, sd, "decoder_norm.", cfg.norm_eps)
    return O.linear(x, sd, "decoder_pred.")[:, 1:, :]


def grad_sd(m):
    """the model's weights on the CPU, the trainable ones as autograd leaves"""
    train = {n for n, p in m.named_parameters() if p.requires_grad}
    return {k: v.detach().cpu().clone().requires_grad_(k in train) for k, v in m.state_dict().items()}


def worst_grad(m, sd, prefixes):
    """worst per-parameter maxrel over the parameters under `prefixes`; every other parameter must have no grad"""
    worst, name_w = 0.0, None
    for n, p in m.named_parameters():
        if n.startswith(prefixes) and p.requires_grad:
            assert p.grad is not None, n
            r = maxrel(p.grad, sd[n].grad)
            if r > worst:
                worst, name_w = r, n
        else:
            assert p.grad is None, n
    return worst, name_w


@pytest.fixture(scope="module")
def golden(golden_dir):
    f = np.load(os.path.join(golden_dir, "mcm_tiny.npz"))
    return {k: torch.from_numpy(f[k]) for k in ("imgs", "scores", "z_noise", "y_noise", "train_x_hat")}


@pytest.fixture(scope="module")
def tiny(tmae, golden):
    """TINY model (the golden fixture's weights, seed 7) + the oracle's eval forward of the golden inputs"""
    m, cfg, sd = build(tmae, TINY, 7)
    ref = mcm_forward(sd, cfg, golden["imgs"], golden["scores"], keep_intermediates=True)
    return m, cfg, sd, ref


# ------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("n,C,H,W,P", [(2, 3, 32, 32, 16), (1, 3, 48, 48, 16), (3, 3, 24, 24, 8), (2, 3, 28, 28, 14),
                                       (2, 1, 32, 32, 16)])
def test_unpatchify_kernel_bitwise(tmae, n, C, H, W, P):
    from textmae_amd import train_ops as T

    L = (H // P) * (W // P)
    t = torch.randn(n, L, P * P * C, generator=torch.Generator().manual_seed(n * 100 + P))
    td = t.to(DEV)
    img = T.unpatchify(td, torch.full((n, C, H, W), float("nan"), device=DEV), P)
    assert torch.equal(img.cpu(), O.unpatchify(t, P, C))
    back = T.patchify(img, torch.empty_like(td), P, torch.float32)
    assert torch.equal(back, td)


def test_unpatchify_indivisible_size_is_refused(tmae):
    from textmae_amd import train_ops as T

    t = torch.zeros(1, 30 * 32 * 3, device=DEV)
    img = torch.full((1, 3, 30, 32), 7.0, device=DEV)
    with pytest.raises(ValueError, match="image 30x32, patch 16"):
        T.unpatchify(t, img, 16)
    torch.cuda.synchronize()
    assert bool((img == 7.0).all())  # nothing ran


# ------------------------------------------------------------------------------ 2. forward_encoder, f32 eval
@pytest.mark.parametrize("cfgd,seed", [(TINY, 7), (SMALL12, 11)], ids=["tiny", "small12"])
def test_forward_encoder_f32_eval(tmae, golden, cfgd, seed):
    m, cfg, sd = build(tmae, cfgd, seed)
    m.eval()
    ref = mcm_forward(sd, cfg, golden["imgs"], golden["scores"], keep_intermediates=True)
    imgs, scores = golden["imgs"].to(DEV), golden["scores"].to(DEV)
    with torch.no_grad():
        x, rest = m.forward_encoder(imgs, scores)
        x2, rest2 = m.forward_encoder(imgs, scores)
    assert x.dtype == torch.float32 and tuple(x.shape) == (2, cfg.num_keep_patches, cfg.encoder_embed_dim)
    assert rest.dtype == torch.int64 and torch.equal(rest.cpu(), ref.ids_restore)
    check("maxrel:enc_x_remain", maxrel(x, ref.inter["enc_out"]), 1e-3, strict=False)
    assert x2.data_ptr() != x.data_ptr() and rest2.data_ptr() != rest.data_ptr()
    assert torch.equal(x2, x) and torch.equal(rest2, rest)
    with torch.no_grad():  # the composed reference the other tests use is the oracle's encoder
        xr, rr = ref_encoder(sd, cfg, golden["imgs"], golden["scores"])
    assert torch.equal(rr, ref.ids_restore) and maxrel(xr, ref.inter["enc_out"]) < 1e-6


# ------------------------------------------------------------------------------ 3. forward_decoder, f32 eval
@pytest.mark.parametrize("ntok", [16, 9])
def test_forward_decoder_f32_eval(tiny, ntok):
    m, cfg, sd, ref = tiny
    m.eval()
    t = torch.randn(2, ntok, cfg.encoder_embed_dim, generator=torch.Generator().manual_seed(50 + ntok))
    with torch.no_grad():
        want = ref_decoder(sd, cfg, t, ref.ids_restore)
    with torch.no_grad():
        p = m.forward_decoder(t.to(DEV), ref.ids_restore.to(DEV))
        p2 = m.forward_decoder(t.to(DEV), ref.ids_restore)  # ids on the host are moved; a fresh tensor per call
    assert p.dtype == torch.float32 and tuple(p.shape) == (2, 64, 16 * 16 * 3)
    check(f"maxrel:dec_preds_ntok{ntok}", maxrel(p, want), 1e-3, strict=False)
    assert p2.data_ptr() != p.data_ptr() and torch.equal(p2, p)


def test_forward_decoder_shape_errors(tiny):
    m, cfg, sd, ref = tiny
    rest = ref.ids_restore.to(DEV)
    with pytest.raises(ValueError, match="E=64"):
        m.forward_decoder(torch.zeros(2, 16, 48, device=DEV), rest)
    with pytest.raises(ValueError, match="L=64"):
        m.forward_decoder(torch.zeros(2, 16, 64, device=DEV), rest[:, :49].contiguous())
    with pytest.raises(ValueError, match="ntok"):
        m.forward_decoder(torch.zeros(2, 65, 64, device=DEV), rest)


# ------------------------------------------------------------------------------ 4. forward_loss on tokens
def test_forward_loss_tokens(tiny, golden):
    m, cfg, sd, ref = tiny
    m.eval()
    imgs = golden["imgs"]
    preds = O.patchify(ref.x_hat, cfg.patch_size)  # [2, 64, 768]
    with torch.no_grad():
        s3, l3, v3 = m.forward_loss(imgs.to(DEV), preds.to(DEV))
        s4, l4, v4 = m.forward_loss(imgs.to(DEV), m.unpatchify(preds.to(DEV)).contiguous())
    assert torch.equal(s3, s4) and torch.equal(l3, l4) and torch.equal(v3, v4)
    rs, rl = O.forward_loss(O.unpatchify(preds, cfg.patch_size, cfg.in_chans), imgs)
    np.testing.assert_allclose(float(s3), float(rs), rtol=1e-3)
    np.testing.assert_allclose(float(l3), float(rl), rtol=1e-3)
    with pytest.raises(ValueError, match="L=64"):
        m.forward_loss(imgs.to(DEV), preds[:, :49].contiguous().to(DEV))


# ------------------------------------------------------------------------------ 5. the staged chain under autograd
def test_staged_chain_grads_f32_vs_oracle(tmae, golden):
    """forward_encoder -> forward_decoder -> forward_loss(imgs, preds) as separate calls, (ssim + l1).backward():
    one autograd node per stage plus UnpatchifyFn / DistortionFn; batch 3 (the golden pair and a mirrored image)"""
    m, cfg, _ = build(tmae, TINY, 7)
    m.train()
    imgs = torch.cat([golden["imgs"], golden["imgs"][:1].flip(-1)])
    scores = torch.cat([golden["scores"], golden["scores"][1:].flip(-1)])
    sd = grad_sd(m)
    xr, rest_r = ref_encoder(sd, cfg, imgs, scores)
    pr = ref_decoder(sd, cfg, xr, rest_r)
    rs, rl = O.forward_loss(O.unpatchify(pr, cfg.patch_size, cfg.in_chans), imgs)
    (rs + rl).backward()

    m.zero_grad(set_to_none=True)
    x, r = m.forward_encoder(imgs.to(DEV), scores.to(DEV))
    assert x.requires_grad and not r.requires_grad and torch.equal(r.cpu(), rest_r)
    p = m.forward_decoder(x, r)
    s, l1, _ = m.forward_loss(imgs.to(DEV), p)
    (s + l1).backward()
    check("maxrel:chain_x_remain", maxrel(x, xr), 1e-3, strict=False)
    check("maxrel:chain_preds", maxrel(p, pr), 1e-3, strict=False)
    np.testing.assert_allclose(float(s.detach()), float(rs.detach()), rtol=1e-3)
    np.testing.assert_allclose(float(l1.detach()), float(rl.detach()), rtol=1e-3)
    worst, name = worst_grad(m, sd, ENC + DEC)  # also: every LIC parameter has grad None
    check("maxrel:chain_grads", worst, 1e-3, strict=False, note=name)


# ------------------------------------------------------------------------------ 6. each stage alone
def test_encoder_alone_grads(tmae, golden):
    m, cfg, _ = build(tmae, TINY, 7)
    m.train()
    imgs, scores = golden["imgs"], golden["scores"]
    sd = grad_sd(m)
    xr, _ = ref_encoder(sd, cfg, imgs, scores)
    R = torch.randn(xr.shape, generator=torch.Generator().manual_seed(61))
    (xr * R).sum().backward()
    m.zero_grad(set_to_none=True)
    x, _ = m.forward_encoder(imgs.to(DEV), scores.to(DEV))
    (x * R.to(DEV)).sum().backward()
    worst, name = worst_grad(m, sd, ENC)
    check("maxrel:enc_alone_grads", worst, 1e-3, strict=False, note=name)


def test_decoder_alone_grads(tiny):
    m, cfg, _, ref = tiny
    m.train()
    sd = grad_sd(m)
    x_o = torch.randn(2, 16, cfg.encoder_embed_dim, generator=torch.Generator().manual_seed(62)).requires_grad_(True)
    pr = ref_decoder(sd, cfg, x_o, ref.ids_restore)
    R = torch.randn(pr.shape, generator=torch.Generator().manual_seed(63))
    (pr * R).sum().backward()
    m.zero_grad(set_to_none=True)
    x = x_o.detach().to(DEV).requires_grad_(True)
    p = m.forward_decoder(x, ref.ids_restore.to(DEV))
    check("maxrel:dec_alone_preds", maxrel(p, pr), 1e-3, strict=False)
    (p * R.to(DEV)).sum().backward()
    assert x.grad.dtype == torch.float32
    check("maxrel:dec_alone_dx", maxrel(x.grad, x_o.grad), 1e-3, strict=False)
    worst, name = worst_grad(m, sd, DEC)
    check("maxrel:dec_alone_grads", worst, 1e-3, strict=False, note=name)
    m.zero_grad(set_to_none=True)
    with torch.no_grad():  # no grad mode: the eval executor, whatever x_remain asks for
        assert not m.forward_decoder(x, ref.ids_restore.to(DEV)).requires_grad
    with pytest.raises(ValueError, match="num_keep_patches"):
        m.forward_decoder(x[:, :9].detach().requires_grad_(True), ref.ids_restore.to(DEV))


def test_stage_forward_twice_before_backward_is_refused(tiny, golden):
    m, cfg, _, ref = tiny
    m.train()
    imgs, scores = golden["imgs"].to(DEV), golden["scores"].to(DEV)
    m.zero_grad(set_to_none=True)
    x1, r1 = m.forward_encoder(imgs, scores)
    x2, _ = m.forward_encoder(imgs, scores)
    with pytest.raises(RuntimeError, match="forward_encoder"):
        x1.sum().backward()
    p1 = m.forward_decoder(x2, r1)
    p2 = m.forward_decoder(x2.detach(), r1)
    with pytest.raises(RuntimeError, match="forward_decoder"):
        p1.sum().backward()
    p2.sum().backward()  # the latest forward of each stage still backs up
    x2.sum().backward()
    # a whole forward replaces both stages' activations
    x3, r3 = m.forward_encoder(imgs, scores)
    noise = (golden["z_noise"].to(DEV), golden["y_noise"].to(DEV))
    m(imgs, scores, noise=noise)
    with pytest.raises(RuntimeError, match="forward_encoder"):
        x3.sum().backward()
    m.zero_grad(set_to_none=True)


def test_full_training_forward_intact_after_staged_step(tmae, golden):
    """the staged nodes share the training executor with forward(): after a staged step the whole training forward
    still reproduces the reference's golden output"""
    m, cfg, _ = build(tmae, TINY, 7)
    m.train()
    imgs, scores = golden["imgs"].to(DEV), golden["scores"].to(DEV)
    x, r = m.forward_encoder(imgs, scores)
    p = m.forward_decoder(x, r)
    s, l1, _ = m.forward_loss(imgs, p)
    (s + l1).backward()
    m.zero_grad(set_to_none=True)
    out = m(imgs, scores, noise=(golden["z_noise"].to(DEV), golden["y_noise"].to(DEV)))
    assert out["x_hat"].requires_grad
    check("maxrel:train_x_hat_after_staged", maxrel(out["x_hat"], golden["train_x_hat"]), 1e-3, strict=False)


def test_staged_methods_refuse_grad_sync(tiny, golden):
    m, cfg, _, ref = tiny
    m.train()
    m.grad_sync = object()
    try:
        with pytest.raises(RuntimeError, match="forward\\(\\) only"):
            m.forward_encoder(golden["imgs"].to(DEV), golden["scores"].to(DEV))
        with pytest.raises(RuntimeError, match="forward\\(\\) only"):
            m.forward_decoder(torch.zeros(2, 16, 64, device=DEV), ref.ids_restore.to(DEV))
    finally:
        del m.grad_sync


# ------------------------------------------------------------------------------ 7. bf16 at real dimensions
def test_stages_bf16_vitb_close_to_oracle(tmae):
    """ViT-B, 256x256, K=144, batch 2: the shape at which the fused qkv_attn kernel and the LDS-DMA GEMMs run;
    only the ViT parts are composed on the CPU"""
    m, cfg, sd = build(tmae, dict(img_size=256, num_keep_patches=144), 3, torch.bfloat16)
    m.eval()
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(((rng.random((2, 3, 256, 256), dtype=np.float32) - 0.45) / 0.225).astype(np.float32))
    scores = torch.from_numpy(rng.random((2, 256), dtype=np.float32))
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with torch.no_grad():
        xr, rest_r = ref_encoder(sd, cfg, imgs, scores)
        pr = ref_decoder(sd, cfg, xr, rest_r)
    with torch.no_grad():
        x, rest = m.forward_encoder(imgs.to(DEV), scores.to(DEV))
        p = m.forward_decoder(xr.to(DEV), rest_r.to(DEV))
    assert x.dtype == torch.float32 and torch.equal(rest.cpu(), rest_r)
    check("rel_l2:enc_bf16_vitb", rel_l2(x, xr), 3e-2)
    assert p.dtype == torch.float32 and tuple(p.shape) == (2, 256, 768)
    check("rel_l2:dec_bf16_vitb", rel_l2(p, pr), 3e-2)


# ------------------------------------------------------------------------------ 8. capture
def test_stages_graph_capture(tiny, golden):
    m, cfg, _, ref = tiny
    m.eval()
    imgs, scores = golden["imgs"].to(DEV), golden["scores"].to(DEV)
    with torch.no_grad():
        ex, er = m.forward_encoder(imgs, scores)
        ep = m.forward_decoder(ex, er)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.forward_decoder(m.forward_encoder(imgs, scores)[0], er)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            x, r = m.forward_encoder(imgs, scores)
            p = m.forward_decoder(x, r)
        for _ in range(2):
            x.zero_()
            p.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(x, ex) and torch.equal(r, er) and torch.equal(p, ep)
