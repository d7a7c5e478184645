"""Models at 384 and 512 pixels: token sequences past what one head's K / V fit in LDS (T = 577 and 1025), which
run on the streamed attention kernels (csrc/attention_stream.hip).  Before those kernels every call here stopped at
"sequence length ... too long".

No quantiser sits in the compared paths, so no element is excluded.  Bounds are those of the same checks at 128
pixels: MCM f32 max|a-b| / max|b| <= 1e-3 for forward_decoder, its input gradient and the worst parameter gradient
(test_gpu_mcm_stages.py: test_forward_decoder_f32_eval, test_decoder_alone_grads), bf16 relative L2 < 3e-2
(test_stages_bf16_vitb_close_to_oracle); MAE f32 1e-3 on loss, pred and every gradient, bf16 gradients relative
L2 < 2e-2 (test_gpu_mae_train.py); the device coder's round trip equals the eval forward bit for bit
(test_gpu_device_coder.py)."""
from functools import partial

import pytest
import torch
from parity_log import check  # noqa: E402

from oracle.mae_oracle import mae_decoder, mae_encoder, mae_forward
from test_gpu_device_coder import build as build_coded
from test_gpu_device_coder import inputs as coder_inputs
from test_gpu_mcm_stages import DEC, TINY, build, grad_sd, maxrel, ref_decoder, rel_l2, worst_grad

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
TINY384 = dict(TINY, img_size=384)  # L = 576: the decoder runs at T = 577, one head of 32


def _streams(tmae, T, dh, dt, backward=False):
    return "stream" in tmae.ops.mha_plan(T, dh, dt, backward)


def _restore(n, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(L, generator=g) for _ in range(n)])


# ------------------------------------------------------------------------------------------------ MCM, 384 pixels
@pytest.fixture(scope="module")
def mcm384(tmae):
    m, cfg, sd = build(tmae, TINY384, 7)
    return m, cfg, sd, _restore(2, 576, 70)


def test_mcm384_forward_decoder_f32(tmae, mcm384):
    m, cfg, sd, rest = mcm384
    assert _streams(tmae, 577, 32, F32)
    m.eval()
    m.compute_dtype = F32
    t = torch.randn(2, 16, cfg.encoder_embed_dim, generator=torch.Generator().manual_seed(71))
    with torch.no_grad():
        want = ref_decoder(sd, cfg, t, rest)
        p = m.forward_decoder(t.to(DEV), rest.to(DEV))
    assert p.dtype == torch.float32 and tuple(p.shape) == (2, 576, 16 * 16 * 3)
    check("maxrel:mcm384_dec_preds", maxrel(p, want), 1e-3, strict=False)


def test_mcm384_forward_decoder_bf16(tmae, mcm384):
    m, cfg, sd, rest = mcm384
    assert _streams(tmae, 577, 32, BF16)
    m.eval()
    m.compute_dtype = BF16
    try:
        t = torch.randn(2, 16, cfg.encoder_embed_dim, generator=torch.Generator().manual_seed(72))
        with torch.no_grad():
            want = ref_decoder(sd, cfg, t, rest)
            p = m.forward_decoder(t.to(DEV), rest.to(DEV))
    finally:
        m.compute_dtype = F32
    check("rel_l2:mcm384_dec_bf16", rel_l2(p, want), 3e-2)


def test_mcm384_decoder_alone_grads_f32(tmae, mcm384):
    m, cfg, _, rest = mcm384
    assert _streams(tmae, 577, 32, F32, backward=True)
    m.train()
    m.compute_dtype = F32
    sd = grad_sd(m)
    x_o = torch.randn(2, 16, cfg.encoder_embed_dim, generator=torch.Generator().manual_seed(73)).requires_grad_(True)
    pr = ref_decoder(sd, cfg, x_o, rest)
    R = torch.randn(pr.shape, generator=torch.Generator().manual_seed(74))
    (pr * R).sum().backward()
    m.zero_grad(set_to_none=True)
    x = x_o.detach().to(DEV).requires_grad_(True)
    p = m.forward_decoder(x, rest.to(DEV))
    check("maxrel:mcm384_dec_alone_preds", maxrel(p, pr), 1e-3, strict=False)
    (p * R.to(DEV)).sum().backward()
    check("maxrel:mcm384_dec_alone_dx", maxrel(x.grad, x_o.grad), 1e-3, strict=False)
    worst, name = worst_grad(m, sd, DEC)
    check("maxrel:mcm384_dec_alone_grads", worst, 1e-3, strict=False, note=name)
    m.zero_grad(set_to_none=True)


# ------------------------------------------------------------------------------------------------ MAE, 384 pixels
def mae384(tmae):
    torch.manual_seed(81)
    return tmae.MaskedAutoencoderViT(img_size=384, patch_size=16, in_chans=3, embed_dim=64, depth=1, num_heads=1,
                                     decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=1, mlp_ratio=4.0,
                                     norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), norm_pix_loss=False).to(DEV)


def _mae_inputs(seed):
    imgs = torch.randn(2, 3, 384, 384, generator=torch.Generator().manual_seed(seed))
    noise = torch.rand(2, 576, generator=torch.Generator().manual_seed(seed + 1))
    return imgs, noise


def test_mae384_full_length_f32(tmae):
    """mask_ratio = 0: the dh 64 encoder at the full length T = 577 and the dh 32 decoder at T = 577.  With no
    patch masked the reference's loss is 0 / 0 (models_mae.py divides by mask.sum()), so the gradients are taken
    through a fixed random projection of pred instead; the loss itself is checked at mask_ratio = 1/16 below."""
    assert _streams(tmae, 577, 64, F32) and _streams(tmae, 577, 64, F32, True) and _streams(tmae, 577, 32, F32, True)
    m = mae384(tmae)
    imgs, noise = _mae_inputs(82)
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    lat_o, mask_o, rest_o = mae_encoder(sd, imgs, noise, 0.0, 16, 1, 1)
    pred_o = mae_decoder(sd, lat_o, rest_o, 1, 1)
    R = torch.randn(pred_o.shape, generator=torch.Generator().manual_seed(84))
    (pred_o * R).sum().backward()
    m.zero_grad(set_to_none=True)
    lat, mask, rest = m.forward_encoder(imgs.to(DEV), 0.0, noise=noise.to(DEV))
    assert tuple(lat.shape) == (2, 577, 64) and torch.equal(rest.cpu(), rest_o) and torch.equal(mask.cpu(), mask_o)
    pred = m.forward_decoder(lat, rest)
    (pred * R.to(DEV)).sum().backward()
    check("maxrel:mae384_full_latent", maxrel(lat.detach(), lat_o.detach()), 1e-3)
    check("maxrel:mae384_full_pred", maxrel(pred.detach(), pred_o.detach()), 1e-3)
    worst, name_w = 0.0, None
    for n, p_ in m.named_parameters():
        if not p_.requires_grad:
            assert p_.grad is None, n
            continue
        r = maxrel(p_.grad, sd[n].grad)
        if r > worst:
            worst, name_w = r, n
    check("maxrel:mae384_full_grads", worst, 1e-3, note=name_w)


def _oracle(m, imgs, noise, ratio):
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    loss, pred, mask = mae_forward(sd, imgs, noise, ratio, 16, 1, 1, 1, 1, norm_pix=False)
    loss.backward()
    return loss.detach(), pred.detach(), mask, {k: v.grad for k, v in sd.items()}


def _train(m, imgs, noise, ratio):
    m.zero_grad(set_to_none=True)
    loss, pred, mask = m(imgs.to(DEV), ratio, noise=noise.to(DEV))
    loss.backward()
    return loss.detach(), pred.detach(), mask, {n: p.grad for n, p in m.named_parameters() if p.requires_grad}


RATIO = 1.0 / 16  # 540 of 576 patches kept: the encoder at T = 541, still past every resident kernel's limit


def test_mae384_loss_and_grads_f32(tmae):
    assert _streams(tmae, 541, 64, F32) and _streams(tmae, 541, 64, F32, True)
    m = mae384(tmae)
    imgs, noise = _mae_inputs(85)
    rl, rp, rm, rg = _oracle(m, imgs, noise, RATIO)
    loss, pred, mask, grads = _train(m, imgs, noise, RATIO)
    assert torch.equal(mask.cpu(), rm)
    check("maxrel:mae384_pred", maxrel(pred, rp), 1e-3)
    assert abs(float(loss) - float(rl)) <= 1e-3 * abs(float(rl))
    worst, name_w = 0.0, None
    for name, g in grads.items():
        r = maxrel(g, rg[name])
        if r > worst:
            worst, name_w = r, name
    check("maxrel:mae384_grads", worst, 1e-3, note=name_w)


def test_mae384_bf16_step(tmae):
    assert _streams(tmae, 541, 64, BF16) and _streams(tmae, 541, 64, BF16, True) and _streams(tmae, 577, 32, BF16, True)
    m = mae384(tmae)
    m.compute_dtype = BF16
    imgs, noise = _mae_inputs(87)
    rl, rp, rm, rg = _oracle(m, imgs, noise, RATIO)
    loss, pred, mask, grads = _train(m, imgs, noise, RATIO)
    assert torch.isfinite(loss).item() and all(bool(torch.isfinite(g).all()) for g in grads.values())
    worst, name_w = 0.0, None
    for name, g in grads.items():
        ref = rg[name].double()
        r = float((g.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-30))
        if r > worst:
            worst, name_w = r, name
    check("relL2:mae384_bf16_grads", worst, 2e-2, note=name_w)


# ------------------------------------------------------------------------------------------------ MCM, 512 pixels
def test_mcm512_bf16_forward_and_round_trip(tmae):
    """L = 1024, the longest sequence tmae_ids_shuffle takes: the decoder runs at T = 1025"""
    assert _streams(tmae, 1025, 32, BF16)
    m = build_coded(tmae, dict(TINY, img_size=512, num_keep_patches=16), 7, BF16)
    imgs, scores = coder_inputs(1, 512, 1024, 90)
    with torch.no_grad():
        fwd = m(imgs.to(DEV), scores.to(DEV))["x_hat"]
        out = m.compress_batch(imgs.to(DEV), scores.to(DEV))
        rec = m.decompress_batch(out["string"], out["shape"], out["ids_restore"])["x_hat"]
    assert tuple(fwd.shape) == (1, 3, 512, 512) and bool(torch.isfinite(fwd).all())
    assert torch.equal(rec, fwd)
