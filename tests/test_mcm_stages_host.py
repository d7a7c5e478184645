"""Host-side surface of MCM's staged methods (reference MCM.py:590-712): forward_encoder / forward_decoder exist with
the reference's parameter names, forward_loss takes `preds`, CPU inputs and wrong ranks are refused before any kernel
launch, and the unpatchify entry point is declared and bound.  CPU only."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small(tmae):
    return tmae.MCM(img_size=64, encoder_embed_dim=64, encoder_depth=1, encoder_num_heads=2, decoder_embed_dim=32,
                    decoder_depth=1, decoder_num_heads=1, latent_depth=64, hyperprior_depth=32, num_slices=4,
                    num_keep_patches=16)


def params(fn):
    return [n for n in inspect.signature(fn).parameters if n != "self"]


def test_staged_methods_exist_with_reference_names(tmae):
    assert hasattr(tmae.MCM, "forward_encoder") and hasattr(tmae.MCM, "forward_decoder")
    assert params(tmae.MCM.forward_encoder) == ["imgs", "total_scores"]
    assert params(tmae.MCM.forward_decoder) == ["x_remain", "ids_restore"]
    assert params(tmae.MCM.forward_loss) == ["imgs", "preds"]


def test_staged_methods_refuse_cpu_tensors(tmae):
    m = small(tmae)
    with pytest.raises(ValueError, match="GPU"):
        m.forward_encoder(torch.zeros(1, 3, 64, 64), torch.zeros(1, 16))
    with pytest.raises(ValueError, match="GPU"):
        m.forward_decoder(torch.zeros(1, 16, 64), torch.arange(16).view(1, 16))
    with pytest.raises(ValueError, match="GPU"):
        m.forward_loss(torch.zeros(1, 3, 64, 64), torch.zeros(1, 16, 768))


def test_forward_loss_refuses_other_ranks_and_shapes(tmae):
    m = small(tmae)
    imgs = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match=r"\[N, L=16, p\*p\*in_chans=768\].*\[N, 3, H, W\]"):
        m.forward_loss(imgs, torch.zeros(16, 768))
    with pytest.raises(ValueError, match="L=16"):
        m.forward_loss(imgs, torch.zeros(1, 9, 768))
    with pytest.raises(ValueError, match="768"):
        m.forward_loss(imgs, torch.zeros(1, 16, 256))


def test_unpatchify_declared_and_bound(tmae):
    src = open(os.path.join(ROOT, "include", "tmae.h")).read()
    assert re.search(r"^int\s+tmae_unpatchify\s*\(const float\* tokens, float\* imgs, int n, int C, int H, int W, "
                     r"int patch,\s*void\* stream\);", src, flags=re.M)
    from textmae_amd import _lib

    assert len(_lib.SIGNATURES["tmae_unpatchify"]) == 8
    assert hasattr(tmae.load_library(), "tmae_unpatchify")
    # the shape check runs on the host, before any launch
    with pytest.raises(ValueError, match="image 30x32, patch 16"):
        _lib.call("tmae_unpatchify", 16, 16, 1, 3, 30, 32, 16, None)
