"""RateDistortionLoss — counterpart of reference models/Compression/loss/rd_loss.py:7-28.

Same constructor (`lmbda`), same output keys ("bpp_loss", "ssim_loss", "L1_loss", "vgg_loss", "loss")
and the same formula: loss = lmbda * (0.25*ssim + 10*L1 + 0.1*vgg) + bpp.  The bpp reduction over
both likelihood tensors runs on the device (tmae_bpp_sum).
"""
import torch
import torch.nn as nn

from . import ops


def lmbda_for_q(lmbda, q, exponent=2.0):
    """the rate-distortion weight to train with at ladder position q: lmbda * step(q)^(-exponent),
    step(q) = bitstream.qstep(q) = 2^(q/8), so that lmbda is the weight at q = 0 and a coarser step asks for less
    distortion weight.  The default exponent 2 is the high-rate rule for an MSE distortion (D grows like step^2, so the
    slope dD/dR does too); the distortion here is 0.25 (1 - SSIM) + 10 L1 + 0.1 VGG, and which exponent suits it has not
    been measured."""
    from .bitstream import check_q, qstep

    return float(lmbda) * float(qstep(check_q(q, "lmbda_for_q: q"))) ** (-float(exponent))


class RateDistortionLoss(nn.Module):
    def __init__(self, lmbda=1e-2):
        super().__init__()
        self.lmbda = lmbda

    def forward(self, output, target, lmbda=None):
        """lmbda: a float or a 0-d tensor that replaces self.lmbda for this call (lmbda_for_q; a device tensor keeps
        a captured training step capturable and lets its value change between replays)"""
        if lmbda is None:
            lmbda = self.lmbda
        elif torch.is_tensor(lmbda) and lmbda.dim() != 0:
            raise ValueError(f"RateDistortionLoss: lmbda must be a float or a 0-d tensor, got shape {tuple(lmbda.shape)}")
        N, _, H, W = target.size()
        out = {}
        lik = output["likelihoods"]
        if torch.is_grad_enabled() and (lik["y"].requires_grad or lik["z"].requires_grad):
            from .mcm_train import BppFn

            out["bpp_loss"] = BppFn.apply(lik["y"], lik["z"], N * H * W)
        else:
            out["bpp_loss"] = ops.bpp(lik["y"], lik["z"], N * H * W)
        out["ssim_loss"] = output["loss"][0]
        out["L1_loss"] = output["loss"][1]
        out["vgg_loss"] = output["loss"][2]
        out["loss"] = lmbda * (0.25 * out["ssim_loss"] + 10 * out["L1_loss"] + 0.1 * out["vgg_loss"]) \
            + out["bpp_loss"]
        return out
