"""MCM training steps with seeded weights, inputs and noise, the resulting parameters (and losses) saved to a file, so
that two builds (TMAE_LIB=...) or two checkouts of the package can be compared bit for bit.  Run it from the root
of the checkout under test (the package, bench.py and tests/ are taken from the working directory):
    python tools/train_dump.py out_a.pt [batch]                 bench configuration (ViT-B, 256^2, K=144), bf16, eager
    python tools/train_dump.py out.pt --config small            SMALL of tests/test_gpu_train.py (12 slices)
    python tools/train_dump.py out.pt --config small2           SMALL with num_slices=2, latent_depth=32 (nser = S)
    ... --dtype f32                                             the f32 operand path (per-layer slice stacks)
    ... --set USE_LIC_STACK_BWD=False --set SIDE_SLOT_DIV=1     TrainExec class hooks (tools/train_ab.py's names)
    ... --graphed 3                                             GraphedTrainStep(warmup=1) + that many replays
    ... --steps 2                                               eager: that many train_steps (default 1)
    python tools/train_dump.py --compare out_a.pt out_b.pt      exit status 1 unless every tensor is equal"""
import argparse
import ast
import os
import sys

import torch

sys.path.insert(0, os.getcwd())


def compare(fa, fb):
    a, b = torch.load(fa, weights_only=True), torch.load(fb, weights_only=True)
    bad = [k for k in a if k not in b or not torch.equal(a[k], b[k])] + [k for k in b if k not in a]
    print(f"{len(a)} tensors, {len(a) - len(bad)} bitwise equal")
    for k in bad[:20]:
        same = k in a and k in b and a[k].shape == b[k].shape
        print(k, f"DIFFERS max {float((a[k] - b[k]).abs().max()):.3e}" if same else "MISSING / other shape")
    sys.exit(1 if bad else 0)


def main():
    if sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("batch", nargs="?", type=int)
    ap.add_argument("--config", choices=("bench", "small", "small2"), default="bench")
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--set", action="append", default=[], metavar="HOOK=VALUE")
    ap.add_argument("--graphed", type=int, default=0, metavar="REPLAYS")
    ap.add_argument("--steps", type=int, default=1)
    a = ap.parse_args()
    import bench
    import textmae_amd
    from textmae_amd import engine
    from textmae_amd.mcm_train import TrainExec
    from textmae_amd.optim import configure_optimizers
    from textmae_amd.rd_loss import RateDistortionLoss

    for kv in a.set:
        k, v = kv.split("=", 1)
        if not hasattr(TrainExec, k):
            raise SystemExit(f"TrainExec has no hook {k}")
        setattr(TrainExec, k, ast.literal_eval(v))
    torch.manual_seed(0)
    if a.config == "bench":
        B, img = a.batch or 16, 256
        m = textmae_amd.MCM(img_size=256, num_keep_patches=144)
    else:
        sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
        from test_gpu_train import SMALL

        cfg = dict(SMALL, num_slices=2, latent_depth=32) if a.config == "small2" else SMALL
        B, img = a.batch or 2, cfg["img_size"]
        m = textmae_amd.MCM(**cfg)
    m = m.cuda().train()
    m.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    m.distortion = "ssim+l1"
    opt, aux = configure_optimizers(m, lr=1e-4, aux_lr=1e-4, fused=True)
    crit = RateDistortionLoss(lmbda=1e-2)
    n = a.graphed + 1 if a.graphed else a.steps
    batches = [bench.synthetic_inputs(B, img, m.encoder_embed.num_patches, 2000 + s, "cuda") for s in range(n)]
    torch.manual_seed(1)
    torch.cuda.manual_seed(1)
    losses = []
    if a.graphed:  # the constructor runs one eager warm-up step on batch 0 and captures
        g = engine.GraphedTrainStep(m, crit, opt, aux, *batches[0], clip_max_norm=1.0, warmup=1)
        losses = [g(*b)["loss"].detach().float().cpu().clone() for b in batches[1:]]
    else:
        for b in batches:
            losses.append(engine.train_step(m, crit, *b, opt, aux, clip_max_norm=1.0)["loss"].detach().float().cpu())
    torch.cuda.synchronize()
    # the parameters after clipped Adam steps carry every gradient
    out = {k: v.detach().float().cpu() for k, v in m.named_parameters()}
    out["__losses__"] = torch.stack(losses) if losses else torch.zeros(0)
    torch.save(out, a.out)
    print("saved", a.out, "losses", [float(v) for v in losses])


if __name__ == "__main__":
    main()
