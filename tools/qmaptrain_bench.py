#!/usr/bin/env python3
"""What a map of per-patch quantiser steps costs in the graphed training step and in the eval forward (DESIGN.md
§3.20), stated against the same step without q and with a per-image q (§3.18).

ViT-B, 256 x 256, K = 144, batch 64, bf16, seeded weights and inputs (the bench configuration).  Three variants, their
HIP graphs replayed in turn in one process: "plain" (no q), "q" (q mixed = (-16, -5, 0, 3, 8, 16) repeated over the
images, a device tensor) and "map" (the same q as the base position, offsets (-8, -3, 0, 5), levels from the scores:
MCM.forward_qmap).  Eval forward: one graph per variant, `--rounds` rounds of `--replays` replays each; training:
engine.GraphedTrainStep per variant on one model, `--train-rounds` rounds of `--train-steps` steps.  The figure of a
round is its wall clock around a device synchronise divided by the replays.  Prints ONE JSON line: median / min / max
over the rounds per variant.

    python tools/qmaptrain_bench.py [--out profiles/qmaptrain/step_cost.json] [--no-train]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

QMIX = (-16, -5, 0, 3, 8, 16)
OFFSETS = (-8, -3, 0, 5)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def inputs(batch, img, L, seed, device):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(batch, 3, img, img, generator=g)
    x = (x - torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
    s = torch.rand(batch, L, generator=torch.Generator().manual_seed(seed + 1))
    return x.to(device), s.to(device)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def rounds_of(fns, rounds, reps, warm):
    """fns: {variant: callable}; the variants alternate within every round -> {variant: [ms per call, per round]}"""
    t = {k: [] for k in fns}
    for r in range(warm + rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            if r >= warm:
                t[k].append((time.perf_counter() - t0) * 1e3 / reps)
    return t


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--train-rounds", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--keep", type=int, default=144)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import textmae_amd
    from textmae_amd import engine
    from textmae_amd.bitstream import offsets_row
    from textmae_amd.optim import configure_optimizers
    from textmae_amd.rd_loss import RateDistortionLoss

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = textmae_amd.MCM(img_size=args.img, num_keep_patches=args.keep).to(dev).eval()
    model.compute_dtype = torch.bfloat16
    model.distortion = "none"
    model.update(force=True)
    B, L = args.batch, model.encoder_embed.num_patches
    x, s = inputs(B, args.img, L, 1000, dev)
    q = torch.tensor([QMIX[b % len(QMIX)] for b in range(B)], dtype=torch.int32, device=dev)
    rows = torch.tensor([offsets_row(OFFSETS)] * B, dtype=torch.int32).to(dev)
    res = {"tool": "qmaptrain_bench", "batch": B, "img": args.img, "dtype": "bf16",
           "device": torch.cuda.get_device_name(0), "q": list(QMIX), "offsets": list(OFFSETS)}

    with torch.no_grad():
        fwd = {"plain": lambda: model(x, s), "q": lambda: model(x, s, q=q),
               "map": lambda: model.forward_qmap(x, s, q=q, qoffsets=OFFSETS, _rows=rows)}
        graphs = {k: capture(f) for k, f in fwd.items()}
        want = model(x, s, q=q, qoffsets=OFFSETS)["x_hat"]
        graphs["map"][0].replay()
        torch.cuda.synchronize()
        if not torch.equal(graphs["map"][1]["x_hat"], want):
            raise SystemExit("qmaptrain_bench: the captured forward at a map differs from forward(qoffsets=)")
        t = rounds_of({k: g.replay for k, (g, _) in graphs.items()}, args.rounds, args.replays, 1)
    res["forward_graph_ms_per_step"] = {k: stats(v) for k, v in t.items()}
    res["forward_rounds"] = [args.rounds, args.replays]
    del graphs

    if not args.no_train:
        model.train()
        model.distortion = "ssim+l1"
        opt, aux_opt = configure_optimizers(model, lr=1e-4, aux_lr=1e-4, fused=True)
        crit = RateDistortionLoss(lmbda=1e-2)
        kws = {"plain": {}, "q": dict(q=q, lmbda=1e-2), "map": dict(q=q, lmbda=1e-2, qoffsets=OFFSETS)}
        steps = {k: engine.GraphedTrainStep(model, crit, opt, aux_opt, x, s, clip_max_norm=1.0, warmup=1, **kw)
                 for k, kw in kws.items()}
        t = rounds_of({k: (lambda k=k: steps[k](x, s, **kws[k])) for k in steps}, args.train_rounds, args.train_steps, 1)
        res["graphed_train_ms_per_step"] = {k: stats(v) for k, v in t.items()}
        res["train_rounds"] = [args.train_rounds, args.train_steps]
        loss = float(steps["map"](x, s, **kws["map"])["loss"])
        if loss != loss:
            raise SystemExit("qmaptrain_bench: the training loss at a map is not finite")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
