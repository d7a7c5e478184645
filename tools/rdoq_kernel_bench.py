#!/usr/bin/env python3
"""Time tmae_gc_slices_code_rdo against tmae_gc_slices_code_q on the same buffers, with DENSE non-zero symbols: the
benched model's seeded weights give almost only zero symbols, for which the decision of DESIGN.md §3.21 is never
taken, so its cost does not show there.  One slice step of the benched shape (64 images, 12 x 12 latent grid, 6 slices
of 16 channels: the batched later slices), y - mu ~ 3 N(0, 1) steps, sigma / step uniform in [0.05, 2.6], step 1.
Three columns alternate in one process (the _q kernel, the _rdo kernel at w = 0, and at w = 0.5), each timed with
device events over --iters launches per round.  Prints ONE JSON line.

    python tools/rdoq_kernel_bench.py [--rounds 10] [--iters 50] [--out profiles/rdoq/kernel_cost.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from textmae_amd import ops
    from textmae_amd.entropy import GaussianConditional, get_scale_table

    dev = torch.device("cuda:0")
    n, HW, nsl, sw = 64, 144, 6, 16
    M, C = n * HW, nsl * sw
    g = torch.Generator().manual_seed(5)
    mu = torch.randn(nsl, M, sw, generator=g)
    sigma = 0.05 + 2.55 * torch.rand(nsl, M, sw, generator=g)
    y = (mu + 3 * torch.randn(nsl, M, sw, generator=g)).permute(1, 0, 2).reshape(M, C).contiguous()
    y, mu, sigma = y.to(dev), mu.contiguous().to(dev), sigma.contiguous().to(dev)
    gc = GaussianConditional(None).to(dev)
    gc.update_scale_table(get_scale_table())
    _, sizes, offsets = gc.device_tables(dev)
    rate = gc.device_rate_table(dev)
    yhat = torch.empty(M, C, dtype=torch.bfloat16, device=dev)
    yhat32 = torch.empty(M, C, dtype=torch.float32, device=dev)
    sym = torch.empty(nsl * M * sw, dtype=torch.int32, device=dev)
    idx = torch.empty_like(sym)
    changed = torch.zeros(n, dtype=torch.int32, device=dev)
    w0 = torch.zeros(n, dtype=torch.float32, device=dev)
    w1 = torch.full((n,), 0.5, dtype=torch.float32, device=dev)
    head = (y, C, 0, mu, sigma, M * sw, sw, None, C, yhat, torch.bfloat16, C, yhat32, C, n, HW, nsl, sw, sym, idx,
            gc.scale_table, 0.11)
    cols = {"code_q": lambda: ops.gc_slices_code_q(*head, None),
            "code_rdo_w0": lambda: ops.gc_slices_code_rdo(*head, None, None, w0, rate, sizes, offsets, changed),
            "code_rdo_w0.5": lambda: ops.gc_slices_code_rdo(*head, None, None, w1, rate, sizes, offsets, changed)}
    t = {c: [] for c in cols}
    moved = {}
    for r in range(3 + args.rounds):
        for c, fn in cols.items():
            changed.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r >= 3:
                t[c].append(a.elapsed_time(b) * 1e3 / args.iters)
            moved[c] = int(changed.sum()) // args.iters
    res = {"tool": "rdoq_kernel_bench", "device": torch.cuda.get_device_name(0),
           "shape": f"n {n}, HW {HW}, {nsl} slices of {sw} channels, bf16 y_hat, step 1, LDS form",
           "rounds": args.rounds, "iters": args.iters, "nonzero_symbols": int((sym != 0).sum()), "elements": sym.numel(),
           "moved_at_w0.5": moved["code_rdo_w0.5"]}
    for c, v in t.items():
        res[c + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
