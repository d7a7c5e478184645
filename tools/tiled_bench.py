#!/usr/bin/env python3
"""Time the tiled full-resolution codec: MCM.encode_image / decode_image of a seeded 768 x 512 image (tiles of 224,
overlap 32: 3 x 4 = 12 tiles, lanes 8, bf16, seeded ViT-B weights, K = 144) against MCM.encode_bytes / decode_bytes
of the same 12 tiles cut beforehand, i.e. the same coding work without the cut, the scores, the file and the blend.

The two paths alternate in one process; each timed call is a wall clock around a device synchronise (both end in
host bytes / a host status read anyway).  The two tile kernels are also timed on their own with device events over
many back-to-back launches.  Prints ONE JSON line: medians and spread (min, max, interquartile range) per call, the
deltas, and whether the image calls are slower than the tile calls by more than the run-to-run spread (the fastest
image round slower than the slowest tile round).

    python tools/tiled_bench.py [--rounds 10] [--warmup 3] [--out profiles/tiled/tiled_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "iqr_ms": round(q[2] - q[0], 3), "n": len(ms)}


def kernel_us(fn, iters=200):
    """mean device time of one launch over iters back-to-back launches, after a warm-up"""
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1e3 / iters, 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--lanes", type=int, default=8)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.rounds < 2:
        ap.error("--rounds must be at least 2")

    import textmae_amd
    from textmae_amd import ops, tiling
    from textmae_amd.scores import image_scores

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    S, K = 224, 144
    model = textmae_amd.MCM(img_size=S, num_keep_patches=K).to(dev).eval()
    model.compute_dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    model.update(force=True)
    H, W, O = args.height, args.width, args.overlap
    g = tiling.grid(H, W, S, O)
    # a seeded smooth image with noise: flat noise would make every tile's scores alike
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(7)
    a = np.stack([127 + 120 * np.sin(xx / (9.0 + 4 * c)) * np.cos(yy / (11.0 + 3 * c)) for c in range(3)], -1)
    img = torch.from_numpy(np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)).to(dev)
    tiles, gray = ops.tile_cut_u8(img, S, O)
    scores = image_scores(gray, S, 16)
    paths = {
        "image": (lambda: model.encode_image(img, overlap=O, lanes=args.lanes, tile_batch=g.T),
                  lambda c: model.decode_image(c)),
        "tiles": (lambda: model.encode_bytes(tiles, scores, lanes=args.lanes),
                  lambda c: model.decode_bytes(c)["x_hat"]),
    }
    t = {f"{p}_{k}": [] for p in paths for k in ("encode", "decode")}
    rec, size = {}, {}
    with torch.no_grad():
        for r in range(args.warmup + args.rounds):
            for p, (enc, dec) in paths.items():  # the paths alternate within every round
                c, te = timed(enc)
                d, td = timed(lambda: dec(c))
                if r >= args.warmup:
                    t[f"{p}_encode"].append(te)
                    t[f"{p}_decode"].append(td)
                rec[p] = d.clone()
                size[p] = len(c) if p == "image" else sum(len(b) for b in c)
        if not torch.equal(rec["image"], ops.tile_blend(rec["tiles"], H, W, O)):
            raise SystemExit("tiled_bench: the two paths reconstruct different images")
        x_hat = rec["tiles"].float().contiguous()
        kern = {"tile_cut_u8_us": kernel_us(lambda: ops.tile_cut_u8(img, S, O, tiles=tiles, gray=gray)),
                "image_scores_us": kernel_us(lambda: image_scores(gray, S, 16), iters=50),
                "tile_blend_us": kernel_us(lambda: ops.tile_blend(x_hat, H, W, O))}
    res = {"tool": "tiled_bench", "config": f"ViT-B img {S} K {K} {args.dtype}, {W}x{H}, overlap {O}, "
           f"{g.ny} x {g.nx} = {g.T} tiles, lanes {args.lanes}", "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "warmup": args.warmup}
    res.update({k: stats(v) for k, v in t.items()})
    for k in ("encode", "decode"):
        a_, b_ = res[f"image_{k}"], res[f"tiles_{k}"]
        res[f"image_{k}_vs_tiles"] = {"median_delta_ms": round(a_["median_ms"] - b_["median_ms"], 3),
                                      "tiles_spread_ms": round(b_["max_ms"] - b_["min_ms"], 3),
                                      "slower_beyond_spread": bool(a_["min_ms"] > b_["max_ms"])}
    res["kernels"] = kern
    res["bytes"] = {"image_file": size["image"], "tile_blobs": size["tiles"],
                    "bpp_file": round(8.0 * size["image"] / (W * H), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
