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

--region times region decode on the same file instead: MCM.decode_image of the whole file,
MCM.decode_region of a window inside one tile and of a window across four tiles alternate in one process, each timed
the same way, and the JSON line says whether the one-tile window's median is below the whole image's.  Each call is
then also timed repeated back to back ("back_to_back"), where the model's per-batch-size preparation is not redone.

    python tools/tiled_bench.py --region [--rounds 20] [--out profiles/tiled/region_bench.json]
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


def region_bench(args, model, img, g):
    """--region: decode_image against decode_region of a one-tile and of a four-tile window of the same file"""
    from textmae_amd import tiling

    H, W, O, S = g.H, g.W, g.O, g.S
    blob = model.encode_image(img, overlap=O, lanes=args.lanes, tile_batch=min(g.T, 64))  # larger images in chunks
    one = (O, O, S - 2 * O, S - 2 * O)                 # (x0, y0, w, h): the part of tile 0 that is its alone
    four = (g.stride - 64, g.stride - 64, 256, 256)    # across the corner of tiles 0, 1, nx, nx + 1
    tiles = {"one_tile": tiling.region_tiles(g, *one), "four_tiles": tiling.region_tiles(g, *four)}
    if [len(v) for v in tiles.values()] != [1, 4]:
        raise SystemExit(f"tiled_bench: the windows need {tiles}, not one and four tiles")
    calls = {"image": lambda: model.decode_image(blob),
             "one_tile": lambda: model.decode_region(blob, *one),
             "four_tiles": lambda: model.decode_region(blob, *four)}
    t, steady, rec = {k: [] for k in calls}, {k: [] for k in calls}, {}
    with torch.no_grad():
        for r in range(args.warmup + args.rounds):
            for k, fn in calls.items():  # the calls alternate within every round
                rec[k], ms = timed(fn)
                if r >= args.warmup:
                    t[k].append(ms)
        # the same calls back to back.  The model keeps its prepared weights and workspaces for one batch size
        # (MCM._executor), so an alternating call prepares them again each time and a repeated one does not
        for k, fn in calls.items():
            for r in range(args.warmup + args.rounds):
                _, ms = timed(fn)
                if r >= args.warmup:
                    steady[k].append(ms)
        for k, (x0, y0, w, h) in (("one_tile", one), ("four_tiles", four)):
            if not torch.equal(rec[k], rec["image"][:, y0:y0 + h, x0:x0 + w]):
                raise SystemExit(f"tiled_bench: the {k} window is not the crop of the image")
    res = {"tool": "tiled_bench --region", "config": f"ViT-B img {S} K 144 {args.dtype}, {W}x{H}, overlap {O}, "
           f"{g.ny} x {g.nx} = {g.T} tiles, lanes {args.lanes}", "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "warmup": args.warmup, "file_bytes": len(blob),
           "windows": {"one_tile": {"x0_y0_w_h": one, "tiles": tiles["one_tile"]},
                       "four_tiles": {"x0_y0_w_h": four, "tiles": tiles["four_tiles"]}}}
    res.update({f"decode_{k}": stats(v) for k, v in t.items()})
    res["back_to_back"] = {f"decode_{k}": stats(v) for k, v in steady.items()}
    m = {k: res[f"decode_{k}"]["median_ms"] for k in calls}
    res["image_over_one_tile"] = round(m["image"] / m["one_tile"], 2)
    res["image_over_four_tiles"] = round(m["image"] / m["four_tiles"], 2)
    res["one_tile_faster_than_image"] = bool(m["one_tile"] < m["image"])
    return res


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--region", action="store_true", help="time decode_region against decode_image instead")
    ap.add_argument("--rounds", type=int, default=None, help="default 10, with --region 20")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--lanes", type=int, default=8)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.rounds is None:
        args.rounds = 20 if args.region else 10
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
    if args.region:
        return emit(region_bench(args, model, img, g), args.out)
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
    emit(res, args.out)


if __name__ == "__main__":
    main()
