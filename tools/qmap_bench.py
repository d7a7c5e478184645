#!/usr/bin/env python3
"""Time MCM.encode_bytes / decode_bytes with a quantiser step per kept patch against the same calls
with a step per image (§3.17): what the map costs.

ViT-B, 256 x 256, K = 144, batch 64, bf16, seeded weights and inputs (the bench configuration).  q mixed = (-16, -5, 0,
3, 8, 16) repeated over the images.  Three columns alternate in one process: "q" (TQC blobs), "q+offsets" (the same q
as the base position, offsets -8,-3,0,5, levels from the scores: TPC blobs) and "q+map" (the levels from a caller's
device map).  Each timed call is a wall clock around a device synchronise.  Prints ONE JSON line: median / min / max /
interquartile range per column and call, the mean blob bytes and the bytes of the level section.

    python tools/qmap_bench.py [--rounds 10] [--warmup 3] [--batch 64] [--lanes 1] [--out profiles/qmap/x.json]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--keep", type=int, default=144)
    ap.add_argument("--lanes", type=int, default=1)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.rounds < 2:
        ap.error("--rounds must be at least 2")

    import textmae_amd
    from textmae_amd import bitstream

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = textmae_amd.MCM(img_size=args.img, num_keep_patches=args.keep).to(dev).eval()
    model.compute_dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    model.update(force=True)
    B, L = args.batch, model.encoder_embed.num_patches
    x, s = inputs(B, args.img, L, 1000, dev)
    q = [QMIX[b % len(QMIX)] for b in range(B)]
    with torch.no_grad():  # a caller's map that reproduces the scores' levels: the same bytes by another source
        out = model.compress_batch(x, s, qoffsets=OFFSETS)
        shuf = torch.argsort(out["ids_restore"], dim=1)
        cmap = torch.zeros((B, L), dtype=torch.int32, device=dev)
        cmap.scatter_(1, shuf[:, :args.keep], out["qlevels"])
    cols = {"q": dict(q=q), "q+offsets": dict(q=q, qoffsets=OFFSETS), "q+map": dict(q=q, qoffsets=OFFSETS, qlevels=cmap)}
    t = {f"{c}_{k}": [] for c in cols for k in ("encode", "decode")}
    blobs = {}
    with torch.no_grad():
        for r in range(args.warmup + args.rounds):
            for c, kw in cols.items():  # the columns alternate within every round
                blobs[c], te = timed(lambda kw=kw: model.encode_bytes(x, s, lanes=args.lanes, **kw))
                _, td = timed(lambda c=c: model.decode_bytes(blobs[c]))
                if r >= args.warmup:
                    t[f"{c}_encode"].append(te)
                    t[f"{c}_decode"].append(td)
    if blobs["q+offsets"] != blobs["q+map"]:
        raise SystemExit("qmap_bench: the caller's map does not reproduce the scores' bytes")
    res = {"tool": "qmap_bench", "config": f"ViT-B img {args.img} K {args.keep} batch {B} {args.dtype} lanes {args.lanes}",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup, "q": list(QMIX),
           "offsets": list(OFFSETS)}
    res.update({k: stats(v) for k, v in t.items()})
    for c in cols:
        res[f"{c}_total"] = stats([a + b for a, b in zip(t[f"{c}_encode"], t[f"{c}_decode"])])
        res[f"{c}_bytes_per_image"] = round(sum(len(b) for b in blobs[c]) / B, 1)
    res["level_section_bytes"] = 4 * bitstream.level_words(args.keep, len(OFFSETS))
    res["header_bytes"] = {"TQC": bitstream.QHEADER_BYTES, "TPC": bitstream.PHEADER_BYTES}
    for k in ("encode", "decode", "total"):
        a, b = res[f"q+offsets_{k}"], res[f"q_{k}"]
        res[f"offsets_{k}_vs_q"] = {"median_delta_ms": round(a["median_ms"] - b["median_ms"], 3),
                                    "slower_beyond_spread": bool(a["min_ms"] > b["max_ms"])}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
