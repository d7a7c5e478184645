#!/usr/bin/env python3
"""Time entropy coding end to end: MCM.compress + decompress (host rANS coder, one y string per batch) against
MCM.compress_batch + decompress_batch (device rANS kernels, one y and one z stream per image).

ViT-B, 256 x 256, K = 144, bf16, seeded weights and inputs, at batch 64 and batch 1.  The two paths alternate in one
process; each timed call is a wall clock around a device synchronise (both paths end in host bytes / a host
status read anyway).  Prints ONE JSON line: medians and spread (min, max, interquartile range) of both paths per
batch, and the bytes per image of both formats.  --lanes 1,4,16,64 adds one device column per value above 1
(compress_batch(lanes=N), lane-interleaved records; 1 is the plain device column), alternating with the others.
--bitstream adds, beside every device column, a "bytes" column: MCM.encode_bytes + decode_bytes at the same lanes (the
self-contained blobs: compress_batch's records behind a header and the packed kept ids), the mean blob size split
into header, ids, z and y, and whether either call is slower than its device column by more than the spread.
--rdoq W adds, beside every device column, an "_rdoq" column: compress_batch(rdoq=W) (rate-distortion optimised
quantisation of y; the decoder is the same call), alternating with the others; it reports the cost
against its device column by the same rule, the symbols moved per image and the bytes.  Those columns reconstruct
other images than the plain ones, on purpose, and are left out of the equality check.

    python tools/coding_bench.py [--rounds 10] [--warmup 3] [--batches 64,1] [--lanes 1,4,16,64] [--bitstream]
                                 [--rdoq W] [--out profiles/coding_device/x.json]
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


def blob_split(blobs):
    """mean bytes per blob of each section"""
    from textmae_amd import bitstream

    parts = [bitstream.parse(b) for b in blobs]
    n = len(parts)
    return {"header": bitstream.HEADER_BYTES, "ids": round(sum(4 * p.ids.size for p in parts) / n, 1),
            "z": round(sum(len(p.z) for p in parts) / n, 1), "y": round(sum(len(p.y) for p in parts) / n, 1),
            "total": round(sum(len(b) for b in blobs) / n, 1)}


def run_batch(model, batch, img, rounds, warmup, dev, lanes=(), bitstream=False, rdoq=None):
    L = model.encoder_embed.num_patches
    x, s = inputs(batch, img, L, 1000, dev)
    paths = {
        "host": (lambda: model.compress(x, s),
                 lambda c: model.decompress(c["string"], c["shape"], c["ids_restore"])),
        "device": (lambda: model.compress_batch(x, s),
                   lambda c: model.decompress_batch(c["string"], c["shape"], c["ids_restore"])),
    }
    for n in lanes:
        if n != 1:
            paths[f"device_l{n}"] = (lambda n=n: model.compress_batch(x, s, lanes=n),
                                     lambda c, n=n: model.decompress_batch(c["string"], c["shape"], c["ids_restore"],
                                                                           lanes=n))
    rdo = {}  # rdoq column -> the device column it runs beside
    if rdoq is not None:
        for n in [1] + [n for n in lanes if n != 1]:
            devname = "device" if n == 1 else f"device_l{n}"
            paths[devname + "_rdoq"] = (lambda n=n: model.compress_batch(x, s, lanes=n, rdoq=rdoq),
                                        lambda c, n=n: model.decompress_batch(c["string"], c["shape"],
                                                                              c["ids_restore"], lanes=n))
            rdo[devname + "_rdoq"] = devname
    changed = {}
    pairs = {}  # bytes column -> the device column it wraps
    if bitstream:
        for n in [1] + [n for n in lanes if n != 1]:
            name, devname = ("bytes", "device") if n == 1 else (f"bytes_l{n}", f"device_l{n}")
            paths[name] = (lambda n=n: model.encode_bytes(x, s, lanes=n), lambda c: model.decode_bytes(c))
            pairs[name] = devname
    t = {f"{p}_{k}": [] for p in paths for k in ("compress", "decompress")}
    rec, size, split = {}, {}, {}
    with torch.no_grad():
        for r in range(warmup + rounds):
            for p, (comp, decomp) in paths.items():  # the paths alternate within every round
                c, tc = timed(comp)
                d, td = timed(lambda: decomp(c))
                if r >= warmup:
                    t[f"{p}_compress"].append(tc)
                    t[f"{p}_decompress"].append(td)
                rec[p] = d["x_hat"]
                if p in rdo:
                    changed[p] = float(model._exec.last_streams["y_changed"].mean())
                if p in pairs:
                    size[p], split[p] = sum(len(b) for b in c) / batch, blob_split(c)
                else:
                    size[p] = sum(len(b) for part in c["string"] for b in part) / batch
    if not all(torch.equal(rec["host"], rec[p]) for p in paths if p not in rdo):
        raise SystemExit("coding_bench: the paths reconstruct different images")
    out = {k: stats(v) for k, v in t.items()}
    for p in paths:
        total = [a + b for a, b in zip(t[f"{p}_compress"], t[f"{p}_decompress"])]
        out[f"{p}_total"] = stats(total)
    out["bytes_per_image"] = {p: round(v, 1) for p, v in size.items()}
    h, d = out["host_total"], out["device_total"]
    out["speedup_total"] = round(h["median_ms"] / d["median_ms"], 2)
    # faster by more than the run-to-run spread: the slowest device round beats the fastest host round
    out["device_faster_beyond_spread"] = bool(d["max_ms"] < h["min_ms"])
    for p in paths:
        if p.startswith("device_l"):  # against both yardsticks, by the same rule
            v = out[f"{p}_total"]
            out[f"{p}_faster_than_host_beyond_spread"] = bool(v["max_ms"] < h["min_ms"])
            out[f"{p}_faster_than_device_beyond_spread"] = bool(v["max_ms"] < d["min_ms"])
    for p, q in rdo.items():  # what the decision costs, by the rule of the bytes columns
        for k in ("compress", "decompress", "total"):
            a, b = out[f"{p}_{k}"], out[f"{q}_{k}"]
            out[f"{p}_{k}_vs_{q}"] = {"median_delta_ms": round(a["median_ms"] - b["median_ms"], 3),
                                      "slower_beyond_spread": bool(a["min_ms"] > b["max_ms"])}
        out[f"{p}_y_changed_per_image"] = round(changed[p], 1)
    if pairs:
        out["blob_bytes_per_image"] = split
    for p, q in pairs.items():  # slower beyond the spread: the fastest blob round is slower than the slowest device one
        for k in ("compress", "decompress", "total"):
            a, b = out[f"{p}_{k}"], out[f"{q}_{k}"]
            out[f"{p}_{k}_vs_{q}"] = {"median_delta_ms": round(a["median_ms"] - b["median_ms"], 3),
                                      "slower_beyond_spread": bool(a["min_ms"] > b["max_ms"])}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--keep", type=int, default=144)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--lanes", default="", help="comma-separated y lane counts (powers of two up to 64)")
    ap.add_argument("--bitstream", action="store_true",
                    help="add encode_bytes / decode_bytes beside every device column")
    ap.add_argument("--rdoq", type=float, default=None, metavar="W",
                    help="add compress_batch(rdoq=W) beside every device column")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.rounds < 2:
        ap.error("--rounds must be at least 2")
    lanes = [int(v) for v in args.lanes.split(",") if v]
    if any(n not in (1, 2, 4, 8, 16, 32, 64) for n in lanes):
        ap.error("--lanes takes powers of two in 1..64")

    import textmae_amd

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = textmae_amd.MCM(img_size=args.img, num_keep_patches=args.keep).to(dev).eval()
    model.compute_dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    model.update(force=True)
    res = {"tool": "coding_bench", "config": f"ViT-B img {args.img} K {args.keep} {args.dtype}",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup}
    if lanes:
        res["lanes"] = lanes
    if args.rdoq is not None:
        res["rdoq"] = args.rdoq
    for b in (int(v) for v in args.batches.split(",")):
        res[f"batch_{b}"] = run_batch(model, b, args.img, args.rounds, args.warmup, dev, lanes, args.bitstream,
                                      args.rdoq)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
