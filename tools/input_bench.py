#!/usr/bin/env python3
"""Time building model inputs from decoded images: the host path against the device path.

Both start from a batch of decoded uint8 RGB images in host memory (seeded noise with flat blocks; the decode is
outside both) and end with (imgs f32 [B, 3, 224, 224], total_scores [B, 196]) on the device:
  host    per image PIL resize((224, 224), BICUBIC) + ToTensor (testing.load_test_images) and the grayscale
          formula of scores.imread_gray on the host, one upload of the f32 batch and one of the gray batch, then the
          device score producer;
  device  data.prepare_batch: one upload of the uint8 batch, then grayscale, score producer and the Pillow-exact
          resize on the device.
The two alternate in one process; each timed call is a wall clock around a device synchronise.  Two more columns
split the device path, from a batch that is already resident: the resize alone and grayscale + scores alone.
Prints ONE JSON line with median [min, max] per column and shape.

    python tools/input_bench.py [--rounds 20] [--warmup 3] [--out profiles/input_pipeline/input_bench.json]
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

SHAPES = [(1356, 2040, 64), (512, 768, 1), (512, 768, 24)]  # DIV2K at batch 64, Kodak at batch 1 and 24


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "n": len(ms)}


def images(batch, H, W, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (batch, H, W, 3), dtype=np.uint8)
    a[:, : H // 2, : W // 3] = rng.integers(0, 256, (batch, 1, 1, 3), dtype=np.uint8)  # flat blocks: quadtree merges
    return a


def host_path(batch, size, dev):
    from PIL import Image

    from textmae_amd.scores import image_scores

    imgs, grays = [], []
    for a in batch:
        r = np.array(Image.fromarray(a).resize((size, size), Image.BICUBIC), dtype=np.float32) / 255.0
        imgs.append(torch.from_numpy(r).permute(2, 0, 1))
        v = a.astype(np.uint32)
        grays.append(((9798 * v[..., 0] + 19235 * v[..., 1] + 3735 * v[..., 2] + 16384) >> 15).astype(np.uint8))
    x = torch.stack(imgs).to(dev)
    g = torch.from_numpy(np.stack(grays)).to(dev)
    return x, image_scores(g, size)


def run_shape(H, W, batch, size, rounds, warmup, dev):
    from textmae_amd import ops
    from textmae_amd.data import prepare_batch
    from textmae_amd.scores import image_scores

    a = images(batch, H, W, 7)
    resident = torch.from_numpy(a).to(dev)
    paths = {
        "host": lambda: host_path(a, size, dev),
        "device": lambda: prepare_batch(a, size, normalize=False, device=dev),
        "device_resident_resize": lambda: ops.resize_u8(resident, size, out="f32"),
        "device_resident_gray_scores": lambda: image_scores(ops.rgb_to_gray_u8(resident), size),
    }
    t = {p: [] for p in paths}
    last = {}
    for r in range(warmup + rounds):
        for p, fn in paths.items():  # the paths alternate within every round
            last[p], ms = timed(fn)
            if r >= warmup:
                t[p].append(ms)
    if not (torch.equal(last["host"][0], last["device"][0]) and torch.equal(last["host"][1], last["device"][1])):
        raise SystemExit("input_bench: the two paths build different inputs")
    out = {p: stats(v) for p, v in t.items()}
    h, d = out["host"], out["device"]
    out["speedup"] = round(h["median_ms"] / d["median_ms"], 2)
    # faster only if the slowest round of one path beats the fastest round of the other
    out["device_faster_beyond_spread"] = bool(d["max_ms"] < h["min_ms"])
    out["host_faster_beyond_spread"] = bool(h["max_ms"] < d["min_ms"])
    out["upload_mb"] = {"host": round((batch * 3 * size * size * 4 + batch * H * W) / 1e6, 1),
                        "device": round(batch * H * W * 3 / 1e6, 1)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.rounds < 2:
        ap.error("--rounds must be at least 2")

    import PIL

    import textmae_amd  # noqa: F401

    dev = torch.device("cuda:0")
    res = {"tool": "input_bench", "size": args.size, "device": torch.cuda.get_device_name(0), "pillow": PIL.__version__,
           "host_threads": 1, "rounds": args.rounds, "warmup": args.warmup}
    for H, W, batch in SHAPES:
        res[f"{W}x{H}_batch_{batch}"] = run_shape(H, W, batch, args.size, args.rounds, args.warmup, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
