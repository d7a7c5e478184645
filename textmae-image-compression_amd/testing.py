"""Kodak evaluation harness — counterpart of reference testing.py: load a checkpoint,
``update(force=True)``, then per image compress -> Huffman-code ids_restore (side info) -> decompress ->
PSNR / MS-SSIM / bpp / encode and decode times, averaged, printed and written as report.txt JSON.

Same function names and arithmetic as the reference (testing.py:40-165, 199-250):
  * compute_metrics: both images rounded to 0..255, PSNR over the batch (psnr, testing.py:40-41),
    pytorch_msssim ms_ssim with data_range 255 -- both on the device (csrc/metrics.hip);
  * bpp = 8 * sum(len(s[0]) for s in strings) / pixels + len(huffman_bits) / pixels (testing.py:88-89):
    the y string plus ONLY the first image's z string (s[0] of the z list), as the reference counts it;
  * batch 1, the test transform (PIL bicubic resize to 224, ToTensor; no normalisation,
    utils/dataloader.py:69-73), scores from <dataset>_scores/test.pt or, when absent, from the device
    score-map producer (scores.py) instead of the reference's RuntimeError (dataloader.py:30-31).
``--bitstream DIR`` (no reference counterpart) sends every image through a self-contained file ``DIR/<name>.tmc``
(MCM.encode_bytes, written, read back, MCM.decode_bytes) and reports the files' own bpp, 8 * size / pixels, which
counts the container header and the side information in full.
``--tiled [--overlap N]`` (no reference counterpart) codes every image at its own resolution as overlapping
model-sized tiles (MCM.encode_image / decode_image; with ``--bitstream DIR`` through
``DIR/<name>.tmt``): PSNR / MS-SSIM against the original pixels, bpp = 8 * file size / (W * H); an image whose
smaller side is at most 160 is too small for MS-SSIM's five scales and reports PSNR only.
Deviation: ``inference_entropy_estimation`` takes the scores (the reference calls model.forward(x) without
them, testing.py:106, which raises).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

from . import _lib, ops
from .huffman import HuffmanCoding
from .ops import _stream

IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def collect_images(rootpath):
    files = []
    for ext in IMG_EXTENSIONS:
        files.extend(Path(rootpath).rglob(f"*{ext}"))
    return sorted(files)


def compute_metrics(org: torch.Tensor, rec: torch.Tensor, max_val: int = 255):
    """testing.py:44-49 -> {"psnr", "ms-ssim"} (device kernels; one D2H read of two floats)"""
    if max_val != 255:
        raise ValueError("compute_metrics: the reference evaluates at max_val=255")
    a = org.detach().float().contiguous()
    b = rec.detach().float().contiguous()
    if a.shape != b.shape or not a.is_cuda:
        raise ValueError("compute_metrics needs two device tensors of one shape")
    n, C, H, W = a.shape
    work = torch.empty(int(_lib.value("tmae_metrics_workspace", n, C, H, W)), dtype=torch.float32, device=a.device)
    out = torch.empty(2, dtype=torch.float32, device=a.device)
    _lib.call("tmae_image_metrics", a.data_ptr(), b.data_ptr(), n, C, H, W, work.data_ptr(), work.numel(),
              out.data_ptr(), _stream())
    v = out.tolist()
    return {"psnr": v[0], "ms-ssim": v[1]}


def bits_per_pixel(strings, huffman_bits, num_pixels):
    """testing.py:88-89 (the s[0] of each string list: the y string and the first z string)"""
    return sum(len(s[0]) for s in strings) * 8.0 / num_pixels + len(huffman_bits) / num_pixels


def save_output(x, ori_shape, file_name, output_dir, original_size=False):
    """testing.py:52-57.  The reference resizes the output back to ``ori_shape`` and discards the result: the
    saved file is the 224^2 output, and that stays the default.  With ``original_size`` the resize (PIL bicubic,
    on the device: ops.resize_u8) is the image that is saved; ori_shape is PIL's (W, H)."""
    from PIL import Image

    a = x.squeeze().clamp(0, 1).mul(255).round().byte().permute(1, 2, 0)
    if original_size:
        a = ops.resize_u8(a.contiguous(), (int(ori_shape[1]), int(ori_shape[0])))
    Image.fromarray(a.cpu().numpy()).save(os.path.join(output_dir, file_name))


@torch.no_grad()
def inference(model, x, ori_shape, total_score, file_name=None, output_dir=None, lanes=None, original_size=False):
    """testing.py:60-100; lanes (--lanes N) codes through compress_batch / decompress_batch with N y lanes;
    original_size (--original_size) saves the output resized back to ori_shape"""
    device = next(model.parameters()).device
    x = x.to(device)
    total_score = total_score.to(device)
    torch.cuda.synchronize()
    start = time.time()
    out_enc = model.compress(x, total_score) if lanes is None else model.compress_batch(x, total_score, lanes=lanes)
    enc_time = time.time() - start
    ids_keep = out_enc["ids_restore"]
    huffman = HuffmanCoding()
    compressed_ids_keep, shape, dev = huffman.compress(ids_keep)
    decompressed_ids_keep = huffman.decompress(compressed_ids_keep, shape, dev)
    start = time.time()
    if lanes is None:
        out_dec = model.decompress(out_enc["string"], out_enc["shape"], decompressed_ids_keep)
    else:
        out_dec = model.decompress_batch(out_enc["string"], out_enc["shape"], decompressed_ids_keep, lanes=lanes)
    torch.cuda.synchronize()
    dec_time = time.time() - start
    metrics = compute_metrics(x, out_dec["x_hat"], 255)
    num_pixels = x.size(0) * x.size(2) * x.size(3)
    bpp = bits_per_pixel(out_enc["string"], compressed_ids_keep, num_pixels)
    if output_dir is not None and file_name is not None:
        save_output(out_dec["x_hat"], ori_shape, file_name, output_dir, original_size)
    return {"psnr": metrics["psnr"], "ms-ssim": metrics["ms-ssim"], "bpp": bpp, "encoding_time": enc_time,
            "decoding_time": dec_time}


@torch.no_grad()
def inference_bitstream(model, x, ori_shape, total_score, file_name, bitstream_dir, output_dir=None, lanes=None,
                        original_size=False, q=None, qoffsets=None, rdoq=None):
    """--bitstream DIR: encode_bytes -> DIR/<name>.tmc -> read the file back -> decode_bytes.  The bpp is that of
    the file, 8 * size / pixels: header and side information counted in full.  original_size takes the size the
    blob itself recorded.  q (--q N): the y quantiser step's ladder position (MCM.encode_bytes), read back from the
    file by decode_bytes.  qoffsets (--q-offsets): a step per kept patch, recorded in the file
    too.  rdoq (--rdoq W): rate-distortion optimised quantisation of y at the encoder (§3.21); the file says nothing
    of it and decodes as any other."""
    device = next(model.parameters()).device
    x = x.to(device)
    total_score = total_score.to(device)
    path = os.path.join(bitstream_dir, Path(file_name).stem + ".tmc")
    torch.cuda.synchronize()
    start = time.time()
    blobs = model.encode_bytes(x, total_score, lanes=1 if lanes is None else lanes,
                               orig_sizes=[(int(ori_shape[0]), int(ori_shape[1]))], q=q, qoffsets=qoffsets,
                               rdoq=rdoq)
    enc_time = time.time() - start
    with open(path, "wb") as f:
        f.write(blobs[0])
    with open(path, "rb") as f:
        blob = f.read()
    start = time.time()
    out_dec = model.decode_bytes([blob])
    torch.cuda.synchronize()
    dec_time = time.time() - start
    metrics = compute_metrics(x, out_dec["x_hat"], 255)
    num_pixels = x.size(0) * x.size(2) * x.size(3)
    if output_dir is not None:
        save_output(out_dec["x_hat"], out_dec["orig_sizes"][0], file_name, output_dir, original_size)
    return {"psnr": metrics["psnr"], "ms-ssim": metrics["ms-ssim"], "bpp": 8.0 * os.path.getsize(path) / num_pixels,
            "encoding_time": enc_time, "decoding_time": dec_time}


MS_SSIM_MIN_SIDE = 161  # five scales of an 11-tap window: the smaller side must exceed 160 (tmae_image_metrics)


@torch.no_grad()
def inference_tiled(model, rgb, file_name, overlap=32, bitstream_dir=None, output_dir=None, lanes=None, tile_batch=16,
                    q=None, qoffsets=None, rdoq=None):
    """--tiled: the image at its own resolution, rgb uint8 [H, W, 3] -> MCM.encode_image -> (with bitstream_dir)
    DIR/<name>.tmt, read back -> MCM.decode_image.  PSNR / MS-SSIM against the original pixels at that resolution,
    bpp = 8 * file size / (W * H).  An image too small for MS-SSIM's five scales gets PSNR only (no "ms-ssim")."""
    import math

    device = next(model.parameters()).device
    x = torch.from_numpy(np.ascontiguousarray(rgb)).to(device)
    H, W = int(x.shape[0]), int(x.shape[1])
    torch.cuda.synchronize()
    start = time.time()
    blob = model.encode_image(x, overlap=overlap, lanes=1 if lanes is None else lanes, tile_batch=tile_batch, q=q,
                              qoffsets=qoffsets, rdoq=rdoq)
    enc_time = time.time() - start
    if bitstream_dir is not None:
        path = os.path.join(bitstream_dir, Path(file_name).stem + ".tmt")
        with open(path, "wb") as f:
            f.write(blob)
        with open(path, "rb") as f:
            blob = f.read()
    start = time.time()
    rec = model.decode_image(blob)
    torch.cuda.synchronize()
    dec_time = time.time() - start
    org = x.permute(2, 0, 1).float().div(255).unsqueeze(0)
    rv = {"bpp": 8.0 * len(blob) / (W * H), "encoding_time": enc_time, "decoding_time": dec_time}
    if min(H, W) >= MS_SSIM_MIN_SIDE:
        rv.update(compute_metrics(org, rec.unsqueeze(0), 255))
    else:  # compute_metrics' PSNR alone: both images rounded to 0..255
        r255 = rec.mul(255).clamp(0, 255).round()
        mse = float((org[0].mul(255).round() - r255).square().mean())
        rv["psnr"] = 20.0 * math.log10(255.0) - 10.0 * math.log10(mse) if mse > 0 else float("inf")
    if output_dir is not None:
        from PIL import Image

        a = rec.clamp(0, 1).mul(255).round().byte().permute(1, 2, 0)  # save_output's chain, at the image's own size
        Image.fromarray(a.cpu().numpy()).save(os.path.join(output_dir, Path(file_name).stem + ".png"))
    return rv


def eval_tiled(model, output_dir, filepaths, overlap=32, lanes=None, bitstream_dir=None, tile_batch=16, q=None,
               qoffsets=None, rdoq=None):
    """--tiled counterpart of eval_model over image files: every metric averaged over the images that have it
    -> (metrics, number of images with MS-SSIM)"""
    from PIL import Image

    for d in (output_dir, bitstream_dir):
        if d is not None:
            os.makedirs(d, exist_ok=True)
    sums, counts = defaultdict(float), defaultdict(int)
    for p in filepaths:
        rv = inference_tiled(model, np.array(Image.open(p).convert("RGB")), p.name, overlap, bitstream_dir, output_dir,
                             lanes, tile_batch, q, qoffsets, rdoq)
        for k, v in rv.items():
            sums[k] += v
            counts[k] += 1
    return {k: sums[k] / counts[k] for k in sums}, counts["ms-ssim"]


@torch.no_grad()
def inference_entropy_estimation(model, x, total_score, q=None, qoffsets=None):
    """testing.py:103-120 with the scores passed (the reference omits them and raises).  q (--q N): the estimate at
    the y quantiser step 2^(N/8) (MCM.forward's q); qoffsets (--q-offsets): at a step per kept patch
    (§3.19)"""
    device = next(model.parameters()).device
    x, total_score = x.to(device), total_score.to(device)
    torch.cuda.synchronize()
    start = time.time()
    kw = {k: v for k, v in (("q", q), ("qoffsets", qoffsets)) if v is not None}
    out = model.forward(x, total_score, **kw)
    torch.cuda.synchronize()
    elapsed = time.time() - start
    metrics = compute_metrics(x, out["x_hat"], 255)
    num_pixels = x.size(0) * x.size(2) * x.size(3)
    bpp = float(ops.bpp(out["likelihoods"]["y"], out["likelihoods"]["z"], num_pixels))  # device reduction
    return {"psnr": metrics["psnr"], "ms-ssim": metrics["ms-ssim"], "bpp": bpp, "encoding_time": elapsed / 2.0,
            "decoding_time": elapsed / 2.0}


def load_test_images(paths, size=224, device=None):
    """the test transform (utils/dataloader.py:69-73): RGB, PIL bicubic resize to size^2, ToTensor.  With a
    ``device`` the host only decodes: the uint8 image is uploaded and the resize + ToTensor run there
    (ops.resize_u8, equal to the host path bit for bit); the tensors stay on that device."""
    from PIL import Image

    out = []
    for p in paths:
        im = Image.open(p).convert("RGB")
        ori = im.size
        if device is not None:
            x = torch.from_numpy(np.array(im)).to(device)
            out.append((ops.resize_u8(x.unsqueeze(0), size, out="f32"), ori))
            continue
        a = np.array(im.resize((size, size), Image.BICUBIC), dtype=np.float32) / 255.0
        out.append((torch.from_numpy(a).permute(2, 0, 1).unsqueeze(0).contiguous(), ori))
    return out


def eval_model(model, output_dir, images, scores, names=None, entropy_estimation=False, lanes=None,
               original_size=False, bitstream_dir=None, q=None, qoffsets=None, rdoq=None):
    """testing.py:128-165 over pre-loaded (img [1,3,S,S], orig_shape) pairs and a [N, L] score tensor; with
    bitstream_dir every image goes through its .tmc file there (inference_bitstream; needs names)"""
    metrics = defaultdict(float)
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
    if bitstream_dir is not None:
        if names is None:
            raise ValueError("eval_model: bitstream_dir needs the images' names")
        os.makedirs(bitstream_dir, exist_ok=True)
    for i, (img, ori_shape) in enumerate(images):
        ts = scores[i:i + 1]
        if entropy_estimation:
            rv = inference_entropy_estimation(model, img, ts, q=q, qoffsets=qoffsets)
        elif bitstream_dir is not None:
            rv = inference_bitstream(model, img, ori_shape, ts, names[i], bitstream_dir, output_dir, lanes=lanes,
                                     original_size=original_size, q=q, qoffsets=qoffsets, rdoq=rdoq)
        else:
            rv = inference(model, img, ori_shape, ts, None if names is None else names[i], output_dir, lanes=lanes,
                           original_size=original_size)
        for k, v in rv.items():
            metrics[k] += v
    for k in metrics:
        metrics[k] /= len(images)
    return dict(metrics)


def load_checkpoint(num_keep_patches, checkpoint_path, img_size=224, **model_kwargs):
    """testing.py:123-125: the checkpoint's 'model' state_dict into MCM.from_state_dict (CDF buffers resized
    by the compressai-style load_state_dict).  Loaded with weights_only=True; the reference's save_model
    (models/Compression/common/model_utils.py:30-55) stores ``args`` as an argparse.Namespace next to the
    model, so that one class is allow-listed for the weights-only unpickler."""
    from .mcm import MCM

    with torch.serialization.safe_globals([argparse.Namespace]):
        sd = torch.load(checkpoint_path, map_location="cpu", weights_only=True)["model"]
    net = MCM(img_size=img_size, num_keep_patches=num_keep_patches, **model_kwargs)
    net.load_state_dict(sd)
    return net.eval()


def setup_args():
    p = argparse.ArgumentParser()
    p.add_argument("-d", "--dataset", type=str, help="Path to the dataset")
    p.add_argument("-o", "--output_path", type=str, default="reconstruction")
    p.add_argument("-e", "--entropy-coder", default="ans", choices=["ans"])
    p.add_argument("--cuda", action="store_true")
    p.add_argument("--half", action="store_true", help="bf16 operands (the MI355X counterpart of --half)")
    p.add_argument("--entropy-estimation", action="store_true")
    p.add_argument("-v", "--verbose", action="store_true")
    p.add_argument("-c", "--checkpoint", dest="checkpoint_paths", type=str, nargs="*", required=True)
    p.add_argument("--num_keep_patches", type=int, default=144, required=True)
    p.add_argument("--input_size", type=int, default=224, required=True)
    p.add_argument("--lanes", type=int, default=None, choices=[1, 2, 4, 8, 16, 32, 64],
                   help="code on the device (compress_batch / decompress_batch) with this many interleaved y lanes")
    p.add_argument("--original_size", action="store_true",
                   help="save each output resized back to its image's original size (bicubic, on the device)")
    p.add_argument("--bitstream", type=str, default=None, metavar="DIR",
                   help="code every image into the self-contained file DIR/<name>.tmc (encode_bytes, --lanes y lanes, "
                        "default 1), read it back and decode that (decode_bytes); bpp = 8 * file size / pixels")
    p.add_argument("--tiled", action="store_true",
                   help="code every image at its own resolution as overlapping model-sized tiles (encode_image / "
                        "decode_image; with --bitstream DIR through DIR/<name>.tmt); metrics against the original "
                        "pixels, bpp = 8 * file size / (W * H)")
    p.add_argument("--overlap", type=int, default=32, help="tile overlap in pixels (--tiled)")
    p.add_argument("--q", type=int, default=None, metavar="N",
                   help="quantiser step 2^(N/8) on the y latents, N in -32..32 (--bitstream / --tiled: DESIGN.md "
                        "§3.17; --entropy-estimation: the estimated rate and x_hat at that step, §3.18): larger N, "
                        "smaller files")
    p.add_argument("--q-offsets", type=_q_offsets, default=None, metavar="A,B,C,...", dest="q_offsets",
                   help="a quantiser step per kept patch (DESIGN.md §3.19): 2..16 ladder offsets in -64..64, the first "
                        "for the most text-like share of the kept patches, added to --q (default 0); with "
                        "--bitstream / --tiled / --entropy-estimation")
    p.add_argument("--rdoq", type=_rdoq, default=None, metavar="W",
                   help="rate-distortion optimised quantisation of y at the encoder (DESIGN.md §3.21): a y symbol moves "
                        "one step toward zero where W times the bits that saves exceeds the squared latent error it "
                        "adds; W >= 0 in squared latent units per bit, 0 = plain rounding; with --bitstream / --tiled")
    return p


def _rdoq(text):
    import math

    try:
        w = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--rdoq {text!r} is not a number") from None
    if not (math.isfinite(w) and w >= 0):
        raise argparse.ArgumentTypeError(f"--rdoq {text} must be finite and >= 0")
    return w


def _q_offsets(text):
    from .bitstream import check_offsets

    try:
        return check_offsets([int(v) for v in text.split(",")], "--q-offsets")
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def main(argv):
    from .codec import join_q_offsets

    args = setup_args().parse_args(join_q_offsets(argv))
    filepaths = collect_images(args.dataset)
    if not filepaths:
        print("Error: no images found in directory.", file=sys.stderr)
        sys.exit(1)
    if args.tiled and args.entropy_estimation:
        print("Error: --tiled codes real files; it does not combine with --entropy-estimation.", file=sys.stderr)
        sys.exit(1)
    if args.q is not None and not (args.tiled or args.bitstream is not None or args.entropy_estimation):
        print("Error: --q needs --bitstream DIR or --tiled (real files) or --entropy-estimation (the estimate).",
              file=sys.stderr)
        sys.exit(1)
    if args.q_offsets is not None and not (args.tiled or args.bitstream is not None or args.entropy_estimation):
        print("Error: --q-offsets needs --bitstream DIR or --tiled (real files) or --entropy-estimation (the "
              "estimate).", file=sys.stderr)
        sys.exit(1)
    if args.rdoq is not None and not (args.tiled or args.bitstream is not None) or \
            args.rdoq is not None and args.entropy_estimation:
        print("Error: --rdoq is an encoder decision: it needs --bitstream DIR or --tiled (real files).", file=sys.stderr)
        sys.exit(1)
    if not args.tiled:
        ds = Path(args.dataset)
        score_file = ds.parent / f"{ds.name}_scores" / "test.pt"
        if score_file.exists():
            scores = torch.load(score_file, map_location="cpu", weights_only=True)
        else:
            from .scores import preprocess_image_scores

            scores = preprocess_image_scores(filepaths, args.input_size)
        images = load_test_images(filepaths, args.input_size)
    results = defaultdict(list)
    with_msssim = 0
    for run in args.checkpoint_paths:
        model = load_checkpoint(args.num_keep_patches, run, args.input_size).to("cuda")
        if args.half:
            model.compute_dtype = torch.bfloat16
        model.update(force=True)
        if args.tiled:
            m, with_msssim = eval_tiled(model, args.output_path, filepaths, args.overlap, lanes=args.lanes,
                                        bitstream_dir=args.bitstream, q=args.q, qoffsets=args.q_offsets,
                                        rdoq=args.rdoq)
        else:
            m = eval_model(model, args.output_path, images, scores, [p.name for p in filepaths],
                           args.entropy_estimation, lanes=args.lanes, original_size=args.original_size,
                           bitstream_dir=args.bitstream, q=args.q, qoffsets=args.q_offsets, rdoq=args.rdoq)
        for k, v in m.items():
            results[k].append(v)
    desc = "entropy estimation" if args.entropy_estimation else args.entropy_coder
    if args.tiled:
        desc += (f"; tiled at the images' own resolution, overlap {args.overlap}: bpp of the .tmt files over W x H; "
                 f"MS-SSIM over the {with_msssim} of {len(filepaths)} images whose smaller side exceeds "
                 f"{MS_SSIM_MIN_SIDE - 1}, PSNR only for the others")
    elif args.bitstream is not None and not args.entropy_estimation:
        desc += "; bpp of the .tmc files: header and side information counted in full"
    if args.q:
        desc += f"; y quantiser step 2^({args.q}/8)"
    if args.q_offsets is not None:
        desc += f"; per-patch ladder offsets {','.join(str(v) for v in args.q_offsets)} by score rank"
    if args.rdoq is not None:
        desc += f"; rate-distortion optimised quantisation of y, weight {args.rdoq:g} per bit (encoder only)"
    output = {"name": "MCM", "description": f"Inference ({desc})", "results": results}
    print(json.dumps(output, indent=2))
    os.makedirs(args.output_path, exist_ok=True)
    with open(os.path.join(args.output_path, "report.txt"), "w") as f:
        json.dump(output, f, indent=2)
    return output


if __name__ == "__main__":
    main(sys.argv[1:])
