"""Command-line codec on the self-contained bitstreams (bitstream.py, MCM.encode_bytes / decode_bytes):

    python -m textmae_amd.codec encode -c CKPT -d FOLDER -o OUT [--lanes N --batch B]
    python -m textmae_amd.codec decode -c CKPT -d OUT -o PNGS [--original_size]
    python -m textmae_amd.codec encode --tiled [--overlap N] -c CKPT -d FOLDER -o OUT
    python -m textmae_amd.codec decode --region X,Y,W,H -c CKPT -d OUT -o PNGS
    python -m textmae_amd.codec encode [--tiled] --q N | --target-bytes N ...
    python -m textmae_amd.codec encode [--tiled] --q-offsets A,B,C,... [--q N | --target-bytes N] ...
    python -m textmae_amd.codec encode [--tiled] --rdoq W [--q N | --target-bytes N] [--q-offsets A,B,C,...] ...

``encode --tiled`` codes every image at its own resolution as overlapping model-sized tiles (MCM.encode_image,
one ``<name>.tmt`` each); ``decode`` takes ``.tmt`` files next to ``.tmc`` ones and saves them at their native size.
``decode --region X,Y,W,H`` saves that window of every ``.tmt`` file instead, reading and decoding only the tiles
the window needs (MCM.decode_region); ``.tmc`` files beside them decode as before.

``encode --q N`` codes the y latents at the quantiser step 2^(N/8), N in -32..32: larger N, smaller
files.  ``encode --target-bytes N`` instead picks, per file, the smallest N whose file is at most that many bytes,
and warns about a file that does not fit even at N = 32.  The files record N; ``decode`` needs no flag.

``encode --q-offsets A,B,C,...`` (2..16 integers in -64..64) codes every kept patch at its own step:
the kept patches of an image (of a tile with ``--tiled``) are ranked by their text score, split into as many levels
as there are offsets, the most text-like share first, and level l is coded at ladder position N + offset l (clamped
to -32..32), N being ``--q`` (default 0) or what ``--target-bytes`` picks.  The files record the table and the
levels; ``decode`` needs no flag.

``encode --rdoq W`` lets the encoder move a y symbol one step toward zero where W times the bits that
saves through the symbol's own CDF row exceeds the squared latent error it adds; W >= 0, in squared latent units per
bit, 0 being plain rounding.  It works with ``--q``, ``--target-bytes``, ``--q-offsets`` and ``--tiled``; the files
are of the same kinds, record nothing of it, and ``decode`` needs no flag.

``encode`` reads FOLDER through ``data.ImageFolderLoader`` (the test transform: bicubic resize to the model's
size, scores from ``<FOLDER>_scores/test.pt`` or the device producer) and writes one ``<name>.tmc`` per image,
which records the image's original size.  ``decode`` needs only the checkpoint and those files: the geometry
(input size, kept patches) comes from the first file's header, and every file is checked against the model.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

import torch

from PIL import Image

from . import bitstream
from .data import ImageFolderLoader
from .testing import collect_images, load_checkpoint, save_output


def _model(checkpoint, num_keep_patches, input_size, half):
    model = load_checkpoint(num_keep_patches, checkpoint, input_size).to("cuda")
    if half:
        model.compute_dtype = torch.bfloat16
    model.update(force=True)
    return model


def _warn_target(args, name, blob):
    if args.target_bytes is not None and len(blob) > args.target_bytes:
        print(f"Warning: {name}: {len(blob)} bytes at the coarsest step (q = {bitstream.Q_MAX}), above "
              f"--target-bytes {args.target_bytes}.", file=sys.stderr)


@torch.no_grad()
def encode_tiled(args, model):
    """--tiled: every image at its own resolution (no resize, no loader) -> <name>.tmt, MCM.encode_image"""
    import numpy as np

    files = collect_images(args.dataset)
    if not files:
        print(f"Error: no images found in {args.dataset}.", file=sys.stderr)
        sys.exit(1)
    os.makedirs(args.output, exist_ok=True)
    nbytes = npixels = 0
    for p in files:
        a = np.array(Image.open(p).convert("RGB"))
        blob = model.encode_image(a, overlap=args.overlap, lanes=args.lanes, tile_batch=args.batch, q=args.q,
                                  target_bytes=args.target_bytes, qoffsets=args.q_offsets, rdoq=args.rdoq)
        _warn_target(args, p.name, blob)
        with open(os.path.join(args.output, p.stem + ".tmt"), "wb") as f:
            f.write(blob)
        nbytes += len(blob)
        npixels += a.shape[0] * a.shape[1]
    print(f"{len(files)} images -> {args.output}: {nbytes} bytes, {8.0 * nbytes / npixels:.4f} bpp over "
          f"{npixels} pixels at the images' own sizes")
    return len(files)


@torch.no_grad()
def encode(args):
    model = _model(args.checkpoint, args.num_keep_patches, args.input_size, args.half)
    if args.tiled:
        return encode_tiled(args, model)
    loader = ImageFolderLoader(args.dataset, "test", args.batch, size=args.input_size,
                               patch=model.encoder_embed.patch_size[0])
    os.makedirs(args.output, exist_ok=True)
    paths, done, nbytes = loader.imgs_path, 0, 0
    for imgs, ori_shapes, scores in loader:  # unshuffled: batch i holds paths[done : done + B]
        blobs = model.encode_bytes(imgs, scores, lanes=args.lanes, orig_sizes=ori_shapes, q=args.q,
                                   target_bytes=args.target_bytes, qoffsets=args.q_offsets, rdoq=args.rdoq)
        for p, blob in zip(paths[done:done + len(blobs)], blobs):
            _warn_target(args, p.name, blob)
            with open(os.path.join(args.output, p.stem + ".tmc"), "wb") as f:
                f.write(blob)
            nbytes += len(blob)
        done += len(blobs)
    print(f"{done} images -> {args.output}: {nbytes} bytes, "
          f"{8.0 * nbytes / (done * args.input_size ** 2):.4f} bpp at {args.input_size}^2")
    return done


@torch.no_grad()
def decode(args):
    files = sorted(Path(args.dataset).glob("*.tmc"))
    tiled = sorted(Path(args.dataset).glob("*.tmt"))
    if not files and not tiled:
        print(f"Error: no .tmc or .tmt files found in {args.dataset}.", file=sys.stderr)
        sys.exit(1)
    first = min(files[:1] + tiled[:1])
    with open(first, "rb") as f:
        head = bitstream.read_image_index(f) if first.suffix == ".tmt" else bitstream.parse(f.read())
    model = _model(args.checkpoint, head.num_keep_patches, head.img_size, args.half)
    os.makedirs(args.output, exist_ok=True)
    for p in tiled:  # one image each, at its own size
        try:
            if args.region is None:
                a = model.decode_image(p.read_bytes(), out="u8")
            else:  # the file object: only the header, the table and the needed tiles are read
                with open(p, "rb") as f:
                    a = model.decode_region(f, *args.region, out="u8")
        except ValueError as e:
            raise ValueError(f"{p.name}: {e}") from None
        Image.fromarray(a.cpu().numpy()).save(os.path.join(args.output, p.stem + ".png"))
    for s in range(0, len(files), args.batch):
        group = files[s:s + args.batch]
        blobs = [p.read_bytes() for p in group]
        try:
            out = model.decode_bytes(blobs)
        except ValueError as e:
            raise ValueError(f"{e} (blobs of this call: {', '.join(p.name for p in group)})") from None
        for b, p in enumerate(group):
            size = out["orig_sizes"][b]
            save_output(out["x_hat"][b], size, p.stem + ".png", args.output, args.original_size and size is not None)
    print(f"{len(files) + len(tiled)} images -> {args.output}")
    return len(files) + len(tiled)


def _region(text):
    """--region X,Y,W,H -> (x0, y0, w, h)"""
    try:
        x0, y0, w, h = (int(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not X,Y,W,H (four integers)") from None
    return x0, y0, w, h


def join_q_offsets(argv):
    """"--q-offsets", "-8,0,4" -> "--q-offsets=-8,0,4": argparse would take a list that starts with a minus sign for
    an option"""
    argv, out = list(argv), []
    while argv:
        a = argv.pop(0)
        out.append(a + "=" + argv.pop(0) if a == "--q-offsets" and argv else a)
    return out


def q_offsets(text):
    """--q-offsets A,B,C,... -> the table of ladder offsets as a tuple (bitstream.check_offsets)"""
    try:
        return bitstream.check_offsets([int(v) for v in text.split(",")], "--q-offsets")
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def setup_args():
    p = argparse.ArgumentParser(prog="textmae_amd.codec", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="command", required=True)
    for name in ("encode", "decode"):
        q = sub.add_parser(name)
        q.add_argument("-c", "--checkpoint", type=str, required=True)
        q.add_argument("-d", "--dataset", type=str, required=True,
                       help="image folder (encode) / folder of .tmc files (decode)")
        q.add_argument("-o", "--output", type=str, required=True)
        q.add_argument("--batch", type=int, default=16, help="images per device call")
        q.add_argument("--half", action="store_true", help="bf16 operands; encoder and decoder must agree")
    q = sub.choices["encode"]
    q.add_argument("--lanes", type=int, default=1, choices=[1, 2, 4, 8, 16, 32, 64], help="interleaved y lanes")
    q.add_argument("--num_keep_patches", type=int, default=144)
    q.add_argument("--input_size", type=int, default=224)
    q.add_argument("--tiled", action="store_true",
                   help="code every image at its own resolution as overlapping model-sized tiles -> <name>.tmt "
                        "(--batch tiles per device call)")
    q.add_argument("--overlap", type=int, default=32, help="tile overlap in pixels (--tiled), 0..input_size / 2")
    rate = q.add_mutually_exclusive_group()
    rate.add_argument("--q", type=int, default=None, metavar="N",
                      help="quantiser step 2^(N/8) on the y latents, N in -32..32: larger N, smaller files")
    rate.add_argument("--target-bytes", type=int, default=None, metavar="N", dest="target_bytes",
                      help="per file, the smallest step whose file is at most N bytes")
    q.add_argument("--q-offsets", type=q_offsets, default=None, metavar="A,B,C,...", dest="q_offsets",
                   help="a quantiser step per kept patch: 2..16 ladder offsets, the first for the most text-like "
                        "share of the kept patches (added to --q or to what --target-bytes picks)")
    q.add_argument("--rdoq", type=_rdoq, default=None, metavar="W",
                   help="rate-distortion optimised quantisation of y: a symbol moves one step toward zero where W "
                        "times the bits that saves exceeds the squared latent error it adds (W >= 0, 0 = plain "
                        "rounding); with --q, --target-bytes, --q-offsets and --tiled; decode needs no flag")
    sub.choices["decode"].add_argument("--original_size", action="store_true",
                                       help="save each output resized to the size its file recorded")
    sub.choices["decode"].add_argument("--region", type=_region, default=None, metavar="X,Y,W,H",
                                       help="of every .tmt file, decode and save only this window (origin X,Y, "
                                            "size W x H), from the tiles it needs")
    return p


def _rdoq(text):
    """--rdoq W -> the weight as a float (MCM._check_rdoq's conditions)"""
    import math

    try:
        w = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--rdoq {text!r} is not a number") from None
    if not (math.isfinite(w) and w >= 0):
        raise argparse.ArgumentTypeError(f"--rdoq {text} must be finite and >= 0")
    return w


def main(argv):
    args = setup_args().parse_args(join_q_offsets(argv))
    return encode(args) if args.command == "encode" else decode(args)


if __name__ == "__main__":
    main(sys.argv[1:])
