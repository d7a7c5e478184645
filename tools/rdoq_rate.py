#!/usr/bin/env python3
"""Record what rate-distortion optimised quantisation of y does to rate and latent error, per image
and per weight W: the bytes of the y record, coder.table_bits of the y symbols, the symbols moved (y_changed) and the
latent error sum (y_hat before the LRP - y)^2, for W = 0 and a few W > 0.

Two configurations, both with SEEDED RANDOM weights and inputs: "small12" (128 px, K = 16, f32, batch 3, q = -16:
tests/test_gpu_rdoq_model.py's) and "bench" (ViT-B, 256 x 256, K = 144, bf16, batch 64, lanes 16, q = 0 and -16).
Seeded weights say nothing about trained ones: this is a record of the mechanism, not a rate-distortion result.

    python tools/rdoq_rate.py [--weights 0,0.001,0.004,0.016] [--batch 64] [--out profiles/rdoq/rate_vs_w.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def record(model, x, s, q, weights, lanes, show):
    from textmae_amd import coder

    tabs = model.gaussian_conditional.host_tables()
    B, S = x.shape[0], model.num_slices
    rows = []
    for w in weights:
        out = model.compress_batch(x, s, lanes=lanes, q=q, rdoq=w)
        ex = model._exec
        st = ex.last_streams
        sym, idx = (np.array(st[k]).reshape(S, B, -1) for k in ("y_symbols", "y_indexes"))
        n = B * ex.g * ex.g  # the rows of the latent grid; the workspaces may be padded past them
        err = (ex.YPRE[:n].float() - ex.Y32[:n].float()).square().reshape(B, -1).sum(dim=1).cpu().numpy()
        bits = [coder.table_bits(sym[:, b].reshape(-1), idx[:, b].reshape(-1), *tabs) for b in range(B)]
        ybytes = [len(r) for r in out["string"][0]]
        changed = np.array(st["y_changed"]).tolist()
        keep = slice(0, show)
        rows.append({"rdoq": w, "q": q, "y_record_bytes": ybytes[keep], "table_bits": [round(v, 1) for v in bits[keep]],
                     "y_changed": changed[keep], "latent_error": [round(float(v), 4) for v in err[keep]],
                     "mean": {"y_record_bytes": round(float(np.mean(ybytes)), 1), "table_bits": round(float(np.mean(bits)), 1),
                              "y_changed": round(float(np.mean(changed)), 1), "latent_error": round(float(err.mean()), 4),
                              "nonzero_symbols": round(float((sym != 0).sum() / B), 1)}})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--weights", default="0,0.001,0.004,0.016")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    weights = [float(v) for v in args.weights.split(",")]

    import textmae_amd
    from oracle.mcm_oracle import MCMConfig, make_state_dict

    dev = torch.device("cuda:0")
    res = {"tool": "rdoq_rate", "device": torch.cuda.get_device_name(0),
           "caveat": "seeded random weights and inputs: no trained checkpoint is at hand, so these figures show the "
                     "mechanism (bits saved against latent error added) and say nothing about the rate-distortion "
                     "behaviour of a trained model; no reference counterpart, no rate-distortion gain measured",
           "latent_error": "sum over the image's y elements of (y_hat before the LRP - y)^2"}
    with torch.no_grad():
        cfg = MCMConfig(img_size=128, patch_size=16, encoder_embed_dim=128, encoder_depth=1, encoder_num_heads=2,
                        decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2, latent_depth=192,
                        hyperprior_depth=96, num_slices=12, num_keep_patches=16)
        m = textmae_amd.MCM(**cfg.kwargs())
        sd = m.state_dict()
        sd.update(make_state_dict(cfg, 11))
        m.load_state_dict(sd)
        m = m.to(dev).eval()
        m.update(force=True)
        g = torch.Generator().manual_seed(47)
        x = ((torch.rand(3, 3, 128, 128, generator=g) - 0.45) / 0.225).to(dev)
        s = torch.rand(3, 64, generator=g).to(dev)
        res["small12"] = {"config": "128 px, K 16, f32, batch 3, weight seed 11, input seed 47, lanes 1",
                          "rows": record(m, x, s, -16, weights, 1, 3)}
        torch.manual_seed(0)
        m = textmae_amd.MCM(img_size=256, num_keep_patches=144).to(dev).eval()
        m.compute_dtype = torch.bfloat16
        m.update(force=True)
        g = torch.Generator().manual_seed(1000)
        x = torch.rand(args.batch, 3, 256, 256, generator=g)
        x = ((x - torch.tensor((0.485, 0.456, 0.406)).view(1, 3, 1, 1)) / torch.tensor((0.229, 0.224, 0.225)).view(1, 3, 1, 1))
        s = torch.rand(args.batch, 256, generator=torch.Generator().manual_seed(1001))
        x, s = x.to(dev), s.to(dev)
        res["bench"] = {"config": f"ViT-B, 256 x 256, K 144, bf16, batch {args.batch}, lanes 16, torch seed 0 weights; "
                                  "per-image lists show the first 4 images, means are over the batch",
                        "rows": record(m, x, s, 0, weights, 16, 4) + record(m, x, s, -16, weights, 16, 4)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
