"""Attention-core micro-benchmark at the bench shapes (batch 64): encoder T=145, 12 heads x 64;
decoder T=257, 16 heads x 32 (or the shapes given as name=B,T,H,dh arguments).  Forward and backward;
MFMA utilisation = algorithmic flops (4 B H T^2 dh fwd, 2.5x that bwd incl. recompute) / time / 2.5 PF.

    python tools/attn_bench.py --long [--out FILE]
times the streamed kernels (csrc/attention_stream.hip) at the long-sequence shapes -- batch 64, 16 heads x 32 at
T = 577 and 1025, 12 heads x 64 at T = 577, bf16, random normal data -- next to
torch.nn.functional.scaled_dot_product_attention on the same tensors in the same process, rounds interleaved;
median and minimum per launch, written as JSON (default profiles/attn_stream/attn_stream_bench.json)."""
import json
import os
import sys

import torch

sys.path.insert(0, ".")
import textmae_amd  # noqa: E402,F401
from textmae_amd import ops, train_ops  # noqa: E402

PEAK = 2.5e15


def ev(fn, reps=20):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(5):
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        best = min(best, s.elapsed_time(e) / reps * 1e-3)
    return best


def _round(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e3  # us


def long_main(path, rounds=9, reps=10):
    import statistics

    import torch.nn.functional as F

    dt = torch.bfloat16
    shapes = {"dh32_T577": (64, 577, 16, 32), "dh32_T1025": (64, 1025, 16, 32), "dh64_T577": (64, 577, 12, 64)}
    out = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "rounds": rounds, "reps_per_round": reps,
           "unit": "us per launch", "shapes": {}}
    for name, (B, T, H, dh) in shapes.items():
        D = H * dh
        scale = dh ** -0.5
        qkv = torch.randn(B * T, 3 * D, device="cuda").to(dt)
        o = torch.empty(B * T, D, device="cuda", dtype=dt)
        lse = torch.empty(B * H * T, device="cuda")
        do = torch.randn(B * T, D, device="cuda").to(dt)
        dq = torch.empty_like(qkv)
        # torch on the same tensors: [B][H][T][dh] views of qkv, the output in the [B*T][H*dh] layout
        q, k, v = (t.requires_grad_(True) for t in qkv.view(B, T, 3, H, dh).permute(2, 0, 3, 1, 4).unbind(0))
        do_t = do.view(B, T, H, dh).transpose(1, 2)
        with torch.no_grad():
            ref = F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).reshape(B * T, D)
        train_ops.mha_lse(qkv, B, T, H, dh, scale, dt, o, lse)
        err = float((o.float() - ref.float()).abs().max())
        o_t = F.scaled_dot_product_attention(q, k, v, scale=scale)
        fns = {
            "tmae_fwd": lambda: train_ops.mha_lse(qkv, B, T, H, dh, scale, dt, o, lse),
            "torch_fwd": lambda: F.scaled_dot_product_attention(q.detach(), k.detach(), v.detach(), scale=scale),
            "tmae_bwd": lambda: train_ops.mha_bwd(qkv, o, do, lse, dq, B, T, H, dh, scale, dt),
            "torch_bwd": lambda: torch.autograd.grad(o_t, (q, k, v), do_t, retain_graph=True),
        }
        times = {n: [] for n in fns}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):  # interleaved: one round of each per pass
            for n, fn in fns.items():
                times[n].append(_round(fn, reps))
        res = {"B": B, "T": T, "H": H, "dh": dh, "plan_fwd": ops.mha_plan(T, dh, dt),
               "plan_bwd": ops.mha_plan(T, dh, dt, True), "max_abs_diff_vs_torch": err}
        for n, ts in times.items():
            res[n] = {"median": round(statistics.median(ts), 1), "min": round(min(ts), 1)}
        for d in ("fwd", "bwd"):
            res[f"{d}_ratio_to_torch_median"] = round(res[f"tmae_{d}"]["median"] / res[f"torch_{d}"]["median"], 3)
        out["shapes"][name] = res
        print(name, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    if "--long" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            os.path.join("profiles", "attn_stream", "attn_stream_bench.json")
        return long_main(path)
    out = {}
    dt = torch.bfloat16
    shapes = {"enc": (64, 145, 12, 64), "dec": (64, 257, 16, 32)}
    if len(sys.argv) > 1:  # name=B,T,H,dh ...
        shapes = {a.split("=")[0]: tuple(int(v) for v in a.split("=")[1].split(",")) for a in sys.argv[1:]}
    for name, (B, T, H, dh) in shapes.items():
        D = H * dh
        qkv = torch.randn(B * T, 3 * D, device="cuda").to(dt)
        o = torch.empty(B * T, D, device="cuda", dtype=dt)
        lse = torch.empty(B * H * T, device="cuda")
        do = torch.randn(B * T, D, device="cuda").to(dt)
        dq = torch.empty_like(qkv)
        fl = 4.0 * B * H * T * T * dh
        res = {}
        t = ev(lambda: ops.mha(qkv, B, T, H, dh, dh ** -0.5, dt, out=o))
        res["fwd_us"] = round(t * 1e6, 1)
        res["fwd_mfma_frac"] = round(fl / t / PEAK, 4)
        train_ops.mha_lse(qkv, B, T, H, dh, dh ** -0.5, dt, o, lse)
        t = ev(lambda: train_ops.mha_bwd(qkv, o, do, lse, dq, B, T, H, dh, dh ** -0.5, dt))
        res["bwd_us"] = round(t * 1e6, 1)
        res["bwd_mfma_frac"] = round(2.5 * fl / t / PEAK, 4)
        out[name] = res
        print(name, res, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
