"""Streamed attention, host side (CPU only): the dispatch rule as tmae_mha_plan reports it, the force hook, and
the code objects of the three streamed kernels.

Every length the LDS-resident kernels take keeps the kernel it had (their names, below); every length they refused
takes the streamed family, whose plan string carries the workgroup's block and chunk sizes."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_resources as kr  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16

# (T, dh, dtype, backward) -> the resident kernel: the shapes of the models the tests and the benchmark run today
RESIDENT = {
    (145, 64, BF16, False): "mha_fwd_bf16_kernel<64>",
    (145, 64, F32, False): "mha_fwd_kernel<f32,64>",
    (257, 32, BF16, False): "mha_fwd_bf16_kernel<32>",
    (257, 32, F32, False): "mha_fwd_kernel<f32,32>",
    (65, 80, BF16, False): "mha_fwd_kernel<bf16,80,512>",
    (65, 80, F32, False): "mha_fwd_kernel<f32,80>",
    (145, 64, BF16, True): "mha_bwd1_bf16_kernel<64>",
    (145, 64, F32, True): "mha_bwd_f32_kernel<64>",
    (257, 32, BF16, True): "mha_bwd1_bf16_kernel<32,640>",
    (257, 32, F32, True): "mha_bwd_f32_kernel<32>",
    (65, 80, BF16, True): "mha_bwd_bf16_kernel<80>",
    (65, 80, F32, True): "mha_bwd_f32_kernel<80>",
    (256, 64, BF16, True): "mha_bwd_bf16_kernel<64>",  # the longest bf16 dh 64 backward: one-pass LDS exceeded
}
STREAMED = [(577, 32, BF16, False), (577, 32, F32, False), (1025, 64, BF16, False), (1025, 64, F32, False),
            (513, 80, BF16, False), (513, 80, F32, False), (289, 64, F32, False),
            (257, 64, BF16, True), (513, 32, BF16, True)]


def _resident_plans(ops):
    return {k: ops.mha_plan(*k) for k in RESIDENT}


def test_plan_names_resident_and_streamed(tmae):
    from textmae_amd import _lib

    ops = tmae.ops
    _lib.value("tmae_mha_force_stream", 0)
    assert _resident_plans(ops) == RESIDENT
    for T, dh, dt, bwd in STREAMED:
        plan = ops.mha_plan(T, dh, dt, bwd)
        name = "bf16" if dt == BF16 else "f32"
        m = re.fullmatch(rf"stream<{name},dh{dh},q(\d+)(?:,k(\d+))?,c(\d+)>", plan)
        assert m, plan
        assert (m.group(2) is not None) == bwd, plan  # the backward also names its keys per workgroup
        q, c = int(m.group(1)), int(m.group(3))
        assert q % 32 == 0 and c % 32 == 0 and q > 0 and c > 0, plan
    # the boundaries of the table: the last resident length and the first streamed one
    for T, dh, dt, bwd in [(512, 32, BF16, False), (480, 64, BF16, False), (416, 80, BF16, False), (512, 32, F32, False),
                           (288, 64, F32, False), (224, 80, F32, False),
                           (256, 80, BF16, True), (512, 32, BF16, True), (512, 64, F32, True), (256, 80, F32, True)]:
        assert "stream" not in ops.mha_plan(T, dh, dt, bwd), (T, dh, dt, bwd)
        assert "stream" in ops.mha_plan(T + 1, dh, dt, bwd), (T + 1, dh, dt, bwd)


def test_force_hook(tmae):
    from textmae_amd import _lib

    ops = tmae.ops
    assert _lib.value("tmae_mha_force_stream", 0) == 0
    free = _resident_plans(ops)
    assert "stream" not in ops.mha_plan(33, 32, BF16)
    with ops.mha_force_stream():
        assert _lib.value("tmae_mha_force_stream", 1) == 1  # returns the previous value
        for bwd in (False, True):
            for dt in (BF16, F32):
                assert ops.mha_plan(33, 32, dt, bwd).startswith("stream<"), (dt, bwd)
        assert all("stream" in p for p in _resident_plans(ops).values())
    assert _lib.value("tmae_mha_force_stream", 0) == 0  # restored on exit
    assert _resident_plans(ops) == free == RESIDENT


def test_plan_rejects_bad_arguments(tmae):
    with pytest.raises(ValueError, match="head dim"):
        tmae.ops.mha_plan(100, 48, BF16)


@pytest.mark.skipif(not kr.tools_present() or not os.path.isdir(kr.OBJ) or
                    not any(f.endswith(".hip.o") for f in os.listdir(kr.OBJ)),
                    reason="ROCm LLVM tools or built objects absent")
def test_streamed_kernels_present_and_scratch_free():
    names = [k for ks in kr.all_kernels().values() for k in ks]
    for kern in ("mha_fwd_stream_kernel", "mha_bwd_stream_dkv_kernel", "mha_bwd_stream_dq_kernel"):
        hits = [k for k in names if kern in k["name"]]
        assert len(hits) >= 6, f"{kern}: {len(hits)} instantiations (two dtypes x three head dims expected)"
        bad = [k["name"] for k in hits if k.get("private_segment_fixed_size", 0)]
        assert not bad, f"scratch in {bad}"
        assert all(k.get("group_segment_fixed_size", 0) <= 80 * 1024 for k in hits), kern  # two workgroups per CU
