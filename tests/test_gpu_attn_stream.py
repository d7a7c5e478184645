"""Streamed attention kernels (csrc/attention_stream.hip) on the MI355X.

The streamed family runs where the LDS-resident kernels refuse a sequence length; ops.mha_force_stream() puts
every launch on it, which is how these tests reach the chunk and block edges at a few dozen tokens.  The chunk
length and the queries per workgroup are read from ops.mha_plan, not written here.

References are full-tensor float64 CPU attention on inputs already rounded to the operand dtype.  Bounds are the
resident kernels' own (tests/test_gpu_kernels.py::test_mha, tests/test_gpu_train.py::test_mha_bwd): forward
max-norm 1e-4 (f32, summation order only) / 7e-3 (bf16 operand rounding of P and the output); backward f32 out 1e-5
and dqkv 1e-4, bf16 relative L2 5e-3; lse within the bound glue_check.lse_reference derives."""
import re

import pytest
import torch
from parity_log import check  # noqa: E402

import glue_check as gk

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
B, H = 2, 2


@pytest.fixture(scope="module")
def T():
    import textmae_amd  # noqa: F401
    from textmae_amd import train_ops

    return train_ops


@pytest.fixture(scope="module")
def ops():
    import textmae_amd  # noqa: F401
    from textmae_amd import ops

    return ops


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    den = b.abs().max().item()
    return (a - b).abs().max().item() / (den if den > 0 else 1.0)


def _rel2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    den = b.norm().item()
    return (a - b).norm().item() / (den if den > 0 else 1.0)


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _sizes(ops, dh, dt, backward=False):
    """(queries per workgroup, chunk length) of the streamed launch, from the plan string"""
    with ops.mha_force_stream():
        plan = ops.mha_plan(33, dh, dt, backward)
    m = re.fullmatch(r"stream<\w+,dh\d+,q(\d+)(?:,k(\d+))?,c(\d+)>", plan)
    assert m, plan
    return int(m.group(1)), int(m.group(3))


def _length(ops, spec, dh, dt, backward=False):
    q, c = _sizes(ops, dh, dt, backward)
    return {"c-1": c - 1, "c": c, "c+1": c + 1, "q+1": q + 1}.get(spec, spec)


def _ref_attn64(qkv, Bn, Tn, Hn, dh):
    q, k, v = qkv.double().reshape(Bn, Tn, 3, Hn, dh).permute(2, 0, 3, 1, 4)
    a = ((q @ k.transpose(-2, -1)) * dh ** -0.5).softmax(-1)
    return (a @ v).transpose(1, 2).reshape(Bn * Tn, Hn * dh)


def _fwd_tol(dt):
    return 1e-4 if dt == F32 else 7e-3


def _run_fwd(T, qkv, Bn, Tn, Hn, dh, dt):
    """out and lse of tmae_mha_fwd_lse, and the output of tmae_mha_fwd (must be the same bits), NaN-filled before"""
    from textmae_amd import ops

    qg = qkv.to(DEV)
    out = torch.full((Bn * Tn, Hn * dh), float("nan"), device=DEV, dtype=dt)
    lse = torch.full((Bn * Hn * Tn,), float("nan"), device=DEV)
    T.mha_lse(qg, Bn, Tn, Hn, dh, dh ** -0.5, dt, out, lse)
    plain = ops.mha(qg, Bn, Tn, Hn, dh, dh ** -0.5, dt)
    torch.cuda.synchronize()
    assert torch.equal(out, plain)
    return out, lse


def _check_fwd(tag, T, qkv, Bn, Tn, Hn, dh, dt):
    out, lse = _run_fwd(T, qkv, Bn, Tn, Hn, dh, dt)
    check(f"rel:stream_out:{tag}", _rel(out.float(), _ref_attn64(qkv, Bn, Tn, Hn, dh)), _fwd_tol(dt))
    ref, bound = gk.lse_reference(qkv, Bn, Tn, Hn, dh, dh ** -0.5)
    ratio = ((lse.double().cpu().reshape(1, -1) - ref).abs() / bound).max().item()
    check(f"lse_over_bound:stream:{tag}", ratio, 1.0, strict=False)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dh", [32, 64, 80])
@pytest.mark.parametrize("spec", [1, 31, 32, 33, 65, "c-1", "c", "c+1", "q+1"])
def test_fwd_forced(T, ops, spec, dh, dt):
    """hook on: tile, chunk and query-block edges of the streamed forward"""
    Tn = _length(ops, spec, dh, dt)
    qkv = _rnd(B * Tn, 3 * H * dh, seed=Tn + dh, scale=1.5).to(dt)
    with ops.mha_force_stream():
        assert "stream" in ops.mha_plan(Tn, dh, dt)
        _check_fwd(f"T{Tn}:dh{dh}", T, qkv, B, Tn, H, dh, dt)


def test_fwd_forced_at_a_shared_shape(T, ops):
    """(145, 64) bf16 is a shape both families take: the streamed output meets the same bound (no bitwise claim)"""
    qkv = _rnd(B * 145, 3 * H * 64, seed=145, scale=1.5).to(BF16)
    with ops.mha_force_stream():
        _check_fwd("shared:T145:dh64", T, qkv, B, 145, H, 64, BF16)


@pytest.mark.parametrize("Tn,dh,dt", [(577, 32, F32), (577, 32, BF16), (1025, 64, F32), (1025, 64, BF16),
                                      (513, 80, F32), (513, 80, BF16), (289, 64, F32)])
def test_fwd_long(T, ops, Tn, dh, dt):
    """hook off: the lengths the resident kernels refuse (each raised "sequence length ... too long" before)"""
    assert "stream" in ops.mha_plan(Tn, dh, dt)
    qkv = _rnd(B * Tn, 3 * H * dh, seed=Tn + dh, scale=1.5).to(dt)
    _check_fwd(f"long:T{Tn}:dh{dh}", T, qkv, B, Tn, H, dh, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("where", ["chunk2_first_tile", "chunk_last_tile", "ragged_last_tile"])
@pytest.mark.parametrize("spike", [12.0, 40.0])
def test_fwd_rescale(T, ops, where, spike, dt):
    """The running-max rescale across tiles and chunks.  One K row is aligned with one Q row so that this query's
    score there exceeds everything before it by `spike` (17 / 58 in log2 units, both past the deferred-rescale
    threshold of 8): chunk2_first_tile forces the rescale of O and l carried in registers over a chunk boundary,
    chunk_last_tile a rescale followed by a restaged chunk that must keep the new max, ragged_last_tile a rescale
    in the one masked tile; in all three every earlier tile's maximum (scores of order 1) is far below the spike,
    so O and l shrink by 2^-17 or 2^-58 and the spiked key dominates the row."""
    dh = 64
    _, c = _sizes(ops, dh, dt)
    Tn = 2 * c + 17
    key = {"chunk2_first_tile": c, "chunk_last_tile": c - 1, "ragged_last_tile": Tn - 1}[where]
    qrow = 40  # second wave of the first query block
    qkv = _rnd(B * Tn, 3 * H * dh, seed=7, scale=0.5).reshape(B, Tn, 3, H, dh)
    qv = qkv[:, qrow, 0]  # [B][H][dh]
    # scale q.k = spike: k = q * spike / (scale |q|^2)
    qkv[:, key, 1] = qv * (spike / (dh ** -0.5 * (qv * qv).sum(-1, keepdim=True)))
    qkv = qkv.reshape(B * Tn, 3 * H * dh).to(dt)
    with ops.mha_force_stream():
        _check_fwd(f"rescale:{where}:{spike:g}", T, qkv, B, Tn, H, dh, dt)
        out, _ = _run_fwd(T, qkv, B, Tn, H, dh, dt)
    # the spiked row is (nearly) the spiked key's V row
    v = qkv.float().reshape(B, Tn, 3, H, dh)[:, key, 2].reshape(B, H * dh)
    got = out.float().cpu().reshape(B, Tn, H * dh)[:, qrow]
    assert _rel(got, v) < 2e-2


# ------------------------------------------------------------------------------------------------ backward
def _autograd(qkv, do, Bn, Tn, Hn, dh):
    D = Hn * dh
    q_ = qkv.double().clone().requires_grad_(True)
    t = q_.reshape(Bn, Tn, 3, Hn, dh).permute(2, 0, 3, 1, 4)
    att = ((t[0] @ t[1].transpose(-2, -1)) * dh ** -0.5).softmax(-1)
    o = (att @ t[2]).transpose(1, 2).reshape(Bn * Tn, D)
    (o * do.double()).sum().backward()
    return o.detach(), q_.grad


def _run_bwd(T, ops, qkv, do, Bn, Tn, Hn, dh, dt, fwd_stream, bwd_stream):
    """forward (+ lse) and backward, each on the family asked for (None: the dispatch's own choice)"""
    D = Hn * dh
    scale = dh ** -0.5
    qg, dg = qkv.to(DEV), do.to(DEV)
    out = torch.full((Bn * Tn, D), float("nan"), device=DEV, dtype=dt)
    lse = torch.full((Bn * Hn * Tn,), float("nan"), device=DEV)

    def family(on):
        return ops.mha_force_stream(bool(on)) if on is not None else ops.mha_force_stream(False)

    with family(fwd_stream):
        if fwd_stream is not None:
            assert ("stream" in ops.mha_plan(Tn, dh, dt)) == fwd_stream
        T.mha_lse(qg, Bn, Tn, Hn, dh, scale, dt, out, lse)
    dq = torch.full((Bn * Tn, 3 * D), float("nan"), device=DEV, dtype=dt)
    dq2 = torch.full((Bn * Tn, 3 * D), float("nan"), device=DEV, dtype=dt)
    with family(bwd_stream):
        if bwd_stream is not None:
            assert ("stream" in ops.mha_plan(Tn, dh, dt, True)) == bwd_stream
        T.mha_bwd(qg, out, dg, lse, dq, Bn, Tn, Hn, dh, scale, dt)
        T.mha_bwd(qg, out, dg, lse, dq2, Bn, Tn, Hn, dh, scale, dt)
    torch.cuda.synchronize()
    assert torch.equal(dq, dq2)  # fixed summation order: bitwise reproducible (NaN anywhere would fail this too)
    return out, dq


def _check_bwd(tag, T, ops, Bn, Tn, Hn, dh, dt, fwd_stream, bwd_stream):
    D = Hn * dh
    qkv = _rnd(Bn * Tn, 3 * D, seed=21).to(dt)
    do = _rnd(Bn * Tn, D, seed=22).to(dt)
    o_ref, g_ref = _autograd(qkv, do, Bn, Tn, Hn, dh)
    out, dq = _run_bwd(T, ops, qkv, do, Bn, Tn, Hn, dh, dt, fwd_stream, bwd_stream)
    if dt == F32:
        check(f"_rel:stream_out:{tag}", _rel(out, o_ref), 1e-5)
        check(f"_rel:stream_dq:{tag}", _rel(dq, g_ref), 1e-4)
    else:
        check(f"_rel2:stream_dq:{tag}", _rel2(dq.float(), g_ref), 5e-3)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("dh", [32, 64, 80])
@pytest.mark.parametrize("spec", [1, 32, 33, 65, "c+1"])
def test_bwd_forced(T, ops, spec, dh, dt):
    """hook on: streamed forward with lse into the streamed backward"""
    Tn = _length(ops, spec, dh, dt, backward=True)
    _check_bwd(f"T{Tn}:dh{dh}", T, ops, B, Tn, H, dh, dt, True, True)


def test_bwd_forced_past_a_key_block(T, ops):
    """more keys than one dK / dV workgroup holds and more queries than one dQ workgroup: two blocks of each"""
    q, _ = _sizes(ops, 32, BF16, backward=True)
    _check_bwd(f"T{q + 1}:dh32", T, ops, B, q + 1, H, 32, BF16, True, True)


@pytest.mark.parametrize("Tn,dh,dt", [(257, 64, BF16), (577, 32, F32), (577, 32, BF16), (1025, 64, BF16)])
def test_bwd_long(T, ops, Tn, dh, dt):
    """hook off: the lengths the resident backward refuses; at (257, 64) bf16 the forward is a resident kernel and
    its lse feeds the streamed backward"""
    assert "stream" in ops.mha_plan(Tn, dh, dt, True)
    assert ("stream" in ops.mha_plan(Tn, dh, dt)) == (Tn != 257)
    _check_bwd(f"long:T{Tn}:dh{dh}", T, ops, 1, Tn, H, dh, dt, None, None)


@pytest.mark.parametrize("fwd_stream,bwd_stream", [(True, False), (False, True)])
def test_mixed_families(T, ops, fwd_stream, bwd_stream):
    """(145, 64) bf16: a forward of one family feeds the backward of the other (the same base-2 lse)"""
    _check_bwd(f"mixed:fwd{int(fwd_stream)}:bwd{int(bwd_stream)}", T, ops, B, 145, H, 64, BF16, fwd_stream, bwd_stream)
