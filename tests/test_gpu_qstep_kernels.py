"""tmae_gc_slices_code_q / tmae_gc_indexes_q / tmae_gc_dequantize_q (csrc/coding.hip) element by
element against the numpy f32 restatement of tests/qstep_check.py.

n = 3 images at q = (-32, 0, 11): steps 1/16, 1 and 2^(11/8).  HW = 16, sw = 16 with 1, 2 and 6 slices runs the
LDS-tiled kernel, HW = 324 (324 x 17 floats > the 4800 of the LDS tile) the element kernel.  Symbols, indexes and both
y_hat outputs are compared bit for bit, no element skipped; the likelihood against the restatement with
entropy_check's E bound.  The classes planted per image are counted on the CPU by test_qstep_host.py."""
import pytest
import torch

import entropy_check as ek
import glue_check as gk
import qstep_check as qk
from glue_check import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def tname(dt):
    return "bf16" if dt == BF16 else "f32"


def qdev(q):
    return None if q is None else torch.tensor(q, dtype=torch.int32, device=DEV)


def launch(tmae, c, yt, q, yhat32=True, lik=True):
    inp = ek.gcf_inputs(c, False, DEV)
    o = ek.gcf_outputs(c, yt, True, DEV, yhat32)
    y32, ld32 = (o.yhat32.view(), o.yhat32.ld) if yhat32 else (None, 0)
    tmae.ops.gc_slices_code_q(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms,
                              o.lik.view() if lik else None, c.Mtot, o.yhat.view(), yt, o.yhat.ld, y32, ld32, c.n, c.HW,
                              c.nsl, c.sw, o.sym.view(), o.idx.view(), dev(c.table), 0.11, qdev(q))
    torch.cuda.synchronize()
    return inp, o


def check_outputs(tag, c, o, out, yt, yhat32, lik):
    ek.check_exact(f"{tag}:symbols", o.sym, out["sym"])
    ek.check_exact(f"{tag}:indexes", o.idx, out["idx"])
    ek.check_bits(f"{tag}:yhat", o.yhat, qk.yhat_values(c, out, yt))
    if yhat32:
        ek.check_bits(f"{tag}:yhat32", o.yhat32, out["yhat32"])
    if lik:
        gk.check(f"{tag}:lik", o.lik, *out["lik"])
    else:  # NULL: nothing of the buffer the test holds was written
        ref = ek.to_nchw(c.lik0, c.n, c.HW).reshape(1, -1)
        ek.check_bits(f"{tag}:lik_untouched", o.lik, ref)


@pytest.mark.parametrize("lik", [True, False])
@pytest.mark.parametrize("yhat32", [True, False])
@pytest.mark.parametrize("yt", [F32, BF16])
@pytest.mark.parametrize("shape", list(qk.SHAPES))
def test_code_q_against_restatement(tmae, shape, yt, yhat32, lik):
    c = qk.case(shape)
    out, _ = qk.reference(shape)
    inp, o = launch(tmae, c, yt, c.q, yhat32, lik)
    tag = f"gc_slices_code_q:{shape}:{tname(yt)}"
    check_outputs(tag, c, o, out, yt, yhat32, lik)
    total = c.nsl * c.M * c.sw
    # the decoder's two kernels: the same indexes from sigma, the same y_hat from the symbols
    idx = ek.GuardedInt(1, total, device=DEV)
    tmae.ops.gc_indexes_q(inp.sigma, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, dev(c.table), 0.11, idx.view(),
                          qdev(c.q))
    d = ek.gcf_outputs(c, yt, False, DEV, yhat32)
    y32, ld32 = (d.yhat32.view(), d.yhat32.ld) if yhat32 else (None, 0)
    tmae.ops.gc_dequantize_q(o.sym.view(), inp.mu, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, c.yoff, d.yhat.view(),
                             yt, d.yhat.ld, y32, ld32, qdev(c.q))
    torch.cuda.synchronize()
    ek.check_exact(f"gc_indexes_q:{shape}", idx, out["idx"])
    ek.check_bits(f"gc_dequantize_q:{shape}:yhat:{tname(yt)}", d.yhat, qk.yhat_values(c, out, yt))
    assert torch.equal(d.yhat.block().cpu(), o.yhat.block().cpu())  # bitwise, bf16 included
    if yhat32:
        ek.check_bits(f"gc_dequantize_q:{shape}:yhat32", d.yhat32, out["yhat32"])
        assert torch.equal(d.yhat32.block().cpu(), o.yhat32.block().cpu())


@pytest.mark.parametrize("q", [None, (0, 0, 0)], ids=["null", "zeros"])
@pytest.mark.parametrize("yt", [F32, BF16])
@pytest.mark.parametrize("shape", ["tiled2", "tiled6", "element2"])
def test_step_one_is_the_existing_kernels(tmae, shape, yt, q):
    """q = NULL and q = (0, 0, 0): the restatement, and bit for bit what tmae_gc_slices_code / tmae_gc_indexes /
    tmae_gc_dequantize give on the same buffers (the likelihood excepted: the existing kernel takes |y_hat - mu|,
    this one |qi|)"""
    c = qk.case(shape, None)
    out, _ = qk.reference(shape, None)
    inp, o = launch(tmae, c, yt, q)
    check_outputs(f"gc_slices_code_q:{shape}:q0:{tname(yt)}", c, o, out, yt, True, True)
    old = ek.gcf_outputs(c, yt, True, DEV, True)
    tmae.ops.gc_slices_code(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, old.lik.view(), c.Mtot,
                            old.yhat.view(), yt, old.yhat.ld, old.yhat32.view(), old.yhat32.ld, c.n, c.HW, c.nsl, c.sw,
                            old.sym.view(), old.idx.view(), dev(c.table))
    total = c.nsl * c.M * c.sw
    idx_old, idx_new = ek.GuardedInt(1, total, device=DEV), ek.GuardedInt(1, total, device=DEV)
    tmae.ops.gc_indexes(inp.sigma, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, dev(c.table), 0.11, idx_old.view())
    tmae.ops.gc_indexes_q(inp.sigma, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, dev(c.table), 0.11, idx_new.view(),
                          qdev(q))
    d_old, d_new = ek.gcf_outputs(c, yt, False, DEV), ek.gcf_outputs(c, yt, False, DEV)
    tmae.ops.gc_dequantize(old.sym.view(), inp.mu, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, c.yoff,
                           d_old.yhat.view(), yt, d_old.yhat.ld, d_old.yhat32.view(), d_old.yhat32.ld)
    tmae.ops.gc_dequantize_q(o.sym.view(), inp.mu, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, c.yoff,
                             d_new.yhat.view(), yt, d_new.yhat.ld, d_new.yhat32.view(), d_new.yhat32.ld, qdev(q))
    torch.cuda.synchronize()
    for name, a, b in (("symbols", o.sym, old.sym), ("indexes", o.idx, old.idx), ("yhat", o.yhat, old.yhat),
                       ("yhat32", o.yhat32, old.yhat32), ("gc_indexes", idx_new, idx_old),
                       ("dequantize yhat", d_new.yhat, d_old.yhat), ("dequantize yhat32", d_new.yhat32, d_old.yhat32)):
        assert a.guard_hits() == 0 and b.guard_hits() == 0, name
        assert torch.equal(a.block().cpu(), b.block().cpu()), name


def test_other_scale_bound(tmae):
    """scale_bound = 0.25: the bound is the kernels' argument and is applied to sigma / delta, not to sigma"""
    c = qk.case("tiled2")
    out, _ = qk.reference("tiled2", qk.Q3, 0.25)
    assert int((out["idx"] != qk.reference("tiled2")[0]["idx"]).sum()) >= 4
    inp = ek.gcf_inputs(c, False, DEV)
    o = ek.gcf_outputs(c, F32, True, DEV, True)
    tmae.ops.gc_slices_code_q(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, o.lik.view(), c.Mtot,
                              o.yhat.view(), F32, o.yhat.ld, o.yhat32.view(), o.yhat32.ld, c.n, c.HW, c.nsl, c.sw,
                              o.sym.view(), o.idx.view(), dev(c.table), 0.25, qdev(c.q))
    idx = ek.GuardedInt(1, c.nsl * c.M * c.sw, device=DEV)
    tmae.ops.gc_indexes_q(inp.sigma, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, dev(c.table), 0.25, idx.view(),
                          qdev(c.q))
    torch.cuda.synchronize()
    ek.check_exact("gc_slices_code_q:bound0.25:indexes", o.idx, out["idx"])
    ek.check_exact("gc_indexes_q:bound0.25", idx, out["idx"])
    gk.check("gc_slices_code_q:bound0.25:lik", o.lik, *out["lik"])


def test_q_of_the_wrong_length_or_type(tmae):
    c = qk.case("tiled1")
    inp = ek.gcf_inputs(c, False, DEV)
    idx = ek.GuardedInt(1, c.nsl * c.M * c.sw, device=DEV)
    args = (inp.sigma, c.ms_stride, c.ld_ms, c.n, c.HW, c.nsl, c.sw, dev(c.table), 0.11, idx.view())
    with pytest.raises(ValueError, match=r"q holds 2 entries for 3 images"):
        tmae.ops.gc_indexes_q(*args, qdev((0, 1)))
    with pytest.raises(ValueError, match=r"q must be torch.int32"):
        tmae.ops.gc_indexes_q(*args, torch.zeros(3, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    assert idx.guard_hits() == 0 and int((idx.block() != ek.SENTINEL).sum()) == 0  # nothing was launched
