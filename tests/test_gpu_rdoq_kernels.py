"""tmae_gc_slices_code_rdo (csrc/coding_rdo.hip) element by element against the numpy f32 restatement
of tests/rdoq_check.py.

n = 3 images at the weights (0, 0.5, 1000).  HW = 16, sw = 16, 2 slices runs the LDS form, HW = 324 the element form;
the step comes per image (q = (-32, 0, 11)), from a map per pixel (three and more steps inside an image) or from
neither (both pointers NULL).  Symbols, indexes, both y_hat outputs and the per-image counts of moved symbols are
compared bit for bit, no element skipped; the likelihood against the restatement at the chosen symbol with
entropy_check's E bound.  The classes planted are counted on the CPU by test_rdoq_host.py."""
import numpy as np
import pytest
import torch

import entropy_check as ek
import glue_check as gk
import qstep_check as qk
import rdoq_check as rk
from glue_check import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(s, m) for s in rk.SHAPES for m in rk.MODES]


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def tname(dt):
    return "bf16" if dt == BF16 else "f32"


def idev(a):
    return None if a is None else torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV).contiguous()


def dev_tables():
    tb = rk.tables()
    return torch.from_numpy(tb.rate).to(DEV), idev(tb.sizes), idev(tb.offsets)


def launch(tmae, c, yt, w, yhat32=True, lik=True, changed=True):
    inp = ek.gcf_inputs(c, False, DEV)
    o = ek.gcf_outputs(c, yt, True, DEV, yhat32)
    o.changed = ek.GuardedInt(1, c.n, device=DEV, init=torch.zeros(1, c.n)) if changed else None
    y32, ld32 = (o.yhat32.view(), o.yhat32.ld) if yhat32 else (None, 0)
    rate, sizes, offsets = dev_tables()
    tmae.ops.gc_slices_code_rdo(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms,
                                o.lik.view() if lik else None, c.Mtot, o.yhat.view(), yt, o.yhat.ld, y32, ld32, c.n,
                                c.HW, c.nsl, c.sw, o.sym.view(), o.idx.view(), dev(c.table), 0.11, idev(c.q),
                                idev(c.qmap), torch.tensor(w, dtype=torch.float32, device=DEV), rate, sizes, offsets,
                                o.changed.view() if changed else None)
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
        ek.check_bits(f"{tag}:lik_untouched", o.lik, ek.to_nchw(c.lik0, c.n, c.HW).reshape(1, -1))
    if o.changed is not None:
        ek.check_exact(f"{tag}:changed", o.changed, out["changed"])


@pytest.mark.parametrize("yt", [F32, BF16])
@pytest.mark.parametrize("shape,mode", CASES)
def test_code_rdo_against_restatement(tmae, shape, mode, yt):
    c = rk.case(shape, mode)
    out, r = rk.reference(shape, mode)
    assert int(out["changed"][1]) > 0 and int(out["changed"][2]) > 0 and int(out["changed"][0]) == 0
    _, o = launch(tmae, c, yt, c.w)
    check_outputs(f"gc_slices_code_rdo:{shape}:{mode}:{tname(yt)}", c, o, out, yt, True, True)


@pytest.mark.parametrize("shape", rk.SHAPES)
def test_optional_outputs(tmae, shape):
    """yhat32, lik and changed NULL: the rest is what it was, and nothing of those buffers is written"""
    c = rk.case(shape, "q")
    out, _ = rk.reference(shape, "q")
    _, o = launch(tmae, c, BF16, c.w, yhat32=False, lik=False, changed=False)
    check_outputs(f"gc_slices_code_rdo:{shape}:q:optional", c, o, out, BF16, False, False)


@pytest.mark.parametrize("yt", [F32, BF16])
@pytest.mark.parametrize("shape,mode", CASES)
def test_weight_zero_is_the_plain_kernels(tmae, shape, mode, yt):
    """w = 0: the restatement at w = 0, and bit for bit what tmae_gc_slices_code_q / _qm give on the same buffers,
    the likelihood included"""
    c = rk.case(shape, mode)
    out, _ = rk.reference(shape, mode, (0.0, 0.0, 0.0))
    inp, o = launch(tmae, c, yt, (0.0, 0.0, 0.0))
    check_outputs(f"gc_slices_code_rdo:{shape}:{mode}:w0:{tname(yt)}", c, o, out, yt, True, True)
    assert int(o.changed.block().abs().sum()) == 0
    old = ek.gcf_outputs(c, yt, True, DEV, True)
    args = (inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, old.lik.view(), c.Mtot, old.yhat.view(), yt,
            old.yhat.ld, old.yhat32.view(), old.yhat32.ld, c.n, c.HW, c.nsl, c.sw, old.sym.view(), old.idx.view(),
            dev(c.table), 0.11)
    if mode == "qmap":
        tmae.ops.gc_slices_code_qm(*args, idev(c.qmap))
    else:
        tmae.ops.gc_slices_code_q(*args, idev(c.q))
    torch.cuda.synchronize()
    for name, a, b in (("symbols", o.sym, old.sym), ("indexes", o.idx, old.idx), ("yhat", o.yhat, old.yhat),
                       ("yhat32", o.yhat32, old.yhat32), ("lik", o.lik, old.lik)):
        assert a.guard_hits() == 0 and b.guard_hits() == 0, name
        assert torch.equal(a.block().cpu(), b.block().cpu()), name


def test_the_two_forms_agree(tmae):
    """the same rows as 3 images of 324 pixels (element form) and as 54 images of 18 pixels (LDS form): inputs, y_hat
    and the map are indexed by the row alone, so the outputs by row must be bitwise equal"""
    import copy

    import qmap_check as qm

    c = rk.case("element2", "qmap")
    d = copy.copy(c)
    d.n, d.HW = 54, 18
    assert d.n * d.HW == c.M and d.HW * (d.sw + 1) <= 4800 < c.HW * (c.sw + 1)
    d.qmap = c.qmap.reshape(d.n, d.HW)
    w = tuple(np.repeat(np.asarray(c.w, dtype=np.float32), 18).tolist())
    _, a = launch(tmae, c, F32, c.w)
    _, b = launch(tmae, d, F32, w)
    for name in ("sym", "idx"):
        assert torch.equal(qm.by_row(c, getattr(a, name).block().cpu()), qm.by_row(d, getattr(b, name).block().cpu())), name
    assert torch.equal(a.yhat.block().cpu(), b.yhat.block().cpu())
    assert torch.equal(a.yhat32.block().cpu(), b.yhat32.block().cpu())
    assert torch.equal(qm.lik_by_row(c, a.lik.block().cpu())[:, c.sl], qm.lik_by_row(d, b.lik.block().cpu())[:, c.sl])
    assert b.changed.guard_hits() == 0
    assert torch.equal(a.changed.block().cpu().reshape(-1), b.changed.block().cpu().reshape(3, 18).sum(dim=1))


def test_arguments_checked_before_the_launch(tmae):
    c = rk.case("tiled2", "q")
    inp = ek.gcf_inputs(c, False, DEV)
    o = ek.gcf_outputs(c, F32, True, DEV, True)
    rate, sizes, offsets = dev_tables()

    def call(w=None, rate=rate, sizes=sizes, q=idev(c.q), qmap=None):
        w = torch.zeros(c.n, dtype=torch.float32, device=DEV) if w is None else w
        tmae.ops.gc_slices_code_rdo(inp.y, c.ldy, c.yoff, inp.mu, inp.sigma, c.ms_stride, c.ld_ms, None, c.Mtot,
                                    o.yhat.view(), F32, o.yhat.ld, None, 0, c.n, c.HW, c.nsl, c.sw, o.sym.view(),
                                    o.idx.view(), dev(c.table), 0.11, q, qmap, w, rate, sizes, offsets, None)

    with pytest.raises(ValueError, match=r"rdo_w holds 2 entries for 3 images"):
        call(w=torch.zeros(2, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match=r"rdo_w must be torch.float32"):
        call(w=torch.zeros(3, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match=r"for 64 scales"):
        call(rate=rate[:63].contiguous())
    with pytest.raises(ValueError, match=r"for 64 scales"):
        call(sizes=sizes[:10].contiguous())
    with pytest.raises(ValueError, match=r"q holds 2 entries for 3 images"):
        call(q=idev((0, 1)))
    with pytest.raises(ValueError, match=r"qmap holds"):
        call(qmap=idev(np.zeros((3, 5))))
    torch.cuda.synchronize()
    assert o.sym.guard_hits() == 0 and int((o.sym.block() != ek.SENTINEL).sum()) == 0  # nothing was launched
