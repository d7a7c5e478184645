"""Host side of the device input pipeline (CPU only): ops.resize_tables restates Pillow's precompute_coeffs +
normalize_coeffs_8bpc, so the tables applied in numpy -- horizontal pass, then vertical, uint8 between them, the
arithmetic csrc/resize.hip runs -- equal PIL.Image.resize bit for bit; and tmae_resize_u8 / tmae_rgb_to_gray_u8
validate their arguments on the host before any launch."""
import ctypes

import numpy as np
import pytest
from PIL import Image

# (H, W) of the source -> PIL's (Wo, Ho)
SHAPES = [((512, 768), (224, 224)), ((37, 53), (224, 224)), ((224, 224), (768, 512)), ((100, 300), (17, 333)),
          ((16, 16), (16, 16)), ((1, 5), (7, 3))]
FILTERS = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}


def apply_tables(a, tables):
    """one pass along axis 1 of a uint8 [rows][cols][3]: clip8((2^21 + sum px * k) >> 22) in int32"""
    kk, bounds = tables
    out = np.empty((a.shape[0], kk.shape[0], a.shape[2]), dtype=np.uint8)
    a64 = a.astype(np.int64)
    for xo in range(kk.shape[0]):
        x0, n = bounds[xo]
        acc = (1 << 21) + np.tensordot(a64[:, x0:x0 + n], kk[xo, :n].astype(np.int64), axes=([1], [0]))
        assert np.abs(acc).max() < 2 ** 31  # the sum fits int32, as in Pillow
        out[:, xo] = np.clip(acc >> 22, 0, 255)
    return out


def resize_numpy(ops, a, Wo, Ho, filt):
    H, W, _ = a.shape
    if W != Wo:
        a = apply_tables(a, ops.resize_tables(W, Wo, filt))
    if H != Ho:
        a = apply_tables(a.transpose(1, 0, 2), ops.resize_tables(H, Ho, filt)).transpose(1, 0, 2)
    return a


@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("hw,size", SHAPES, ids=[f"{h}x{w}-to-{s[1]}x{s[0]}" for (h, w), s in SHAPES])
def test_tables_equal_pil(tmae, hw, size, filt):
    rng = np.random.default_rng(hw[0] * 1000 + hw[1])
    a = rng.integers(0, 256, (*hw, 3), dtype=np.uint8)
    ref = np.array(Image.fromarray(a).resize(size, FILTERS[filt]))
    got = resize_numpy(tmae.ops, a, size[0], size[1], filt)
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("sizes", [(768, 224), (53, 224), (224, 768), (300, 17), (2040, 256), (16, 16), (1, 7), (5, 3)])
def test_table_invariants(tmae, sizes, filt):
    import math

    n_in, n_out = sizes
    kk, bounds = tmae.ops.resize_tables(n_in, n_out, filt)
    support = (2.0 if filt == "bicubic" else 1.0) * max(n_in / n_out, 1.0)
    ksize = int(math.ceil(support)) * 2 + 1
    assert kk.dtype == np.int32 and bounds.dtype == np.int32
    assert kk.shape == (n_out, ksize) and bounds.shape == (n_out, 2)
    # every weight is rounded to 2^-22 once, so a row sums to 2^22 within half a unit per tap
    assert np.all(np.abs(kk.sum(axis=1, dtype=np.int64) - (1 << 22)) <= ksize)
    xmin, n = bounds[:, 0], bounds[:, 1]
    assert np.all(xmin >= 0) and np.all(n >= 1) and np.all(n <= ksize) and np.all(xmin + n <= n_in)
    for xo in range(n_out):
        assert not kk[xo, n[xo]:].any()
    assert tmae.ops.resize_tables(n_in, n_out, filt)[0] is kk  # cached per (in, out, filter)


def test_wide_tap_counts(tmae):
    """the tap loop's trip count comes from the table: 33 at 2040 -> 256, 73 at 300 -> 17"""
    assert tmae.ops.resize_tables(2040, 256)[0].shape[1] == 33
    assert tmae.ops.resize_tables(300, 17)[0].shape[1] == 73


def test_tables_reject_bad_arguments(tmae):
    with pytest.raises(ValueError, match="sizes must be >= 1"):
        tmae.ops.resize_tables(0, 4)
    with pytest.raises(ValueError, match="unknown filter"):
        tmae.ops.resize_tables(8, 4, "lanczos")


def _resize_args(n=1, H=8, W=8, Ho=4, Wo=4, tables=True, mode=0, work_bytes=None, mean_std=True):
    """argument list of tmae_resize_u8 with fake (never dereferenced) non-NULL addresses"""
    t = 0x1000 if tables else None
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5) if mean_std else None
    need = n * H * Wo * 3
    return [0x1000, n, H, W, Ho, Wo, t, 0x1000, 5, 0x1000, 0x1000, 5, mode, f3, f3, 0x1000, 0x1000,
            need if work_bytes is None else work_bytes, None]


def test_resize_abi_validation(tmae):
    """every check runs on the host before any launch: a status and a message, no GPU needed"""
    from textmae_amd import _lib

    tmae.load_library()
    assert _lib.value("tmae_resize_u8_workspace", 2, 8, 8, 4, 4) == 2 * 8 * 4 * 3
    assert _lib.value("tmae_resize_u8_workspace", 2, 8, 8, 8, 4) == 0  # one pass: no intermediate
    assert _lib.value("tmae_resize_u8_workspace", 2, 8, 8, 4, 8) == 0
    with pytest.raises(ValueError, match="sizes must be >= 1"):
        _lib.call("tmae_resize_u8", *_resize_args(Wo=0))
    with pytest.raises(ValueError, match="sizes must be >= 1"):
        _lib.call("tmae_resize_u8", *_resize_args(n=0))
    with pytest.raises(ValueError, match="table is NULL"):
        _lib.call("tmae_resize_u8", *_resize_args(tables=False))
    with pytest.raises(ValueError, match="workspace too small"):
        _lib.call("tmae_resize_u8", *_resize_args(work_bytes=8 * 4 * 3 - 1))
    with pytest.raises(ValueError, match="unknown output mode"):
        _lib.call("tmae_resize_u8", *_resize_args(mode=3))
    with pytest.raises(ValueError, match="mean / std are NULL"):
        _lib.call("tmae_resize_u8", *_resize_args(mode=2, mean_std=False))
    with pytest.raises(ValueError, match="at least one pixel"):
        _lib.call("tmae_rgb_to_gray_u8", 0x1000, 0, 0x1000, None)
    with pytest.raises(ValueError, match="NULL"):
        _lib.call("tmae_rgb_to_gray_u8", None, 16, 0x1000, None)
