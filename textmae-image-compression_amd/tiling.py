"""Tile geometry of the full-resolution codec: the one definition the kernels (csrc/tile.hip),
the container (bitstream.parse_image) and MCM.encode_image / decode_image share, and its numpy restatement.

An image of H x W pixels is coded as overlapping S x S tiles (S = the model's img_size), overlap 0 <= O <= S // 2,
stride = S - O:

  * nx = max(1, ceil((W - O) / stride)), ny likewise from H, T = nx * ny <= MAX_TILES;
  * tile t = ty * nx + tx (row-major) has its origin at (ty * stride, tx * stride);
  * tiles may reach past the image: a sample outside it is the nearest edge pixel (coordinates clamped to
    [0, H - 1] / [0, W - 1]), which is defined for every size, H < S included;
  * the grid is regular and O <= S / 2, so at most two tiles cover a pixel per axis and every overlap is O wide;
  * blend weight per axis at tile-local coordinate i: i + 1 when i < O and the tile has a neighbour before it,
    S - i when i >= S - O and it has a neighbour after it, otherwise O + 1.  In an overlap the earlier tile is at
    local S - O + k and the later at k (0 <= k < O): (O - k) + (k + 1) = O + 1, so the weights over the tiles
    covering a pixel sum to O + 1 per axis and their 2-D products to (O + 1)^2;
  * a pixel's column tiles: tx_hi = min(x // stride, nx - 1), and tx_hi - 1 as well when tx_hi > 0 and
    x - tx_hi * stride < O.  Rows the same.

``region_tiles`` names the tiles a window of the image needs (region decode).

``tile_cut_host`` / ``tile_blend_host`` restate the two kernels in f64 numpy, straight from the lines above; the
tests use them as the oracle.  Nothing here touches the device.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

MAX_TILES = 4096


class Grid(NamedTuple):
    H: int
    W: int
    S: int
    O: int
    stride: int
    ny: int
    nx: int

    @property
    def T(self) -> int:
        return self.ny * self.nx

    def origin(self, t: int):
        """(y0, x0) of tile t"""
        ty, tx = divmod(int(t), self.nx)
        return ty * self.stride, tx * self.stride


def _count(extent: int, O: int, stride: int) -> int:
    return max(1, -(-(extent - O) // stride))


def grid(H, W, S, O) -> Grid:
    """the tile grid of an H x W image; ValueError on sizes the format does not hold"""
    H, W, S, O = int(H), int(W), int(S), int(O)
    if H < 1 or W < 1:
        raise ValueError(f"image of {H}x{W} pixels: both sizes must be >= 1")
    if S < 1:
        raise ValueError(f"tile size {S} must be >= 1")
    if not 0 <= O <= S // 2:
        raise ValueError(f"overlap {O} outside 0..{S // 2} (half the tile size {S})")
    stride = S - O
    ny, nx = _count(H, O, stride), _count(W, O, stride)
    if ny * nx > MAX_TILES:
        raise ValueError(f"{ny} x {nx} tiles: at most {MAX_TILES}")
    return Grid(H, W, S, O, stride, ny, nx)


def axis_weights(k: int, n: int, S: int, O: int) -> np.ndarray:
    """int64 [S]: the blend weights of tile index k (of n) along one axis"""
    i = np.arange(S)
    w = np.full(S, O + 1, dtype=np.int64)
    if k > 0:
        w[i < O] = i[i < O] + 1
    if k < n - 1:
        w[i >= S - O] = S - i[i >= S - O]
    return w


def covering(c: int, n: int, stride: int, O: int):
    """tile indices along one axis that cover coordinate c, ascending"""
    hi = min(c // stride, n - 1)
    return [hi - 1, hi] if hi > 0 and c - hi * stride < O else [hi]


def region_tiles(g: Grid, x0, y0, w, h):
    """ascending tile indices whose blend contributes to any pixel of the window [x0, x0 + w) x [y0, y0 + h) of grid
    g.  covering() grows with the coordinate, so per axis the tiles are the contiguous range from
    covering(first)[0] to covering(last)[-1], and the result is the row-major rectangle of the two ranges.
    ValueError for an empty window or one that is not wholly inside the image."""
    x0, y0, w, h = int(x0), int(y0), int(w), int(h)
    if w < 1 or h < 1:
        raise ValueError(f"window of {w}x{h} pixels: both sizes must be >= 1")
    if x0 < 0 or y0 < 0 or x0 + w > g.W or y0 + h > g.H:
        raise ValueError(f"window {w}x{h} at ({x0}, {y0}) is not inside the image of {g.W}x{g.H} pixels")
    tx0, tx1 = covering(x0, g.nx, g.stride, g.O)[0], covering(x0 + w - 1, g.nx, g.stride, g.O)[-1]
    ty0, ty1 = covering(y0, g.ny, g.stride, g.O)[0], covering(y0 + h - 1, g.ny, g.stride, g.O)[-1]
    return [ty * g.nx + tx for ty in range(ty0, ty1 + 1) for tx in range(tx0, tx1 + 1)]


def tile_cut_host(img, S, O) -> np.ndarray:
    """img [H, W, C] (any dtype) -> tiles [T, S, S, C] of the same dtype: tmae_tile_cut_u8's gather"""
    a = np.asarray(img)
    g = grid(a.shape[0], a.shape[1], S, O)
    out = np.empty((g.T, S, S) + a.shape[2:], dtype=a.dtype)
    for t in range(g.T):
        y0, x0 = g.origin(t)
        ys = np.minimum(y0 + np.arange(S), g.H - 1)
        xs = np.minimum(x0 + np.arange(S), g.W - 1)
        out[t] = a[ys[:, None], xs[None, :]]
    return out


def tile_blend_host(tiles, H, W, O) -> np.ndarray:
    """tiles [T, C, S, S] -> f64 [C, H, W]: tmae_tile_blend in f64 (weighted sum over the covering tiles divided by
    (O + 1)^2; a pixel one tile covers is that tile's value)"""
    t = np.asarray(tiles, dtype=np.float64)
    S = t.shape[-1]
    g = grid(H, W, S, O)
    if t.ndim != 4 or t.shape[0] != g.T or t.shape[2] != S:
        raise ValueError(f"tile_blend_host: tiles must be [{g.T}, C, {S}, {S}], got {t.shape}")
    acc = np.zeros((t.shape[1], H, W), dtype=np.float64)
    cover = np.zeros((H, W), dtype=np.int64)
    for k in range(g.T):
        ty, tx = divmod(k, g.nx)
        y0, x0 = g.origin(k)
        h, w = min(S, H - y0), min(S, W - x0)  # the part of the tile inside the image
        if h <= 0 or w <= 0:
            continue
        wy, wx = axis_weights(ty, g.ny, S, O)[:h], axis_weights(tx, g.nx, S, O)[:w]
        acc[:, y0:y0 + h, x0:x0 + w] += (wy[:, None] * wx[None, :]).astype(np.float64) * t[k, :, :h, :w]
        cover[y0:y0 + h, x0:x0 + w] += 1
    out = acc / float((O + 1) ** 2)
    # singly-covered pixels: the tile's value itself (weight (O + 1)^2 over (O + 1)^2)
    for k in range(g.T):
        y0, x0 = g.origin(k)
        h, w = min(S, H - y0), min(S, W - x0)
        if h <= 0 or w <= 0:
            continue
        one = cover[y0:y0 + h, x0:x0 + w] == 1
        out[:, y0:y0 + h, x0:x0 + w][:, one] = t[k, :, :h, :w][:, one]
    return out
