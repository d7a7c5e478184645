// Rate-distortion optimised quantisation of y at encode time: per element one candidate besides the
// rounded symbol, one step toward zero, taken when the bits it saves through the element's own CDF row, weighted by
// w, exceed the latent error it adds.  Every operation is rounded to f32 on its own (contraction off, as gc_q.h), so
// that the numpy f32 restatement of tests/rdoq_check.py is bit exact:
//
//   t    = fl(fl(y - mu) / delta)          gcq_scaled
//   qi0  = rint(t)                         the symbol of plain rounding
//   if qi0 == 0: keep qi0
//   qi1  = qi0 - copysign(1, qi0)          the one candidate: one step toward zero
//   e0 = qi0 - t;  e1 = qi1 - t
//   dd   = fl(fl(e1 e1) - fl(e0 e0))       >= 0
//   rhs  = fl(fl(delta delta) dd)
//   lhs  = fl(w fl(bits(r, qi0) - bits(r, qi1)))
//   qi   = qi1 if lhs > rhs else qi0       strict: w = 0 is plain rounding bit for bit
//   y_hat = gcq_recon(qi, mu, delta);  r = gcq_index(gcq_scale(...)), unchanged
//
// bits(r, v) is what the coder spends on v through row r, read from a host-built f32 table B[r][k] =
// 16 - log2(cdf[r][k + 1] - cdf[r][k]) (no log2 runs here), with the clamp and escape rule of enc_clamp_escape
// (rans_device.hip): value = v - offset[r]; inside [0, size_r - 2) it costs B[r][value], otherwise the escape symbol
// B[r][size_r - 2] plus 4 (1 + ndig) bits, ndig the 4-bit digits of raw = -2 value - 1 below the support and
// 2 (value - max_value) above it.  The decoder needs nothing: it reads the symbols the encoder chose.  The reference
// has no counterpart.
#pragma once
#include "common.h"
#include "gc_q.h"

// row: B[r]; the row's size comes from a device table, so it is clamped into the row before anything is indexed
__device__ __forceinline__ float gcr_bits(const float* __restrict__ row, int rate_stride, int size, int off, int v) {
#pragma clang fp contract(off)
  const int max_value = min(max(size - 2, 0), rate_stride - 1);
  const int value = (int)((uint32_t)v - (uint32_t)off);
  if (value >= 0 && value < max_value) return row[value];
  const uint32_t raw =
      value < 0 ? (uint32_t)(-2 * (long long)value - 1) : (uint32_t)(2 * (long long)(value - max_value));
  const uint32_t ndig = raw ? 8u - ((uint32_t)__clz((int)raw) >> 2) : 0u;
  return row[max_value] + 4.0f * (float)(1u + ndig);
}

struct GcrElem { float qi, yhat, s; int idx, flipped; };

__device__ __forceinline__ GcrElem gcr_quantize(float yv, float mv, float sv, float delta, float bound, float w,
                                                const float* __restrict__ scale_table, int nscale,
                                                const float* __restrict__ rate, int rate_stride,
                                                const int* __restrict__ sizes, const int* __restrict__ offs) {
#pragma clang fp contract(off)
  const float t = gcq_scaled(yv, mv, delta);
  const float qi0 = rintf(t);
  const float s = gcq_scale(sv, delta, bound);
  const int r = gcq_index(s, scale_table, nscale);  // in [0, nscale - 1] by construction
  float qi = qi0;
  int flipped = 0;
  if (qi0 != 0.0f) {
    const float qi1 = qi0 - copysignf(1.0f, qi0);
    const float e0 = qi0 - t, e1 = qi1 - t;
    const float a1 = e1 * e1, a0 = e0 * e0;
    const float dd = a1 - a0;
    const float d2 = delta * delta;
    const float rhs = d2 * dd;
    const float* __restrict__ row = rate + (size_t)r * rate_stride;
    const int size = sizes[r], off = offs[r];
    const float db = gcr_bits(row, rate_stride, size, off, (int)qi0) - gcr_bits(row, rate_stride, size, off, (int)qi1);
    const float lhs = w * db;
    if (lhs > rhs) {
      qi = qi1;
      flipped = 1;
    }
  }
  return GcrElem{qi, gcq_recon(qi, mv, delta), s, r, flipped};
}
