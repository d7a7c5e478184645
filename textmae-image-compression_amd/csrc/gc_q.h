// Per-element arithmetic of the per-image quantiser step on y, shared by the coding
// kernels (coding.hip), the forward / backward at a step (coding.hip, train.hip) and the chained slice stacks
// (lic_stack.hip), so that what a model is trained and evaluated on is bit for bit what the coder does:
// symbols rint((y - mu) / delta), reconstruction fl(fl(qi delta) + mu), entropy model at max(sigma / delta, bound).
// The reference has no counterpart.  Encoder and decoder must produce the same bits, and the tests restate the
// arithmetic in numpy f32, so every operation is rounded on its own: the helpers are compiled with contraction off
// (the __fmul_rn / __fadd_rn forms of the HIP headers are plain operators, which the default -ffp-contract=fast
// may still fuse into one fma after inlining; the pragma is what keeps the product rounded).
#pragma once
#include "common.h"

struct GcqElem { float qi, yhat, s; };

__device__ __forceinline__ float gcq_recon(float qi, float mv, float delta) {
#pragma clang fp contract(off)
  const float p = qi * delta;
  return p + mv;
}

__device__ __forceinline__ float gcq_scale(float sv, float delta, float bound) { return fmaxf(sv / delta, bound); }

__device__ __forceinline__ GcqElem gcq_quantize(float yv, float mv, float sv, float delta, float bound) {
#pragma clang fp contract(off)
  const float d = yv - mv;
  const float qi = rintf(d / delta);
  return GcqElem{qi, gcq_recon(qi, mv, delta), gcq_scale(sv, delta, bound)};
}

// build_indexes on the scale at a step (shared by coding.hip and coding_qmap.hip)
__device__ __forceinline__ int gcq_index(float s, const float* __restrict__ scale_table, int nscale) {
  int id = nscale - 1;
  for (int t = 0; t < nscale - 1; ++t) id -= (s <= scale_table[t]) ? 1 : 0;
  return id;
}

// the symbol's probability mass under N(0, s): the table entry the coder approximates
__device__ __forceinline__ float gcq_likelihood(float qi, float s) {
  const float val = fabsf(qi);
  const float k = -0.70710678118654752440f;
  const float up = 0.5f * erfcf(k * ((0.5f - val) / s));
  const float lo = 0.5f * erfcf(k * ((-0.5f - val) / s));
  return fmaxf(up - lo, 1e-9f);
}

// t = (y - mu) / delta, the value gcq_quantize rounds (the training forward adds the noise to it)
__device__ __forceinline__ float gcq_scaled(float yv, float mv, float delta) {
#pragma clang fp contract(off)
  const float d = yv - mv;
  return d / delta;
}

// the training likelihood: gcq_likelihood's form at v = |t + noise|
__device__ __forceinline__ float gcq_likelihood_noisy(float t, float nz, float s) {
  const float val = fabsf(t + nz);
  const float k = -0.70710678118654752440f;
  const float up = 0.5f * erfcf(k * ((0.5f - val) / s));
  const float lo = 0.5f * erfcf(k * ((-0.5f - val) / s));
  return fmaxf(up - lo, 1e-9f);
}
