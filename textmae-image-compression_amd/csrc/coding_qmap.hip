// Per-patch quantiser steps on y: the four kernels of coding.hip that take a step per image
// (tmae_gc_slices_code_q / tmae_gc_indexes_q / tmae_gc_dequantize_q / tmae_gc_slices_fwd_q) with the step taken per
// pixel of the latent grid instead, from a map qmap[image][pixel] of clamped ladder positions (tmae_qmap_build,
// qlevels.hip).  g_a is 1x1 convolutions, so pixel p of the grid is kept patch p and a per-pixel step is a per-patch
// step.  Layouts, both launch forms and the per-element arithmetic (gc_q.h) are those of the _q kernels; a translation
// unit of its own, so that coding.hip's code objects stay what they are.  The reference has no counterpart.
#include "common.h"
#include "gc_q.h"

// one element per thread (maps past the LDS tile): gcq_slices_kernel's indexing, m = image * HW + pixel is the map's
template <typename YT>
__global__ void __launch_bounds__(256)
gcqm_slices_kernel(const float* __restrict__ y, int ldy, int yoff, const float* __restrict__ mu,
                   const float* __restrict__ sigma, long long ms_stride, int ld_ms, float* __restrict__ lik, int Mtot,
                   YT* __restrict__ yhat, int ld_yhat, float* __restrict__ yhat32, int ld32, int n, int HW, int nslices,
                   int sw, int total, int* __restrict__ sym, int* __restrict__ idx,
                   const float* __restrict__ scale_table, int nscale, float bound, const int* __restrict__ qmap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int per_pix = nslices * sw;
  const int m = i / per_pix, r = i - m * per_pix;
  const int j = r / sw, c = r - j * sw;
  const int ch = yoff + j * sw + c;
  const int b = m / HW, pix = m - b * HW;
  const float delta = tmae_qstep(qmap[m]);
  const size_t ms = j * ms_stride + (size_t)m * ld_ms + c;
  const GcqElem e = gcq_quantize(y[(size_t)m * ldy + ch], mu[ms], sigma[ms], delta, bound);
  if (yhat) yhat[(size_t)m * ld_yhat + ch] = to_out<YT>(e.yhat);
  if (yhat32) yhat32[(size_t)m * ld32 + ch] = e.yhat;
  if (lik) lik[((size_t)b * Mtot + ch) * HW + pix] = gcq_likelihood(e.qi, e.s);
  const size_t pos = (size_t)j * n * sw * HW + ((size_t)b * sw + c) * HW + pix;
  sym[pos] = (int)e.qi;
  idx[pos] = gcq_index(e.s, scale_table, nscale);
}

// One 1024-thread workgroup per (image, slice): gcq_slices_tiled_kernel's two phases.  The step is no longer uniform
// over the workgroup: phase 1 takes it per element from the map (HW ints, cache resident; the same tmae_qstep of the
// same integer as the element kernel, so the two forms agree bit for bit), phase 2 needs none.
constexpr int GCQM_TILE_MAX = 4800;  // coding.hip's GCQ_TILE_MAX
template <typename YT>
__global__ void __launch_bounds__(1024)
gcqm_slices_tiled_kernel(const float* __restrict__ y, int ldy, int yoff, const float* __restrict__ mu,
                         const float* __restrict__ sigma, long long ms_stride, int ld_ms, float* __restrict__ lik,
                         int Mtot, YT* __restrict__ yhat, int ld_yhat, float* __restrict__ yhat32, int ld32, int n,
                         int HW, int nslices, int sw, int* __restrict__ sym, int* __restrict__ idx,
                         const float* __restrict__ scale_table, int nscale, float bound,
                         const int* __restrict__ qmap) {
  __shared__ float qs[GCQM_TILE_MAX], ss[GCQM_TILE_MAX];
  const int b = blockIdx.x / nslices, j = blockIdx.x - b * nslices;
  const int ld = sw + 1, tot = HW * sw;
  // phase 1: NHWC order
  for (int e = threadIdx.x; e < tot; e += 1024) {
    const int pix = e / sw, c = e - pix * sw;
    const int m = b * HW + pix, ch = yoff + j * sw + c;
    const size_t ms = j * ms_stride + (size_t)m * ld_ms + c;
    const GcqElem v = gcq_quantize(y[(size_t)m * ldy + ch], mu[ms], sigma[ms], tmae_qstep(qmap[m]), bound);
    if (yhat) yhat[(size_t)m * ld_yhat + ch] = to_out<YT>(v.yhat);
    if (yhat32) yhat32[(size_t)m * ld32 + ch] = v.yhat;
    qs[pix * ld + c] = v.qi;
    ss[pix * ld + c] = v.s;
  }
  __syncthreads();
  // phase 2: pixel fastest
  for (int e = threadIdx.x; e < tot; e += 1024) {
    const int c = e / HW, pix = e - c * HW;
    const float qi = qs[pix * ld + c], s = ss[pix * ld + c];
    if (lik) lik[((size_t)b * Mtot + yoff + j * sw + c) * HW + pix] = gcq_likelihood(qi, s);
    const size_t pos = (size_t)j * n * sw * HW + ((size_t)b * sw + c) * HW + pix;
    sym[pos] = (int)qi;
    idx[pos] = gcq_index(s, scale_table, nscale);
  }
}

extern "C" int tmae_gc_slices_code_qm(const float* y, int ldy, int yoff, const float* mu, const float* sigma,
                                      long long ms_stride, int ld_ms, float* lik, int Mtot, void* yhat, int yhat_dtype,
                                      int ld_yhat, float* yhat32, int ld32, int n, int HW, int nslices, int sw,
                                      int* symbols, int* indexes, const float* scale_table, int nscale,
                                      float scale_bound, const int* qmap, void* stream) {
  TMAE_REQUIRE(y && mu && sigma && symbols && indexes && scale_table && qmap && nscale >= 1,
               "tmae_gc_slices_code_qm: y/mu/sigma/symbols/indexes/scale_table/qmap required");
  TMAE_REQUIRE(n >= 0 && HW >= 0 && nslices >= 0 && sw >= 0, "tmae_gc_slices_code_qm: negative extent");
  const hipStream_t st = (hipStream_t)stream;
  const int total = n * HW * nslices * sw;
  if (total <= 0) return TMAE_OK;
  if (HW * (sw + 1) <= GCQM_TILE_MAX) {
    const dim3 tg(n * nslices);
    if (yhat_dtype == TMAE_BF16)
      hipLaunchKernelGGL(gcqm_slices_tiled_kernel<bf16>, tg, dim3(1024), 0, st, y, ldy, yoff, mu, sigma, ms_stride,
                         ld_ms, lik, Mtot, (bf16*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, symbols, indexes,
                         scale_table, nscale, scale_bound, qmap);
    else
      hipLaunchKernelGGL(gcqm_slices_tiled_kernel<float>, tg, dim3(1024), 0, st, y, ldy, yoff, mu, sigma, ms_stride,
                         ld_ms, lik, Mtot, (float*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, symbols, indexes,
                         scale_table, nscale, scale_bound, qmap);
    TMAE_LAUNCH_CHECK("tmae_gc_slices_code_qm");
  }
  const dim3 grid(ceil_div(total, 256));
  if (yhat_dtype == TMAE_BF16)
    hipLaunchKernelGGL(gcqm_slices_kernel<bf16>, grid, dim3(256), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms, lik,
                       Mtot, (bf16*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, total, symbols, indexes,
                       scale_table, nscale, scale_bound, qmap);
  else
    hipLaunchKernelGGL(gcqm_slices_kernel<float>, grid, dim3(256), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms,
                       lik, Mtot, (float*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, total, symbols, indexes,
                       scale_table, nscale, scale_bound, qmap);
  TMAE_LAUNCH_CHECK("tmae_gc_slices_code_qm");
}

__global__ void __launch_bounds__(256)
gcqm_indexes_kernel(const float* __restrict__ sigma, long long ms_stride, int ld_ms, int n, int HW, int nslices, int sw,
                    const float* __restrict__ scale_table, int nscale, float bound, int* __restrict__ idx, int total,
                    const int* __restrict__ qmap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int per_pix = nslices * sw;
  const int m = i / per_pix, r = i - m * per_pix;
  const int j = r / sw, c = r - j * sw;
  const int b = m / HW, pix = m - b * HW;
  const float s = gcq_scale(sigma[j * ms_stride + (size_t)m * ld_ms + c], tmae_qstep(qmap[m]), bound);
  idx[(size_t)j * n * sw * HW + ((size_t)b * sw + c) * HW + pix] = gcq_index(s, scale_table, nscale);
}

extern "C" int tmae_gc_indexes_qm(const float* sigma, long long ms_stride, int ld_ms, int n, int HW, int nslices,
                                  int sw, const float* scale_table, int nscale, float scale_bound, int* indexes,
                                  const int* qmap, void* stream) {
  TMAE_REQUIRE(sigma && scale_table && indexes && qmap && nscale >= 1, "tmae_gc_indexes_qm: bad arguments");
  TMAE_REQUIRE(n >= 0 && HW >= 0 && nslices >= 0 && sw >= 0, "tmae_gc_indexes_qm: negative extent");
  const int total = n * HW * nslices * sw;
  if (total <= 0) return TMAE_OK;
  hipLaunchKernelGGL(gcqm_indexes_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, sigma,
                     ms_stride, ld_ms, n, HW, nslices, sw, scale_table, nscale, scale_bound, indexes, total, qmap);
  TMAE_LAUNCH_CHECK("tmae_gc_indexes_qm");
}

template <typename YT>
__global__ void __launch_bounds__(256)
gcqm_dequantize_kernel(const int* __restrict__ sym, const float* __restrict__ mu, long long ms_stride, int ld_ms, int n,
                       int HW, int nslices, int sw, int yoff, YT* __restrict__ yhat, int ld_yhat,
                       float* __restrict__ yhat32, int ld32, int total, const int* __restrict__ qmap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int per_pix = nslices * sw;
  const int m = i / per_pix, r = i - m * per_pix;
  const int j = r / sw, c = r - j * sw;
  const int b = m / HW, pix = m - b * HW;
  const int ch = yoff + j * sw + c;
  const float v = gcq_recon((float)sym[(size_t)j * n * sw * HW + ((size_t)b * sw + c) * HW + pix],
                            mu[j * ms_stride + (size_t)m * ld_ms + c], tmae_qstep(qmap[m]));
  yhat[(size_t)m * ld_yhat + ch] = to_out<YT>(v);
  if (yhat32) yhat32[(size_t)m * ld32 + ch] = v;
}

extern "C" int tmae_gc_dequantize_qm(const int* symbols, const float* mu, long long ms_stride, int ld_ms, int n,
                                     int HW, int nslices, int sw, int yoff, void* yhat, int yhat_dtype, int ld_yhat,
                                     float* yhat32, int ld32, const int* qmap, void* stream) {
  TMAE_REQUIRE(symbols && mu && yhat && qmap, "tmae_gc_dequantize_qm: bad arguments");
  TMAE_REQUIRE(n >= 0 && HW >= 0 && nslices >= 0 && sw >= 0, "tmae_gc_dequantize_qm: negative extent");
  const int total = n * HW * nslices * sw;
  if (total <= 0) return TMAE_OK;
  const dim3 grid(ceil_div(total, 256));
  if (yhat_dtype == TMAE_BF16)
    hipLaunchKernelGGL(gcqm_dequantize_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, symbols, mu, ms_stride,
                       ld_ms, n, HW, nslices, sw, yoff, (bf16*)yhat, ld_yhat, yhat32, ld32, total, qmap);
  else
    hipLaunchKernelGGL(gcqm_dequantize_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, symbols, mu, ms_stride,
                       ld_ms, n, HW, nslices, sw, yoff, (float*)yhat, ld_yhat, yhat32, ld32, total, qmap);
  TMAE_LAUNCH_CHECK("tmae_gc_dequantize_qm");
}

// ------------------------------------------------------------------ forward at a map
// tmae_gc_slices_fwd_q at a step per pixel: both of its forms, same layouts; eval (noise NULL) is bit for bit
// tmae_gc_slices_code_qm's y_hat and likelihood
template <typename YT>
__global__ void __launch_bounds__(256)
gcqm_fwd_kernel(const float* __restrict__ y, int ldy, int yoff, const float* __restrict__ mu,
                const float* __restrict__ sigma, long long ms_stride, int ld_ms, const float* __restrict__ noise,
                float* __restrict__ lik, int Mtot, YT* __restrict__ yhat, int ld_yhat, float* __restrict__ yhat32,
                int ld32, int HW, int nslices, int sw, int total, float bound, const int* __restrict__ qmap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int per_pix = nslices * sw;
  const int m = i / per_pix, r = i - m * per_pix;
  const int j = r / sw, c = r - j * sw;
  const int ch = yoff + j * sw + c;
  const int b = m / HW, pix = m - b * HW;
  const float delta = tmae_qstep(qmap[m]);
  const size_t ms = j * ms_stride + (size_t)m * ld_ms + c;
  const float yv = y[(size_t)m * ldy + ch], mv = mu[ms];
  const GcqElem e = gcq_quantize(yv, mv, sigma[ms], delta, bound);
  if (yhat) yhat[(size_t)m * ld_yhat + ch] = to_out<YT>(e.yhat);
  if (yhat32) yhat32[(size_t)m * ld32 + ch] = e.yhat;
  const size_t nchw = ((size_t)b * Mtot + ch) * HW + pix;
  lik[nchw] = noise ? gcq_likelihood_noisy(gcq_scaled(yv, mv, delta), noise[nchw], e.s) : gcq_likelihood(e.qi, e.s);
}

template <typename YT>
__global__ void __launch_bounds__(1024)
gcqm_fwd_tiled_kernel(const float* __restrict__ y, int ldy, int yoff, const float* __restrict__ mu,
                      const float* __restrict__ sigma, long long ms_stride, int ld_ms, const float* __restrict__ noise,
                      float* __restrict__ lik, int Mtot, YT* __restrict__ yhat, int ld_yhat, float* __restrict__ yhat32,
                      int ld32, int HW, int nslices, int sw, float bound, const int* __restrict__ qmap) {
  __shared__ float ts[GCQM_TILE_MAX], ss[GCQM_TILE_MAX];
  const int b = blockIdx.x / nslices, j = blockIdx.x - b * nslices;
  const int ld = sw + 1, tot = HW * sw;
  // phase 1: NHWC order
  for (int e = threadIdx.x; e < tot; e += 1024) {
    const int pix = e / sw, c = e - pix * sw;
    const int m = b * HW + pix, ch = yoff + j * sw + c;
    const float delta = tmae_qstep(qmap[m]);
    const size_t ms = j * ms_stride + (size_t)m * ld_ms + c;
    const float yv = y[(size_t)m * ldy + ch], mv = mu[ms];
    const GcqElem v = gcq_quantize(yv, mv, sigma[ms], delta, bound);
    if (yhat) yhat[(size_t)m * ld_yhat + ch] = to_out<YT>(v.yhat);
    if (yhat32) yhat32[(size_t)m * ld32 + ch] = v.yhat;
    ts[pix * ld + c] = gcq_scaled(yv, mv, delta);
    ss[pix * ld + c] = v.s;
  }
  __syncthreads();
  // phase 2: pixel fastest
  for (int e = threadIdx.x; e < tot; e += 1024) {
    const int c = e / HW, pix = e - c * HW;
    const float t = ts[pix * ld + c], s = ss[pix * ld + c];
    const size_t nchw = ((size_t)b * Mtot + yoff + j * sw + c) * HW + pix;
    lik[nchw] = noise ? gcq_likelihood_noisy(t, noise[nchw], s) : gcq_likelihood(rintf(t), s);
  }
}

extern "C" int tmae_gc_slices_fwd_qm(const float* y, int ldy, int yoff, const float* mu, const float* sigma,
                                     long long ms_stride, int ld_ms, const float* noise, float* lik, int Mtot,
                                     void* yhat, int yhat_dtype, int ld_yhat, float* yhat32, int ld32, int n, int HW,
                                     int nslices, int sw, float scale_bound, const int* qmap, void* stream) {
  TMAE_REQUIRE(y && mu && sigma && lik && qmap, "tmae_gc_slices_fwd_qm: y/mu/sigma/lik/qmap required");
  TMAE_REQUIRE(n >= 0 && HW >= 0 && nslices >= 0 && sw >= 0, "tmae_gc_slices_fwd_qm: negative extent");
  const hipStream_t st = (hipStream_t)stream;
  const int total = n * HW * nslices * sw;
  if (total <= 0) return TMAE_OK;
  if (HW * (sw + 1) <= GCQM_TILE_MAX) {
    const dim3 tg(n * nslices);
    if (yhat_dtype == TMAE_BF16)
      hipLaunchKernelGGL(gcqm_fwd_tiled_kernel<bf16>, tg, dim3(1024), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms,
                         noise, lik, Mtot, (bf16*)yhat, ld_yhat, yhat32, ld32, HW, nslices, sw, scale_bound, qmap);
    else
      hipLaunchKernelGGL(gcqm_fwd_tiled_kernel<float>, tg, dim3(1024), 0, st, y, ldy, yoff, mu, sigma, ms_stride,
                         ld_ms, noise, lik, Mtot, (float*)yhat, ld_yhat, yhat32, ld32, HW, nslices, sw, scale_bound,
                         qmap);
    TMAE_LAUNCH_CHECK("tmae_gc_slices_fwd_qm");
  }
  const dim3 grid(ceil_div(total, 256));
  if (yhat_dtype == TMAE_BF16)
    hipLaunchKernelGGL(gcqm_fwd_kernel<bf16>, grid, dim3(256), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms, noise,
                       lik, Mtot, (bf16*)yhat, ld_yhat, yhat32, ld32, HW, nslices, sw, total, scale_bound, qmap);
  else
    hipLaunchKernelGGL(gcqm_fwd_kernel<float>, grid, dim3(256), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms, noise,
                       lik, Mtot, (float*)yhat, ld_yhat, yhat32, ld32, HW, nslices, sw, total, scale_bound, qmap);
  TMAE_LAUNCH_CHECK("tmae_gc_slices_fwd_qm");
}
