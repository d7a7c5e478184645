// Device side of MCM.compress / decompress (reference MCM.py:805-968) around the host rANS coder
// (rans.cpp): the GaussianConditional CDF-table pmf (update_scale_table, testing.py:223), scale-table
// indexes (build_indexes, MCM.py:867, 938), dequantisation of decoded symbols into the slice loop's
// y_hat buffers (MCM.py:946), and the ids_restore -> ids_shuffle inverse the decoder kernels index by.
// The symbol-emitting form of the slice likelihood kernel lives with it in conv.hip
// (tmae_gc_slices_code); the EntropyBottleneck ones with its density tables in entropy.hip.
#include "common.h"
#include "gc_q.h"

// GaussianConditional.update: pmf[i][j] = Phi((1/2 - s) / scale_i) - Phi((-1/2 - s) / scale_i),
// s = |j - center_i|, Phi(x) = erfc(-x / sqrt 2) / 2; tail[i] = 2 Phi((-1/2 - center_i) / scale_i)
__device__ __forceinline__ float std_cumulative(float x) { return 0.5f * erfcf(-0.70710678118654752440f * x); }

__global__ void __launch_bounds__(256)
gc_pmf_kernel(const float* __restrict__ scale_table, const int* __restrict__ center, int n, int max_length,
              float* __restrict__ pmf, float* __restrict__ tail) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * max_length) return;
  const int r = i / max_length, j = i - r * max_length;
  const float sc = scale_table[r];
  const float s = (float)abs(j - center[r]);
  const float upper = std_cumulative((0.5f - s) / sc);
  const float lower = std_cumulative((-0.5f - s) / sc);
  pmf[i] = upper - lower;
  if (j == 0) tail[r] = 2.0f * lower;
}

extern "C" int tmae_gc_pmf(const float* scale_table, const int* pmf_center, int n, int max_length, float* pmf,
                           float* tail, void* stream) {
  TMAE_REQUIRE(scale_table && pmf_center && pmf && tail && n > 0 && max_length > 0, "tmae_gc_pmf: bad arguments");
  hipLaunchKernelGGL(gc_pmf_kernel, dim3(ceil_div(n * max_length, 256)), dim3(256), 0, (hipStream_t)stream,
                     scale_table, pmf_center, n, max_length, pmf, tail);
  TMAE_LAUNCH_CHECK("tmae_gc_pmf");
}

// build_indexes: index = (nscale - 1) - #{t < nscale - 1 : max(sigma, bound) <= table[t]}.
// sigma rows: slice j of the launch at sigma + j * ms_stride, row m (= image * HW + pixel), channel c
// at m * ld_ms + c; indexes written in the coder's order [slice][image][channel][pixel].
__global__ void __launch_bounds__(256)
gc_indexes_kernel(const float* __restrict__ sigma, long long ms_stride, int ld_ms, int n, int HW, int nslices, int sw,
                  const float* __restrict__ scale_table, int nscale, float bound, int* __restrict__ idx, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int per_pix = nslices * sw;
  const int m = i / per_pix, r = i - m * per_pix;
  const int j = r / sw, c = r - j * sw;
  const int b = m / HW, pix = m - b * HW;
  const float s = fmaxf(sigma[j * ms_stride + (size_t)m * ld_ms + c], bound);
  int id = nscale - 1;
  for (int t = 0; t < nscale - 1; ++t) id -= (s <= scale_table[t]) ? 1 : 0;
  idx[(size_t)j * n * sw * HW + ((size_t)b * sw + c) * HW + pix] = id;
}

extern "C" int tmae_gc_indexes(const float* sigma, long long ms_stride, int ld_ms, int n, int HW, int nslices, int sw,
                               const float* scale_table, int nscale, float scale_bound, int* indexes, void* stream) {
  TMAE_REQUIRE(sigma && scale_table && indexes && nscale >= 1, "tmae_gc_indexes: bad arguments");
  const int total = n * HW * nslices * sw;
  if (total <= 0) return TMAE_OK;
  hipLaunchKernelGGL(gc_indexes_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, sigma,
                     ms_stride, ld_ms, n, HW, nslices, sw, scale_table, nscale, scale_bound, indexes, total);
  TMAE_LAUNCH_CHECK("tmae_gc_indexes");
}

// decompress: y_hat_pre = symbols + mu (GaussianConditional.dequantize, MCM.py:946) into the same
// slice buffers the forward's slice kernel writes (operand dtype + f32 copy for the LRP residual)
template <typename YT>
__global__ void __launch_bounds__(256)
gc_dequantize_kernel(const int* __restrict__ sym, const float* __restrict__ mu, long long ms_stride, int ld_ms, int n,
                     int HW, int nslices, int sw, int yoff, YT* __restrict__ yhat, int ld_yhat,
                     float* __restrict__ yhat32, int ld32, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int per_pix = nslices * sw;
  const int m = i / per_pix, r = i - m * per_pix;
  const int j = r / sw, c = r - j * sw;
  const int b = m / HW, pix = m - b * HW;
  const int ch = yoff + j * sw + c;
  const float q = (float)sym[(size_t)j * n * sw * HW + ((size_t)b * sw + c) * HW + pix] +
                  mu[j * ms_stride + (size_t)m * ld_ms + c];
  yhat[(size_t)m * ld_yhat + ch] = to_out<YT>(q);
  if (yhat32) yhat32[(size_t)m * ld32 + ch] = q;
}

extern "C" int tmae_gc_dequantize(const int* symbols, const float* mu, long long ms_stride, int ld_ms, int n, int HW,
                                  int nslices, int sw, int yoff, void* yhat, int yhat_dtype, int ld_yhat,
                                  float* yhat32, int ld32, void* stream) {
  TMAE_REQUIRE(symbols && mu && yhat, "tmae_gc_dequantize: bad arguments");
  const int total = n * HW * nslices * sw;
  if (total <= 0) return TMAE_OK;
  const dim3 grid(ceil_div(total, 256));
  if (yhat_dtype == TMAE_BF16)
    hipLaunchKernelGGL(gc_dequantize_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, symbols, mu, ms_stride,
                       ld_ms, n, HW, nslices, sw, yoff, (bf16*)yhat, ld_yhat, yhat32, ld32, total);
  else
    hipLaunchKernelGGL(gc_dequantize_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, symbols, mu, ms_stride,
                       ld_ms, n, HW, nslices, sw, yoff, (float*)yhat, ld_yhat, yhat32, ld32, total);
  TMAE_LAUNCH_CHECK("tmae_gc_dequantize");
}

// ------------------------------------------------------------------ per-image quantiser step
// The three kernels above with y quantised at a step delta(q[image]) of the ladder in common.h.  The per-element
// arithmetic (gcq_quantize / gcq_recon / gcq_scale / gcq_likelihood / gcq_index) is in gc_q.h, shared with the forward
// and the backward at a step and with the kernels at a step per patch (coding_qmap.hip, §3.19).

// one element per thread (maps past the LDS tile): gc_slices_kernel<YT, true>'s indexing
template <typename YT>
__global__ void __launch_bounds__(256)
gcq_slices_kernel(const float* __restrict__ y, int ldy, int yoff, const float* __restrict__ mu,
                  const float* __restrict__ sigma, long long ms_stride, int ld_ms, float* __restrict__ lik, int Mtot,
                  YT* __restrict__ yhat, int ld_yhat, float* __restrict__ yhat32, int ld32, int n, int HW, int nslices,
                  int sw, int total, int* __restrict__ sym, int* __restrict__ idx,
                  const float* __restrict__ scale_table, int nscale, float bound, const int* __restrict__ q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int per_pix = nslices * sw;
  const int m = i / per_pix, r = i - m * per_pix;
  const int j = r / sw, c = r - j * sw;
  const int ch = yoff + j * sw + c;
  const int b = m / HW, pix = m - b * HW;
  const float delta = tmae_qstep(q ? q[b] : 0);
  const size_t ms = j * ms_stride + (size_t)m * ld_ms + c;
  const GcqElem e = gcq_quantize(y[(size_t)m * ldy + ch], mu[ms], sigma[ms], delta, bound);
  if (yhat) yhat[(size_t)m * ld_yhat + ch] = to_out<YT>(e.yhat);
  if (yhat32) yhat32[(size_t)m * ld32 + ch] = e.yhat;
  if (lik) lik[((size_t)b * Mtot + ch) * HW + pix] = gcq_likelihood(e.qi, e.s);
  const size_t pos = (size_t)j * n * sw * HW + ((size_t)b * sw + c) * HW + pix;
  sym[pos] = (int)e.qi;
  idx[pos] = gcq_index(e.s, scale_table, nscale);
}

// One 1024-thread workgroup per (image, slice), as gc_slices_tiled_kernel (conv.hip, whose comment gives the
// reason): y / mu / sigma read and y_hat written channel fastest, then the rounded value and the bounded scale go
// through LDS and the symbols, indexes and likelihoods are written pixel fastest.  The step is uniform over the
// workgroup.  Same arithmetic per element as the kernel above.
constexpr int GCQ_TILE_MAX = 4800;  // HW * (sw + 1) floats per LDS array (2 arrays, 38.4 KB): conv.hip's GC_TILE_MAX
template <typename YT>
__global__ void __launch_bounds__(1024)
gcq_slices_tiled_kernel(const float* __restrict__ y, int ldy, int yoff, const float* __restrict__ mu,
                        const float* __restrict__ sigma, long long ms_stride, int ld_ms, float* __restrict__ lik,
                        int Mtot, YT* __restrict__ yhat, int ld_yhat, float* __restrict__ yhat32, int ld32, int n,
                        int HW, int nslices, int sw, int* __restrict__ sym, int* __restrict__ idx,
                        const float* __restrict__ scale_table, int nscale, float bound, const int* __restrict__ q) {
  __shared__ float qs[GCQ_TILE_MAX], ss[GCQ_TILE_MAX];
  const int b = blockIdx.x / nslices, j = blockIdx.x - b * nslices;
  const int ld = sw + 1, tot = HW * sw;
  const float delta = tmae_qstep(q ? q[b] : 0);
  // phase 1: NHWC order
  for (int e = threadIdx.x; e < tot; e += 1024) {
    const int pix = e / sw, c = e - pix * sw;
    const int m = b * HW + pix, ch = yoff + j * sw + c;
    const size_t ms = j * ms_stride + (size_t)m * ld_ms + c;
    const GcqElem v = gcq_quantize(y[(size_t)m * ldy + ch], mu[ms], sigma[ms], delta, bound);
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

extern "C" int tmae_gc_slices_code_q(const float* y, int ldy, int yoff, const float* mu, const float* sigma,
                                     long long ms_stride, int ld_ms, float* lik, int Mtot, void* yhat, int yhat_dtype,
                                     int ld_yhat, float* yhat32, int ld32, int n, int HW, int nslices, int sw,
                                     int* symbols, int* indexes, const float* scale_table, int nscale,
                                     float scale_bound, const int* q, void* stream) {
  TMAE_REQUIRE(y && mu && sigma && symbols && indexes && scale_table && nscale >= 1,
               "tmae_gc_slices_code_q: y/mu/sigma/symbols/indexes/scale_table required");
  TMAE_REQUIRE(n >= 0 && HW >= 0 && nslices >= 0 && sw >= 0, "tmae_gc_slices_code_q: negative extent");
  const hipStream_t st = (hipStream_t)stream;
  const int total = n * HW * nslices * sw;
  if (total <= 0) return TMAE_OK;
  if (HW * (sw + 1) <= GCQ_TILE_MAX) {
    const dim3 tg(n * nslices);
    if (yhat_dtype == TMAE_BF16)
      hipLaunchKernelGGL(gcq_slices_tiled_kernel<bf16>, tg, dim3(1024), 0, st, y, ldy, yoff, mu, sigma, ms_stride,
                         ld_ms, lik, Mtot, (bf16*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, symbols, indexes,
                         scale_table, nscale, scale_bound, q);
    else
      hipLaunchKernelGGL(gcq_slices_tiled_kernel<float>, tg, dim3(1024), 0, st, y, ldy, yoff, mu, sigma, ms_stride,
                         ld_ms, lik, Mtot, (float*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, symbols, indexes,
                         scale_table, nscale, scale_bound, q);
    TMAE_LAUNCH_CHECK("tmae_gc_slices_code_q");
  }
  const dim3 grid(ceil_div(total, 256));
  if (yhat_dtype == TMAE_BF16)
    hipLaunchKernelGGL(gcq_slices_kernel<bf16>, grid, dim3(256), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms, lik,
                       Mtot, (bf16*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, total, symbols, indexes,
                       scale_table, nscale, scale_bound, q);
  else
    hipLaunchKernelGGL(gcq_slices_kernel<float>, grid, dim3(256), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms, lik,
                       Mtot, (float*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, total, symbols, indexes,
                       scale_table, nscale, scale_bound, q);
  TMAE_LAUNCH_CHECK("tmae_gc_slices_code_q");
}

__global__ void __launch_bounds__(256)
gcq_indexes_kernel(const float* __restrict__ sigma, long long ms_stride, int ld_ms, int n, int HW, int nslices, int sw,
                   const float* __restrict__ scale_table, int nscale, float bound, int* __restrict__ idx, int total,
                   const int* __restrict__ q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int per_pix = nslices * sw;
  const int m = i / per_pix, r = i - m * per_pix;
  const int j = r / sw, c = r - j * sw;
  const int b = m / HW, pix = m - b * HW;
  const float s = gcq_scale(sigma[j * ms_stride + (size_t)m * ld_ms + c], tmae_qstep(q ? q[b] : 0), bound);
  idx[(size_t)j * n * sw * HW + ((size_t)b * sw + c) * HW + pix] = gcq_index(s, scale_table, nscale);
}

extern "C" int tmae_gc_indexes_q(const float* sigma, long long ms_stride, int ld_ms, int n, int HW, int nslices,
                                 int sw, const float* scale_table, int nscale, float scale_bound, int* indexes,
                                 const int* q, void* stream) {
  TMAE_REQUIRE(sigma && scale_table && indexes && nscale >= 1, "tmae_gc_indexes_q: bad arguments");
  TMAE_REQUIRE(n >= 0 && HW >= 0 && nslices >= 0 && sw >= 0, "tmae_gc_indexes_q: negative extent");
  const int total = n * HW * nslices * sw;
  if (total <= 0) return TMAE_OK;
  hipLaunchKernelGGL(gcq_indexes_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, sigma,
                     ms_stride, ld_ms, n, HW, nslices, sw, scale_table, nscale, scale_bound, indexes, total, q);
  TMAE_LAUNCH_CHECK("tmae_gc_indexes_q");
}

template <typename YT>
__global__ void __launch_bounds__(256)
gcq_dequantize_kernel(const int* __restrict__ sym, const float* __restrict__ mu, long long ms_stride, int ld_ms, int n,
                      int HW, int nslices, int sw, int yoff, YT* __restrict__ yhat, int ld_yhat,
                      float* __restrict__ yhat32, int ld32, int total, const int* __restrict__ q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int per_pix = nslices * sw;
  const int m = i / per_pix, r = i - m * per_pix;
  const int j = r / sw, c = r - j * sw;
  const int b = m / HW, pix = m - b * HW;
  const int ch = yoff + j * sw + c;
  const float v = gcq_recon((float)sym[(size_t)j * n * sw * HW + ((size_t)b * sw + c) * HW + pix],
                            mu[j * ms_stride + (size_t)m * ld_ms + c], tmae_qstep(q ? q[b] : 0));
  yhat[(size_t)m * ld_yhat + ch] = to_out<YT>(v);
  if (yhat32) yhat32[(size_t)m * ld32 + ch] = v;
}

extern "C" int tmae_gc_dequantize_q(const int* symbols, const float* mu, long long ms_stride, int ld_ms, int n, int HW,
                                    int nslices, int sw, int yoff, void* yhat, int yhat_dtype, int ld_yhat,
                                    float* yhat32, int ld32, const int* q, void* stream) {
  TMAE_REQUIRE(symbols && mu && yhat, "tmae_gc_dequantize_q: bad arguments");
  TMAE_REQUIRE(n >= 0 && HW >= 0 && nslices >= 0 && sw >= 0, "tmae_gc_dequantize_q: negative extent");
  const int total = n * HW * nslices * sw;
  if (total <= 0) return TMAE_OK;
  const dim3 grid(ceil_div(total, 256));
  if (yhat_dtype == TMAE_BF16)
    hipLaunchKernelGGL(gcq_dequantize_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, symbols, mu, ms_stride,
                       ld_ms, n, HW, nslices, sw, yoff, (bf16*)yhat, ld_yhat, yhat32, ld32, total, q);
  else
    hipLaunchKernelGGL(gcq_dequantize_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, symbols, mu, ms_stride,
                       ld_ms, n, HW, nslices, sw, yoff, (float*)yhat, ld_yhat, yhat32, ld32, total, q);
  TMAE_LAUNCH_CHECK("tmae_gc_dequantize_q");
}

// ------------------------------------------------------------------ forward at a step
// tmae_gc_slices_fwd (conv.hip) at delta(q[image]): y_hat = gcq_recon, s = gcq_scale, likelihood at |qi| (eval: bit
// for bit tmae_gc_slices_code_q's) or at |t + noise| (training), t = (y - mu) / delta.  Both of its forms, same layouts.
template <typename YT>
__global__ void __launch_bounds__(256)
gcq_fwd_kernel(const float* __restrict__ y, int ldy, int yoff, const float* __restrict__ mu,
               const float* __restrict__ sigma, long long ms_stride, int ld_ms, const float* __restrict__ noise,
               float* __restrict__ lik, int Mtot, YT* __restrict__ yhat, int ld_yhat, float* __restrict__ yhat32,
               int ld32, int HW, int nslices, int sw, int total, float bound, const int* __restrict__ q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int per_pix = nslices * sw;
  const int m = i / per_pix, r = i - m * per_pix;
  const int j = r / sw, c = r - j * sw;
  const int ch = yoff + j * sw + c;
  const int b = m / HW, pix = m - b * HW;
  const float delta = tmae_qstep(q ? q[b] : 0);
  const size_t ms = j * ms_stride + (size_t)m * ld_ms + c;
  const float yv = y[(size_t)m * ldy + ch], mv = mu[ms];
  const GcqElem e = gcq_quantize(yv, mv, sigma[ms], delta, bound);
  if (yhat) yhat[(size_t)m * ld_yhat + ch] = to_out<YT>(e.yhat);
  if (yhat32) yhat32[(size_t)m * ld32 + ch] = e.yhat;
  const size_t nchw = ((size_t)b * Mtot + ch) * HW + pix;
  lik[nchw] = noise ? gcq_likelihood_noisy(gcq_scaled(yv, mv, delta), noise[nchw], e.s) : gcq_likelihood(e.qi, e.s);
}

// one 1024-thread workgroup per (image, slice): gcq_slices_tiled_kernel's two phases; t goes through LDS (qi = rint(t))
template <typename YT>
__global__ void __launch_bounds__(1024)
gcq_fwd_tiled_kernel(const float* __restrict__ y, int ldy, int yoff, const float* __restrict__ mu,
                     const float* __restrict__ sigma, long long ms_stride, int ld_ms, const float* __restrict__ noise,
                     float* __restrict__ lik, int Mtot, YT* __restrict__ yhat, int ld_yhat, float* __restrict__ yhat32,
                     int ld32, int HW, int nslices, int sw, float bound, const int* __restrict__ q) {
  __shared__ float ts[GCQ_TILE_MAX], ss[GCQ_TILE_MAX];
  const int b = blockIdx.x / nslices, j = blockIdx.x - b * nslices;
  const int ld = sw + 1, tot = HW * sw;
  const float delta = tmae_qstep(q ? q[b] : 0);
  // phase 1: NHWC order
  for (int e = threadIdx.x; e < tot; e += 1024) {
    const int pix = e / sw, c = e - pix * sw;
    const int m = b * HW + pix, ch = yoff + j * sw + c;
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

extern "C" int tmae_gc_slices_fwd_q(const float* y, int ldy, int yoff, const float* mu, const float* sigma,
                                    long long ms_stride, int ld_ms, const float* noise, float* lik, int Mtot,
                                    void* yhat, int yhat_dtype, int ld_yhat, float* yhat32, int ld32, int n, int HW,
                                    int nslices, int sw, float scale_bound, const int* q, void* stream) {
  TMAE_REQUIRE(y && mu && sigma && lik, "tmae_gc_slices_fwd_q: y/mu/sigma/lik required");
  TMAE_REQUIRE(n >= 0 && HW >= 0 && nslices >= 0 && sw >= 0, "tmae_gc_slices_fwd_q: negative extent");
  const hipStream_t st = (hipStream_t)stream;
  const int total = n * HW * nslices * sw;
  if (total <= 0) return TMAE_OK;
  if (HW * (sw + 1) <= GCQ_TILE_MAX) {
    const dim3 tg(n * nslices);
    if (yhat_dtype == TMAE_BF16)
      hipLaunchKernelGGL(gcq_fwd_tiled_kernel<bf16>, tg, dim3(1024), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms,
                         noise, lik, Mtot, (bf16*)yhat, ld_yhat, yhat32, ld32, HW, nslices, sw, scale_bound, q);
    else
      hipLaunchKernelGGL(gcq_fwd_tiled_kernel<float>, tg, dim3(1024), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms,
                         noise, lik, Mtot, (float*)yhat, ld_yhat, yhat32, ld32, HW, nslices, sw, scale_bound, q);
    TMAE_LAUNCH_CHECK("tmae_gc_slices_fwd_q");
  }
  const dim3 grid(ceil_div(total, 256));
  if (yhat_dtype == TMAE_BF16)
    hipLaunchKernelGGL(gcq_fwd_kernel<bf16>, grid, dim3(256), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms, noise,
                       lik, Mtot, (bf16*)yhat, ld_yhat, yhat32, ld32, HW, nslices, sw, total, scale_bound, q);
  else
    hipLaunchKernelGGL(gcq_fwd_kernel<float>, grid, dim3(256), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms, noise,
                       lik, Mtot, (float*)yhat, ld_yhat, yhat32, ld32, HW, nslices, sw, total, scale_bound, q);
  TMAE_LAUNCH_CHECK("tmae_gc_slices_fwd_q");
}

// inv[b][p[b][j]] = j  (ids_shuffle = argsort(ids_restore) for a permutation, MCM.py:580)
__global__ void invert_permutation_kernel(const int64_t* __restrict__ p, int64_t* __restrict__ inv, int L, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int b = i / L, j = i - b * L;
  const int64_t v = p[i];
  if (v >= 0 && v < L) inv[(size_t)b * L + v] = j;
}

extern "C" int tmae_invert_permutation(const int64_t* perm, int64_t* inverse, int n, int L, void* stream) {
  TMAE_REQUIRE(perm && inverse && n >= 0 && L >= 0, "tmae_invert_permutation: bad arguments");
  const int total = n * L;
  if (total <= 0) return TMAE_OK;
  hipLaunchKernelGGL(invert_permutation_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, perm,
                     inverse, L, total);
  TMAE_LAUNCH_CHECK("tmae_invert_permutation");
}
