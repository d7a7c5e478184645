// Rate-distortion optimised quantisation of y in the encoder's slice kernel: tmae_gc_slices_code_q /
// _qm (coding.hip, coding_qmap.hip) with the symbol chosen by the rule of gc_rdo.h instead of plain rounding.  The step
// comes from a map per pixel (qmap), else per image (q), else is 1.  Layouts and both launch forms are the siblings';
// a translation unit of its own, so that their code objects stay what they are.  The slice loop is serial and the
// encoder's y_hat feeds the later slices, so a decision made here propagates by itself, and the decoder, which reads
// the symbols, needs nothing.  The reference has no counterpart.
#include "common.h"
#include "gc_rdo.h"

__device__ __forceinline__ float gcr_step(const int* __restrict__ q, const int* __restrict__ qmap, int b, int m) {
  return tmae_qstep(qmap ? qmap[m] : (q ? q[b] : 0));
}

// one element per thread (maps past the LDS tile): gcq_slices_kernel's indexing
template <typename YT>
__global__ void __launch_bounds__(256)
gcr_slices_kernel(const float* __restrict__ y, int ldy, int yoff, const float* __restrict__ mu,
                  const float* __restrict__ sigma, long long ms_stride, int ld_ms, float* __restrict__ lik, int Mtot,
                  YT* __restrict__ yhat, int ld_yhat, float* __restrict__ yhat32, int ld32, int n, int HW, int nslices,
                  int sw, int total, int* __restrict__ sym, int* __restrict__ idx,
                  const float* __restrict__ scale_table, int nscale, float bound, const int* __restrict__ q,
                  const int* __restrict__ qmap, const float* __restrict__ rdo_w, const float* __restrict__ rate,
                  int rate_stride, const int* __restrict__ cdf_sizes, const int* __restrict__ cdf_offsets,
                  int* __restrict__ changed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int per_pix = nslices * sw;
  const int m = i / per_pix, r = i - m * per_pix;
  const int j = r / sw, c = r - j * sw;
  const int ch = yoff + j * sw + c;
  const int b = m / HW, pix = m - b * HW;
  const float delta = gcr_step(q, qmap, b, m);
  const size_t ms = j * ms_stride + (size_t)m * ld_ms + c;
  const GcrElem e = gcr_quantize(y[(size_t)m * ldy + ch], mu[ms], sigma[ms], delta, bound, rdo_w[b], scale_table,
                                 nscale, rate, rate_stride, cdf_sizes, cdf_offsets);
  if (yhat) yhat[(size_t)m * ld_yhat + ch] = to_out<YT>(e.yhat);
  if (yhat32) yhat32[(size_t)m * ld32 + ch] = e.yhat;
  if (lik) lik[((size_t)b * Mtot + ch) * HW + pix] = gcq_likelihood(e.qi, e.s);
  const size_t pos = (size_t)j * n * sw * HW + ((size_t)b * sw + c) * HW + pix;
  sym[pos] = (int)e.qi;
  idx[pos] = e.idx;
  if (changed && e.flipped) atomicAdd(&changed[b], 1);
}

// One 1024-thread workgroup per (image, slice): gcq_slices_tiled_kernel's two phases.  The decision needs the row
// before y_hat is written, so the index is computed in phase 1 (NHWC order) and goes through a third LDS array to
// phase 2, which writes it pixel fastest with the symbol and the likelihood.  The flips are counted in LDS and leave
// the workgroup as one atomic add.  Same arithmetic per element as the kernel above (gcr_quantize).
constexpr int GCR_TILE_MAX = 4800;  // HW * (sw + 1) entries per LDS array (3 arrays, 57.6 KB): coding.hip's GCQ_TILE_MAX
template <typename YT>
__global__ void __launch_bounds__(1024)
gcr_slices_tiled_kernel(const float* __restrict__ y, int ldy, int yoff, const float* __restrict__ mu,
                        const float* __restrict__ sigma, long long ms_stride, int ld_ms, float* __restrict__ lik,
                        int Mtot, YT* __restrict__ yhat, int ld_yhat, float* __restrict__ yhat32, int ld32, int n,
                        int HW, int nslices, int sw, int* __restrict__ sym, int* __restrict__ idx,
                        const float* __restrict__ scale_table, int nscale, float bound, const int* __restrict__ q,
                        const int* __restrict__ qmap, const float* __restrict__ rdo_w, const float* __restrict__ rate,
                        int rate_stride, const int* __restrict__ cdf_sizes, const int* __restrict__ cdf_offsets,
                        int* __restrict__ changed) {
  __shared__ float qs[GCR_TILE_MAX], ss[GCR_TILE_MAX];
  __shared__ int is[GCR_TILE_MAX];
  __shared__ int nflip;
  const int b = blockIdx.x / nslices, j = blockIdx.x - b * nslices;
  const int ld = sw + 1, tot = HW * sw;
  const float w = rdo_w[b];
  if (threadIdx.x == 0) nflip = 0;
  __syncthreads();
  // phase 1: NHWC order
  int flips = 0;
  for (int e = threadIdx.x; e < tot; e += 1024) {
    const int pix = e / sw, c = e - pix * sw;
    const int m = b * HW + pix, ch = yoff + j * sw + c;
    const size_t ms = j * ms_stride + (size_t)m * ld_ms + c;
    const GcrElem v = gcr_quantize(y[(size_t)m * ldy + ch], mu[ms], sigma[ms], gcr_step(q, qmap, b, m), bound, w,
                                   scale_table, nscale, rate, rate_stride, cdf_sizes, cdf_offsets);
    if (yhat) yhat[(size_t)m * ld_yhat + ch] = to_out<YT>(v.yhat);
    if (yhat32) yhat32[(size_t)m * ld32 + ch] = v.yhat;
    qs[pix * ld + c] = v.qi;
    ss[pix * ld + c] = v.s;
    is[pix * ld + c] = v.idx;
    flips += v.flipped;
  }
  if (changed && flips) atomicAdd(&nflip, flips);
  __syncthreads();
  if (changed && threadIdx.x == 0 && nflip) atomicAdd(&changed[b], nflip);
  // phase 2: pixel fastest
  for (int e = threadIdx.x; e < tot; e += 1024) {
    const int c = e / HW, pix = e - c * HW;
    const float qi = qs[pix * ld + c], s = ss[pix * ld + c];
    if (lik) lik[((size_t)b * Mtot + yoff + j * sw + c) * HW + pix] = gcq_likelihood(qi, s);
    const size_t pos = (size_t)j * n * sw * HW + ((size_t)b * sw + c) * HW + pix;
    sym[pos] = (int)qi;
    idx[pos] = is[pix * ld + c];
  }
}

extern "C" int tmae_gc_slices_code_rdo(const float* y, int ldy, int yoff, const float* mu, const float* sigma,
                                       long long ms_stride, int ld_ms, float* lik, int Mtot, void* yhat,
                                       int yhat_dtype, int ld_yhat, float* yhat32, int ld32, int n, int HW,
                                       int nslices, int sw, int* symbols, int* indexes, const float* scale_table,
                                       int nscale, float scale_bound, const int* q, const int* qmap,
                                       const float* rdo_w, const float* rate, int rate_stride, const int* cdf_sizes,
                                       const int* cdf_offsets, int* changed, void* stream) {
  TMAE_REQUIRE(y && mu && sigma && symbols && indexes && scale_table && nscale >= 1,
               "tmae_gc_slices_code_rdo: y/mu/sigma/symbols/indexes/scale_table required");
  TMAE_REQUIRE(rdo_w && rate && cdf_sizes && cdf_offsets && rate_stride >= 1,
               "tmae_gc_slices_code_rdo: rdo_w/rate/cdf_sizes/cdf_offsets required, rate_stride >= 1");
  TMAE_REQUIRE(n >= 0 && HW >= 0 && nslices >= 0 && sw >= 0, "tmae_gc_slices_code_rdo: negative extent");
  const hipStream_t st = (hipStream_t)stream;
  const int total = n * HW * nslices * sw;
  if (total <= 0) return TMAE_OK;
  if (HW * (sw + 1) <= GCR_TILE_MAX) {
    const dim3 tg(n * nslices);
    if (yhat_dtype == TMAE_BF16)
      hipLaunchKernelGGL(gcr_slices_tiled_kernel<bf16>, tg, dim3(1024), 0, st, y, ldy, yoff, mu, sigma, ms_stride,
                         ld_ms, lik, Mtot, (bf16*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, symbols, indexes,
                         scale_table, nscale, scale_bound, q, qmap, rdo_w, rate, rate_stride, cdf_sizes, cdf_offsets,
                         changed);
    else
      hipLaunchKernelGGL(gcr_slices_tiled_kernel<float>, tg, dim3(1024), 0, st, y, ldy, yoff, mu, sigma, ms_stride,
                         ld_ms, lik, Mtot, (float*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, symbols, indexes,
                         scale_table, nscale, scale_bound, q, qmap, rdo_w, rate, rate_stride, cdf_sizes, cdf_offsets,
                         changed);
    TMAE_LAUNCH_CHECK("tmae_gc_slices_code_rdo");
  }
  const dim3 grid(ceil_div(total, 256));
  if (yhat_dtype == TMAE_BF16)
    hipLaunchKernelGGL(gcr_slices_kernel<bf16>, grid, dim3(256), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms, lik,
                       Mtot, (bf16*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, total, symbols, indexes,
                       scale_table, nscale, scale_bound, q, qmap, rdo_w, rate, rate_stride, cdf_sizes, cdf_offsets,
                       changed);
  else
    hipLaunchKernelGGL(gcr_slices_kernel<float>, grid, dim3(256), 0, st, y, ldy, yoff, mu, sigma, ms_stride, ld_ms, lik,
                       Mtot, (float*)yhat, ld_yhat, yhat32, ld32, n, HW, nslices, sw, total, symbols, indexes,
                       scale_table, nscale, scale_bound, q, qmap, rdo_w, rate, rate_stride, cdf_sizes, cdf_offsets,
                       changed);
  TMAE_LAUNCH_CHECK("tmae_gc_slices_code_rdo");
}
