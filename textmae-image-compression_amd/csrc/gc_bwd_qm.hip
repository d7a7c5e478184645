// GaussianConditional backward at a quantiser step per pixel of the latent grid, i.e. per kept patch:
// train.hip's gcq_bwd_kernel (§3.18) with delta taken from a map qmap[image][pixel] of clamped ladder positions
// (tmae_qmap_build, qlevels.hip) instead of q[image].  The backward of tmae_gc_slices_fwd_qm (coding_qmap.hip).  The
// same helpers of gc_q.h on the same operands in the same order, so a map that is constant over an image gives
// tmae_gc_bwd_q's bits.  A translation unit of its own, so that train.hip's code objects stay what they are.
//   t = (y - mu) / delta, s = LB_bound(sigma / delta), v = |t + noise| (train) | |rint(t)| (eval),
//   lik = LB_1e-9( Phi((1/2 - v)/s) - Phi((-1/2 - v)/s) ),  y_hat_pre = STE: d/dy = 1, d/dmu = 0,
//   d lik / dy = sign(t + noise) (phi_b - phi_a) / (s delta) = -d lik / dmu in training, none in eval,
//   dsigma = g (b phi_b - a phi_a) / (s delta), the scale bound tested on sigma / delta;  delta = delta(qmap[m]).
#include "common.h"
#include "gc_q.h"

template <typename T>
__global__ void __launch_bounds__(256)
gcqm_bwd_kernel(const float* __restrict__ y, int ldy, int yoff, const float* __restrict__ mu,
                const float* __restrict__ sigma, int ld_ms, const float* __restrict__ noise, int Mtot,
                const float* __restrict__ glik, const float* __restrict__ gyp, int ldg, float* __restrict__ dy, int lddy,
                T* __restrict__ dmu, T* __restrict__ dsig, int ldd, int n, int HW, int sw, float bound,
                const int* __restrict__ qmap) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n * HW * sw) return;
  const int m = i / sw, c = i - m * sw;  // m = image * HW + pixel: the map's index
  const int ch = yoff + c;
  const int b = m / HW, pix = m - b * HW;
  const size_t nchw = ((size_t)b * Mtot + ch) * HW + pix;
  const float delta = tmae_qstep(qmap[m]);
  const float t = gcq_scaled(y[(size_t)m * ldy + ch], mu[(size_t)m * ld_ms + c], delta);
  const float sr = sigma[(size_t)m * ld_ms + c] / delta;
  const float s = fmaxf(sr, bound);
  const float dd = noise ? t + noise[nchw] : rintf(t);
  const float v = fabsf(dd);
  const float a = (0.5f - v) / s, bb = (-0.5f - v) / s;
  const float k = -0.70710678118654752440f;
  const float lik = 0.5f * erfcf(k * a) - 0.5f * erfcf(k * bb);
  float g = glik ? glik[nchw] : 0.0f;
  if (!(lik >= 1e-9f || g < 0.0f)) g = 0.0f;
  const float inv_sqrt2pi = 0.39894228040143267794f;
  const float pa = inv_sqrt2pi * expf(-0.5f * a * a), pb = inv_sqrt2pi * expf(-0.5f * bb * bb);
  const float sd = s * delta;
  const float dv = g * (pb - pa) / sd;
  float ds = g * (bb * pb - a * pa) / sd;
  if (!(sr >= bound || ds < 0.0f)) ds = 0.0f;
  const float sg = dd > 0.0f ? 1.0f : (dd < 0.0f ? -1.0f : 0.0f);
  const float ddd = noise ? dv * sg : 0.0f;  // d lik / dy
  const float dyv = (gyp ? gyp[(size_t)m * ldg + ch] : 0.0f) + ddd;  // + the STE path of y_hat_pre
  dy[(size_t)m * lddy + ch] += dyv;
  dmu[(size_t)m * ldd + c] = to_out<T>(-ddd);
  dsig[(size_t)m * ldd + c] = to_out<T>(ds);
}

extern "C" int tmae_gc_bwd_qm(const float* y, int ldy, int yoff, const float* mu, const float* sigma, int ld_ms,
                              const float* noise, int Mtot, const float* glik, const float* gyp, int ldg, float* dy,
                              int lddy, void* dmu, void* dsigma, int ldd, int n, int HW, int sw, int dtype,
                              float scale_bound, const int* qmap, void* stream) {
  TMAE_REQUIRE(y && mu && sigma && dy && dmu && dsigma && qmap,
               "tmae_gc_bwd_qm: y/mu/sigma/dy/dmu/dsigma/qmap required");
  TMAE_REQUIRE(n >= 0 && HW >= 0 && sw >= 0, "tmae_gc_bwd_qm: negative extent");
  const int total = n * HW * sw;
  if (total == 0) return TMAE_OK;
  const dim3 grid(ceil_div(total, 256));
  if (dtype == TMAE_BF16)
    hipLaunchKernelGGL(gcqm_bwd_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, y, ldy, yoff, mu, sigma, ld_ms,
                       noise, Mtot, glik, gyp, ldg, dy, lddy, (bf16*)dmu, (bf16*)dsigma, ldd, n, HW, sw, scale_bound,
                       qmap);
  else
    hipLaunchKernelGGL(gcqm_bwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, y, ldy, yoff, mu, sigma, ld_ms,
                       noise, Mtot, glik, gyp, ldg, dy, lddy, (float*)dmu, (float*)dsigma, ldd, n, HW, sw, scale_bound,
                       qmap);
  TMAE_LAUNCH_CHECK("tmae_gc_bwd_qm");
}
