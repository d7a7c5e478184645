// One whole slice-transform stack per workgroup, activations resident in LDS (bf16).
//
// cc_transform_mean[i] / cc_transform_scale[i] / lrp_transform[i] (MCM.py:165-293, applied at
// MCM.py:761-784) are five 3x3 convs (224 -> 176 -> 128 -> 80 -> 32 channels at the default config)
// with GELU between them, over the 12x12 latent grid.  Run layer by layer (conv_halo.h) every layer is
// a separate launch of 64-256 workgroups whose ~0.7 us per (chunk, tap) step chain, not the MFMA rate,
// sets the time, and the serial slice chain (slices 0..5) is a row of such launches.  Here ONE
// workgroup owns one (problem, image) and runs the whole stack:
//   * the layer-0 input (y_hat slices, MCM.py:756-760, torch.cat of two sources without a copy) goes
//     global -> LDS once; every layer's output stays in LDS (two ping-pong buffers, 144 rows of up to
//     224 channels each) and is the next layer's input -- no HBM round trip between layers;
//   * weights never touch LDS: they are pre-packed in MFMA fragment order ([tap][k32][cout16][lane][8])
//     so every A-fragment is one coalesced 1-KiB wave load from L2 (all images of a problem share them),
//     prefetched 4-6 K-steps ahead into VGPRs; so the K loop has NO workgroup barrier at all, only the
//     one between layers;
//   * pixel fragments are 16 consecutive pixels; tap (dy, dx) shifts the LDS row by dy*G + dx, pixels
//     whose tap falls outside the grid read the matching row of a 16-row zero block.  Row pitch =
//     2 * round32(C) + 32 bytes, so every fragment read is bank-conflict-free for every tap shift.
// Work split: 8 waves (two per SIMD); a wave item = two 16-channel output fragments x all 9 pixel
// fragments (224-wide layers), x a pixel half (176 / 128), or one fragment x a half (80 / 32); items
// dealt round-robin to the waves (the layer loop below).
// Chain mode (TMAE_LIC_STACK_CHAIN): a slice's mean-stack workgroups go on with the slice's lrp stack.
// MFMA v_mfma_f32_16x16x32_bf16 issued swapped (A = weights 16 couts x 32 k, B = 32 k x 16 pixels):
// each lane ends with 4 consecutive output channels of one pixel (one 8-B LDS store per fragment).
// The first layer's epilogue adds the latent-channel partial sums (the P buffer of mcm.py _slices) and
// the last layer's writes mu / sigma (f32) or, for lrp, y_hat = y_hat_pre + 0.5 tanh(.) (MCM.py:779-784).
#include "lic_stack_kernel.h"

// the QSTEP instantiations and their launches (lic_stack_q.hip: a step per image, lic_stack_qm.hip: a step per pixel)
int lic_stack_launch_q(const tmae_lic_stack_args& a, int nwg, hipStream_t stream);
int lic_stack_launch_qm(const tmae_lic_stack_args& a, int nwg, hipStream_t stream);

extern "C" int tmae_lic_stack(const tmae_lic_stack_args* args, void* stream) {
  using namespace lstk;
  TMAE_REQUIRE(args != nullptr, "tmae_lic_stack: args is NULL");
  const tmae_lic_stack_args& a = *args;
  TMAE_REQUIRE(a.G >= 1 && a.G * a.G <= MAXPIX, "tmae_lic_stack: grid %dx%d exceeds %d pixels", a.G, a.G, MAXPIX);
  TMAE_REQUIRE(a.nlayers >= 1 && a.nlayers <= TMAE_LIC_STACK_MAXL, "tmae_lic_stack: %d layers", a.nlayers);
  TMAE_REQUIRE(a.nb1 >= 1 && a.nb2 >= 1 && a.n >= 1, "tmae_lic_stack: batch %d x %d, n %d", a.nb1, a.nb2, a.n);
  const bool bwd = (a.flags & TMAE_LIC_STACK_BWD) != 0;
  TMAE_REQUIRE(!a.cq || (!bwd && (a.flags & TMAE_LIC_STACK_CHAIN)),
               "tmae_lic_stack: cq (the chain's quantiser step) needs TMAE_LIC_STACK_CHAIN and no TMAE_LIC_STACK_BWD");
  TMAE_REQUIRE(!a.cqm || !a.cq, "tmae_lic_stack: cqm (a step per pixel) and cq (a step per image) exclude each other");
  TMAE_REQUIRE(!a.cqm || !bwd, "tmae_lic_stack: cqm (the chain's quantiser steps per pixel) takes no TMAE_LIC_STACK_BWD");
  TMAE_REQUIRE(!a.cqm || (a.flags & TMAE_LIC_STACK_CHAIN),
               "tmae_lic_stack: cqm (the chain's quantiser steps per pixel) needs TMAE_LIC_STACK_CHAIN");
  TMAE_REQUIRE(a.x1 != nullptr && (a.y != nullptr || bwd), "tmae_lic_stack: x1 / y required");
  if (bwd) {
    TMAE_REQUIRE(!(a.flags & TMAE_LIC_STACK_CHAIN) && !a.addend && !a.lrp_src && !a.x2 && !a.sv_t,
                 "tmae_lic_stack: the backward chain takes no chain / addend / lrp / second source");
    const bool rt = a.racc[0] != nullptr;
    for (int l = 0; l < a.nlayers; ++l)
      TMAE_REQUIRE(a.w[l] && ((rt && l + 1 == a.nlayers) || (a.sv_pre[l] && a.sv_act[l])),
                   "tmae_lic_stack: backward layer %d needs w / sv_pre / sv_act", l);
    if (rt) {
      const int cl = a.cout[a.nlayers - 1];
      // the routed accumulators step by the problem's nb1 index only (racc + b1 * rs)
      TMAE_REQUIRE(a.nb2 <= 1, "tmae_lic_stack: routed accumulators need nb2 == 1 (got %d)", a.nb2);
      TMAE_REQUIRE(a.rlim[0] >= 0 && a.rlim[0] <= a.rlim[1] && a.rlim[1] <= a.rlim[2] && a.rlim[2] == cl &&
                   a.rlim[0] % 4 == 0 && a.rlim[1] % 4 == 0, "tmae_lic_stack: routes %d / %d / %d of %d channels",
                   a.rlim[0], a.rlim[1], a.rlim[2], cl);
      for (int r = 0; r < 3; ++r)
        TMAE_REQUIRE((r == 0 ? a.rlim[0] : a.rlim[r] - a.rlim[r - 1]) == 0 || (a.racc[r] && a.rld[r] % 4 == 0),
                     "tmae_lic_stack: route %d accumulator", r);
    }
  }
  TMAE_REQUIRE(a.c1 >= 0 && a.c2 >= 0 && (a.c2 == 0 || a.x2 != nullptr), "tmae_lic_stack: channels %d + %d", a.c1, a.c2);
  TMAE_REQUIRE(a.c1 % 8 == 0 && a.c2 % 8 == 0 && a.ld1 % 8 == 0 && (a.c2 == 0 || a.ld2 % 8 == 0),
               "tmae_lic_stack: input channels / strides must be multiples of 8");
  TMAE_REQUIRE(pad32(a.c1 + a.c2) <= MAXC, "tmae_lic_stack: %d input channels exceed %d", a.c1 + a.c2, MAXC);
  for (int l = 0; l < a.nlayers; ++l) {
    TMAE_REQUIRE((a.w[l] != nullptr || (l == 0 && a.c1 + a.c2 == 0)) && (a.bias[l] != nullptr || bwd),
                 "tmae_lic_stack: layer %d weights", l);
    TMAE_REQUIRE(a.cout[l] >= 4 && a.cout[l] % 8 == 0, "tmae_lic_stack: layer %d cout %d (multiple of 8)", l, a.cout[l]);
    TMAE_REQUIRE((l + 1 == a.nlayers && (!bwd || a.racc[0])) || pad32(a.cout[l]) <= MAXC,
                 "tmae_lic_stack: layer %d cout %d exceeds %d", l, a.cout[l], MAXC);
  }
  TMAE_REQUIRE(!a.lrp_src || !a.y_f32, "tmae_lic_stack: lrp output is bf16");
  if (a.flags & TMAE_LIC_STACK_CHAIN) {
    TMAE_REQUIRE(a.nb1 == 2 && a.y_f32 && !a.lrp_src && a.cn >= 1 && a.cn <= TMAE_LIC_STACK_MAXL,
                 "tmae_lic_stack: chain needs the 2 x nb2 mean / scale problems with f32 outputs");
    TMAE_REQUIRE(a.ccout[a.cn - 1] == a.cout[a.nlayers - 1] && a.cx1 && a.yv && a.csrc && a.cy,
                 "tmae_lic_stack: chain operands");
    TMAE_REQUIRE(a.cc1 % 8 == 0 && a.cld1 % 8 == 0 && a.ldyv % 4 == 0 && a.cld_src % 4 == 0 && a.ldy % 4 == 0 &&
                 pad32(a.cc1 + a.ccout[a.cn - 1]) <= MAXC, "tmae_lic_stack: chain channels %d + %d", a.cc1,
                 a.ccout[a.cn - 1]);
    for (int l = 0; l < a.cn; ++l)
      TMAE_REQUIRE(a.cw[l] && a.cb[l] && a.ccout[l] % 8 == 0 && (l + 1 == a.cn || pad32(a.ccout[l]) <= MAXC),
                   "tmae_lic_stack: chain layer %d", l);
  }
  if (a.addend) TMAE_REQUIRE(a.ld_add % 4 == 0, "tmae_lic_stack: addend stride %d", a.ld_add);
  for (int l = 0; l < a.nlayers; ++l)
    TMAE_REQUIRE(!a.sv_pre[l] == !a.sv_act[l], "tmae_lic_stack: layer %d keeps pre-activation and output together", l);
  for (int l = 0; l < a.cn && (a.flags & TMAE_LIC_STACK_CHAIN); ++l)
    TMAE_REQUIRE(!a.csv_pre[l] == !a.csv_act[l], "tmae_lic_stack: chain layer %d keeps pre and output together", l);
  TMAE_REQUIRE(!a.sv_t || a.lrp_src, "tmae_lic_stack: sv_t is the lrp stack's pre-tanh value");
  const int nwg = a.n * a.nb1 * a.nb2;
  if (bwd) hipLaunchKernelGGL((lic_stack_kernel<true, 0>), dim3(nwg), dim3(NW * 64), 0, (hipStream_t)stream, a);
  else if (a.cq) return lic_stack_launch_q(a, nwg, (hipStream_t)stream);
  else if (a.cqm) return lic_stack_launch_qm(a, nwg, (hipStream_t)stream);
  else hipLaunchKernelGGL((lic_stack_kernel<false, 0>), dim3(nwg), dim3(NW * 64), 0, (hipStream_t)stream, a);
  TMAE_LAUNCH_CHECK("tmae_lic_stack");
}

// ================================================================== latent-channel partial sums
// tmae_lic_latent: the first convs' latent part of every slice stack as ONE packed conv (cin <= 384, one image x 16
// output fragments per workgroup).  The halo kernel (conv_halo.h) it replaces stages the weight slab of every
// (64-channel chunk, tap) step through LDS behind a barrier: operands of both sides read from LDS and a barrier per
// step.  Here, as in lic_stack, the image's input rows stay in LDS for the whole K sweep and every wave streams its
// own two weight fragments per K-step from L2 into registers: no barrier inside the sweep, B reads shared by two
// MFMAs.  Summation order per output: taps outer, 32-channel steps inner.
namespace llat {
constexpr int NW = 8, FPW = 2 * NW;  // fragments per workgroup (one pair per wave)
constexpr int MAXCIN = 384;
constexpr unsigned PMAX = lstk::pitch(MAXCIN);
constexpr unsigned ZOFF = lstk::MAXPIX * PMAX;  // 16 zero rows past the 144 input rows
constexpr unsigned TMASK = ZOFF + 16 * PMAX;
constexpr int LDS_BYTES = TMASK + 320;
}  // namespace llat
__device__ __forceinline__ constexpr unsigned llat_zoff() { return llat::ZOFF; }
__device__ __forceinline__ constexpr unsigned llat_tmask() { return llat::TMASK; }

// one wave: output fragments f0, f0 + 1 x all 9 pixel fragments over the 9 x NKC K-steps.  The tap loop is rolled
// (108 unrolled steps at cin 384 left the ring arrays in scratch); inside a tap the NKC steps are unrolled, and
// with D | NKC the A ring's slots stay static registers across taps (step s in slot (s mod NKC) mod D).
// epilogue operands of one problem: output (f32 or bf16, rows ldy apart) starting at the problem's first fragment's
// column, optional bias over those columns, optional GELU
struct LlatOut {
  void* y;
  int ldy, bf, act;
  const float* bias;
};

template <int NKC>
__device__ __forceinline__ void llat_item(const bf16* w, int nfr, long long blk, int f0, int fcol, bool two,
                                          const unsigned char* lb, unsigned pin, int G, int npix, int img,
                                          const LlatOut& o, int lane) {
  constexpr int MF = 9, NS = 9 * NKC;
  constexpr int D = NKC % 4 == 0 ? 4 : NKC % 3 == 0 ? 3 : NKC % 2 == 0 ? 2 : (NKC <= 7 ? NKC : 1);
  asm volatile("" : "+v"(lane));
  const int fr = lane & 15, fq = lane >> 4;
  f32x4 acc[2][MF];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < MF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const unsigned sstride = (unsigned)nfr * 512u;
  const bf16* wl[2];
  bf16x8 ar[D][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int f = two || i == 0 ? f0 + i : f0;  // a lone last fragment: the pair's second half re-reads the first
    const int b = f / nfr, fi = f - b * nfr;
    wl[i] = w + b * blk + ((size_t)fi * 64 + lane) * 8;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      ar[d][i] = *reinterpret_cast<const bf16x8*>(wl[i]);
      wl[i] += sstride;
    }
  }
  unsigned tmask[MF];
#pragma unroll
  for (int j = 0; j < MF; ++j) tmask[j] = *reinterpret_cast<const unsigned short*>(lb + llat_tmask() + 2 * (16 * j + fr));
  auto row = [&](int t, int j) -> unsigned {
    const int p = 16 * j + fr, sh = (t / 3 - 1) * G + (t % 3 - 1);
    const unsigned r = (unsigned)(p + sh);
    return ((tmask[j] >> t) & 1u ? r * pin : llat_zoff() + (r & 15u) * pin) + 16u * fq;
  };
  bf16x8 bv[2][MF];
  unsigned rb[MF];
#pragma unroll
  for (int j = 0; j < MF; ++j) {
    rb[j] = row(0, j);
    bv[0][j] = *reinterpret_cast<const bf16x8*>(lb + rb[j]);
  }
  for (int t = 0; t < 9; ++t) {
    unsigned rn[MF];
#pragma unroll
    for (int j = 0; j < MF; ++j) rn[j] = row(t + 1 < 9 ? t + 1 : t, j);
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      if (kc + 1 < NKC) {
#pragma unroll
        for (int j = 0; j < MF; ++j) bv[(kc + 1) & 1][j] = *reinterpret_cast<const bf16x8*>(lb + rb[j] + 64u * (kc + 1));
      } else if (t + 1 < 9) {
#pragma unroll
        for (int j = 0; j < MF; ++j) bv[(kc + 1) & 1][j] = *reinterpret_cast<const bf16x8*>(lb + rn[j]);
      }
      bf16x8 a0[2];
      const bool more = t * NKC + kc + D < NS;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a0[i] = ar[kc % D][i];
        if (more) {
          ar[kc % D][i] = *reinterpret_cast<const bf16x8*>(wl[i]);
          wl[i] += sstride;
        }
      }
#pragma unroll
      for (int j = 0; j < MF; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[i], bv[kc & 1][j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (NKC & 1) {  // odd step count per tap: the next tap's first B fragments went to buffer 1
#pragma unroll
      for (int j = 0; j < MF; ++j) bv[0][j] = bv[1][j];
    }
#pragma unroll
    for (int j = 0; j < MF; ++j) rb[j] = rn[j];
  }
  // lane: columns fcol + 16 i + 4 fq .. + 3 (fragment f0 + i) of pixel 16 j + fr
  f32x4 bias[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    bias[i] = o.bias ? load4f(o.bias + fcol + 16 * (two ? i : 0) + 4 * fq) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < MF; ++j) {
    const int p = 16 * j + fr;
    if (p >= npix) continue;
    const size_t at = ((size_t)img * npix + p) * o.ldy + fcol + 4 * fq;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i == 1 && !two) break;
      f32x4 v = acc[i][j] + bias[i];
      if (o.act == TMAE_ACT_GELU) {
        const f32x2 lo = gelu2_bf16out(v.xy), hi = gelu2_bf16out(v.zw);
        v = f32x4{lo.x, lo.y, hi.x, hi.y};
      }
      if (o.bf) store4(reinterpret_cast<bf16*>(o.y) + at + 16 * i, v);
      else store4(reinterpret_cast<float*>(o.y) + at + 16 * i, v);
    }
  }
}

template <int NKC>
__global__ void __launch_bounds__(llat::NW * 64) lic_latent_kernel(tmae_lic_latent_args a) {
  using namespace llat;
  __shared__ __attribute__((aligned(16))) uint4 lds[LDS_BYTES / 16];
  unsigned char* lb = reinterpret_cast<unsigned char*>(lds);
  const int n = a.n, G = a.G, npix = G * G, cin = 32 * NKC;
  const int t = xcd_remap(blockIdx.x, gridDim.x);  // tile-major: an XCD's run shares its tiles' weights in L2
  const int tile = t / n, img = t - tile * n, prob = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned pin = lstk::pitch(cin);
  for (int i = tid; i < 16 * (int)pin / 16; i += NW * 64) reinterpret_cast<uint4*>(lds)[ZOFF / 16 + i] = uint4{0, 0, 0, 0};
  for (int p = tid; p < 160; p += NW * 64) {
    unsigned m = 0;
    if (p < npix) {
      const int py = p / G, px = p - py * G;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int yy = py + k / 3 - 1, xx = px + k % 3 - 1;
        m |= ((unsigned)yy < (unsigned)G && (unsigned)xx < (unsigned)G) ? (1u << k) : 0u;
      }
    }
    *reinterpret_cast<unsigned short*>(lb + TMASK + 2 * p) = (unsigned short)m;
  }
  {
    const bf16* x = reinterpret_cast<const bf16*>(a.x[prob]);
    constexpr int q = 4 * NKC;  // 16-B pieces per row
    for (int i = tid; i < npix * q; i += NW * 64) {
      const int p = i / q, ch = 8 * (i - p * q);
      *reinterpret_cast<uint4*>(lb + p * pin + 2 * ch) =
          *reinterpret_cast<const uint4*>(x + ((size_t)img * npix + p) * a.ldx + ch);
    }
  }
  __syncthreads();
  const int fr0 = a.f_lo + tile * FPW + 2 * wave;  // this wave's first fragment, relative to the problem's
  if (fr0 >= a.f_hi) return;  // past this launch's fragments (no barrier follows)
  LlatOut o;
  o.ldy = a.ldy;
  o.bf = a.y_bf16;
  o.act = a.act;
  o.bias = a.bias[prob];
  o.y = a.y_bf16 ? (void*)(reinterpret_cast<bf16*>(a.y) + a.y_s[prob]) : (void*)(a.y + a.y_s[prob]);
  llat_item<NKC>(reinterpret_cast<const bf16*>(a.w), a.nfr, a.blk, a.f_off[prob] + fr0, 16 * fr0, fr0 + 1 < a.f_hi, lb,
                 pin, G, npix, img, o, lane);
}

extern "C" int tmae_lic_latent(const tmae_lic_latent_args* args, void* stream) {
  TMAE_REQUIRE(args != nullptr, "tmae_lic_latent: args is NULL");
  const tmae_lic_latent_args& a = *args;
  TMAE_REQUIRE(a.G >= 1 && a.G * a.G <= lstk::MAXPIX, "tmae_lic_latent: grid %dx%d", a.G, a.G);
  TMAE_REQUIRE(a.cin >= 32 && a.cin % 32 == 0 && a.cin <= llat::MAXCIN, "tmae_lic_latent: cin %d (multiple of 32, <= %d)",
               a.cin, llat::MAXCIN);
  TMAE_REQUIRE(a.nb >= 1 && a.nb <= TMAE_LIC_LATENT_MAXP && a.n >= 1, "tmae_lic_latent: %d problems, %d images", a.nb,
               a.n);
  TMAE_REQUIRE(a.w && a.y && a.ldx % 8 == 0 && a.ldx >= a.cin, "tmae_lic_latent: operands / strides");
  TMAE_REQUIRE(a.nfr >= 1 && a.f_lo >= 0 && a.f_hi > a.f_lo && a.f_lo % 2 == 0, "tmae_lic_latent: fragments [%d, %d) "
               "of blocks of %d (f_lo even)", a.f_lo, a.f_hi, a.nfr);
  TMAE_REQUIRE(a.blk >= 9LL * (a.cin / 32) * a.nfr * 512 || a.f_off[0] + a.f_hi <= a.nfr, "tmae_lic_latent: block stride");
  TMAE_REQUIRE(a.act == TMAE_ACT_NONE || a.act == TMAE_ACT_GELU, "tmae_lic_latent: act %d", a.act);
  TMAE_REQUIRE(a.ldy % 4 == 0 && (a.ldy >= 16 * a.f_hi), "tmae_lic_latent: ldy %d", a.ldy);
  for (int j = 0; j < a.nb; ++j)
    TMAE_REQUIRE(a.x[j] && a.f_off[j] >= 0 && a.y_s[j] % 4 == 0, "tmae_lic_latent: problem %d", j);
  const int ntile = (a.f_hi - a.f_lo + llat::FPW - 1) / llat::FPW;
  const dim3 grid(a.n * ntile, a.nb);
  hipStream_t st = (hipStream_t)stream;
  switch (a.cin / 32) {
#define LLAT_CASE(K) \
  case K: hipLaunchKernelGGL(lic_latent_kernel<K>, grid, dim3(llat::NW * 64), 0, st, a); break;
    LLAT_CASE(1) LLAT_CASE(2) LLAT_CASE(3) LLAT_CASE(4) LLAT_CASE(5) LLAT_CASE(6)
    LLAT_CASE(7) LLAT_CASE(8) LLAT_CASE(9) LLAT_CASE(10) LLAT_CASE(11) LLAT_CASE(12)
#undef LLAT_CASE
    default: break;
  }
  TMAE_LAUNCH_CHECK("tmae_lic_latent");
}
