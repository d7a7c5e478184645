// Model inputs on the device: the reference loader's per-sample work (utils/dataloader.py:57-73 --
// Image.open().convert("RGB"), transforms.Resize((224, 224), BICUBIC) on the PIL image, ToTensor, Normalize)
// after the decode, and the grayscale conversion in front of the score-map producer (scores.imread_gray).
//
// Pillow's 8-bit resample (ImagingResample, libImaging/Resample.c) is integer arithmetic: per axis a table of
// 22-bit fixed-point coefficients kk[out][ksize] and tap ranges bounds[out] = (xmin, n), built in doubles on
// the host (ops.resize_tables restates precompute_coeffs / normalize_coeffs_8bpc); every output value is
//   clip8((2^21 + sum_{t < n} px[xmin + t] * kk[xx][t]) >> 22)        (int32 sum, arithmetic shift)
// and the two passes run horizontal first, then vertical, with a uint8 image between them -- the rounding to
// 8 bits between the passes is part of the result.  A pass whose input and output sizes are equal is skipped.
// The kernels below do exactly that, so the output equals Image.resize bit for bit.
//
// Horizontal pass: one workgroup takes RS_ROWS source rows x a tile of output columns.  The source columns the
// tile's taps cover are staged in LDS with aligned dword loads (a row is 3 W bytes, so rows start at any byte
// offset: each staged row keeps its own misalignment), then every (row, output column) item walks its taps
// over LDS bytes; its coefficient row kk[xo][0 .. n) is contiguous per lane, so the compiler fetches several taps per
// load and the table (a few tens of KB) stays cache resident.  The tap count comes from the table: no per-thread
// coefficient array.  Vertical pass: a workgroup owns one output row, its coefficient row and tap range are
// wave-uniform, threads walk the row's bytes, every load coalesced.
// Whichever pass runs last stores the output form: uint8 HWC, or f32 NCHW as ToTensor (v / 255) with the
// optional Normalize ((x - mean) / std) -- the same f32 operations in the same order as crop_normalize_u8_kernel
// (misc.hip), so the result is torch's bitwise.
#include "common.h"

#define RS_THREADS 256
#define RS_ROWS 4
#define RS_ROW_BYTES 12288                    // staged bytes per source row, misalignment included
#define RS_MAX_COLS ((RS_ROW_BYTES - 4) / 3)  // source columns one tile may span
#define RS_PRECISION_BITS 22

// Normalize's per-channel mean / std travel as six scalar kernel arguments and are picked with selects: a struct
// indexed by the run-time channel would be copied to scratch
struct rs_norm {
  float m0, m1, m2, s0, s1, s2;
};
#define RS_NORM_PARAMS float m0, float m1, float m2, float s0, float s1, float s2
#define RS_NORM_ARGS(nm) (nm).m0, (nm).m1, (nm).m2, (nm).s0, (nm).s1, (nm).s2

__device__ __forceinline__ int rs_clip8(int acc) { return min(max(acc >> RS_PRECISION_BITS, 0), 255); }

// value v of image b, output pixel (y, x), channel c (mean m, std s) in the output form MODE
template <int MODE>
__device__ __forceinline__ void rs_store(void* __restrict__ out, int v, int b, int y, int x, int c, int Ho, int Wo,
                                         float m, float s) {
  if constexpr (MODE == TMAE_RESIZE_U8_HWC) {
    static_cast<unsigned char*>(out)[(((size_t)b * Ho + y) * Wo + x) * 3 + c] = (unsigned char)v;
  } else {
    float f = v / 255.0f;
    if constexpr (MODE == TMAE_RESIZE_F32_NCHW_NORM) f = (f - m) / s;
    static_cast<float*>(out)[(((size_t)b * 3 + c) * Ho + y) * Wo + x] = f;
  }
}

// src [n][H][W][3] -> out rows of Wo pixels (H rows per image).  grid.x = n * ceil(H / RS_ROWS),
// grid.y = ceil(Wo / tx): tx output columns per workgroup, chosen on the host so that their taps span at most
// RS_MAX_COLS source columns; the span is clamped here as well, so a bad table cannot read outside the image
// or the staged rows.
template <int MODE>
__global__ void __launch_bounds__(RS_THREADS)
resize_h_kernel(const unsigned char* __restrict__ src, int n, int H, int W, int Wo, const int* __restrict__ kk,
                const int* __restrict__ bounds, int ksize, int tx, void* __restrict__ out, RS_NORM_PARAMS) {
  __shared__ unsigned int seg[RS_ROWS][RS_ROW_BYTES / 4];
  const int row_tiles = (H + RS_ROWS - 1) / RS_ROWS;
  const int b = blockIdx.x / row_tiles;
  const int y0 = (blockIdx.x - b * row_tiles) * RS_ROWS;
  const int rows = min(RS_ROWS, H - y0);
  const int xo0 = blockIdx.y * tx;
  const int nxo = min(tx, Wo - xo0);
  // the tile's source span: tap ranges move right with the output column
  int seg_lo = min(max(bounds[2 * xo0], 0), W);
  const int last = xo0 + nxo - 1;
  int seg_hi = min(max(bounds[2 * last] + bounds[2 * last + 1], seg_lo), W);
  seg_hi = min(seg_hi, seg_lo + RS_MAX_COLS);
  const int nbytes = (seg_hi - seg_lo) * 3;
  const unsigned char* lo_addr = src;
  const unsigned char* hi_addr = src + (size_t)n * H * W * 3;
  for (int r = 0; r < rows; ++r) {
    const unsigned char* g = src + (((size_t)b * H + y0 + r) * W + seg_lo) * 3;
    const int mis = (int)((uintptr_t)g & 3);
    const unsigned char* ga = g - mis;  // aligned down: LDS byte mis + i holds g[i]
    const int ndw = (mis + nbytes + 3) >> 2;
    for (int d = threadIdx.x; d < ndw; d += RS_THREADS) {
      const unsigned char* a = ga + 4 * (size_t)d;
      unsigned int v;
      if (a >= lo_addr && a + 4 <= hi_addr) {
        v = *reinterpret_cast<const unsigned int*>(a);
      } else {  // the first / last dword of the whole batch: only the bytes inside it
        v = 0;
        for (int j = 0; j < 4; ++j)
          if (a + j >= lo_addr && a + j < hi_addr) v |= (unsigned int)a[j] << (8 * j);
      }
      seg[r][d] = v;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rows * nxo; i += RS_THREADS) {
    const int r = i / nxo;
    const int xo = xo0 + (i - r * nxo);
    const int x0 = min(max(bounds[2 * xo], seg_lo), seg_hi);
    const int cnt = min(min(bounds[2 * xo + 1], ksize), seg_hi - x0);
    const unsigned char* g = src + (((size_t)b * H + y0 + r) * W + seg_lo) * 3;
    const int mis = (int)((uintptr_t)g & 3);
    const unsigned char* p = reinterpret_cast<const unsigned char*>(seg[r]) + mis + 3 * (x0 - seg_lo);
    const int* k = kk + (size_t)xo * ksize;
    int a0 = 1 << (RS_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < cnt; ++t) {
      const int kv = k[t];
      a0 += (int)p[3 * t] * kv;
      a1 += (int)p[3 * t + 1] * kv;
      a2 += (int)p[3 * t + 2] * kv;
    }
    rs_store<MODE>(out, rs_clip8(a0), b, y0 + r, xo, 0, H, Wo, m0, s0);
    rs_store<MODE>(out, rs_clip8(a1), b, y0 + r, xo, 1, H, Wo, m1, s1);
    rs_store<MODE>(out, rs_clip8(a2), b, y0 + r, xo, 2, H, Wo, m2, s2);
  }
}

// src [n][H][Wo][3] -> out [n][Ho] rows.  grid.x = n * Ho (one output row each), grid.y covers the row's
// 3 Wo bytes.  kk == nullptr copies row yo of the source (both passes skipped: only the output form changes).
template <int MODE>
__global__ void __launch_bounds__(RS_THREADS)
resize_v_kernel(const unsigned char* __restrict__ src, int H, int Wo, int Ho, const int* __restrict__ kk,
                const int* __restrict__ bounds, int ksize, void* __restrict__ out, RS_NORM_PARAMS) {
  const int b = blockIdx.x / Ho;
  const int yo = blockIdx.x - b * Ho;
  const int rowbytes = 3 * Wo;
  const int j = blockIdx.y * RS_THREADS + threadIdx.x;
  if (j >= rowbytes) return;
  int v;
  if (kk == nullptr) {
    v = src[((size_t)b * H + min(yo, H - 1)) * rowbytes + j];
  } else {
    const int y0 = min(max(bounds[2 * yo], 0), H);
    const int cnt = min(min(bounds[2 * yo + 1], ksize), H - y0);
    const int* k = kk + (size_t)yo * ksize;
    const unsigned char* p = src + ((size_t)b * H + y0) * rowbytes + j;
    int acc = 1 << (RS_PRECISION_BITS - 1);
    for (int t = 0; t < cnt; ++t) acc += (int)p[(size_t)t * rowbytes] * k[t];
    v = rs_clip8(acc);
  }
  const int x = j / 3, c = j - 3 * x;
  rs_store<MODE>(out, v, b, yo, x, c, Ho, Wo, c == 0 ? m0 : (c == 1 ? m1 : m2), c == 0 ? s0 : (c == 1 ? s1 : s2));
}

template <int MODE>
static void launch_h(hipStream_t st, const unsigned char* src, int n, int H, int W, int Wo, const int* kk,
                     const int* bounds, int ksize, int tx, void* out, rs_norm nm) {
  const dim3 grid((unsigned)((long long)n * ceil_div(H, RS_ROWS)), (unsigned)ceil_div(Wo, tx));
  hipLaunchKernelGGL(resize_h_kernel<MODE>, grid, dim3(RS_THREADS), 0, st, src, n, H, W, Wo, kk, bounds, ksize, tx,
                     out, RS_NORM_ARGS(nm));
}

template <int MODE>
static void launch_v(hipStream_t st, const unsigned char* src, int n, int H, int Wo, int Ho, const int* kk,
                     const int* bounds, int ksize, void* out, rs_norm nm) {
  const dim3 grid((unsigned)((long long)n * Ho), (unsigned)ceil_div(3 * Wo, RS_THREADS));
  hipLaunchKernelGGL(resize_v_kernel<MODE>, grid, dim3(RS_THREADS), 0, st, src, H, Wo, Ho, kk, bounds, ksize, out,
                     RS_NORM_ARGS(nm));
}

#define RS_DISPATCH(mode, fn, ...)                                               \
  do {                                                                           \
    if ((mode) == TMAE_RESIZE_U8_HWC) fn<TMAE_RESIZE_U8_HWC>(__VA_ARGS__);       \
    else if ((mode) == TMAE_RESIZE_F32_NCHW) fn<TMAE_RESIZE_F32_NCHW>(__VA_ARGS__); \
    else fn<TMAE_RESIZE_F32_NCHW_NORM>(__VA_ARGS__);                             \
  } while (0)

extern "C" long long tmae_resize_u8_workspace(int n, int H, int W, int Ho, int Wo) {
  if (n < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return 0;
  return (W != Wo && H != Ho) ? (long long)n * H * Wo * 3 : 0;  // the uint8 image between the two passes
}

extern "C" int tmae_resize_u8(const unsigned char* src, int n, int H, int W, int Ho, int Wo, const int* kk_h,
                              const int* bounds_h, int ksize_h, const int* kk_v, const int* bounds_v, int ksize_v,
                              int out_mode, const float* mean, const float* std, void* out, unsigned char* work,
                              long long work_bytes, void* stream) {
  TMAE_REQUIRE(n >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1,
               "tmae_resize_u8: sizes must be >= 1, got n=%d %dx%d -> %dx%d", n, H, W, Ho, Wo);
  const long long lim = 1ll << 31;
  TMAE_REQUIRE((long long)n * ceil_div(H, RS_ROWS) < lim && (long long)n * Ho < lim && 3ll * W < lim && 3ll * Wo < lim,
               "tmae_resize_u8: n=%d %dx%d -> %dx%d exceeds the launch grid", n, H, W, Ho, Wo);
  TMAE_REQUIRE(src != nullptr && out != nullptr, "tmae_resize_u8: src / out are NULL");
  TMAE_REQUIRE(kk_h != nullptr && bounds_h != nullptr && kk_v != nullptr && bounds_v != nullptr,
               "tmae_resize_u8: a coefficient or bounds table is NULL");
  TMAE_REQUIRE(ksize_h >= 1 && ksize_v >= 1, "tmae_resize_u8: ksize must be >= 1, got %d / %d", ksize_h, ksize_v);
  TMAE_REQUIRE(out_mode == TMAE_RESIZE_U8_HWC || out_mode == TMAE_RESIZE_F32_NCHW ||
                   out_mode == TMAE_RESIZE_F32_NCHW_NORM,
               "tmae_resize_u8: unknown output mode %d", out_mode);
  rs_norm nm = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f};
  if (out_mode == TMAE_RESIZE_F32_NCHW_NORM) {
    TMAE_REQUIRE(mean != nullptr && std != nullptr, "tmae_resize_u8: mean / std are NULL");
    nm = {mean[0], mean[1], mean[2], std[0], std[1], std[2]};
  }
  const long long need = tmae_resize_u8_workspace(n, H, W, Ho, Wo);
  TMAE_REQUIRE(need == 0 || (work != nullptr && work_bytes >= need),
               "tmae_resize_u8: workspace too small (%lld bytes, needs %lld)", work ? work_bytes : 0ll, need);
  hipStream_t st = (hipStream_t)stream;
  const bool do_h = W != Wo, do_v = H != Ho;
  int tx = RS_THREADS;
  if (do_h) {
    // tx output columns span at most (tx - 1) * scale + 1 + ksize source columns
    TMAE_REQUIRE(ksize_h + 2 <= RS_MAX_COLS, "tmae_resize_u8: %d horizontal taps exceed the staged row (%d columns)",
                 ksize_h, RS_MAX_COLS);
    const double scale = (double)W / (double)Wo;
    const double fit = (double)(RS_MAX_COLS - ksize_h - 2) / scale + 1.0;
    if (fit < (double)tx) tx = (int)fit;
    if (tx < 1) tx = 1;
    TMAE_REQUIRE(ceil_div(Wo, tx) <= 65535, "tmae_resize_u8: %d -> %d columns needs too many tiles", W, Wo);
  }
  TMAE_REQUIRE(ceil_div(3 * Wo, RS_THREADS) <= 65535, "tmae_resize_u8: %d output columns exceed the launch grid", Wo);
  if (do_h && do_v) {
    launch_h<TMAE_RESIZE_U8_HWC>(st, src, n, H, W, Wo, kk_h, bounds_h, ksize_h, tx, work, nm);
    TMAE_LAUNCH_CHECK_NORET("tmae_resize_u8");
    RS_DISPATCH(out_mode, launch_v, st, work, n, H, Wo, Ho, kk_v, bounds_v, ksize_v, out, nm);
  } else if (do_h) {
    RS_DISPATCH(out_mode, launch_h, st, src, n, H, W, Wo, kk_h, bounds_h, ksize_h, tx, out, nm);
  } else if (do_v) {
    RS_DISPATCH(out_mode, launch_v, st, src, n, H, Wo, Ho, kk_v, bounds_v, ksize_v, out, nm);
  } else {  // Pillow returns a copy
    RS_DISPATCH(out_mode, launch_v, st, src, n, H, Wo, Ho, (const int*)nullptr, (const int*)nullptr, 1, out, nm);
  }
  TMAE_LAUNCH_CHECK("tmae_resize_u8");
}

// ---------------------------------------------------------------------------------------------- RGB -> gray
// scores.imread_gray for non-JPEG files: gray = rgb_gray15 (common.h)

// four pixels per thread: three aligned dwords in, one out (both pointers 4-byte aligned)
__global__ void __launch_bounds__(RS_THREADS)
rgb_to_gray4_kernel(const unsigned int* __restrict__ rgb, long long ngroups, unsigned int* __restrict__ gray) {
  const long long i = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
  if (i >= ngroups) return;
  const unsigned int w0 = rgb[3 * i], w1 = rgb[3 * i + 1], w2 = rgb[3 * i + 2];
  const unsigned int g0 = rgb_gray15(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255);
  const unsigned int g1 = rgb_gray15(w0 >> 24, w1 & 255, (w1 >> 8) & 255);
  const unsigned int g2 = rgb_gray15((w1 >> 16) & 255, w1 >> 24, w2 & 255);
  const unsigned int g3 = rgb_gray15((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24);
  gray[i] = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
}

__global__ void __launch_bounds__(RS_THREADS)
rgb_to_gray_kernel(const unsigned char* __restrict__ rgb, long long first, long long npixels,
                   unsigned char* __restrict__ gray) {
  const long long i = first + (long long)blockIdx.x * RS_THREADS + threadIdx.x;
  if (i >= npixels) return;
  gray[i] = (unsigned char)rgb_gray15(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
}

extern "C" int tmae_rgb_to_gray_u8(const unsigned char* rgb, long long npixels, unsigned char* gray, void* stream) {
  TMAE_REQUIRE(npixels >= 1, "tmae_rgb_to_gray_u8: needs at least one pixel, got %lld", npixels);
  TMAE_REQUIRE(rgb != nullptr && gray != nullptr, "tmae_rgb_to_gray_u8: rgb / gray are NULL");
  TMAE_REQUIRE(npixels < (1ll << 39), "tmae_rgb_to_gray_u8: %lld pixels exceed the launch grid", npixels);
  hipStream_t st = (hipStream_t)stream;
  long long done = 0;
  if ((((uintptr_t)rgb | (uintptr_t)gray) & 3) == 0 && npixels >= 4) {
    const long long groups = npixels / 4;
    hipLaunchKernelGGL(rgb_to_gray4_kernel, dim3((unsigned)((groups + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS),
                       0, st, reinterpret_cast<const unsigned int*>(rgb), groups, reinterpret_cast<unsigned int*>(gray));
    TMAE_LAUNCH_CHECK_NORET("tmae_rgb_to_gray_u8");
    done = groups * 4;
  }
  if (done < npixels) {
    const long long rest = npixels - done;
    hipLaunchKernelGGL(rgb_to_gray_kernel, dim3((unsigned)((rest + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS), 0,
                       st, rgb, done, npixels, gray);
  }
  TMAE_LAUNCH_CHECK("tmae_rgb_to_gray_u8");
}
