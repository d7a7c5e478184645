// Tiled full-resolution coding (tiling.py): cut an H x W image into overlapping S x S tiles for
// the fixed-geometry model, and blend the decoded tiles back with weights that sum to one.
//
// Geometry (one definition, tiling.py): overlap O <= S / 2, stride = S - O, nx = max(1, ceil((W - O) / stride)),
// ny likewise, tile t = ty * nx + tx has its origin at (ty * stride, tx * stride).  A tile sample outside the
// image is the nearest edge pixel.  Per axis at most two tiles cover a pixel and every overlap is O wide; the
// blend weight at tile-local coordinate i is i + 1 on a side that has a neighbour and i < O, S - i on the other
// side when i >= S - O, else O + 1, so the two weights of an overlap sum to O + 1 and the 2-D products to
// (O + 1)^2.
//
// The kernels are streaming and index-only: one thread per element of the side with the coalesced f32 planes
// (tile pixel in the cut, image pixel in the blend), no LDS, no atomics.
//
// Region decode: the crops blend evaluates the pixels of R fixed-size windows, each of its own
// image, from a compact buffer that holds only the decoded tiles, through one slot map per image.  It shares the
// per-pixel arithmetic with the whole-image blend (tl_blend_pixel), so a window is the crop of that blend bit for
// bit.
#include "common.h"

#define TL_THREADS 256
#define TL_MAX_TILES 4096
#define TL_DESC 8  // int32 per window descriptor of the crops blend: H, W, y0, x0, map_base, three unused

struct tl_grid {
  int stride, nx, ny;
};

__host__ __device__ static inline int tl_count(int extent, int O, int stride) {
  return extent > O ? (int)(((long long)extent - O + stride - 1) / stride) : 1;
}

// per-axis blend weight of tile index k (of n) at local coordinate i
__device__ __forceinline__ int tl_weight(int i, int k, int n, int S, int O) {
  if (i < O && k > 0) return i + 1;
  if (i >= S - O && k < n - 1) return S - i;
  return O + 1;
}

// src [H][W][3] u8 -> tiles [nt][3][S][S] f32 = v / 255, gray [nt][S][S] u8, tiles t0 .. t0 + nt
__global__ void __launch_bounds__(TL_THREADS)
tile_cut_u8_kernel(const unsigned char* __restrict__ src, int H, int W, int S, int stride, int nx, int t0,
                   long long total, float* __restrict__ tiles, unsigned char* __restrict__ gray) {
  const long long p = (long long)blockIdx.x * TL_THREADS + threadIdx.x;
  if (p >= total) return;
  const long long SS = (long long)S * S;
  const int lt = (int)(p / SS);
  const int q = (int)(p - lt * SS);
  const int i = q / S, j = q - i * S;
  const int t = t0 + lt;
  const int ty = t / nx, tx = t - ty * nx;
  const int y = min(ty * stride + i, H - 1);
  const int x = min(tx * stride + j, W - 1);
  const unsigned char* s = src + ((size_t)y * W + x) * 3;
  const unsigned int r = s[0], g = s[1], b = s[2];
  float* o = tiles + (size_t)lt * 3 * SS + q;
  o[0] = (float)r / 255.0f;
  o[SS] = (float)g / 255.0f;
  o[2 * SS] = (float)b / 255.0f;
  gray[p] = (unsigned char)rgb_gray15(r, g, b);
}

// One pixel (y, x) of the blend, shared by the two blend kernels: sum(float(wy * wx) * v) over the covering tiles
// (ty, then tx ascending), unfused, divided once by float((O + 1)^2); a pixel one tile covers is that tile's value
// untouched.  slot_of(t) is the position of tile t = ty * nx + tx in the tile buffer.  Needs 0 <= y, 0 <= x and
// nx, ny >= 1: the local coordinates then stay inside [0, S).
template <class SlotOf>
__device__ __forceinline__ void tl_blend_pixel(const float* __restrict__ tiles, SlotOf slot_of, int y, int x, int S,
                                               int O, int stride, int nx, int ny, float& v0, float& v1, float& v2) {
#pragma clang fp contract(off)
  // the last tile covering the pixel per axis (pixels past n * stride read the last tile), and whether the one
  // before it covers the pixel as well
  const int tx1 = min(x / stride, nx - 1), ty1 = min(y / stride, ny - 1);
  const int lx = min(x - tx1 * stride, S - 1), ly = min(y - ty1 * stride, S - 1);
  const bool two_x = tx1 > 0 && lx < O, two_y = ty1 > 0 && ly < O;
  const size_t SS = (size_t)S * S;
  if (!two_x && !two_y) {
    const float* s = tiles + slot_of(ty1 * nx + tx1) * 3 * SS + (size_t)ly * S + lx;
    v0 = s[0];
    v1 = s[SS];
    v2 = s[2 * SS];
  } else {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int dy = two_y ? 1 : 0; dy >= 0; --dy) {  // ty ascending, then tx ascending
      const int ty = ty1 - dy, iy = ly + dy * stride;
      const int wy = tl_weight(iy, ty, ny, S, O);
      for (int dx = two_x ? 1 : 0; dx >= 0; --dx) {
        const int tx = tx1 - dx, ix = lx + dx * stride;
        const float w = (float)(wy * tl_weight(ix, tx, nx, S, O));
        const float* s = tiles + slot_of(ty * nx + tx) * 3 * SS + (size_t)iy * S + ix;
        a0 += w * s[0];
        a1 += w * s[SS];
        a2 += w * s[2 * SS];
      }
    }
    const float d = (float)((O + 1) * (O + 1));
    v0 = a0 / d;
    v1 = a1 / d;
    v2 = a2 / d;
  }
}

// torch's clamp(0, 1).mul(255).round().byte(): round half to even
__device__ __forceinline__ unsigned char tl_to_u8(float v) {
#pragma clang fp contract(off)
  return (unsigned char)__builtin_rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f);
}

struct tl_slot_identity {
  __device__ __forceinline__ size_t operator()(int t) const { return (size_t)t; }
};

// a compact tile buffer of n slots behind a slot map: entry base + t is tile t's slot.  Whatever the map holds,
// the index into it and the slot it gives are clamped, so a read stays inside the map and the buffer.
struct tl_slot_map {
  const int* __restrict__ map;
  long long base, len;
  int n;
  __device__ __forceinline__ size_t operator()(int t) const {
    const long long at = min(max(base + t, 0ll), len - 1);
    return (size_t)min(max(map[at], 0), n - 1);
  }
};

// tiles [nx * ny][3][S][S] f32 -> out_f32 [3][H][W] and / or out_u8 [H][W][3]
__global__ void __launch_bounds__(TL_THREADS)
tile_blend_kernel(const float* __restrict__ tiles, int H, int W, int S, int O, int stride, int nx, int ny,
                  float* __restrict__ out_f32, unsigned char* __restrict__ out_u8) {
  const long long p = (long long)blockIdx.x * TL_THREADS + threadIdx.x;
  if (p >= (long long)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (long long)y * W);
  float v0, v1, v2;
  tl_blend_pixel(tiles, tl_slot_identity(), y, x, S, O, stride, nx, ny, v0, v1, v2);
  if (out_f32 != nullptr) {
    const size_t HW = (size_t)H * W;
    out_f32[p] = v0;
    out_f32[HW + p] = v1;
    out_f32[2 * HW + p] = v2;
  }
  if (out_u8 != nullptr) {
    unsigned char* o = out_u8 + (size_t)p * 3;
    o[0] = tl_to_u8(v0);
    o[1] = tl_to_u8(v1);
    o[2] = tl_to_u8(v2);
  }
}

// R windows of h x w pixels, each of its own image, from a compact buffer of N decoded tiles: tiles [N][3][S][S],
// map: the images' slot maps one after the other (map_len entries), desc [R][TL_DESC]: the window's image H, W,
// its origin y0, x0 and the image's first map entry -> out_f32 [R][3][h][w] and / or out_u8 [R][h][w][3].
// Thread (r, i, j) is tile_blend_kernel's thread of image pixel (y0 + i, x0 + j).
__global__ void __launch_bounds__(TL_THREADS)
tile_blend_crops_kernel(const float* __restrict__ tiles, int N, const int* __restrict__ map, long long map_len,
                        const int* __restrict__ desc, int R, int h, int w, int S, int O, int stride,
                        float* __restrict__ out_f32, unsigned char* __restrict__ out_u8) {
  const long long p = (long long)blockIdx.x * TL_THREADS + threadIdx.x;
  const long long hw = (long long)h * w;
  if (p >= R * hw) return;
  const int r = (int)(p / hw);
  const int q = (int)(p - r * hw);
  const int i = q / w, j = q - i * w;
  const int* d = desc + (size_t)r * TL_DESC;
  const int H = max(d[0], 1), W = max(d[1], 1);
  const int y = (int)min(max((long long)d[2] + i, 0ll), (long long)H - 1);
  const int x = (int)min(max((long long)d[3] + j, 0ll), (long long)W - 1);
  const int nx = tl_count(W, O, stride), ny = tl_count(H, O, stride);
  const tl_slot_map slots = {map, (long long)d[4], map_len, N};
  float v0, v1, v2;
  tl_blend_pixel(tiles, slots, y, x, S, O, stride, nx, ny, v0, v1, v2);
  if (out_f32 != nullptr) {
    float* o = out_f32 + (size_t)r * 3 * hw + q;
    o[0] = v0;
    o[hw] = v1;
    o[2 * hw] = v2;
  }
  if (out_u8 != nullptr) {
    unsigned char* o = out_u8 + (size_t)p * 3;
    o[0] = tl_to_u8(v0);
    o[1] = tl_to_u8(v1);
    o[2] = tl_to_u8(v2);
  }
}

// the checks both entry points share; fills the grid
static int tl_check(const char* name, int H, int W, int S, int O, tl_grid* g) {
  TMAE_REQUIRE(H >= 1 && W >= 1, "%s: image of %dx%d pixels, both sizes must be >= 1", name, H, W);
  TMAE_REQUIRE(S >= 1 && S <= 32768, "%s: tile size %d outside 1..32768", name, S);
  TMAE_REQUIRE(O >= 0 && O <= S / 2, "%s: overlap %d outside 0..S/2 = %d", name, O, S / 2);
  g->stride = S - O;
  const long long nx = tl_count(W, O, g->stride), ny = tl_count(H, O, g->stride);
  TMAE_REQUIRE(nx * ny <= TL_MAX_TILES, "%s: %lld x %lld tiles, at most %d", name, ny, nx, TL_MAX_TILES);
  g->nx = (int)nx;
  g->ny = (int)ny;
  return TMAE_OK;
}

extern "C" int tmae_tile_cut_u8(const unsigned char* src, int H, int W, int S, int O, int t0, int nt, float* tiles,
                                unsigned char* gray, void* stream) {
  tl_grid g;
  if (int rc = tl_check("tmae_tile_cut_u8", H, W, S, O, &g)) return rc;
  const int T = g.nx * g.ny;
  TMAE_REQUIRE(t0 >= 0 && nt >= 1 && t0 <= T - nt, "tmae_tile_cut_u8: tiles %d..%d outside the image's %d", t0,
               t0 + nt, T);
  TMAE_REQUIRE(src != nullptr && tiles != nullptr && gray != nullptr, "tmae_tile_cut_u8: src / tiles / gray are NULL");
  const long long total = (long long)nt * S * S;
  const long long blocks = (total + TL_THREADS - 1) / TL_THREADS;
  TMAE_REQUIRE(blocks < (1ll << 31), "tmae_tile_cut_u8: %d tiles of %d^2 exceed the launch grid", nt, S);
  hipLaunchKernelGGL(tile_cut_u8_kernel, dim3((unsigned)blocks), dim3(TL_THREADS), 0, (hipStream_t)stream, src, H, W,
                     S, g.stride, g.nx, t0, total, tiles, gray);
  TMAE_LAUNCH_CHECK("tmae_tile_cut_u8");
}

extern "C" int tmae_tile_blend(const float* tiles, int H, int W, int S, int O, float* out_f32, unsigned char* out_u8,
                               void* stream) {
  tl_grid g;
  if (int rc = tl_check("tmae_tile_blend", H, W, S, O, &g)) return rc;
  TMAE_REQUIRE(tiles != nullptr, "tmae_tile_blend: tiles is NULL");
  TMAE_REQUIRE(out_f32 != nullptr || out_u8 != nullptr, "tmae_tile_blend: out_f32 and out_u8 are both NULL");
  const long long blocks = ((long long)H * W + TL_THREADS - 1) / TL_THREADS;
  TMAE_REQUIRE(blocks < (1ll << 31), "tmae_tile_blend: %dx%d pixels exceed the launch grid", H, W);
  hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)blocks), dim3(TL_THREADS), 0, (hipStream_t)stream, tiles, H, W,
                     S, O, g.stride, g.nx, g.ny, out_f32, out_u8);
  TMAE_LAUNCH_CHECK("tmae_tile_blend");
}

extern "C" int tmae_tile_blend_crops(const float* tiles, int N, const int* map, long long map_len, const int* desc,
                                     int R, int h, int w, int S, int O, float* out_f32, unsigned char* out_u8,
                                     void* stream) {
  const char* name = "tmae_tile_blend_crops";
  TMAE_REQUIRE(S >= 1 && S <= 32768, "%s: tile size %d outside 1..32768", name, S);
  TMAE_REQUIRE(O >= 0 && O <= S / 2, "%s: overlap %d outside 0..S/2 = %d", name, O, S / 2);
  TMAE_REQUIRE(R >= 1 && h >= 1 && w >= 1, "%s: %d windows of %dx%d pixels, all three must be >= 1", name, R, h, w);
  TMAE_REQUIRE(N >= 1 && map_len >= 1, "%s: %d tile slots and %lld map entries, both must be >= 1", name, N, map_len);
  TMAE_REQUIRE(tiles != nullptr && map != nullptr && desc != nullptr, "%s: tiles / map / desc are NULL", name);
  TMAE_REQUIRE(out_f32 != nullptr || out_u8 != nullptr, "%s: out_f32 and out_u8 are both NULL", name);
  TMAE_REQUIRE((long long)h * w < (1ll << 31), "%s: windows of %dx%d pixels exceed the launch grid", name, h, w);
  const long long blocks = ((long long)R * h * w + TL_THREADS - 1) / TL_THREADS;
  TMAE_REQUIRE(blocks < (1ll << 31), "%s: %d windows of %dx%d pixels exceed the launch grid", name, R, h, w);
  hipLaunchKernelGGL(tile_blend_crops_kernel, dim3((unsigned)blocks), dim3(TL_THREADS), 0, (hipStream_t)stream, tiles,
                     N, map, map_len, desc, R, h, w, S, O, S - O, out_f32, out_u8);
  TMAE_LAUNCH_CHECK("tmae_tile_blend_crops");
}
