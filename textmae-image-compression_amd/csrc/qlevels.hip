// Side information of the per-patch quantiser steps (bitstream.py): per kept patch p of an image a
// level l[p] in 0..nlev-1 (2 <= nlev <= 16) into the image's table of ladder offsets.  Four kernels:
//   select  the levels, from the scores (rank of the kept patch among the kept patches, by counting) or from a
//           caller's map in image patch order, gathered by ids_shuffle;
//   pack    K fields of lbits = max(1, ceil(log2 nlev)) bits, LSB first, tail bits zero (tmae_ids_pack's bit order);
//   unpack  the inverse with validation and a per-image nlev, so that tiles of files with different tables decode in
//           one batch; an image with a fault gets all-zero levels, so nothing downstream reads outside a table;
//   build   qmap[b][p] = clamp(q[b] + offsets[b][l[b][p]], -32, 32), the map the _qm coding kernels take.
// Integers and comparisons only: bitstream.py restates all four in numpy and the tests compare with equality.
#include "common.h"

#define QL_MAXL 1024    // as tmae_ids_shuffle / tmae_ids_pack
#define QL_MAXLEV 16    // a level fits 4 bits
#define QL_THREADS 256

static inline int ql_bits(int nlev) {
  int bits = 1;
  while ((1 << bits) < nlev) ++bits;
  return bits;
}
__device__ __forceinline__ int ql_bits_dev(int nlev) { return nlev <= 2 ? 1 : 32 - __clz(nlev - 1); }

// One workgroup per image.  Scores: s[p] = scores[b][ids_shuffle[b][p]] staged in LDS, rank r[p] = #{p' : s[p'] > s[p]
// or (s[p'] == s[p] and p' < p)} by counting (K <= 1024: at most 4 K comparisons per thread), level = r nlev / K.  A
// NaN compares false either way, so it ranks 0: still a level in range.  Map: the gathered entry, range-checked; one
// entry outside 0..nlev-1 -> status 1 and all-zero levels.  An id outside 0..L-1 (never produced by tmae_ids_shuffle /
// tmae_ids_unpack) reads entry 0 instead of memory outside the row.
__global__ void __launch_bounds__(QL_THREADS)
qlevels_select_kernel(const float* __restrict__ scores, const int* __restrict__ map,
                      const int64_t* __restrict__ ids_shuffle, int* __restrict__ levels, int* __restrict__ status,
                      int L, int K, int nlev) {
  __shared__ float s[QL_MAXL];
  __shared__ int fault;
  const int b = blockIdx.x, t = threadIdx.x;
  const int64_t* ids = ids_shuffle + (size_t)b * L;
  int* lev = levels + (size_t)b * K;
  if (map) {
    if (t == 0) fault = 0;
    __syncthreads();
    const int* mp = map + (size_t)b * L;
    for (int p = t; p < K; p += QL_THREADS) {
      const int64_t id = ids[p];
      const int v = mp[(id >= 0 && id < L) ? (int)id : 0];
      if (v < 0 || v >= nlev) atomicOr(&fault, 1);
    }
    __syncthreads();
    const int f = fault;
    if (t == 0) status[b] = f;
    for (int p = t; p < K; p += QL_THREADS) {
      const int64_t id = ids[p];
      lev[p] = f ? 0 : mp[(id >= 0 && id < L) ? (int)id : 0];
    }
    return;
  }
  const float* sc = scores + (size_t)b * L;
  for (int p = t; p < K; p += QL_THREADS) {
    const int64_t id = ids[p];
    s[p] = sc[(id >= 0 && id < L) ? (int)id : 0];
  }
  __syncthreads();
  if (t == 0) status[b] = 0;
  for (int p = t; p < K; p += QL_THREADS) {
    const float v = s[p];
    int r = 0;
    for (int o = 0; o < K; ++o) {
      const float w = s[o];
      r += (w > v || (w == v && o < p)) ? 1 : 0;
    }
    lev[p] = (r * nlev) / K;  // r <= K - 1, so the level is <= nlev - 1
  }
}

extern "C" int tmae_qlevels_select(const float* scores, const int* map, const int64_t* ids_shuffle, int* levels,
                                   int* status, int n, int L, int K, int nlev, void* stream) {
  TMAE_REQUIRE(n >= 0 && K >= 1 && K <= L && L <= QL_MAXL, "tmae_qlevels_select: need 1 <= K=%d <= L=%d <= %d", K, L,
               QL_MAXL);
  TMAE_REQUIRE(nlev >= 2 && nlev <= QL_MAXLEV, "tmae_qlevels_select: nlev=%d outside 2..%d", nlev, QL_MAXLEV);
  TMAE_REQUIRE((scores != nullptr) != (map != nullptr), "tmae_qlevels_select: exactly one of scores and map");
  if (n == 0) return TMAE_OK;
  TMAE_REQUIRE(ids_shuffle && levels && status, "tmae_qlevels_select: null pointer");
  hipLaunchKernelGGL(qlevels_select_kernel, dim3(n), dim3(QL_THREADS), 0, (hipStream_t)stream, scores, map, ids_shuffle,
                     levels, status, L, K, nlev);
  TMAE_LAUNCH_CHECK("tmae_qlevels_select");
}

// one thread per output word: OR together the levels that touch it (ids_pack_kernel with lbits-wide fields)
__global__ void __launch_bounds__(256)
qlevels_pack_kernel(const int* __restrict__ levels, uint32_t* __restrict__ words, int K, int W, int bits, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int b = i / W, w = i - b * W;
  const int lo = 32 * w;
  const int k1 = min(K - 1, (lo + 31) / bits);
  const uint32_t mask = (1u << bits) - 1u;
  const int* lev = levels + (size_t)b * K;
  uint32_t word = 0;
  for (int k = lo / bits; k <= k1; ++k) {
    const uint32_t v = (uint32_t)lev[k] & mask;
    const int pos = k * bits - lo;  // in (-bits, 32)
    word |= pos >= 0 ? v << pos : v >> -pos;
  }
  words[i] = word;
}

extern "C" int tmae_qlevels_pack(const int* levels, uint32_t* words, int n, int K, int nlev, void* stream) {
  TMAE_REQUIRE(n >= 0 && K >= 1 && K <= QL_MAXL, "tmae_qlevels_pack: need 1 <= K=%d <= %d", K, QL_MAXL);
  TMAE_REQUIRE(nlev >= 2 && nlev <= QL_MAXLEV, "tmae_qlevels_pack: nlev=%d outside 2..%d", nlev, QL_MAXLEV);
  if (n == 0) return TMAE_OK;
  TMAE_REQUIRE(levels && words, "tmae_qlevels_pack: null pointer");
  const int bits = ql_bits(nlev), W = (K * bits + 31) / 32;
  TMAE_REQUIRE((long long)n * W < (1ll << 31), "tmae_qlevels_pack: n=%d images of %d words overflow int", n, W);
  const int total = n * W;
  hipLaunchKernelGGL(qlevels_pack_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, levels, words,
                     K, W, bits, total);
  TMAE_LAUNCH_CHECK("tmae_qlevels_pack");
}

// One workgroup per image, its own nlev.  nlev == 1: no map, no word is read, all levels 0.  Otherwise the image's
// W2 = ceil(K lbits / 32) words (W2 <= ldw, or the image counts as faulty and is not read) are range-checked first;
// status 1 a level >= nlev (or an nlev outside 1..16), 2 non-zero tail bits, the lowest that applies.
__global__ void __launch_bounds__(QL_THREADS)
qlevels_unpack_kernel(const uint32_t* __restrict__ words, int ldw, const int* __restrict__ nlev_img,
                      int* __restrict__ levels, int* __restrict__ status, int K) {
  __shared__ uint32_t faults;  // bit c: a fault of status code c was seen
  const int b = blockIdx.x, t = threadIdx.x;
  const int nlev = nlev_img[b];
  int* lev = levels + (size_t)b * K;
  if (t == 0) faults = 0;
  __syncthreads();
  const bool table_ok = nlev >= 1 && nlev <= QL_MAXLEV;
  const int bits = table_ok ? ql_bits_dev(nlev) : 1;
  const int W = (K * bits + 31) / 32;
  const bool readable = table_ok && nlev >= 2 && W <= ldw;
  const uint32_t* w = words + (size_t)b * ldw;
  const uint32_t mask = (1u << bits) - 1u;
  if (!table_ok || (nlev >= 2 && W > ldw)) {
    if (t == 0) faults = 1u << 1;
  } else if (readable) {
    for (int k = t; k < K; k += QL_THREADS) {
      const int bit = k * bits, i = bit >> 5, s = bit & 31;  // bits divides 32 or is 3: a field may cross words
      uint32_t v = w[i] >> s;
      if (s + bits > 32) v |= w[i + 1] << (32 - s);  // k < K: word i + 1 < W exists whenever the field crosses
      if ((v & mask) >= (uint32_t)nlev) atomicOr(&faults, 1u << 1);
    }
    if (t == 0) {
      const int r = (K * bits) & 31;  // the tail lies inside the last word
      if (r != 0 && (w[W - 1] >> r) != 0) atomicOr(&faults, 1u << 2);
    }
  }
  __syncthreads();
  const uint32_t f = faults;
  if (t == 0) status[b] = f ? __ffs(f) - 1 : 0;
  for (int k = t; k < K; k += QL_THREADS) {
    int out = 0;
    if (readable && f == 0) {
      const int bit = k * bits, i = bit >> 5, s = bit & 31;
      uint32_t v = w[i] >> s;
      if (s + bits > 32) v |= w[i + 1] << (32 - s);
      out = (int)(v & mask);
    }
    lev[k] = out;
  }
}

extern "C" int tmae_qlevels_unpack(const uint32_t* words, int ldw, const int* nlev, int* levels, int* status, int n,
                                   int K, void* stream) {
  TMAE_REQUIRE(n >= 0 && K >= 1 && K <= QL_MAXL && ldw >= 0, "tmae_qlevels_unpack: need 1 <= K=%d <= %d, ldw=%d >= 0",
               K, QL_MAXL, ldw);
  if (n == 0) return TMAE_OK;
  TMAE_REQUIRE(nlev && levels && status && (words || ldw == 0), "tmae_qlevels_unpack: null pointer");
  hipLaunchKernelGGL(qlevels_unpack_kernel, dim3(n), dim3(QL_THREADS), 0, (hipStream_t)stream, words, ldw, nlev, levels,
                     status, K);
  TMAE_LAUNCH_CHECK("tmae_qlevels_unpack");
}

// qmap[b][p] = clamp(q[b] + offsets[b][levels[b][p]], -32, 32); saturation is part of the definition.  The level is
// masked to the table's 16 entries, so a level no kernel above produces still reads inside the row.
__global__ void __launch_bounds__(256)
qmap_build_kernel(const int* __restrict__ levels, const int* __restrict__ q, const int* __restrict__ offsets,
                  int* __restrict__ qmap, int K, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int b = i / K;
  const int v = (q ? q[b] : 0) + offsets[b * QL_MAXLEV + (levels[i] & (QL_MAXLEV - 1))];
  qmap[i] = max(TMAE_Q_MIN, min(TMAE_Q_MAX, v));
}

extern "C" int tmae_qmap_build(const int* levels, const int* q, const int* offsets, int* qmap, int n, int K,
                               void* stream) {
  TMAE_REQUIRE(n >= 0 && K >= 1 && K <= QL_MAXL, "tmae_qmap_build: need 1 <= K=%d <= %d", K, QL_MAXL);
  if (n == 0) return TMAE_OK;
  TMAE_REQUIRE(levels && offsets && qmap, "tmae_qmap_build: null pointer");
  TMAE_REQUIRE((long long)n * K < (1ll << 31), "tmae_qmap_build: n=%d images of %d patches overflow int", n, K);
  const int total = n * K;
  hipLaunchKernelGGL(qmap_build_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, levels, q,
                     offsets, qmap, K, total);
  TMAE_LAUNCH_CHECK("tmae_qmap_build");
}
