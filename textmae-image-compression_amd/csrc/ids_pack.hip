// Side information of the per-image bitstream (bitstream.py, DESIGN.md "Container format"): the ordered list of kept
// patch ids, ids_shuffle[b][0..K), as K fields of bits = max(1, ceil(log2 L)) bits each.  Id k occupies bits
// [k * bits, (k + 1) * bits) of the image's bit string, LSB first; bit i of the string is bit i % 32 of word i / 32;
// W = ceil(K * bits / 32) words per image, unused tail bits zero.
//
// The decoder's output depends on nothing else of the permutation (tmae_decoder_embed_fwd places token k at row
// 1 + ids_shuffle[b][k-1], tmae_mask_rows fills the other rows whatever their order), so unpack completes it with the
// unused ids in ascending order, and it is the one place where ids from outside are validated: an image whose words
// do not hold K distinct ids below L gets the identity permutation, so that no later kernel indexes outside its rows.
#include "common.h"

#define IDS_MAXL 1024  // as tmae_ids_shuffle; bits <= 10, so an id spans at most two words
#define UNPACK_THREADS 256

static inline int ids_bits(int L) {
  int bits = 1;
  while ((1 << bits) < L) ++bits;
  return bits;
}

// one thread per output word: OR together the ids that touch it (at most ceil(32 / bits) + 1)
__global__ void __launch_bounds__(256)
ids_pack_kernel(const int64_t* __restrict__ ids_shuffle, uint32_t* __restrict__ words, int L, int K, int W, int bits,
                int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int b = i / W, w = i - b * W;
  const int lo = 32 * w;                          // first bit of this word
  const int k1 = min(K - 1, (lo + 31) / bits);    // last id with a bit in it
  const uint32_t mask = (1u << bits) - 1u;
  const int64_t* ids = ids_shuffle + (size_t)b * L;
  uint32_t word = 0;
  for (int k = lo / bits; k <= k1; ++k) {
    const uint32_t id = (uint32_t)ids[k] & mask;
    const int pos = k * bits - lo;                // in (-bits, 32)
    word |= pos >= 0 ? id << pos : id >> -pos;
  }
  words[i] = word;
}

extern "C" int tmae_ids_pack(const int64_t* ids_shuffle, uint32_t* words, int n, int L, int K, void* stream) {
  TMAE_REQUIRE(n >= 0 && K >= 1 && K <= L && L <= IDS_MAXL, "tmae_ids_pack: need 1 <= K=%d <= L=%d <= %d", K, L,
               IDS_MAXL);
  if (n == 0) return TMAE_OK;
  TMAE_REQUIRE(ids_shuffle && words, "tmae_ids_pack: null pointer");
  const int bits = ids_bits(L), W = (K * bits + 31) / 32;
  TMAE_REQUIRE((long long)n * W < (1ll << 31), "tmae_ids_pack: n=%d images of %d words overflow int", n, W);
  const int total = n * W;
  hipLaunchKernelGGL(ids_pack_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, ids_shuffle, words,
                     L, K, W, bits, total);
  TMAE_LAUNCH_CHECK("tmae_ids_pack");
}

// id k of an image's words (k < K, so word w + 1 exists whenever the id crosses into it)
__device__ __forceinline__ uint32_t ids_field(const uint32_t* __restrict__ w, int k, int bits, uint32_t mask) {
  const int bit = k * bits, i = bit >> 5, s = bit & 31;
  uint32_t v = w[i] >> s;
  if (s + bits > 32) v |= w[i + 1] << (32 - s);
  return v & mask;
}

// One workgroup per image.  Pass 1 range-checks every id and enters it in an LDS presence bitmap (an atomicOr that
// finds its bit already set is a duplicate); one thread checks the tail bits.  A fault of any kind -> status and
// the identity.  Otherwise pass 2 writes ids_shuffle[0..K) and their inverse, and every id whose bit is clear takes
// position K + (its rank among the clear bits), from popcount prefixes over the bitmap words.
__global__ void __launch_bounds__(UNPACK_THREADS)
ids_unpack_kernel(const uint32_t* __restrict__ words, int64_t* __restrict__ ids_shuffle,
                  int64_t* __restrict__ ids_restore, int* __restrict__ status, int L, int K, int W, int bits) {
  __shared__ uint32_t present[IDS_MAXL / 32];
  __shared__ int before[IDS_MAXL / 32];  // unused ids below bitmap word j
  __shared__ uint32_t faults;            // bit c: a fault of status code c was seen
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint32_t* w = words + (size_t)b * W;
  int64_t* shuf = ids_shuffle + (size_t)b * L;
  int64_t* rest = ids_restore + (size_t)b * L;
  const uint32_t mask = (1u << bits) - 1u;
  if (tid < IDS_MAXL / 32) present[tid] = 0;
  if (tid == 0) faults = 0;
  __syncthreads();
  for (int k = tid; k < K; k += UNPACK_THREADS) {
    const uint32_t id = ids_field(w, k, bits, mask);
    if (id >= (uint32_t)L) {
      atomicOr(&faults, 1u << 1);
    } else {
      const uint32_t bit = 1u << (id & 31);
      if (atomicOr(&present[id >> 5], bit) & bit) atomicOr(&faults, 1u << 2);
    }
  }
  if (tid == 0) {
    const int r = (K * bits) & 31;  // the tail lies inside the last word
    if (r != 0 && (w[W - 1] >> r) != 0) atomicOr(&faults, 1u << 3);
  }
  __syncthreads();
  const uint32_t f = faults;
  if (f != 0) {  // the lowest code wins: 1 id >= L, 2 duplicate id, 3 non-zero tail bits
    if (tid == 0) status[b] = __ffs(f) - 1;
    for (int i = tid; i < L; i += UNPACK_THREADS) {
      shuf[i] = i;
      rest[i] = i;
    }
    return;
  }
  const int nbm = (L + 31) >> 5;
  if (tid < nbm) {
    int c = 0;
    for (int j = 0; j < tid; ++j) c += __popc(~present[j]);  // words below the last hold 32 valid ids each
    before[tid] = c;
  }
  __syncthreads();
  if (tid == 0) status[b] = 0;
  for (int k = tid; k < K; k += UNPACK_THREADS) {
    const uint32_t id = ids_field(w, k, bits, mask);
    shuf[k] = id;
    rest[id] = k;
  }
  for (int i = tid; i < L; i += UNPACK_THREADS) {
    const uint32_t unused = ~present[i >> 5], bit = 1u << (i & 31);
    if (unused & bit) {
      const int pos = K + before[i >> 5] + __popc(unused & (bit - 1u));  // < L: exactly L - K ids are unused
      shuf[pos] = i;
      rest[i] = pos;
    }
  }
}

extern "C" int tmae_ids_unpack(const uint32_t* words, int64_t* ids_shuffle, int64_t* ids_restore, int* status, int n,
                               int L, int K, void* stream) {
  TMAE_REQUIRE(n >= 0 && K >= 1 && K <= L && L <= IDS_MAXL, "tmae_ids_unpack: need 1 <= K=%d <= L=%d <= %d", K, L,
               IDS_MAXL);
  if (n == 0) return TMAE_OK;
  TMAE_REQUIRE(words && ids_shuffle && ids_restore && status, "tmae_ids_unpack: null pointer");
  const int bits = ids_bits(L), W = (K * bits + 31) / 32;
  hipLaunchKernelGGL(ids_unpack_kernel, dim3(n), dim3(UNPACK_THREADS), 0, (hipStream_t)stream, words, ids_shuffle,
                     ids_restore, status, L, K, W, bits);
  TMAE_LAUNCH_CHECK("tmae_ids_unpack");
}
