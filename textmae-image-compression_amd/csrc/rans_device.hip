// Device rANS coder behind MCM.compress_batch / decompress_batch: one independent stream per image, each bit for
// bit what the host coder (rans.cpp) writes for that image alone.  The format is restated from the top of rans.cpp:
//   * 64-bit state in [2^31, 2^63), 32-bit words written from the END of the buffer and read from the front, an
//     8-byte state flush (low word first) at the front of the stream;
//   * 16-bit precision: symbol s of row c occupies [cdf[s], cdf[s+1]) of 2^16;
//   * a value outside [offset, offset + size - 2) is coded as the row's last symbol (size - 2) followed by 4-bit
//     bypass digits: the digit count (<= 8, so always one count digit), then the raw value (negatives 2|v|-1,
//     overflow 2(v - max)) LSB digit first;
//   * the encoder walks the symbols in reverse, last first, and for an escaped symbol puts the value digits (last
//     first), the count digit and then the symbol, so the decoder reads symbol, count, digits in forward order.
//
// Stream layout (both directions): stream b codes segments j = 0..nseg-1 in order, segment j being seg_len
// consecutive int32 at base + j * seg_stride + b * stream_stride (separate strides for symbols and indexes).
//
// One wave per stream: the only serial chain is the state update.  Per 64-symbol chunk the lanes do what is
// parallel (index / symbol loads, clamp + escape, the cdf row reads and the exact reciprocal of the frequency for
// encode) and keep the results in registers; the walk over the chunk is wave-uniform code that fetches symbol k's
// fields with v_readlane, so the state lives in scalar registers and the chain is scalar arithmetic (lane 0
// stores).  The chunks are software-pipelined, one stage per level of dependent loads, so that every load is
// consumed one chunk walk after it was issued.  Every loop's trip count comes from the arguments, never from
// stream content.
#include "common.h"

namespace {

constexpr uint64_t kRansLow = 1ull << 31;
constexpr int kWave = 64;
constexpr int kMaxWinRows = 128;  // 64-entry int32 windows kept in LDS: 32 KB at most

// per-stream status words (0 = fine)
enum {
  kStOverflow = 1,  // encode / pack: the output slab (or dense buffer) would overflow
  kStSymbol = 2,    // decode: symbol search fell outside the row
  kStEscape = 3,    // decode: escape longer than 8 digits
  kStOverrun = 4,   // decode: read past the stream's length
  kStIndex = 5,     // a table index outside [0, ncdf)
  kStStream = 6,    // decode: stream offset / length / position outside the word buffer
};

// lane `lane` (wave-uniform) of v, as a scalar
__device__ __forceinline__ int bcast_i(int v, int lane) {
  return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(lane));
}
__device__ __forceinline__ uint32_t bcast_u(uint32_t v, int lane) { return (uint32_t)bcast_i((int)v, lane); }

// ------------------------------------------------------------------------------------------------ encode
// The arithmetic of the format lives in the helpers of this section and of "decode" below; the wave-per-stream
// kernels and the thread-per-sub-stream kernels ("lanes") differ in schedule only and both call them.
struct EncState {
  uint64_t x;
  long long head;  // words [head, cap) of the slab are written
  int st;
};

// `store`: this thread writes the word (lane 0 of a wave that shares one state, every thread that owns its state)
__device__ __forceinline__ void enc_emit(EncState& e, uint32_t* __restrict__ slab, bool store) {
  if (e.head <= 0) {  // the slab is full: stop this stream, never write outside it
    e.st = kStOverflow;
    return;
  }
  --e.head;
  if (store) slab[e.head] = (uint32_t)e.x;
  e.x >>= 32;
}

// raw bits: freq = 2^12 of 2^16, so x_max = 2^12 << 47
__device__ __forceinline__ void enc_put_bits(EncState& e, uint32_t* __restrict__ slab, bool store, uint32_t val) {
  if (e.st) return;
  if (e.x >= (1ull << 59)) enc_emit(e, slab, store);
  if (e.st) return;
  e.x = (e.x << 4) | val;
}

// the 8-byte state flush: high word first (the buffer grows downward), so the stream starts with the low word
__device__ __forceinline__ void enc_flush(EncState& e, uint32_t* __restrict__ slab, bool store) {
  if (e.st == 0 && e.head < 2) e.st = kStOverflow;
  if (e.st) return;
  e.head -= 2;
  if (store) {
    slab[e.head + 1] = (uint32_t)(e.x >> 32);
    slab[e.head] = (uint32_t)e.x;
  }
}

// stage C: a symbol v of a row (offset, size entries) -> the value coded through the row; outside [0, size - 2) it is
// the row's last symbol with raw = 2|v|-1 (below) or 2(v - max) (above) in ndig nibbles (up to the top non-zero one)
struct EncValue {
  int value;
  uint32_t raw, esc, ndig;
};

__device__ __forceinline__ EncValue enc_clamp_escape(int v, int off, int size) {
  const int max_value = size - 2;
  EncValue r{(int)((uint32_t)v - (uint32_t)off), 0u, 0u, 0u};
  if (r.value < 0) {
    r.raw = (uint32_t)(-2 * (long long)r.value - 1);
    r.value = max_value;
  } else if (r.value >= max_value) {
    r.raw = (uint32_t)(2 * (long long)(r.value - max_value));
    r.value = max_value;
  }
  if (r.value == max_value) {
    r.esc = 1;
    r.ndig = r.raw ? 8u - ((uint32_t)__clz((int)r.raw) >> 2) : 0u;
  }
  return r;
}

// exact reciprocal of freq in [2, 2^16) (ryg_rans Rans64EncSymbolInit): floor(x / freq) = mulhi(x, rcp) >> shift for
// x < 2^63, rcp = ceil(2^(shift + 64) / freq), shift = ceil(log2 freq) - 1; the 128-bit dividend has the base-2^16
// digits [2^(shift+15), 0, 0, freq - 1], so the long division is four 32-bit divisions
__device__ __forceinline__ uint64_t enc_reciprocal(uint32_t freq, uint32_t& shift) {
  const uint32_t bits = 32u - (uint32_t)__clz((int)(freq - 1));  // ceil(log2 freq)
  const uint32_t a = 1u << (bits + 15);
  const uint32_t q1 = a / freq, r1 = a - q1 * freq;
  const uint32_t q2 = (r1 << 16) / freq, r2 = (r1 << 16) - q2 * freq;
  const uint32_t q3 = (r2 << 16) / freq, r3 = (r2 << 16) - q3 * freq;
  const uint32_t q4 = ((r3 << 16) + (freq - 1)) / freq;
  shift = bits - 1;
  return ((((uint64_t)q1 << 16) + q2) << 32) + (((uint64_t)q3 << 16) + q4);
}

// stage D: the fields of the put step from a symbol's two cdf entries
struct EncSymbol {
  uint64_t rcp;
  uint32_t freq, shift, bias;
};

__device__ __forceinline__ EncSymbol enc_symbol(uint32_t start, uint32_t next) {
  EncSymbol s{~0ull, next - start, 0u, start + (1u << 16) - 1};  // freq 1: q = x - 1, so x + bias + q (2^16 - 1) =
  if (s.freq >= 2) {                                             // (x << 16) + start
    s.rcp = enc_reciprocal(s.freq, s.shift);
    s.bias = start;
  }
  return s;
}

// the put step: a state x >= freq << 47 stores a word first, then x += bias + floor(x / freq) (2^16 - freq)
__device__ __forceinline__ bool enc_must_emit(uint64_t x, uint32_t freq) { return (uint32_t)(x >> 32) >= (freq << 15); }

__device__ __forceinline__ uint64_t enc_put(uint64_t x, uint32_t freq, uint32_t shift, uint64_t rcp, uint32_t bias) {
  const uint64_t q = __umul64hi(x, rcp) >> shift;
  return x + bias + q * (uint64_t)((1u << 16) - freq);
}

__global__ void __launch_bounds__(kWave)
rans_encode_streams_kernel(const int* __restrict__ sym, long long sym_ss, long long sym_ts, const int* __restrict__ idx,
                           long long idx_ss, long long idx_ts, int nseg, int seg_len, const int* __restrict__ cdfs,
                           int cdf_stride, const int* __restrict__ sizes, const int* __restrict__ offs, int ncdf,
                           uint32_t* __restrict__ slabs, long long cap, int* __restrict__ nwords,
                           int* __restrict__ status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = nseg * seg_len;
  uint32_t* __restrict__ slab = slabs + (size_t)b * cap;
  EncState e{kRansLow, cap, 0};
  const int nchunks = (n + kWave - 1) / kWave;
  // pipeline registers.  Stage A: index and symbol of a chunk; B: its row's size and offset; C: clamp / escape and
  // the two cdf entries; D: reciprocal, then the walk.  In iteration t the stages hold chunks t, t-1, t-2, t-3 of the
  // reversed order (chunk nchunks-1 first).
  int a_ci = 0, a_v = 0;
  int b_ci = 0, b_v = 0, b_size = 3, b_off = 0;
  uint32_t c_start = 0, c_next = 1, c_raw = 0, c_flags = 0;  // flags: escaped | ndig << 1 | bad index << 8
  bool b_bad = false;
  for (int t = 0; t < nchunks + 3 && e.st == 0; ++t) {
    // ---- D: fields of the chunk walked in this iteration, from the cdf entries loaded one iteration ago
    const int cd = nchunks - 1 - (t - 3);
    uint32_t d_rcp_lo = 0, d_rcp_hi = 0, d_bias = 0, d_meta = 0, d_raw = c_raw;
    bool d_bad = false;
    if (t >= 3) {
      const EncSymbol s = enc_symbol(c_start, c_next);
      d_bias = s.bias;
      d_rcp_lo = (uint32_t)s.rcp;
      d_rcp_hi = (uint32_t)(s.rcp >> 32);
      // meta = freq (17 bits) | shift << 17 (5 bits) | escaped << 22 | ndig << 23
      d_meta = s.freq | (s.shift << 17) | ((c_flags & 1u) << 22) | (((c_flags >> 1) & 15u) << 23);
      d_bad = (c_flags >> 8) & 1u;
    }
    // ---- C: clamp and escape the value, issue the loads of cdf[value] and cdf[value + 1]
    if (t >= 2 && t < nchunks + 2) {
      const EncValue v = enc_clamp_escape(b_v, b_off, b_size);
      const int* __restrict__ row = cdfs + (size_t)b_ci * cdf_stride;
      c_start = (uint32_t)row[v.value];
      c_next = (uint32_t)row[v.value + 1];
      c_raw = v.raw;
      c_flags = v.esc | (v.ndig << 1) | (b_bad ? 1u << 8 : 0u);
    }
    // ---- B: the row's size and offset (lanes past the end of the stream code nothing: row 0, never walked)
    if (t >= 1 && t < nchunks + 1) {
      b_bad = a_ci < 0 || a_ci >= ncdf;
      b_ci = b_bad ? 0 : a_ci;
      b_v = a_v;
      b_size = sizes[b_ci];
      b_off = offs[b_ci];
    }
    // ---- A: index and symbol
    if (t < nchunks) {
      const int i = (nchunks - 1 - t) * kWave + lane;
      a_ci = 0;
      a_v = 0;
      if (i < n) {
        const int j = i / seg_len, k = i - j * seg_len;
        a_ci = idx[j * idx_ss + b * idx_ts + k];
        a_v = sym[j * sym_ss + b * sym_ts + k];
      }
    }
    if (t < 3) continue;
    // ---- walk chunk cd, last symbol first
    if (__any(d_bad)) {
      e.st = kStIndex;
      break;
    }
    const int cnt = min(kWave, n - cd * kWave);
    for (int k = cnt - 1; k >= 0 && e.st == 0; --k) {
      const uint32_t m = bcast_u(d_meta, k);
      const uint32_t freq = m & 0x1FFFF, shift = (m >> 17) & 31;
      if ((m >> 22) & 1) {
        const uint32_t r = bcast_u(d_raw, k);
        const int ndig = (int)(m >> 23);
        for (int d = 7; d >= 0; --d)
          if (d < ndig) enc_put_bits(e, slab, lane == 0, (r >> (4 * d)) & 15u);
        enc_put_bits(e, slab, lane == 0, (uint32_t)ndig);
        if (e.st) break;
      }
      if (enc_must_emit(e.x, freq)) {
        enc_emit(e, slab, lane == 0);
        if (e.st) break;
      }
      const uint64_t rcp = (uint64_t)bcast_u(d_rcp_lo, k) | ((uint64_t)bcast_u(d_rcp_hi, k) << 32);
      e.x = enc_put(e.x, freq, shift, rcp, bcast_u(d_bias, k));
    }
  }
  enc_flush(e, slab, lane == 0);
  if (lane == 0) {
    nwords[b] = e.st ? 0 : (int)(cap - e.head);
    status[b] = e.st;
  }
}

// ------------------------------------------------------------------------------------------------ pack
// dense[offsets[b] .. offsets[b] + nwords[b]) = the tail of slab b; offsets[nstreams] = the total
__global__ void __launch_bounds__(256)
rans_pack_streams_kernel(const uint32_t* __restrict__ slabs, long long cap, const int* __restrict__ nwords, int nstreams,
                         uint32_t* __restrict__ dense, long long dense_cap, long long* __restrict__ offsets,
                         int* __restrict__ status) {
  __shared__ long long s_part[256];
  const int b = blockIdx.x, t = threadIdx.x;
  long long part = 0;
  for (int i = t; i < b; i += 256) part += min((long long)max(nwords[i], 0), cap);
  s_part[t] = part;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) s_part[t] += s_part[t + s];
    __syncthreads();
  }
  const long long off = s_part[0];
  long long nw = min((long long)max(nwords[b], 0), cap);
  if (off + nw > dense_cap) {
    nw = 0;
    if (t == 0) status[b] = kStOverflow;
  }
  if (t == 0) {
    offsets[b] = off;
    if (b == nstreams - 1) offsets[nstreams] = off + nw;
  }
  const uint32_t* __restrict__ src = slabs + (size_t)b * cap + (cap - nw);
  for (long long i = t; i < nw; i += 256) dense[off + i] = src[i];
}

// ------------------------------------------------------------------------------------------------ decode
__device__ __forceinline__ int win_start(int size) { return size > kWave ? size / 2 - kWave / 2 : 0; }

struct DecState {
  uint64_t x;
  int pos, len;    // next word to read, words in the stream
  int wbase;       // lane l of wbuf holds word wbase + l
  uint32_t wbuf;
  int st;
};

__device__ __forceinline__ uint32_t dec_next_word(DecState& d, const uint32_t* __restrict__ w, int lane) {
  if (d.pos < 0 || d.pos >= d.len) {
    d.st = kStOverrun;
    return 0;
  }
  int r = d.pos - d.wbase;
  if (r < 0 || r >= kWave) {
    d.wbase = d.pos;
    d.wbuf = d.pos + lane < d.len ? w[d.pos + lane] : 0u;
    r = 0;
  }
  ++d.pos;
  return bcast_u(d.wbuf, r);
}

// the thread-per-sub-stream decoder's state ("lanes" below): the next word waits in a register
struct LaneDec {
  uint64_t x;
  int pos, len;    // next word to read, words in the sub-stream
  uint32_t nextw;  // words[pos] while pos < len: loaded when the word before it was taken
  int st;
};

__device__ __forceinline__ uint32_t dec_next_word(LaneDec& d, const uint32_t* __restrict__ w, int) {
  if (d.pos < 0 || d.pos >= d.len) {
    d.st = kStOverrun;
    return 0;
  }
  const uint32_t r = d.nextw;
  ++d.pos;
  d.nextw = d.pos < d.len ? w[d.pos] : 0u;
  return r;
}

// D = DecState or LaneDec in what follows: the arithmetic is one, only dec_next_word differs
template <class D>
__device__ __forceinline__ void dec_renorm(D& d, const uint32_t* __restrict__ w, int lane) {
  if (d.x < kRansLow) d.x = (d.x << 32) | dec_next_word(d, w, lane);
}

// advance over the symbol [start, next) found for cum = x & 0xFFFF: x = freq * (x >> 16) + cum - start, then renormalise
template <class D>
__device__ __forceinline__ void dec_advance(D& d, const uint32_t* __restrict__ w, int lane, int cum, int start,
                                            int next) {
  d.x = (uint64_t)(uint32_t)(next - start) * (d.x >> 16) + (uint64_t)(uint32_t)cum - (uint32_t)start;
  dec_renorm(d, w, lane);
}

template <class D>
__device__ __forceinline__ uint32_t dec_get_bits4(D& d, const uint32_t* __restrict__ w, int lane) {
  const uint32_t v = (uint32_t)(d.x & 15u);
  d.x >>= 4;
  dec_renorm(d, w, lane);
  return v;
}

// the escape read: the count digit, then the raw value LSB digit first -> the value (kStEscape: more than 8 digits)
template <class D>
__device__ __forceinline__ int dec_escape(D& d, const uint32_t* __restrict__ w, int lane, int max_value) {
  int value = max_value;
  const uint32_t ndig = dec_get_bits4(d, w, lane);  // 15 = "another count digit follows": more than 8 anyway
  if (ndig > 8) {
    d.st = kStEscape;
  } else {
    uint32_t raw = 0;
    for (uint32_t q = 0; q < 8; ++q)
      if (q < ndig && d.st == 0) raw |= dec_get_bits4(d, w, lane) << (4 * q);
    const int half = (int)(raw >> 1);
    value = (raw & 1) ? -half - 1 : half + max_value;
  }
  return value;
}

// open a (sub-)stream of d.len words at word `off`: the state flush on the first call, the carried state and cursor
// after it -> the stream's words (read only while d.st == 0)
template <class D>
__device__ __forceinline__ const uint32_t* dec_open(D& d, const uint32_t* __restrict__ words, long long total_words,
                                                    long long off, int first, unsigned long long state, int pos) {
  if (d.st == 0 && (off < 0 || d.len < 2 || off + d.len > total_words)) d.st = kStStream;
  const uint32_t* __restrict__ w = words + (d.st == 0 ? off : 0);
  if (d.st == 0) {
    if (first) {
      d.x = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
      d.pos = 2;
    } else {
      d.x = state;
      d.pos = pos;
      if (d.pos < 2 || d.pos > d.len) d.st = kStStream;
    }
  }
  return w;
}

// s_win[r][i] = entry win_start(size) + i of row r < win_rows, INT_MAX past its end; one 64-thread block
__device__ __forceinline__ void dec_fill_windows(int* __restrict__ s_win, int win_rows, const int* __restrict__ cdfs,
                                                 int cdf_stride, const int* __restrict__ sizes, int t) {
#pragma unroll 4
  for (int r = 0; r < win_rows; ++r) {
    const int size = sizes[r], ent = win_start(size) + t;
    s_win[r * kWave + t] = ent < size ? cdfs[(size_t)r * cdf_stride + ent] : INT_MAX;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kWave)
rans_decode_streams_kernel(const uint32_t* __restrict__ words, long long total_words, const long long* __restrict__ woff,
                           const int* __restrict__ wlen, const int* __restrict__ idx, long long idx_ss, long long idx_ts,
                           int* __restrict__ out, long long out_ss, long long out_ts, int seg0, int nseg, int seg_len,
                           const int* __restrict__ cdfs, int cdf_stride, const int* __restrict__ sizes,
                           const int* __restrict__ offs, int ncdf, int win_rows, unsigned long long* __restrict__ state,
                           int* __restrict__ pos, int* __restrict__ status, int first) {
  extern __shared__ int s_win[];  // [win_rows][64]: entries win_start(size) + l of each row, INT_MAX past its end
  const int b = blockIdx.x, lane = threadIdx.x;
  dec_fill_windows(s_win, win_rows, cdfs, cdf_stride, sizes, lane);

  DecState d{0, 0, wlen[b], 0, 0u, first ? 0 : status[b]};
  const uint32_t* __restrict__ w = dec_open(d, words, total_words, woff[b], first, state[b], pos[b]);
  if (d.st == 0) {
    d.wbase = d.pos;
    d.wbuf = d.pos + lane < d.len ? w[d.pos + lane] : 0u;
  }

  const int n = nseg * seg_len;
  const int nchunks = (n + kWave - 1) / kWave;
  // pipeline registers.  Stage A: the indexes of a chunk; B: their rows' sizes and offsets; then the walk.  In
  // iteration t the stages hold chunks t, t-1 and t-2.
  int a_ci = 0;
  int b_ci = 0, b_size = 3, b_off = 0;
  bool b_bad = false;
  for (int t = 0; t < nchunks + 2; ++t) {
    const int ci = b_ci, size_l = b_size, off_l = b_off;
    const bool bad = b_bad;
    if (t >= 1 && t < nchunks + 1) {
      b_bad = a_ci < 0 || a_ci >= ncdf;
      b_ci = b_bad ? 0 : a_ci;
      b_size = sizes[b_ci];
      b_off = offs[b_ci];
    }
    if (t < nchunks) {
      const int i = t * kWave + lane;
      a_ci = 0;
      if (i < n) {
        const int j = i / seg_len, kk = i - j * seg_len;
        a_ci = idx[(seg0 + j) * idx_ss + b * idx_ts + kk];
      }
    }
    if (t < 2) continue;
    // ---- walk chunk c
    const int c = t - 2;
    if (d.st == 0 && __any(bad)) d.st = kStIndex;
    int myval = 0;
    const int cnt = min(kWave, n - c * kWave);
    // the probe window of symbol k + 1 is read while symbol k is decoded (its address does not depend on the state);
    // a row without a window reads as INT_MAX: no entry <= cum, so the search over the whole row runs
    int ck_n = bcast_i(ci, 0);
    int wv_n = ck_n < win_rows ? s_win[ck_n * kWave + lane] : INT_MAX;
    for (int k = 0; k < cnt && d.st == 0; ++k) {
      const int ck = ck_n, wv = wv_n;
      const int size = bcast_i(size_l, k);
      if (k + 1 < cnt) {
        ck_n = bcast_i(ci, k + 1);
        wv_n = ck_n < win_rows ? s_win[ck_n * kWave + lane] : INT_MAX;
      }
      const int cum = (int)(d.x & 0xFFFFu);
      const int* __restrict__ row = cdfs + (size_t)ck * cdf_stride;
      int s = -1, start = 0, next = 0;
      const int cw = __popcll(__ballot(wv <= cum));  // wave-wide probe of the row's centre window
      if (cw >= 1 && cw < kWave) {
        s = win_start(size) + cw - 1;
        start = bcast_i(wv, cw - 1);
        next = bcast_i(wv, cw);
      } else {  // 64-way search over the whole row: s = last entry <= cum
        int lo = 0, len_r = size;
        bool ok = true;
        for (int lvl = 0; lvl < 6 && len_r > kWave && ok; ++lvl) {
          const int step = (len_r + kWave - 1) / kWave;
          const long long ent = (long long)lane * step;
          const int v = ent < len_r ? row[lo + ent] : INT_MAX;
          const int c1 = __popcll(__ballot(v <= cum));
          if (c1 == 0) {
            ok = false;
          } else {
            lo += (c1 - 1) * step;
            len_r = min(step, len_r - (c1 - 1) * step);
          }
        }
        if (ok && len_r <= kWave) {
          const int v = lane < len_r ? row[lo + lane] : INT_MAX;
          s = lo + __popcll(__ballot(v <= cum)) - 1;
        }
        if (s >= 0 && s <= size - 2) {
          start = row[s];
          next = row[s + 1];
        }
      }
      if (s < 0 || s > size - 2) {
        d.st = kStSymbol;
        break;
      }
      dec_advance(d, w, lane, cum, start, next);
      int value = s;
      if (s == size - 2 && d.st == 0) value = dec_escape(d, w, lane, size - 2);
      if (d.st) break;
      if (lane == k) myval = (int)((uint32_t)value + (uint32_t)off_l);
    }
    const int i = c * kWave + lane;
    if (i < n) {  // zeros from the failing symbol on
      const int j = i / seg_len, kk = i - j * seg_len;
      out[(seg0 + j) * out_ss + b * out_ts + kk] = myval;
    }
  }
  if (lane == 0) {
    state[b] = d.x;
    pos[b] = d.pos;
    status[b] = d.st;
  }
}

// ------------------------------------------------------------------------------------------------ lanes
// Lane-interleaved records: a stream's symbols are dealt round-robin over L = 2^lg sub-streams (sub-stream l codes
// the symbols k = l (mod L) of every segment, segments in order, k ascending), and every sub-stream is an ordinary
// stream of the format above.  One THREAD per sub-stream: thread t of a wave is lane l = t mod L of stream
// blockIdx.x * (64 / L) + t / L, so a wave holds 64 / L whole streams and lane l reads element step * L + l of a
// segment (coalesced).  State, slab tail / word cursor and escape handling are per-thread registers in plain
// divergent code; the loads are software-pipelined over the steps exactly as the kernels above pipeline chunks.
// A stream's status is the maximum over its lanes (a shuffle reduction, then one store by lane 0).
__device__ __forceinline__ int group_max(int v, int L) {
  for (int m = 1; m < L; m <<= 1) v = max(v, __shfl_xor(v, m, kWave));
  return v;
}

__global__ void __launch_bounds__(kWave)
rans_encode_lanes_kernel(const int* __restrict__ sym, long long sym_ss, long long sym_ts, const int* __restrict__ idx,
                         long long idx_ss, long long idx_ts, int nstreams, int nseg, int seg_len,
                         const int* __restrict__ cdfs, int cdf_stride, const int* __restrict__ sizes,
                         const int* __restrict__ offs, int ncdf, uint32_t* __restrict__ slabs, long long cap,
                         int* __restrict__ nwords, int* __restrict__ status, int lg) {
  const int L = 1 << lg, t = threadIdx.x;
  const int b = blockIdx.x * (kWave >> lg) + (t >> lg), l = t & (L - 1);
  const bool active = b < nstreams;
  const long long q = active ? (long long)b * L + l : 0;
  uint32_t* __restrict__ slab = slabs + (size_t)q * cap;
  const int* __restrict__ symb = sym + (active ? b * sym_ts : 0);
  const int* __restrict__ idxb = idx + (active ? b * idx_ts : 0);
  EncState e{kRansLow, cap, 0};
  const int nsteps = (seg_len + L - 1) >> lg;  // steps per segment; lane l has a symbol in step s if s * L + l < seg_len
  const int T = nseg * nsteps;
  // pipeline registers, one step per stage, steps in reverse (last segment, last step first).  Stage A: index and
  // symbol; B: the row's size and offset; C: clamp / escape and the two cdf entries; D: reciprocal, then the put.
  int aj = nseg - 1, as = nsteps - 1;
  int a_ci = 0, a_v = 0;
  bool a_ok = false;
  int b_ci = 0, b_v = 0, b_size = 3, b_off = 0;
  bool b_ok = false, b_bad = false;
  uint32_t c_start = 0, c_next = 1, c_raw = 0, c_flags = 0;  // flags: escaped | ndig << 1 | bad index << 8 | valid << 9
  for (int it = 0; it < T + 3; ++it) {
    // ---- D: fields of the symbol put in this iteration, from the cdf entries loaded one iteration ago
    const EncSymbol d = enc_symbol(c_start, c_next);
    const uint32_t d_raw = c_raw, d_flags = c_flags;
    // ---- C: clamp and escape the value, issue the loads of cdf[value] and cdf[value + 1]
    c_flags = 0;
    c_start = 0;
    c_next = 1;
    if (b_ok) {
      const EncValue v = enc_clamp_escape(b_v, b_off, b_size);
      const int* __restrict__ row = cdfs + (size_t)b_ci * cdf_stride;
      c_start = (uint32_t)row[v.value];
      c_next = (uint32_t)row[v.value + 1];
      c_raw = v.raw;
      c_flags = v.esc | (v.ndig << 1) | (b_bad ? 1u << 8 : 0u) | (1u << 9);
    }
    // ---- B: the row's size and offset (a bad index reads row 0 and is never put)
    b_ok = a_ok;
    if (a_ok) {
      b_bad = a_ci < 0 || a_ci >= ncdf;
      b_ci = b_bad ? 0 : a_ci;
      b_v = a_v;
      b_size = sizes[b_ci];
      b_off = offs[b_ci];
    }
    // ---- A: index and symbol
    a_ok = false;
    if (it < T) {
      const int k = (as << lg) + l;
      a_ok = active && k < seg_len;
      if (a_ok) {
        a_ci = idxb[aj * idx_ss + k];
        a_v = symb[aj * sym_ss + k];
      }
      if (--as < 0) {
        as = nsteps - 1;
        --aj;
      }
    }
    // ---- put
    if (!((d_flags >> 9) & 1u) || e.st) continue;
    if ((d_flags >> 8) & 1u) {
      e.st = kStIndex;
      continue;
    }
    if (d_flags & 1u) {
      const int ndig = (int)((d_flags >> 1) & 15u);
      for (int g = 7; g >= 0; --g)
        if (g < ndig) enc_put_bits(e, slab, true, (d_raw >> (4 * g)) & 15u);
      enc_put_bits(e, slab, true, (uint32_t)ndig);
      if (e.st) continue;
    }
    if (enc_must_emit(e.x, d.freq)) {
      enc_emit(e, slab, true);
      if (e.st) continue;
    }
    e.x = enc_put(e.x, d.freq, d.shift, d.rcp, d.bias);
  }
  if (active) enc_flush(e, slab, true);
  const int st = group_max(active ? e.st : 0, L);
  if (active) {
    nwords[q] = st ? 0 : (int)(cap - e.head);
    if (l == 0) status[b] = st;
  }
}

__global__ void __launch_bounds__(kWave)
rans_decode_lanes_kernel(const uint32_t* __restrict__ words, long long total_words, const long long* __restrict__ woff,
                         const int* __restrict__ wlen, const int* __restrict__ idx, long long idx_ss, long long idx_ts,
                         int* __restrict__ out, long long out_ss, long long out_ts, int nstreams, int seg0, int nseg,
                         int seg_len, const int* __restrict__ cdfs, int cdf_stride, const int* __restrict__ sizes,
                         const int* __restrict__ offs, int ncdf, int win_rows, unsigned long long* __restrict__ state,
                         int* __restrict__ pos, int* __restrict__ status, int first, int lg) {
  extern __shared__ int s_win[];  // [win_rows][64]: entries win_start(size) + i of each row, INT_MAX past its end
  const int L = 1 << lg, t = threadIdx.x;
  dec_fill_windows(s_win, win_rows, cdfs, cdf_stride, sizes, t);

  const int b = blockIdx.x * (kWave >> lg) + (t >> lg), l = t & (L - 1);
  const bool active = b < nstreams;
  const long long q = active ? (long long)b * L + l : 0;
  LaneDec d{0, 0, 0, 0u, 0};
  const uint32_t* __restrict__ w = words;
  if (active) {
    d.st = first ? 0 : status[b];
    d.len = wlen[q];
    w = dec_open(d, words, total_words, woff[q], first, state[q], pos[q]);
    if (d.st == 0) d.nextw = d.pos < d.len ? w[d.pos] : 0u;
  }
  const int* __restrict__ idxb = idx + (active ? b * idx_ts : 0);
  int* __restrict__ outb = out + (active ? b * out_ts : 0);

  const int nsteps = (seg_len + L - 1) >> lg;
  const int T = nseg * nsteps;
  // pipeline registers.  Stage A: the index of a step; B: its row's size and offset; then the step itself.
  int aj = 0, as = 0;
  int a_ci = 0;
  long long a_o = 0;
  bool a_ok = false;
  int b_ci = 0, b_size = 3, b_off = 0;
  long long b_o = 0;
  bool b_ok = false, b_bad = false;
  for (int it = 0; it < T + 2; ++it) {
    const int ci = b_ci, size = b_size, off_l = b_off;
    const long long o = b_o;
    const bool ok = b_ok, bad = b_bad;
    b_ok = a_ok;
    if (a_ok) {
      b_bad = a_ci < 0 || a_ci >= ncdf;
      b_ci = b_bad ? 0 : a_ci;
      b_o = a_o;
      b_size = sizes[b_ci];
      b_off = offs[b_ci];
    }
    a_ok = false;
    if (it < T) {
      const int k = (as << lg) + l;
      a_ok = active && k < seg_len;
      if (a_ok) {
        a_ci = idxb[(seg0 + aj) * idx_ss + k];
        a_o = (seg0 + aj) * out_ss + k;
      }
      if (++as == nsteps) {
        as = 0;
        ++aj;
      }
    }
    if (!ok) continue;
    // ---- one symbol of this lane's sub-stream (zeros from the failing symbol on)
    int outv = 0;
    if (d.st == 0 && bad) d.st = kStIndex;
    if (d.st == 0) {
      const int cum = (int)(d.x & 0xFFFFu);
      int s = -1, start = 0, next = 0;
      bool found = false;
      if (ci < win_rows) {  // 6-step binary search of the row's centre window: cnt = entries <= cum of its first 63
        const int* win = s_win + ci * kWave;
        const int last = win[kWave - 1];
        int cnt = 0;
#pragma unroll
        for (int h = kWave / 2; h > 0; h >>= 1)
          if (win[cnt + h - 1] <= cum) cnt += h;
        if (cnt >= 1 && last > cum) {
          s = win_start(size) + cnt - 1;
          start = win[cnt - 1];
          next = win[cnt];
          found = true;
        }
      }
      if (!found) {  // binary search over the whole row: 12 halvings cover 4096 entries
        const int* __restrict__ row = cdfs + (size_t)ci * cdf_stride;
        int lo = 0, n = size;
        for (int i = 0; i < 12; ++i) {
          if (n > 1) {
            const int half = n >> 1;
            if (row[lo + half] <= cum) {
              lo += half;
              n -= half;
            } else {
              n = half;
            }
          }
        }
        if (n == 1 && lo <= size - 2) {
          start = row[lo];
          next = row[lo + 1];
          if (start <= cum && cum < next) s = lo;
        }
      }
      if (s < 0 || s > size - 2) {
        d.st = kStSymbol;
      } else {
        dec_advance(d, w, t, cum, start, next);
        int value = s;
        if (s == size - 2 && d.st == 0) value = dec_escape(d, w, t, size - 2);
        if (d.st == 0) outv = (int)((uint32_t)value + (uint32_t)off_l);
      }
    }
    outb[o] = outv;
  }
  const int st = group_max(active ? d.st : 0, L);
  if (active) {
    state[q] = d.x;
    pos[q] = d.pos;
    if (l == 0) status[b] = st;
  }
}

}  // namespace

// words that always hold a stream of n symbols.  With the state at or above 2^31 (2^27 for a bypass digit, after a
// word store) a put multiplies it by at most 2^16 (1 + 2^-15) (symbol) or 2^4 (1 + 2^-27) (bypass digit), a word
// store divides it by at least 2^32, and it starts at 2^31 and ends at or above 2^31: 32 W <= n (16 + 9 * 4 + 4.5e-5)
// bits.  The excess over 52 n / 32 is below n / 2^19 words; + 2 words of state flush, + 1 spare.
extern "C" long long tmae_rans_stream_cap_words(long long nsymbols) {
  if (nsymbols < 0) return -1;
  return (52 * nsymbols + 31) / 32 + (nsymbols >> 19) + 3;
}

// log2 of a lane count that is a power of two in 1..64, -1 otherwise
static int lanes_log2(int lanes) {
  for (int lg = 0; lg <= 6; ++lg)
    if (lanes == 1 << lg) return lg;
  return -1;
}

// what the encode and the decode entry points require alike; `name` is the entry point, for the message
static int check_common(const char* name, bool buffers, int nstreams, int nseg, int seg_len, const void* cdfs,
                        int cdf_stride, const void* cdf_sizes, const void* offsets, int ncdf, int lanes, int* lg) {
  TMAE_REQUIRE(buffers, "%s: NULL buffer", name);
  TMAE_REQUIRE(nstreams > 0, "%s: nstreams = %d must be positive", name, nstreams);
  TMAE_REQUIRE(nseg > 0 && seg_len > 0 && (long long)nseg * seg_len <= (1ll << 30),
               "%s: nseg * seg_len = %d * %d must be in [1, 2^30]", name, nseg, seg_len);
  TMAE_REQUIRE(cdfs && cdf_sizes && offsets && ncdf > 0 && cdf_stride > 1, "%s: CDF tables required", name);
  *lg = lanes_log2(lanes);
  TMAE_REQUIRE(*lg >= 0, "%s: lanes = %d must be a power of two in 1..64", name, lanes);
  TMAE_REQUIRE((long long)nstreams * lanes <= INT32_MAX, "%s: nstreams * lanes = %d * %d overflows int32", name,
               nstreams, lanes);
  return TMAE_OK;
}

// lanes = 1 with the wave-per-stream kernel (by_wave) is tmae_rans_encode_streams, else tmae_rans_encode_lanes
static int encode_entry(const char* name, bool by_wave, const int32_t* symbols, long long sym_seg_stride,
                        long long sym_stream_stride, const int32_t* indexes, long long idx_seg_stride,
                        long long idx_stream_stride, int nstreams, int nseg, int seg_len, const int32_t* cdfs,
                        int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int ncdf, uint32_t* slabs,
                        long long cap_words, int32_t* nwords, int32_t* status, int lanes, void* stream) {
  int lg = 0;
  if (int rc = check_common(name, symbols && indexes && slabs && nwords && status, nstreams, nseg, seg_len, cdfs,
                            cdf_stride, cdf_sizes, offsets, ncdf, lanes, &lg))
    return rc;
  TMAE_REQUIRE(cap_words > 0 && cap_words <= INT32_MAX, "%s: cap_words = %lld outside [1, 2^31)", name, cap_words);
  TMAE_REQUIRE(sym_seg_stride >= 0 && sym_stream_stride >= 0 && idx_seg_stride >= 0 && idx_stream_stride >= 0,
               "%s: negative stride", name);
  if (by_wave) {
    hipLaunchKernelGGL(rans_encode_streams_kernel, dim3(nstreams), dim3(kWave), 0, (hipStream_t)stream, symbols,
                       sym_seg_stride, sym_stream_stride, indexes, idx_seg_stride, idx_stream_stride, nseg, seg_len,
                       cdfs, cdf_stride, cdf_sizes, offsets, ncdf, slabs, cap_words, nwords, status);
  } else {
    const int per_wave = kWave >> lg;
    hipLaunchKernelGGL(rans_encode_lanes_kernel, dim3((nstreams + per_wave - 1) / per_wave), dim3(kWave), 0,
                       (hipStream_t)stream, symbols, sym_seg_stride, sym_stream_stride, indexes, idx_seg_stride,
                       idx_stream_stride, nstreams, nseg, seg_len, cdfs, cdf_stride, cdf_sizes, offsets, ncdf, slabs,
                       cap_words, nwords, status, lg);
  }
  TMAE_LAUNCH_CHECK(name);
}

static int decode_entry(const char* name, bool by_wave, const uint32_t* words, long long total_words,
                        const long long* word_offsets, const int32_t* word_counts, const int32_t* indexes,
                        long long idx_seg_stride, long long idx_stream_stride, int32_t* symbols,
                        long long sym_seg_stride, long long sym_stream_stride, int nstreams, int seg0, int nseg,
                        int seg_len, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                        const int32_t* offsets, int ncdf, unsigned long long* state, int32_t* pos, int32_t* status,
                        int first, int lanes, void* stream) {
  int lg = 0;
  if (int rc = check_common(name, words && word_offsets && word_counts && indexes && symbols && state && pos && status,
                            nstreams, nseg, seg_len, cdfs, cdf_stride, cdf_sizes, offsets, ncdf, lanes, &lg))
    return rc;
  TMAE_REQUIRE(total_words > 0 && seg0 >= 0, "%s: total_words = %lld, seg0 = %d", name, total_words, seg0);
  TMAE_REQUIRE(sym_seg_stride >= 0 && sym_stream_stride >= 0 && idx_seg_stride >= 0 && idx_stream_stride >= 0,
               "%s: negative stride", name);
  const int win_rows = ncdf < kMaxWinRows ? ncdf : kMaxWinRows;
  const size_t lds = (size_t)win_rows * kWave * sizeof(int);
  if (by_wave) {
    hipLaunchKernelGGL(rans_decode_streams_kernel, dim3(nstreams), dim3(kWave), lds, (hipStream_t)stream, words,
                       total_words, word_offsets, word_counts, indexes, idx_seg_stride, idx_stream_stride, symbols,
                       sym_seg_stride, sym_stream_stride, seg0, nseg, seg_len, cdfs, cdf_stride, cdf_sizes, offsets,
                       ncdf, win_rows, state, pos, status, first ? 1 : 0);
  } else {
    const int per_wave = kWave >> lg;
    hipLaunchKernelGGL(rans_decode_lanes_kernel, dim3((nstreams + per_wave - 1) / per_wave), dim3(kWave), lds,
                       (hipStream_t)stream, words, total_words, word_offsets, word_counts, indexes, idx_seg_stride,
                       idx_stream_stride, symbols, sym_seg_stride, sym_stream_stride, nstreams, seg0, nseg, seg_len,
                       cdfs, cdf_stride, cdf_sizes, offsets, ncdf, win_rows, state, pos, status, first ? 1 : 0, lg);
  }
  TMAE_LAUNCH_CHECK(name);
}

extern "C" int tmae_rans_encode_streams(const int32_t* symbols, long long sym_seg_stride, long long sym_stream_stride,
                                        const int32_t* indexes, long long idx_seg_stride, long long idx_stream_stride,
                                        int nstreams, int nseg, int seg_len, const int32_t* cdfs, int cdf_stride,
                                        const int32_t* cdf_sizes, const int32_t* offsets, int ncdf, uint32_t* slabs,
                                        long long cap_words, int32_t* nwords, int32_t* status, void* stream) {
  return encode_entry("tmae_rans_encode_streams", true, symbols, sym_seg_stride, sym_stream_stride, indexes,
                      idx_seg_stride, idx_stream_stride, nstreams, nseg, seg_len, cdfs, cdf_stride, cdf_sizes, offsets,
                      ncdf, slabs, cap_words, nwords, status, 1, stream);
}

extern "C" int tmae_rans_encode_lanes(const int32_t* symbols, long long sym_seg_stride, long long sym_stream_stride,
                                      const int32_t* indexes, long long idx_seg_stride, long long idx_stream_stride,
                                      int nstreams, int nseg, int seg_len, const int32_t* cdfs, int cdf_stride,
                                      const int32_t* cdf_sizes, const int32_t* offsets, int ncdf, uint32_t* slabs,
                                      long long cap_words, int32_t* nwords, int32_t* status, int lanes, void* stream) {
  return encode_entry("tmae_rans_encode_lanes", false, symbols, sym_seg_stride, sym_stream_stride, indexes,
                      idx_seg_stride, idx_stream_stride, nstreams, nseg, seg_len, cdfs, cdf_stride, cdf_sizes, offsets,
                      ncdf, slabs, cap_words, nwords, status, lanes, stream);
}

extern "C" int tmae_rans_pack_streams(const uint32_t* slabs, long long cap_words, const int32_t* nwords, int nstreams,
                                      uint32_t* dense, long long dense_cap_words, long long* word_offsets,
                                      int32_t* status, void* stream) {
  TMAE_REQUIRE(slabs && nwords && dense && word_offsets && status, "tmae_rans_pack_streams: NULL buffer");
  TMAE_REQUIRE(nstreams > 0, "tmae_rans_pack_streams: nstreams = %d must be positive", nstreams);
  TMAE_REQUIRE(cap_words > 0 && dense_cap_words > 0, "tmae_rans_pack_streams: capacities must be positive");
  hipLaunchKernelGGL(rans_pack_streams_kernel, dim3(nstreams), dim3(256), 0, (hipStream_t)stream, slabs, cap_words,
                     nwords, nstreams, dense, dense_cap_words, word_offsets, status);
  TMAE_LAUNCH_CHECK("tmae_rans_pack_streams");
}

extern "C" int tmae_rans_decode_streams(const uint32_t* words, long long total_words, const long long* word_offsets,
                                        const int32_t* word_counts, const int32_t* indexes, long long idx_seg_stride,
                                        long long idx_stream_stride, int32_t* symbols, long long sym_seg_stride,
                                        long long sym_stream_stride, int nstreams, int seg0, int nseg, int seg_len,
                                        const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                                        const int32_t* offsets, int ncdf, unsigned long long* state, int32_t* pos,
                                        int32_t* status, int first, void* stream) {
  return decode_entry("tmae_rans_decode_streams", true, words, total_words, word_offsets, word_counts, indexes,
                      idx_seg_stride, idx_stream_stride, symbols, sym_seg_stride, sym_stream_stride, nstreams, seg0, nseg,
                      seg_len, cdfs, cdf_stride, cdf_sizes, offsets, ncdf, state, pos, status, first, 1, stream);
}

extern "C" int tmae_rans_decode_lanes(const uint32_t* words, long long total_words, const long long* word_offsets,
                                      const int32_t* word_counts, const int32_t* indexes, long long idx_seg_stride,
                                      long long idx_stream_stride, int32_t* symbols, long long sym_seg_stride,
                                      long long sym_stream_stride, int nstreams, int seg0, int nseg, int seg_len,
                                      const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                                      const int32_t* offsets, int ncdf, unsigned long long* state, int32_t* pos,
                                      int32_t* status, int first, int lanes, void* stream) {
  return decode_entry("tmae_rans_decode_lanes", false, words, total_words, word_offsets, word_counts, indexes,
                      idx_seg_stride, idx_stream_stride, symbols, sym_seg_stride, sym_stream_stride, nstreams, seg0, nseg,
                      seg_len, cdfs, cdf_stride, cdf_sizes, offsets, ncdf, state, pos, status, first, lanes, stream);
}
