// Streamed multi-head attention (timm Attention, MCM.py:629-630, 678-679) for the sequence lengths the
// LDS-resident kernels of attention.hip refuse: a 384- or 512-pixel model's decoder runs at T = 577 or 1025.
//
// Nothing of a head is held whole.  A workgroup owns a block of queries (forward, backward dQ) or of keys
// (backward dK / dV) of one (image, head) and walks the other axis in chunks staged in LDS; the running softmax
// state or the gradient accumulators stay in registers across chunks.  The per-tile math is the math of the
// resident kernels (S^T = K Q^T with the query on the lane, the score accumulator fed back as the next MFMA
// operand), so both families agree to rounding and a forward of either feeds a backward of either: lse is the
// same base-2 [b][h][t] array.
//
// Workgroup ids go through xcd_remap: the blocks of one (image, head) get consecutive logical ids, which one XCD
// runs, so its L2 fetches that head's K / V (or Q / dO) once for all of them.
#include "attn_stream.h"

#include "attn_core.h"

namespace {

// ------------------------------------------------------------------------------------------------ sizes
// Forward: 8 waves = 256 queries per workgroup, chunks of 128 (bf16) / 64 (f32) keys.  LDS per workgroup:
//   bf16 dh 32 / 64 (K [C][DH + 8], V [C][LDV] for ds_read_b64_tr_b16)   18 / 42 KB
//   bf16 dh 80      (K [C][DH + 8], V^T [96][C + 4])                     47 KB
//   f32             (K [C][DH + 4], V^T [DHP][C + 1])                    17 / 33 / 46 KB
// all below 80 KB (two workgroups per CU) and below the 64 KB of a static allocation.
template <typename T, int DH> struct StreamFwd {
  static constexpr bool BF = sizeof(T) == 2;
  static constexpr bool LEAN = BF && DH % 32 == 0;  // row-major V and transposed reads
  static constexpr int NW = 8, QB = 32 * NW, NTHR = 64 * NW;
  static constexpr int C = BF ? 128 : 64;
  static constexpr int DHP = (DH + 31) / 32 * 32;
  static constexpr int LDK = DH + (BF ? 8 : 4);
  static constexpr int LDV = LEAN ? AttnTr<DH>::LDV : C + (BF ? 4 : 1);
  static constexpr int VROWS = LEAN ? C : DHP;
};

// Backward: 4 waves = 128 keys (dK / dV kernel) or 128 queries (dQ kernel) per workgroup, the same chunk
// lengths.  Staged rows are [C][LD], LD = the resident backward's stride for bf16 (48 / 16 dwords: conflict-free
// transposed reads; dh 80 padded to 96 columns of which 80..95 are zeros) and DHP + 4 floats for f32.
template <typename T, int DH> struct StreamBwd {
  static constexpr bool BF = sizeof(T) == 2;
  static constexpr int NW = 4, RB = 32 * NW, NTHR = 64 * NW;
  static constexpr int C = BF ? 128 : 64;
  static constexpr int DHP = (DH + 31) / 32 * 32, NDT = DHP / 32;
  static constexpr int LD = BF ? (DH == 32 ? 32 : 96) : DHP + 4;
};

// B (or A) operand of a 32x32x16 MFMA whose k runs over 16 ROWS of a row-major LDS array (rows k0.., columns
// c0..c0+31 on the lanes): two transposed 4-row reads in the accumulator layout's element order
// (k = (j & 3) + 8 (j >> 2) + 4 hh).  The form attention.hip uses; EXEC must be all ones.
template <int LD>
__device__ __forceinline__ bf16x8 stream_tr_frag(const bf16* arr, int k0, int c0, int lane) {
  const int g = lane >> 4, gi = lane & 15, qq = gi >> 2, pp = gi & 3;
  const int trow = 4 * (g >> 1) + qq, tcol = 16 * (g & 1) + 4 * pp;
  const bf16* p = arr + (size_t)(k0 + trow) * LD + c0 + tcol;
  const attn_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((attn_lds_s4*)p);
  const attn_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((attn_lds_s4*)(p + 8 * LD));
  typedef __attribute__((ext_vector_type(8))) short s8;
  s8 v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return *reinterpret_cast<bf16x8*>(&v);
}

// rowsum(dO * O) of one row (DH values), the order of the resident kernels: ascending head-dim index
template <typename T, int DH>
__device__ __forceinline__ float stream_delta(const T* orow, const T* grow) {
  float d = 0.0f;
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int c = 0; c < DH / 8; ++c) {
      const bf16x8 ov = *reinterpret_cast<const bf16x8*>(orow + 8 * c);
      const bf16x8 gv = *reinterpret_cast<const bf16x8*>(grow + 8 * c);
#pragma unroll
      for (int e = 0; e < 8; ++e) d += (float)ov[e] * (float)gv[e];
    }
  } else {
#pragma unroll
    for (int c = 0; c < DH / 4; ++c) {
      const f32x4 ov = *reinterpret_cast<const f32x4*>(orow + 4 * c);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(grow + 4 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) d += ov[e] * gv[e];
    }
  }
  return d;
}

// rows r0 .. r0 + C - 1 of two head slices -> A0 / A1 (row-major, stride LD, 16-B chunks); rows at or past Tn
// and the columns DH..DHP-1 that pad the head dim to whole 32-wide tiles are zeros
template <typename T, int DH, int LD, int C, int NTHR>
__device__ __forceinline__ void stream_stage2(T* A0, const T* g0, int ld0, T* A1, const T* g1, int ld1, int r0, int Tn,
                                              int tid) {
  constexpr int EPC = 16 / sizeof(T), CPR = (DH + 31) / 32 * 32 / EPC;
  for (int i = tid; i < C * CPR; i += NTHR) {
    const int r = i / CPR, c = i - r * CPR;
    uint4 x = uint4{0, 0, 0, 0}, y = x;
    if (r0 + r < Tn && EPC * c < DH) {
      x = *reinterpret_cast<const uint4*>(g0 + (size_t)(r0 + r) * ld0 + c * EPC);
      y = *reinterpret_cast<const uint4*>(g1 + (size_t)(r0 + r) * ld1 + c * EPC);
    }
    *reinterpret_cast<uint4*>(A0 + (size_t)r * LD + c * EPC) = x;
    *reinterpret_cast<uint4*>(A1 + (size_t)r * LD + c * EPC) = y;
  }
}

}  // namespace

// ================================================================================================= forward
// One workgroup: one (image, head), 256 queries (32 per wave, Q fragments in registers).  The keys arrive in
// chunks of C: every thread loads its 16-B pieces of chunk i + 1 into registers before the tiles of chunk i are
// computed and writes them to LDS after (the split load / write staging: the HBM latency runs under the MFMAs
// of the chunk before; one LDS buffer, two barriers per chunk).  Online softmax per 32-key tile with the running
// max m, the row sum l and O^T in registers; every tile rescales O and l by exp2(m_old - m_new), which is 1 when
// the max did not move, so a chunk boundary is no special case.  Only a tile that reaches past Tn (the last one)
// carries the ragged mask: its rows are zeros in LDS and their scores -inf.  Tiles wholly past Tn are skipped.
template <typename T, int DH>
__global__ void __launch_bounds__(512)
mha_fwd_stream_kernel(const T* __restrict__ qkv, T* __restrict__ out, float* __restrict__ lse, int Tn, int H, int nqb,
                      float scale_log2e) {
  using Cfg = StreamFwd<T, DH>;
  constexpr bool BF = Cfg::BF, LEAN = Cfg::LEAN;
  constexpr int C = Cfg::C, NTHR = Cfg::NTHR, DHP = Cfg::DHP, NDT = DHP / 32;
  constexpr int LDK = Cfg::LDK, LDV = Cfg::LDV;
  constexpr int EPC = 16 / sizeof(T), CPR = DH / EPC;  // 16-B pieces per row
  constexpr int NIT = (C * CPR + NTHR - 1) / NTHR;     // pieces per thread and operand
  static_assert(DH % 16 == 0, "head dim must be a multiple of 16");
  __shared__ __attribute__((aligned(16))) T Ks[C * LDK];
  __shared__ __attribute__((aligned(16))) T Vs[Cfg::VROWS * LDV];

  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = id / nqb, qblk = id - bh * nqb, b = bh / H, h = bh - b * H;
  const int D = H * DH, ld = 3 * D;
  const T* base = qkv + (size_t)b * Tn * ld + h * DH;
  const int tid = threadIdx.x;

  uint4 kreg[NIT], vreg[NIT];
  auto load_chunk = [&](int c0) {
#pragma unroll
    for (int u = 0; u < NIT; ++u) {
      const int i = tid + u * NTHR, r = i / CPR, c = i - r * CPR;
      kreg[u] = vreg[u] = uint4{0, 0, 0, 0};
      if (i < C * CPR && c0 + r < Tn) {
        kreg[u] = *reinterpret_cast<const uint4*>(base + (size_t)(c0 + r) * ld + D + c * EPC);
        vreg[u] = *reinterpret_cast<const uint4*>(base + (size_t)(c0 + r) * ld + 2 * D + c * EPC);
      }
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int u = 0; u < NIT; ++u) {
      const int i = tid + u * NTHR, r = i / CPR, c = i - r * CPR;
      if (i < C * CPR) {
        *reinterpret_cast<uint4*>(Ks + (size_t)r * LDK + c * EPC) = kreg[u];
        if constexpr (LEAN) {
          *reinterpret_cast<uint4*>(Vs + (size_t)r * LDV + c * EPC) = vreg[u];
        } else {
          const T* ve = reinterpret_cast<const T*>(&vreg[u]);
#pragma unroll
          for (int e = 0; e < EPC; ++e) Vs[(size_t)(c * EPC + e) * LDV + r] = ve[e];
        }
      }
    }
  };
  // a head dim that is no multiple of 32 (80): rows DH..DHP-1 of V^T are zeros, written once
  if constexpr (!LEAN && DHP != DH)
    for (int i = tid; i < (DHP - DH) * LDV; i += NTHR) Vs[(size_t)DH * LDV + i] = (T)0.0f;

  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int q0 = qblk * Cfg::QB + wave * 32;
  const bool active = q0 < Tn;  // wave-uniform: EXEC stays all ones inside
  const int q = q0 + col;
  const T* qrow = base + (size_t)(q < Tn ? q : Tn - 1) * ld;

  bf16x8 qb[BF ? DH / 16 : 1];
  float qf[BF ? 1 : DH / 2];
  if constexpr (BF) {
#pragma unroll
    for (int s = 0; s < DH / 16; ++s) qb[s] = *reinterpret_cast<const bf16x8*>(qrow + 16 * s + 8 * hh);
  } else {
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) qf[s] = qrow[2 * s + hh];
  }

  f32x16 O[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) O[dt][r] = 0.0f;
  float m_run = -INFINITY, l_run = 0.0f;

  const int nch = (Tn + C - 1) / C;
  load_chunk(0);
  for (int ci = 0; ci < nch; ++ci) {
    const int c0 = ci * C;
    __syncthreads();  // every wave is done with the chunk before
    store_chunk();
    __syncthreads();
    if (ci + 1 < nch) load_chunk(c0 + C);
    if (!active) continue;
    const int ntl = min(C / 32, (Tn - c0 + 31) / 32);
    for (int kt = 0; kt < ntl; ++kt) {
      const int kg = c0 + 32 * kt;        // first key of the tile
      const bool ragged = kg + 32 > Tn;   // wave-uniform
      f32x16 S;
#pragma unroll
      for (int r = 0; r < 16; ++r) S[r] = 0.0f;
      if constexpr (BF) {
        const T* krow = Ks + (size_t)(32 * kt + col) * LDK + 8 * hh;
#pragma unroll
        for (int s = 0; s < DH / 16; ++s) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(krow + 16 * s);
          S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qb[s], S, 0, 0, 0);
        }
      } else {
        const T* krow = Ks + (size_t)(32 * kt + col) * LDK + hh;
#pragma unroll
        for (int s = 0; s < DH / 2; ++s) S = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[2 * s], qf[s], S, 0, 0, 0);
      }
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kg + (r & 3) + 8 * (r >> 2) + 4 * hh;
        S[r] = (!ragged || key < Tn) ? S[r] * scale_log2e : -INFINITY;
        tmax = fmaxf(tmax, S[r]);
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
      const float m_new = fmaxf(m_run, tmax);  // finite: a tile that is computed holds a key below Tn
      const float alpha = exp2f(m_run - m_new);
      float ps = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        S[r] = exp2f(S[r] - m_new);
        ps += S[r];
      }
      ps += __shfl_xor(ps, 32);
      l_run = l_run * alpha + ps;
      m_run = m_new;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) O[dt] *= alpha;
      if constexpr (BF) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8 pb;
#pragma unroll
          for (int j = 0; j < 8; ++j) pb[j] = (bf16)S[8 * s + j];
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            bf16x8 a;
            if constexpr (LEAN) {
              a = stream_tr_frag<LDV>(Vs, 32 * kt + 16 * s, 32 * dt, lane);
            } else {
              const T* vrow = Vs + (size_t)(32 * dt + col) * LDV + 32 * kt + 16 * s + 4 * hh;
              const bf16x4 v0 = *reinterpret_cast<const bf16x4*>(vrow);
              const bf16x4 v1 = *reinterpret_cast<const bf16x4*>(vrow + 8);
              a[0] = v0[0]; a[1] = v0[1]; a[2] = v0[2]; a[3] = v0[3];
              a[4] = v1[0]; a[5] = v1[1]; a[6] = v1[2]; a[7] = v1[3];
            }
            O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pb, O[dt], 0, 0, 0);
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kl = 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * hh;
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            const float a = Vs[(size_t)(32 * dt + col) * LDV + kl];
            O[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, S[r], O[dt], 0, 0, 0);
          }
        }
      }
    }
  }

  if (!active || q >= Tn) return;
  if (lse && hh == 0) lse[(size_t)bh * Tn + q] = m_run + log2f(l_run);  // base-2 log-sum-exp of the scaled scores
  const float inv_l = 1.0f / l_run;
  T* orow = out + ((size_t)b * Tn + q) * D + h * DH;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * dt + 8 * g + 4 * hh;
      if (DHP != DH && d >= DH) continue;
      f32x4 v{O[dt][4 * g] * inv_l, O[dt][4 * g + 1] * inv_l, O[dt][4 * g + 2] * inv_l, O[dt][4 * g + 3] * inv_l};
      store4(orow + d, v);
    }
}

// ================================================================================================ backward
// The two phases of the resident two-phase backward as two kernels, each owning its outputs: no atomics, every
// element of dqkv written once, a fixed summation order (chunks, then tiles, ascending), bitwise reproducible.
// P is recomputed from Q, K and the forward's base-2 lse; delta = rowsum(dO * O) is recomputed from o and dout
// (while a chunk is staged in the dK / dV kernel, per lane in the dQ kernel), so no workspace is needed.
//
// dK / dV: a wave holds 32 keys (K, V fragments and dK, dV accumulators in registers) and walks the queries in
// chunks of Q, dO, lse and delta staged in LDS.  S = Q K^T and dP = dO V^T with the key on the lane, so P and
// dS = P (dP - delta) are already the A operands of dV += P^T dO and dK += scale dS^T Q.
template <typename T, int DH>
__global__ void __launch_bounds__(256)
mha_bwd_stream_dkv_kernel(const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ dout,
                          const float* __restrict__ lse, T* __restrict__ dqkv, int Tn, int H, int nkb, float scale) {
  using Cfg = StreamBwd<T, DH>;
  constexpr bool BF = Cfg::BF;
  constexpr int C = Cfg::C, NTHR = Cfg::NTHR, LD = Cfg::LD, NDT = Cfg::NDT;
  static_assert(DH % 16 == 0, "head dim must be a multiple of 16");
  __shared__ __attribute__((aligned(16))) T A0[C * LD];  // Q
  __shared__ __attribute__((aligned(16))) T A1[C * LD];  // dO
  __shared__ __attribute__((aligned(16))) float lse_s[C];
  __shared__ __attribute__((aligned(16))) float dl_s[C];

  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = id / nkb, kblk = id - bh * nkb, b = bh / H, h = bh - b * H;
  const int D = H * DH, ld = 3 * D;
  const T* base = qkv + (size_t)b * Tn * ld + h * DH;
  const T* obase = o + (size_t)b * Tn * D + h * DH;
  const T* gbase = dout + (size_t)b * Tn * D + h * DH;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const float c2 = scale * 1.4426950408889634f;

  const int kb = kblk * Cfg::RB + 32 * wave;
  const bool active = kb < Tn;  // wave-uniform
  const bool kok = kb + col < Tn;
  const int kr = min(kb + col, Tn - 1);
  bf16x8 kfb[BF ? DH / 16 : 1], vfb[BF ? DH / 16 : 1];
  float kff[BF ? 1 : DH / 2], vff[BF ? 1 : DH / 2];
  if constexpr (BF) {
#pragma unroll
    for (int s = 0; s < DH / 16; ++s) {
      kfb[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)kr * ld + D + 16 * s + 8 * hh);
      vfb[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)kr * ld + 2 * D + 16 * s + 8 * hh);
    }
  } else {
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) {
      kff[s] = kok ? base[(size_t)kr * ld + D + 2 * s + hh] : 0.0f;
      vff[s] = kok ? base[(size_t)kr * ld + 2 * D + 2 * s + hh] : 0.0f;
    }
  }
  f32x16 dV[NDT], dK[NDT];
#pragma unroll
  for (int t = 0; t < NDT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dV[t][r] = dK[t][r] = 0.0f;

  const int nch = (Tn + C - 1) / C;
  for (int ci = 0; ci < nch; ++ci) {
    const int c0 = ci * C;
    __syncthreads();  // every wave is done with the chunk before
    stream_stage2<T, DH, LD, C, NTHR>(A0, base, ld, A1, gbase, D, c0, Tn, tid);
    for (int r = tid; r < C; r += NTHR) {
      float d = 0.0f, l = 0.0f;
      if (c0 + r < Tn) {
        d = stream_delta<T, DH>(obase + (size_t)(c0 + r) * D, gbase + (size_t)(c0 + r) * D);
        l = lse[(size_t)bh * Tn + c0 + r];
      }
      dl_s[r] = d;
      lse_s[r] = l;
    }
    __syncthreads();
    if (!active) continue;
    const int ntl = min(C / 32, (Tn - c0 + 31) / 32);
    for (int qt = 0; qt < ntl; ++qt) {
      f32x16 S, G;
#pragma unroll
      for (int r = 0; r < 16; ++r) S[r] = G[r] = 0.0f;
      if constexpr (BF) {
#pragma unroll
        for (int s = 0; s < DH / 16; ++s) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(A0 + (size_t)(qt * 32 + col) * LD + 16 * s + 8 * hh);
          S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, kfb[s], S, 0, 0, 0);
          const bf16x8 g = *reinterpret_cast<const bf16x8*>(A1 + (size_t)(qt * 32 + col) * LD + 16 * s + 8 * hh);
          G = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g, vfb[s], G, 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int s = 0; s < DH / 2; ++s) {
          S = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[(size_t)(qt * 32 + col) * LD + 2 * s + hh], kff[s], S, 0, 0, 0);
          G = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[(size_t)(qt * 32 + col) * LD + 2 * s + hh], vff[s], G, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ql = qt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        const float p = (kok && c0 + ql < Tn) ? exp2f(S[r] * c2 - lse_s[ql]) : 0.0f;
        S[r] = p;
        G[r] = p * (G[r] - dl_s[ql]) * scale;
      }
      if constexpr (BF) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8 pa, da;
#pragma unroll
          for (int j = 0; j < 8; ++j) { pa[j] = (bf16)S[8 * s + j]; da[j] = (bf16)G[8 * s + j]; }
          const int k0 = qt * 32 + 16 * s;
#pragma unroll
          for (int t = 0; t < NDT; ++t) {
            const bf16x8 gt = stream_tr_frag<LD>(A1, k0, 32 * t, lane), qt2 = stream_tr_frag<LD>(A0, k0, 32 * t, lane);
            dV[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, gt, dV[t], 0, 0, 0);
            dK[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, qt2, dK[t], 0, 0, 0);
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql = qt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
#pragma unroll
          for (int t = 0; t < NDT; ++t) {
            dV[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(S[r], A1[(size_t)ql * LD + 32 * t + col], dV[t], 0, 0, 0);
            dK[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(G[r], A0[(size_t)ql * LD + 32 * t + col], dK[t], 0, 0, 0);
          }
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int t = 0; t < NDT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kb + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (key < Tn && 32 * t + col < DH) {
        T* row = dqkv + ((size_t)b * Tn + key) * ld + h * DH + 32 * t + col;
        row[D] = to_out<T>(dK[t][r]);
        row[2 * D] = to_out<T>(dV[t][r]);
      }
    }
}

// dQ: a wave holds 32 queries (Q, dO fragments, lse, delta and the dQ accumulators in registers) and walks the
// keys in chunks of K and V staged in LDS.  S^T and dP^T with the query on the lane, so dS^T is already the A
// operand of dQ += scale dS K.
template <typename T, int DH>
__global__ void __launch_bounds__(256)
mha_bwd_stream_dq_kernel(const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ dout,
                         const float* __restrict__ lse, T* __restrict__ dqkv, int Tn, int H, int nqb, float scale) {
  using Cfg = StreamBwd<T, DH>;
  constexpr bool BF = Cfg::BF;
  constexpr int C = Cfg::C, NTHR = Cfg::NTHR, LD = Cfg::LD, NDT = Cfg::NDT;
  __shared__ __attribute__((aligned(16))) T A0[C * LD];  // K
  __shared__ __attribute__((aligned(16))) T A1[C * LD];  // V

  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = id / nqb, qblk = id - bh * nqb, b = bh / H, h = bh - b * H;
  const int D = H * DH, ld = 3 * D;
  const T* base = qkv + (size_t)b * Tn * ld + h * DH;
  const T* obase = o + (size_t)b * Tn * D + h * DH;
  const T* gbase = dout + (size_t)b * Tn * D + h * DH;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const float c2 = scale * 1.4426950408889634f;

  const int qb = qblk * Cfg::RB + 32 * wave;
  const bool active = qb < Tn;  // wave-uniform
  const bool qok = qb + col < Tn;
  const int qr = min(qb + col, Tn - 1);
  bf16x8 qfb[BF ? DH / 16 : 1], gfb[BF ? DH / 16 : 1];
  float qff[BF ? 1 : DH / 2], gff[BF ? 1 : DH / 2];
  if constexpr (BF) {
#pragma unroll
    for (int s = 0; s < DH / 16; ++s) {
      qfb[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)qr * ld + 16 * s + 8 * hh);
      gfb[s] = *reinterpret_cast<const bf16x8*>(gbase + (size_t)qr * D + 16 * s + 8 * hh);
    }
  } else {
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) {
      qff[s] = qok ? base[(size_t)qr * ld + 2 * s + hh] : 0.0f;
      gff[s] = qok ? gbase[(size_t)qr * D + 2 * s + hh] : 0.0f;
    }
  }
  const float lq = lse[(size_t)bh * Tn + qr];
  const float dq = stream_delta<T, DH>(obase + (size_t)qr * D, gbase + (size_t)qr * D);
  f32x16 dQ[NDT];
#pragma unroll
  for (int t = 0; t < NDT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dQ[t][r] = 0.0f;

  const int nch = (Tn + C - 1) / C;
  for (int ci = 0; ci < nch; ++ci) {
    const int c0 = ci * C;
    __syncthreads();  // every wave is done with the chunk before
    stream_stage2<T, DH, LD, C, NTHR>(A0, base + D, ld, A1, base + 2 * D, ld, c0, Tn, tid);
    __syncthreads();
    if (!active) continue;
    const int ntl = min(C / 32, (Tn - c0 + 31) / 32);
    for (int kt = 0; kt < ntl; ++kt) {
      f32x16 S, G;
#pragma unroll
      for (int r = 0; r < 16; ++r) S[r] = G[r] = 0.0f;
      if constexpr (BF) {
#pragma unroll
        for (int s = 0; s < DH / 16; ++s) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(A0 + (size_t)(kt * 32 + col) * LD + 16 * s + 8 * hh);
          S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qfb[s], S, 0, 0, 0);
          const bf16x8 v = *reinterpret_cast<const bf16x8*>(A1 + (size_t)(kt * 32 + col) * LD + 16 * s + 8 * hh);
          G = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v, gfb[s], G, 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int s = 0; s < DH / 2; ++s) {
          S = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[(size_t)(kt * 32 + col) * LD + 2 * s + hh], qff[s], S, 0, 0, 0);
          G = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[(size_t)(kt * 32 + col) * LD + 2 * s + hh], gff[s], G, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = c0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        const float p = (qok && key < Tn) ? exp2f(S[r] * c2 - lq) : 0.0f;
        G[r] = p * (G[r] - dq) * scale;
      }
      if constexpr (BF) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8 da;
#pragma unroll
          for (int j = 0; j < 8; ++j) da[j] = (bf16)G[8 * s + j];
          const int k0 = kt * 32 + 16 * s;
#pragma unroll
          for (int t = 0; t < NDT; ++t)
            dQ[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, stream_tr_frag<LD>(A0, k0, 32 * t, lane), dQ[t], 0, 0,
                                                            0);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kl = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
#pragma unroll
          for (int t = 0; t < NDT; ++t)
            dQ[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(G[r], A0[(size_t)kl * LD + 32 * t + col], dQ[t], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int t = 0; t < NDT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = qb + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (qi < Tn && 32 * t + col < DH)
        dqkv[((size_t)b * Tn + qi) * ld + h * DH + 32 * t + col] = to_out<T>(dQ[t][r]);
    }
}

// ================================================================================================ launchers
// the same block and chunk sizes at every head dim
MhaStreamSizes mha_stream_sizes(int dtype, int backward) {
  const bool bf = dtype == TMAE_BF16;
  if (backward) {
    constexpr int RB = StreamBwd<bf16, 32>::RB;
    return {RB, RB, bf ? StreamBwd<bf16, 32>::C : StreamBwd<float, 32>::C};
  }
  return {StreamFwd<bf16, 32>::QB, 0, bf ? StreamFwd<bf16, 32>::C : StreamFwd<float, 32>::C};
}

// workgroups of a launch: one per block of `rows` rows of every (image, head); the grid is an int
static int stream_grid(const char* who, int B, int H, int Tn, int rows, int* nblk, int* grid) {
  const long long nb = ((long long)Tn + rows - 1) / rows, g = (long long)B * H * nb;
  TMAE_REQUIRE(g <= 0x7fffffffLL, "%s: B * H * ceil(T / %d) = %lld workgroups exceed the grid limit", who, rows, g);
  *nblk = (int)nb;
  *grid = (int)g;
  return TMAE_OK;
}

template <typename T, int DH>
static int stream_fwd_launch(const void* qkv, void* out, float* lse, int B, int Tn, int H, float scale,
                             hipStream_t st) {
  using Cfg = StreamFwd<T, DH>;
  int nqb, grid;
  if (int rc = stream_grid("tmae_mha_fwd", B, H, Tn, Cfg::QB, &nqb, &grid)) return rc;
  hipLaunchKernelGGL((mha_fwd_stream_kernel<T, DH>), dim3(grid), dim3(Cfg::NTHR), 0, st, (const T*)qkv, (T*)out, lse,
                     Tn, H, nqb, scale * 1.4426950408889634f);
  TMAE_LAUNCH_CHECK("tmae_mha_fwd");
}

template <typename T, int DH>
static int stream_bwd_launch(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, int B,
                             int Tn, int H, float scale, hipStream_t st) {
  using Cfg = StreamBwd<T, DH>;
  int nb, grid;
  if (int rc = stream_grid("tmae_mha_bwd", B, H, Tn, Cfg::RB, &nb, &grid)) return rc;
  hipLaunchKernelGGL((mha_bwd_stream_dkv_kernel<T, DH>), dim3(grid), dim3(Cfg::NTHR), 0, st, (const T*)qkv,
                     (const T*)o, (const T*)dout, lse, (T*)dqkv, Tn, H, nb, scale);
  TMAE_LAUNCH_CHECK_NORET("tmae_mha_bwd");
  hipLaunchKernelGGL((mha_bwd_stream_dq_kernel<T, DH>), dim3(grid), dim3(Cfg::NTHR), 0, st, (const T*)qkv,
                     (const T*)o, (const T*)dout, lse, (T*)dqkv, Tn, H, nb, scale);
  TMAE_LAUNCH_CHECK("tmae_mha_bwd");
}

int mha_stream_fwd(const void* qkv, void* out, float* lse, int B, int T, int H, int dh, float scale, int dtype,
                   hipStream_t st) {
  TMAE_REQUIRE(B >= 0 && H >= 0 && T >= 0, "tmae_mha_fwd: negative shape");
  if ((long long)B * H == 0 || T == 0) return TMAE_OK;
  if (dtype == TMAE_BF16) {
    if (dh == 64) return stream_fwd_launch<bf16, 64>(qkv, out, lse, B, T, H, scale, st);
    if (dh == 80) return stream_fwd_launch<bf16, 80>(qkv, out, lse, B, T, H, scale, st);
    return stream_fwd_launch<bf16, 32>(qkv, out, lse, B, T, H, scale, st);
  }
  if (dh == 64) return stream_fwd_launch<float, 64>(qkv, out, lse, B, T, H, scale, st);
  if (dh == 80) return stream_fwd_launch<float, 80>(qkv, out, lse, B, T, H, scale, st);
  return stream_fwd_launch<float, 32>(qkv, out, lse, B, T, H, scale, st);
}

int mha_stream_bwd(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, int B, int T, int H,
                   int dh, float scale, int dtype, hipStream_t st) {
  TMAE_REQUIRE(B >= 0 && H >= 0 && T >= 0, "tmae_mha_bwd: negative shape");
  if ((long long)B * H == 0 || T == 0) return TMAE_OK;
  if (dtype == TMAE_BF16) {
    if (dh == 64) return stream_bwd_launch<bf16, 64>(qkv, o, dout, lse, dqkv, B, T, H, scale, st);
    if (dh == 80) return stream_bwd_launch<bf16, 80>(qkv, o, dout, lse, dqkv, B, T, H, scale, st);
    return stream_bwd_launch<bf16, 32>(qkv, o, dout, lse, dqkv, B, T, H, scale, st);
  }
  if (dh == 64) return stream_bwd_launch<float, 64>(qkv, o, dout, lse, dqkv, B, T, H, scale, st);
  if (dh == 80) return stream_bwd_launch<float, 80>(qkv, o, dout, lse, dqkv, B, T, H, scale, st);
  return stream_bwd_launch<float, 32>(qkv, o, dout, lse, dqkv, B, T, H, scale, st);
}
