// Fused multi-head attention: softmax(scale * Q K^T + mask) V per (batch,
// head), forward and a two-kernel backward. No [Tq, Tk] tensor is written and
// nothing here uses atomics: every output element has one writer and a fixed
// summation order, so two calls give bit-identical results.
//
// Operands. q, k, v (and dO) are read through (batch, head, row) element
// strides with a unit last stride, as bf16 or as fp32 rounded to bf16 while
// staging. Head dim 1 <= Dh <= 128 runs the instance DP in {32, 64, 128};
// d in Dh .. DP - 1 is zero-filled by guarded loads. Rows past Tq / Tk are
// zero-filled and never stored. O, dQ, dK, dV are contiguous
// [B, T, heads, Dh] in the input dtype; lse and delta are fp32
// [B, heads, Tq]. lse is kept in base 2: m + log2(sum 2^(s - m)) of the
// scores s = scale * log2(e) * q.k; a fully masked row has lse = 0, O = 0.
//
// Scale. The fp32 scores are scaled after the MFMA (one multiply per score).
// Folding scale * log2(e) into the bf16 Q fragments was not kept: it rounds
// q a second time, and the backward needs the unscaled Q for dK anyway.
//
// MFMA. v_mfma_f32_16x16x32_bf16: lane l gives A(row = l & 15, k = 8 (l >> 4)
// .. + 7), B(k = 8 (l >> 4) .. + 7, col = l & 15) and holds C(row = 4 (l >> 4)
// + r, col = l & 15). quad = l >> 4, col = l & 15 below.
//
// Key slots. A wave computes the scores of a 32-key group as two 16x16
// accumulators with keys as ROWS: S^T = K Q^T. Lane (quad, col) then holds,
// for query col, keys 4 quad + r and 16 + 4 quad + r. Those 8 values, rounded
// to bf16 in place, ARE a B operand (k = key slot, col = query) if slot
// (quad, j) is read as key 4 quad + j (j < 4) or 16 + 4 quad + j - 4. The
// other operand only has to use the same slot order: it is read from a
// TRANSPOSED LDS tile [d][key] as two 8-byte pieces. So P never goes through
// LDS, and the second product comes out transposed, O^T[d][query = col]: the
// running max, sum and the rescale factor of a query live in the lanes that
// hold its column. The same trick carries dS into dQ (attn_bwd_dq), and with
// queries and keys exchanged P^T and dS^T into dV and dK (attn_bwd_dkv).
//
// attn_fwd / attn_bwd_dq: grid = B * heads * ceil(Tq / 64), 4 waves, 16
// query rows per wave; Q (and dO) fragments stay in registers; the key loop
// stages 64 keys per step: K as [64][DP + 8] (16-byte fragment reads, rows
// shifted by 4 banks), V^T (forward) or K^T and V (dq) likewise.
// attn_bwd_dkv: grid = B * heads * ceil(Tk / 64), 16 keys per wave with the K
// and V fragments in registers; the query loop stages Q, Q^T, dO, dO^T, lse
// and delta for 64 queries (DP <= 64) or 32 (DP = 128, to stay under 64 KB of
// static LDS). Key tiles that are wholly masked are skipped block-uniformly:
// every wave ballots the same 64 mask bytes, so all waves agree without LDS.
#include "common.h"

#include <c10/util/BFloat16.h>
#include <c10/util/Optional.h>

#include <algorithm>
#include <cmath>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

constexpr int ATTN_MAX_DH = 128;
constexpr int ATTN_THREADS = 256;  // 4 waves
constexpr int ATTN_BQ = 64;        // query rows per block (fwd, dq): 16 a wave
constexpr int ATTN_BK = 64;        // keys per tile: the width of a ballot
constexpr int ATTN_PAD = 8;        // bf16 elements of LDS row padding (16 B)
constexpr float ATTN_LOG2E = 1.4426950408889634f;

// query rows per step of attn_bwd_dkv: four tiles (Q, Q^T, dO, dO^T) in LDS
constexpr int attn_dkv_bq(int dp) { return dp > 64 ? 32 : 64; }

// one (batch, head, row)-strided operand; strides in elements
struct AttnView {
  const void* p;
  int64_t sb, sh, st;
};

// 8 consecutive elements as bf16; elements n .. 7 are zero and not read
template <typename T>
__device__ inline bf16x8 attn_load8(const T* p, int n, bool vec) {
  bf16x8 out;
  if (vec && n >= 8) {
    if constexpr (std::is_same<T, float>::value) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p);
      const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        out[i] = (__bf16)a[i];
        out[4 + i] = (__bf16)b[i];
      }
    } else {
      out = *reinterpret_cast<const bf16x8*>(p);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float v = 0.0f;
      if (i < n) v = (float)p[i];
      out[i] = (__bf16)v;
    }
  }
  return out;
}

// rows r0 .. r0 + ROWS - 1 of a [R, Dh] slice -> s[row][d], zero-filled
template <typename T, int ROWS, int DP, int LD>
__device__ inline void attn_stage_rows(const T* base, int64_t st, int r0,
                                       int R, int Dh, bool vec,
                                       __bf16 (*s)[LD]) {
  constexpr int CH = DP / 8;
  for (int idx = threadIdx.x; idx < ROWS * CH; idx += ATTN_THREADS) {
    const int row = idx / CH, c = idx - row * CH;
    const int n = r0 + row < R ? Dh - c * 8 : 0;
    *reinterpret_cast<bf16x8*>(&s[row][c * 8]) =
        attn_load8(base + (int64_t)(r0 + row) * st + c * 8, n, vec);
  }
}

// the same rows -> sT[d][row] (a wave writes 64 consecutive rows of one d)
// and, with ROWMAJOR, s[row][d] from the same load
template <typename T, int ROWS, int DP, int LDR, int LDT, bool ROWMAJOR>
__device__ inline void attn_stage_tr(const T* base, int64_t st, int r0, int R,
                                     int Dh, bool vec, __bf16 (*s)[LDR],
                                     __bf16 (*sT)[LDT]) {
  constexpr int CH = DP / 8;
  for (int idx = threadIdx.x; idx < ROWS * CH; idx += ATTN_THREADS) {
    const int c = idx / ROWS, row = idx - c * ROWS;
    const int n = r0 + row < R ? Dh - c * 8 : 0;
    const bf16x8 v =
        attn_load8(base + (int64_t)(r0 + row) * st + c * 8, n, vec);
    if constexpr (ROWMAJOR) *reinterpret_cast<bf16x8*>(&s[row][c * 8]) = v;
#pragma unroll
    for (int i = 0; i < 8; ++i) sT[c * 8 + i][row] = v[i];
  }
}

// operand of the slot order above from a transposed tile: [x][g0 + 4 quad ..]
// and [x][g0 + 16 + 4 quad ..]
template <int LDT>
__device__ inline bf16x8 attn_slots(__bf16 (*sT)[LDT], int x, int g0,
                                    int quad) {
  const bf16x4 lo = *reinterpret_cast<const bf16x4*>(&sT[x][g0 + quad * 4]);
  const bf16x4 hi =
      *reinterpret_cast<const bf16x4*>(&sT[x][g0 + 16 + quad * 4]);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ inline bf16x8 attn_pack(const f32x4& lo, const f32x4& hi) {
  bf16x8 out;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    out[i] = (__bf16)lo[i];
    out[4 + i] = (__bf16)hi[i];
  }
  return out;
}

// 4 consecutive d of one row, d = d0 .. d0 + 3, guarded by Dh
template <typename T>
__device__ inline void attn_store4(T* row, int d0, int Dh, bool vec4,
                                   const f32x4& v) {
  if (vec4 && d0 + 3 < Dh) {
    if constexpr (std::is_same<T, float>::value) {
      *reinterpret_cast<f32x4*>(row + d0) = v;
    } else {
      bf16x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (__bf16)v[i];
      *reinterpret_cast<bf16x4*>(row + d0) = o;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (d0 + i < Dh) row[d0 + i] = (T)v[i];
  }
}

// bit i: key k0 + i exists and is not masked (the same word in every wave)
__device__ inline unsigned long long attn_live(const unsigned char* mask,
                                               int64_t b, int Tk, int k0) {
  const int kk = k0 + (int)(threadIdx.x & 63);
  bool ok = kk < Tk;
  if (ok && mask != nullptr) ok = mask[b * Tk + kk] == 0;
  return __ballot(ok);
}

__device__ inline float attn_quad_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}

__device__ inline float attn_quad_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

}  // namespace

// ------------------------------------------------------------------ forward
template <typename T, int DP>
__global__ void __launch_bounds__(ATTN_THREADS)
attn_fwd_kernel(AttnView q, AttnView k, AttnView v,
                const unsigned char* __restrict__ mask, T* __restrict__ o,
                float* __restrict__ lse, int heads, int Tq, int Tk, int Dh,
                float scale, int causal, int vec) {
  constexpr int KS = DP / 32, ND = DP / 16;
  constexpr int LDK = DP + ATTN_PAD, LDT = ATTN_BK + ATTN_PAD;
  __shared__ __attribute__((aligned(16))) __bf16 s_k[ATTN_BK][LDK];
  __shared__ __attribute__((aligned(16))) __bf16 s_vt[DP][LDT];

  const int nqt = (Tq + ATTN_BQ - 1) / ATTN_BQ;
  const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt;
  const int h = bh % heads;
  const int64_t b = bh / heads;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 15, quad = lane >> 4;
  const int q0 = qt * ATTN_BQ;
  const int qrow = q0 + wave * 16 + col;  // the lane's query

  const T* qb = static_cast<const T*>(q.p) + b * q.sb + h * q.sh;
  const T* kb = static_cast<const T*>(k.p) + b * k.sb + h * k.sh;
  const T* vb = static_cast<const T*>(v.p) + b * v.sb + h * v.sh;

  bf16x8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int d0 = ks * 32 + quad * 8;
    qf[ks] = attn_load8(qb + (int64_t)qrow * q.st + d0,
                        qrow < Tq ? Dh - d0 : 0, vec != 0);
  }

  const float sc = scale * ATTN_LOG2E;
  float m = -INFINITY, l = 0.0f;
  f32x4 oacc[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) oacc[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  int nkt = (Tk + ATTN_BK - 1) / ATTN_BK;
  if (causal) {  // the block's last row sees keys <= itself
    const int last = min(q0 + ATTN_BQ, Tq) - 1;
    nkt = min(nkt, last / ATTN_BK + 1);
  }
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * ATTN_BK;
    const unsigned long long live = attn_live(mask, b, Tk, k0);
    if (live == 0) continue;  // block-uniform
    __syncthreads();          // the tiles of the step before are done with
    attn_stage_rows<T, ATTN_BK, DP, LDK>(kb, k.st, k0, Tk, Dh, vec != 0, s_k);
    attn_stage_tr<T, ATTN_BK, DP, LDK, LDT, false>(vb, v.st, k0, Tk, Dh,
                                                   vec != 0, nullptr, s_vt);
    __syncthreads();

    // st[t][r] = S^T(key = 16 t + 4 quad + r, query = col)
    f32x4 st[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(
            &s_k[t * 16 + col][ks * 32 + quad * 8]);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf[ks], st[t], 0,
                                                        0, 0);
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = t * 16 + quad * 4 + r;
        bool ok = (live >> key) & 1ull;
        if (causal) ok = ok && k0 + key <= qrow;
        st[t][r] = ok ? st[t][r] * sc : -INFINITY;
        mx = fmaxf(mx, st[t][r]);
      }
    mx = attn_quad_max(mx);
    const float m_new = fmaxf(m, mx);
    // every key so far masked: keep the exponents finite, all terms are 0
    const float m_use = m_new == -INFINITY ? 0.0f : m_new;
    const float alpha = exp2f(m - m_use);
    float psum = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st[t][r] = exp2f(st[t][r] - m_use);
        psum += st[t][r];
      }
    l = l * alpha + attn_quad_sum(psum);
    m = m_new;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) oacc[dt][r] *= alpha;
    // O^T(d = 16 dt + 4 quad + r, query = col) += V^T P^T
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const bf16x8 pb = attn_pack(st[2 * g], st[2 * g + 1]);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
        const bf16x8 a = attn_slots<LDT>(s_vt, dt * 16 + col, g * 32, quad);
        oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pb, oacc[dt], 0,
                                                           0, 0);
      }
    }
  }

  if (qrow < Tq) {
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;
    T* orow = o + ((b * Tq + qrow) * heads + h) * Dh;
    const bool vec4 = (Dh & 3) == 0;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      f32x4 val;
#pragma unroll
      for (int r = 0; r < 4; ++r) val[r] = oacc[dt][r] * inv;
      attn_store4(orow, dt * 16 + quad * 4, Dh, vec4, val);
    }
    if (quad == 0)
      lse[(b * heads + h) * Tq + qrow] = l > 0.0f ? m + log2f(l) : 0.0f;
  }
}

// -------------------------------------------------------------------- delta
// delta(b, h, q) = sum_d dO O: 16 lanes per row, a fixed butterfly
template <typename T>
__global__ void __launch_bounds__(ATTN_THREADS)
attn_delta_kernel(const T* __restrict__ o, AttnView dO,
                  float* __restrict__ delta, int64_t rows, int heads, int Tq,
                  int Dh) {
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  float acc = 0.0f;
  if (row < rows) {
    const int64_t bh = row / Tq, qr = row - bh * Tq;
    const int64_t b = bh / heads, h = bh - b * heads;
    const T* orow = o + ((b * Tq + qr) * heads + h) * Dh;
    const T* grow =
        static_cast<const T*>(dO.p) + b * dO.sb + h * dO.sh + qr * dO.st;
    for (int d = sub; d < Dh; d += 16)
      acc += (float)orow[d] * (float)grow[d];
  }
#pragma unroll
  for (int s = 8; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
  if (sub == 0 && row < rows) delta[row] = acc;
}

// ------------------------------------------------------------- backward dK dV
template <typename T, int DP>
__global__ void __launch_bounds__(ATTN_THREADS)
attn_bwd_dkv_kernel(AttnView q, AttnView k, AttnView v, AttnView dO,
                    const unsigned char* __restrict__ mask,
                    const float* __restrict__ lse,
                    const float* __restrict__ delta, T* __restrict__ dk,
                    T* __restrict__ dv, int heads, int Tq, int Tk, int Dh,
                    float scale, int causal, int vec) {
  constexpr int BQ = attn_dkv_bq(DP);
  constexpr int KS = DP / 32, ND = DP / 16;
  constexpr int LDR = DP + ATTN_PAD, LDT = BQ + ATTN_PAD;
  __shared__ __attribute__((aligned(16))) __bf16 s_q[BQ][LDR];
  __shared__ __attribute__((aligned(16))) __bf16 s_do[BQ][LDR];
  __shared__ __attribute__((aligned(16))) __bf16 s_qt[DP][LDT];
  __shared__ __attribute__((aligned(16))) __bf16 s_dot[DP][LDT];
  __shared__ float s_lse[BQ], s_dl[BQ];

  const int nkt = (Tk + ATTN_BK - 1) / ATTN_BK;
  const int kt = blockIdx.x % nkt, bh = blockIdx.x / nkt;
  const int h = bh % heads;
  const int64_t b = bh / heads;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 15, quad = lane >> 4;
  const int k0 = kt * ATTN_BK;
  const int key = k0 + wave * 16 + col;  // the lane's key in S, dP

  const T* qb = static_cast<const T*>(q.p) + b * q.sb + h * q.sh;
  const T* kb = static_cast<const T*>(k.p) + b * k.sb + h * k.sh;
  const T* vb = static_cast<const T*>(v.p) + b * v.sb + h * v.sh;
  const T* gb = static_cast<const T*>(dO.p) + b * dO.sb + h * dO.sh;
  const float* lse_b = lse + (b * heads + h) * Tq;
  const float* dl_b = delta + (b * heads + h) * Tq;

  f32x4 dkacc[ND], dvacc[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) {
    dkacc[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    dvacc[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  const unsigned long long live = attn_live(mask, b, Tk, k0);
  if (live != 0) {  // block-uniform: a wholly masked tile stores zeros
    const bool keyok = (live >> (wave * 16 + col)) & 1ull;
    bf16x8 kf[KS], vf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = ks * 32 + quad * 8;
      const int n = key < Tk ? Dh - d0 : 0;
      kf[ks] = attn_load8(kb + (int64_t)key * k.st + d0, n, vec != 0);
      vf[ks] = attn_load8(vb + (int64_t)key * v.st + d0, n, vec != 0);
    }
    const float sc = scale * ATTN_LOG2E;
    const int nqt = (Tq + BQ - 1) / BQ;
    for (int qt = causal ? k0 / BQ : 0; qt < nqt; ++qt) {
      const int q0 = qt * BQ;
      __syncthreads();
      attn_stage_tr<T, BQ, DP, LDR, LDT, true>(qb, q.st, q0, Tq, Dh, vec != 0,
                                               s_q, s_qt);
      attn_stage_tr<T, BQ, DP, LDR, LDT, true>(gb, dO.st, q0, Tq, Dh,
                                               vec != 0, s_do, s_dot);
      if (threadIdx.x < BQ) {
        const int qq = q0 + threadIdx.x;
        s_lse[threadIdx.x] = qq < Tq ? lse_b[qq] : 0.0f;
        s_dl[threadIdx.x] = qq < Tq ? dl_b[qq] : 0.0f;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < BQ / 32; ++c) {
        // s[hf][r], dp[hf][r]: (query = 32 c + 16 hf + 4 quad + r, key = col)
        f32x4 s[2], dp[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          s[hf] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          dp[hf] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          const int row = c * 32 + hf * 16 + col;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 aq = *reinterpret_cast<const bf16x8*>(
                &s_q[row][ks * 32 + quad * 8]);
            const bf16x8 ag = *reinterpret_cast<const bf16x8*>(
                &s_do[row][ks * 32 + quad * 8]);
            s[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq, kf[ks], s[hf],
                                                            0, 0, 0);
            dp[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ag, vf[ks],
                                                             dp[hf], 0, 0, 0);
          }
        }
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ql = c * 32 + hf * 16 + quad * 4 + r;
            bool ok = keyok && q0 + ql < Tq;
            if (causal) ok = ok && key <= q0 + ql;
            const float p = ok ? exp2f(s[hf][r] * sc - s_lse[ql]) : 0.0f;
            s[hf][r] = p;
            dp[hf][r] = p * (dp[hf][r] - s_dl[ql]) * scale;
          }
        // P^T and dS^T (key = col, query slots) are A operands as they are
        const bf16x8 pa = attn_pack(s[0], s[1]);
        const bf16x8 dsa = attn_pack(dp[0], dp[1]);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          const bf16x8 bg = attn_slots<LDT>(s_dot, dt * 16 + col, c * 32, quad);
          const bf16x8 bq = attn_slots<LDT>(s_qt, dt * 16 + col, c * 32, quad);
          dvacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, bg, dvacc[dt],
                                                              0, 0, 0);
          dkacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa, bq,
                                                              dkacc[dt], 0, 0, 0);
        }
      }
    }
  }
  // acc[dt][r]: (key = 16 wave + 4 quad + r, d = 16 dt + col)
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kr = k0 + wave * 16 + quad * 4 + r, d = dt * 16 + col;
      if (kr < Tk && d < Dh) {
        const int64_t idx = ((b * Tk + kr) * heads + h) * Dh + d;
        dk[idx] = (T)dkacc[dt][r];
        dv[idx] = (T)dvacc[dt][r];
      }
    }
}

// ---------------------------------------------------------------- backward dQ
template <typename T, int DP>
__global__ void __launch_bounds__(ATTN_THREADS)
attn_bwd_dq_kernel(AttnView q, AttnView k, AttnView v, AttnView dO,
                   const unsigned char* __restrict__ mask,
                   const float* __restrict__ lse,
                   const float* __restrict__ delta, T* __restrict__ dq,
                   int heads, int Tq, int Tk, int Dh, float scale, int causal,
                   int vec) {
  constexpr int KS = DP / 32, ND = DP / 16;
  constexpr int LDK = DP + ATTN_PAD, LDT = ATTN_BK + ATTN_PAD;
  __shared__ __attribute__((aligned(16))) __bf16 s_k[ATTN_BK][LDK];
  __shared__ __attribute__((aligned(16))) __bf16 s_v[ATTN_BK][LDK];
  __shared__ __attribute__((aligned(16))) __bf16 s_kt[DP][LDT];

  const int nqt = (Tq + ATTN_BQ - 1) / ATTN_BQ;
  const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt;
  const int h = bh % heads;
  const int64_t b = bh / heads;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 15, quad = lane >> 4;
  const int q0 = qt * ATTN_BQ;
  const int qrow = q0 + wave * 16 + col;

  const T* qb = static_cast<const T*>(q.p) + b * q.sb + h * q.sh;
  const T* kb = static_cast<const T*>(k.p) + b * k.sb + h * k.sh;
  const T* vb = static_cast<const T*>(v.p) + b * v.sb + h * v.sh;
  const T* gb = static_cast<const T*>(dO.p) + b * dO.sb + h * dO.sh;

  bf16x8 qf[KS], gf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int d0 = ks * 32 + quad * 8;
    const int n = qrow < Tq ? Dh - d0 : 0;
    qf[ks] = attn_load8(qb + (int64_t)qrow * q.st + d0, n, vec != 0);
    gf[ks] = attn_load8(gb + (int64_t)qrow * dO.st + d0, n, vec != 0);
  }
  float lse_q = 0.0f, dl_q = 0.0f;
  if (qrow < Tq) {
    lse_q = lse[(b * heads + h) * Tq + qrow];
    dl_q = delta[(b * heads + h) * Tq + qrow];
  }
  const float sc = scale * ATTN_LOG2E;
  f32x4 dqacc[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) dqacc[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  int nkt = (Tk + ATTN_BK - 1) / ATTN_BK;
  if (causal) {
    const int last = min(q0 + ATTN_BQ, Tq) - 1;
    nkt = min(nkt, last / ATTN_BK + 1);
  }
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * ATTN_BK;
    const unsigned long long live = attn_live(mask, b, Tk, k0);
    if (live == 0) continue;  // block-uniform
    __syncthreads();
    attn_stage_tr<T, ATTN_BK, DP, LDK, LDT, true>(kb, k.st, k0, Tk, Dh,
                                                  vec != 0, s_k, s_kt);
    attn_stage_rows<T, ATTN_BK, DP, LDK>(vb, v.st, k0, Tk, Dh, vec != 0, s_v);
    __syncthreads();
    // st, dpt: (key = 16 t + 4 quad + r, query = col)
    f32x4 st[4], dpt[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      dpt[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 ak = *reinterpret_cast<const bf16x8*>(
            &s_k[t * 16 + col][ks * 32 + quad * 8]);
        const bf16x8 av = *reinterpret_cast<const bf16x8*>(
            &s_v[t * 16 + col][ks * 32 + quad * 8]);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak, qf[ks], st[t], 0,
                                                        0, 0);
        dpt[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, gf[ks], dpt[t], 0,
                                                         0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kl = t * 16 + quad * 4 + r;
        bool ok = ((live >> kl) & 1ull) && qrow < Tq;
        if (causal) ok = ok && k0 + kl <= qrow;
        const float p = ok ? exp2f(st[t][r] * sc - lse_q) : 0.0f;
        dpt[t][r] = p * (dpt[t][r] - dl_q) * scale;
      }
    // dQ^T(d = 16 dt + 4 quad + r, query = col) += K^T dS^T
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const bf16x8 dsb = attn_pack(dpt[2 * g], dpt[2 * g + 1]);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
        const bf16x8 a = attn_slots<LDT>(s_kt, dt * 16 + col, g * 32, quad);
        dqacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, dsb, dqacc[dt],
                                                            0, 0, 0);
      }
    }
  }
  if (qrow < Tq) {
    T* row = dq + ((b * Tq + qrow) * heads + h) * Dh;
    const bool vec4 = (Dh & 3) == 0;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
      attn_store4(row, dt * 16 + quad * 4, Dh, vec4, dqacc[dt]);
  }
}

// ---------------------------------------------------------------- host side
namespace {

struct AttnArgs {
  int64_t B, heads, Tq, Tk, Dh;
  int dp;
  bool bf16;
  bool vec = true;
  const unsigned char* mask = nullptr;
};

// [B, heads, T, Dh] with a unit last stride -> view; clears a.vec when a
// 16-byte load of 8 elements could be misaligned
AttnView attn_view(const torch::Tensor& t, const char* name, int64_t T,
                   AttnArgs& a) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 4 && t.size(0) == a.B &&
              t.size(1) == a.heads && t.size(2) == T && t.size(3) == a.Dh,
              "attention: ", name, " must be a GPU tensor [", a.B, ", ",
              a.heads, ", ", T, ", ", a.Dh, "]");
  TORCH_CHECK(t.scalar_type() == (a.bf16 ? torch::kBFloat16 : torch::kFloat32),
              "attention: ", name, " must have q's dtype");
  TORCH_CHECK(a.Dh == 1 || t.stride(3) == 1, "attention: ", name,
              " needs a unit last stride");
  AttnView vw;
  vw.p = t.data_ptr();
  vw.sb = a.B > 1 ? t.stride(0) : 0;
  vw.sh = a.heads > 1 ? t.stride(1) : 0;
  vw.st = T > 1 ? t.stride(2) : 0;
  const int64_t al = a.bf16 ? 8 : 4;  // elements per 16 bytes
  if (reinterpret_cast<uintptr_t>(vw.p) % 16 != 0 || vw.sb % al != 0 ||
      vw.sh % al != 0 || vw.st % al != 0)
    a.vec = false;
  return vw;
}

AttnArgs attn_args(const torch::Tensor& q, const torch::Tensor& k,
                   const c10::optional<torch::Tensor>& mask, bool causal) {
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4,
              "attention: q and k must be [B, heads, T, Dh]");
  AttnArgs a;
  a.B = q.size(0), a.heads = q.size(1), a.Tq = q.size(2), a.Dh = q.size(3);
  a.Tk = k.size(2);
  TORCH_CHECK(a.B >= 1 && a.heads >= 1 && a.Tq >= 1 && a.Tk >= 1 &&
              a.Dh >= 1 && a.Dh <= ATTN_MAX_DH,
              "attention: needs B, heads, Tq, Tk >= 1 and 1 <= Dh <= ",
              ATTN_MAX_DH);
  TORCH_CHECK(!causal || a.Tq == a.Tk, "attention: causal needs Tq == Tk");
  TORCH_CHECK(q.scalar_type() == torch::kFloat32 ||
              q.scalar_type() == torch::kBFloat16,
              "attention: fp32 or bf16 only");
  a.bf16 = q.scalar_type() == torch::kBFloat16;
  a.dp = a.Dh <= 32 ? 32 : a.Dh <= 64 ? 64 : 128;
  // one block per (batch, head, 64-row tile) on grid.x; rows index as int
  const int64_t lim = ((int64_t)1 << 31) - 1;
  const int64_t tmax = std::max(a.Tq, a.Tk);
  TORCH_CHECK(tmax <= lim - 2 * ATTN_BK &&
              a.B * a.heads * ((tmax + 15) / 16) <= lim,
              "attention: B * heads * ceil(T / 16) = ",
              a.B * a.heads * ((tmax + 15) / 16),
              " exceeds the launch limit of ", lim, " blocks");
  if (mask.has_value()) {
    TORCH_CHECK(mask->is_cuda() && mask->scalar_type() == torch::kBool &&
                mask->dim() == 2 && mask->size(0) == a.B &&
                mask->size(1) == a.Tk && mask->is_contiguous(),
                "attention: key_padding_mask must be a contiguous bool GPU "
                "tensor [B, Tk]");
    a.mask = static_cast<const unsigned char*>(mask->data_ptr());
  }
  return a;
}

template <class T>
struct AttnType { using type = T; };

// f(element type tag, padded head dim constant)
template <class F>
void attn_dispatch(const AttnArgs& a, F&& f) {
  auto by_dp = [&](auto tag) {
    switch (a.dp) {
      case 32: f(tag, IntC<32>{}); break;
      case 64: f(tag, IntC<64>{}); break;
      default: f(tag, IntC<128>{}); break;
    }
  };
  if (a.bf16) by_dp(AttnType<c10::BFloat16>{});
  else by_dp(AttnType<float>{});
}

unsigned attn_blocks(const AttnArgs& a, int64_t T, int64_t tile) {
  return (unsigned)(a.B * a.heads * ((T + tile - 1) / tile));
}

}  // namespace

// q [B, heads, Tq, Dh], k and v [B, heads, Tk, Dh] (any batch / head / row
// strides) -> (O [B, Tq, heads, Dh] in q's dtype, lse [B, heads, Tq] fp32)
std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v,
                                    c10::optional<torch::Tensor> mask,
                                    bool causal, double scale) {
  AttnArgs a = attn_args(q, k, mask, causal);
  const AttnView qv = attn_view(q, "q", a.Tq, a);
  const AttnView kv = attn_view(k, "k", a.Tk, a);
  const AttnView vv = attn_view(v, "v", a.Tk, a);
  auto o = torch::empty({a.B, a.Tq, a.heads, a.Dh}, q.options());
  auto lse = torch::empty({a.B, a.heads, a.Tq},
                          q.options().dtype(torch::kFloat32));
  attn_dispatch(a, [&](auto tag, auto dpc) {
    using T = typename decltype(tag)::type;
    constexpr int DP = decltype(dpc)::value;
    hipLaunchKernelGGL((attn_fwd_kernel<T, DP>),
                       dim3(attn_blocks(a, a.Tq, ATTN_BQ)), dim3(ATTN_THREADS),
                       0, current_stream(), qv, kv, vv, a.mask,
                       static_cast<T*>(o.data_ptr()), lse.data_ptr<float>(),
                       (int)a.heads, (int)a.Tq, (int)a.Tk, (int)a.Dh,
                       (float)scale, (int)causal, (int)a.vec);
  });
  return {o, lse};
}

// delta [B, heads, Tq] = rowsum(dO * O); o is attn_fwd's buffer, dout a
// [B, heads, Tq, Dh] view
torch::Tensor attn_delta(torch::Tensor o, torch::Tensor dout) {
  TORCH_CHECK(o.is_cuda() && o.dim() == 4 && o.is_contiguous(),
              "attn_delta: o must be attn_fwd's [B, Tq, heads, Dh] buffer");
  AttnArgs a;
  a.B = o.size(0), a.Tq = o.size(1), a.heads = o.size(2), a.Dh = o.size(3);
  a.bf16 = o.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(a.bf16 || o.scalar_type() == torch::kFloat32,
              "attn_delta: fp32 or bf16 only");
  const AttnView gv = attn_view(dout, "dout", a.Tq, a);
  auto delta = torch::empty({a.B, a.heads, a.Tq},
                            o.options().dtype(torch::kFloat32));
  const int64_t rows = a.B * a.heads * a.Tq;
  TORCH_CHECK((rows + 15) / 16 <= ((int64_t)1 << 31) - 1,
              "attn_delta: too many rows for one launch");
  const dim3 grid((unsigned)((rows + 15) / 16));
  if (a.bf16) {
    hipLaunchKernelGGL(attn_delta_kernel<c10::BFloat16>, grid,
                       dim3(ATTN_THREADS), 0, current_stream(),
                       static_cast<const c10::BFloat16*>(o.data_ptr()), gv,
                       delta.data_ptr<float>(), rows, (int)a.heads, (int)a.Tq,
                       (int)a.Dh);
  } else {
    hipLaunchKernelGGL(attn_delta_kernel<float>, grid, dim3(ATTN_THREADS), 0,
                       current_stream(), o.data_ptr<float>(), gv,
                       delta.data_ptr<float>(), rows, (int)a.heads, (int)a.Tq,
                       (int)a.Dh);
  }
  return delta;
}

namespace {

void attn_check_stats(const torch::Tensor& t, const AttnArgs& a,
                      const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == torch::kFloat32 &&
              t.numel() == a.B * a.heads * a.Tq,
              "attention: ", name, " must be contiguous fp32 [B, heads, Tq]");
}

}  // namespace

// (dK, dV), each [B, Tk, heads, Dh] in q's dtype
std::vector<torch::Tensor> attn_bwd_dkv(torch::Tensor q, torch::Tensor k,
                                        torch::Tensor v, torch::Tensor dout,
                                        c10::optional<torch::Tensor> mask,
                                        torch::Tensor lse, torch::Tensor delta,
                                        bool causal, double scale) {
  AttnArgs a = attn_args(q, k, mask, causal);
  const AttnView qv = attn_view(q, "q", a.Tq, a);
  const AttnView kv = attn_view(k, "k", a.Tk, a);
  const AttnView vv = attn_view(v, "v", a.Tk, a);
  const AttnView gv = attn_view(dout, "dout", a.Tq, a);
  attn_check_stats(lse, a, "lse");
  attn_check_stats(delta, a, "delta");
  auto dk = torch::empty({a.B, a.Tk, a.heads, a.Dh}, q.options());
  auto dv = torch::empty({a.B, a.Tk, a.heads, a.Dh}, q.options());
  attn_dispatch(a, [&](auto tag, auto dpc) {
    using T = typename decltype(tag)::type;
    constexpr int DP = decltype(dpc)::value;
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, DP>),
                       dim3(attn_blocks(a, a.Tk, ATTN_BK)), dim3(ATTN_THREADS),
                       0, current_stream(), qv, kv, vv, gv, a.mask,
                       lse.data_ptr<float>(), delta.data_ptr<float>(),
                       static_cast<T*>(dk.data_ptr()),
                       static_cast<T*>(dv.data_ptr()), (int)a.heads, (int)a.Tq,
                       (int)a.Tk, (int)a.Dh, (float)scale, (int)causal,
                       (int)a.vec);
  });
  return {dk, dv};
}

// dQ [B, Tq, heads, Dh] in q's dtype
torch::Tensor attn_bwd_dq(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                          torch::Tensor dout,
                          c10::optional<torch::Tensor> mask, torch::Tensor lse,
                          torch::Tensor delta, bool causal, double scale) {
  AttnArgs a = attn_args(q, k, mask, causal);
  const AttnView qv = attn_view(q, "q", a.Tq, a);
  const AttnView kv = attn_view(k, "k", a.Tk, a);
  const AttnView vv = attn_view(v, "v", a.Tk, a);
  const AttnView gv = attn_view(dout, "dout", a.Tq, a);
  attn_check_stats(lse, a, "lse");
  attn_check_stats(delta, a, "delta");
  auto dq = torch::empty({a.B, a.Tq, a.heads, a.Dh}, q.options());
  attn_dispatch(a, [&](auto tag, auto dpc) {
    using T = typename decltype(tag)::type;
    constexpr int DP = decltype(dpc)::value;
    hipLaunchKernelGGL((attn_bwd_dq_kernel<T, DP>),
                       dim3(attn_blocks(a, a.Tq, ATTN_BQ)), dim3(ATTN_THREADS),
                       0, current_stream(), qv, kv, vv, gv, a.mask,
                       lse.data_ptr<float>(), delta.data_ptr<float>(),
                       static_cast<T*>(dq.data_ptr()), (int)a.heads, (int)a.Tq,
                       (int)a.Tk, (int)a.Dh, (float)scale, (int)causal,
                       (int)a.vec);
  });
  return dq;
}
