// Transposed convolution, kernel 2x2x2 / stride 2 (the learned 2x upsample of
// the 3D U-Net family): y = conv_transpose3d(x, w, bias, stride = 2) with
// x[N,Cin,D,H,W], w[Cin,Cout,2,2,2] (torch's layout), y[N,Cout,2D,2H,2W],
// bf16 operands, fp32 accumulation on v_mfma_f32_16x16x32_bf16.
//
// Kernel == stride, so taps never overlap: output parity class
// p = (pd, ph, pw), packed pd*4 + ph*2 + pw, is a pointwise GEMM of the
// low-res input with its own [Cout, Cin] slice of w:
//   fwd    y[n, co, 2s + p]  = bias[co] + sum_ci x[n, ci, s] w[ci, co, p]
//   dgrad  dx[n, ci, s]      = sum_{co, p} go[n, co, 2s + p] w[ci, co, p]
//   wgrad  dw[ci, co, p]     = sum_{n, s} x[n, ci, s] go[n, co, 2s + p]
// with s = (d, h, w) a low-res position and 2s + p = (2d+pd, 2h+ph, 2w+pw).
// All three are HBM-bound (about 50 FLOP/byte at 64 -> 32 channels): each
// reads its large operand once and writes its result once, and a block serves
// all 8 classes from one staged tile.
//
// Positions are tiled FLAT: s = (d*H + h)*W + w is contiguous per (n, ci) in
// x and dx, so a tile of DC_PT consecutive s is one contiguous run per
// channel at any W; only the high-res side (y, go) decodes s into (d, h, w),
// where every low-res position owns the adjacent pair (2w, 2w+1) of 4 rows.
//
// The MFMA kernels have no fp32 VALU arithmetic (the bias enters as the
// accumulators' initial value), so they cannot compile to the packed-fp32
// forms; the one kernel that adds fp32 values, deconv3d_wgrad_fold_kernel,
// carries target("no-packed-fp32-ops").
#include "common.h"

#include <hip/hip_bf16.h>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

struct DcDims {
  int N, Cin, Cout;
  int D, H, W;  // low-res side; the high-res side is 2D x 2H x 2W
  int S;        // D*H*W
};

constexpr int DC_PT = 64;   // low-res positions per tile
constexpr int DC_KST = 4;   // 32-wide k-steps staged per barrier pair

// Operand tile shared by the forward (k = ci) and the dgrad (k = (co, p)):
// [k-step][DC_PT positions][32 k] bf16, k innermost, so lane (position, kg)
// reads its 8 k as one 16-byte word. A position is 64 B = 16 banks and
// position mod 4 picks the quarter of the 64 banks; the 16-byte chunk is
// XORed with bits 2-3 of the position, so the 4 positions of a 16-lane group
// that share a quarter (p, p+4, p+8, p+12) sit on its 4 distinct chunks:
// every 16-lane group of a ds_read_b128 covers the 64 banks once, whichever
// kg values it mixes.
__device__ __forceinline__ int dc_off(int pos, int chunk) {
  return pos * 32 + ((chunk ^ ((pos >> 2) & 3)) << 3);
}

// element offset of high-res (2d+pd, 2h+ph, 2w) inside one (n, co) volume
__device__ __forceinline__ int64_t dc_hi_off(const DcDims& dd, int s, int pd,
                                             int ph) {
  const int hw = dd.H * dd.W;
  const int d = s / hw, r = s - d * hw;
  const int h = r / dd.W, w = r - h * dd.W;
  return ((int64_t)(2 * d + pd) * (2 * dd.H) + (2 * h + ph)) * (2 * dd.W) +
         2 * w;
}

__device__ __forceinline__ unsigned dc_pack(float a, float b) {
  const bf16x2 v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(unsigned, v);
}

// 4x4 transpose of 32-bit words across the 4 lanes of a quad: lane q gives
// v[r], r = 0..3, and ends with v[j] = (lane j's v[q]). Two butterfly steps
// on DPP quad_perm (0xB1 = lanes ^ 1, 0x4E = lanes ^ 2); every lane of the
// wave must be active.
__device__ __forceinline__ void dc_quad_transpose(unsigned (&v)[4], int q) {
  const bool b = q & 1, c = q & 2;
#pragma unroll
  for (int i = 0; i < 4; i += 2) {
    const unsigned send = b ? v[i] : v[i + 1];
    const unsigned recv = (unsigned)__builtin_amdgcn_update_dpp(
        0, (int)send, 0xB1, 0xF, 0xF, false);
    if (b) v[i] = recv;
    else v[i + 1] = recv;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const unsigned send = c ? v[i] : v[i + 2];
    const unsigned recv = (unsigned)__builtin_amdgcn_update_dpp(
        0, (int)send, 0x4E, 0xF, 0xF, false);
    if (c) v[i] = recv;
    else v[i + 2] = recv;
  }
}

// ---------------------------------------------------------------------------
// Weight prep for the forward: WP[8 classes][coutp][cinp] bf16, K (= ci)
// contiguous, from w[Cin][Cout][8]. coutp is a multiple of the block's Cout
// tile and cinp of the k-step; the padding is zero, so the forward has no row
// or k check on A.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void deconv3d_prep_w_kernel(
    const __bf16* __restrict__ w, __bf16* __restrict__ wp, int cin, int cout,
    int cinp, int coutp, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ci = idx % cinp;
  const int co = (idx / cinp) % coutp;
  const int cls = idx / (cinp * coutp);
  __bf16 v = (__bf16)0.f;
  if (ci < cin && co < cout) v = w[((int64_t)ci * cout + co) * 8 + cls];
  wp[idx] = v;
}

// ---------------------------------------------------------------------------
// Forward. A block owns DC_PT flat positions of one n and COT = 16*NCF
// output channels, for ALL 8 classes: GEMM rows are (class, co), columns are
// positions, D[row = co][col = s]. Wave v owns the two classes (pd, ph) =
// (v >> 1, v & 1), pw = 0 and 1, each NCF row fragments x 4 column
// fragments: a lane holds the pw = 0 and pw = 1 results of the same (co, s),
// which are the adjacent output elements 2w and 2w+1.
// x is staged once per block, DC_KST k-steps (128 ci) per barrier pair: a
// thread fetches the same 8 positions of 4 adjacent ci as 16-byte vectors
// and stores 8 interleaved 8-byte words. B fragments come from that tile
// (dc_off), A fragments are 16-byte reads of WP (L2-resident: 16 * Cout * Cin
// bytes).
// Store: the pair is one 32-bit word; with W % 4 == 0 a quad transposes its
// 4 (co) x 4 (s) words so that a lane holds 4 consecutive pairs of one co, 8
// consecutive output elements: one 16-byte store, 4 lanes a 64-byte run.
// Other W store the 32-bit pairs (always 4-byte aligned: rows are 2W long).
// ---------------------------------------------------------------------------
template <int NCF>
__global__ __launch_bounds__(256, 2) void deconv3d_fwd_kernel(
    const __bf16* __restrict__ x, const __bf16* __restrict__ wp,
    const float* __restrict__ bias, __bf16* __restrict__ y, DcDims dd,
    int coutp, int cinp, int ncot, int tiles_per_n, int xvec, int wide) {
  constexpr int COT = 16 * NCF;
  constexpr int NPF = DC_PT / 16;
  __shared__ __attribute__((aligned(16))) __bf16 sX[DC_KST * DC_PT * 32];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, kg = lane >> 4;
  // Cout tiles of one position tile are neighbours in launch order: where
  // Cout > COT the re-read of the x tile finds it in L2
  const int cot = blockIdx.x % ncot;
  const int tile = blockIdx.x / ncot;
  const int n = tile / tiles_per_n;
  const int s0 = (tile % tiles_per_n) * DC_PT;
  const int pd = wave >> 1, ph = wave & 1;
  const int kts = cinp / 32;

  f32x4 acc[2][NCF][NPF];
#pragma unroll
  for (int cf = 0; cf < NCF; ++cf) {
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (bias) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = cot * COT + cf * 16 + kg * 4 + r;
        if (co < dd.Cout) b[r] = bias[co];
      }
    }
#pragma unroll
    for (int pf = 0; pf < NPF; ++pf) acc[0][cf][pf] = acc[1][cf][pf] = b;
  }

  // A: lane (row = col, kg) reads 8 ci of its co, for pw = 0 and pw = 1
  const __bf16* wa = wp + ((int64_t)(wave * 2) * coutp + cot * COT + col) *
                              cinp + kg * 8;
  const int64_t wcls = (int64_t)coutp * cinp;

  const int sv = tid & 7;             // 8-position vector of the tile
  const int scg = tid >> 3;           // 4-ci group of the stage, 0..31
  const int sks = scg >> 3, scl = (scg & 7) * 4;
  const int64_t x_n = (int64_t)n * dd.Cin * dd.S;

  for (int kt0 = 0; kt0 < kts; kt0 += DC_KST) {
    if (kt0) __syncthreads();
    if (kt0 + sks < kts) {
      const int sp = s0 + sv * 8;
      __bf16 tv[4][8];
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const int ci = (kt0 + sks) * 32 + scl + cc;
#pragma unroll
        for (int j = 0; j < 8; ++j) tv[cc][j] = (__bf16)0.f;
        if (ci < dd.Cin) {
          const __bf16* src = x + x_n + (int64_t)ci * dd.S + sp;
          if (xvec && sp + 8 <= dd.S) {
            const bf16x8 vec = *reinterpret_cast<const bf16x8*>(src);
#pragma unroll
            for (int j = 0; j < 8; ++j) tv[cc][j] = vec[j];
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (sp + j < dd.S) tv[cc][j] = src[j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bf16x4 o = {tv[0][j], tv[1][j], tv[2][j], tv[3][j]};
        *reinterpret_cast<bf16x4*>(sX + sks * (DC_PT * 32) +
                                   dc_off(sv * 8 + j, scl >> 3) + (scl & 7)) =
            o;
      }
    }
    __syncthreads();

    const int nks = kts - kt0 < DC_KST ? kts - kt0 : DC_KST;
    for (int ks = 0; ks < nks; ++ks) {
      bf16x8 bfrag[NPF];
#pragma unroll
      for (int pf = 0; pf < NPF; ++pf)
        bfrag[pf] = *reinterpret_cast<const bf16x8*>(
            sX + ks * (DC_PT * 32) + dc_off(pf * 16 + col, kg));
      const __bf16* wk = wa + (kt0 + ks) * 32;
#pragma unroll
      for (int cf = 0; cf < NCF; ++cf) {
        const bf16x8 a0 =
            *reinterpret_cast<const bf16x8*>(wk + (int64_t)cf * 16 * cinp);
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(
            wk + (int64_t)cf * 16 * cinp + wcls);
#pragma unroll
        for (int pf = 0; pf < NPF; ++pf) {
          acc[0][cf][pf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a0, bfrag[pf], acc[0][cf][pf], 0, 0, 0);
          acc[1][cf][pf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a1, bfrag[pf], acc[1][cf][pf], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue ----------------------------------------------------------
  const int64_t hi_vol = (int64_t)8 * dd.S;  // one (n, co) output volume
  __bf16* y_n = y + (int64_t)n * dd.Cout * hi_vol;
  if (wide) {
    // W % 4 == 0: S % 4 == 0 too, so an aligned group of 4 positions is
    // inside the tensor as soon as its first position is, and in one row
    const int q = lane & 3;
#pragma unroll
    for (int pf = 0; pf < NPF; ++pf) {
      const int s4 = s0 + pf * 16 + (col & ~3);
      const int64_t off = s4 < dd.S ? dc_hi_off(dd, s4, pd, ph) : 0;
#pragma unroll
      for (int cf = 0; cf < NCF; ++cf) {
        unsigned v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          v[r] = dc_pack(acc[0][cf][pf][r], acc[1][cf][pf][r]);
        dc_quad_transpose(v, q);
        const int co = cot * COT + cf * 16 + kg * 4 + q;
        if (s4 < dd.S && co < dd.Cout) {
          const u32x4 o = {v[0], v[1], v[2], v[3]};
          *reinterpret_cast<u32x4*>(y_n + (int64_t)co * hi_vol + off) = o;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int pf = 0; pf < NPF; ++pf) {
    const int s = s0 + pf * 16 + col;
    if (s >= dd.S) continue;
    const int64_t off = dc_hi_off(dd, s, pd, ph);
#pragma unroll
    for (int cf = 0; cf < NCF; ++cf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = cot * COT + cf * 16 + kg * 4 + r;
        if (co < dd.Cout)
          *reinterpret_cast<unsigned*>(y_n + (int64_t)co * hi_vol + off) =
              dc_pack(acc[0][cf][pf][r], acc[1][cf][pf][r]);
      }
  }
}

// ---------------------------------------------------------------------------
// dgrad: per position a GEMM row over K = (co, p), 8*Cout long, against
// w[ci][(co, p)], which torch's layout already stores K-contiguous: B
// fragments are 16-byte reads of w itself (lane kg's 8 k are the 8 taps of
// co = 4*kt + kg), masked past Cout and Cin, and there is no weight prep.
// D[row = s][col = ci]: a lane ends with 4 consecutive s of one ci, an
// 8-byte store of dx.
// A block owns DC_PT flat positions of one n and CIT = 16*NCF input channels
// and stages go once, DC_KST k-steps (16 co) per barrier pair, as
// [k-step][position][co mod 4][8 p]: thread (co, pd, ph, 4 positions) loads
// the 8 consecutive elements (2w .. 2w+7) of high-res row (2d+pd, 2h+ph) as
// one 16-byte vector when W % 4 == 0, 4-byte pairs otherwise. The pair
// (pw = 0, 1) is adjacent in the row and adjacent in k, so it moves as one
// 32-bit word and nothing is de-interleaved.
// The 4 waves split the CIT columns first (each B fragment is then loaded by
// one wave only) and the 4 position fragments with what is left:
//   NCF 8, 4: 4 x 1 waves, 2 or 1 column fragments x 4 position fragments
//   NCF 2:    2 x 2 waves, 1 x 2        NCF 1: 1 x 4 waves, 1 x 1
// ---------------------------------------------------------------------------
template <int NCF>
__global__ __launch_bounds__(256, 2) void deconv3d_dgrad_kernel(
    const __bf16* __restrict__ go, const __bf16* __restrict__ w,
    __bf16* __restrict__ dx, DcDims dd, int ncit, int tiles_per_n, int gvec,
    int dvec) {
  constexpr int CIT = 16 * NCF;
  constexpr int WC = NCF < 4 ? NCF : 4;  // waves along ci
  constexpr int WM = 4 / WC;             // waves along positions
  constexpr int CPW = NCF / WC;          // column fragments per wave
  constexpr int MPW = (DC_PT / 16) / WM; // position fragments per wave
  __shared__ __attribute__((aligned(16))) __bf16 sG[DC_KST * DC_PT * 32];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, kg = lane >> 4;
  const int wc = wave % WC, wm = wave / WC;
  const int cit = blockIdx.x % ncit;
  const int tile = blockIdx.x / ncit;
  const int n = tile / tiles_per_n;
  const int s0 = (tile % tiles_per_n) * DC_PT;
  const int kts = (dd.Cout + 3) / 4;

  f32x4 acc[MPW][CPW];
#pragma unroll
  for (int i = 0; i < MPW; ++i)
#pragma unroll
    for (int j = 0; j < CPW; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // staging item: 4 positions x one (co mod 4, pd, ph)
  const int pg = tid & 15, dh = (tid >> 4) & 3, cq = tid >> 6;
  const int sp = s0 + pg * 4;
  const int64_t hi_vol = (int64_t)8 * dd.S;
  const __bf16* go_n = go + (int64_t)n * dd.Cout * hi_vol;
  int64_t goff[4];
  if (gvec) {
    goff[0] = sp < dd.S ? dc_hi_off(dd, sp, dh >> 1, dh & 1) : -1;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      goff[j] = sp + j < dd.S ? dc_hi_off(dd, sp + j, dh >> 1, dh & 1) : -1;
  }

  for (int kt0 = 0; kt0 < kts; kt0 += DC_KST) {
    if (kt0) __syncthreads();
    const int nks = kts - kt0 < DC_KST ? kts - kt0 : DC_KST;
#pragma unroll
    for (int ks = 0; ks < DC_KST; ++ks) {
      if (ks >= nks) break;
      const int co = (kt0 + ks) * 4 + cq;
      const __bf16* src = go_n + (int64_t)co * hi_vol;
      bf16x2 pr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) pr[j] = {(__bf16)0.f, (__bf16)0.f};
      if (co < dd.Cout) {
        if (gvec) {
          if (goff[0] >= 0) {
            const bf16x8 vec =
                *reinterpret_cast<const bf16x8*>(src + goff[0]);
#pragma unroll
            for (int j = 0; j < 4; ++j) pr[j] = {vec[2 * j], vec[2 * j + 1]};
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (goff[j] >= 0)
              pr[j] = *reinterpret_cast<const bf16x2*>(src + goff[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *reinterpret_cast<bf16x2*>(sG + ks * (DC_PT * 32) +
                                   dc_off(pg * 4 + j, cq) + dh * 2) = pr[j];
    }
    __syncthreads();

    for (int ks = 0; ks < nks; ++ks) {
      bf16x8 afrag[MPW];
#pragma unroll
      for (int i = 0; i < MPW; ++i)
        afrag[i] = *reinterpret_cast<const bf16x8*>(
            sG + ks * (DC_PT * 32) + dc_off((wm * MPW + i) * 16 + col, kg));
      const int co = (kt0 + ks) * 4 + kg;
#pragma unroll
      for (int j = 0; j < CPW; ++j) {
        const int ci = cit * CIT + (wc * CPW + j) * 16 + col;
        bf16x8 bfrag;
#pragma unroll
        for (int e = 0; e < 8; ++e) bfrag[e] = (__bf16)0.f;
        if (ci < dd.Cin && co < dd.Cout)
          bfrag = *reinterpret_cast<const bf16x8*>(
              w + ((int64_t)ci * dd.Cout + co) * 8);
#pragma unroll
        for (int i = 0; i < MPW; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[i], bfrag, acc[i][j], 0, 0, 0);
      }
    }
  }

  __bf16* dx_n = dx + (int64_t)n * dd.Cin * dd.S;
#pragma unroll
  for (int j = 0; j < CPW; ++j) {
    const int ci = cit * CIT + (wc * CPW + j) * 16 + col;
    if (ci >= dd.Cin) continue;
#pragma unroll
    for (int i = 0; i < MPW; ++i) {
      const int s = s0 + (wm * MPW + i) * 16 + kg * 4;
      __bf16* dst = dx_n + (int64_t)ci * dd.S + s;
      if (dvec) {  // S % 4 == 0: s < S puts all 4 inside
        if (s < dd.S) {
          const bf16x4 o = {(__bf16)acc[i][j][0], (__bf16)acc[i][j][1],
                            (__bf16)acc[i][j][2], (__bf16)acc[i][j][3]};
          *reinterpret_cast<bf16x4*>(dst) = o;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (s + r < dd.S) dst[r] = (__bf16)acc[i][j][r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad: M = Cin, N = (co, p), K = (n, s). A block owns 64 ci x 16 co (128
// columns) and a contiguous range of position tiles (split-K over batch and
// depth), keeps its 64 x 128 fp32 tile in registers (8 fragments per wave:
// 4 ci fragments x the wave's 2 column fragments) and stores it into its
// range's slice of part[ranges][Cin][Cout][8]: lane col runs along (co, p),
// so one store of a 16-lane group is one 64-byte run. The slices are added
// by deconv3d_wgrad_fold_kernel (see deconv3d_wgrad for the choice).
// Both operands want 8 consecutive s per lane. x has them in memory; go has
// them at stride 2 in three axes, so its tile is staged ONCE for all 8
// classes as [column (co, p)][64 s]: a thread loads 8 consecutive elements of
// a high-res row (4 positions x pw), splits even and odd elements and stores
// two 8-byte words, to columns (co, pd, ph, 0) and (co, pd, ph, 1). x is
// staged [ci][64 s] with 16-byte vectors.
// Row pitch 72 elements = 36 banks: the 16 rows of a ds_read_b128 group
// start at 36*r mod 64 = {0, 36, 8, 44, ...}, 16 distinct multiples of 4, so
// the 16 x 4 banks of the group are the 64 banks once.
// ---------------------------------------------------------------------------
constexpr int DW_PITCH = 72;
constexpr int DW_CIT = 64;
constexpr int DW_COT = 16;

__global__ __launch_bounds__(256, 2) void deconv3d_wgrad_kernel(
    const __bf16* __restrict__ x, const __bf16* __restrict__ go,
    float* __restrict__ part, DcDims dd, int tiles_per_n, int total_tiles,
    int tiles_per_block, int xvec, int gvec) {
  __shared__ __attribute__((aligned(16))) __bf16 sXw[DW_CIT * DW_PITCH];
  __shared__ __attribute__((aligned(16))) __bf16 sGw[DW_COT * 8 * DW_PITCH];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, kg = lane >> 4;
  const int cit = blockIdx.x, cot = blockIdx.y;
  const int t0 = blockIdx.z * tiles_per_block;
  const int t1 = t0 + tiles_per_block < total_tiles ? t0 + tiles_per_block
                                                    : total_tiles;
  const int64_t hi_vol = (int64_t)8 * dd.S;

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  for (int t = t0; t < t1; ++t) {
    const int n = t / tiles_per_n;
    const int s0 = (t % tiles_per_n) * DC_PT;
    if (t != t0) __syncthreads();
    // x: 64 ci x 8 vectors of 8 positions
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int it = tid + u * 256;
      const int v = it & 7, cl = it >> 3;
      const int ci = cit * DW_CIT + cl;
      const int sp = s0 + v * 8;
      bf16x8 val;
#pragma unroll
      for (int j = 0; j < 8; ++j) val[j] = (__bf16)0.f;
      if (ci < dd.Cin) {
        const __bf16* src = x + ((int64_t)n * dd.Cin + ci) * dd.S + sp;
        if (xvec && sp + 8 <= dd.S) {
          val = *reinterpret_cast<const bf16x8*>(src);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (sp + j < dd.S) val[j] = src[j];
        }
      }
      *reinterpret_cast<bf16x8*>(sXw + cl * DW_PITCH + v * 8) = val;
    }
    // go: 16 co x 4 (pd, ph) x 16 groups of 4 positions
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = tid + u * 256;
      const int pg = it & 15, dh = (it >> 4) & 3, cl = it >> 6;
      const int co = cot * DW_COT + cl;
      const int sp = s0 + pg * 4;
      bf16x4 ev, od;
#pragma unroll
      for (int j = 0; j < 4; ++j) ev[j] = od[j] = (__bf16)0.f;
      if (co < dd.Cout) {
        const __bf16* src = go + ((int64_t)n * dd.Cout + co) * hi_vol;
        if (gvec) {
          if (sp < dd.S) {
            const bf16x8 vec = *reinterpret_cast<const bf16x8*>(
                src + dc_hi_off(dd, sp, dh >> 1, dh & 1));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              ev[j] = vec[2 * j];
              od[j] = vec[2 * j + 1];
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (sp + j < dd.S) {
              const bf16x2 pr = *reinterpret_cast<const bf16x2*>(
                  src + dc_hi_off(dd, sp + j, dh >> 1, dh & 1));
              ev[j] = pr[0];
              od[j] = pr[1];
            }
        }
      }
      __bf16* dst = sGw + (cl * 8 + dh * 2) * DW_PITCH + pg * 4;
      *reinterpret_cast<bf16x4*>(dst) = ev;
      *reinterpret_cast<bf16x4*>(dst + DW_PITCH) = od;
    }
    __syncthreads();

#pragma unroll
    for (int ks = 0; ks < DC_PT / 32; ++ks) {
      bf16x8 afrag[4], bfrag[2];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        afrag[i] = *reinterpret_cast<const bf16x8*>(
            sXw + (i * 16 + col) * DW_PITCH + ks * 32 + kg * 8);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        bfrag[j] = *reinterpret_cast<const bf16x8*>(
            sGw + ((wave * 2 + j) * 16 + col) * DW_PITCH + ks * 32 + kg * 8);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[i], bfrag[j], acc[i][j], 0, 0, 0);
    }
  }

  // column (wave*2 + j)*16 + col of the tile is (co, p) = (.. >> 3, .. & 7);
  // plain stores into this range's slice: 16 lanes a 64-byte run
  float* slice = part + (int64_t)blockIdx.z * dd.Cin * dd.Cout * 8;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int cc = (wave * 2 + j) * 16 + col;
    const int co = cot * DW_COT + (cc >> 3);
    if (co >= dd.Cout) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ci = cit * DW_CIT + i * 16 + kg * 4 + r;
        if (ci < dd.Cin)
          slice[((int64_t)ci * dd.Cout + co) * 8 + (cc & 7)] = acc[i][j][r];
      }
  }
}

// dw[i] = sum over the nz slices of part[z][i], one thread per element,
// slices added in order (deterministic). The only fp32 VALU arithmetic of the
// file: the attribute keeps its adds plain v_add_f32.
#if defined(__HIP_DEVICE_COMPILE__)
#define DC_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define DC_NO_PK_F32
#endif
__global__ DC_NO_PK_F32 __launch_bounds__(256) void deconv3d_wgrad_fold_kernel(
    const float* __restrict__ part, float* __restrict__ dw, int total,
    int nz) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  float sum = 0.f;
#pragma unroll 8
  for (int z = 0; z < nz; ++z) sum += part[(int64_t)z * total + idx];
  dw[idx] = sum;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

// bf16, contiguous, and 16-byte aligned (a contiguous view may start
// anywhere in its storage): the kernels' vector and pair accesses assume it
static torch::Tensor dc_operand(const torch::Tensor& t) {
  auto c = t.to(torch::kBFloat16).contiguous();
  if (reinterpret_cast<uintptr_t>(c.data_ptr()) % 16 != 0) c = c.clone();
  return c;
}

static DcDims dc_dims(int64_t N, int64_t Cin, int64_t Cout, int64_t D,
                      int64_t H, int64_t W) {
  TORCH_CHECK(N >= 1 && Cin >= 1 && Cout >= 1 && D >= 1 && H >= 1 && W >= 1,
              "deconv3d: empty dimension");
  TORCH_CHECK(D * H * W < ((int64_t)1 << 28), "deconv3d: volume too large");
  DcDims dd;
  dd.N = (int)N, dd.Cin = (int)Cin, dd.Cout = (int)Cout;
  dd.D = (int)D, dd.H = (int)H, dd.W = (int)W;
  dd.S = (int)(D * H * W);
  return dd;
}

static void dc_check_w(const torch::Tensor& w, const char* who) {
  TORCH_CHECK(w.dim() == 5 && w.size(2) == 2 && w.size(3) == 2 &&
              w.size(4) == 2, who, ": w[Cin,Cout,2,2,2]");
}

// The forward block covers COT = 16, 32 or 64 output channels, the smallest
// that holds Cout: up to Cout 64 (every decoder of the models here) x is read
// from HBM exactly once. 64 is the cap because the 8 classes of 64 channels
// x 64 positions are 128 accumulator registers per lane; wider layers run
// ceil(Cout / 64) blocks per position tile, neighbours in launch order.
torch::Tensor deconv3d_fwd(torch::Tensor x, torch::Tensor w,
                           c10::optional<torch::Tensor> bias) {
  CHECK_GPU(x);
  CHECK_GPU(w);
  dc_check_w(w, "deconv3d_fwd");
  TORCH_CHECK(x.dim() == 5 && x.size(1) == w.size(0),
              "deconv3d_fwd: x[N,Cin,D,H,W], w[Cin,Cout,2,2,2]");
  auto xc = dc_operand(x);
  auto wc = dc_operand(w);
  const DcDims dd = dc_dims(xc.size(0), xc.size(1), wc.size(1), xc.size(2),
                            xc.size(3), xc.size(4));
  auto y = torch::empty({dd.N, dd.Cout, 2 * dd.D, 2 * dd.H, 2 * dd.W},
                        xc.options());
  const float* bp = nullptr;
  torch::Tensor bc;
  if (bias.has_value() && bias->defined() && bias->numel() > 0) {
    CHECK_GPU(*bias);
    TORCH_CHECK(bias->numel() == dd.Cout, "deconv3d_fwd: bias[Cout]");
    bc = bias->to(torch::kFloat32).contiguous();
    bp = bc.data_ptr<float>();
  }

  const int ncf = dd.Cout <= 16 ? 1 : (dd.Cout <= 32 ? 2 : 4);
  const int cot = 16 * ncf;
  const int ncot = (dd.Cout + cot - 1) / cot;
  const int coutp = ncot * cot;
  const int cinp = (dd.Cin + 31) / 32 * 32;
  const int64_t wp_total = (int64_t)8 * coutp * cinp;
  TORCH_CHECK(wp_total < (int64_t)1 << 31, "deconv3d_fwd: weight too large");
  auto wpt = torch::empty({wp_total}, wc.options());
  auto s = current_stream();
  hipLaunchKernelGGL(deconv3d_prep_w_kernel,
                     dim3((unsigned)((wp_total + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const __bf16*>(wc.data_ptr()),
                     reinterpret_cast<__bf16*>(wpt.data_ptr()), dd.Cin,
                     dd.Cout, cinp, coutp, (int)wp_total);

  const int tiles_per_n = (dd.S + DC_PT - 1) / DC_PT;
  const int64_t nblk = (int64_t)dd.N * tiles_per_n * ncot;
  TORCH_CHECK(nblk < (int64_t)1 << 31, "deconv3d_fwd: grid too large");
  const int xvec = dd.S % 8 == 0;
  const int wide = dd.W % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(y.data_ptr()) % 16 == 0;
  auto L = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(256), 0, s,
                       reinterpret_cast<const __bf16*>(xc.data_ptr()),
                       reinterpret_cast<const __bf16*>(wpt.data_ptr()), bp,
                       reinterpret_cast<__bf16*>(y.data_ptr()), dd, coutp,
                       cinp, ncot, tiles_per_n, xvec, wide);
  };
  if (ncf == 1) L(deconv3d_fwd_kernel<1>);
  else if (ncf == 2) L(deconv3d_fwd_kernel<2>);
  else L(deconv3d_fwd_kernel<4>);
  return y;
}

// The dgrad block covers CIT = 16 .. 128 input channels, the smallest that
// holds Cin: up to Cin 128 go is read from HBM exactly once.
torch::Tensor deconv3d_dgrad(torch::Tensor go, torch::Tensor w,
                             std::vector<int64_t> in_shape) {
  CHECK_GPU(go);
  CHECK_GPU(w);
  dc_check_w(w, "deconv3d_dgrad");
  TORCH_CHECK(in_shape.size() == 5 && go.dim() == 5 &&
              in_shape[1] == w.size(0) && go.size(0) == in_shape[0] &&
              go.size(1) == w.size(1) && go.size(2) == 2 * in_shape[2] &&
              go.size(3) == 2 * in_shape[3] && go.size(4) == 2 * in_shape[4],
              "deconv3d_dgrad: go[N,Cout,2D,2H,2W] against in_shape");
  auto gc = dc_operand(go);
  auto wc = dc_operand(w);
  const DcDims dd = dc_dims(in_shape[0], in_shape[1], wc.size(1), in_shape[2],
                            in_shape[3], in_shape[4]);
  auto dx = torch::empty({dd.N, dd.Cin, dd.D, dd.H, dd.W}, gc.options());

  const int ncf = dd.Cin <= 16 ? 1 : (dd.Cin <= 32 ? 2 : (dd.Cin <= 64 ? 4 : 8));
  const int ncit = (dd.Cin + 16 * ncf - 1) / (16 * ncf);
  const int tiles_per_n = (dd.S + DC_PT - 1) / DC_PT;
  const int64_t nblk = (int64_t)dd.N * tiles_per_n * ncit;
  TORCH_CHECK(nblk < (int64_t)1 << 31, "deconv3d_dgrad: grid too large");
  const int gvec = dd.W % 4 == 0;
  const int dvec = dd.S % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(dx.data_ptr()) % 8 == 0;
  auto L = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(256), 0,
                       current_stream(),
                       reinterpret_cast<const __bf16*>(gc.data_ptr()),
                       reinterpret_cast<const __bf16*>(wc.data_ptr()),
                       reinterpret_cast<__bf16*>(dx.data_ptr()), dd, ncit,
                       tiles_per_n, gvec, dvec);
  };
  if (ncf == 1) L(deconv3d_dgrad_kernel<1>);
  else if (ncf == 2) L(deconv3d_dgrad_kernel<2>);
  else if (ncf == 4) L(deconv3d_dgrad_kernel<4>);
  else L(deconv3d_dgrad_kernel<8>);
  return dx;
}

// Split-K: position tiles are dealt out in contiguous ranges so that the
// launch has about 1024 blocks (4 per CU), a range at least 4 tiles and at
// most 256 ranges. Each range owns a slice of part[nz][Cin][Cout][8] and
// writes every element of it with plain stores (no zero fill);
// deconv3d_wgrad_fold_kernel adds the slices in order, so dw is
// deterministic. An fp32-atomic fold into a zeroed dw measured the same
// (docs/KERNELS.md K1g); the slices cost nz * Cin * Cout * 32 bytes written
// and read once.
torch::Tensor deconv3d_wgrad(torch::Tensor x, torch::Tensor go) {
  CHECK_GPU(x);
  CHECK_GPU(go);
  TORCH_CHECK(x.dim() == 5 && go.dim() == 5 && go.size(0) == x.size(0) &&
              go.size(2) == 2 * x.size(2) && go.size(3) == 2 * x.size(3) &&
              go.size(4) == 2 * x.size(4),
              "deconv3d_wgrad: x[N,Cin,D,H,W], go[N,Cout,2D,2H,2W]");
  auto xc = dc_operand(x);
  auto gc = dc_operand(go);
  const DcDims dd = dc_dims(xc.size(0), xc.size(1), gc.size(1), xc.size(2),
                            xc.size(3), xc.size(4));
  auto dw = torch::empty({dd.Cin, dd.Cout, 2, 2, 2},
                         xc.options().dtype(torch::kFloat32));

  const int tiles_per_n = (dd.S + DC_PT - 1) / DC_PT;
  const int64_t total_tiles = (int64_t)dd.N * tiles_per_n;
  TORCH_CHECK(total_tiles < (int64_t)1 << 31, "deconv3d_wgrad: too large");
  const int ncit = (dd.Cin + DW_CIT - 1) / DW_CIT;
  const int ncot = (dd.Cout + DW_COT - 1) / DW_COT;
  int64_t tpb = (total_tiles * ncit * ncot + 1023) / 1024;
  if (tpb < 4) tpb = 4;
  if (tpb < (total_tiles + 255) / 256) tpb = (total_tiles + 255) / 256;
  const int64_t nz = (total_tiles + tpb - 1) / tpb;
  const int64_t dw_total = (int64_t)dd.Cin * dd.Cout * 8;
  TORCH_CHECK(ncot < 65536 && dw_total < (int64_t)1 << 31,
              "deconv3d_wgrad: too large");
  auto part = torch::empty({nz, dw_total}, dw.options());
  auto s = current_stream();
  const int xvec = dd.S % 8 == 0;
  const int gvec = dd.W % 4 == 0;
  hipLaunchKernelGGL(deconv3d_wgrad_kernel,
                     dim3((unsigned)ncit, (unsigned)ncot, (unsigned)nz),
                     dim3(256), 0, s,
                     reinterpret_cast<const __bf16*>(xc.data_ptr()),
                     reinterpret_cast<const __bf16*>(gc.data_ptr()),
                     part.data_ptr<float>(), dd, tiles_per_n,
                     (int)total_tiles, (int)tpb, xvec, gvec);
  hipLaunchKernelGGL(deconv3d_wgrad_fold_kernel,
                     dim3((unsigned)((dw_total + 255) / 256)), dim3(256), 0, s,
                     part.data_ptr<float>(), dw.data_ptr<float>(),
                     (int)dw_total, (int)nz);
  return dw;
}
