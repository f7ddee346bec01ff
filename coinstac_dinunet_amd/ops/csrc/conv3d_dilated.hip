// Dilated 3x3x3 conv3d (stride 1, isotropic dilation d in [2, 16], padding d):
// forward, dgrad and wgrad on a SUB-LATTICE slab; d is a runtime argument.
//
// A dense slab for dilation d would need a halo of d on every axis. Instead
// a block works inside one residue class of the h axis: for a fixed rh in
// [0, d) the rows ih = rh + d*j form a lattice on which the conv is a dense
// 3-tap conv in j. The depth axis needs no classes at one output plane per
// block: the three tap planes are od - d, od, od + d. Along w the rows stay
// contiguous (16-byte global loads) and the dilation is a wave-uniform column
// shift kw*d inside a row that carries d halo columns on each side.
//
// Forward / dgrad (conv3d_dil_kernel): out tile = 4 lattice rows x 32 columns
// (128 m) x NCOLT (32 or 64) output channels; wave w owns lattice row w, two
// 16-column m-fragments. Slab [3][6][32 + 2d][CTILE] bf16, channel-innermost,
// in dynamic LDS: CTILE 32 for d <= 8 (41.5 / 46 / 55.3 KB at d = 2 / 4 / 8),
// CTILE 16 for d > 8 or KCH <= 16 (36.9 KB at d = 16). K inside a channel
// tile runs (tap, local channel), so the A fragment of a tap is one 16-byte
// LDS read at (plane kd, row w + kh, column m + kw*d). B fragments are
// 16-byte global loads from the prepared weight matrix of the dense spatial
// kernels (same layout: WB[ncol][kts][KT_PAD], dgrad tap-flipped and
// transposed), loaded one k-step ahead. With stride 1 and pad == d the dgrad
// IS this conv of go with the flipped weights: dx is written once.
// LDS swizzle (CTILE 32: 16-byte chunk ^= 2*bit2(column)) is a function of
// the slab column, applied on store and load alike. A 16-lane read group
// covers 16 CONSECUTIVE columns whatever the shift kw*d is, and any 8
// consecutive columns take every (column mod 4, bit 2) pair once, so the
// conflict-free property of the dense layout does not depend on d. CTILE 16
// (32 B per column) covers all 64 banks with 8 consecutive columns.
//
// Wgrad (conv3d_dil_wgrad_kernel): tap reuse in the manner of
// conv3d_wgrad_s1_kernel. A block owns (32 co, 16 ci); per chunk it stages
// the x slab [16 ci][3][6][32 + 2*ceil8(d)] position-innermost and the go
// tile [32 co][128 m] once; per 32-m sub-chunk one go fragment feeds 27 MFMAs
// whose x fragments read the slab at (plane, row, kw*d column) offsets. Waves
// are 2 (co halves) x 2 (m halves); the 27 accumulators stay in registers
// over the grid-stride chunk loop and every (block z, m half) stores its own
// fp32 slice, summed on the host side: no atomics, no zero fill.
#include "common.h"

#include <hip/hip_bf16.h>

#include <algorithm>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int DIL_OWT = 32;          // output columns per tile
constexpr int DIL_OHT = 4;           // lattice rows per tile (one per wave)
constexpr int DIL_H2 = DIL_OHT + 2;  // staged lattice rows

struct DilDims {
  int N, KCH;       // input-side channels (fwd: Cin; dgrad: Cout)
  int D, H, W;      // spatial size (input == output)
  int NCOL;         // output-side channels
  int d;            // dilation
  int Kpad;         // row length of WB
  int hcls;         // h residue classes: min(d, H)
  int jtiles;       // row tiles per class: ceil(ceil(H / d) / OHT)
  int wtiles;       // column tiles
};

// chunk index -> (n, od, rh, j0, ow0)
struct DilChunk { int n, od, rh, j0, ow0; };
__device__ inline DilChunk dil_chunk(int64_t t, const DilDims& dd) {
  DilChunk c;
  c.ow0 = (int)(t % dd.wtiles) * DIL_OWT;
  t /= dd.wtiles;
  c.j0 = (int)(t % dd.jtiles) * DIL_OHT;
  t /= dd.jtiles;
  c.rh = (int)(t % dd.hcls);
  t /= dd.hcls;
  c.od = (int)(t % dd.D);
  c.n = (int)(t / dd.D);
  return c;
}

// 8 elements of row `src` from column iw: one 16-byte load when the row is
// 16-byte aligned and the vector lies inside it, guarded elements otherwise
// (columns outside [0, W) are padding)
__device__ inline bf16x8 dil_load8(const __bf16* __restrict__ src, int iw,
                                   int W, bool wvec) {
  if (wvec && iw >= 0 && iw + 8 <= W)
    return *reinterpret_cast<const bf16x8*>(src + iw);
  bf16x8 v = bf16x8{};
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if ((unsigned)(iw + j) < (unsigned)W) v[j] = src[iw + j];
  return v;
}

template <int CTILE, int NCOLT>
__global__ __launch_bounds__(256) void conv3d_dil_kernel(
    const __bf16* __restrict__ in, const __bf16* __restrict__ wb,
    __bf16* __restrict__ out, DilDims dd) {
  constexpr int OWT = DIL_OWT, H2 = DIL_H2;
  constexpr int KT_PAD = ((CTILE * 27 + 31) / 32) * 32;
  constexpr int KS = KT_PAD / 32;
  constexpr int NCF = NCOLT / 16;
  constexpr int NCG = CTILE / 8;
  static_assert(CTILE == 32 || CTILE == 16, "channel tiles: 32 or 16");
  extern __shared__ __attribute__((aligned(16))) __bf16 sXd[];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int row = lane & 15, kg = lane >> 4;
  const int d = dd.d;
  const int W2 = OWT + 2 * d;
  const int ncol0 = blockIdx.y * NCOLT;
  const DilChunk ck = dil_chunk(blockIdx.x, dd);
  // a short residue class has no rows in its last tiles
  if (ck.rh + (int64_t)d * ck.j0 >= dd.H) return;

  auto slab_off = [W2](int a, int h, int c, int cl) -> int {
    int chunk = cl >> 3;
    if (CTILE == 32) chunk ^= ((c >> 2) & 1) << 1;
    return ((a * H2 + h) * W2 + c) * CTILE + chunk * 8 + (cl & 7);
  };
  // A address = lanew[kw][i] + (kd, kh) row constant: the swizzle bits
  // depend on the column only
  int lanew[3][2];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      lanew[kw][i] = slab_off(0, wave, i * 16 + row + kw * d,
                              (CTILE == 32 ? kg : (kg & 1)) * 8);
  const int rowp = W2 * CTILE;  // elements per slab row

  f32x4 acc[2][NCF];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NCF; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // WB has zero rows up to the next multiple of 128 columns: a ragged
  // column tile reads in bounds without a check
  const __bf16* wbl = wb + (int64_t)(ncol0 + row) * dd.Kpad + kg * 8;
  auto bload = [&](int j, int g) -> bf16x8 {
    return *reinterpret_cast<const bf16x8*>(
        wbl + (int64_t)j * 16 * dd.Kpad + (int64_t)g * 32);
  };
  bf16x8 bcur[NCF];
#pragma unroll
  for (int j = 0; j < NCF; ++j) bcur[j] = bload(j, 0);

  // staging runs over 16-byte-aligned global vectors: vector v starts at
  // iw = ow0 - ceil8(d) + 8v, slab column 8v - coff
  const int d8 = (d + 7) & ~7;
  const int coff = d8 - d;
  const int NV = (W2 + coff + 7) >> 3;
  const int nitem = 3 * H2 * NV * NCG;
  const bool wvec = (dd.W & 7) == 0;
  const int64_t HW = (int64_t)dd.H * dd.W;
  const int64_t in_n = (int64_t)ck.n * dd.KCH * dd.D * HW;
  const int kts = (dd.KCH + CTILE - 1) / CTILE;

  for (int kt = 0; kt < kts; ++kt) {
    if (kt) __syncthreads();
    // every slab element is stored each tile; rows, columns and channels
    // outside the tensor store zeros (the padding the off-centre taps read)
    for (int it = tid; it < nitem; it += 256) {
      const int cg = it % NCG;
      const int r = it / NCG;
      const int v = r % NV;
      const int hr = (r / NV) % H2;
      const int a = r / (NV * H2);
      const int id = ck.od + (a - 1) * d;
      const int ih = ck.rh + d * (ck.j0 - 1 + hr);
      const int iw = ck.ow0 - d8 + v * 8;
      const bool row_ok = (unsigned)id < (unsigned)dd.D &&
                          (unsigned)ih < (unsigned)dd.H;
      bf16x8 t[8];
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) {
        const int ch = kt * CTILE + cg * 8 + cc;
        t[cc] = bf16x8{};
        if (row_ok && ch < dd.KCH)
          t[cc] = dil_load8(in + in_n + ((int64_t)ch * dd.D + id) * HW +
                                (int64_t)ih * dd.W,
                            iw, dd.W, wvec);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = v * 8 + j - coff;
        if ((unsigned)c < (unsigned)W2) {
          bf16x8 o;
#pragma unroll
          for (int cc = 0; cc < 8; ++cc) o[cc] = t[cc][j];
          *reinterpret_cast<bf16x8*>(sXd + slab_off(a, hr, c, cg * 8)) = o;
        }
      }
    }
    __syncthreads();

    // ---- k-steps of 32: one tap x 32 channels, or two taps x 16 ---------
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bool more = ks + 1 < KS || kt + 1 < kts;
      bf16x8 bnext[NCF];
      if (more) {
#pragma unroll
        for (int j = 0; j < NCF; ++j) bnext[j] = bload(j, kt * KS + ks + 1);
      }
      bf16x8 afrag[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        int lk;
        if (CTILE == 32) {
          lk = lanew[ks % 3][i] + ((ks / 9) * H2 + (ks / 3) % 3) * rowp;
        } else {
          // taps 2ks (kg 0,1) and 2ks+1 (kg 2,3); the 28th tap has zero
          // weights and re-reads the 27th
          const int t0 = 2 * ks, t1 = 2 * ks + 1 < 27 ? 2 * ks + 1 : 26;
          const int l0 =
              lanew[t0 % 3][i] + ((t0 / 9) * H2 + (t0 / 3) % 3) * rowp;
          const int l1 =
              lanew[t1 % 3][i] + ((t1 / 9) * H2 + (t1 / 3) % 3) * rowp;
          lk = (kg >> 1) ? l1 : l0;
        }
        afrag[i] = *reinterpret_cast<const bf16x8*>(sXd + lk);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NCF; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[i], bcur[j], acc[i][j], 0, 0, 0);
      if (more) {
#pragma unroll
        for (int j = 0; j < NCF; ++j) bcur[j] = bnext[j];
      }
    }
  }

  // ---- epilogue: wave = lattice row, a lane's 4 m are 4 adjacent columns -
  const int oh = ck.rh + d * (ck.j0 + wave);
  if (oh >= dd.H) return;
  const bool pack4 = (dd.W & 3) == 0;
  const int64_t out_n = (int64_t)ck.n * dd.NCOL * dd.D * HW;
  const int ccol = lane & 15;
  const int crow0 = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ow = ck.ow0 + i * 16 + crow0;
#pragma unroll
    for (int j = 0; j < NCF; ++j) {
      const int col = ncol0 + j * 16 + ccol;
      if (col >= dd.NCOL) continue;
      __bf16* dst = out + out_n + ((int64_t)col * dd.D + ck.od) * HW +
                    (int64_t)oh * dd.W + ow;
      if (pack4) {
        if (ow < dd.W) {  // ow % 4 == 0 and W % 4 == 0: ow + 3 < W too
          bf16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (__bf16)acc[i][j][r];
          *reinterpret_cast<bf16x4*>(dst) = o;
        }
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (ow + r < dd.W) dst[r] = (__bf16)acc[i][j][r];
    }
  }
}

// WB of the dense spatial kernels: [rows = NCOL up to a multiple of 128]
// [kts][KT_PAD], k inside a channel tile = tap*CTILE + local channel; taps
// >= 27, channels >= KCH and rows >= NCOL are zero. Forward reads
// w[col][ch][tap], dgrad (KCH = Cout, NCOL = Cin) w[ch][col][26 - tap].
__global__ __launch_bounds__(256) void conv3d_dil_prep_wb_kernel(
    const __bf16* __restrict__ w, __bf16* __restrict__ wb, int ncol, int kch,
    int ctile, int kt_pad, int kpad, int dgrad) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= (ncol + 127) / 128 * 128 * kpad) return;
  const int col = idx / kpad, k = idx - col * kpad;
  const int kt = k / kt_pad, kk = k - kt * kt_pad;
  const int tap = kk / ctile, ch = kt * ctile + kk % ctile;
  __bf16 v = (__bf16)0.f;
  if (tap < 27 && ch < kch && col < ncol)
    v = dgrad ? w[((int64_t)ch * ncol + col) * 27 + 26 - tap]
              : w[((int64_t)col * kch + ch) * 27 + tap];
  wb[idx] = v;
}

// x fragment: 8 consecutive positions of one slab row. ALIGN is what the
// column shift (kw - 1)*d leaves of the 16-byte alignment of the tile:
// 8 -> one 16-byte read, 4 -> two 8-byte reads, 1 -> eight 2-byte reads.
template <int ALIGN>
__device__ inline bf16x8 dil_xfrag(const __bf16* src) {
  if constexpr (ALIGN == 8) {
    return *reinterpret_cast<const bf16x8*>(src);
  } else if constexpr (ALIGN == 4) {
    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(src);
    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(src + 4);
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  } else {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[j];
    return v;
  }
}

constexpr int DILW_CT = 16;    // ci per block
constexpr int DILW_COT = 32;   // co per block
constexpr int DILW_CHUNK = DIL_OWT * DIL_OHT;
constexpr int DILW_GOP = DILW_CHUNK + 8;  // go row pitch: 272 B, 16 mod 256

// x slab geometry for dilation d: row pitch (elements) and channel stride.
// The stride is 8 mod 128 elements (16 B mod 256 B): the 16 ci rows of a
// fragment read 16 distinct 16-byte bank groups.
static inline int dilw_pitch(int d) { return DIL_OWT + 2 * ((d + 7) & ~7); }
static inline int dilw_chs(int d) {
  return (3 * DIL_H2 * dilw_pitch(d) + 127) / 128 * 128 + 8;
}

// part[2 * zstride][27][Cout][Cin] fp32; dd.KCH = Cin, dd.NCOL = Cout
template <int ALIGN>
__global__ __launch_bounds__(256) void conv3d_dil_wgrad_kernel(
    const __bf16* __restrict__ x, const __bf16* __restrict__ go,
    float* __restrict__ part, DilDims dd, int64_t nchunks, int pitch,
    int chs) {
  constexpr int OWT = DIL_OWT, OHT = DIL_OHT, H2 = DIL_H2;
  constexpr int CT = DILW_CT, COT = DILW_COT, GOP = DILW_GOP;
  extern __shared__ __attribute__((aligned(16))) __bf16 sWd[];
  __bf16* sGo = sWd;              // [COT][GOP]
  __bf16* sX = sWd + COT * GOP;   // [CT] x chs: [3][H2][pitch]

  const int co0 = blockIdx.x * COT;
  const int ci0 = blockIdx.y * CT;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wi = wave & 1;   // co half
  const int wm = wave >> 1;  // m half: sub-chunks (lattice rows) 2wm, 2wm+1
  const int row = lane & 15, kg = lane >> 4;
  const int d = dd.d;
  const int d8 = (d + 7) & ~7;
  const int NVP = pitch >> 3;
  const bool wvec = (dd.W & 7) == 0;
  const int64_t HW = (int64_t)dd.H * dd.W;

  f32x4 acc[27];
#pragma unroll
  for (int t = 0; t < 27; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};

  for (int64_t z = blockIdx.z; z < nchunks; z += gridDim.z) {
    const DilChunk ck = dil_chunk(z, dd);
    if (ck.rh + (int64_t)d * ck.j0 >= dd.H) continue;  // block-uniform

    // ---- x slab: slab column c is iw = ow0 - ceil8(d) + c, so 16-byte
    // global vectors land on 16-byte LDS words; every word is written ------
    const __bf16* xn = x + (int64_t)ck.n * dd.KCH * dd.D * HW;
    for (int it = tid; it < CT * 3 * H2 * NVP; it += 256) {
      const int v = it % NVP;
      const int r = it / NVP;
      const int hr = r % H2;
      const int a = (r / H2) % 3;
      const int ci = r / (3 * H2);
      const int id = ck.od + (a - 1) * d;
      const int ih = ck.rh + d * (ck.j0 - 1 + hr);
      bf16x8 vec = bf16x8{};
      if ((unsigned)id < (unsigned)dd.D && (unsigned)ih < (unsigned)dd.H &&
          ci0 + ci < dd.KCH)
        vec = dil_load8(xn + ((int64_t)(ci0 + ci) * dd.D + id) * HW +
                            (int64_t)ih * dd.W,
                        ck.ow0 - d8 + v * 8, dd.W, wvec);
      *reinterpret_cast<bf16x8*>(sX + ci * chs + (a * H2 + hr) * pitch +
                                 v * 8) = vec;
    }
    // ---- go tile [co][lattice row][32 columns]; masked positions are zero
    const __bf16* gon = go + (int64_t)ck.n * dd.NCOL * dd.D * HW;
    for (int it = tid; it < COT * OHT * (OWT / 8); it += 256) {
      const int v = it % (OWT / 8);
      const int jl = (it / (OWT / 8)) % OHT;
      const int co = it / (OWT / 8 * OHT);
      const int oh = ck.rh + d * (ck.j0 + jl);
      bf16x8 vec = bf16x8{};
      if (oh < dd.H && co0 + co < dd.NCOL)
        vec = dil_load8(gon + ((int64_t)(co0 + co) * dd.D + ck.od) * HW +
                            (int64_t)oh * dd.W,
                        ck.ow0 + v * 8, dd.W, wvec);
      *reinterpret_cast<bf16x8*>(sGo + co * GOP + jl * OWT + v * 8) = vec;
    }
    __syncthreads();

    // ---- 32-m sub-chunk = one lattice row: go fragment x 27 taps ---------
#pragma unroll 1
    for (int ms = 2 * wm; ms < 2 * wm + 2; ++ms) {
      const bf16x8 afrag = *reinterpret_cast<const bf16x8*>(
          sGo + (wi * 16 + row) * GOP + ms * OWT + kg * 8);
      // tap (kd, kh, kw) of output column kg*8: plane kd, row ms + kh,
      // slab column ceil8(d) + kg*8 + (kw - 1)*d
      const __bf16* xb = sX + row * chs + ms * pitch + d8 - d + kg * 8;
#pragma unroll
      for (int kd = 0; kd < 3; ++kd)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const bf16x8 bfrag = dil_xfrag<ALIGN>(
                xb + (kd * H2 + kh) * pitch + kw * d);
            acc[(kd * 3 + kh) * 3 + kw] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    afrag, bfrag, acc[(kd * 3 + kh) * 3 + kw], 0, 0, 0);
          }
    }
    __syncthreads();
  }

  // ---- this (z, m half)'s slice, tap-major: 16 ci are one 64-byte run ----
  float* outp = part + (int64_t)(blockIdx.z * 2 + wm) * 27 * dd.NCOL * dd.KCH;
  const int ci = ci0 + (lane & 15);
  const int crow0 = (lane >> 4) * 4;
#pragma unroll
  for (int tp = 0; tp < 27; ++tp)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + wi * 16 + crow0 + r;
      if (co < dd.NCOL && ci < dd.KCH)
        outp[((int64_t)tp * dd.NCOL + co) * dd.KCH + ci] = acc[tp][r];
    }
}

static DilDims make_dildims(const torch::Tensor& in, int ncol, int d) {
  DilDims dd;
  dd.N = (int)in.size(0); dd.KCH = (int)in.size(1);
  dd.D = (int)in.size(2); dd.H = (int)in.size(3); dd.W = (int)in.size(4);
  dd.NCOL = ncol;
  dd.d = d;
  dd.Kpad = 0;
  dd.hcls = std::min(d, dd.H);
  dd.jtiles = ((dd.H + d - 1) / d + DIL_OHT - 1) / DIL_OHT;
  dd.wtiles = (dd.W + DIL_OWT - 1) / DIL_OWT;
  return dd;
}

static int64_t dil_nchunks(const DilDims& dd) {
  return (int64_t)dd.N * dd.D * dd.hcls * dd.jtiles * dd.wtiles;
}

static void check_dil(const torch::Tensor& t, int64_t d) {
  CHECK_GPU(t);
  TORCH_CHECK(t.dim() == 5 && t.numel() > 0, "expected a non-empty NCDHW tensor");
  TORCH_CHECK(d >= 2 && d <= 16, "conv3d_dilated: dilation must be in [2, 16]");
}

// the dilated conv of `in` with w (dgrad: tap-flipped, transposed)
static torch::Tensor dil_conv(torch::Tensor in, torch::Tensor wc, int ncol, int d,
                       bool dgrad) {
  DilDims dd = make_dildims(in, ncol, d);
  // tile choice: 32-channel tiles while the slab fits 64 KB (d <= 8) and the
  // channels fill them; 64 output columns per block when there are that many
  const int ctile = (d > 8 || dd.KCH <= 16) ? 16 : 32;
  const int ncolt = ncol > 32 ? 64 : 32;
  const int kt_pad = (ctile * 27 + 31) / 32 * 32;
  const int kts = (dd.KCH + ctile - 1) / ctile;
  const int kpad = kts * kt_pad;
  const int rows = (ncol + 127) / 128 * 128;
  TORCH_CHECK((int64_t)rows * kpad < (int64_t)1 << 31, "WB too large");
  const int64_t nchunks = dil_nchunks(dd);
  TORCH_CHECK(nchunks < (int64_t)1 << 31, "grid too large");
  auto s = current_stream();
  auto wb = torch::empty({rows, (int64_t)kpad}, wc.options());
  hipLaunchKernelGGL(conv3d_dil_prep_wb_kernel,
                     dim3((rows * kpad + 255) / 256), dim3(256), 0, s,
                     reinterpret_cast<const __bf16*>(wc.data_ptr()),
                     reinterpret_cast<__bf16*>(wb.data_ptr()), ncol, dd.KCH,
                     ctile, kt_pad, kpad, dgrad ? 1 : 0);
  dd.Kpad = kpad;
  auto out = torch::empty({dd.N, ncol, dd.D, dd.H, dd.W}, in.options());
  const size_t lds =
      (size_t)3 * DIL_H2 * (DIL_OWT + 2 * d) * ctile * sizeof(__bf16);
  TORCH_CHECK(lds <= 64 * 1024, "conv3d_dilated: slab exceeds 64 KB");
  dim3 grid((unsigned)nchunks, (ncol + ncolt - 1) / ncolt);
  dispatch_bool(ctile == 32, [&](auto c32) {
    dispatch_bool(ncolt == 64, [&](auto n64) {
      hipLaunchKernelGGL(
          (conv3d_dil_kernel<decltype(c32)::value ? 32 : 16,
                             decltype(n64)::value ? 64 : 32>),
          grid, dim3(256), lds, s,
          reinterpret_cast<const __bf16*>(in.data_ptr()),
          reinterpret_cast<const __bf16*>(wb.data_ptr()),
          reinterpret_cast<__bf16*>(out.data_ptr()), dd);
    });
  });
  return out;
}

torch::Tensor conv3d_dil_fwd(torch::Tensor x, torch::Tensor w, int64_t d) {
  check_dil(x, d);
  auto xc = x.to(torch::kBFloat16).contiguous();
  auto wc = w.to(torch::kBFloat16).contiguous();
  TORCH_CHECK(wc.dim() == 5 && wc.size(2) == 3 && wc.size(3) == 3 &&
              wc.size(4) == 3, "conv3d_dilated: 3x3x3 weights");
  TORCH_CHECK(wc.size(1) == xc.size(1), "weight/input channel mismatch");
  return dil_conv(xc, wc, (int)wc.size(0), (int)d, false);
}

torch::Tensor conv3d_dil_dgrad(torch::Tensor go, torch::Tensor w,
                               std::vector<int64_t> in_shape, int64_t d) {
  check_dil(go, d);
  auto g = go.to(torch::kBFloat16).contiguous();
  auto wc = w.to(torch::kBFloat16).contiguous();
  TORCH_CHECK(in_shape.size() == 5 && wc.dim() == 5 &&
              wc.size(0) == g.size(1) && wc.size(1) == in_shape[1],
              "weight/grad channel mismatch");
  TORCH_CHECK(in_shape[0] == g.size(0) && in_shape[2] == g.size(2) &&
              in_shape[3] == g.size(3) && in_shape[4] == g.size(4),
              "pad == dilation: dx has the spatial shape of go");
  return dil_conv(g, wc, (int)in_shape[1], (int)d, true);
}

torch::Tensor conv3d_dil_wgrad(torch::Tensor x, torch::Tensor go, int64_t d) {
  check_dil(x, d);
  CHECK_GPU(go);
  auto xc = x.to(torch::kBFloat16).contiguous();
  auto g = go.to(torch::kBFloat16).contiguous();
  TORCH_CHECK(g.dim() == 5 && g.size(0) == xc.size(0) &&
              g.size(2) == xc.size(2) && g.size(3) == xc.size(3) &&
              g.size(4) == xc.size(4), "x / go shape mismatch");
  DilDims dd = make_dildims(xc, (int)g.size(1), (int)d);
  const int co_t = (dd.NCOL + DILW_COT - 1) / DILW_COT;
  const int ci_t = (dd.KCH + DILW_CT - 1) / DILW_CT;
  const int64_t nchunks = dil_nchunks(dd);
  // 512 blocks in flight, the target the dense tap-reuse wgrad was swept to
  const int zs = (int)std::max<int64_t>(
      1, std::min<int64_t>(nchunks, 512 / std::max(co_t * ci_t, 1)));
  const int pitch = dilw_pitch((int)d), chs = dilw_chs((int)d);
  const size_t lds =
      (size_t)(DILW_COT * DILW_GOP + DILW_CT * chs) * sizeof(__bf16);
  TORCH_CHECK(lds <= 64 * 1024, "conv3d_dilated wgrad: LDS exceeds 64 KB");
  auto part = torch::empty({2 * (int64_t)zs, 27, dd.NCOL, dd.KCH},
                           xc.options().dtype(torch::kFloat32));
  dim3 grid(co_t, ci_t, zs);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, current_stream(),
                       reinterpret_cast<const __bf16*>(xc.data_ptr()),
                       reinterpret_cast<const __bf16*>(g.data_ptr()),
                       part.data_ptr<float>(), dd, nchunks, pitch, chs);
  };
  if (d % 8 == 0) launch(conv3d_dil_wgrad_kernel<8>);
  else if (d % 4 == 0) launch(conv3d_dil_wgrad_kernel<4>);
  else launch(conv3d_dil_wgrad_kernel<1>);
  return part.sum(0).permute({1, 2, 0}).contiguous()
      .view({dd.NCOL, dd.KCH, 3, 3, 3});
}
