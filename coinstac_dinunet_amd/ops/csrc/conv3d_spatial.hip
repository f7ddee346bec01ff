// Conv3d fwd/dgrad with spatial-slab tap reuse (stride 1 and stride-2 fwd).
// The igemm formulation re-gathers x once per (ci,tap) — 27x traffic.
// Here a block stages one input spatial slab per channel tile and computes
// the whole K loop from it:
//   - CTILE >= 16: the slab is channel-innermost, [3][H2][W2][CTILE], and K
//     inside a tile runs (tap, local channel), so an A fragment is one
//     16-byte LDS read at a wave-uniform tap offset. Rows are fetched as
//     16-byte vectors along w, BN+ReLU applied per channel, and 4 or 8
//     adjacent channels interleaved into one wide LDS store;
//   - CTILE 1 (first layer): the slab is [3][H2][W2] and the A fragments
//     read it at base(m) + sKtab[k], a precomputed u16 tap-offset table;
//   - the B fragments are contiguous 16-byte global loads from the small
//     L2-resident prepared-weight matrix WB[ncol][kts*KT_PAD] (fwd: w
//     reordered; dgrad: tap-flipped + transposed; each CTILE-channel block
//     zero-padded to a 32-multiple so MFMA k-windows never straddle tiles),
//     loaded one k-step ahead of the MFMAs that use them.
// Geometry: out tile = (OWT*OHT) m x NCOLT ncol (32, 64 or 128); 4 waves x
// MPW m-fragments x NCOLT/16 ncol-fragments; chunk = (n, d, h-tile, w-tile)
// of the OUTPUT grid.
// STRIDE=2 stages the strided window (IW = 2*OWT interior) with CTILE=16.
// The stride-2 dgrad (conv3d_dgrad_s2_sp_kernel, below) is its own kernel:
// 8 parity classes of a dx brick from one staged go slab.
#include "common.h"
#include "conv3d_dispatch.h"

#include <hip/hip_bf16.h>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

struct SpDims {
  int N, KCH;        // input-side channels (fwd: Cin; dgrad: Cout)
  int D, H, W;       // input-side spatial (fwd: x dims; dgrad: go dims)
  int NCOL;          // output-side channels
  int TD, TH, TW;    // output-side spatial
  int Kpad;          // row length of WB = kts * KT_PAD
};

#ifndef LDA_PAD
#define LDA_PAD 8
#endif

// Waves per SIMD the register allocation must leave room for. The
// small-slab chunk-64 instances are not LDS-limited, and the unrolled tap
// loop would otherwise trade their occupancy for hoisted loads.
constexpr int sp_min_waves(int ctile, int chunk, int ncolt, bool fuse_bn,
                           int dt) {
  // depth-blocked: DT * NCOLT/16 accumulator fragments (64 registers on the
  // kept instances) next to the staging registers; the 46-49 KB slab holds
  // a CU to 3 blocks anyway
  if (dt > 1) return 2;
  if (ctile < 16 || chunk != 64) return 1;
  if (ncolt == 128 || fuse_bn) return 4;
  return ncolt == 32 ? 6 : 5;
}

// FUSE_BN: normalize-on-load — the staged input is the PREVIOUS block's
// raw conv output; z = relu(a[c]*x + b[c]) is applied per element during
// staging (a = gamma*rstd, b = beta - mean*a, exactly bn_normalize's
// folding) so the normalized tensor never exists in HBM. Padding halo
// stays 0 (conv pads the BN OUTPUT with zeros).
// SMODE 1: the epilogue also folds per-output-channel (sum, sumsq) of
// the written elements into stats[hash_slice][NCOL][2] — the NEXT
// block's BN statistics come for free (no standalone bn_reduce pass).
// Hash slices (blockIdx.x & 63) spread the atomics.
// DT > 1 (whole-plane chunk-64 tiles, TW == 8 and TH <= 8): a block covers
// DT consecutive output depth planes from one slab of (DT-1)*STRIDE + 3
// input planes. Fragment i of a wave is the wave's 16 rows of plane td + i,
// a whole-plane stride away in the slab, so each B load feeds DT MFMAs and
// an input plane is staged (DT+2)/DT times instead of 3. The tile covers
// the plane, so the halo rows and columns are padding: zeroed once, never
// staged. K order per output element is that of DT = 1.
template <int OWT, int STRIDE, int CTILE,
          int CHUNK = (STRIDE == 1 ? 256 : 128), bool FUSE_BN = false,
          int SMODE = 0, int NCOLT = 32, int DT = 1>
__global__ __launch_bounds__(
    256, sp_min_waves(CTILE, CHUNK, NCOLT, FUSE_BN, DT))
void conv3d_spatial_kernel(
    const __bf16* __restrict__ in, const __bf16* __restrict__ wb,
    __bf16* __restrict__ out, SpDims sd, int64_t nchunks,
    const float* __restrict__ bn_ab = nullptr,
    float* __restrict__ stats = nullptr) {
  constexpr int OHT = CHUNK / OWT;
  constexpr int IW = STRIDE * OWT;                  // staged interior width
  constexpr int W2 = IW + (STRIDE == 1 ? 4 : 2);
  constexpr int H2 = STRIDE * (OHT - 1) + 3;
  constexpr int MPW = DT * CHUNK / 64;              // m-frags per wave
  static_assert(MPW >= 1, "chunk too small");
  static_assert(DT == 1 || (CTILE >= 16 && OWT == 8 && CHUNK == 64),
                "depth blocking: whole-plane chunk-64 tiles only");
  constexpr int PD = (DT - 1) * STRIDE + 3;         // staged depth planes
  constexpr int KT_PAD = ((CTILE * 27 + 31) / 32) * 32;
  constexpr int NCF = NCOLT / 16;  // ncol fragments per wave
  constexpr bool CL = CTILE >= 16;  // channel-innermost slab, b128 A reads
  static_assert(!CL || (CTILE == 32 && STRIDE == 1) || CTILE == 16,
                "channel-innermost tiles: 32 (stride 1) or 16");
  static_assert(!CL || (CHUNK / 4) % OWT == 0 || OWT == 8,
                "a wave's fragments must start on a tile row");
  __shared__ __attribute__((aligned(16))) __bf16 sXf[CTILE * PD * H2 * W2];
  __shared__ unsigned short sKtab[CL ? 8 : KT_PAD + 8];
  auto sX = reinterpret_cast<__bf16(*)[3][H2][W2]>(sXf);  // !CL view

  const int ncol0 = blockIdx.y * NCOLT;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int row = lane & 15, kg = lane >> 4;

  const int wtiles = (sd.TW + OWT - 1) / OWT;
  const int htiles = (sd.TH + OHT - 1) / OHT;

  int64_t t = blockIdx.x;
  const int wt = (int)(t % wtiles);
  t /= wtiles;
  const int ht = (int)(t % htiles);
  t /= htiles;
  const int dgroups = (sd.TD + DT - 1) / DT;
  const int td = (int)(t % dgroups) * DT;  // first output plane
  const int n = (int)(t / dgroups);
  const int oh0 = ht * OHT, ow0 = wt * OWT;

  // k -> slab element offset (pad entries -> 0: their weights are zero)
  for (int k = tid; !CL && k < KT_PAD; k += 256) {
    unsigned short off = 0;
    if (k < CTILE * 27) {
      const int cl = k / 27;
      const int r27 = k - cl * 27;
      const int a = r27 / 9, b = (r27 / 3) % 3, c = r27 % 3;
      off = (unsigned short)(((cl * 3 + a) * H2 + b) * W2 + c);
    }
    sKtab[k] = off;
  }

  f32x4 acc[MPW][NCF];
#pragma unroll
  for (int i = 0; i < MPW; ++i)
#pragma unroll
    for (int j = 0; j < NCF; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int64_t HW = (int64_t)sd.H * sd.W;
  const int64_t in_n = (int64_t)n * sd.KCH * sd.D * HW;
  const int kts = (sd.KCH + CTILE - 1) / CTILE;

  if constexpr (CL) {
    // ---- channel-innermost slab [3][H2][W2][CTILE] --------------------
    // K inside a channel tile runs (tap, local channel), so the 8 k of
    // lane (row, kg) are ONE 16-byte word of the slab. A ds_read_b128 is
    // served in four groups of 16 lanes, each holding 16 distinct rows
    // under two kg values; the XOR swizzles below spread every group over
    // all 64 banks:
    //   CTILE 32 (64 B per position):            chunk    ^= 2 * bit2(w)
    //   CTILE 16, stride 2 (rows 64 B apart):    position ^= bit3(w)
    //   CTILE 16, stride 1 (rows 32 B apart):    conflict-free as it is
    auto slab_off = [](int a, int h, int w, int cl) -> int {
      int pos = w, chunk = cl >> 3;
      if (CTILE == 32) chunk ^= ((w >> 2) & 1) << 1;
      if (CTILE == 16 && STRIDE == 2) pos ^= (w >> 3) & 1;
      return ((a * H2 + h) * W2 + pos) * CTILE + chunk * 8 + (cl & 7);
    };
    // A address = lanew[c] + (fragment, tap-plane) constants: the swizzle
    // bits of w depend on (row, c) only, fragments start 16 or 32 columns
    // apart and tap planes whole rows apart
    const int m_l = (DT > 1 ? wave * 16 : wave * (MPW * 16)) + row;
    int lanew[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      lanew[c] = slab_off(0, STRIDE * (m_l / OWT), STRIDE * (m_l % OWT) + c,
                          (CTILE == 32 ? kg : (kg & 1)) * 8);
    auto frag_off = [](int i) -> int {
      if (DT > 1) return i * STRIDE * H2 * W2 * CTILE;
      return (STRIDE * ((i * 16) / OWT) * W2 + STRIDE * ((i * 16) % OWT)) *
             CTILE;
    };

    // B: lane (col = row, kg) reads 8 consecutive k of its column; channel
    // tiles are contiguous in WB, so k-step g = kt*KS + ks sits at g*32.
    // WB has zero rows up to the next multiple of 128 columns, so a ragged
    // column tile needs no bounds check here.
    constexpr int KS = KT_PAD / 32;
    const __bf16* wbl = wb + (int64_t)(ncol0 + row) * sd.Kpad + kg * 8;
    auto bload = [&](int j, int g) -> bf16x8 {
      return *reinterpret_cast<const bf16x8*>(
          wbl + (int64_t)j * 16 * sd.Kpad + (int64_t)g * 32);
    };
    constexpr bool BPF = NCF <= 2;  // one-deep B register pipeline
    bf16x8 bcur[NCF];
#pragma unroll
    for (int j = 0; BPF && j < NCF; ++j)
      bcur[j] = bload(j, 0);

    constexpr int NV = IW / 8;  // 8-column vectors per interior row
    // a thread carries one 8-column vector of CG adjacent channels and
    // stores 8 interleaved CG-channel words (lanes run over channel group,
    // then column vector: 2- to 4-way conflicted stores, but the row-
    // interleaved conflict-free order lost, profiles/spatial_b128_ab.md)
    // DT > 1 stages the STRIDE*8 interior rows only (slab rows 1..)
    constexpr int HR = DT > 1 ? STRIDE * 8 : H2;
    constexpr int HR0 = DT > 1 ? 1 : 0;
    constexpr int CG = (PD * HR * NV * (CTILE / 8) >= 256) ? 8 : 4;
    constexpr int NCG = CTILE / CG;
    constexpr int NITEM = PD * HR * NV * NCG;
    constexpr int NHALO = STRIDE == 1 ? 2 : 1;  // halo columns the taps read
    const int iw0 = STRIDE * ow0;
    const bool wvec = (sd.W & 7) == 0;  // rows 16-byte aligned

    if constexpr (DT > 1) {
      // the halo is conv padding (zero AFTER the BN transform): written
      // here once, the interior stores below never touch it
      for (int it = tid; it < CTILE * PD * H2 * W2 / 8; it += 256)
        reinterpret_cast<bf16x8*>(sXf)[it] = bf16x8{};
      __syncthreads();
    }

    for (int kt = 0; kt < kts; ++kt) {
      if (kt) __syncthreads();
      for (int it = tid; it < NITEM; it += 256) {
        const int cg = it % NCG;
        const int v = (it / NCG) % NV;
        const int hrow = HR0 + (it / (NCG * NV)) % HR;
        const int a = it / (NCG * NV * HR);
        const int id = STRIDE * td - 1 + a;
        const int ih = STRIDE * oh0 - 1 + hrow;
        const int iw = iw0 + v * 8;
        const bool row_ok = (unsigned)id < (unsigned)sd.D &&
                            (unsigned)ih < (unsigned)sd.H;
        __bf16 t[CG][8];
#pragma unroll
        for (int cc = 0; cc < CG; ++cc) {
          const int ch = kt * CTILE + cg * CG + cc;
#pragma unroll
          for (int j = 0; j < 8; ++j) t[cc][j] = (__bf16)0.f;
          if (row_ok && ch < sd.KCH) {
            const __bf16* src = in + in_n + ((int64_t)ch * sd.D + id) * HW +
                                (int64_t)ih * sd.W;
            float a_c = 1.f, b_c = 0.f;
            if (FUSE_BN) { a_c = bn_ab[ch * 2]; b_c = bn_ab[ch * 2 + 1]; }
            auto tx = [&](__bf16 x) -> __bf16 {
              if (!FUSE_BN) return x;
              return (__bf16)fmaxf(a_c * (float)x + b_c, 0.f);
            };
            if (wvec && iw + 8 <= sd.W) {
              const bf16x8 vec = *reinterpret_cast<const bf16x8*>(src + iw);
#pragma unroll
              for (int j = 0; j < 8; ++j) t[cc][j] = tx(vec[j]);
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j)
                if (iw + j < sd.W) t[cc][j] = tx(src[iw + j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          __bf16* dst = sXf + slab_off(a, hrow, 1 + v * 8 + j, cg * CG);
          if constexpr (CG == 8) {
            bf16x8 o;
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) o[cc] = t[cc][j];
            *reinterpret_cast<bf16x8*>(dst) = o;
          } else {
            bf16x4 o;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) o[cc] = t[cc][j];
            *reinterpret_cast<bf16x4*>(dst) = o;
          }
        }
      }
      // halo columns: one element per (plane, row, side, channel)
      for (int it = tid; DT == 1 && it < 3 * H2 * NHALO * CTILE; it += 256) {
        const int cl = it % CTILE;
        const int side = (it / CTILE) % NHALO;
        const int hrow = (it / (CTILE * NHALO)) % H2;
        const int a = it / (CTILE * NHALO * H2);
        const int col = side ? IW + 1 : 0;
        const int id = STRIDE * td - 1 + a;
        const int ih = STRIDE * oh0 - 1 + hrow;
        const int iw = iw0 - 1 + col;
        const int ch = kt * CTILE + cl;
        __bf16 val = (__bf16)0.f;
        if ((unsigned)id < (unsigned)sd.D && (unsigned)ih < (unsigned)sd.H &&
            (unsigned)iw < (unsigned)sd.W && ch < sd.KCH) {
          val = in[in_n + ((int64_t)ch * sd.D + id) * HW +
                   (int64_t)ih * sd.W + iw];
          if (FUSE_BN)
            val = (__bf16)fmaxf(
                bn_ab[ch * 2] * (float)val + bn_ab[ch * 2 + 1], 0.f);
        }
        sXf[slab_off(a, hrow, col, cl)] = val;
      }
      __syncthreads();

      // ---- k-steps of 32: one tap x 32 channels, or two taps x 16 -----
      // the next step's B fragments are in flight under this step's MFMAs
      // (narrow instances; the wide ones have no registers to spare for it)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if constexpr (!BPF) {
#pragma unroll
          for (int j = 0; j < NCF; ++j)
            bcur[j] = bload(j, kt * KS + ks);
        }
        const bool more = BPF && (ks + 1 < KS || kt + 1 < kts);
        bf16x8 bnext[NCF];
        if (more) {
#pragma unroll
          for (int j = 0; j < NCF; ++j)
            bnext[j] = bload(j, kt * KS + ks + 1);
        }
        int lk;
        if (CTILE == 32) {
          lk = lanew[ks % 3] + ((ks / 9) * H2 + (ks / 3) % 3) * W2 * CTILE;
        } else {
          // taps 2ks (kg 0,1) and 2ks+1 (kg 2,3); the 28th tap has zero
          // weights and re-reads the 27th
          const int t0 = 2 * ks, t1 = 2 * ks + 1 < 27 ? 2 * ks + 1 : 26;
          const int l0 =
              lanew[t0 % 3] + ((t0 / 9) * H2 + (t0 / 3) % 3) * W2 * CTILE;
          const int l1 =
              lanew[t1 % 3] + ((t1 / 9) * H2 + (t1 / 3) % 3) * W2 * CTILE;
          lk = (kg >> 1) ? l1 : l0;
        }
        bf16x8 afrag[MPW];
#pragma unroll
        for (int i = 0; i < MPW; ++i)
          afrag[i] =
              *reinterpret_cast<const bf16x8*>(sXf + lk + frag_off(i));
#pragma unroll
        for (int i = 0; i < MPW; ++i)
#pragma unroll
          for (int j = 0; j < NCF; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag[i], bcur[j], acc[i][j], 0, 0, 0);
        if (more) {
#pragma unroll
          for (int j = 0; j < NCF; ++j) bcur[j] = bnext[j];
        }
        // keep the unrolled loop's B loads in their own k-step: hoisted
        // over the DT * NCF accumulator fragments they spill
        if constexpr (DT > 1) __builtin_amdgcn_sched_barrier(0);
      }
    }
  } else {
  // CTILE 1 (first layer): w-innermost slab, A gathered through sKtab
  for (int kt = 0; kt < kts; ++kt) {
    // ---- stage the slab row-wise (16B interior, scalar halo) ----------
    constexpr int NROWS = CTILE * 3 * H2;
    if (kt) __syncthreads();
    for (int r = tid; r < NROWS; r += 256) {
      const int hrow = r % H2;
      const int a = (r / H2) % 3;
      const int c = r / (3 * H2);
      const int id = STRIDE * td - 1 + a;
      const int ih = STRIDE * oh0 - 1 + hrow;
      const int ch = kt * CTILE + c;
      __bf16* dst = &sX[c][a][hrow][0];
      const bool row_ok = (unsigned)id < (unsigned)sd.D &&
                          (unsigned)ih < (unsigned)sd.H && ch < sd.KCH;
      if (!row_ok) {
#pragma unroll
        for (int col = 0; col < W2; ++col) dst[col] = (__bf16)0.f;
        continue;
      }
      const __bf16* src = in + in_n + ((int64_t)ch * sd.D + id) * HW +
                          (int64_t)ih * sd.W;
      float a_c = 1.f, b_c = 0.f;
      if (FUSE_BN) { a_c = bn_ab[ch * 2]; b_c = bn_ab[ch * 2 + 1]; }
      auto tx = [&](__bf16 v) -> __bf16 {
        if (!FUSE_BN) return v;
        return (__bf16)fmaxf(a_c * (float)v + b_c, 0.f);
      };
      const int iw0 = STRIDE * ow0;
      dst[0] = (iw0 > 0) ? tx(src[iw0 - 1]) : (__bf16)0.f;
#pragma unroll
      for (int v = 0; v < IW / 8; ++v) {
        bf16x8 vec = *reinterpret_cast<const bf16x8*>(src + iw0 + v * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[1 + v * 8 + j] = tx(vec[j]);
      }
#pragma unroll
      for (int e = 0; e < W2 - IW - 1; ++e) {
        const int iw = iw0 + IW + e;
        dst[1 + IW + e] = (iw < sd.W) ? tx(src[iw]) : (__bf16)0.f;
      }
    }
    __syncthreads();

    // ---- k-steps of 32 over (ch_local, tap) ---------------------------
    const int kbase_g = kt * KT_PAD;
#pragma unroll 1
    for (int ks = 0; ks < KT_PAD / 32; ++ks) {
      bf16x8 afrag[MPW];
      {
        const int kb = ks * 32 + kg * 8;
        const u16x8 kt8 = *reinterpret_cast<const u16x8*>(&sKtab[kb]);
        const __bf16* slab = &sX[0][0][0][0];
#pragma unroll
        for (int i = 0; i < MPW; ++i) {
          const int m = (wave * MPW + i) * 16 + row;
          const int base = (STRIDE * (m / OWT)) * W2 + STRIDE * (m % OWT);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            afrag[i][j] = slab[base + kt8[j]];
        }
      }
      bf16x8 bfrag[NCF];
#pragma unroll
      for (int i = 0; i < NCF; ++i) {
        const int col = ncol0 + i * 16 + row;
        const int64_t off =
            (int64_t)col * sd.Kpad + kbase_g + ks * 32 + kg * 8;
        bfrag[i] = (col < sd.NCOL)
                       ? *reinterpret_cast<const bf16x8*>(wb + off)
                       : bf16x8{};
      }
#pragma unroll
      for (int i = 0; i < MPW; ++i)
#pragma unroll
        for (int j = 0; j < NCF; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[i], bfrag[j], acc[i][j], 0, 0, 0);
    }
  }
  }

  // ---- epilogue: out[n][col][td][oh0+][ow0+] --------------------------
  // a lane's 4 consecutive m share an output row (OWT is a multiple of 8):
  // one 8-byte store when the rows are 8-byte aligned (TW % 4 == 0)
  const bool pack4 = (sd.TW & 3) == 0;
  const int64_t THW = (int64_t)sd.TH * sd.TW;
  const int64_t out_n = (int64_t)n * sd.NCOL * sd.TD * THW;
  const int ccol = lane & 15;
  const int crow0 = (lane >> 4) * 4;
  float cs[8] = {}, css[8] = {};  // per-col-frag partials (NCF <= 8)
  static_assert(NCF <= 8, "stats buffers sized for NCF <= 8");
#pragma unroll
  for (int i = 0; i < MPW; ++i) {
    // depth-blocked: fragment i is the wave's 16 rows of plane td + i;
    // planes of a ragged last group past TD are neither stored nor counted
    const int tdi = DT > 1 ? td + i : td;
    const int mw = DT > 1 ? wave * 16 : (wave * MPW + i) * 16;
    if (tdi >= sd.TD) continue;
#pragma unroll
    for (int j = 0; j < NCF; ++j) {
      const int col = ncol0 + j * 16 + ccol;
      if (col >= sd.NCOL) continue;
      if (pack4) {
        const int m = mw + crow0;
        const int oh = oh0 + m / OWT;
        const int ow = ow0 + m % OWT;
        if (oh < sd.TH && ow < sd.TW) {  // ow % 4 == 0: ow + 3 < TW too
          bf16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            o[r] = (__bf16)acc[i][j][r];
            if (SMODE == 1) {
              const float vb = (float)o[r];
              cs[j] += vb;
              css[j] += vb * vb;
            }
          }
          *reinterpret_cast<bf16x4*>(
              out + out_n + ((int64_t)col * sd.TD + tdi) * THW +
              (int64_t)oh * sd.TW + ow) = o;
        }
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mw + crow0 + r;
        const int oh = oh0 + m / OWT;
        const int ow = ow0 + m % OWT;
        if (oh < sd.TH && ow < sd.TW) {
          const float v = acc[i][j][r];
          const int64_t off = out_n + ((int64_t)col * sd.TD + tdi) * THW +
                              (int64_t)oh * sd.TW + ow;
          out[off] = (__bf16)v;
          if (SMODE == 1) {
            // accumulate the ROUNDED value: bit-matches bn3d_stats on
            // the stored bf16 tensor
            const float vb = (float)(__bf16)v;
            cs[j] += vb;
            css[j] += vb * vb;
          }
        }
      }
    }
  }
  if (SMODE != 0) {
    // lanes l, l+16, l+32, l+48 share ccol: fold over lane bits 4-5
#pragma unroll
    for (int j = 0; j < NCF; ++j) {
      cs[j] += __shfl_xor(cs[j], 16);
      cs[j] += __shfl_xor(cs[j], 32);
      css[j] += __shfl_xor(css[j], 16);
      css[j] += __shfl_xor(css[j], 32);
    }
    __shared__ float sred[4][NCF][16][2];
    if ((lane >> 4) == 0) {
#pragma unroll
      for (int j = 0; j < NCF; ++j) {
        sred[wave][j][ccol][0] = cs[j];
        sred[wave][j][ccol][1] = css[j];
      }
    }
    __syncthreads();
    // NCF*32 (col, stat) pairs: low threads fold the 4 waves and emit
    // one atomicAdd each into the hashed stats slice
    if (tid < NCF * 32) {
      const int j = tid >> 5;           // col fragment
      const int cc = (tid >> 1) & 15;   // ccol
      const int st = tid & 1;           // 0 = sum, 1 = sumsq
      const int col = ncol0 + j * 16 + cc;
      if (col < sd.NCOL) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) t += sred[w][j][cc][st];
        float* slice = stats +
            ((int64_t)(blockIdx.x & 63) * sd.NCOL + col) * 2 + st;
        atomicAdd(slice, t);
      }
    }
  }
}

// ---- host -----------------------------------------------------------------
static SpDims make_spdims(const torch::Tensor& in, int ncol, int td, int th,
                          int tw) {
  SpDims sd;
  sd.N = (int)in.size(0); sd.KCH = (int)in.size(1);
  sd.D = (int)in.size(2); sd.H = (int)in.size(3); sd.W = (int)in.size(4);
  sd.NCOL = ncol;
  sd.TD = td; sd.TH = th; sd.TW = tw;
  sd.Kpad = 0;  // set once the weights are prepared
  return sd;
}

// What the caller wants from conv3d_spatial_kernel; which instance serves it
// is plan_spatial's business.
enum SpMode {
  SP_PLAIN,        // forward
  SP_CTILE1,       // forward, Cin < 16 (stride 1): single-channel tiles
  SP_CTILE1_STATS,  // ... and the epilogue BN statistics
  SP_FUSED,        // forward with normalize-on-load
  SP_FUSED_STATS,  // ... and the epilogue BN statistics
  SP_DGRAD,        // stride-1 input gradient (go in, tap-flipped weights)
};

struct SpatialPlan {
  int owt, chunk, ctile, ncolt;  // template arguments of the instance
  int gcolt;                     // column tile the grid's y extent is cut by
  int dt;                        // output depth planes per block
};

static SpatialPlan plan_spatial(const SpDims& sd, int stride, SpMode mode) {
  SpatialPlan p;
  p.owt = sd.TW % 32 == 0 ? 32 : (sd.TW % 16 == 0 ? 16 : 8);
  p.chunk = stride == 1 ? 256 : 128;
  const bool ctile1 = mode == SP_CTILE1 || mode == SP_CTILE1_STATS;
  p.ctile = ctile1 ? 1 : (stride == 1 ? 32 : 16);
  p.ncolt = p.gcolt = 32;
  p.dt = 1;
  const bool fused = mode == SP_FUSED || mode == SP_FUSED_STATS;
  // thin-channel large-plane stride-1 layers (L2-class): chunk 512 at
  // CTILE 16 doubles the m that amortizes each staged slab — dgrad 36.2 vs
  // 36.6, fused-stats fwd 35.8 vs 36.1 ms/step on the flagship (r2)
  if ((mode == SP_FUSED_STATS || mode == SP_DGRAD) && stride == 1 &&
      sd.KCH <= 32 && sd.TW % 32 == 0 && sd.TH * sd.TW >= 512) {
    p.chunk = 512;
    p.ctile = 16;
    return p;
  }
  // 64-col chunk-256 forward instances: halve the slab re-reads of the big
  // stride-1 layers — 36.7 vs 37.5 ms/step on the flagship (r2)
  if (stride == 1 && sd.NCOL >= 64 && (mode == SP_PLAIN || fused))
    p.gcolt = 64;
  // stride-2 chunk-128 forwards: the 57 KB slab feeds only 56 MFMAs per
  // wave at 32 columns, so every epilogue has 64- and 128-column instances
  // (grid and kernel column tile are the same number here)
  if (stride == 2 && sd.NCOL >= 64) p.gcolt = sd.NCOL >= 128 ? 128 : 64;
  // small images (d8-class): 64-position chunks keep the grid dense;
  // wide-column instances halve the slab-staging redundancy there
  // (PMC: 86% SQ_WAIT on the 32-col chunk-64 forms)
  if (sd.TH * sd.TW < p.chunk) {
    p.chunk = 64;
    p.owt = 8;  // the chunk-64 instances are OWT=8
    // swept on MI355X (r2): 128-col instances won at the deep layers
    // (37.7 vs 38.2 ms/step flagship) — slab re-reads drop 4x vs 32-col
    if (sd.NCOL >= 64 && !ctile1)
      p.gcolt = sd.NCOL >= 128 ? 128 : 64;
    // one tile is the whole output plane (d8-class forwards): depth-blocked
    // instances, one (DT, column tile) per stride whatever NCOL is — 4
    // planes x 64 columns at stride 1 (the 6-plane slab is 46 KB), 2 x 128
    // at stride 2 (49 KB; DT 4 does not fit). Swept on MI355X,
    // profiles/smallplane_ab.md.
    if ((mode == SP_PLAIN || fused) && sd.TW == 8 && sd.TH <= 8) {
      p.dt = stride == 1 ? 4 : 2;
      p.gcolt = stride == 1 ? 64 : 128;
    }
  }
  p.ncolt = p.gcolt;
  // KNOWN DEFECT, kept as it was (docs/NEXT.md, "Under-covered column
  // grid"): the fused chunk-256 forwards and the dgrad have no wide
  // instances and run the 32-column kernel on the grid cut for gcolt, so
  // with NCOL >= 64 output columns past 32 of each gcolt are never written.
  if (mode == SP_DGRAD || (fused && p.chunk == 256)) p.ncolt = 32;
  return p;
}

// WB layout: [NCOL][kts][KT_PAD], k inside a channel tile = tap*CTILE + local
// channel (CTILE 1: just the tap); taps >= 27 and channels >= KCH are zero.
// Rows [NCOL, next multiple of 128) exist and are zero, so the widest column
// tile of the last grid row reads in bounds without a check.
// One launch writes every element straight from the bf16 weight
// w[Cout][Cin][27]: forward reads w[col][ch][tap], dgrad (KCH = Cout,
// NCOL = Cin) the tap-flipped transpose w[ch][col][26 - tap].
__global__ __launch_bounds__(256) void conv3d_spatial_prep_wb_kernel(
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

static torch::Tensor prep_wb(torch::Tensor w, int ncol, int KCH,
                             const SpatialPlan& p, bool dgrad) {
  const int kt_pad = (p.ctile * 27 + 31) / 32 * 32;
  const int kts = (KCH + p.ctile - 1) / p.ctile;
  const int kpad = kts * kt_pad;
  const int rows = (ncol + 127) / 128 * 128;
  TORCH_CHECK((int64_t)rows * kpad < (int64_t)1 << 31, "WB too large");
  auto wb = torch::empty({rows, (int64_t)kpad}, w.options());
  hipLaunchKernelGGL(conv3d_spatial_prep_wb_kernel,
                     dim3((rows * kpad + 255) / 256), dim3(256), 0,
                     current_stream(),
                     reinterpret_cast<const __bf16*>(w.data_ptr()),
                     reinterpret_cast<__bf16*>(wb.data_ptr()), ncol, KCH,
                     p.ctile, kt_pad, kpad, dgrad ? 1 : 0);
  return wb;
}

static void launch_spatial(torch::Tensor in, torch::Tensor wb,
                           torch::Tensor out, SpDims sd, int stride,
                           SpMode mode, const SpatialPlan& p,
                           const float* bn_ab = nullptr,
                           float* stats = nullptr) {
  const int oht = p.chunk / p.owt;
  const int wtiles = (sd.TW + p.owt - 1) / p.owt;
  const int htiles = (sd.TH + oht - 1) / oht;
  const int64_t nchunks =
      (int64_t)sd.N * ((sd.TD + p.dt - 1) / p.dt) * htiles * wtiles;
  dim3 grid((unsigned)nchunks, (sd.NCOL + p.gcolt - 1) / p.gcolt);
  auto s = current_stream();
  const __bf16* ip = reinterpret_cast<const __bf16*>(in.data_ptr());
  const __bf16* wp = reinterpret_cast<const __bf16*>(wb.data_ptr());
  __bf16* op = reinterpret_cast<__bf16*>(out.data_ptr());
  // launches instance <OWT, STRIDE, CTILE, CHUNK, FUSE_BN, SMODE, NCOLT, DT>
  auto K = [&](auto owt, auto st, auto ct, auto ch, auto fz, auto sm,
               auto nc, auto dt) {
    hipLaunchKernelGGL(
        (conv3d_spatial_kernel<decltype(owt)::value, decltype(st)::value,
                               decltype(ct)::value, decltype(ch)::value,
                               decltype(fz)::value, decltype(sm)::value,
                               decltype(nc)::value, decltype(dt)::value>),
        grid, dim3(256), 0, s, ip, wp, op, sd, nchunks, bn_ab, stats);
  };
  const IntC<1> dt1{};
  auto with_owt = [&](auto f) {
    if (p.owt == 32) f(IntC<32>{});
    else if (p.owt == 16) f(IntC<16>{});
    else f(IntC<8>{});
  };
  // f(FUSE_BN, SMODE) of the mode
  auto with_epilogue = [&](auto f) {
    if (mode == SP_FUSED_STATS) f(std::true_type{}, IntC<1>{});
    else if (mode == SP_FUSED) f(std::true_type{}, IntC<0>{});
    else f(std::false_type{}, IntC<0>{});
  };
  auto with_ncolt = [&](auto f) {
    if (p.ncolt == 128) f(IntC<128>{});
    else if (p.ncolt == 64) f(IntC<64>{});
    else f(IntC<32>{});
  };
  const std::false_type plain{};
  if (p.ctile == 1) {
    // single-channel (first-layer) instances: one 32-k-step covers the
    // whole 27-tap K, slab is [1][3][H2][W2]; plain staging, with or
    // without the epilogue statistics
    dispatch_bool(mode == SP_CTILE1_STATS, [&](auto st) {
      const IntC<decltype(st)::value ? 1 : 0> sm{};
      if (p.chunk == 64)
        K(IntC<8>{}, IntC<1>{}, IntC<1>{}, IntC<64>{}, plain, sm,
          IntC<32>{}, dt1);
      else
        with_owt([&](auto owt) {
          K(owt, IntC<1>{}, IntC<1>{}, IntC<256>{}, plain, sm, IntC<32>{},
            dt1);
        });
    });
  } else if (p.chunk == 512) {
    // plain (dgrad) and fused+stats (fwd) only
    dispatch_bool(mode == SP_FUSED_STATS, [&](auto fs) {
      K(IntC<32>{}, IntC<1>{}, IntC<16>{}, IntC<512>{}, fs,
        IntC<decltype(fs)::value ? 1 : 0>{}, IntC<32>{}, dt1);
    });
  } else if (p.chunk == 64 && p.dt > 1) {
    // whole-plane depth-blocked: every epilogue, one (DT, NCOLT) per stride
    TORCH_CHECK(stride == 1 ? (p.dt == 4 && p.ncolt == 64)
                            : (p.dt == 2 && p.ncolt == 128),
                "no depth-blocked instance for this plan");
    with_epilogue([&](auto fz, auto sm) {
      if (stride == 1)
        K(IntC<8>{}, IntC<1>{}, IntC<32>{}, IntC<64>{}, fz, sm, IntC<64>{},
          IntC<4>{});
      else
        K(IntC<8>{}, IntC<2>{}, IntC<16>{}, IntC<64>{}, fz, sm, IntC<128>{},
          IntC<2>{});
    });
  } else if (p.chunk == 64) {
    // every epilogue x {32, 64, 128} columns x stride
    with_epilogue([&](auto fz, auto sm) {
      with_ncolt([&](auto nc) {
        if (stride == 1)
          K(IntC<8>{}, IntC<1>{}, IntC<32>{}, IntC<64>{}, fz, sm, nc, dt1);
        else
          K(IntC<8>{}, IntC<2>{}, IntC<16>{}, IntC<64>{}, fz, sm, nc, dt1);
      });
    });
  } else if (stride == 2) {
    // chunk 128: every epilogue x {32, 64, 128} columns x OWT
    with_epilogue([&](auto fz, auto sm) {
      with_ncolt([&](auto nc) {
        with_owt([&](auto owt) {
          K(owt, IntC<2>{}, IntC<16>{}, IntC<128>{}, fz, sm, nc, dt1);
        });
      });
    });
  } else if (p.ncolt == 64) {
    // wide chunk-256: plain forward only (the fused-stats wide form lost,
    // docs/KERNELS.md)
    with_owt([&](auto owt) {
      K(owt, IntC<1>{}, IntC<32>{}, IntC<256>{}, plain, IntC<0>{},
        IntC<64>{}, dt1);
    });
  } else {
    with_epilogue([&](auto fz, auto sm) {
      with_owt([&](auto owt) {
        K(owt, IntC<1>{}, IntC<32>{}, IntC<256>{}, fz, sm, IntC<32>{}, dt1);
      });
    });
  }
}

// shared body of the two forward entry points: {out, stats-or-undefined}
static std::vector<torch::Tensor> spatial_fwd(torch::Tensor x,
                                              torch::Tensor w, int stride,
                                              SpMode mode,
                                              torch::Tensor bn_ab) {
  CHECK_GPU(x);
  auto xc = x.contiguous();
  auto wc = w.to(torch::kBFloat16).contiguous();
  TORCH_CHECK(xc.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(stride == 1 || stride == 2);
  torch::Tensor ab, stats;
  if (mode == SP_FUSED || mode == SP_FUSED_STATS) {
    ab = bn_ab.to(torch::kFloat32).contiguous();
    TORCH_CHECK(ab.numel() == 2 * x.size(1), "bn_ab must be [Cin,2]");
  }
  auto odim = [&](int i) { return ((int)xc.size(i) + 2 - 3) / stride + 1; };
  SpDims sd = make_spdims(xc, (int)wc.size(0), odim(2), odim(3), odim(4));
  const SpatialPlan plan = plan_spatial(sd, stride, mode);
  TORCH_CHECK(wc.size(1) == sd.KCH, "weight/input channel mismatch");
  auto wb = prep_wb(wc, sd.NCOL, sd.KCH, plan, false);
  sd.Kpad = (int)wb.size(1);
  auto out = torch::empty({sd.N, sd.NCOL, sd.TD, sd.TH, sd.TW},
                          xc.options());
  // stats[64][Cout][2]: hash-sliced partial sums; callers fold with sum(0)
  if (mode == SP_FUSED_STATS || mode == SP_CTILE1_STATS)
    stats = torch::zeros({64, sd.NCOL, 2},
                         xc.options().dtype(torch::kFloat32));
  launch_spatial(xc, wb, out, sd, stride, mode, plan,
                 ab.defined() ? ab.data_ptr<float>() : nullptr,
                 stats.defined() ? stats.data_ptr<float>() : nullptr);
  return {out, stats};
}

// ctile_opt: 0 = the default tiling; 1 = the CTILE=1 single-channel
// instances (stride 1; ignored at stride 2).
torch::Tensor conv3d_fwd_spatial(torch::Tensor x, torch::Tensor w,
                                 int64_t stride, int64_t ctile_opt,
                                 c10::optional<torch::Tensor> bn_ab_opt) {
  torch::Tensor bn_ab = bn_ab_opt.value_or(torch::Tensor());
  TORCH_CHECK(ctile_opt == 0 || ctile_opt == 1, "ctile_opt must be 0 or 1");
  const bool fuse = bn_ab.defined() && bn_ab.numel() > 0;
  TORCH_CHECK(!fuse || ctile_opt == 0, "fused BN requires default tiling");
  const SpMode mode = fuse ? SP_FUSED
                           : (ctile_opt == 1 && stride == 1 ? SP_CTILE1
                                                            : SP_PLAIN);
  return spatial_fwd(x, w, (int)stride, mode, bn_ab)[0];
}

// fused fwd + epilogue BN statistics: returns {out, stats[64][Cout][2]}
std::vector<torch::Tensor> conv3d_fwd_spatial_stats(
    torch::Tensor x, torch::Tensor w, int64_t stride,
    c10::optional<torch::Tensor> bn_ab_opt) {
  torch::Tensor bn_ab = bn_ab_opt.value_or(torch::Tensor());
  TORCH_CHECK(bn_ab.defined() && bn_ab.numel() > 0,
              "stats form requires the fused-BN path");
  return spatial_fwd(x, w, (int)stride, SP_FUSED_STATS, bn_ab);
}

// single-channel-tile stride-1 forward (the first layer) + epilogue BN
// statistics: out is bitwise conv3d_fwd_spatial(x, w, 1, 1)
std::vector<torch::Tensor> conv3d_fwd_ci1_stats(torch::Tensor x,
                                                torch::Tensor w) {
  return spatial_fwd(x, w, 1, SP_CTILE1_STATS, torch::Tensor());
}

torch::Tensor conv3d_dgrad_spatial(torch::Tensor go, torch::Tensor w,
                                   std::vector<int64_t> in_shape) {
  CHECK_GPU(go);
  auto g = go.to(torch::kBFloat16).contiguous();
  auto wc = w.to(torch::kBFloat16).contiguous();
  SpDims sd = make_spdims(g, (int)in_shape[1], (int)in_shape[2],
                          (int)in_shape[3], (int)in_shape[4]);
  TORCH_CHECK(wc.size(0) == sd.KCH && wc.size(1) == sd.NCOL,
              "weight/grad channel mismatch");
  const SpatialPlan plan = plan_spatial(sd, 1, SP_DGRAD);
  auto wb = prep_wb(wc, sd.NCOL, sd.KCH, plan, true);
  sd.Kpad = (int)wb.size(1);
  // On the under-covered grid (plan_spatial, docs/NEXT.md) the kernel never
  // writes the dx columns past 32 of each gcolt. Until that is fixed they
  // are at least zero, not whatever the allocator hands back: a training
  // run must not depend on which tensors were freed before it.
  const bool undercovered = plan.ncolt < plan.gcolt && sd.NCOL > plan.ncolt;
  auto dx = undercovered ? torch::zeros(in_shape, g.options())
                         : torch::empty(in_shape, g.options());
  launch_spatial(g, wb, dx, sd, 1, SP_DGRAD, plan);
  return dx;
}

// ---------------------------------------------------------------------------
// Stride-2 DGRAD: all 8 parity classes of a tile from ONE staged go slab.
// dx decomposes by (id,ih,iw) mod 2 into 8 dense sub-problems ("classes");
// per axis, dx index i = 2i' + p takes
//   p = 0: tap k = 1 at go index i'
//   p = 1: tap k = 0 at go index i' + 1, and tap k = 2 at go index i'
// so the 27 taps read the go window at only 8 shifts (dod,doh,dow) in
// {0,1}^3. A block owns OHT x OWT sub-grid positions at DT sub-grid depths
// from id' (a 2*DT x 2*OHT x 2*OWT brick of dx; OHT = 128 / (OWT*DT)) and
// stages the channel-innermost slab
// [DT+1][OHT+1][OWT+1 (row pitch OWT+4)][32 co] once per 32-co tile. K runs
// (tap, local co): a k-step of 32 is one tap, and lane (row, kg) reads its
// 8 k as one 16-byte LDS word at lanew[dow] + (shift, fragment) constants.
// Each shifted fragment is read once and multiplied into every class that
// has a tap at that shift: per wave 8 x 4 A reads and 27 B loads feed
// 27 x 4 = 108 MFMAs on 8 x 4 accumulator fragments (128 registers).
// A lane holds the c = 0 and c = 1 accumulators of the same 4 iw', which
// are 8 consecutive dx elements of one row: one 16-byte store.
// DT = 2 (OWT 8 only) is the depth-blocked form for 8-wide sub-grid planes:
// the 128 m are the whole 8 x 8 plane at TWO sub-grid depths id', id' + 1,
// wave row wm owning depth plane wm. The slab is [3][9][pitch 12][32 co],
// shift dod of plane p reads slab plane p + dod, and the fragment offsets
// inside a plane are those of <8>. With an odd sub-grid depth the last
// block's second plane is past the end: its go planes stage as zeros
// (od >= D) and its stores are cut by id >= TD.
// ---------------------------------------------------------------------------
// class = parity bits (a, b, c) of (id, ih, iw), shift = (dod, doh, dow),
// both packed depth-major into 3 bits
__host__ __device__ constexpr bool s2_feeds(int cls, int s) {
  return (s & ~cls) == 0;  // only odd-parity axes have a shifted tap
}

__host__ __device__ constexpr int s2_tap(int cls, int s) {
  int tap = 0;
  for (int ax = 2; ax >= 0; --ax) {
    const int par = (cls >> ax) & 1, sh = (s >> ax) & 1;
    tap = tap * 3 + (par ? (sh ? 0 : 2) : 1);
  }
  return tap;
}

// WB slot of (class, shift): class-major, shifts ascending inside a class
__host__ __device__ constexpr int s2_slot(int cls, int s) {
  int n = 0;
  for (int c2 = 0; c2 < cls; ++c2)
    n += 1 << (((c2 >> 2) & 1) + ((c2 >> 1) & 1) + (c2 & 1));
  for (int s2 = 0; s2 < s; ++s2) n += s2_feeds(cls, s2) ? 1 : 0;
  return n;
}

struct S2TapTable { int tap[27]; };
constexpr S2TapTable s2_tap_table() {
  S2TapTable t{};
  for (int cls = 0; cls < 8; ++cls)
    for (int s = 0; s < 8; ++s)
      if (s2_feeds(cls, s)) t.tap[s2_slot(cls, s)] = s2_tap(cls, s);
  return t;
}

template <int OWT, int DT = 1>
__global__ __launch_bounds__(256, 2) void conv3d_dgrad_s2_sp_kernel(
    const __bf16* __restrict__ go, const __bf16* __restrict__ wb,
    __bf16* __restrict__ dx, SpDims sd) {
  static_assert(DT == 1 || DT == 2, "a wave row owns one depth plane");
  constexpr int OHT = 128 / (OWT * DT);
  constexpr int PM = OHT * OWT;  // m per sub-grid depth plane
  constexpr int W2 = OWT + 4;  // OWT+1 used; a row pitch of 4k positions
                               // keeps the OWT-8 two-row fragments off
                               // each other's banks
  constexpr int H2 = OHT + 1;
  // the 4 waves tile the 128 m x 32 columns as 2 x 2: a wave owns 4
  // m-fragments of ONE column fragment, so each 16-byte B load from L2
  // feeds 4 MFMAs (2 m-fragments x 2 column fragments would load twice the
  // B bytes per MFMA; every wave of a block reads the same WB rows)
  constexpr int NCF = 1;           // column fragments per wave
  constexpr int WCOL = 2 / NCF;    // waves side by side over the columns
  constexpr int MPW = 2 * WCOL;    // m-fragments per wave
  static_assert(PM % (MPW * 16) == 0, "a wave's m stay inside one plane");
  __shared__ __attribute__((aligned(16))) __bf16 sG[(DT + 1) * H2 * W2 * 32];

  // the CTILE 32 layout of conv3d_spatial_kernel: 64 B per position, 16-byte
  // chunk ^= 2*bit2(w). Rows of a fragment are dense in w (or whole rows
  // apart), the stride-1 case, so the four 16-lane groups of a 16-byte read
  // land on distinct banks the same way.
  auto slab_off = [](int p, int h, int w, int cl) -> int {
    const int chunk = (cl >> 3) ^ (((w >> 2) & 1) << 1);
    return ((p * H2 + h) * W2 + w) * 32 + chunk * 8 + (cl & 7);
  };

  const int ncol0 = blockIdx.y * 32;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int row = lane & 15, kg = lane >> 4;
  const int wm = wave / WCOL, wj = wave % WCOL;

  // sub-grid extents of the even classes; the odd ones are at most one
  // shorter and are cut by the epilogue guards
  const int Dq = (sd.TD + 1) >> 1;
  const int Hq = (sd.TH + 1) >> 1;
  const int Wq = (sd.TW + 1) >> 1;
  const int wtiles = (Wq + OWT - 1) / OWT;
  const int htiles = (Hq + OHT - 1) / OHT;

  int64_t t = blockIdx.x;
  const int wt = (int)(t % wtiles);
  t /= wtiles;
  const int ht = (int)(t % htiles);
  t /= htiles;
  const int dtiles = (Dq + DT - 1) / DT;
  const int tdp = (int)(t % dtiles) * DT;  // id' (sub-grid d) of plane 0
  const int n = (int)(t / dtiles);
  const int oh0 = ht * OHT, ow0 = wt * OWT;

  f32x4 acc[8][MPW][NCF];
#pragma unroll
  for (int cls = 0; cls < 8; ++cls)
#pragma unroll
    for (int i = 0; i < MPW; ++i)
#pragma unroll
      for (int j = 0; j < NCF; ++j) acc[cls][i][j] = {0.f, 0.f, 0.f, 0.f};

  // A address = lanew[dow] + (shift plane/row, fragment) constants: the
  // swizzle bit of w depends on (row, dow) only, fragments start 16 columns
  // or whole rows apart
  const int m_l = wm * (MPW * 16) + row;
  int lanew[2];
#pragma unroll
  for (int dow = 0; dow < 2; ++dow)
    lanew[dow] = slab_off(DT == 1 ? 0 : m_l / PM,
                          (DT == 1 ? m_l : m_l % PM) / OWT,
                          m_l % OWT + dow, kg * 8);
  auto frag_off = [](int i) -> int {
    return (((i * 16) / OWT) * W2 + (i * 16) % OWT) * 32;
  };

  // B: lane (col = row, kg) reads 8 consecutive local co of its ci row;
  // tap slot g of co tile kt sits at (kt*27 + g)*32. WB has zero rows up to
  // the next multiple of 32 ci, so a ragged column tile needs no check.
  const int kts = (sd.KCH + 31) / 32;        // co tiles
  const __bf16* wbl =
      wb + (int64_t)(ncol0 + wj * NCF * 16 + row) * sd.Kpad + kg * 8;

  const int64_t OHW = (int64_t)sd.H * sd.W;  // go plane (input-side dims)
  const int64_t go_n = (int64_t)n * sd.KCH * sd.D * OHW;
  constexpr int NV = OWT / 8;   // 8-column vectors per interior row
  // a thread carries one 8-column vector of 4 adjacent co and stores 8
  // interleaved 8-byte words, as the stride-1 staging does
  constexpr int CG = 4, NCG = 32 / CG;
  constexpr int NITEM = (DT + 1) * H2 * NV * NCG;
  const bool wvec = (sd.W & 7) == 0;  // rows 16-byte aligned

  for (int kt = 0; kt < kts; ++kt) {
    if (kt) __syncthreads();
    for (int it = tid; it < NITEM; it += 256) {
      const int cg = it % NCG;
      const int v = (it / NCG) % NV;
      const int hrow = (it / (NCG * NV)) % H2;
      const int p = it / (NCG * NV * H2);
      const int od = tdp + p;
      const int oh = oh0 + hrow;
      const int ow = ow0 + v * 8;
      const bool row_ok = od < sd.D && oh < sd.H;
      __bf16 tv[CG][8];
#pragma unroll
      for (int cc = 0; cc < CG; ++cc) {
        const int ch = kt * 32 + cg * CG + cc;
#pragma unroll
        for (int j = 0; j < 8; ++j) tv[cc][j] = (__bf16)0.f;
        if (row_ok && ch < sd.KCH) {
          const __bf16* src = go + go_n + ((int64_t)ch * sd.D + od) * OHW +
                              (int64_t)oh * sd.W;
          if (wvec && ow + 8 <= sd.W) {
            const bf16x8 vec = *reinterpret_cast<const bf16x8*>(src + ow);
#pragma unroll
            for (int j = 0; j < 8; ++j) tv[cc][j] = vec[j];
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (ow + j < sd.W) tv[cc][j] = src[ow + j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bf16x4 o;
#pragma unroll
        for (int cc = 0; cc < CG; ++cc) o[cc] = tv[cc][j];
        *reinterpret_cast<bf16x4*>(
            sG + slab_off(p, hrow, v * 8 + j, cg * CG)) = o;
      }
    }
    // the +1 column: one element per (plane, row, co)
    for (int it = tid; it < (DT + 1) * H2 * 32; it += 256) {
      const int cl = it % 32;
      const int hrow = (it / 32) % H2;
      const int p = it / (32 * H2);
      const int od = tdp + p;
      const int oh = oh0 + hrow;
      const int ow = ow0 + OWT;
      const int ch = kt * 32 + cl;
      __bf16 val = (__bf16)0.f;
      if (od < sd.D && oh < sd.H && ow < sd.W && ch < sd.KCH)
        val = go[go_n + ((int64_t)ch * sd.D + od) * OHW +
                 (int64_t)oh * sd.W + ow];
      sG[slab_off(p, hrow, OWT, cl)] = val;
    }
    __syncthreads();

    // ---- 8 shifts; each feeds the classes that have a tap there --------
    const __bf16* wbk = wbl + (int64_t)kt * (27 * 32);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int lk =
          lanew[s & 1] + ((s >> 2) * H2 + ((s >> 1) & 1)) * W2 * 32;
      bf16x8 afrag[MPW];
#pragma unroll
      for (int i = 0; i < MPW; ++i)
        afrag[i] = *reinterpret_cast<const bf16x8*>(sG + lk + frag_off(i));
#pragma unroll
      for (int cls = 0; cls < 8; ++cls) {
        if (!s2_feeds(cls, s)) continue;
        bf16x8 bfrag[NCF];
#pragma unroll
        for (int j = 0; j < NCF; ++j)
          bfrag[j] = *reinterpret_cast<const bf16x8*>(
              wbk + (int64_t)j * 16 * sd.Kpad + s2_slot(cls, s) * 32);
#pragma unroll
        for (int i = 0; i < MPW; ++i)
#pragma unroll
          for (int j = 0; j < NCF; ++j)
            acc[cls][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag[i], bfrag[j], acc[cls][i][j], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: dx[n][ci][2*id'+a][2*ih'+b][2*iw'+c] ------------------
  // a lane's 4 consecutive m are 4 consecutive iw'; with both c classes
  // they are 8 consecutive dx elements: one 16-byte store when the rows are
  // 16-byte aligned (TW % 8 == 0; iw is a multiple of 8, so iw + 8 <= TW)
  const bool pack8 = (sd.TW & 7) == 0;
  const int64_t THW = (int64_t)sd.TH * sd.TW;
  const int64_t dx_n = (int64_t)n * sd.NCOL * sd.TD * THW;
  const int ccol = lane & 15;
  const int crow0 = (lane >> 4) * 4;
#pragma unroll
  for (int ab = 0; ab < 4; ++ab) {
    // a wave's m all lie in depth plane wm * MPW * 16 / PM of the block
    const int id =
        2 * (tdp + (DT == 1 ? 0 : (wm * MPW * 16) / PM)) + (ab >> 1);
    if (id >= sd.TD) continue;
#pragma unroll
    for (int i = 0; i < MPW; ++i) {
#pragma unroll
      for (int j = 0; j < NCF; ++j) {
        const int col = ncol0 + (wj * NCF + j) * 16 + ccol;
        const int m = (wm * MPW + i) * 16 + crow0;
        const int ih = 2 * (oh0 + (DT == 1 ? m : m % PM) / OWT) + (ab & 1);
        const int iw = 2 * (ow0 + m % OWT);
        if (col >= sd.NCOL || ih >= sd.TH || iw >= sd.TW) continue;
        __bf16* drow = dx + dx_n + ((int64_t)col * sd.TD + id) * THW +
                       (int64_t)ih * sd.TW;
        if (pack8) {
          bf16x8 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            o[2 * r] = (__bf16)acc[2 * ab][i][j][r];
            o[2 * r + 1] = (__bf16)acc[2 * ab + 1][i][j][r];
          }
          *reinterpret_cast<bf16x8*>(drow + iw) = o;
          continue;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (iw + 2 * r < sd.TW)
            drow[iw + 2 * r] = (__bf16)acc[2 * ab][i][j][r];
          if (iw + 2 * r + 1 < sd.TW)
            drow[iw + 2 * r + 1] = (__bf16)acc[2 * ab + 1][i][j][r];
        }
      }
    }
  }
}

// WB[ci][co tile][27 slots][32 local co], one launch straight from
// w[Cout][Cin][27]: slot s2_slot(class, shift) holds tap s2_tap(class,
// shift). co >= Cout and the rows [Cin, next multiple of 32) are zero.
__global__ __launch_bounds__(256) void conv3d_dgrad_s2_prep_wb_kernel(
    const __bf16* __restrict__ w, __bf16* __restrict__ wb, int cin, int cout,
    int kpad, int total) {
  constexpr S2TapTable tab = s2_tap_table();
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ci = idx / kpad, k = idx - ci * kpad;
  const int g = k >> 5;  // kt*27 + slot
  const int co = (g / 27) * 32 + (k & 31);
  __bf16 v = (__bf16)0.f;
  if (ci < cin && co < cout)
    v = w[((int64_t)co * cin + ci) * 27 + tab.tap[g % 27]];
  wb[idx] = v;
}

torch::Tensor conv3d_dgrad_s2_spatial(torch::Tensor go, torch::Tensor w,
                                      std::vector<int64_t> in_shape) {
  CHECK_GPU(go);
  auto g = go.to(torch::kBFloat16).contiguous();
  auto wc = w.to(torch::kBFloat16).contiguous();
  const int Cout = (int)wc.size(0), Cin = (int)wc.size(1);
  TORCH_CHECK(in_shape.size() == 5 && in_shape[0] == g.size(0) &&
              in_shape[1] == Cin && g.size(1) == Cout,
              "weight/grad/input shape mismatch");
  SpDims sd = make_spdims(g, Cin, (int)in_shape[2], (int)in_shape[3],
                          (int)in_shape[4]);
  for (int i = 2; i < 5; ++i)
    TORCH_CHECK(g.size(i) == (in_shape[i] + 1) / 2,
                "go is not the stride-2 output of in_shape");

  const int kts = (Cout + 31) / 32;
  const int kpad = kts * 27 * 32;
  const int rows = (Cin + 31) / 32 * 32;
  TORCH_CHECK((int64_t)rows * kpad < (int64_t)1 << 31, "WB too large");
  auto wb = torch::empty({rows, (int64_t)kpad}, wc.options());
  auto s = current_stream();
  hipLaunchKernelGGL(conv3d_dgrad_s2_prep_wb_kernel,
                     dim3((rows * kpad + 255) / 256), dim3(256), 0, s,
                     reinterpret_cast<const __bf16*>(wc.data_ptr()),
                     reinterpret_cast<__bf16*>(wb.data_ptr()), Cin, Cout,
                     kpad, rows * kpad);
  sd.Kpad = kpad;

  auto dx = torch::empty(in_shape, g.options());
  const int Wq = (sd.TW + 1) >> 1, Hq = (sd.TH + 1) >> 1;
  const int Dq = (sd.TD + 1) >> 1;
  const int OWT = Wq % 32 == 0 ? 32 : (Wq % 16 == 0 ? 16 : 8);
  // a whole small plane per block, two sub-grid depths deep
  const int DT = s2_dgrad_depth_blocked(Hq, Wq) ? 2 : 1;
  const int OHT = 128 / (OWT * DT);
  const int wtiles = (Wq + OWT - 1) / OWT;
  const int htiles = (Hq + OHT - 1) / OHT;
  const int64_t nchunks =
      (int64_t)sd.N * ((Dq + DT - 1) / DT) * htiles * wtiles;
  TORCH_CHECK(nchunks < (int64_t)1 << 31, "grid too large");
  dim3 grid((unsigned)nchunks, (Cin + 31) / 32);
  auto L = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s,
                       reinterpret_cast<const __bf16*>(g.data_ptr()),
                       reinterpret_cast<const __bf16*>(wb.data_ptr()),
                       reinterpret_cast<__bf16*>(dx.data_ptr()), sd);
  };
  if (DT == 2) L(conv3d_dgrad_s2_sp_kernel<8, 2>);
  else if (OWT == 32) L(conv3d_dgrad_s2_sp_kernel<32>);
  else if (OWT == 16) L(conv3d_dgrad_s2_sp_kernel<16>);
  else L(conv3d_dgrad_s2_sp_kernel<8>);
  return dx;
}
