// Nearest-2x upsample followed by a 3x3x3/pad-1 conv, without the upsampled
// tensor: upconv3d_fwd_kernel computes all 8 output parity classes of a
// brick from ONE staged slab of the low-resolution input.
//
// Per axis, output index o = 2i' + p; tap t in {0,1,2} reads upsampled index
// o + t - 1, that is low-res index i' + floor((p + t - 1) / 2):
//   p = 0: shift -1 <- w[0]          shift 0 <- w[1] + w[2]
//   p = 1: shift  0 <- w[0] + w[1]   shift +1 <- w[2]
// In 3D each class is a dense 2x2x2 conv of the low-res input with summed
// weights: 8 classes x 8 shifts = 64 (class, shift) slots over 27 distinct
// shifts, against 8 x 27 = 216 for conv-after-upsample. The conv's zero
// padding of the upsampled tensor (indices -1 and 2D) is the zero halo of the
// low-res slab (indices -1 and D), so no border case differs.
//
// The mirror image of conv3d_dgrad_s2_sp_kernel (conv3d_spatial.hip): there 8
// shifts feed 27 (class, tap) pairs, here 27 shifts feed 64.
#include "common.h"

#include <hip/hip_bf16.h>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// No kernel of this file uses the packed-fp32 VALU forms (v_pk_add_f32 /
// v_pk_mul_f32 / v_pk_fma_f32). Only fold2_sum3d_kernel has fp32 VALU
// arithmetic the compiler would pack: with this attribute its 32 brick adds
// stay v_add_f32, in a kernel bound by its loads. The other kernels compile
// to the same code with or without it and do not carry it (on the MFMA
// kernel it would keep its lambdas from inlining).
#if defined(__HIP_DEVICE_COMPILE__)
#define UP_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define UP_NO_PK_F32
#endif

struct UpDims {
  int N, Cin, Cout;
  int D, H, W;  // low-res input; the output is 2D x 2H x 2W
  int kts;      // 32-channel ci tiles
};

// ---- the (class, shift) algebra, per axis and packed ----------------------
// class = parity bits (a, b, c) of (od, oh, ow) packed depth-major into 3
// bits; shift = slab offsets (sd, sh, sw) in {0,1,2}^3 packed sd*9 + sh*3 +
// sw, slab offset s being low-res offset s - 1.

// taps t (bitmask) of parity p that read low-res offset s - 1
__host__ __device__ constexpr int up_tapmask_ax(int p, int s) {
  int mask = 0;
  for (int t = 0; t < 3; ++t)
    if ((p + t - 1 + 2) / 2 - 1 == s - 1) mask |= 1 << t;  // floor((p+t-1)/2)
  return mask;
}

__host__ __device__ constexpr bool up_feeds(int cls, int s) {
  return up_tapmask_ax((cls >> 2) & 1, s / 9) != 0 &&
         up_tapmask_ax((cls >> 1) & 1, (s / 3) % 3) != 0 &&
         up_tapmask_ax(cls & 1, s % 3) != 0;
}

// WB slot of (class, shift): class-major; inside a class the 8 shifts that
// feed it, (s - p) in {0,1} per axis, depth-major
__host__ __device__ constexpr int up_slot(int cls, int s) {
  return cls * 8 + ((s / 9 - ((cls >> 2) & 1)) << 2) +
         (((s / 3) % 3 - ((cls >> 1) & 1)) << 1) + (s % 3 - (cls & 1));
}

// the shift that tap (td*9 + th*3 + tw) of class cls reads: per axis
// floor((p + t - 1) / 2) + 1, the index up_tapmask_ax tests
__host__ __device__ constexpr int up_shift_of(int cls, int tap) {
  return ((((cls >> 2) & 1) + tap / 9 + 1) / 2) * 9 +
         ((((cls >> 1) & 1) + (tap / 3) % 3 + 1) / 2) * 3 +
         ((cls & 1) + tap % 3 + 1) / 2;
}

// slot -> 27-bit set of the taps (td*9 + th*3 + tw) it sums
struct UpTapTable { unsigned taps[64]; };
constexpr UpTapTable up_tap_table() {
  UpTapTable t{};
  for (int cls = 0; cls < 8; ++cls)
    for (int s = 0; s < 27; ++s) {
      if (!up_feeds(cls, s)) continue;
      const int md = up_tapmask_ax((cls >> 2) & 1, s / 9);
      const int mh = up_tapmask_ax((cls >> 1) & 1, (s / 3) % 3);
      const int mw = up_tapmask_ax(cls & 1, s % 3);
      unsigned set = 0;
      for (int tap = 0; tap < 27; ++tap)
        if (((md >> (tap / 9)) & 1) && ((mh >> ((tap / 3) % 3)) & 1) &&
            ((mw >> (tap % 3)) & 1))
          set |= 1u << tap;
      t.taps[up_slot(cls, s)] = set;
    }
  return t;
}

// ---------------------------------------------------------------------------
// A block owns OHT x OWT low-res positions at DT low-res depths from d0 (a
// 2*DT x 2*OHT x 2*OWT brick of the output; OHT = 128 / (OWT*DT)) and one
// 32-column tile of Cout. Per 32-ci tile it stages the channel-innermost slab
// [DT+2][OHT+2][OWT+2 (row pitch OWT+4)][32 ci], slab coordinate = low-res
// coordinate + 1 - tile origin, halo and everything past the tensor zero.
// K runs (shift, local ci): a k-step of 32 is one shift, and lane (row, kg)
// reads its 8 k as one 16-byte LDS word at lanew[sw] + (shift plane/row,
// fragment) constants. The loop runs over the 27 shifts; each shifted A
// fragment is read once and multiplied into every class it feeds: per wave
// 27 x 4 A reads and 64 B loads feed 64 x 4 = 256 MFMAs on 8 x 4 accumulator
// fragments (128 registers).
// The slab is conv3d_spatial_kernel's CTILE-32 stride-1 slab (64 B per
// position, 16-byte chunk ^= 2*bit2(w), pitch OWT+4, w shifts 0..2, fragments
// 16 columns or whole rows apart), so its A reads land on the banks exactly
// as that kernel's do: the four 16-lane groups of a ds_read_b128 on distinct
// banks for OWT 32, 16 and 8.
// The 4 waves tile 128 m x 32 columns as 2 x 2, a wave owning 4 m-fragments
// of ONE column fragment, so each 16-byte B load feeds 4 MFMAs.
// A lane holds the c = 0 and c = 1 accumulators of the same 4 iw', which are
// 8 consecutive output elements of one row: one 16-byte store.
// DT = 2 (OWT 8 only): the 128 m are a whole 8 x 8 plane at TWO low-res
// depths, wave row wm owning depth plane wm; the slab has 4 planes and shift
// sd of plane p reads slab plane p + sd. With an odd D the last block's
// second plane is past the end: it stages zeros and stores nothing.
// ---------------------------------------------------------------------------
template <int OWT, int DT = 1>
__global__ __launch_bounds__(256, 2) void upconv3d_fwd_kernel(
    const __bf16* __restrict__ x, const __bf16* __restrict__ wb,
    __bf16* __restrict__ out, UpDims ud, int xvec) {
  static_assert(DT == 1 || DT == 2, "a wave row owns one depth plane");
  constexpr int OHT = 128 / (OWT * DT);
  constexpr int PM = OHT * OWT;  // m per low-res depth plane
  constexpr int W2 = OWT + 4;    // OWT+2 used; see the bank note above
  constexpr int H2 = OHT + 2;
  constexpr int P2 = DT + 2;
  constexpr int MPW = 4;         // m-fragments per wave
  static_assert(PM % (MPW * 16) == 0, "a wave's m stay inside one plane");
  __shared__ __attribute__((aligned(16))) __bf16 sX[P2 * H2 * W2 * 32];

  auto slab_off = [](int p, int h, int w, int cl) -> int {
    const int chunk = (cl >> 3) ^ (((w >> 2) & 1) << 1);
    return ((p * H2 + h) * W2 + w) * 32 + chunk * 8 + (cl & 7);
  };

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int row = lane & 15, kg = lane >> 4;
  const int wm = wave >> 1, wj = wave & 1;

  const int wtiles = (ud.W + OWT - 1) / OWT;
  const int htiles = (ud.H + OHT - 1) / OHT;
  const int dtiles = (ud.D + DT - 1) / DT;
  int64_t t = blockIdx.x;
  const int wt = (int)(t % wtiles);
  t /= wtiles;
  const int ht = (int)(t % htiles);
  t /= htiles;
  const int d0 = (int)(t % dtiles) * DT;
  const int n = (int)(t / dtiles);
  const int h0 = ht * OHT, w0 = wt * OWT;
  const int cot = blockIdx.y;  // 32-column tile of Cout

  f32x4 acc[8][MPW];
#pragma unroll
  for (int cls = 0; cls < 8; ++cls)
#pragma unroll
    for (int i = 0; i < MPW; ++i) acc[cls][i] = {0.f, 0.f, 0.f, 0.f};

  const int m_l = wm * (MPW * 16) + row;
  int lanew[3];
#pragma unroll
  for (int sw = 0; sw < 3; ++sw)
    lanew[sw] = slab_off(DT == 1 ? 0 : m_l / PM,
                         (DT == 1 ? m_l : m_l % PM) / OWT, m_l % OWT + sw,
                         kg * 8);
  auto frag_off = [](int i) -> int {
    return (((i * 16) / OWT) * W2 + (i * 16) % OWT) * 32;
  };

  // B: WB[co tile][ci tile][64 slots][32 local co][32 local ci]; lane
  // (col = row, kg) reads 8 consecutive local ci of its co, a wave 1 KB
  // contiguous. Padding rows and columns are zero: no check here.
  const __bf16* wbl = wb + (int64_t)cot * ud.kts * (64 * 1024) +
                      (wj * 16 + row) * 32 + kg * 8;

  const int64_t HW = (int64_t)ud.H * ud.W;
  const int64_t x_n = (int64_t)n * ud.Cin * ud.D * HW;
  constexpr int NV = OWT / 8;  // 8-column vectors per interior row
  // a thread carries one 8-column vector of 4 adjacent ci and stores 8
  // interleaved 8-byte words
  constexpr int CG = 4, NCG = 32 / CG;
  constexpr int NITEM = P2 * H2 * NV * NCG;

  for (int kt = 0; kt < ud.kts; ++kt) {
    if (kt) __syncthreads();
    for (int it = tid; it < NITEM; it += 256) {
      const int cg = it % NCG;
      const int v = (it / NCG) % NV;
      const int hrow = (it / (NCG * NV)) % H2;
      const int p = it / (NCG * NV * H2);
      const int id = d0 - 1 + p;
      const int ih = h0 - 1 + hrow;
      const int iw = w0 + v * 8;
      const bool row_ok = id >= 0 && id < ud.D && ih >= 0 && ih < ud.H;
      __bf16 tv[CG][8];
#pragma unroll
      for (int cc = 0; cc < CG; ++cc) {
        const int ch = kt * 32 + cg * CG + cc;
#pragma unroll
        for (int j = 0; j < 8; ++j) tv[cc][j] = (__bf16)0.f;
        if (row_ok && ch < ud.Cin) {
          const __bf16* src =
              x + x_n + ((int64_t)ch * ud.D + id) * HW + (int64_t)ih * ud.W;
          if (xvec && iw + 8 <= ud.W) {
            const bf16x8 vec = *reinterpret_cast<const bf16x8*>(src + iw);
#pragma unroll
            for (int j = 0; j < 8; ++j) tv[cc][j] = vec[j];
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (iw + j < ud.W) tv[cc][j] = src[iw + j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bf16x4 o;
#pragma unroll
        for (int cc = 0; cc < CG; ++cc) o[cc] = tv[cc][j];
        *reinterpret_cast<bf16x4*>(
            sX + slab_off(p, hrow, 1 + v * 8 + j, cg * CG)) = o;
      }
    }
    // the two halo columns: one element per (plane, row, side, ci)
    for (int it = tid; it < P2 * H2 * 2 * 32; it += 256) {
      const int cl = it % 32;
      const int side = (it / 32) & 1;
      const int hrow = (it / 64) % H2;
      const int p = it / (64 * H2);
      const int id = d0 - 1 + p;
      const int ih = h0 - 1 + hrow;
      const int iw = side ? w0 + OWT : w0 - 1;
      const int ch = kt * 32 + cl;
      __bf16 val = (__bf16)0.f;
      if (id >= 0 && id < ud.D && ih >= 0 && ih < ud.H && iw >= 0 &&
          iw < ud.W && ch < ud.Cin)
        val = x[x_n + ((int64_t)ch * ud.D + id) * HW + (int64_t)ih * ud.W +
                iw];
      sX[slab_off(p, hrow, side ? OWT + 1 : 0, cl)] = val;
    }
    __syncthreads();

    // ---- 27 shifts; each feeds the classes that have a slot there -------
    const __bf16* wbk = wbl + (int64_t)kt * (64 * 1024);
#pragma unroll
    for (int s = 0; s < 27; ++s) {
      const int lk = lanew[s % 3] + ((s / 9) * H2 + (s / 3) % 3) * W2 * 32;
      bf16x8 afrag[MPW];
#pragma unroll
      for (int i = 0; i < MPW; ++i)
        afrag[i] = *reinterpret_cast<const bf16x8*>(sX + lk + frag_off(i));
#pragma unroll
      for (int cls = 0; cls < 8; ++cls) {
        if (!up_feeds(cls, s)) continue;
        const bf16x8 bfrag =
            *reinterpret_cast<const bf16x8*>(wbk + up_slot(cls, s) * 1024);
#pragma unroll
        for (int i = 0; i < MPW; ++i)
          acc[cls][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[i], bfrag, acc[cls][i], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: out[n][co][2*id'+a][2*ih'+b][2*iw'+c] ------------------
  // a lane's 4 consecutive m are 4 consecutive iw' (a multiple of 4, so ow
  // is a multiple of 8): with both c classes 8 consecutive output elements,
  // one 16-byte store when the output rows are 16-byte aligned and iw' + 4
  // <= W; guarded scalars otherwise
  const int TD = 2 * ud.D, TH = 2 * ud.H, TW = 2 * ud.W;
  const bool pack8 = (ud.W & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int64_t THW = (int64_t)TH * TW;
  const int64_t out_n = (int64_t)n * ud.Cout * TD * THW;
  const int col = cot * 32 + wj * 16 + (lane & 15);
  const int crow0 = (lane >> 4) * 4;
  const int idp = d0 + (DT == 1 ? 0 : wm);  // a wave's m lie in one plane
  if (col >= ud.Cout || idp >= ud.D) return;
#pragma unroll
  for (int ab = 0; ab < 4; ++ab) {
    const int od = 2 * idp + (ab >> 1);
#pragma unroll
    for (int i = 0; i < MPW; ++i) {
      const int m = (wm * MPW + i) * 16 + crow0;
      const int ihp = h0 + (DT == 1 ? m : m % PM) / OWT;
      const int iwp = w0 + m % OWT;
      if (ihp >= ud.H || iwp >= ud.W) continue;
      __bf16* orow = out + out_n + ((int64_t)col * TD + od) * THW +
                     (int64_t)(2 * ihp + (ab & 1)) * TW;
      const int ow = 2 * iwp;
      if (pack8) {  // W % 4 == 0 and iwp % 4 == 0: iwp + 4 <= W
        bf16x8 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          o[2 * r] = (__bf16)acc[2 * ab][i][r];
          o[2 * r + 1] = (__bf16)acc[2 * ab + 1][i][r];
        }
        *reinterpret_cast<bf16x8*>(orow + ow) = o;
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (iwp + r < ud.W) {
          orow[ow + 2 * r] = (__bf16)acc[2 * ab][i][r];
          orow[ow + 2 * r + 1] = (__bf16)acc[2 * ab + 1][i][r];
        }
      }
    }
  }
}

// Slot weights, one launch straight from w[Cout][Cin][27]: slot
// up_slot(class, shift) holds the sum of its 1, 2, 4 or 8 taps, added in fp32
// and rounded once. co >= Cout and ci >= Cin are zero.
//   tr = 0 (forward): WB[co tile][ci tile][64 slots][32 local co][32 local ci]
//   tr = 1 (dgrad):   WBT[ci tile][co tile][64 slots][32 local ci][32 local co]
// inner_tiles is the tile count of the inner tile index (ci tiles for the
// forward, co tiles for the dgrad).
__global__ __launch_bounds__(256) void upconv3d_prep_wb_kernel(
    const __bf16* __restrict__ w, __bf16* __restrict__ wb, int cin, int cout,
    int inner_tiles, int total, int tr) {
  constexpr UpTapTable tab = up_tap_table();
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int lo = idx & 31, hi = (idx >> 5) & 31, slot = (idx >> 10) & 63;
  const int tile = idx >> 16;  // outer tile * inner_tiles + inner tile
  const int t_in = (tile % inner_tiles) * 32, t_out = (tile / inner_tiles) * 32;
  const int ci = tr ? t_out + hi : t_in + lo;
  const int co = tr ? t_in + lo : t_out + hi;
  float sum = 0.f;
  if (ci < cin && co < cout) {
    const __bf16* wp = w + ((int64_t)co * cin + ci) * 27;
    const unsigned set = tab.taps[slot];
#pragma unroll
    for (int tap = 0; tap < 27; ++tap)
      if ((set >> tap) & 1) sum += (float)wp[tap];
  }
  wb[idx] = (__bf16)sum;
}

// Launch geometry of the forward: which instance takes a low-res plane.
//   W % 32 == 0            <32>     4 x 32 tile
//   W % 16 == 0            <16>     8 x 16 tile
//   W == 8 and H <= 8      <8, 2>   whole plane, two low-res depths
//   everything else        <8>      16 x 8 tile (ragged W by the guarded path)
torch::Tensor upconv3d_fwd(torch::Tensor x, torch::Tensor w) {
  CHECK_GPU(x);
  CHECK_GPU(w);
  TORCH_CHECK(x.dim() == 5 && w.dim() == 5 && w.size(1) == x.size(1) &&
              w.size(2) == 3 && w.size(3) == 3 && w.size(4) == 3,
              "upconv3d_fwd: x[N,Cin,D,H,W], w[Cout,Cin,3,3,3]");
  auto xc = x.to(torch::kBFloat16).contiguous();
  auto wc = w.to(torch::kBFloat16).contiguous();
  UpDims ud;
  ud.N = (int)xc.size(0), ud.Cin = (int)xc.size(1), ud.Cout = (int)wc.size(0);
  ud.D = (int)xc.size(2), ud.H = (int)xc.size(3), ud.W = (int)xc.size(4);
  ud.kts = (ud.Cin + 31) / 32;
  const int cots = (ud.Cout + 31) / 32;
  auto out = torch::empty({ud.N, ud.Cout, 2 * ud.D, 2 * ud.H, 2 * ud.W},
                          xc.options());
  if (out.numel() == 0) return out;

  const int64_t wb_total = (int64_t)cots * ud.kts * 64 * 1024;
  TORCH_CHECK(wb_total < (int64_t)1 << 31, "WB too large");
  auto wbt = torch::empty({wb_total}, wc.options());
  auto s = current_stream();
  hipLaunchKernelGGL(upconv3d_prep_wb_kernel,
                     dim3((unsigned)((wb_total + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const __bf16*>(wc.data_ptr()),
                     reinterpret_cast<__bf16*>(wbt.data_ptr()), ud.Cin,
                     ud.Cout, ud.kts, (int)wb_total, 0);

  const int DT = (ud.W == 8 && ud.H <= 8) ? 2 : 1;
  const int OWT = ud.W % 32 == 0 ? 32 : (ud.W % 16 == 0 ? 16 : 8);
  const int OHT = 128 / (OWT * DT);
  const int64_t nblk = (int64_t)ud.N * ((ud.D + DT - 1) / DT) *
                       ((ud.H + OHT - 1) / OHT) * ((ud.W + OWT - 1) / OWT);
  TORCH_CHECK(nblk < (int64_t)1 << 31, "grid too large");
  // every instance covers exactly one 32-column tile of Cout per block
  dim3 grid((unsigned)nblk, cots);
  const int xvec = (ud.W % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(xc.data_ptr()) % 16 == 0)
                       ? 1 : 0;
  auto L = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s,
                       reinterpret_cast<const __bf16*>(xc.data_ptr()),
                       reinterpret_cast<const __bf16*>(wbt.data_ptr()),
                       reinterpret_cast<__bf16*>(out.data_ptr()), ud, xvec);
  };
  if (DT == 2) L(upconv3d_fwd_kernel<8, 2>);
  else if (OWT == 32) L(upconv3d_fwd_kernel<32>);
  else if (OWT == 16) L(upconv3d_fwd_kernel<16>);
  else L(upconv3d_fwd_kernel<8>);
  return out;
}

// ---------------------------------------------------------------------------
// Collapsed dgrad: the forward's transpose on the same 64 slots,
//   dx[i] = sum over (class, slot e, co) of go_cls[i + 1 - p - e] * WS^T,
// per axis with p the class parity and e = shift - p in {0, 1} the slot's
// sub-index: a parity-0 class gives its positions i and i+1, a parity-1 class
// i-1 and i. No full-resolution dx and no fold2_sum3d: the low-res tile is
// accumulated over all 64 slots x Cout and written once.
//
// A block owns the forward's tile (OHT x OWT positions at DT depths) and
// 32*CPW columns of Cin. go is de-interleaved by parity class into LDS class
// sub-slabs [DT+1][OHT+1][OWT+1 (pitch OWT+4)][32 co], channel-innermost with
// the forward's chunk swizzle; sub-slab coordinate u of class parity p is
// low-res position origin + u - p, high-res index 2*(origin + u) - p, so the
// A fragment of slot e sits at u = local position + 1 - e: the forward's
// read pattern with w shifts {0, 1}, same pitch, same banks. Two classes that
// differ in w parity are staged together: one 16-byte read of 8 high-res w
// is 4 elements of each, 4 adjacent co interleaved into 8-byte LDS words; the
// two columns no aligned vector reaches (u = 0 of c = 1, u = OWT of c = 0)
// are one element per thread. Per (co tile, class pair): stage, 2 x 8 slots.
// Two class sub-slabs are 46080 B (<32>, <16>), 52224 B (<8>), 41472 B
// (<8, 2>); all 8 would be about 170 KB.
// Waves tile 128 m x 32*CPW columns as 2 x 2; a wave owns 4 m-fragments of
// CPW column fragments (16*CPW accumulator registers). CPW = 2 when
// Cin > 32: each A fragment then feeds two MFMAs and go is read once per 64
// ci. B: WBT[ci tile][co tile][64][32 ci][32 co], lane (col, kg) reads 8
// consecutive co of its ci; padding is zero.
// A lane's 4 accumulator rows are 4 consecutive w of one ci: an 8-byte store.
// ---------------------------------------------------------------------------
template <int OWT, int DT, int CPW>
__global__ __launch_bounds__(256, 2) void upconv3d_dgrad_kernel(
    const __bf16* __restrict__ go, const __bf16* __restrict__ wbt,
    __bf16* __restrict__ dx, UpDims ud, int cots, int gvec, int dvec) {
  constexpr int OHT = 128 / (OWT * DT);
  constexpr int PM = OHT * OWT;
  constexpr int W2 = OWT + 4;  // OWT+1 used
  constexpr int H2 = OHT + 1;
  constexpr int P2 = DT + 1;
  constexpr int MPW = 4;
  constexpr int CLS = P2 * H2 * W2 * 32;  // one class sub-slab
  static_assert(2 * CLS * 2 <= 64 * 1024, "static LDS cap");
  __shared__ __attribute__((aligned(16))) __bf16 sG[2 * CLS];

  auto slab_off = [](int p, int h, int w, int cl) -> int {
    const int chunk = (cl >> 3) ^ (((w >> 2) & 1) << 1);
    return ((p * H2 + h) * W2 + w) * 32 + chunk * 8 + (cl & 7);
  };

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int row = lane & 15, kg = lane >> 4;
  const int wm = wave >> 1, wj = wave & 1;

  const int wtiles = (ud.W + OWT - 1) / OWT;
  const int htiles = (ud.H + OHT - 1) / OHT;
  const int dtiles = (ud.D + DT - 1) / DT;
  int64_t t = blockIdx.x;
  const int wt = (int)(t % wtiles);
  t /= wtiles;
  const int ht = (int)(t % htiles);
  t /= htiles;
  const int d0 = (int)(t % dtiles) * DT;
  const int n = (int)(t / dtiles);
  const int h0 = ht * OHT, w0 = wt * OWT;
  // the wave's 32-ci tile of WBT and its first column fragment inside it
  const int cit = blockIdx.y * CPW + (CPW == 2 ? wj : 0);
  const int cf0 = CPW == 2 ? 0 : wj;

  f32x4 acc[MPW][CPW];
#pragma unroll
  for (int i = 0; i < MPW; ++i)
#pragma unroll
    for (int j = 0; j < CPW; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int m_l = wm * (MPW * 16) + row;
  int lanew[2];
#pragma unroll
  for (int sw = 0; sw < 2; ++sw)
    lanew[sw] = slab_off(DT == 1 ? 0 : m_l / PM,
                         (DT == 1 ? m_l : m_l % PM) / OWT, m_l % OWT + sw,
                         kg * 8);
  auto frag_off = [](int i) -> int {
    return (((i * 16) / OWT) * W2 + (i * 16) % OWT) * 32;
  };

  const __bf16* wbl = wbt + (int64_t)cit * cots * (64 * 1024) +
                      (cf0 * 16 + row) * 32 + kg * 8;

  const int TD = 2 * ud.D, TH = 2 * ud.H, TW = 2 * ud.W;
  const int64_t THW = (int64_t)TH * TW;
  const int64_t go_n = (int64_t)n * ud.Cout * TD * THW;
  constexpr int NV = OWT / 4;  // 8-element vectors per high-res row
  constexpr int CG = 4, NCG = 32 / CG;
  constexpr int NITEM = P2 * H2 * NV * NCG;

  for (int cot = 0; cot < cots; ++cot) {
    for (int ab = 0; ab < 4; ++ab) {
      const int a = ab >> 1, b = ab & 1;
      if (cot | ab) __syncthreads();
      for (int it = tid; it < NITEM; it += 256) {
        const int cg = it % NCG;
        const int v = (it / NCG) % NV;
        const int hrow = (it / (NCG * NV)) % H2;
        const int p = it / (NCG * NV * H2);
        const int gd = 2 * (d0 + p) - a;
        const int gh = 2 * (h0 + hrow) - b;
        const int gw = 2 * w0 + v * 8;
        const bool row_ok = gd >= 0 && gd < TD && gh >= 0 && gh < TH;
        __bf16 tv[CG][8];
#pragma unroll
        for (int cc = 0; cc < CG; ++cc) {
          const int ch = cot * 32 + cg * CG + cc;
#pragma unroll
          for (int j = 0; j < 8; ++j) tv[cc][j] = (__bf16)0.f;
          if (row_ok && ch < ud.Cout) {
            const __bf16* src =
                go + go_n + ((int64_t)ch * TD + gd) * THW + (int64_t)gh * TW;
            if (gvec && gw + 8 <= TW) {
              const bf16x8 vec = *reinterpret_cast<const bf16x8*>(src + gw);
#pragma unroll
              for (int j = 0; j < 8; ++j) tv[cc][j] = vec[j];
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j)
                if (gw + j < TW) tv[cc][j] = src[gw + j];
            }
          }
        }
        // element j is class c = j & 1 at u = 4v + (j >> 1) + c
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          bf16x4 o;
#pragma unroll
          for (int cc = 0; cc < CG; ++cc) o[cc] = tv[cc][j];
          *reinterpret_cast<bf16x4*>(
              sG + (j & 1) * CLS +
              slab_off(p, hrow, v * 4 + (j >> 1) + (j & 1), cg * CG)) = o;
        }
      }
      // u = 0 of c = 1 (high-res 2*w0 - 1) and u = OWT of c = 0 (2*w0 + 2*OWT)
      for (int it = tid; it < P2 * H2 * 2 * 32; it += 256) {
        const int cl = it % 32;
        const int side = (it / 32) & 1;
        const int hrow = (it / 64) % H2;
        const int p = it / (64 * H2);
        const int gd = 2 * (d0 + p) - a;
        const int gh = 2 * (h0 + hrow) - b;
        const int gw = side ? 2 * w0 + 2 * OWT : 2 * w0 - 1;
        const int ch = cot * 32 + cl;
        __bf16 val = (__bf16)0.f;
        if (gd >= 0 && gd < TD && gh >= 0 && gh < TH && gw >= 0 && gw < TW &&
            ch < ud.Cout)
          val = go[go_n + ((int64_t)ch * TD + gd) * THW + (int64_t)gh * TW +
                   gw];
        sG[(side ? 0 : CLS) + slab_off(p, hrow, side ? OWT : 0, cl)] = val;
      }
      __syncthreads();

      const __bf16* wbk = wbl + (int64_t)cot * (64 * 1024);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int cls = ab * 2 + c;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int ed = e >> 2, eh = (e >> 1) & 1, ew = e & 1;
          const int lk = c * CLS + lanew[1 - ew] +
                         ((1 - ed) * H2 + (1 - eh)) * W2 * 32;
          bf16x8 afrag[MPW];
#pragma unroll
          for (int i = 0; i < MPW; ++i)
            afrag[i] = *reinterpret_cast<const bf16x8*>(sG + lk + frag_off(i));
          const int slot =
              up_slot(cls, (a + ed) * 9 + (b + eh) * 3 + (c + ew));
#pragma unroll
          for (int j = 0; j < CPW; ++j) {
            const bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
                wbk + slot * 1024 + j * (16 * 32));
#pragma unroll
            for (int i = 0; i < MPW; ++i)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  afrag[i], bfrag, acc[i][j], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- epilogue: dx[n][ci][id][ih][iw .. iw+3] ---------------------------
  const int64_t HW = (int64_t)ud.H * ud.W;
  const int idp = d0 + (DT == 1 ? 0 : wm);
  if (idp >= ud.D) return;
#pragma unroll
  for (int j = 0; j < CPW; ++j) {
    const int ci = cit * 32 + (cf0 + j) * 16 + row;
    if (ci >= ud.Cin) continue;
#pragma unroll
    for (int i = 0; i < MPW; ++i) {
      const int m = (wm * MPW + i) * 16 + kg * 4;
      const int ih = h0 + (DT == 1 ? m : m % PM) / OWT;
      const int iw = w0 + m % OWT;
      if (ih >= ud.H || iw >= ud.W) continue;
      __bf16* dst = dx + (((int64_t)n * ud.Cin + ci) * ud.D + idp) * HW +
                    (int64_t)ih * ud.W + iw;
      if (dvec) {  // W % 4 == 0 and iw % 4 == 0: iw + 4 <= W
        const bf16x4 o = {(__bf16)acc[i][j][0], (__bf16)acc[i][j][1],
                          (__bf16)acc[i][j][2], (__bf16)acc[i][j][3]};
        *reinterpret_cast<bf16x4*>(dst) = o;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (iw + r < ud.W) dst[r] = (__bf16)acc[i][j][r];
      }
    }
  }
}

static UpDims up_dims(const torch::Tensor& go, int64_t N, int64_t Cin,
                      int64_t D, int64_t H, int64_t W, const char* who) {
  TORCH_CHECK(go.dim() == 5 && go.size(0) == N && go.size(2) == 2 * D &&
              go.size(3) == 2 * H && go.size(4) == 2 * W,
              who, ": go[N,Cout,2D,2H,2W] against x[N,Cin,D,H,W]");
  TORCH_CHECK(N >= 1 && Cin >= 1 && go.size(1) >= 1 && D >= 1 && H >= 1 &&
              W >= 1, who, ": empty dimension");
  TORCH_CHECK(8 * D * H * W < ((int64_t)1 << 31), who, ": volume too large");
  UpDims ud;
  ud.N = (int)N, ud.Cin = (int)Cin, ud.Cout = (int)go.size(1);
  ud.D = (int)D, ud.H = (int)H, ud.W = (int)W;
  ud.kts = (ud.Cin + 31) / 32;
  return ud;
}

// bf16, contiguous and 16-byte aligned (a contiguous view may start anywhere
// in its storage)
static torch::Tensor up_operand(const torch::Tensor& t) {
  auto c = t.to(torch::kBFloat16).contiguous();
  if (reinterpret_cast<uintptr_t>(c.data_ptr()) % 16 != 0) c = c.clone();
  return c;
}

// Instances follow the forward's geometry rule; CPW = 2 (64 ci per block)
// when Cin > 32.
torch::Tensor upconv3d_dgrad(torch::Tensor go, torch::Tensor w,
                             std::vector<int64_t> x_shape) {
  CHECK_GPU(go);
  CHECK_GPU(w);
  TORCH_CHECK(x_shape.size() == 5 && w.dim() == 5 &&
              w.size(1) == x_shape[1] && go.dim() == 5 &&
              go.size(1) == w.size(0) && w.size(2) == 3 && w.size(3) == 3 &&
              w.size(4) == 3,
              "upconv3d_dgrad: go[N,Cout,2D,2H,2W], w[Cout,Cin,3,3,3]");
  auto gc = up_operand(go);
  auto wc = up_operand(w);
  const UpDims ud = up_dims(gc, x_shape[0], x_shape[1], x_shape[2],
                            x_shape[3], x_shape[4], "upconv3d_dgrad");
  auto dx = torch::empty({ud.N, ud.Cin, ud.D, ud.H, ud.W}, gc.options());

  const int cots = (ud.Cout + 31) / 32;
  const int cpw = ud.Cin > 32 ? 2 : 1;
  const int cigs = (ud.Cin + 32 * cpw - 1) / (32 * cpw);  // blocks along ci
  const int64_t wb_total = (int64_t)cigs * cpw * cots * 64 * 1024;
  TORCH_CHECK(wb_total < (int64_t)1 << 31, "WBT too large");
  auto wbt = torch::empty({wb_total}, wc.options());
  auto s = current_stream();
  hipLaunchKernelGGL(upconv3d_prep_wb_kernel,
                     dim3((unsigned)((wb_total + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const __bf16*>(wc.data_ptr()),
                     reinterpret_cast<__bf16*>(wbt.data_ptr()), ud.Cin,
                     ud.Cout, cots, (int)wb_total, 1);

  const int DT = (ud.W == 8 && ud.H <= 8) ? 2 : 1;
  const int OWT = ud.W % 32 == 0 ? 32 : (ud.W % 16 == 0 ? 16 : 8);
  const int OHT = 128 / (OWT * DT);
  const int64_t nblk = (int64_t)ud.N * ((ud.D + DT - 1) / DT) *
                       ((ud.H + OHT - 1) / OHT) * ((ud.W + OWT - 1) / OWT);
  TORCH_CHECK(nblk < (int64_t)1 << 31 && cigs < 65536, "grid too large");
  dim3 grid((unsigned)nblk, cigs);
  const int gvec = ud.W % 4 == 0;  // high-res rows are 16-byte multiples
  const int dvec = ud.W % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(dx.data_ptr()) % 8 == 0;
  auto L = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s,
                       reinterpret_cast<const __bf16*>(gc.data_ptr()),
                       reinterpret_cast<const __bf16*>(wbt.data_ptr()),
                       reinterpret_cast<__bf16*>(dx.data_ptr()), ud, cots,
                       gvec, dvec);
  };
  dispatch_bool(cpw == 2, [&](auto two) {
    constexpr int CPW = decltype(two)::value ? 2 : 1;
    if (DT == 2) L(upconv3d_dgrad_kernel<8, 2, CPW>);
    else if (OWT == 32) L(upconv3d_dgrad_kernel<32, 1, CPW>);
    else if (OWT == 16) L(upconv3d_dgrad_kernel<16, 1, CPW>);
    else L(upconv3d_dgrad_kernel<8, 1, CPW>);
  });
  return dx;
}

// ---------------------------------------------------------------------------
// Collapsed wgrad. Slot gradients
//   dWS[slot (cls, e)][co][ci] = sum over (n, j) of go_cls[j][co] * x[j+off][ci]
// with off = p + e - 1 per axis: a GEMM with M = co, N = ci and K the low-res
// positions, so both operands are staged POSITION-innermost (a lane's 8 k are
// 8 consecutive w of one channel); the forward's channel-innermost slab would
// put a lane's 8 k in 8 different 64-byte positions. No upsampled temporary.
//
// A block owns one depth parity a (4 classes, 32 slots), one 32-co and one
// 32-ci tile, and a contiguous range of position tiles (split K); wave v owns
// class (b, c) = (v >> 1, v & 1): 8 slots x 2 co fragments x 2 ci fragments
// = 128 accumulator registers, kept over the whole range.
// A position tile is TH x TW = 64 positions of one (n, d); k-group g (8
// positions) is row g / (TW/8), columns 8 * (g % (TW/8)).
//   sG[4 classes][32 co][64 positions (pitch 72)]: a 16-byte read of 8
//     high-res w splits into even and odd elements, two 8-byte stores to
//     classes (b, 0) and (b, 1).
//   sX[32 ci][2 planes d+a-1, d+a][TH+2 rows][pitch TW+16]: column w0 sits at
//     index 8, so interior vectors are aligned in HBM and in LDS; indices 7
//     and TW+8 are the halo columns. Slot (ed, eh, ew) reads plane ed, row
//     + b + eh, and the w shift c + ew - 1 in {-1, 0, +1}: the aligned
//     16-byte word for shift 0, and for -1 / +1 the same word funnel-shifted
//     by one element with the neighbouring 32-bit word (a wave needs one
//     side only: -1 for c = 0, +1 for c = 1). Staged once per tile for all
//     4 classes.
// Channel strides are 8 * odd elements (4 * odd banks): the 16 rows of a
// ds_read_b128 start on 16 distinct multiples of 4 banks.
// Everything past the tensor is staged as zero and adds nothing, so ragged
// W, H, Cin, Cout need no check in the loop.
// Fold: fp32 atomics into dWS[64][Cout][Cin]; the 16 lanes of a fragment
// row are 16 consecutive ci, one 64-byte run per atomic instruction.
// ---------------------------------------------------------------------------
constexpr int up_odd8(int n) { return (n / 8) % 2 == 1 ? n : n + 8; }

template <int TW>
__global__ __launch_bounds__(256, 2) void upconv3d_wgrad_kernel(
    const __bf16* __restrict__ x, const __bf16* __restrict__ go,
    float* __restrict__ dws, UpDims ud, int cots, int total_tiles,
    int tiles_per_block, int xvec, int gvec) {
  constexpr int TH = 64 / TW;
  constexpr int XR = TH + 2, XP = TW + 16;
  constexpr int XCS = up_odd8(2 * XR * XP);
  constexpr int GCS = 72;
  constexpr int GV = TW / 8;  // k-groups per tile row
  static_assert((32 * XCS + 4 * 32 * GCS) * 2 <= 64 * 1024, "static LDS cap");
  __shared__ __attribute__((aligned(16))) __bf16 sX[32 * XCS];
  __shared__ __attribute__((aligned(16))) __bf16 sG[4 * 32 * GCS];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int row = lane & 15, kg = lane >> 4;
  const int b = wave >> 1, c = wave & 1;
  int y = blockIdx.y;
  const int cit = y % ud.kts;
  y /= ud.kts;
  const int cot = y % cots;
  const int a = y / cots;
  const int t0 = blockIdx.x * tiles_per_block;
  const int t1 = t0 + tiles_per_block < total_tiles ? t0 + tiles_per_block
                                                    : total_tiles;
  const int wtiles = (ud.W + TW - 1) / TW;
  const int htiles = (ud.H + TH - 1) / TH;
  const int TD2 = 2 * ud.D, TH2 = 2 * ud.H, TW2 = 2 * ud.W;
  const int64_t HW = (int64_t)ud.H * ud.W;
  const int64_t THW = (int64_t)TH2 * TW2;
  // a co fragment wholly past Cout is zero: skip its MFMAs (wave-uniform)
  const bool cf_live[2] = {cot * 32 < ud.Cout, cot * 32 + 16 < ud.Cout};

  f32x4 acc[8][2][2];
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[e][i][j] = {0.f, 0.f, 0.f, 0.f};

  for (int t = t0; t < t1; ++t) {
    int r = t;
    const int w0 = (r % wtiles) * TW;
    r /= wtiles;
    const int h0 = (r % htiles) * TH;
    r /= htiles;
    const int d = r % ud.D;
    const int n = r / ud.D;
    if (t != t0) __syncthreads();

    // x interior: 32 ci x 2 planes x XR rows x GV vectors
    for (int it = tid; it < 32 * 2 * XR * GV; it += 256) {
      const int v = it % GV;
      const int rr = (it / GV) % XR;
      const int pl = (it / (GV * XR)) & 1;
      const int cl = it / (GV * XR * 2);
      const int ci = cit * 32 + cl;
      const int id = d + a - 1 + pl, ih = h0 - 1 + rr, iw = w0 + v * 8;
      bf16x8 val;
#pragma unroll
      for (int j = 0; j < 8; ++j) val[j] = (__bf16)0.f;
      if (ci < ud.Cin && id >= 0 && id < ud.D && ih >= 0 && ih < ud.H) {
        const __bf16* src = x + (((int64_t)n * ud.Cin + ci) * ud.D + id) * HW +
                            (int64_t)ih * ud.W;
        if (xvec && iw + 8 <= ud.W) {
          val = *reinterpret_cast<const bf16x8*>(src + iw);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (iw + j < ud.W) val[j] = src[iw + j];
        }
      }
      *reinterpret_cast<bf16x8*>(sX + cl * XCS + (pl * XR + rr) * XP + 8 +
                                 v * 8) = val;
    }
    // x halo columns w0 - 1 (index 7) and w0 + TW (index TW + 8)
    for (int it = tid; it < 32 * 2 * XR * 2; it += 256) {
      const int side = it & 1;
      const int rr = (it >> 1) % XR;
      const int pl = (it / (2 * XR)) & 1;
      const int cl = it / (4 * XR);
      const int ci = cit * 32 + cl;
      const int id = d + a - 1 + pl, ih = h0 - 1 + rr;
      const int iw = side ? w0 + TW : w0 - 1;
      __bf16 val = (__bf16)0.f;
      if (ci < ud.Cin && id >= 0 && id < ud.D && ih >= 0 && ih < ud.H &&
          iw >= 0 && iw < ud.W)
        val = x[(((int64_t)n * ud.Cin + ci) * ud.D + id) * HW +
                (int64_t)ih * ud.W + iw];
      sX[cl * XCS + (pl * XR + rr) * XP + (side ? TW + 8 : 7)] = val;
    }
    // go: 32 co x (TH rows x 2 b) x TW/4 vectors of 8 high-res w
    for (int it = tid; it < 32 * TH * 2 * (TW / 4); it += 256) {
      const int v = it % (TW / 4);
      const int hb = (it / (TW / 4)) % (2 * TH);  // hl * 2 + b
      const int cl = it / ((TW / 4) * 2 * TH);
      const int hl = hb >> 1, gb = hb & 1;
      const int co = cot * 32 + cl;
      const int ih = h0 + hl, gw = 2 * w0 + v * 8;
      bf16x4 ev, od;
#pragma unroll
      for (int j = 0; j < 4; ++j) ev[j] = od[j] = (__bf16)0.f;
      if (co < ud.Cout && ih < ud.H) {
        const __bf16* src = go +
                            (((int64_t)n * ud.Cout + co) * TD2 + 2 * d + a) *
                                THW +
                            (int64_t)(2 * ih + gb) * TW2;
        if (gvec && gw + 8 <= TW2) {
          const bf16x8 vec = *reinterpret_cast<const bf16x8*>(src + gw);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            ev[j] = vec[2 * j];
            od[j] = vec[2 * j + 1];
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (gw + 2 * j < TW2) ev[j] = src[gw + 2 * j];
            if (gw + 2 * j + 1 < TW2) od[j] = src[gw + 2 * j + 1];
          }
        }
      }
      __bf16* dst = sG + (gb * 2 * 32 + cl) * GCS + hl * TW + v * 4;
      *reinterpret_cast<bf16x4*>(dst) = ev;
      *reinterpret_cast<bf16x4*>(dst + 32 * GCS) = od;
    }
    __syncthreads();

#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int g = ks * 4 + kg;
      const int hl = g / GV, wv = g % GV;
      bf16x8 afrag[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        afrag[i] = *reinterpret_cast<const bf16x8*>(
            sG + (wave * 32 + i * 16 + row) * GCS + g * 8);
#pragma unroll
      for (int dh = 0; dh < 4; ++dh) {
        const int ed = dh >> 1, eh = dh & 1;
        const int base = (ed * XR + hl + b + eh) * XP + 8 + wv * 8;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const __bf16* px = sX + (j * 16 + row) * XCS + base;
          const u32x4 mid = *reinterpret_cast<const u32x4*>(px);
          // the 32-bit neighbour: elements (6, 7) before or (8, 9) after
          const unsigned nb =
              *reinterpret_cast<const unsigned*>(px + (c ? 8 : -2));
          u32x4 sh;
          if (c == 0) {  // shift -1: element k is mid's element k - 1
            sh[0] = (nb >> 16) | (mid[0] << 16);
#pragma unroll
            for (int q = 1; q < 4; ++q)
              sh[q] = (mid[q - 1] >> 16) | (mid[q] << 16);
          } else {       // shift +1: element k is mid's element k + 1
#pragma unroll
            for (int q = 0; q < 3; ++q)
              sh[q] = (mid[q] >> 16) | (mid[q + 1] << 16);
            sh[3] = (mid[3] >> 16) | (nb << 16);
          }
          // ew = 0 reads shift c - 1, ew = 1 reads shift c
          const bf16x8 x0 = __builtin_bit_cast(bf16x8, c ? mid : sh);
          const bf16x8 x1 = __builtin_bit_cast(bf16x8, c ? sh : mid);
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            if (!cf_live[i]) continue;
            acc[dh * 2][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag[i], x0, acc[dh * 2][i][j], 0, 0, 0);
            acc[dh * 2 + 1][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag[i], x1, acc[dh * 2 + 1][i][j], 0, 0, 0);
          }
        }
      }
    }
  }

  const int cls = a * 4 + b * 2 + c;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int slot = up_slot(
        cls, (a + (e >> 2)) * 9 + (b + ((e >> 1) & 1)) * 3 + (c + (e & 1)));
    float* dst = dws + (int64_t)slot * ud.Cout * ud.Cin;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ci = cit * 32 + j * 16 + row;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = cot * 32 + i * 16 + kg * 4 + r;
          if (co < ud.Cout && ci < ud.Cin)
            atomicAdd(&dst[(int64_t)co * ud.Cin + ci], acc[e][i][j][r]);
        }
      }
  }
}

// dw[co][ci][tap] = sum over the 8 classes of dWS[up_slot(cls, shift of
// (cls, tap))][co][ci]: every tap lies in exactly one slot per class. Also
// the permuting copy from slot-major to torch's layout. The file's second
// kernel with fp32 adds: plain v_add_f32.
__global__ UP_NO_PK_F32 __launch_bounds__(256) void upconv3d_wgrad_finish_kernel(
    const float* __restrict__ dws, float* __restrict__ dw, int cin, int cout,
    int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int tap = idx % 27;
  const int64_t cc = idx / 27;  // co * cin + ci
  const int64_t slot_sz = (int64_t)cout * cin;
  float sum = 0.f;
  for (int cls = 0; cls < 8; ++cls)
    sum += dws[up_slot(cls, up_shift_of(cls, tap)) * slot_sz + cc];
  dw[idx] = sum;
}

// Split K: position tiles are dealt out in contiguous ranges so that the
// launch has about 1024 blocks, a range being at least 4 tiles (each block
// ends with 32 K atomics, whatever its range).
torch::Tensor upconv3d_wgrad(torch::Tensor x, torch::Tensor go) {
  CHECK_GPU(x);
  CHECK_GPU(go);
  TORCH_CHECK(x.dim() == 5, "upconv3d_wgrad: x[N,Cin,D,H,W]");
  auto xc = up_operand(x);
  auto gc = up_operand(go);
  const UpDims ud = up_dims(gc, xc.size(0), xc.size(1), xc.size(2),
                            xc.size(3), xc.size(4), "upconv3d_wgrad");
  const auto f32 = xc.options().dtype(torch::kFloat32);
  auto dw = torch::empty({ud.Cout, ud.Cin, 3, 3, 3}, f32);
  auto dws = torch::zeros({64, ud.Cout, ud.Cin}, f32);

  const int TW = ud.W % 32 == 0 ? 32 : (ud.W % 16 == 0 ? 16 : 8);
  const int TH = 64 / TW;
  const int cots = (ud.Cout + 31) / 32;
  const int64_t total_tiles = (int64_t)ud.N * ud.D * ((ud.H + TH - 1) / TH) *
                              ((ud.W + TW - 1) / TW);
  const int64_t ny = (int64_t)2 * cots * ud.kts;
  const int64_t dw_total = (int64_t)ud.Cout * ud.Cin * 27;
  TORCH_CHECK(total_tiles < (int64_t)1 << 31 && ny < 65536 &&
              dw_total * 3 < (int64_t)1 << 31, "upconv3d_wgrad: too large");
  int64_t tpb = (total_tiles * ny + 1023) / 1024;
  if (tpb < 4) tpb = 4;
  const int64_t nz = (total_tiles + tpb - 1) / tpb;
  auto s = current_stream();
  const int xvec = ud.W % 8 == 0;
  const int gvec = ud.W % 4 == 0;
  auto L = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)nz, (unsigned)ny), dim3(256), 0, s,
                       reinterpret_cast<const __bf16*>(xc.data_ptr()),
                       reinterpret_cast<const __bf16*>(gc.data_ptr()),
                       dws.data_ptr<float>(), ud, cots, (int)total_tiles,
                       (int)tpb, xvec, gvec);
  };
  if (TW == 32) L(upconv3d_wgrad_kernel<32>);
  else if (TW == 16) L(upconv3d_wgrad_kernel<16>);
  else L(upconv3d_wgrad_kernel<8>);
  hipLaunchKernelGGL(upconv3d_wgrad_finish_kernel,
                     dim3((unsigned)((dw_total + 255) / 256)), dim3(256), 0, s,
                     dws.data_ptr<float>(), dw.data_ptr<float>(), ud.Cin,
                     ud.Cout, (int)dw_total);
  return dw;
}

// ---------------------------------------------------------------------------
// upsample2_nearest3d and its adjoint fold2_sum3d. A thread owns 4 low-res
// elements of one row: 8 consecutive high-res elements in each of the 4
// (depth, row) copies of the 2x2x2 bricks, moved as one vector per row when
// W % 4 == 0 and the base is aligned, as guarded scalars otherwise.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void upsample2_nearest3d_kernel(
    const __bf16* __restrict__ x, __bf16* __restrict__ y, int64_t rows, int H,
    int W, int vec) {
  const int wq = (W + 3) / 4;
  const int64_t total = rows * wq;  // rows = N*C*D*H low-res rows
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total;
       it += (int64_t)gridDim.x * 256) {
    const int q = (int)(it % wq);
    const int64_t r = it / wq;          // (n*C + c)*D*H + d*H + h
    const int h = (int)(r % H);
    const int64_t pd = r / H;           // (n*C + c)*D + d
    const __bf16* src = x + r * W + q * 4;
    __bf16 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (__bf16)0.f;
    if (vec) {
      const bf16x4 t4 = *reinterpret_cast<const bf16x4*>(src);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = t4[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (q * 4 + j < W) v[j] = src[j];
    }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[2 * j] = o[2 * j + 1] = v[j];
#pragma unroll
    for (int ab = 0; ab < 4; ++ab) {
      __bf16* dst = y + ((2 * pd + (ab >> 1)) * (2 * H) + 2 * h + (ab & 1)) *
                            (int64_t)(2 * W) + q * 8;
      if (vec) {
        *reinterpret_cast<bf16x8*>(dst) = o;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (q * 8 + j < 2 * W) dst[j] = o[j];
      }
    }
  }
}

torch::Tensor upsample2_nearest3d(torch::Tensor x) {
  CHECK_GPU(x);
  TORCH_CHECK(x.dim() == 5, "upsample2_nearest3d: x[N,C,D,H,W]");
  auto xc = x.to(torch::kBFloat16).contiguous();
  const int64_t N = xc.size(0), C = xc.size(1), D = xc.size(2);
  const int H = (int)xc.size(3), W = (int)xc.size(4);
  auto y = torch::empty({N, C, 2 * D, 2 * H, 2 * W}, xc.options());
  if (y.numel() == 0) return y;
  const int64_t rows = N * C * D * H;
  const int vec = (W % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(xc.data_ptr()) % 8 == 0 &&
                   reinterpret_cast<uintptr_t>(y.data_ptr()) % 16 == 0)
                      ? 1 : 0;
  hipLaunchKernelGGL(upsample2_nearest3d_kernel,
                     dim3(elem_grid(rows * ((W + 3) / 4), 1)), dim3(256), 0,
                     current_stream(),
                     reinterpret_cast<const __bf16*>(xc.data_ptr()),
                     reinterpret_cast<__bf16*>(y.data_ptr()), rows, H, W, vec);
  return y;
}

template <typename T>
__global__ UP_NO_PK_F32 __launch_bounds__(256) void fold2_sum3d_kernel(
    const T* __restrict__ g, T* __restrict__ y, int64_t rows, int H, int W,
    int vec) {
  typedef __attribute__((ext_vector_type(8))) T Tx8;
  const int wq = (W + 3) / 4;
  const int64_t total = rows * wq;  // rows = N*C*D*H low-res rows
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total;
       it += (int64_t)gridDim.x * 256) {
    const int q = (int)(it % wq);
    const int64_t r = it / wq;
    const int h = (int)(r % H);
    const int64_t pd = r / H;
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ab = 0; ab < 4; ++ab) {
      const T* src = g + ((2 * pd + (ab >> 1)) * (2 * H) + 2 * h + (ab & 1)) *
                             (int64_t)(2 * W) + q * 8;
      if (vec) {
        const Tx8 t8 = *reinterpret_cast<const Tx8*>(src);
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[j >> 1] += (float)t8[j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (q * 8 + j < 2 * W) sum[j >> 1] += (float)src[j];
      }
    }
    T* dst = y + r * W + q * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q * 4 + j < W) dst[j] = (T)sum[j];
  }
}

torch::Tensor fold2_sum3d(torch::Tensor g) {
  CHECK_GPU(g);
  TORCH_CHECK(g.dim() == 5 && g.size(2) % 2 == 0 && g.size(3) % 2 == 0 &&
              g.size(4) % 2 == 0,
              "fold2_sum3d: g[N,C,2D,2H,2W]");
  TORCH_CHECK(g.scalar_type() == torch::kBFloat16 ||
              g.scalar_type() == torch::kFloat32,
              "fold2_sum3d: bf16 or fp32");
  auto gc = g.contiguous();
  const int64_t N = gc.size(0), C = gc.size(1), D = gc.size(2) / 2;
  const int H = (int)gc.size(3) / 2, W = (int)gc.size(4) / 2;
  auto y = torch::empty({N, C, D, H, W}, gc.options());
  if (y.numel() == 0) return y;
  const int64_t rows = N * C * D * H;
  const int vec = (W % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(gc.data_ptr()) %
                           (8 * gc.element_size()) == 0)
                      ? 1 : 0;
  const dim3 grid(elem_grid(rows * ((W + 3) / 4), 1));
  auto s = current_stream();
  if (gc.scalar_type() == torch::kBFloat16)
    hipLaunchKernelGGL(fold2_sum3d_kernel<__bf16>, grid, dim3(256), 0, s,
                       reinterpret_cast<const __bf16*>(gc.data_ptr()),
                       reinterpret_cast<__bf16*>(y.data_ptr()), rows, H, W,
                       vec);
  else
    hipLaunchKernelGGL(fold2_sum3d_kernel<float>, grid, dim3(256), 0, s,
                       gc.data_ptr<float>(), y.data_ptr<float>(), rows, H, W,
                       vec);
  return y;
}
