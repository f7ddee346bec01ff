// Persistent LSTM recurrence: all T steps of one layer in one launch.
//
// The time-parallel GEMMs (Xp = x W_ih^T + b, dW_ih, dW_hh, dx, db) run on
// linear.hip. These kernels do what is sequential in time:
//   pre_t = Xp_t + h_{t-1} W_hh^T;  i, f, o = sigmoid, g = tanh (torch order
//   i, f, g, o);  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)
// and the reverse-time loop that turns dy into dG (the gradient of pre).
//
// Ownership. grid = (ceil(B / 16), directions); a block owns 16 batch rows
// (one MFMA M tile) of one direction for all steps and never talks to another
// block: the only synchronisation is __syncthreads(). Hp = H rounded up to 32.
// A wave owns NU tiles of 16 hidden units, all four gates of each: NU = 1
// and Hp / 16 waves for Hp <= 128, NU = 2 and Hp / 32 waves above (at most
// 512 threads, so a lane keeps a 256-register budget).
// v_mfma_f32_16x16x32_bf16 puts C(row, col) at (row = (lane >> 4) * 4 + reg,
// col = lane & 15), so with col = unit a lane holds i, f, g, o of the same
// four (batch row, unit) pairs: the cell update is in-lane and c lives in
// fp32 registers over all steps. Direction 1 walks t from T - 1 down and uses
// the upper half of y's last axis.
//
// Padding. Units H .. Hp - 1 have zero weights and read Xp as 0: g = 0,
// c = 0, h = 0 exactly at every step, so the step loop has no masks. Rows
// past B compute on zeros and are never stored. Only global loads and stores
// are guarded (unit < H, row < B).
//
// Forward. A = h_{t-1} as bf16 in LDS, [2][16][Hp + 8] (the 8 pad elements
// shift consecutive rows by 4 banks; 16-byte fragment reads). B = W_hh^T
// prepacked by lstm_pack_weights as [unit tile][kstep][gate][lane][8] bf16:
// lane l of fragment (ks, gate) holds k = 32 ks + 8 (l >> 4) .. + 7 of unit
// 16 tile + (l & 15). Hp <= 128: the wave's 4 * Hp / 32 <= 16 fragments are
// loaded once into registers (indexed by unrolled constants). Hp > 128: the
// same loop fetches them each step with 16-byte loads, one k-step ahead of
// the MFMAs (the packed buffer is L2-resident). The accumulators start from
// Xp_t; Xp_{t+1} is loaded before the MFMAs of step t. h_t goes to the other
// LDS buffer and to y: one barrier per step.
//
// Global layouts. Xp, dG and the saved gates are [T, B, D, H, 4] with the
// gate innermost (the facade permutes the rows of W_ih and b once per call),
// so the four values of a (row, unit) are one 16-byte access; the saved cells
// are [T, B, D, H] like y.
//
// Backward. Same grid and ownership. Per step: dh = dy_t + dh_rec, the gate
// gradients from the saved post-activation gates, c_{t-1} and c_t; dG_t goes
// to global memory (fp32, for the time-parallel GEMMs) and as bf16 into an
// LDS tile [16][4 Hp + 8]; dh_rec = dG_t W_hh is 4 Hp / 32 MFMAs per unit
// tile on the second prepacked copy, [unit tile][kstep][lane][8] with
// k = gate * Hp + unit and n = 16 tile + (l & 15): the result lands in the
// lane that owns that (row, unit). dc and dh_rec stay in registers. The dG
// tile is double buffered where two tiles fit 64 KB (Hp <= 224), else a
// second barrier.
//
// Nothing here synchronises the host, uses atomics, or depends on the order
// in which blocks run.
#include "common.h"

#include <c10/util/BFloat16.h>
#include <c10/util/Optional.h>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

constexpr int LSTM_MAX_H = 256;
constexpr int LSTM_ROWS = 16;   // batch rows per block: one MFMA M tile
constexpr int LSTM_PAD = 8;     // bf16 elements of LDS row padding (16 B)

// unit tiles per wave and threads per block of the recurrent kernels
constexpr int lstm_nu(int hp) { return hp > 128 ? 2 : 1; }
constexpr int lstm_threads(int hp) { return hp / (16 * lstm_nu(hp)) * 64; }

__device__ inline float lstm_sigmoid(float x) {
  return 1.0f / (1.0f + __expf(-x));
}

// 1 - 2 / (1 + e^{2x}): exact limits at +-inf, abs error ~1e-7 near 0
__device__ inline float lstm_tanh(float x) {
  return 1.0f - 2.0f / (1.0f + __expf(2.0f * x));
}

inline int lstm_hp(int64_t H) { return (int)((H + 31) / 32 * 32); }

template <class F>
inline void dispatch_hp(int hp, F&& f) {
  switch (hp) {
    case 32: f(IntC<32>{}); break;
    case 64: f(IntC<64>{}); break;
    case 96: f(IntC<96>{}); break;
    case 128: f(IntC<128>{}); break;
    case 160: f(IntC<160>{}); break;
    case 192: f(IntC<192>{}); break;
    case 224: f(IntC<224>{}); break;
    case 256: f(IntC<256>{}); break;
    default: TORCH_CHECK(false, "lstm: padded hidden size ", hp,
                         " is outside [32, 256]");
  }
}

}  // namespace

// ------------------------------------------------------------------ prepack
// out[0]: forward fragments, out[1]: backward fragments, 4 Hp^2 bf16 each.
template <typename TW>
__global__ void __launch_bounds__(ELEM_BLOCK)
lstm_pack_weights_kernel(const TW* __restrict__ w,
                         c10::BFloat16* __restrict__ out, int H, int Hp) {
  const int per = 4 * Hp * Hp;
  for (int idx = blockIdx.x * ELEM_BLOCK + threadIdx.x; idx < 2 * per;
       idx += gridDim.x * ELEM_BLOCK) {
    const int bwd = idx >= per;
    const int r = idx - bwd * per;
    const int e = r & 7, lane = (r >> 3) & 63, frag = r >> 9;
    const int n = lane & 15, k8 = (lane >> 4) * 8 + e;
    float v = 0.0f;
    if (!bwd) {
      const int KS = Hp / 32;
      const int g = frag & 3, ks = (frag >> 2) % KS, tile = (frag >> 2) / KS;
      const int k = ks * 32 + k8, u = tile * 16 + n;
      if (u < H && k < H) v = (float)w[(int64_t)(g * H + u) * H + k];
    } else {
      const int KS = Hp / 8;
      const int ks = frag % KS, tile = frag / KS;
      const int kk = ks * 32 + k8;
      const int g = kk / Hp, j = kk - g * Hp, u = tile * 16 + n;
      if (j < H && u < H) v = (float)w[(int64_t)(g * H + j) * H + u];
    }
    out[idx] = (c10::BFloat16)v;
  }
}

// ------------------------------------------------------------------ forward
template <int HP, bool SAVE>
__global__ void __launch_bounds__(lstm_threads(HP))
lstm_rec_fwd_kernel(const float* __restrict__ xp, const void* wpack,
                    const float* __restrict__ h0, const float* __restrict__ c0,
                    float* __restrict__ y, float* __restrict__ hT,
                    float* __restrict__ cT, float* __restrict__ gates,
                    float* __restrict__ cells, int T, int B, int H, int D) {
  constexpr bool STREAM = HP > 128;
  constexpr int NU = lstm_nu(HP);
  constexpr int KS = HP / 32;
  constexpr int LDH = HP + LSTM_PAD;
  __shared__ __attribute__((aligned(16))) __bf16 s_h[2][LSTM_ROWS][LDH];

  const int dir = blockIdx.y;
  const int b0 = blockIdx.x * LSTM_ROWS;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 15, quad = lane >> 4;
  const int u0 = wave * NU * 16 + col;  // the lane's unit of tile i: u0 + 16 i
  const int brow = b0 + quad * 4;       // the lane's batch row of reg r: + r

  // fragment (tile i, ks, gate) at wp[((i * KS + ks) * 4 + gate) * 64]
  const bf16x8* wp = reinterpret_cast<const bf16x8*>(wpack) +
                     (int64_t)dir * HP * HP + wave * NU * KS * 4 * 64 + lane;
  bf16x8 wst[STREAM ? 1 : KS * 4];
  if constexpr (!STREAM) {
#pragma unroll
    for (int f = 0; f < KS * 4; ++f) wst[f] = wp[f * 64];
  }
  // streamed: an offset the compiler cannot see through (always 0), redefined
  // every step, keeps the fragment loads inside the step loop; hoisted out
  // of it they would need 4 * NU * KS * 4 registers and spill
  int wofs = 0;
  auto wfrag = [&](int i, int ks, int g) -> bf16x8 {
    if constexpr (STREAM) return wp[wofs + ((i * KS + ks) * 4 + g) * 64];
    else return wst[ks * 4 + g];
  };

  float c[NU][4], h[NU][4];
#pragma unroll
  for (int i = 0; i < NU; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int u = u0 + 16 * i;
      const bool ok = u < H && brow + r < B;
      const int64_t sidx = ((int64_t)dir * B + brow + r) * H + u;
      c[i][r] = (c0 != nullptr && ok) ? c0[sidx] : 0.0f;
      h[i][r] = (h0 != nullptr && ok) ? h0[sidx] : 0.0f;
    }
  for (int idx = threadIdx.x; idx < LSTM_ROWS * HP; idx += lstm_threads(HP)) {
    const int row = idx / HP, k = idx - row * HP;
    float v = 0.0f;
    if (h0 != nullptr && b0 + row < B && k < H)
      v = h0[((int64_t)dir * B + b0 + row) * H + k];
    s_h[0][row][k] = (__bf16)v;
  }
  __syncthreads();

  const int64_t xrow = (int64_t)D * 4 * H;  // floats per (t, b) of xp
  auto load_xp = [&](int t, float (&dst)[NU][4][4]) {
#pragma unroll
    for (int i = 0; i < NU; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int u = u0 + 16 * i;
        const bool ok = u < H && brow + r < B;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (ok)
          v = *reinterpret_cast<const f32x4*>(
              xp + ((int64_t)t * B + brow + r) * xrow + (dir * H + u) * 4);
#pragma unroll
        for (int g = 0; g < 4; ++g) dst[i][g][r] = v[g];
      }
  };

  float xcur[NU][4][4], xnxt[NU][4][4];
  const int dt = dir ? -1 : 1;
  int t = dir ? T - 1 : 0;
  load_xp(t, xcur);
  int cur = 0;
  for (int s = 0; s < T; ++s, t += dt) {
    if constexpr (STREAM) asm volatile("" : "+v"(wofs));
    // the four gate fragments of (k-step, tile) q + 1 are fetched before the
    // MFMAs of q
    bf16x8 wc[4], wn[4], a;
#pragma unroll
    for (int g = 0; g < 4; ++g) wc[g] = wfrag(0, 0, g);
    if (s + 1 < T) load_xp(t + dt, xnxt);
    f32x4 acc[NU][4];
#pragma unroll
    for (int i = 0; i < NU; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][g][r] = xcur[i][g][r];
#pragma unroll
    for (int q = 0; q < KS * NU; ++q) {
      const int ks = q / NU, i = q % NU;
      if (q + 1 < KS * NU) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          wn[g] = wfrag((q + 1) % NU, (q + 1) / NU, g);
      }
      if (i == 0)
        a = *reinterpret_cast<const bf16x8*>(
            &s_h[cur][col][ks * 32 + quad * 8]);
#pragma unroll
      for (int g = 0; g < 4; ++g)
        acc[i][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wc[g],
                                                            acc[i][g], 0, 0, 0);
      if (q + 1 < KS * NU) {
#pragma unroll
        for (int g = 0; g < 4; ++g) wc[g] = wn[g];
      }
    }
#pragma unroll
    for (int i = 0; i < NU; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gi = lstm_sigmoid(acc[i][0][r]);
        const float gf = lstm_sigmoid(acc[i][1][r]);
        const float gg = lstm_tanh(acc[i][2][r]);
        const float go = lstm_sigmoid(acc[i][3][r]);
        c[i][r] = gf * c[i][r] + gi * gg;
        h[i][r] = go * lstm_tanh(c[i][r]);
        const int u = u0 + 16 * i;
        s_h[cur ^ 1][quad * 4 + r][u] = (__bf16)h[i][r];
        if (u < H && brow + r < B) {
          const int64_t tb = (int64_t)t * B + brow + r;
          y[tb * ((int64_t)D * H) + dir * H + u] = h[i][r];
          if constexpr (SAVE) {
            const int64_t sidx = (tb * D + dir) * H + u;
            *reinterpret_cast<f32x4*>(gates + sidx * 4) =
                f32x4{gi, gf, gg, go};
            cells[sidx] = c[i][r];
          }
        }
      }
    __syncthreads();
    cur ^= 1;
#pragma unroll
    for (int i = 0; i < NU; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) xcur[i][g][r] = xnxt[i][g][r];
  }
#pragma unroll
  for (int i = 0; i < NU; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int u = u0 + 16 * i;
      if (u < H && brow + r < B) {
        const int64_t sidx = ((int64_t)dir * B + brow + r) * H + u;
        hT[sidx] = h[i][r];
        cT[sidx] = c[i][r];
      }
    }
}

// ----------------------------------------------------------------- backward
template <int HP>
__global__ void __launch_bounds__(lstm_threads(HP))
lstm_rec_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ dhT,
                    const float* __restrict__ dcT,
                    const float* __restrict__ gates,
                    const float* __restrict__ cells,
                    const float* __restrict__ c0, const void* wpack,
                    float* __restrict__ dG, float* __restrict__ dh0,
                    float* __restrict__ dc0, int T, int B, int H, int D) {
  constexpr bool STREAM = HP > 128;
  constexpr int NU = lstm_nu(HP);
  constexpr int KS = HP / 8;  // K = 4 Hp in steps of 32
  constexpr int LDG = 4 * HP + LSTM_PAD;
  constexpr int NBUF = 2 * LSTM_ROWS * LDG * 2 <= 64 * 1024 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) __bf16 s_g[NBUF][LSTM_ROWS][LDG];

  const int dir = blockIdx.y;
  const int b0 = blockIdx.x * LSTM_ROWS;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 15, quad = lane >> 4;
  const int u0 = wave * NU * 16 + col;
  const int brow = b0 + quad * 4;

  // fragment (tile i, ks) at wp[(i * KS + ks) * 64], second packed copy
  const bf16x8* wp = reinterpret_cast<const bf16x8*>(wpack) +
                     ((int64_t)dir * 2 + 1) * (HP * HP / 2) +
                     wave * NU * KS * 64 + lane;
  bf16x8 wst[STREAM ? 1 : KS];
  if constexpr (!STREAM) {
#pragma unroll
    for (int f = 0; f < KS; ++f) wst[f] = wp[f * 64];
  }
  int wofs = 0;  // as in the forward: keeps streamed loads in the step loop
  auto wfrag = [&](int i, int ks) -> bf16x8 {
    if constexpr (STREAM) return wp[wofs + (i * KS + ks) * 64];
    else return wst[ks];
  };

  // what a step reads: the saved gates, c of the step before it in the
  // direction's walk (c0 at the walk's first step) and dy
  struct StepIn { float g[NU][4][4], cp[NU][4], dy[NU][4]; };
  const int dt = dir ? 1 : -1;  // against the direction's walk
  auto load_step = [&](int t, bool first, StepIn& in) {
#pragma unroll
    for (int i = 0; i < NU; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int u = u0 + 16 * i, b = brow + r;
        const bool ok = u < H && b < B;
        const int64_t sidx = (((int64_t)t * B + b) * D + dir) * H + u;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (ok) v = *reinterpret_cast<const f32x4*>(gates + sidx * 4);
#pragma unroll
        for (int g = 0; g < 4; ++g) in.g[i][g][r] = v[g];
        in.dy[i][r] = ok ? dy[sidx] : 0.0f;  // y and cells share the index
        if (!first)  // the cell of (t + dt, b): B rows of D * H further
          in.cp[i][r] = ok ? cells[sidx + (int64_t)dt * B * D * H] : 0.0f;
        else
          in.cp[i][r] = (c0 != nullptr && ok)
                            ? c0[((int64_t)dir * B + b) * H + u] : 0.0f;
      }
  };

  int t = dir ? 0 : T - 1;
  float dh[NU][4], dc[NU][4], ct[NU][4];
#pragma unroll
  for (int i = 0; i < NU; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int u = u0 + 16 * i, b = brow + r;
      const bool ok = u < H && b < B;
      const int64_t sidx = ((int64_t)dir * B + b) * H + u;
      dh[i][r] = ok ? dhT[sidx] : 0.0f;
      dc[i][r] = ok ? dcT[sidx] : 0.0f;
      ct[i][r] =
          ok ? cells[(((int64_t)t * B + b) * D + dir) * H + u] : 0.0f;
    }
  StepIn cur, nxt;
  load_step(t, T == 1, cur);
  int buf = 0;
  for (int s = 0; s < T; ++s, t += dt) {
#pragma unroll
    for (int i = 0; i < NU; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gi = cur.g[i][0][r], gf = cur.g[i][1][r];
        const float gg = cur.g[i][2][r], go = cur.g[i][3][r];
        const float tc = lstm_tanh(ct[i][r]);
        const float dhv = cur.dy[i][r] + dh[i][r];
        const float dcv = dc[i][r] + dhv * go * (1.0f - tc * tc);
        float d[4];
        d[0] = dcv * gg * gi * (1.0f - gi);
        d[1] = dcv * cur.cp[i][r] * gf * (1.0f - gf);
        d[2] = dcv * gi * (1.0f - gg * gg);
        d[3] = dhv * tc * go * (1.0f - go);
        dc[i][r] = dcv * gf;
        ct[i][r] = cur.cp[i][r];
        const int u = u0 + 16 * i;
#pragma unroll
        for (int g = 0; g < 4; ++g)
          s_g[buf][quad * 4 + r][g * HP + u] = (__bf16)d[g];
        if (u < H && brow + r < B)
          *reinterpret_cast<f32x4*>(
              dG + ((((int64_t)t * B + brow + r) * D + dir) * H + u) * 4) =
              f32x4{d[0], d[1], d[2], d[3]};
      }
    __syncthreads();
    if (s + 1 < T) load_step(t + dt, s + 2 == T, nxt);
    // dh_rec = dG_t W_hh, fragments fetched four k-steps ahead
    if constexpr (STREAM) asm volatile("" : "+v"(wofs));
    f32x4 acc[NU];
    bf16x8 wc[NU][4], wn[NU][4];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int j = 0; j < 4; ++j) wc[i][j] = wfrag(i, j);
    }
#pragma unroll
    for (int k4 = 0; k4 < KS; k4 += 4) {
      if (k4 + 4 < KS) {
#pragma unroll
        for (int i = 0; i < NU; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) wn[i][j] = wfrag(i, k4 + 4 + j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(
            &s_g[buf][col][(k4 + j) * 32 + quad * 8]);
#pragma unroll
        for (int i = 0; i < NU; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wc[i][j], acc[i],
                                                           0, 0, 0);
      }
      if (k4 + 4 < KS) {
#pragma unroll
        for (int i = 0; i < NU; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) wc[i][j] = wn[i][j];
      }
    }
#pragma unroll
    for (int i = 0; i < NU; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) dh[i][r] = acc[i][r];
    if constexpr (NBUF == 1) __syncthreads();
    else buf ^= 1;
    cur = nxt;
  }
#pragma unroll
  for (int i = 0; i < NU; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int u = u0 + 16 * i;
      if (u < H && brow + r < B) {
        const int64_t sidx = ((int64_t)dir * B + brow + r) * H + u;
        dh0[sidx] = dh[i][r];
        dc0[sidx] = dc[i][r];
      }
    }
}

// ---------------------------------------------------------------- host side
namespace {

const float* opt_f32(const c10::optional<torch::Tensor>& t, int64_t numel,
                     const char* name) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
              t->scalar_type() == torch::kFloat32 && t->numel() == numel,
              "lstm: ", name, " must be a contiguous fp32 GPU tensor [D, B, H]");
  return t->data_ptr<float>();
}

void check_f32(const torch::Tensor& t, int64_t numel, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == torch::kFloat32 && t.numel() == numel,
              "lstm: ", name, " must be a contiguous fp32 GPU tensor of ",
              numel, " elements");
}

void check_pack(const torch::Tensor& wpack, int64_t D, int hp) {
  TORCH_CHECK(wpack.is_cuda() && wpack.is_contiguous() &&
              wpack.scalar_type() == torch::kBFloat16 &&
              wpack.numel() == D * 8 * hp * hp,
              "lstm: wpack must be the stacked lstm_pack_weights output "
              "[D, 2, 4 Hp^2] bf16");
}

}  // namespace

// W_hh [4H, H] (fp32 or bf16) -> [2, 4 Hp^2] bf16 MFMA B fragments
torch::Tensor lstm_pack_weights(torch::Tensor w_hh) {
  CHECK_GPU(w_hh);
  TORCH_CHECK(w_hh.dim() == 2 && w_hh.size(0) == 4 * w_hh.size(1),
              "lstm_pack_weights: w_hh must be [4H, H]");
  const int64_t H = w_hh.size(1);
  TORCH_CHECK(H >= 1 && H <= LSTM_MAX_H, "lstm_pack_weights: H = ", H,
              " is outside [1, ", LSTM_MAX_H, "]");
  auto w = w_hh.contiguous();
  const int hp = lstm_hp(H);
  auto out = torch::empty({2, (int64_t)4 * hp * hp},
                          w.options().dtype(torch::kBFloat16));
  c10::BFloat16* op = out.data_ptr<c10::BFloat16>();
  const dim3 grid(elem_grid(out.numel(), 1));
  if (w.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(lstm_pack_weights_kernel<float>, grid,
                       dim3(ELEM_BLOCK), 0, current_stream(),
                       w.data_ptr<float>(), op, (int)H, hp);
  } else if (w.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(lstm_pack_weights_kernel<c10::BFloat16>, grid,
                       dim3(ELEM_BLOCK), 0, current_stream(),
                       w.data_ptr<c10::BFloat16>(), op, (int)H, hp);
  } else {
    TORCH_CHECK(false, "lstm_pack_weights: fp32 or bf16 only");
  }
  return out;
}

// xp [T, B, D, H, 4] fp32 (gate innermost) -> (y [T, B, D * H], h_T and c_T
// [D, B, H], gates [T, B, D, H, 4] and cells [T, B, D, H] or both empty),
// all fp32
std::vector<torch::Tensor> lstm_rec_fwd(torch::Tensor xp, torch::Tensor wpack,
                                        c10::optional<torch::Tensor> h0,
                                        c10::optional<torch::Tensor> c0,
                                        int64_t H, bool save) {
  CHECK_GPU(xp);
  TORCH_CHECK(xp.dim() == 3 && xp.is_contiguous() &&
              xp.scalar_type() == torch::kFloat32 &&
              reinterpret_cast<uintptr_t>(xp.data_ptr()) % 16 == 0,
              "lstm_rec_fwd: xp must be contiguous, 16-byte aligned fp32 "
              "[T, B, D * 4H]");
  TORCH_CHECK(H >= 1 && H <= LSTM_MAX_H, "lstm_rec_fwd: H = ", H,
              " is outside [1, ", LSTM_MAX_H, "]");
  const int64_t T = xp.size(0), B = xp.size(1), D = xp.size(2) / (4 * H);
  TORCH_CHECK(T >= 1 && B >= 1 && (D == 1 || D == 2) &&
              xp.size(2) == D * 4 * H,
              "lstm_rec_fwd: xp must be [T >= 1, B >= 1, D * 4H], D in {1, 2}");
  TORCH_CHECK(T * B < ((int64_t)1 << 31), "lstm_rec_fwd: T * B too large");
  const int hp = lstm_hp(H);
  check_pack(wpack, D, hp);
  const float* h0p = opt_f32(h0, D * B * H, "h0");
  const float* c0p = opt_f32(c0, D * B * H, "c0");
  auto y = torch::empty({T, B, D * H}, xp.options());
  auto hT = torch::empty({D, B, H}, xp.options());
  auto cT = torch::empty({D, B, H}, xp.options());
  auto gates = torch::empty({save ? T : 0, B, D, H, 4}, xp.options());
  auto cells = torch::empty({save ? T : 0, B, D, H}, xp.options());
  const dim3 grid((unsigned)((B + LSTM_ROWS - 1) / LSTM_ROWS), (unsigned)D);
  const void* wp = wpack.data_ptr();
  dispatch_hp(hp, [&](auto hh) {
    constexpr int HP = decltype(hh)::value;
    dispatch_bool(save, [&](auto sv) {
      constexpr bool SAVE = decltype(sv)::value;
      hipLaunchKernelGGL((lstm_rec_fwd_kernel<HP, SAVE>), grid,
                         dim3(lstm_threads(HP)), 0, current_stream(),
                         xp.data_ptr<float>(), wp, h0p, c0p,
                         y.data_ptr<float>(), hT.data_ptr<float>(),
                         cT.data_ptr<float>(), gates.data_ptr<float>(),
                         cells.data_ptr<float>(), (int)T, (int)B, (int)H,
                         (int)D);
    });
  });
  return {y, hT, cT, gates, cells};
}

// (dG [T, B, D, H, 4], dh0 [D, B, H], dc0 [D, B, H]) from dy [T, B, D * H],
// the gradients of h_T and c_T and the gates and cells the forward saved
std::vector<torch::Tensor> lstm_rec_bwd(torch::Tensor dy, torch::Tensor dhT,
                                        torch::Tensor dcT, torch::Tensor gates,
                                        torch::Tensor cells,
                                        c10::optional<torch::Tensor> c0,
                                        torch::Tensor wpack) {
  CHECK_GPU(gates);
  TORCH_CHECK(gates.dim() == 5 && gates.size(4) == 4 &&
              gates.is_contiguous() && gates.scalar_type() == torch::kFloat32 &&
              reinterpret_cast<uintptr_t>(gates.data_ptr()) % 16 == 0,
              "lstm_rec_bwd: gates must be contiguous, 16-byte aligned fp32 "
              "[T, B, D, H, 4]");
  const int64_t T = gates.size(0), B = gates.size(1), D = gates.size(2);
  const int64_t H = gates.size(3);
  TORCH_CHECK(T >= 1 && B >= 1 && (D == 1 || D == 2) && H >= 1 &&
              H <= LSTM_MAX_H, "lstm_rec_bwd: bad gates shape");
  const int hp = lstm_hp(H);
  check_pack(wpack, D, hp);
  check_f32(cells, T * B * D * H, "cells");
  check_f32(dy, T * B * D * H, "dy");
  check_f32(dhT, D * B * H, "dhT");
  check_f32(dcT, D * B * H, "dcT");
  const float* c0p = opt_f32(c0, D * B * H, "c0");
  auto dG = torch::empty({T, B, D, H, 4}, gates.options());
  auto dh0 = torch::empty({D, B, H}, gates.options());
  auto dc0 = torch::empty({D, B, H}, gates.options());
  const dim3 grid((unsigned)((B + LSTM_ROWS - 1) / LSTM_ROWS), (unsigned)D);
  const void* wp = wpack.data_ptr();
  dispatch_hp(hp, [&](auto hh) {
    constexpr int HP = decltype(hh)::value;
    hipLaunchKernelGGL((lstm_rec_bwd_kernel<HP>), grid,
                       dim3(lstm_threads(HP)), 0, current_stream(),
                       dy.data_ptr<float>(), dhT.data_ptr<float>(),
                       dcT.data_ptr<float>(), gates.data_ptr<float>(),
                       cells.data_ptr<float>(), c0p, wp,
                       dG.data_ptr<float>(), dh0.data_ptr<float>(),
                       dc0.data_ptr<float>(), (int)T, (int)B, (int)H, (int)D);
  });
  return {dG, dh0, dc0};
}
