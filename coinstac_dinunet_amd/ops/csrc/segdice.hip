// Multi-class soft-dice (+ cross-entropy) loss from [N, C, S...] logits.
//   p = softmax over the C class planes (class stride S), y = one-hot of the
//   labels inside [0, C); a voxel with any other label is dropped: it adds
//   to no sum and its C gradients are exactly zero.
//   rows r = (n, c), or c alone with batch_dice; per row
//   I = sum p y, P = sum p, Y = sum y, dice = (2I + eps) / (P + Y + eps),
//   loss = 1 - mean_r dice + ce_weight / (N S) * sum (lse - logit[label]).
// Two kernel families, each with a 16-byte and a scalar (VEC = 1) instance:
//   reg   2 <= C <= 8: a thread holds the C logits of VEC consecutive voxels
//         in registers (class cap 4 or 8, loops unrolled and predicated on
//         c < C); one global read, one exp per logit, no LDS tile.
//   tile  9 <= C <= 128: a block stages an fp32 [C][TV] tile of one sample
//         in LDS (TV = 512 / 256 / 128 / 64 voxels by what fits 60 KB), a
//         voxel-parallel phase takes max and sum (or the backward's dot over
//         the classes) and writes exp back into the tile, a class-parallel
//         phase (lane = class, bank-rotated voxel order) keeps the per-class
//         sums in registers; in the backward it is the row-wise store loop.
// A block belongs to one sample (blockIdx.x = n * chunks + chunk) and strides
// over that sample's vectors or tiles. Float sums: thread -> wave -> block ->
// one column entry per block in the [2C + 1, grid] partial buffer (P, I, ce)
// -> the finish kernel, where one wave per row adds that row's blocks in
// fixed order and writes the loss and the backward's (a_r, b_r) table. No
// float atomics; label counts are integers (LDS int atomics, int partials).
// Nothing here synchronises the host.
#include "segcommon.h"

#include <limits>

namespace {

constexpr int SD_MAX_C = 128;
constexpr int SD_REG_C = 8;              // register path up to here
constexpr int SD_REG_GRID = 2048;        // blocks, as elem_grid
constexpr int SD_TILE_GRID = 1024;       // 2 blocks of <= 60 KB LDS per CU
constexpr int SD_LDS_BYTES = 60 * 1024;  // dynamic; block_sum's static on top
constexpr int SD_WAVES = ELEM_BLOCK / WAVE_SIZE;

// the label as a class index, -1 when the voxel is dropped
template <typename L>
__device__ inline int keep_label(L t, int C) {
  const int64_t v = (int64_t)t;
  return (v >= 0 && v < C) ? (int)v : -1;
}

__device__ inline int wave_sum(int v) {
  for (int off = WAVE_SIZE / 2; off > 0; off >>= 1)
    v += __shfl_down(v, off, WAVE_SIZE);
  return v;
}

__device__ inline float wave_sum(float v) {
  for (int off = WAVE_SIZE / 2; off > 0; off >>= 1)
    v += __shfl_down(v, off, WAVE_SIZE);
  return v;
}

}  // namespace

// ------------------------------------------------------------ reg forward
// partial column layout (both paths): [P_0..P_{C-1}, I_0..I_{C-1}, ce],
// entry (k, block) at partial[k * grid + block]; ycnt[c * grid + block].
template <typename T, typename L, int VEC, int CAP>
__global__ void __launch_bounds__(ELEM_BLOCK)
seg_sdice_reg_fwd_kernel(const T* __restrict__ x, const L* __restrict__ t,
                         float* __restrict__ lse, float* __restrict__ partial,
                         int* __restrict__ ycnt, int C, int64_t S,
                         int chunks) {
  __shared__ int s_y[CAP];
  const int n = blockIdx.x / chunks;
  const int chunk = blockIdx.x - n * chunks;
  const int grid = gridDim.x;
  if (threadIdx.x < CAP) s_y[threadIdx.x] = 0;
  __syncthreads();
  float acc[2 * CAP + 1];
  int cnt[CAP];
#pragma unroll
  for (int k = 0; k < 2 * CAP + 1; ++k) acc[k] = 0.0f;
#pragma unroll
  for (int c = 0; c < CAP; ++c) cnt[c] = 0;
  const T* xn = x + (int64_t)n * C * S;
  const L* tn = t + (int64_t)n * S;
  float* ln = lse + (int64_t)n * S;
  const int64_t svec = S / VEC;  // exact: the launcher checks S % VEC == 0
  for (int64_t i = (int64_t)chunk * ELEM_BLOCK + threadIdx.x; i < svec;
       i += (int64_t)chunks * ELEM_BLOCK) {
    const int64_t s = i * VEC;
    const Vec<L, VEC> tv = ldv<L, VEC>(tn + s);
    float e[CAP][VEC];
#pragma unroll
    for (int c = 0; c < CAP; ++c) {
      if (c < C) {
        const Vec<T, VEC> xv = ldv<T, VEC>(xn + (int64_t)c * S + s);
#pragma unroll
        for (int j = 0; j < VEC; ++j) e[c][j] = (float)xv.v[j];
      }
    }
    Vec<float, VEC> lv;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int lab = keep_label(tv.v[j], C);
      float m = e[0][j];
#pragma unroll
      for (int c = 1; c < CAP; ++c)
        if (c < C) m = fmaxf(m, e[c][j]);
      float sum = 0.0f, pick = 0.0f;
#pragma unroll
      for (int c = 0; c < CAP; ++c) {
        if (c < C) {
          const float d = e[c][j] - m;
          if (lab == c) pick = d;
          e[c][j] = __expf(d);
          sum += e[c][j];
        }
      }
      const float lg = __logf(sum);
      lv.v[j] = m + lg;
      const float inv = lab >= 0 ? 1.0f / sum : 0.0f;  // dropped: p = 0
      acc[2 * CAP] += lab >= 0 ? lg - pick : 0.0f;
#pragma unroll
      for (int c = 0; c < CAP; ++c) {
        if (c < C) {
          const float p = e[c][j] * inv;
          acc[c] += p;
          acc[CAP + c] += lab == c ? p : 0.0f;
          cnt[c] += lab == c;
        }
      }
    }
    stv<float, VEC>(ln + s, lv);
  }
#pragma unroll
  for (int c = 0; c < CAP; ++c) {
    const int v = wave_sum(cnt[c]);
    if ((threadIdx.x % WAVE_SIZE) == 0 && v) atomicAdd(&s_y[c], v);
  }
  const float tot = block_sum<2 * CAP + 1>(acc);  // its barriers cover s_y
  const int k = threadIdx.x;
  if (k < CAP) {
    if (k < C) {
      partial[(int64_t)k * grid + blockIdx.x] = tot;
      ycnt[(int64_t)k * grid + blockIdx.x] = s_y[k];
    }
  } else if (k < 2 * CAP) {
    if (k - CAP < C) partial[(int64_t)(C + k - CAP) * grid + blockIdx.x] = tot;
  } else if (k == 2 * CAP) {
    partial[(int64_t)2 * C * grid + blockIdx.x] = tot;
  }
}

// ------------------------------------------------------------ finish
// One block. Wave w takes rows w, w + 4, ...: its lanes stride over the
// row's blocks, a shuffle tree adds the lanes, lane 0 writes
//   a_r = -2 / (K den_r), b_r = num_r / (K den_r^2)   (0 for excluded rows)
// and keeps the wave's dice sum; the four wave sums are added in order.
__global__ void __launch_bounds__(ELEM_BLOCK)
seg_sdice_finish_kernel(const float* __restrict__ partial,
                        const int* __restrict__ ycnt, int N, int C, int chunks,
                        int batch_dice, int include_bg, float eps,
                        float ce_scale, float* __restrict__ coef,
                        float* __restrict__ loss) {
  __shared__ float s_dice[SD_WAVES];
  const int grid = N * chunks;
  const int R = batch_dice ? C : N * C;
  const float K = (float)(include_bg ? R : R - R / C);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  float dsum = 0.0f;
  for (int r = wave; r < R; r += SD_WAVES) {
    const int c = r % C;
    const int first = batch_dice ? 0 : (r / C) * chunks;
    const int count = batch_dice ? grid : chunks;
    const float* pP = partial + (int64_t)c * grid + first;
    const float* pI = partial + (int64_t)(C + c) * grid + first;
    const int* pY = ycnt + (int64_t)c * grid + first;
    float P = 0.0f, I = 0.0f;
    long long Y = 0;
    for (int b = lane; b < count; b += WAVE_SIZE) {
      P += pP[b];
      I += pI[b];
      Y += pY[b];
    }
    P = wave_sum(P);
    I = wave_sum(I);
    for (int off = WAVE_SIZE / 2; off > 0; off >>= 1)
      Y += __shfl_down(Y, off, WAVE_SIZE);
    if (lane == 0) {
      float a = 0.0f, b = 0.0f;
      if (include_bg || c != 0) {
        const float num = 2.0f * I + eps;
        const float den = P + (float)Y + eps;
        dsum += num / den;
        a = -2.0f / (K * den);
        b = num / (K * den * den);
      }
      coef[2 * r] = a;
      coef[2 * r + 1] = b;
    }
  }
  if (lane == 0) s_dice[wave] = dsum;
  const float ce = sum_rows<1>(partial + (int64_t)2 * C * grid, grid);
  if (threadIdx.x == 0) {
    float d = 0.0f;
    for (int w = 0; w < SD_WAVES; ++w) d += s_dice[w];
    loss[0] = 1.0f - d / K + ce_scale * ce;
  }
}

// ------------------------------------------------------------ reg backward
// g_k = go * (p_k (b_k + a_k [k == t] - dot) + ce_scale (p_k - [k == t])),
// dot = sum_j p_j b_j + a_t p_t; go is folded into a, b and ce_scale.
template <typename T, typename L, int VEC, int CAP>
__global__ void __launch_bounds__(ELEM_BLOCK)
seg_sdice_reg_bwd_kernel(const T* __restrict__ x, const L* __restrict__ t,
                         const float* __restrict__ lse,
                         const float* __restrict__ coef,
                         const float* __restrict__ grad_out,
                         T* __restrict__ gx, float ce_scale, int C, int64_t S,
                         int chunks, int batch_dice) {
  const int n = blockIdx.x / chunks;
  const int chunk = blockIdx.x - n * chunks;
  const float go = grad_out[0];
  const float cs = ce_scale * go;
  float a[CAP], b[CAP];
#pragma unroll
  for (int c = 0; c < CAP; ++c) {
    a[c] = b[c] = 0.0f;
    if (c < C) {
      const float* cf = coef + 2 * ((batch_dice ? 0 : n * C) + c);
      a[c] = cf[0] * go;
      b[c] = cf[1] * go;
    }
  }
  const int64_t base = (int64_t)n * C * S;
  const L* tn = t + (int64_t)n * S;
  const float* ln = lse + (int64_t)n * S;
  const int64_t svec = S / VEC;
  for (int64_t i = (int64_t)chunk * ELEM_BLOCK + threadIdx.x; i < svec;
       i += (int64_t)chunks * ELEM_BLOCK) {
    const int64_t s = i * VEC;
    const Vec<L, VEC> tv = ldv<L, VEC>(tn + s);
    const Vec<float, VEC> lv = ldv<float, VEC>(ln + s);
    int lab[VEC];
    float dot[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      lab[j] = keep_label(tv.v[j], C);
      dot[j] = 0.0f;
    }
    float p[CAP][VEC];
#pragma unroll
    for (int c = 0; c < CAP; ++c) {
      if (c < C) {
        const Vec<T, VEC> xv = ldv<T, VEC>(x + base + (int64_t)c * S + s);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          p[c][j] = __expf((float)xv.v[j] - lv.v[j]);
          dot[j] += p[c][j] * (b[c] + (lab[j] == c ? a[c] : 0.0f));
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CAP; ++c) {
      if (c < C) {
        Vec<T, VEC> gv;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const bool hit = lab[j] == c;
          const float g = p[c][j] * (b[c] + (hit ? a[c] : 0.0f) - dot[j]) +
                          cs * (p[c][j] - (hit ? 1.0f : 0.0f));
          gv.v[j] = (T)(lab[j] >= 0 ? g : 0.0f);
        }
        stv<T, VEC>(gx + base + (int64_t)c * S + s, gv);
      }
    }
  }
}

// ------------------------------------------------------------ tile path
namespace {

// Dynamic LDS of the tile kernels, in 4-byte words. The forward's layout is
// the larger: tile [C][TV], inv [TV], label [TV], two slice rows
// [max(TV, 256)]; 3C more cover the backward's a and b rows.
inline size_t tile_lds_bytes(int C, int tv) {
  const int red = tv > ELEM_BLOCK ? tv : ELEM_BLOCK;
  return 4 * ((size_t)C * tv + 2 * tv + 2 * red + 3 * C);
}

// largest power of two in [64, 512] whose forward layout fits the budget:
// C <= 25: 512, <= 55: 256, <= 111: 128, <= 128: 64
inline int tile_voxels(int C) {
  for (int tv = 512; tv > 64; tv >>= 1)
    if (tile_lds_bytes(C, tv) <= (size_t)SD_LDS_BYTES) return tv;
  return 64;
}

// Stage the fp32 [C][TV] tile of voxels s0 .. s0 + nv of one sample and the
// labels; voxels past nv read as logit 0 / dropped.
template <typename T, typename L, int VEC>
__device__ inline void load_tile(const T* __restrict__ xn,
                                 const L* __restrict__ tn, float* s_tile,
                                 int* s_lab, int C, int64_t S, int64_t s0,
                                 int nv, int TV, int tv_shift) {
  constexpr int VSH = VEC == 8 ? 3 : VEC == 4 ? 2 : 0;
  const int row_shift = tv_shift - VSH;
  const int units = C << row_shift;
  for (int idx = threadIdx.x; idx < units; idx += ELEM_BLOCK) {
    const int c = idx >> row_shift;
    const int v = (idx - (c << row_shift)) << VSH;
    Vec<float, VEC> fv;
    if (v < nv) {  // S % VEC == 0: a vector is inside or outside as a whole
      const Vec<T, VEC> xv = ldv<T, VEC>(xn + (int64_t)c * S + s0 + v);
#pragma unroll
      for (int j = 0; j < VEC; ++j) fv.v[j] = (float)xv.v[j];
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) fv.v[j] = 0.0f;
    }
    stv<float, VEC>(s_tile + c * TV + v, fv);
  }
  for (int v = threadIdx.x; v < TV; v += ELEM_BLOCK)
    s_lab[v] = v < nv ? keep_label(tn[s0 + v], C) : -1;
}

}  // namespace

// Phase A items are (slice q, voxel v): with TV < 256 the 256 threads split
// the classes of a voxel into Q = 256 / TV slices (c = q, q + Q, ...) and
// combine through s_red / s_sum in fixed order; with TV >= 256, Q = 1.
template <typename T, typename L, int VEC>
__global__ void __launch_bounds__(ELEM_BLOCK)
seg_sdice_tile_fwd_kernel(const T* __restrict__ x, const L* __restrict__ t,
                          float* __restrict__ lse, float* __restrict__ partial,
                          int* __restrict__ ycnt, int C, int64_t S, int TV,
                          int tv_shift, int chunks) {
  extern __shared__ __attribute__((aligned(16))) char sdice_smem[];
  const int RED = TV > ELEM_BLOCK ? TV : ELEM_BLOCK;
  float* s_tile = reinterpret_cast<float*>(sdice_smem);  // [C][TV]
  float* s_inv = s_tile + C * TV;                        // [TV]
  int* s_lab = reinterpret_cast<int*>(s_inv + TV);       // [TV]
  float* s_red = reinterpret_cast<float*>(s_lab + TV);   // [RED] slice max
  float* s_sum = s_red + RED;                            // [RED] slice sum
  // after the last tile the tile's first 12C words hold the waves' sums
  float* s_fin = s_tile;                                 // [4][2][C] P, I
  int* s_cnt = reinterpret_cast<int*>(s_tile + 8 * C);   // [4][C]
  const int n = blockIdx.x / chunks;
  const int chunk = blockIdx.x - n * chunks;
  const int grid = gridDim.x;
  const int Q = TV < ELEM_BLOCK ? ELEM_BLOCK / TV : 1;
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  float accP[2] = {0.0f, 0.0f}, accI[2] = {0.0f, 0.0f};
  int accY[2] = {0, 0};
  const T* xn = x + (int64_t)n * C * S;
  const L* tn = t + (int64_t)n * S;
  float* ln = lse + (int64_t)n * S;
  const int64_t tiles = (S + TV - 1) >> tv_shift;
  float ce[1] = {0.0f};
  for (int64_t tile = chunk; tile < tiles; tile += chunks) {
    const int64_t s0 = tile << tv_shift;
    const int nv = (int)(S - s0 < TV ? S - s0 : TV);
    load_tile<T, L, VEC>(xn, tn, s_tile, s_lab, C, S, s0, nv, TV, tv_shift);
    __syncthreads();
    // A1: slice max, no exp
    for (int item = threadIdx.x; item < RED; item += ELEM_BLOCK) {
      const int v = item & (TV - 1);
      float m = -std::numeric_limits<float>::infinity();
      for (int c = item >> tv_shift; c < C; c += Q)
        m = fmaxf(m, s_tile[c * TV + v]);
      s_red[item] = m;
    }
    __syncthreads();
    // A2: e = exp(x - m) back into the tile (the one exp per logit), slice
    // sum; the label's x - m goes to s_inv for the CE term
    for (int item = threadIdx.x; item < RED; item += ELEM_BLOCK) {
      const int v = item & (TV - 1);
      float m = s_red[v];
      for (int q = 1; q < Q; ++q) m = fmaxf(m, s_red[q * TV + v]);
      const int lab = s_lab[v];
      float sum = 0.0f;
      for (int c = item >> tv_shift; c < C; c += Q) {
        const float d = s_tile[c * TV + v] - m;
        if (c == lab) s_inv[v] = d;
        const float e = __expf(d);
        s_tile[c * TV + v] = e;
        sum += e;
      }
      s_sum[item] = sum;
    }
    __syncthreads();
    // A3: per voxel lse, CE term and 1 / sum (0 for a dropped voxel: p = 0)
    for (int v = threadIdx.x; v < TV; v += ELEM_BLOCK) {
      float m = s_red[v], sum = s_sum[v];
      for (int q = 1; q < Q; ++q) {
        m = fmaxf(m, s_red[q * TV + v]);
        sum += s_sum[q * TV + v];
      }
      const float lg = __logf(sum);
      if (v < nv) ln[s0 + v] = m + lg;
      const bool kept = s_lab[v] >= 0;
      if (kept) ce[0] += lg - s_inv[v];
      s_inv[v] = kept ? 1.0f / sum : 0.0f;
    }
    __syncthreads();
    // B: class-parallel. Lane l owns classes l and l + 64 and keeps their
    // sums in registers over all the block's tiles: no reduction per tile.
    // Within a group of 64 voxels, lane l reads voxel (k + l) % 64 at step
    // k, so the 64 lanes hit 64 different banks (rows are a multiple of 64
    // words apart); wave w takes steps 16w .. 16w + 15 of every group.
    for (int g = 0; g < TV; g += WAVE_SIZE) {
      for (int k = wave * 16; k < wave * 16 + 16; ++k) {
        const int v = g + ((k + lane) & (WAVE_SIZE - 1));
        const float inv = s_inv[v];
        const int lab = s_lab[v];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int c = lane + h * WAVE_SIZE;
          if (c < C) {
            const float p = s_tile[c * TV + v] * inv;
            const bool hit = lab == c;
            accP[h] += p;
            accI[h] += hit ? p : 0.0f;
            accY[h] += hit;
          }
        }
      }
    }
    __syncthreads();
  }
  // the four waves' sums of a class, added in wave order
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + h * WAVE_SIZE;
    if (c < C) {
      s_fin[(wave * 2 + 0) * C + c] = accP[h];
      s_fin[(wave * 2 + 1) * C + c] = accI[h];
      s_cnt[wave * C + c] = accY[h];
    }
  }
  const float tot = block_sum<1>(ce);  // its barriers cover s_fin / s_cnt
  for (int k = threadIdx.x; k < 2 * C; k += ELEM_BLOCK) {
    const int c = k < C ? k : k - C, which = k < C ? 0 : 1;
    float sum = 0.0f;
    for (int w = 0; w < SD_WAVES; ++w) sum += s_fin[(w * 2 + which) * C + c];
    partial[(int64_t)k * grid + blockIdx.x] = sum;
  }
  for (int c = threadIdx.x; c < C; c += ELEM_BLOCK) {
    int sum = 0;
    for (int w = 0; w < SD_WAVES; ++w) sum += s_cnt[w * C + c];
    ycnt[(int64_t)c * grid + blockIdx.x] = sum;
  }
  if (threadIdx.x == 0) partial[(int64_t)2 * C * grid + blockIdx.x] = tot;
}

// Backward: A1 writes p = exp(x - lse) into the tile (one exp per logit) and
// the slice's part of sum_j p_j b_j; A2 adds a_t p_t per voxel; the store
// loop walks the rows with 16-byte stores. LDS: tile, dot [TV] (holds lse
// until A1 is over), label [TV], slice row, a and b [2C].
template <typename T, typename L, int VEC>
__global__ void __launch_bounds__(ELEM_BLOCK)
seg_sdice_tile_bwd_kernel(const T* __restrict__ x, const L* __restrict__ t,
                          const float* __restrict__ lse,
                          const float* __restrict__ coef,
                          const float* __restrict__ grad_out,
                          T* __restrict__ gx, float ce_scale, int C, int64_t S,
                          int TV, int tv_shift, int chunks, int batch_dice) {
  extern __shared__ __attribute__((aligned(16))) char sdice_smem[];
  const int RED = TV > ELEM_BLOCK ? TV : ELEM_BLOCK;
  float* s_tile = reinterpret_cast<float*>(sdice_smem);  // [C][TV]
  float* s_dot = s_tile + C * TV;                        // [TV]
  int* s_lab = reinterpret_cast<int*>(s_dot + TV);       // [TV]
  float* s_red = reinterpret_cast<float*>(s_lab + TV);   // [RED]
  float* s_a = s_red + RED;                              // [C]
  float* s_b = s_a + C;                                  // [C]
  constexpr int VSH = VEC == 8 ? 3 : VEC == 4 ? 2 : 0;
  const int n = blockIdx.x / chunks;
  const int chunk = blockIdx.x - n * chunks;
  const int Q = TV < ELEM_BLOCK ? ELEM_BLOCK / TV : 1;
  const float go = grad_out[0];
  const float cs = ce_scale * go;
  for (int c = threadIdx.x; c < C; c += ELEM_BLOCK) {
    const float* cf = coef + 2 * ((batch_dice ? 0 : n * C) + c);
    s_a[c] = cf[0] * go;
    s_b[c] = cf[1] * go;
  }
  const T* xn = x + (int64_t)n * C * S;
  T* gn = gx + (int64_t)n * C * S;
  const L* tn = t + (int64_t)n * S;
  const float* ln = lse + (int64_t)n * S;
  const int64_t tiles = (S + TV - 1) >> tv_shift;
  const int row_shift = tv_shift - VSH;
  const int units = C << row_shift;
  for (int64_t tile = chunk; tile < tiles; tile += chunks) {
    const int64_t s0 = tile << tv_shift;
    const int nv = (int)(S - s0 < TV ? S - s0 : TV);
    load_tile<T, L, VEC>(xn, tn, s_tile, s_lab, C, S, s0, nv, TV, tv_shift);
    for (int v = threadIdx.x; v < TV; v += ELEM_BLOCK)
      s_dot[v] = v < nv ? ln[s0 + v] : 0.0f;
    __syncthreads();  // also covers s_a / s_b
    for (int item = threadIdx.x; item < RED; item += ELEM_BLOCK) {
      const int v = item & (TV - 1);
      const float l = s_dot[v];
      float part = 0.0f;
      for (int c = item >> tv_shift; c < C; c += Q) {
        const float p = __expf(s_tile[c * TV + v] - l);
        s_tile[c * TV + v] = p;
        part += p * s_b[c];
      }
      s_red[item] = part;
    }
    __syncthreads();
    for (int v = threadIdx.x; v < TV; v += ELEM_BLOCK) {
      float dot = s_red[v];
      for (int q = 1; q < Q; ++q) dot += s_red[q * TV + v];
      const int lab = s_lab[v];
      if (lab >= 0) dot += s_a[lab] * s_tile[lab * TV + v];
      s_dot[v] = dot;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < units; idx += ELEM_BLOCK) {
      const int c = idx >> row_shift;
      const int v = (idx - (c << row_shift)) << VSH;
      if (v >= nv) continue;
      const float ac = s_a[c], bc = s_b[c];
      Vec<T, VEC> gv;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int lab = s_lab[v + j];
        const float p = s_tile[c * TV + v + j];
        const bool hit = lab == c;
        const float g = p * (bc + (hit ? ac : 0.0f) - s_dot[v + j]) +
                        cs * (p - (hit ? 1.0f : 0.0f));
        gv.v[j] = (T)(lab >= 0 ? g : 0.0f);
      }
      stv<T, VEC>(gn + (int64_t)c * S + s0 + v, gv);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- host side
namespace {

struct SdiceArgs {
  torch::Tensor x, t;
  int64_t N, S;
  int C;
};

SdiceArgs sdice_args(const torch::Tensor& logits,
                     const torch::Tensor& target) {
  CHECK_GPU(logits);
  CHECK_GPU(target);
  TORCH_CHECK(logits.dim() >= 3, "seg_sdice: logits must be [N, C, S...]");
  const int64_t C = logits.size(1);
  TORCH_CHECK(C != 1, "seg_sdice: C == 1 is the binary case, use "
                      "dice_loss_with_logits");
  TORCH_CHECK(C >= 2 && C <= SD_MAX_C, "seg_sdice: C = ", C,
              " is outside [2, ", SD_MAX_C, "]");
  SdiceArgs a;
  a.x = logits.contiguous();
  a.t = target.contiguous();
  a.N = a.x.size(0);
  a.C = (int)C;
  TORCH_CHECK(a.N >= 1 && a.x.numel() > 0, "seg_sdice: empty logits");
  a.S = a.x.numel() / (a.N * a.C);
  TORCH_CHECK(a.t.numel() == a.N * a.S,
              "seg_sdice: target must be [N, S...] with logits' spatial "
              "extent");
  TORCH_CHECK(a.S < (int64_t)1 << 31, "seg_sdice: S must be below 2^31");
  return a;
}

// blocks per sample: every block of work up to the grid cap shared by the
// N samples. `units` is the sample's 16-byte vectors / 256 (reg) or tiles.
inline int sample_chunks(int64_t units, int64_t N, int cap) {
  const int64_t most = cap / N > 1 ? cap / N : 1;
  const int64_t chunks = units < most ? units : most;
  TORCH_CHECK(chunks * N < (int64_t)1 << 31, "seg_sdice: N too large");
  return (int)(chunks < 1 ? 1 : chunks);
}

inline int log2_of(int pow2) {
  int s = 0;
  while ((1 << s) < pow2) ++s;
  return s;
}

}  // namespace

std::vector<torch::Tensor> seg_sdice_fwd(torch::Tensor logits,
                                         torch::Tensor target,
                                         double ce_weight,
                                         bool include_background,
                                         bool batch_dice, double eps) {
  SdiceArgs a = sdice_args(logits, target);
  auto fopt = a.x.options().dtype(torch::kFloat32);
  const int64_t R = batch_dice ? a.C : a.N * a.C;
  auto lse = torch::empty({a.N, a.S}, fopt);
  auto coef = torch::empty({R, 2}, fopt);
  auto loss = torch::empty({}, fopt);
  const float ce_scale = (float)(ce_weight / ((double)a.N * (double)a.S));
  dispatch_logits(a.x.scalar_type(), [&](auto tt) {
    using T = decltype(tt);
    constexpr int V = vec_width<T>();
    dispatch_labels<T, false>(a.t.scalar_type(), [&](auto ll) {
      using L = decltype(ll);
      const T* xp = static_cast<const T*>(a.x.data_ptr());
      const L* tp = static_cast<const L*>(a.t.data_ptr());
      float* lp = lse.data_ptr<float>();
      const bool vec = vec_ok<T, L>(xp, tp) && aligned_to(lp, 16) &&
                       a.S % V == 0;
      const bool reg = a.C <= SD_REG_C;
      const int tv = tile_voxels(a.C);
      const int64_t units =
          reg ? ((vec ? a.S / V : a.S) + ELEM_BLOCK - 1) / ELEM_BLOCK
              : (a.S + tv - 1) / tv;
      const int chunks =
          sample_chunks(units, a.N, reg ? SD_REG_GRID : SD_TILE_GRID);
      const int grid = (int)(a.N * chunks);
      auto partial = torch::empty({2 * a.C + 1, grid}, fopt);
      auto ycnt = torch::empty({a.C, grid}, fopt.dtype(torch::kInt32));
      float* pp = partial.data_ptr<float>();
      int* yp = ycnt.data_ptr<int>();
      auto launch = [&](auto vv) {
        constexpr int VEC = decltype(vv)::value;
        if (reg) {
          if (a.C <= 4)
            hipLaunchKernelGGL((seg_sdice_reg_fwd_kernel<T, L, VEC, 4>),
                               dim3(grid), dim3(ELEM_BLOCK), 0,
                               current_stream(), xp, tp, lp, pp, yp, a.C, a.S,
                               chunks);
          else
            hipLaunchKernelGGL((seg_sdice_reg_fwd_kernel<T, L, VEC, 8>),
                               dim3(grid), dim3(ELEM_BLOCK), 0,
                               current_stream(), xp, tp, lp, pp, yp, a.C, a.S,
                               chunks);
        } else {
          hipLaunchKernelGGL((seg_sdice_tile_fwd_kernel<T, L, VEC>),
                             dim3(grid), dim3(ELEM_BLOCK),
                             tile_lds_bytes(a.C, tv), current_stream(), xp, tp,
                             lp, pp, yp, a.C, a.S, tv, log2_of(tv), chunks);
        }
      };
      if (vec) launch(IntC<V>{});
      else launch(IntC<1>{});
      hipLaunchKernelGGL(seg_sdice_finish_kernel, dim3(1), dim3(ELEM_BLOCK), 0,
                         current_stream(), pp, yp, (int)a.N, a.C, chunks,
                         (int)batch_dice, (int)include_background, (float)eps,
                         ce_scale, coef.data_ptr<float>(),
                         loss.data_ptr<float>());
    });
  });
  return {loss, lse, coef};
}

torch::Tensor seg_sdice_bwd(torch::Tensor logits, torch::Tensor target,
                            torch::Tensor lse, torch::Tensor coef,
                            torch::Tensor grad_out, double ce_weight) {
  SdiceArgs a = sdice_args(logits, target);
  CHECK_GPU(lse);
  CHECK_GPU(coef);
  CHECK_GPU(grad_out);
  TORCH_CHECK(lse.scalar_type() == at::ScalarType::Float &&
              lse.numel() == a.N * a.S && lse.is_contiguous(),
              "seg_sdice: lse must be contiguous fp32 [N, S]");
  TORCH_CHECK(coef.scalar_type() == at::ScalarType::Float &&
              coef.is_contiguous() && coef.dim() == 2 && coef.size(1) == 2 &&
              (coef.size(0) == a.C || coef.size(0) == a.N * a.C),
              "seg_sdice: coef must be contiguous fp32 [C, 2] or [N*C, 2]");
  // N == 1 makes the two row layouts the same table
  const bool batch_dice = coef.size(0) == a.C;
  auto go = grad_out.to(torch::kFloat32).contiguous();
  TORCH_CHECK(go.numel() == 1, "seg_sdice: grad_out must be a scalar");
  auto gx = torch::empty_like(a.x);
  const float ce_scale = (float)(ce_weight / ((double)a.N * (double)a.S));
  dispatch_logits(a.x.scalar_type(), [&](auto tt) {
    using T = decltype(tt);
    constexpr int V = vec_width<T>();
    dispatch_labels<T, false>(a.t.scalar_type(), [&](auto ll) {
      using L = decltype(ll);
      const T* xp = static_cast<const T*>(a.x.data_ptr());
      const L* tp = static_cast<const L*>(a.t.data_ptr());
      const float* lp = lse.data_ptr<float>();
      const float* cp = coef.data_ptr<float>();
      const float* gop = go.data_ptr<float>();
      T* gp = static_cast<T*>(gx.data_ptr());
      const bool vec = vec_ok<T, L>(xp, tp) && aligned_to(gp, 16) &&
                       aligned_to(lp, 16) && a.S % V == 0;
      const bool reg = a.C <= SD_REG_C;
      const int tv = tile_voxels(a.C);
      const int64_t units =
          reg ? ((vec ? a.S / V : a.S) + ELEM_BLOCK - 1) / ELEM_BLOCK
              : (a.S + tv - 1) / tv;
      const int chunks =
          sample_chunks(units, a.N, reg ? SD_REG_GRID : SD_TILE_GRID);
      const int grid = (int)(a.N * chunks);
      auto launch = [&](auto vv) {
        constexpr int VEC = decltype(vv)::value;
        if (reg) {
          if (a.C <= 4)
            hipLaunchKernelGGL((seg_sdice_reg_bwd_kernel<T, L, VEC, 4>),
                               dim3(grid), dim3(ELEM_BLOCK), 0,
                               current_stream(), xp, tp, lp, cp, gop, gp,
                               ce_scale, a.C, a.S, chunks, (int)batch_dice);
          else
            hipLaunchKernelGGL((seg_sdice_reg_bwd_kernel<T, L, VEC, 8>),
                               dim3(grid), dim3(ELEM_BLOCK), 0,
                               current_stream(), xp, tp, lp, cp, gop, gp,
                               ce_scale, a.C, a.S, chunks, (int)batch_dice);
        } else {
          hipLaunchKernelGGL((seg_sdice_tile_bwd_kernel<T, L, VEC>),
                             dim3(grid), dim3(ELEM_BLOCK),
                             tile_lds_bytes(a.C, tv), current_stream(), xp, tp,
                             lp, cp, gop, gp, ce_scale, a.C, a.S, tv,
                             log2_of(tv), chunks, (int)batch_dice);
        }
      };
      if (vec) launch(IntC<V>{});
      else launch(IntC<1>{});
    });
  });
  return gx;
}
