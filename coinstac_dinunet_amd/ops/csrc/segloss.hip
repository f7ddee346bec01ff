// Segmentation head — fused voxelwise losses and metrics from logits.
//   (a/b) binary soft-dice from logits, fwd + bwd (sigmoid recomputed, no
//         probability tensor saved)
//   (c)   voxelwise softmax cross-entropy over [N, C, S...] logits (class
//         stride S), fwd (online max/sum, lse saved as fp32 [N, S]) + bwd
//   (d)   tp/fp/tn/fn from logits: pred = (x > 0), truth = (label != 0)
//   (e)   KxK confusion from logits: argmax over class planes, lowest index
//         wins ties, LDS int histogram -> int64 atomics
// Streaming kernels: 256-thread blocks, grid-stride under the elem_grid cap,
// 16 B per lane on logits and grad stores (8 x bf16/fp16, 4 x fp32). Labels
// are read in their own dtype. The scalar instance (VEC = 1) runs when a
// base pointer is not aligned for the vector or, for the class-strided
// kernels, when S is no multiple of the vector width (plane c starts at c*S).
// The flat kernels (dice, counts) finish a tail shorter than a vector scalar.
// Float sums are reproducible: thread -> wave (__shfl_down) -> block (LDS)
// -> one partial row per block in a [grid, k] buffer -> a one-block finish
// kernel sums the rows in fixed order. No float atomics; integer counts use
// integer atomics as metrics.hip does. Nothing here synchronises the host.
#include "common.h"

namespace {

template <typename T, int N>
struct alignas((sizeof(T) * N < 16 ? sizeof(T) * N : 16)) Vec {
  T v[N];
};

template <typename T>
constexpr int vec_width() { return 16 / (int)sizeof(T); }

template <typename T, int N>
__device__ inline Vec<T, N> ldv(const T* p) {
  return *reinterpret_cast<const Vec<T, N>*>(p);
}

template <typename T, int N>
__device__ inline void stv(T* p, const Vec<T, N>& v) {
  *reinterpret_cast<Vec<T, N>*>(p) = v;
}

// p = sigmoid(x) and q = p(1-p) from e = exp(-|x|) in (0, 1]: no overflow,
// |x| >= ~100 gives p in {0, 1} and q = 0, never NaN.
__device__ inline void sigmoid_pq(float x, float& p, float& q) {
  const float e = __expf(-fabsf(x));
  const float r = 1.0f / (1.0f + e);
  p = x >= 0.0f ? r : e * r;
  q = e * r * r;
}

// Block-wide sum of K per-thread values; thread k < K returns the total of
// value k (others return garbage). Fixed order: lanes by shuffle tree, then
// waves 0..3 in sequence.
template <int K>
__device__ inline float block_sum(float (&acc)[K]) {
  __shared__ float s_part[ELEM_BLOCK / WAVE_SIZE][K];
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int off = WAVE_SIZE / 2; off > 0; off >>= 1)
      acc[k] += __shfl_down(acc[k], off, WAVE_SIZE);
  const int wave = threadIdx.x / WAVE_SIZE;
  if ((threadIdx.x % WAVE_SIZE) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_part[wave][k] = acc[k];
  }
  __syncthreads();
  float tot = 0.0f;
  if (threadIdx.x < K) {
    for (int w = 0; w < ELEM_BLOCK / WAVE_SIZE; ++w)
      tot += s_part[w][threadIdx.x];
  }
  __syncthreads();
  return tot;
}

// Column sums of the [rows, K] partial buffer by ONE block, fixed order.
template <int K>
__device__ inline float sum_rows(const float* __restrict__ partial, int rows) {
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0f;
  for (int r = threadIdx.x; r < rows; r += ELEM_BLOCK) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] += partial[(int64_t)r * K + k];
  }
  return block_sum<K>(acc);
}

}  // namespace

// ---------------------------------------------------------------- (a) dice
// partial row = [I, T, P] = [sum p t w^2, sum t w, sum p w]
template <typename T, typename L, bool HAS_W, int VEC>
__global__ void seg_dice_fwd_kernel(const T* __restrict__ x,
                                    const L* __restrict__ t,
                                    const float* __restrict__ w,
                                    float* __restrict__ partial, int64_t n) {
  float acc[3] = {0.0f, 0.0f, 0.0f};
  auto one = [&](float xv, float tv, float wv) {
    float p, q;
    sigmoid_pq(xv, p, q);
    acc[0] += p * tv * wv * wv;
    acc[1] += tv * wv;
    acc[2] += p * wv;
  };
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
  const int64_t nvec = n / VEC;
  for (int64_t i = tid; i < nvec; i += nthr) {
    const Vec<T, VEC> xv = ldv<T, VEC>(x + i * VEC);
    const Vec<L, VEC> tv = ldv<L, VEC>(t + i * VEC);
    Vec<float, VEC> wv;
    if (HAS_W) wv = ldv<float, VEC>(w + i * VEC);
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      one((float)xv.v[j], (float)tv.v[j], HAS_W ? wv.v[j] : 1.0f);
  }
  for (int64_t i = nvec * VEC + tid; i < n; i += nthr)  // tail (< VEC)
    one((float)x[i], (float)t[i], HAS_W ? w[i] : 1.0f);
  const float tot = block_sum<3>(acc);
  if (threadIdx.x < 3) partial[(int64_t)blockIdx.x * 3 + threadIdx.x] = tot;
}

// sums = [I, T, P]; loss = 1 - ((1+b2) I + eps) / (b2 T + P + eps)
__global__ void seg_dice_finish_kernel(const float* __restrict__ partial,
                                       int rows, float b2, float eps,
                                       float* __restrict__ sums,
                                       float* __restrict__ loss) {
  __shared__ float s_tot[3];
  const float tot = sum_rows<3>(partial, rows);
  if (threadIdx.x < 3) s_tot[threadIdx.x] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    sums[0] = s_tot[0];
    sums[1] = s_tot[1];
    sums[2] = s_tot[2];
    const float num = (1.0f + b2) * s_tot[0] + eps;
    const float den = b2 * s_tot[1] + s_tot[2] + eps;
    loss[0] = 1.0f - num / den;
  }
}

// ---------------------------------------------------------------- (b) dice bwd
// g = go * dL/dp * p(1-p), dL/dp = -((1+b2) t w^2 den - num w) / den^2
template <typename T, typename L, bool HAS_W, int VEC>
__global__ void seg_dice_bwd_kernel(const T* __restrict__ x,
                                    const L* __restrict__ t,
                                    const float* __restrict__ w,
                                    const float* __restrict__ sums,
                                    const float* __restrict__ grad_out,
                                    T* __restrict__ gx, float b2, float eps,
                                    int64_t n) {
  const float num = (1.0f + b2) * sums[0] + eps;
  const float den = b2 * sums[1] + sums[2] + eps;
  const float s = -grad_out[0] / (den * den);
  const float a = (1.0f + b2) * den;
  auto one = [&](float xv, float tv, float wv) -> float {
    float p, q;
    sigmoid_pq(xv, p, q);
    return s * (a * tv * wv * wv - num * wv) * q;
  };
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
  const int64_t nvec = n / VEC;
  for (int64_t i = tid; i < nvec; i += nthr) {
    const Vec<T, VEC> xv = ldv<T, VEC>(x + i * VEC);
    const Vec<L, VEC> tv = ldv<L, VEC>(t + i * VEC);
    Vec<float, VEC> wv;
    if (HAS_W) wv = ldv<float, VEC>(w + i * VEC);
    Vec<T, VEC> gv;
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      gv.v[j] = (T)one((float)xv.v[j], (float)tv.v[j],
                       HAS_W ? wv.v[j] : 1.0f);
    stv<T, VEC>(gx + i * VEC, gv);
  }
  for (int64_t i = nvec * VEC + tid; i < n; i += nthr)
    gx[i] = (T)one((float)x[i], (float)t[i], HAS_W ? w[i] : 1.0f);
}

// ---------------------------------------------------------------- (c) CE
// Thread owns VEC consecutive voxels of one sample and walks the C class
// planes once (online max/sum); the label's logit is picked by comparison in
// the same loop. A label outside [0, C) matches no plane: the voxel adds
// nothing to the loss. Vector instance needs S % VEC == 0.
template <typename T, typename L, int VEC>
__global__ void seg_ce_fwd_kernel(const T* __restrict__ x,
                                  const L* __restrict__ t,
                                  float* __restrict__ lse,
                                  float* __restrict__ partial, int64_t N,
                                  int C, int64_t S) {
  float acc[1] = {0.0f};
  const int64_t svec = S / VEC;  // exact: the launcher checks S % VEC == 0
  const int64_t nvec = N * svec;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / svec;
    const int64_t s = (i - n * svec) * VEC;
    const T* xp = x + n * C * S + s;
    const Vec<L, VEC> tv = ldv<L, VEC>(t + n * S + s);
    float m[VEC], sum[VEC], pick[VEC];
    bool hit[VEC];
    {
      const Vec<T, VEC> xv = ldv<T, VEC>(xp);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        m[j] = (float)xv.v[j];
        sum[j] = 1.0f;
        hit[j] = (int64_t)tv.v[j] == 0;
        pick[j] = hit[j] ? m[j] : 0.0f;
      }
    }
    for (int c = 1; c < C; ++c) {
      const Vec<T, VEC> xv = ldv<T, VEC>(xp + (int64_t)c * S);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float v = (float)xv.v[j];
        const float mn = fmaxf(m[j], v);
        sum[j] = sum[j] * __expf(m[j] - mn) + __expf(v - mn);
        m[j] = mn;
        if ((int64_t)tv.v[j] == c) { pick[j] = v; hit[j] = true; }
      }
    }
    Vec<float, VEC> lv;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      lv.v[j] = m[j] + __logf(sum[j]);
      if (hit[j]) acc[0] += lv.v[j] - pick[j];
    }
    stv<float, VEC>(lse + n * S + s, lv);
  }
  const float tot = block_sum<1>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void seg_ce_finish_kernel(const float* __restrict__ partial,
                                     int rows, float inv_count,
                                     float* __restrict__ loss) {
  const float tot = sum_rows<1>(partial, rows);
  if (threadIdx.x == 0) loss[0] = tot * inv_count;
}

// (exp(x - lse) - [c == label]) * grad_out / (N S), in the logits' dtype
template <typename T, typename L, int VEC>
__global__ void seg_ce_bwd_kernel(const T* __restrict__ x,
                                  const L* __restrict__ t,
                                  const float* __restrict__ lse,
                                  const float* __restrict__ grad_out,
                                  T* __restrict__ gx, float inv_count,
                                  int64_t N, int C, int64_t S) {
  const float scale = grad_out[0] * inv_count;
  const int64_t svec = S / VEC;
  const int64_t nvec = N * svec;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / svec;
    const int64_t s = (i - n * svec) * VEC;
    const int64_t base = n * C * S + s;
    const Vec<L, VEC> tv = ldv<L, VEC>(t + n * S + s);
    const Vec<float, VEC> lv = ldv<float, VEC>(lse + n * S + s);
    for (int c = 0; c < C; ++c) {
      const Vec<T, VEC> xv = ldv<T, VEC>(x + base + (int64_t)c * S);
      Vec<T, VEC> gv;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float p = __expf((float)xv.v[j] - lv.v[j]);
        const float oh = (int64_t)tv.v[j] == c ? 1.0f : 0.0f;
        gv.v[j] = (T)((p - oh) * scale);
      }
      stv<T, VEC>(gx + base + (int64_t)c * S, gv);
    }
  }
}

// ---------------------------------------------------------------- (d) counts
// counts = [tp, fp, tn, fn]; pred = (x > 0) so +0.0, -0.0 and NaN are
// negative; truth = (label != 0).
template <typename T, typename L, int VEC>
__global__ void seg_prf1a_kernel(const T* __restrict__ x,
                                 const L* __restrict__ t,
                                 int64_t* __restrict__ counts, int64_t n) {
  __shared__ int s_counts[4];
  if (threadIdx.x < 4) s_counts[threadIdx.x] = 0;
  __syncthreads();
  int tp = 0, fp = 0, tn = 0, fn = 0;
  auto one = [&](float xv, bool tr) {
    const bool p = xv > 0.0f;
    tp += p && tr;
    fp += p && !tr;
    tn += !p && !tr;
    fn += !p && tr;
  };
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
  const int64_t nvec = n / VEC;
  for (int64_t i = tid; i < nvec; i += nthr) {
    const Vec<T, VEC> xv = ldv<T, VEC>(x + i * VEC);
    const Vec<L, VEC> tv = ldv<L, VEC>(t + i * VEC);
#pragma unroll
    for (int j = 0; j < VEC; ++j) one((float)xv.v[j], tv.v[j] != 0);
  }
  for (int64_t i = nvec * VEC + tid; i < n; i += nthr)
    one((float)x[i], t[i] != 0);
  for (int off = WAVE_SIZE / 2; off > 0; off >>= 1) {
    tp += __shfl_down(tp, off, WAVE_SIZE);
    fp += __shfl_down(fp, off, WAVE_SIZE);
    tn += __shfl_down(tn, off, WAVE_SIZE);
    fn += __shfl_down(fn, off, WAVE_SIZE);
  }
  if ((threadIdx.x % WAVE_SIZE) == 0) {
    atomicAdd(&s_counts[0], tp);
    atomicAdd(&s_counts[1], fp);
    atomicAdd(&s_counts[2], tn);
    atomicAdd(&s_counts[3], fn);
  }
  __syncthreads();
  if (threadIdx.x < 4)
    atomicAdd(reinterpret_cast<unsigned long long*>(&counts[threadIdx.x]),
              (unsigned long long)s_counts[threadIdx.x]);
}

// ---------------------------------------------------------------- (e) confusion
// mat[true][pred]; pred = argmax over the C = K planes with strict '>' so
// the lowest index wins ties. Labels outside [0, K) are dropped.
template <typename T, typename L, int VEC>
__global__ void seg_confusion_kernel(const T* __restrict__ x,
                                     const L* __restrict__ t,
                                     int64_t* __restrict__ mat, int64_t N,
                                     int K, int64_t S) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  int* s_mat = reinterpret_cast<int*>(smem_raw);
  const int kk = K * K;
  for (int i = threadIdx.x; i < kk; i += blockDim.x) s_mat[i] = 0;
  __syncthreads();
  const int64_t svec = S / VEC;
  const int64_t nvec = N * svec;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / svec;
    const int64_t s = (i - n * svec) * VEC;
    const T* xp = x + n * K * S + s;
    const Vec<L, VEC> tv = ldv<L, VEC>(t + n * S + s);
    float best[VEC];
    int besti[VEC];
    {
      const Vec<T, VEC> xv = ldv<T, VEC>(xp);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        best[j] = (float)xv.v[j];
        besti[j] = 0;
      }
    }
    for (int c = 1; c < K; ++c) {
      const Vec<T, VEC> xv = ldv<T, VEC>(xp + (int64_t)c * S);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float v = (float)xv.v[j];
        if (v > best[j]) { best[j] = v; besti[j] = c; }
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int64_t tr = (int64_t)tv.v[j];
      if (tr >= 0 && tr < K) atomicAdd(&s_mat[(int)tr * K + besti[j]], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kk; i += blockDim.x)
    if (s_mat[i])
      atomicAdd(reinterpret_cast<unsigned long long*>(&mat[i]),
                (unsigned long long)s_mat[i]);
}

// ---------------------------------------------------------------- host side
namespace {

inline bool aligned_to(const void* p, size_t a) {
  return (reinterpret_cast<uintptr_t>(p) % a) == 0;
}

template <typename T, typename L>
inline bool vec_ok(const void* x, const void* t) {
  constexpr int V = vec_width<T>();
  return aligned_to(x, 16) && aligned_to(t, alignof(Vec<L, V>));
}

// f(T{}) with T the logits' element type
template <class F>
inline void dispatch_logits(at::ScalarType st, F&& f) {
  switch (st) {
    case at::ScalarType::BFloat16: f(at::BFloat16{}); break;
    case at::ScalarType::Half: f(at::Half{}); break;
    case at::ScalarType::Float: f(float{}); break;
    default:
      TORCH_CHECK(false, "segloss: logits must be bf16, fp16 or fp32, got ",
                  st);
  }
}

// f(L{}) with L the labels' element type; bool is read as its uint8 storage
template <typename T, bool ALLOW_FLOAT, class F>
inline void dispatch_labels(at::ScalarType st, F&& f) {
  if (st == at::ScalarType::Byte || st == at::ScalarType::Bool) {
    f(uint8_t{});
    return;
  }
  if (st == at::ScalarType::Long) {
    f(int64_t{});
    return;
  }
  if constexpr (ALLOW_FLOAT) {  // soft labels (dice only)
    if (st == at::ScalarType::Float) {
      f(float{});
      return;
    }
    if constexpr (!std::is_same<T, float>::value) {
      if (st == c10::CppTypeToScalarType<T>::value) {
        f(T{});
        return;
      }
    }
  }
  TORCH_CHECK(false, "segloss: unsupported label dtype ", st,
              ALLOW_FLOAT ? " (uint8, bool, int64, fp32 or the logits' dtype)"
                          : " (uint8, bool or int64)");
}

struct DiceArgs {
  torch::Tensor x, t, w;
  int64_t n;
  bool has_w;
};

DiceArgs dice_args(const torch::Tensor& logits, const torch::Tensor& target,
                   const c10::optional<torch::Tensor>& weights) {
  CHECK_GPU(logits);
  CHECK_GPU(target);
  DiceArgs a;
  a.x = logits.contiguous();
  a.t = target.contiguous();
  a.n = a.x.numel();
  TORCH_CHECK(a.t.numel() == a.n, "dice: target must have logits' numel");
  a.has_w = weights.has_value() && weights->defined();
  if (a.has_w) {
    CHECK_GPU(*weights);
    a.w = weights->contiguous();
    TORCH_CHECK(a.w.scalar_type() == at::ScalarType::Float,
                "dice: weights must be fp32");
    TORCH_CHECK(a.w.numel() == a.n, "dice: weights must have logits' numel");
  }
  return a;
}

struct PlaneArgs {
  torch::Tensor x, t;
  int64_t N, S;
  int C;
};

PlaneArgs plane_args(const torch::Tensor& logits, const torch::Tensor& target,
                     const char* what) {
  CHECK_GPU(logits);
  CHECK_GPU(target);
  TORCH_CHECK(logits.dim() >= 2, what, ": logits must be [N, C, ...]");
  PlaneArgs a;
  a.x = logits.contiguous();
  a.t = target.contiguous();
  a.N = a.x.size(0);
  a.C = (int)a.x.size(1);
  TORCH_CHECK(a.C >= 1 && a.N >= 1, what, ": empty logits");
  a.S = a.x.numel() / (a.N * a.C);
  TORCH_CHECK(a.t.numel() == a.N * a.S, what,
              ": target must be [N, ...] with logits' spatial extent");
  return a;
}

}  // namespace

std::vector<torch::Tensor> seg_dice_fwd(torch::Tensor logits,
                                        torch::Tensor target,
                                        c10::optional<torch::Tensor> weights,
                                        double beta, double eps) {
  DiceArgs a = dice_args(logits, target, weights);
  auto fopt = a.x.options().dtype(torch::kFloat32);
  auto sums = torch::empty({3}, fopt);
  auto loss = torch::empty({}, fopt);
  const float* wp = a.has_w ? a.w.data_ptr<float>() : nullptr;
  const float b2 = (float)(beta * beta);
  dispatch_logits(a.x.scalar_type(), [&](auto tt) {
    using T = decltype(tt);
    constexpr int V = vec_width<T>();
    dispatch_labels<T, true>(a.t.scalar_type(), [&](auto ll) {
      using L = decltype(ll);
      const T* xp = static_cast<const T*>(a.x.data_ptr());
      const L* tp = static_cast<const L*>(a.t.data_ptr());
      const bool vec = vec_ok<T, L>(xp, tp) && (!a.has_w || aligned_to(wp, 16));
      const int grid = elem_grid(vec ? (a.n + V - 1) / V : a.n, 1);
      auto partial = torch::empty({grid, 3}, fopt);
      float* pp = partial.data_ptr<float>();
      dispatch_bool(a.has_w, [&](auto hw) {
        constexpr bool HW = decltype(hw)::value;
        if (vec)
          hipLaunchKernelGGL((seg_dice_fwd_kernel<T, L, HW, V>), dim3(grid),
                             dim3(ELEM_BLOCK), 0, current_stream(), xp, tp,
                             wp, pp, a.n);
        else
          hipLaunchKernelGGL((seg_dice_fwd_kernel<T, L, HW, 1>), dim3(grid),
                             dim3(ELEM_BLOCK), 0, current_stream(), xp, tp,
                             wp, pp, a.n);
      });
      hipLaunchKernelGGL(seg_dice_finish_kernel, dim3(1), dim3(ELEM_BLOCK), 0,
                         current_stream(), pp, grid, b2, (float)eps,
                         sums.data_ptr<float>(), loss.data_ptr<float>());
    });
  });
  return {loss, sums};
}

torch::Tensor seg_dice_bwd(torch::Tensor logits, torch::Tensor target,
                           c10::optional<torch::Tensor> weights,
                           torch::Tensor sums, torch::Tensor grad_out,
                           double beta, double eps) {
  DiceArgs a = dice_args(logits, target, weights);
  CHECK_GPU(sums);
  CHECK_GPU(grad_out);
  TORCH_CHECK(sums.scalar_type() == at::ScalarType::Float &&
              sums.numel() == 3 && sums.is_contiguous(),
              "dice: sums must be fp32[3]");
  auto go = grad_out.to(torch::kFloat32).contiguous();
  TORCH_CHECK(go.numel() == 1, "dice: grad_out must be a scalar");
  auto gx = torch::empty_like(a.x);
  const float* wp = a.has_w ? a.w.data_ptr<float>() : nullptr;
  const float b2 = (float)(beta * beta);
  dispatch_logits(a.x.scalar_type(), [&](auto tt) {
    using T = decltype(tt);
    constexpr int V = vec_width<T>();
    dispatch_labels<T, true>(a.t.scalar_type(), [&](auto ll) {
      using L = decltype(ll);
      const T* xp = static_cast<const T*>(a.x.data_ptr());
      const L* tp = static_cast<const L*>(a.t.data_ptr());
      T* gp = static_cast<T*>(gx.data_ptr());
      const bool vec = vec_ok<T, L>(xp, tp) && aligned_to(gp, 16) &&
                       (!a.has_w || aligned_to(wp, 16));
      const int grid = elem_grid(vec ? (a.n + V - 1) / V : a.n, 1);
      dispatch_bool(a.has_w, [&](auto hw) {
        constexpr bool HW = decltype(hw)::value;
        if (vec)
          hipLaunchKernelGGL((seg_dice_bwd_kernel<T, L, HW, V>), dim3(grid),
                             dim3(ELEM_BLOCK), 0, current_stream(), xp, tp,
                             wp, sums.data_ptr<float>(), go.data_ptr<float>(),
                             gp, b2, (float)eps, a.n);
        else
          hipLaunchKernelGGL((seg_dice_bwd_kernel<T, L, HW, 1>), dim3(grid),
                             dim3(ELEM_BLOCK), 0, current_stream(), xp, tp,
                             wp, sums.data_ptr<float>(), go.data_ptr<float>(),
                             gp, b2, (float)eps, a.n);
      });
    });
  });
  return gx;
}

std::vector<torch::Tensor> seg_ce_fwd(torch::Tensor logits,
                                      torch::Tensor target) {
  PlaneArgs a = plane_args(logits, target, "seg_ce");
  auto fopt = a.x.options().dtype(torch::kFloat32);
  auto lse = torch::empty({a.N, a.S}, fopt);
  auto loss = torch::empty({}, fopt);
  const float inv_count = (float)(1.0 / ((double)a.N * (double)a.S));
  dispatch_logits(a.x.scalar_type(), [&](auto tt) {
    using T = decltype(tt);
    constexpr int V = vec_width<T>();
    dispatch_labels<T, false>(a.t.scalar_type(), [&](auto ll) {
      using L = decltype(ll);
      const T* xp = static_cast<const T*>(a.x.data_ptr());
      const L* tp = static_cast<const L*>(a.t.data_ptr());
      const bool vec = vec_ok<T, L>(xp, tp) && a.S % V == 0;
      const int grid = elem_grid(vec ? a.N * a.S / V : a.N * a.S, 1);
      auto partial = torch::empty({grid}, fopt);
      if (vec)
        hipLaunchKernelGGL((seg_ce_fwd_kernel<T, L, V>), dim3(grid),
                           dim3(ELEM_BLOCK), 0, current_stream(), xp, tp,
                           lse.data_ptr<float>(), partial.data_ptr<float>(),
                           a.N, a.C, a.S);
      else
        hipLaunchKernelGGL((seg_ce_fwd_kernel<T, L, 1>), dim3(grid),
                           dim3(ELEM_BLOCK), 0, current_stream(), xp, tp,
                           lse.data_ptr<float>(), partial.data_ptr<float>(),
                           a.N, a.C, a.S);
      hipLaunchKernelGGL(seg_ce_finish_kernel, dim3(1), dim3(ELEM_BLOCK), 0,
                         current_stream(), partial.data_ptr<float>(), grid,
                         inv_count, loss.data_ptr<float>());
    });
  });
  return {loss, lse};
}

torch::Tensor seg_ce_bwd(torch::Tensor logits, torch::Tensor target,
                         torch::Tensor lse, torch::Tensor grad_out) {
  PlaneArgs a = plane_args(logits, target, "seg_ce");
  CHECK_GPU(lse);
  CHECK_GPU(grad_out);
  TORCH_CHECK(lse.scalar_type() == at::ScalarType::Float &&
              lse.numel() == a.N * a.S && lse.is_contiguous(),
              "seg_ce: lse must be contiguous fp32 [N, S]");
  auto go = grad_out.to(torch::kFloat32).contiguous();
  TORCH_CHECK(go.numel() == 1, "seg_ce: grad_out must be a scalar");
  auto gx = torch::empty_like(a.x);
  const float inv_count = (float)(1.0 / ((double)a.N * (double)a.S));
  dispatch_logits(a.x.scalar_type(), [&](auto tt) {
    using T = decltype(tt);
    constexpr int V = vec_width<T>();
    dispatch_labels<T, false>(a.t.scalar_type(), [&](auto ll) {
      using L = decltype(ll);
      const T* xp = static_cast<const T*>(a.x.data_ptr());
      const L* tp = static_cast<const L*>(a.t.data_ptr());
      T* gp = static_cast<T*>(gx.data_ptr());
      const bool vec = vec_ok<T, L>(xp, tp) && aligned_to(gp, 16) &&
                       aligned_to(lse.data_ptr(), 16) && a.S % V == 0;
      const int grid = elem_grid(vec ? a.N * a.S / V : a.N * a.S, 1);
      if (vec)
        hipLaunchKernelGGL((seg_ce_bwd_kernel<T, L, V>), dim3(grid),
                           dim3(ELEM_BLOCK), 0, current_stream(), xp, tp,
                           lse.data_ptr<float>(), go.data_ptr<float>(), gp,
                           inv_count, a.N, a.C, a.S);
      else
        hipLaunchKernelGGL((seg_ce_bwd_kernel<T, L, 1>), dim3(grid),
                           dim3(ELEM_BLOCK), 0, current_stream(), xp, tp,
                           lse.data_ptr<float>(), go.data_ptr<float>(), gp,
                           inv_count, a.N, a.C, a.S);
    });
  });
  return gx;
}

torch::Tensor seg_prf1a_counts(torch::Tensor logits, torch::Tensor target) {
  CHECK_GPU(logits);
  CHECK_GPU(target);
  auto x = logits.contiguous();
  auto t = target.contiguous();
  const int64_t n = x.numel();
  TORCH_CHECK(t.numel() == n, "seg_prf1a: target must have logits' numel");
  auto counts = torch::zeros({4}, x.options().dtype(torch::kInt64));
  dispatch_logits(x.scalar_type(), [&](auto tt) {
    using T = decltype(tt);
    constexpr int V = vec_width<T>();
    dispatch_labels<T, false>(t.scalar_type(), [&](auto ll) {
      using L = decltype(ll);
      const T* xp = static_cast<const T*>(x.data_ptr());
      const L* tp = static_cast<const L*>(t.data_ptr());
      const bool vec = vec_ok<T, L>(xp, tp);
      const int grid = elem_grid(vec ? (n + V - 1) / V : n, 8);
      if (vec)
        hipLaunchKernelGGL((seg_prf1a_kernel<T, L, V>), dim3(grid),
                           dim3(ELEM_BLOCK), 0, current_stream(), xp, tp,
                           counts.data_ptr<int64_t>(), n);
      else
        hipLaunchKernelGGL((seg_prf1a_kernel<T, L, 1>), dim3(grid),
                           dim3(ELEM_BLOCK), 0, current_stream(), xp, tp,
                           counts.data_ptr<int64_t>(), n);
    });
  });
  return counts;  // [tp, fp, tn, fn]
}

torch::Tensor seg_confusion_matrix(torch::Tensor logits, torch::Tensor target,
                                   int64_t num_classes) {
  PlaneArgs a = plane_args(logits, target, "seg_confusion");
  TORCH_CHECK(num_classes == a.C, "seg_confusion: num_classes (", num_classes,
              ") must equal the logits' class dimension (", a.C, ")");
  const int K = a.C;
  auto mat = torch::zeros({num_classes, num_classes},
                          a.x.options().dtype(torch::kInt64));
  const size_t smem = (size_t)K * K * sizeof(int);
  TORCH_CHECK(smem <= 160 * 1024, "num_classes too large for LDS histogram");
  dispatch_logits(a.x.scalar_type(), [&](auto tt) {
    using T = decltype(tt);
    constexpr int V = vec_width<T>();
    dispatch_labels<T, false>(a.t.scalar_type(), [&](auto ll) {
      using L = decltype(ll);
      const T* xp = static_cast<const T*>(a.x.data_ptr());
      const L* tp = static_cast<const L*>(a.t.data_ptr());
      const bool vec = vec_ok<T, L>(xp, tp) && a.S % V == 0;
      const int grid = elem_grid(vec ? a.N * a.S / V : a.N * a.S, 8);
      if (vec)
        hipLaunchKernelGGL((seg_confusion_kernel<T, L, V>), dim3(grid),
                           dim3(ELEM_BLOCK), smem, current_stream(), xp, tp,
                           mat.data_ptr<int64_t>(), a.N, K, a.S);
      else
        hipLaunchKernelGGL((seg_confusion_kernel<T, L, 1>), dim3(grid),
                           dim3(ELEM_BLOCK), smem, current_stream(), xp, tp,
                           mat.data_ptr<int64_t>(), a.N, K, a.S);
    });
  });
  return mat;
}
