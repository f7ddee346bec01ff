// Helpers shared by the segmentation-head kernel files (segloss.hip,
// segdice.hip): 16-byte vectors over the logits' element type, the
// reproducible block reduction and the host-side dtype dispatch.
#pragma once
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

// ---------------------------------------------------------------- host side
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

}  // namespace
