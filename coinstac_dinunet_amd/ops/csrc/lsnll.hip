// K3/K16 — fused log_softmax + NLL loss (mean) fwd/bwd + row argmax.
// The reference runs F.log_softmax + F.nll_loss as separate kernels
// (README.md:76-77); here one kernel computes logprobs + the loss partial
// sums, one computes the gradient. Row counts are small (classifier
// heads, C <= 64): one WAVE per row, lanes cover classes, cross-lane
// reduction via __shfl_down (64-wide wave — no CUDA warp idioms).
#include "common.h"

template <typename T>
__device__ inline float to_f32(T x) { return (float)x; }

// one wave per row; C <= blockDim lanes handled by strided lane loop
template <typename T>
__global__ void lsnll_fwd_kernel(const T* __restrict__ logits,
                                 const int64_t* __restrict__ target,
                                 float* __restrict__ logprobs,
                                 double* __restrict__ loss_partial, int64_t B,
                                 int C) {
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int waves_per_block = blockDim.x / WAVE_SIZE;
  // the sum over rows is kept in double: thousands of wave partials folded
  // into one fp32 by atomics lost 2e-6 of the mean loss at B = 8195
  double local_loss = 0.0;
  for (int64_t row = (int64_t)blockIdx.x * waves_per_block + wave; row < B;
       row += (int64_t)gridDim.x * waves_per_block) {
    const T* xrow = logits + row * C;
    float maxv = -INFINITY;
    for (int c = lane; c < C; c += WAVE_SIZE)
      maxv = fmaxf(maxv, to_f32(xrow[c]));
    for (int off = WAVE_SIZE / 2; off > 0; off >>= 1)
      maxv = fmaxf(maxv, __shfl_down(maxv, off));
    maxv = __shfl(maxv, 0);
    float sum = 0.0f;
    for (int c = lane; c < C; c += WAVE_SIZE)
      sum += __expf(to_f32(xrow[c]) - maxv);
    for (int off = WAVE_SIZE / 2; off > 0; off >>= 1)
      sum += __shfl_down(sum, off);
    sum = __shfl(sum, 0);
    // (x - max) - log(sum), not x - (max + log(sum)): the latter rounds
    // log(sum) to an ulp of max, 1e-3 for logits near 1e4
    const float logsum = __logf(sum);
    for (int c = lane; c < C; c += WAVE_SIZE)
      logprobs[row * C + c] = (to_f32(xrow[c]) - maxv) - logsum;
    if (lane == 0)
      local_loss += logsum - (to_f32(xrow[target[row]]) - maxv);
  }
  if (lane == 0) atomicAdd(loss_partial, local_loss);
}

template <typename T>
__global__ void lsnll_bwd_kernel(const float* __restrict__ logprobs,
                                 const int64_t* __restrict__ target,
                                 const float* __restrict__ grad_out,
                                 T* __restrict__ grad_logits, int64_t B,
                                 int C) {
  const float scale = grad_out[0] / (float)B;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < B * C;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t row = i / C;
    int c = (int)(i - row * C);
    float p = __expf(logprobs[i]);
    float g = (p - (target[row] == c ? 1.0f : 0.0f)) * scale;
    grad_logits[i] = (T)g;
  }
}

template <typename T>
__global__ void argmax_rows_kernel(const T* __restrict__ x,
                                   int64_t* __restrict__ out, int64_t B,
                                   int C) {
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int waves_per_block = blockDim.x / WAVE_SIZE;
  for (int64_t row = (int64_t)blockIdx.x * waves_per_block + wave; row < B;
       row += (int64_t)gridDim.x * waves_per_block) {
    const T* xrow = x + row * C;
    float best = -INFINITY;
    int besti = 0;
    for (int c = lane; c < C; c += WAVE_SIZE) {
      float v = to_f32(xrow[c]);
      if (v > best) { best = v; besti = c; }
    }
    for (int off = WAVE_SIZE / 2; off > 0; off >>= 1) {
      float ov = __shfl_down(best, off);
      int oi = __shfl_down(besti, off);
      if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
    }
    if (lane == 0) out[row] = besti;
  }
}

std::vector<torch::Tensor> logsoftmax_nll_fwd(torch::Tensor logits,
                                              torch::Tensor target) {
  CHECK_GPU(logits);
  CHECK_GPU(target);
  TORCH_CHECK(logits.dim() == 2, "logsoftmax_nll_fwd: logits must be [B, C]");
  auto l = logits.contiguous();
  auto t = target.contiguous();
  int64_t B = l.size(0);
  int C = (int)l.size(1);
  TORCH_CHECK(t.scalar_type() == torch::kInt64 && t.numel() == B,
              "logsoftmax_nll_fwd: target must be B int64 class indices");
  auto logprobs = torch::empty({B, (int64_t)C},
                               l.options().dtype(torch::kFloat32));
  if (B == 0)  // mean over no rows, as torch: NaN; nothing to launch
    return {torch::full({}, NAN, l.options().dtype(torch::kFloat32)),
            logprobs};
  auto loss = torch::zeros({}, l.options().dtype(torch::kFloat64));
  TORCH_CHECK(C > 0, "logsoftmax_nll_fwd: no classes");
  int waves_per_block = ELEM_BLOCK / WAVE_SIZE;
  int grid = (int)std::min<int64_t>((B + waves_per_block - 1) / waves_per_block,
                                    2048);
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, l.scalar_type(),
      "lsnll_fwd", [&] {
        hipLaunchKernelGGL(lsnll_fwd_kernel<scalar_t>, dim3(grid),
                           dim3(ELEM_BLOCK), 0, current_stream(),
                           l.data_ptr<scalar_t>(), t.data_ptr<int64_t>(),
                           logprobs.data_ptr<float>(), loss.data_ptr<double>(),
                           B, C);
      });
  return {loss.div_((double)B).to(torch::kFloat32), logprobs};
}

torch::Tensor logsoftmax_nll_bwd(torch::Tensor logprobs, torch::Tensor target,
                                 torch::Tensor grad_out,
                                 torch::ScalarType out_dtype) {
  CHECK_GPU(logprobs); CHECK_CONTIG(logprobs);
  CHECK_GPU(target);
  TORCH_CHECK(logprobs.dim() == 2,
              "logsoftmax_nll_bwd: logprobs must be [B, C]");
  auto t = target.contiguous();
  int64_t B = logprobs.size(0);
  int C = (int)logprobs.size(1);
  TORCH_CHECK(t.scalar_type() == torch::kInt64 && t.numel() == B,
              "logsoftmax_nll_bwd: target must be B int64 class indices");
  auto g = grad_out.to(torch::kFloat32).contiguous();
  TORCH_CHECK(g.numel() == 1, "logsoftmax_nll_bwd: grad_out must be a scalar");
  auto grad_logits = torch::empty({B, (int64_t)C},
                                  logprobs.options().dtype(out_dtype));
  if (B * C == 0) return grad_logits;
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, out_dtype, "lsnll_bwd",
      [&] {
        hipLaunchKernelGGL(lsnll_bwd_kernel<scalar_t>,
                           dim3(elem_grid(B * C)), dim3(ELEM_BLOCK), 0,
                           current_stream(), logprobs.data_ptr<float>(),
                           t.data_ptr<int64_t>(), g.data_ptr<float>(),
                           grad_logits.data_ptr<scalar_t>(), B, C);
      });
  return grad_logits;
}

torch::Tensor argmax_rows(torch::Tensor x) {
  CHECK_GPU(x);
  TORCH_CHECK(x.dim() == 2, "argmax_rows: x must be [B, C]");
  auto l = x.contiguous();
  int64_t B = l.size(0);
  int C = (int)l.size(1);
  auto out = torch::empty({B}, l.options().dtype(torch::kInt64));
  if (B == 0) return out;
  int waves_per_block = ELEM_BLOCK / WAVE_SIZE;
  int grid = (int)std::min<int64_t>((B + waves_per_block - 1) / waves_per_block,
                                    2048);
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, l.scalar_type(),
      "argmax_rows", [&] {
        hipLaunchKernelGGL(argmax_rows_kernel<scalar_t>, dim3(grid),
                           dim3(ELEM_BLOCK), 0, current_stream(),
                           l.data_ptr<scalar_t>(), out.data_ptr<int64_t>(), B,
                           C);
      });
  return out;
}
