// GroupNorm / InstanceNorm with a fused (leaky) ReLU, training fwd/bwd, for
// contiguous bf16 [N, C, S...]: bf16 in and out, fp32 math, 16-byte loads
// and stores on the streaming body.
//
// With G groups of cpg = C/G channels, one group of one sample is ONE
// contiguous run ("row") of L = cpg*S elements; there are N*G rows.
// InstanceNorm is G == C, the LayerNorm-like case G == 1.
//
// Forward, two launches:
//   gn_stats_kernel      grid (splits, N*G). N*G is often 8..32 rows on 256
//                        CUs, so a row is cut into `splits` chunks; a block
//                        reduces its chunk to (count, mean, M2) and stores
//                        it: no atomics, no memset, deterministic. Moments
//                        are merged with Chan's formula at every level
//                        (8-wide vector -> thread -> wave -> block), never
//                        as sum / sum of squares: |mean| >> std would cancel
//                        the variance in fp32.
//   gn_normalize_kernel  grid (chunks, N*C). The prologue merges the
//                        <= 64 partials of the block's row (wave-uniform
//                        loads, same order in every block), so there is no
//                        finalize launch; gamma[c], beta[c] are
//                        block-uniform: y = act(x*a + b), a = gamma*rstd,
//                        b = beta - mean*a. Also stores mean_rstd[N*G][2].
// Backward, three launches, z recomputed from the saved x (no y, no mask):
//   gn_bwd_reduce_kernel grid (splits, N*C): partials of sum(dz) and
//                        sum(dz*xhat) per (plane, split), dz = dy*act'(z).
//   gn_bwd_dx_kernel     same grid. Prologue folds the partials of the cpg
//                        channels of its group, weighted by gamma, into
//                        B = sum(gamma*dz), A = sum(gamma*dz*xhat); then
//                        dx = rstd*(gamma*dz - (B + xhat*A)/L).
//   gn_bwd_affine_kernel one block per channel: dgamma, dbeta = the
//                        partials summed over n and the splits.
//
// A plane starts 16-byte aligned only when S % 8 == 0, so every kernel cuts
// its run into a scalar head (up to the first aligned element), aligned
// 8-wide vectors and a scalar tail (Span); nothing outside the run is read
// or written.
#include "common.h"

#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <hip/hip_bf16.h>

#include <algorithm>

typedef __attribute__((ext_vector_type(8))) __bf16 gn_bf16x8;

#define GN_BLOCK 256
#define GN_WAVES (GN_BLOCK / WAVE_SIZE)

// ---- run geometry ---------------------------------------------------------
// `len` elements that start `off` elements into a 16-byte aligned tensor.
struct Span {
  int64_t head;  // scalar elements before the first aligned one
  int64_t nvec;  // aligned 8-wide vectors
  int nscalar;   // head + tail, < 16
  __device__ Span(int64_t off, int64_t len) {
    head = (8 - (off & 7)) & 7;
    if (head > len) head = len;
    nvec = (len - head) >> 3;
    nscalar = (int)(len - nvec * 8);
  }
  // position in the run of scalar element i in [0, nscalar)
  __device__ int64_t scalar_at(int i) const {
    return i < head ? i : i + nvec * 8;
  }
};

// ---- moments --------------------------------------------------------------
// Counts are floats: only their ratios weigh the merge, so the 2^-24
// rounding of a count above 2^24 is harmless; the variance divides by the
// exact L from the host.
struct Moments {
  float n, mean, m2;
};

static __device__ inline Moments chan(Moments a, Moments b) {
  const float n = a.n + b.n;
  const float w = b.n / fmaxf(n, 1.f);  // both empty: stays all zero
  const float d = b.mean - a.mean;
  return {n, a.mean + d * w, a.m2 + b.m2 + d * d * a.n * w};
}

// merged (mean, rstd) of a row from its `splits` partials, in split order
static __device__ inline void gn_row_stats(const float* __restrict__ part,
                                           int splits, float inv_L, float eps,
                                           float& mean, float& rstd) {
  Moments a = {part[0], part[1], part[2]};
  for (int s = 1; s < splits; ++s)
    a = chan(a, {part[3 * s], part[3 * s + 1], part[3 * s + 2]});
  mean = a.mean;
  rstd = rsqrtf(a.m2 * inv_L + eps);
}

// block-wide sums of two values, returned to every thread (fixed order)
static __device__ inline void block_sum2(float& s0, float& s1) {
  for (int off = WAVE_SIZE / 2; off > 0; off >>= 1) {
    s0 += __shfl_down(s0, off);
    s1 += __shfl_down(s1, off);
  }
  __shared__ float lds[GN_WAVES][2];
  if ((threadIdx.x & (WAVE_SIZE - 1)) == 0) {
    lds[threadIdx.x / WAVE_SIZE][0] = s0;
    lds[threadIdx.x / WAVE_SIZE][1] = s1;
  }
  __syncthreads();
  s0 = 0.f;
  s1 = 0.f;
#pragma unroll
  for (int w = 0; w < GN_WAVES; ++w) {
    s0 += lds[w][0];
    s1 += lds[w][1];
  }
}

template <bool ACT>
static __device__ inline float gn_act(float z, float slope) {
  return (ACT && z <= 0.f) ? slope * z : z;
}

// ---- fwd 1: (count, mean, M2) of one chunk of one row ---------------------
__global__ __launch_bounds__(GN_BLOCK) void gn_stats_kernel(
    const __bf16* __restrict__ x,
    float* __restrict__ part,  // [rows][splits][3]
    int64_t L, int64_t chunk) {
  const int64_t begin = (int64_t)blockIdx.x * chunk;  // < L (host)
  const int64_t len = chunk < L - begin ? chunk : L - begin;
  const int64_t off = (int64_t)blockIdx.y * L + begin;
  const __bf16* p = x + off;
  const Span sp(off, len);

  Moments acc = {0.f, 0.f, 0.f};
  const gn_bf16x8* pv = reinterpret_cast<const gn_bf16x8*>(p + sp.head);
  float k = 0.f;  // vectors merged so far: acc.n == 8k
  auto merge = [&](const gn_bf16x8 t) {
    float f[8], m = 0.f, q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = (float)t[j];
      m += f[j];
    }
    m *= 0.125f;
#pragma unroll
    for (int j = 0; j < 8; ++j) q = fmaf(f[j] - m, f[j] - m, q);
    // Chan with n_a = 8k, n_b = 8: n_b/n = 1/(k+1), n_a*n_b/n = 8k/(k+1)
    k += 1.f;
    const float r = __frcp_rn(k);
    const float d = m - acc.mean;
    acc.mean = fmaf(d, r, acc.mean);
    acc.m2 += q + d * d * 8.f * (1.f - r);
  };
  // four independent 16-byte loads in flight per thread, then the tail
  int64_t v = threadIdx.x;
  for (; v + 3 * GN_BLOCK < sp.nvec; v += 4 * GN_BLOCK) {
    const gn_bf16x8 t0 = pv[v], t1 = pv[v + GN_BLOCK],
                    t2 = pv[v + 2 * GN_BLOCK], t3 = pv[v + 3 * GN_BLOCK];
    merge(t0);
    merge(t1);
    merge(t2);
    merge(t3);
  }
  for (; v < sp.nvec; v += GN_BLOCK) merge(pv[v]);
  acc.n = 8.f * k;
  if ((int)threadIdx.x < sp.nscalar)
    acc = chan(acc, {1.f, (float)p[sp.scalar_at(threadIdx.x)], 0.f});

  for (int o = WAVE_SIZE / 2; o > 0; o >>= 1) {
    Moments b = {__shfl_down(acc.n, o), __shfl_down(acc.mean, o),
                 __shfl_down(acc.m2, o)};
    acc = chan(acc, b);
  }
  __shared__ float lds[GN_WAVES][3];
  if ((threadIdx.x & (WAVE_SIZE - 1)) == 0) {
    float* w = lds[threadIdx.x / WAVE_SIZE];
    w[0] = acc.n;
    w[1] = acc.mean;
    w[2] = acc.m2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < GN_WAVES; ++w)
      acc = chan(acc, {lds[w][0], lds[w][1], lds[w][2]});
    float* o = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
    o[0] = acc.n;
    o[1] = acc.mean;
    o[2] = acc.m2;
  }
}

// ---- fwd 2: y = act(x*a + b) over one plane -------------------------------
template <bool ACT>
__global__ __launch_bounds__(GN_BLOCK) void gn_normalize_kernel(
    const __bf16* __restrict__ x, __bf16* __restrict__ y,
    const float* __restrict__ part,  // [rows][splits][3]
    float* __restrict__ mean_rstd,   // [rows][2], written here
    const float* __restrict__ gamma, const float* __restrict__ beta, int C,
    int cpg, int splits, int64_t S, float inv_L, float eps, float slope) {
  const int nc = blockIdx.y;
  const int c = nc % C;
  const int row = (nc / C) * (C / cpg) + c / cpg;
  float mean, rstd;
  gn_row_stats(part + (int64_t)row * splits * 3, splits, inv_L, eps, mean,
               rstd);
  if (blockIdx.x == 0 && c % cpg == 0 && threadIdx.x == 0) {
    mean_rstd[2 * row] = mean;
    mean_rstd[2 * row + 1] = rstd;
  }
  const float a = gamma[c] * rstd, b = beta[c] - mean * a;

  const int64_t off = (int64_t)nc * S;
  const __bf16* xp = x + off;
  __bf16* yp = y + off;
  const Span sp(off, S);
  const gn_bf16x8* xv = reinterpret_cast<const gn_bf16x8*>(xp + sp.head);
  gn_bf16x8* yv = reinterpret_cast<gn_bf16x8*>(yp + sp.head);
  const int64_t stride = (int64_t)gridDim.x * GN_BLOCK;
#pragma unroll 2
  for (int64_t v = (int64_t)blockIdx.x * GN_BLOCK + threadIdx.x; v < sp.nvec;
       v += stride) {
    const gn_bf16x8 t = xv[v];
    gn_bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = (__bf16)gn_act<ACT>(fmaf((float)t[j], a, b), slope);
    yv[v] = o;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < sp.nscalar) {
    const int64_t i = sp.scalar_at(threadIdx.x);
    yp[i] = (__bf16)gn_act<ACT>(fmaf((float)xp[i], a, b), slope);
  }
}

// ---- bwd 1: sum(dz), sum(dz*xhat) of one chunk of one plane ---------------
template <bool ACT>
__global__ __launch_bounds__(GN_BLOCK) void gn_bwd_reduce_kernel(
    const __bf16* __restrict__ dy, const __bf16* __restrict__ x,
    const float* __restrict__ mean_rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta,
    float* __restrict__ part,  // [N*C][splits][2]
    int C, int cpg, int64_t S, int64_t chunk, float slope) {
  const int nc = blockIdx.y;
  const int c = nc % C;
  const int row = (nc / C) * (C / cpg) + c / cpg;
  const float mean = mean_rstd[2 * row], rstd = mean_rstd[2 * row + 1];
  const float a = gamma[c] * rstd, b = beta[c] - mean * a;

  const int64_t begin = (int64_t)blockIdx.x * chunk;  // < S (host)
  const int64_t len = chunk < S - begin ? chunk : S - begin;
  const int64_t off = (int64_t)nc * S + begin;
  const __bf16* dp = dy + off;
  const __bf16* xp = x + off;
  const Span sp(off, len);
  const gn_bf16x8* dv = reinterpret_cast<const gn_bf16x8*>(dp + sp.head);
  const gn_bf16x8* xv = reinterpret_cast<const gn_bf16x8*>(xp + sp.head);
  float s0 = 0.f, s1 = 0.f;
  auto add = [&](float d, float xf) {
    if (ACT && fmaf(xf, a, b) <= 0.f) d *= slope;
    s0 += d;
    s1 = fmaf(d, (xf - mean) * rstd, s1);
  };
#pragma unroll 2
  for (int64_t v = threadIdx.x; v < sp.nvec; v += GN_BLOCK) {
    const gn_bf16x8 dt = dv[v], xt = xv[v];
#pragma unroll
    for (int j = 0; j < 8; ++j) add((float)dt[j], (float)xt[j]);
  }
  if ((int)threadIdx.x < sp.nscalar) {
    const int64_t i = sp.scalar_at(threadIdx.x);
    add((float)dp[i], (float)xp[i]);
  }
  block_sum2(s0, s1);
  if (threadIdx.x == 0) {
    float* o = part + ((int64_t)nc * gridDim.x + blockIdx.x) * 2;
    o[0] = s0;
    o[1] = s1;
  }
}

// ---- bwd 2: dx = rstd*(gamma*dz - (B + xhat*A)/L) -------------------------
template <bool ACT>
__global__ __launch_bounds__(GN_BLOCK) void gn_bwd_dx_kernel(
    const __bf16* __restrict__ dy, const __bf16* __restrict__ x,
    __bf16* __restrict__ dx, const float* __restrict__ mean_rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ part,  // [N*C][splits][2]
    int C, int cpg, int64_t S, int64_t chunk, float inv_L, float slope) {
  const int nc = blockIdx.y;
  const int c = nc % C;
  const int c0 = c - c % cpg;  // first channel of the group
  const int row = (nc / C) * (C / cpg) + c / cpg;
  const int splits = gridDim.x;

  // the group's cpg*splits partials are contiguous: planes nc0 .. nc0+cpg-1
  const float* gp = part + (int64_t)(nc - c + c0) * splits * 2;
  float B = 0.f, A = 0.f;
  for (int e = threadIdx.x; e < cpg * splits; e += GN_BLOCK) {
    const float g = gamma[c0 + e / splits];
    B = fmaf(g, gp[2 * e], B);
    A = fmaf(g, gp[2 * e + 1], A);
  }
  block_sum2(B, A);
  B *= inv_L;
  A *= inv_L;

  const float mean = mean_rstd[2 * row], rstd = mean_rstd[2 * row + 1];
  const float g = gamma[c];
  const float a = g * rstd, b = beta[c] - mean * a;
  const int64_t begin = (int64_t)blockIdx.x * chunk;  // < S (host)
  const int64_t len = chunk < S - begin ? chunk : S - begin;
  const int64_t off = (int64_t)nc * S + begin;
  const __bf16* dp = dy + off;
  const __bf16* xp = x + off;
  __bf16* op = dx + off;
  const Span sp(off, len);
  const gn_bf16x8* dv = reinterpret_cast<const gn_bf16x8*>(dp + sp.head);
  const gn_bf16x8* xv = reinterpret_cast<const gn_bf16x8*>(xp + sp.head);
  gn_bf16x8* ov = reinterpret_cast<gn_bf16x8*>(op + sp.head);
  auto grad = [&](float d, float xf) {
    if (ACT && fmaf(xf, a, b) <= 0.f) d *= slope;
    const float xh = (xf - mean) * rstd;
    return rstd * (g * d - fmaf(xh, A, B));
  };
#pragma unroll 2
  for (int64_t v = threadIdx.x; v < sp.nvec; v += GN_BLOCK) {
    const gn_bf16x8 dt = dv[v], xt = xv[v];
    gn_bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (__bf16)grad((float)dt[j], (float)xt[j]);
    ov[v] = o;
  }
  if ((int)threadIdx.x < sp.nscalar) {
    const int64_t i = sp.scalar_at(threadIdx.x);
    op[i] = (__bf16)grad((float)dp[i], (float)xp[i]);
  }
}

// ---- bwd 3: dgamma[c], dbeta[c] over n and the splits ---------------------
__global__ __launch_bounds__(GN_BLOCK) void gn_bwd_affine_kernel(
    const float* __restrict__ part,  // [N][C][splits][2]
    float* __restrict__ dgamma, float* __restrict__ dbeta, int N, int C,
    int splits) {
  const int c = blockIdx.x;
  float s0 = 0.f, s1 = 0.f;
  for (int e = threadIdx.x; e < N * splits; e += GN_BLOCK) {
    const float* p =
        part + (((int64_t)(e / splits) * C + c) * splits + e % splits) * 2;
    s0 += p[0];
    s1 += p[1];
  }
  block_sum2(s0, s1);
  if (threadIdx.x == 0) {
    dbeta[c] = s0;
    dgamma[c] = s1;
  }
}

// ---- host -----------------------------------------------------------------
// A run of `len` elements, `rows` of them reduced at once, is cut into
// chunks (a multiple of 8 elements, so every chunk of a row has the row's
// alignment) such that rows * splits covers 256 CUs about four times, a
// chunk keeps >= 4 vectors per thread and a consumer merges <= 64 partials.
static const int64_t GN_MAX_SPLITS = 64;
static const int64_t GN_MIN_CHUNK = GN_BLOCK * 8 * 4;

static int64_t gn_split(int64_t len, int64_t rows, int64_t* chunk) {
  const int64_t want = (1024 + rows - 1) / rows;
  const int64_t most =
      std::min(GN_MAX_SPLITS, (len + GN_MIN_CHUNK - 1) / GN_MIN_CHUNK);
  const int64_t splits = std::max<int64_t>(1, std::min(want, most));
  *chunk = ((len + splits - 1) / splits + 7) & ~(int64_t)7;
  return (len + *chunk - 1) / *chunk;  // no empty chunk
}

// splits the statistics (len = L, rows = N*G) or the backward reduction
// (len = S, rows = N*C) takes: what the tests and docs refer to
int64_t gn_splits(int64_t len, int64_t rows) {
  TORCH_CHECK(len > 0 && rows > 0, "gn_splits: empty run");
  int64_t chunk;
  return gn_split(len, rows, &chunk);
}

struct GnShape {
  int N, C, cpg;
  int64_t S, L;
};

static GnShape gn_shape(const torch::Tensor& x, int64_t G, const char* who) {
  TORCH_CHECK(x.is_cuda(), who, ": x must be a GPU tensor");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, who, " wants bf16");
  TORCH_CHECK(x.dim() >= 3, who, ": x must be [N, C, S...]");
  TORCH_CHECK(x.is_contiguous(), who, ": x must be contiguous");
  TORCH_CHECK(x.numel() > 0, who, ": empty input");
  const int64_t N = x.size(0), C = x.size(1);
  TORCH_CHECK(G > 0 && C % G == 0, who, ": ", C,
              " channels do not divide into ", G, " groups");
  TORCH_CHECK(N * C <= 65535, who, ": N*C = ", N * C,
              " exceeds the grid's 65535 planes");
  GnShape s;
  s.N = (int)N;
  s.C = (int)C;
  s.cpg = (int)(C / G);
  s.S = x.numel() / (N * C);
  s.L = s.cpg * s.S;
  return s;
}

// the vector body assumes element 0 of the tensor is 16-byte aligned
static torch::Tensor gn_aligned(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 ? t : t.clone();
}

static torch::Tensor gn_affine(const torch::Tensor& p, const torch::Tensor& x,
                               int C, const char* what) {
  TORCH_CHECK(p.device() == x.device() && p.numel() == C, what,
              " must hold C elements on x's device");
  return p.detach().to(torch::kFloat32).contiguous();
}

static const __bf16* gn_cptr(const torch::Tensor& t) {
  return reinterpret_cast<const __bf16*>(t.data_ptr());
}

std::vector<torch::Tensor> gn_fwd(torch::Tensor x, torch::Tensor gamma,
                                  torch::Tensor beta, int64_t G, double eps,
                                  bool act, double slope) {
  const GnShape s = gn_shape(x, G, "gn_fwd");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto xa = gn_aligned(x);
  auto g = gn_affine(gamma, x, s.C, "gamma");
  auto b = gn_affine(beta, x, s.C, "beta");
  const int64_t rows = (int64_t)s.N * G;
  int64_t chunk;
  const int64_t splits = gn_split(s.L, rows, &chunk);
  auto f32 = x.options().dtype(torch::kFloat32);
  auto part = torch::empty({rows, splits, 3}, f32);
  auto mean_rstd = torch::empty({rows, 2}, f32);
  auto y = torch::empty_like(xa);

  hipLaunchKernelGGL(gn_stats_kernel, dim3((unsigned)splits, (unsigned)rows),
                     dim3(GN_BLOCK), 0, current_stream(), gn_cptr(xa),
                     part.data_ptr<float>(), s.L, chunk);
  const int nc = s.N * s.C;
  const int64_t chunks = std::min<int64_t>(
      std::max<int64_t>(1, (s.S / 8 + GN_BLOCK * 4 - 1) / (GN_BLOCK * 4)),
      std::max<int64_t>(1, 4096 / nc));
  dispatch_bool(act, [&](auto a) {
    hipLaunchKernelGGL((gn_normalize_kernel<decltype(a)::value>),
                       dim3((unsigned)chunks, (unsigned)nc), dim3(GN_BLOCK),
                       0, current_stream(), gn_cptr(xa),
                       reinterpret_cast<__bf16*>(y.data_ptr()),
                       part.data_ptr<float>(), mean_rstd.data_ptr<float>(),
                       g.data_ptr<float>(), b.data_ptr<float>(), s.C, s.cpg,
                       (int)splits, s.S, (float)(1.0 / (double)s.L),
                       (float)eps, (float)slope);
  });
  return {y, mean_rstd};
}

std::vector<torch::Tensor> gn_bwd(torch::Tensor dy, torch::Tensor x,
                                  torch::Tensor mean_rstd,
                                  torch::Tensor gamma, torch::Tensor beta,
                                  int64_t G, bool act, double slope) {
  const GnShape s = gn_shape(x, G, "gn_bwd");
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == torch::kBFloat16 &&
              dy.is_contiguous() && dy.sizes() == x.sizes() &&
              dy.device() == x.device(),
              "gn_bwd: dy must be contiguous bf16 of x's shape and device");
  const int64_t rows = (int64_t)s.N * G;
  TORCH_CHECK(mean_rstd.is_cuda() && mean_rstd.is_contiguous() &&
              mean_rstd.scalar_type() == torch::kFloat32 &&
              mean_rstd.numel() == rows * 2 &&
              mean_rstd.device() == x.device(),
              "gn_bwd: mean_rstd must be contiguous fp32 [N*G][2]");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  auto xa = gn_aligned(x);
  auto dya = gn_aligned(dy);
  auto g = gn_affine(gamma, x, s.C, "gamma");
  auto b = gn_affine(beta, x, s.C, "beta");
  const int nc = s.N * s.C;
  int64_t chunk;
  const int64_t splits = gn_split(s.S, nc, &chunk);
  auto f32 = x.options().dtype(torch::kFloat32);
  auto part = torch::empty({(int64_t)nc, splits, 2}, f32);
  auto dx = torch::empty_like(xa);
  auto dgamma = torch::empty({(int64_t)s.C}, f32);
  auto dbeta = torch::empty({(int64_t)s.C}, f32);
  const dim3 grid((unsigned)splits, (unsigned)nc), blk(GN_BLOCK);

  dispatch_bool(act, [&](auto a) {
    constexpr bool ACT = decltype(a)::value;
    hipLaunchKernelGGL((gn_bwd_reduce_kernel<ACT>), grid, blk, 0,
                       current_stream(), gn_cptr(dya), gn_cptr(xa),
                       mean_rstd.data_ptr<float>(), g.data_ptr<float>(),
                       b.data_ptr<float>(), part.data_ptr<float>(), s.C,
                       s.cpg, s.S, chunk, (float)slope);
    hipLaunchKernelGGL((gn_bwd_dx_kernel<ACT>), grid, blk, 0,
                       current_stream(), gn_cptr(dya), gn_cptr(xa),
                       reinterpret_cast<__bf16*>(dx.data_ptr()),
                       mean_rstd.data_ptr<float>(), g.data_ptr<float>(),
                       b.data_ptr<float>(), part.data_ptr<float>(), s.C,
                       s.cpg, s.S, chunk, (float)(1.0 / (double)s.L),
                       (float)slope);
  });
  hipLaunchKernelGGL(gn_bwd_affine_kernel, dim3((unsigned)s.C), blk, 0,
                     current_stream(), part.data_ptr<float>(),
                     dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), s.N,
                     s.C, (int)splits);
  return {dx, dgamma, dbeta};
}
