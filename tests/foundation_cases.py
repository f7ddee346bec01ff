"""Case tables and float64 references for the first-generation kernels
(adam.hip, lsnll.hip, metrics.hip, pack.hip, linear.hip).

test_foundation_cpu.py validates the references against torch's fp32 CPU
functionals; test_gpu_foundation.py holds the kernels to them. Every
reference is plain float64 arithmetic on the CPU, written out, on inputs
that were already rounded to the kernel's input dtype.

Tolerance rule of the GPU tests (`check`): with err_kernel = max|kernel -
ref64| and err_torch = max|torch - ref64|, torch's own implementation run
on the same device at the same input dtype,

    err_kernel <= 4 * err_torch + 1 ulp(output dtype) at max|ref64|.

The factor 4 allows for another summation order, split-K atomics and the
fast exp/log intrinsics; a dropped element or a transposed fragment is
orders of magnitude. Integer outputs compare with torch.equal.
"""
import math
import random

import torch

EPS = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7,
       torch.float16: 2.0 ** -10, torch.float64: 2.0 ** -52}
TINY = {torch.float32: 2.0 ** -126, torch.bfloat16: 2.0 ** -126,
        torch.float16: 2.0 ** -14, torch.float64: 2.0 ** -1022}


def ulp_at(dtype, mag):
    """Spacing of `dtype` at magnitude `mag` (of its smallest normal at 0)."""
    mag = max(float(mag), TINY[dtype])
    return EPS[dtype] * 2.0 ** math.floor(math.log2(mag))


def max_err(out, ref64):
    if ref64.numel() == 0:
        return 0.0
    return float((out.detach().double().cpu() - ref64).abs().max())


def rule(kernel_out, torch_out, ref64, out_dtype=None):
    """(err_kernel, err_torch, bound) of the tolerance rule above; the ulp
    is that of `out_dtype`, by default kernel_out's own."""
    assert kernel_out.shape == ref64.shape == torch_out.shape, (
        kernel_out.shape, torch_out.shape, ref64.shape)
    assert torch.isfinite(ref64).all()
    err_k, err_t = max_err(kernel_out, ref64), max_err(torch_out, ref64)
    mag = float(ref64.abs().max()) if ref64.numel() else 0.0
    return err_k, err_t, 4.0 * err_t + ulp_at(out_dtype or kernel_out.dtype,
                                              mag)


MEASURED = {}   # family -> (err_kernel, err_torch, bound, case) of the worst


def check(family, case, kernel_out, torch_out, ref64, out_dtype=None):
    """Print the measured pair, keep the worst per family, then assert."""
    err_k, err_t, bound = rule(kernel_out, torch_out, ref64, out_dtype)
    worst = MEASURED.get(family)
    if worst is None or err_k / bound > worst[0] / worst[2]:
        MEASURED[family] = (err_k, err_t, bound, case)
    print(f'FOUNDATION {family} [{case}] err_kernel={err_k:.3e} '
          f'err_torch={err_t:.3e} bound={bound:.3e}')
    assert err_k <= bound, (
        f'{family} [{case}]: err_kernel {err_k:.3e} > 4 * err_torch '
        f'{err_t:.3e} + 1 ulp = {bound:.3e}')


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------- Adam / SGD
ADAM_CHUNK = 16384          # fused_adam cuts tensors into blocks of this
ADAM_LIST_NUMELS = [0, 1, 16383, 16384, 16385, 2 * 16384 + 3]
ADAM_KW = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
ADAM_STEPS = 3

# fused_adam_flat: (n, element offsets of the p, g, m, v views, step).
# n = 2^21 + 4099 exceeds 2048 blocks * 256 threads both as float4 vectors
# (aligned streams) and as scalars (any misaligned stream): it wraps the
# vector loop in the first form and the tail loop in the second.
ADAM_FLAT_OFFSETS = [(0, 0, 0, 0), (1, 0, 0, 0), (1, 1, 1, 1)]
ADAM_FLAT_BIG = 2 ** 21 + 4099
ADAM_FLAT_CASES = (
    [(n, offs, step) for n in (3, 4096, 4097, 4099)
     for offs in ADAM_FLAT_OFFSETS for step in (1, 5000)]
    + [(ADAM_FLAT_BIG, (0, 0, 0, 0), 1), (ADAM_FLAT_BIG, (1, 1, 1, 1), 5000)])

# (momentum, weight_decay, grad dtype, numel)
SGD_CASES = [(0.0, 0.01, torch.float32, 1000), (0.9, 0.01, torch.float32, 1000),
             (0.9, 0.01, torch.bfloat16, 1000), (0.0, 0.01, torch.bfloat16, 257),
             (0.9, 0.01, torch.float32, 0), (0.0, 0.0, torch.float32, 0)]
SGD_LR, SGD_STEPS = 0.1, 3


def adam_ref(p, grads, m=None, v=None, *, lr, betas, eps, weight_decay,
             first_step=1):
    """float64 Adam steps, one per entry of `grads`: L2 weight decay added to
    the gradient, bias-corrected moments, eps outside the sqrt."""
    b1, b2 = betas
    p = p.detach().double().cpu().clone()
    m = torch.zeros_like(p) if m is None else m.double().cpu().clone()
    v = torch.zeros_like(p) if v is None else v.double().cpu().clone()
    for k, g in enumerate(grads):
        t = first_step + k
        g = g.detach().double().cpu() + weight_decay * p
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        mhat, vhat = m / (1 - b1 ** t), v / (1 - b2 ** t)
        p = p - lr * mhat / (vhat.sqrt() + eps)
    return p, m, v


def sgd_ref(p, grads, *, lr, momentum, weight_decay):
    """float64 SGD steps: L2 weight decay, then the momentum buffer
    (buf = momentum * buf + g, zero at the start)."""
    p = p.detach().double().cpu().clone()
    buf = torch.zeros_like(p)
    for g in grads:
        g = g.detach().double().cpu() + weight_decay * p
        if momentum != 0:
            buf = momentum * buf + g
            g = buf
        p = p - lr * g
    return p


# ------------------------------------------------------ cross-entropy, argmax
CE_SHAPES = ([(B, C) for B in (1, 3, 5) for C in (1, 2, 63, 64, 65, 129, 1000)]
             + [(8195, 2), (8195, 65)])     # 8195 > 2048 blocks * 4 waves
CE_DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CE_REGIMES = ['randn', 'confident', 'offset', 'neginf']
CE_GRAD_OUT = 3.5


def ce_inputs(B, C, dtype, regime, seed=0):
    """(logits rounded to `dtype`, int64 target) on the CPU. 'neginf' sets
    one class per row to -inf, never the target's."""
    g = gen(seed * 7919 + B * 1009 + C)
    x = torch.randn(B, C, generator=g, dtype=torch.float64)
    y = torch.randint(0, C, (B,), generator=g)
    if regime == 'confident':
        x = x * 30
    elif regime == 'offset':
        x = x + 1e4
    elif regime == 'neginf':
        if C < 2:
            return None
        off = torch.randint(1, C, (B,), generator=g)
        x[torch.arange(B), (y + off) % C] = -math.inf
    return x.to(dtype), y


def ce_ref(x, y, grad_out=1.0):
    """float64 mean NLL of log-softmax and grad_out * d loss / d logits."""
    x = x.detach().double().cpu()
    y = y.cpu().long()
    B, C = x.shape
    z = x - x.amax(dim=1, keepdim=True)
    lp = z - z.exp().sum(dim=1, keepdim=True).log()
    rows = torch.arange(B)
    loss = -lp[rows, y].sum() / B if B else torch.tensor(math.nan).double()
    onehot = torch.zeros(B, C, dtype=torch.float64)
    onehot[rows, y] = 1.0
    grad = (lp.exp() - onehot) * (grad_out / max(B, 1))
    return loss, grad


def argmax_ref(x):
    """Lowest index among the row maxima (int64), on the CPU."""
    from coinstac_dinunet_amd import ops
    return ops.argmax_lowest(x.detach().cpu().float())


ARGMAX_TIE_C = [64, 65, 130]


def argmax_tie_rows(C, dtype, seed=0):
    """Rows whose maximum is attained more than once, placed so that a
    reduction preferring the higher index, the lower lane or the first hit
    in a lane gives another answer than the lowest index. One wave reduces
    a row: class c sits in lane c % 64."""
    g = gen(seed + C)
    pairs = [(3, 37), (10, 11), (0, C - 1), (31, 32), (62, 63)]
    if C > 64:
        # same lane: c and c + 64; and the lower index in the higher lane
        pairs += [(0, 64), (40, 64), (63, C - 1)]
    if C > 128:
        pairs += [(1, 65), (1, 129), (65, 129), (70, 128)]
    rows = []
    for a, b in pairs:
        r = torch.rand(C, generator=g) - 2.0        # all below the ties
        r[a] = r[b] = 5.0
        rows.append(r)
        r = r.clone()                                # three-way tie
        r[(a + b) // 2] = 5.0
        rows.append(r)
    rows.append(torch.full((C,), 1.25))              # all equal
    rows.append(torch.full((C,), -math.inf))         # all -inf: index 0
    r = torch.full((C,), -math.inf)                  # a single finite value
    r[C - 1] = -3.0
    rows.append(r)
    return torch.stack(rows).to(dtype)


# -------------------------------------------------------------------- metrics
PRF_BIG = 2048 * 256 * 16 + 257     # past 2048 blocks * 256 threads * 16
PRF_NS = [0, 1, 63, 64, 65, 255, 256, 257, PRF_BIG]
PRF_DTYPES = [torch.bool, torch.uint8, torch.int32, torch.int64]
CONF_KS = [1, 2, 7, 128, 129, 202]   # 129^2 * 4 B is the first past 64 KB
CONF_N = 5000
CONF_TOO_LARGE = 203                 # 203^2 * 4 B > 160 KB


def prf_ref(pred, true):
    """[tp, fp, tn, fn] with non-zero counting as positive."""
    cases = ((true.cpu().reshape(-1) != 0).long() * 2
             + (pred.cpu().reshape(-1) != 0).long())
    tn, fp, fn, tp = torch.bincount(cases, minlength=4).tolist()
    return [tp, fp, tn, fn]


def confusion_ref(pred, true, K):
    """int64 [K, K] matrix[true][pred]; pairs with a label outside [0, K)
    on either side are dropped."""
    p, t = pred.cpu().reshape(-1).long(), true.cpu().reshape(-1).long()
    keep = (p >= 0) & (p < K) & (t >= 0) & (t < K)
    return torch.bincount(t[keep] * K + p[keep],
                          minlength=K * K).reshape(K, K)


# ---------------------------------------------------------------- pack/unpack
def _cycle(sizes, count):
    return [sizes[i % len(sizes)] for i in range(count)]


PACK_LISTS = {
    'empty': [],
    'single': [(33, 3)],
    'zero_first': [(0,), (17,), (5, 5)],
    'zero_middle': [(17,), (0,), (5, 5)],
    'zero_last': [(17,), (5, 5), (0,)],
    'zero_adjacent': [(0,), (0, 4), (17,), (0,), (0,), (3,), (0,), (0,)],
    'only_zero': [(0,), (0,)],
    'many': [(s,) for s in _cycle([1, 2, 63, 64, 65, 257], 300)],
}
PACK_GUARD = 3          # sentinel elements between unpack destinations
PACK_SENTINEL = -777.0


# --------------------------------------------------------------------- linear
def linear_shapes():
    """About 25 (M, N, K) out of M, N in {1, 63, 64, 65} and K in {1, 15,
    16, 17, 33} (the block tile is 64 x 64, the K step 16), always with the
    all-ones and the all-65 corner."""
    grid = [(M, N, K) for M in (1, 63, 64, 65) for N in (1, 63, 64, 65)
            for K in (1, 15, 16, 17, 33)]
    fixed = [(1, 1, 1), (65, 65, 65), (65, 65, 33), (64, 64, 16),
             (63, 65, 17), (65, 63, 15)]
    rest = [s for s in grid if s not in fixed]
    return fixed + random.Random(0).sample(rest, 25 - len(fixed))


LINEAR_SHAPES = linear_shapes()
LINEAR_DTYPES = [torch.float32, torch.bfloat16]
SPLITK_SHAPES = [(M, 33, 17) for M in (64, 65, 100, 1000)]  # split: M > 64
COLSUM_SHAPES = [(M, N) for M in (1, 255, 256, 257, 5000) for N in (1, 3)]
GS_SHAPES = [(n, r) for r in (1, 2, 4, 8) for n in (63, 257, 5000)]
GS_EPS = 1e-8


def linear_inputs(M, N, K, dtype, seed=0):
    """x [M, K], w [N, K], b [N] (fp32), go [M, N] on the CPU, rounded to
    `dtype`, with asymmetric spikes so a transposed staging cannot cancel."""
    g = gen(seed + M * 10007 + N * 101 + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g)
    go = torch.randn(M, N, generator=g)
    go[min(2, M - 1), min(5, N - 1)] += 7.0
    w[min(3, N - 1), min(1, K - 1)] += 5.0
    x[min(1, M - 1), min(4, K - 1)] -= 6.0
    return x.to(dtype), w.to(dtype), b, go.to(dtype)


def linear_ref(x, w, b=None, relu=False):
    out = x.double().cpu() @ w.double().cpu().t()
    if b is not None:
        out = out + b.double().cpu()
    return out.clamp_min(0) if relu else out


def dgrad_ref(go, w):
    return go.double().cpu() @ w.double().cpu()


def wgrad_ref(go, x):
    return go.double().cpu().t() @ x.double().cpu()


def colsum_ref(g):
    return g.double().cpu().sum(dim=0)


def gram_schmidt_ref(a, eps=GS_EPS):
    """Classical Gram-Schmidt in float64: column i of `a` minus its
    projections on the finished columns, over (its norm + eps)."""
    a = a.double().cpu()
    q = torch.zeros_like(a)
    for i in range(a.shape[1]):
        v = a[:, i].clone()
        for j in range(i):
            v -= (q[:, j] @ a[:, i]) * q[:, j]
        q[:, i] = v / (v.norm() + eps)
    return q


def gram_schmidt_torch(m, eps=GS_EPS):
    """The torch loop of distrib.powersgd.orthogonalize, in place, in the
    dtype and on the device of `m` (the yardstick for the kernel)."""
    r = m.shape[1]
    for i in range(r):
        col = m[:, i:i + 1]
        col.div_(torch.norm(col) + eps)
        if i + 1 < r:
            rest = m[:, i + 1:]
            rest.sub_(col @ (col.t() @ rest))
    return m
