"""The float64 references of foundation_cases.py against torch's fp32 CPU
functionals, over the same case tables the GPU tests use, and the ops.*
functions that have a CPU path (cross_entropy, argmax_rows, linear) over
those tables too. No GPU.

Bounds are forward-error bounds of the fp32 computation, in units of
u = 2^-24 (one rounding): `roundings * u * scale`, with the count of
roundings and the scale worked out per family below, never taken from
what the functions return."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import foundation_cases as fc
from coinstac_dinunet_amd import ops

U = 2.0 ** -24


def close(out, ref64, roundings, scale):
    err = fc.max_err(out, ref64)
    bound = roundings * U * scale
    assert err <= bound, f'err {err:.3e} > {roundings} u * {scale:.3e}'


# ---------------------------------------------------------------- Adam / SGD
def _torch_adam(p0, grads, m=None, v=None, first_step=1, **kw):
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], **kw)
    if m is not None:
        opt.state[p] = dict(step=torch.tensor(float(first_step - 1)),
                            exp_avg=m.clone(), exp_avg_sq=v.clone())
    for g in grads:
        p.grad = g.clone()
        opt.step()
    return p.detach()


@pytest.mark.parametrize('n', [n for n in fc.ADAM_LIST_NUMELS if n])
def test_adam_ref_matches_torch_cpu(n):
    # per step: p is rounded once (u * |p|); the update lr * mhat /
    # (sqrt(vhat) + eps) is at most a few lr = 1e-2 in size and about ten
    # roundings deep, below u * 1. Four roundings of max(|p|, 1) a step.
    g = fc.gen(n)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (k + 1)
             for k in range(fc.ADAM_STEPS)]
    ref, _, _ = fc.adam_ref(p0, grads, **fc.ADAM_KW)
    out = _torch_adam(p0, grads, **fc.ADAM_KW)
    close(out, ref, 4 * fc.ADAM_STEPS, max(1.0, float(ref.abs().max())))


@pytest.mark.parametrize('step', [1, 5000])
def test_adam_ref_with_state_matches_torch_cpu(step):
    g = fc.gen(step)
    n = 4099
    p0, grad = torch.randn(n, generator=g), torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.1
    ref, m_ref, v_ref = fc.adam_ref(p0, [grad], m, v, first_step=step,
                                    **fc.ADAM_KW)
    out = _torch_adam(p0, [grad], m, v, first_step=step, **fc.ADAM_KW)
    close(out, ref, 4, max(1.0, float(ref.abs().max())))


@pytest.mark.parametrize('momentum,wd', [(0.0, 0.01), (0.9, 0.01)])
def test_sgd_ref_matches_torch_cpu(momentum, wd):
    # per step: g + wd * p and momentum * buf + g are two roundings each of
    # |buf| <= 10 max|g| (geometric sum at 0.9), times lr = 0.1, and p is
    # rounded once: under six roundings of max(|p|, |g|) a step
    g = fc.gen(11)
    n = 1000
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(fc.SGD_STEPS)]
    ref = fc.sgd_ref(p0, grads, lr=fc.SGD_LR, momentum=momentum,
                     weight_decay=wd)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([p], lr=fc.SGD_LR, momentum=momentum,
                          weight_decay=wd)
    for gr in grads:
        p.grad = gr.clone()
        opt.step()
    scale = max(float(ref.abs().max()), max(float(x.abs().max())
                                            for x in grads))
    close(p.detach(), ref, 6 * fc.SGD_STEPS, scale)


# ------------------------------------------------------ cross-entropy, argmax
@pytest.mark.parametrize('fn', [F.cross_entropy, ops.cross_entropy],
                         ids=['torch', 'ops'])
@pytest.mark.parametrize('dtype', fc.CE_DTYPES, ids=str)
@pytest.mark.parametrize('B,C', fc.CE_SHAPES)
def test_ce_ref_matches_torch_cpu(B, C, dtype, fn):
    # a log-probability is (x - max) - log(sum exp): the subtraction from
    # the row maximum is exact or one rounding, exp and log one each, the
    # sum of C terms at most log2(C) + 1 roundings deep when blocked: 16
    # roundings of max|logprob| cover C <= 1000. A softmax entry p =
    # exp(lp) carries lp's absolute error times p, and p * |lp| <= 1/e, so
    # the gradient is within 16 u of grad_out / B.
    for regime in fc.CE_REGIMES:
        made = fc.ce_inputs(B, C, dtype, regime)
        if made is None:
            continue
        x, y = made
        ref_loss, ref_grad = fc.ce_ref(x, y, fc.CE_GRAD_OUT)
        x32 = x.float().requires_grad_(True)
        loss = fn(x32, y)
        (loss * fc.CE_GRAD_OUT).backward()
        close(loss.detach(), ref_loss, 16,
              max(1.0, float(ref_loss.abs()) * B))
        close(x32.grad, ref_grad, 16, fc.CE_GRAD_OUT / B)


def test_ce_ref_empty_batch_is_nan():
    loss, grad = fc.ce_ref(torch.zeros(0, 5), torch.zeros(0).long())
    assert math.isnan(float(loss)) and grad.shape == (0, 5)
    assert math.isnan(float(F.cross_entropy(torch.zeros(0, 5),
                                            torch.zeros(0).long())))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize('C', fc.ARGMAX_TIE_C)
def test_argmax_ref_is_first_occurrence(C, dtype):
    x = fc.argmax_tie_rows(C, dtype)
    ref = fc.argmax_ref(x)
    assert ref.dtype == torch.int64
    # numpy documents first occurrence on ties
    first = torch.from_numpy(np.argmax(x.float().numpy(), axis=1))
    assert torch.equal(ref, first)
    assert torch.equal(ops.argmax_rows(x.float()), ref)
    assert ref[-2] == 0 and ref[-1] == C - 1      # all -inf; one finite


# -------------------------------------------------------------------- metrics
def test_count_refs_against_loops():
    g = fc.gen(5)
    pred = torch.randint(-2, 9, (300,), generator=g)
    true = torch.randint(-2, 9, (300,), generator=g)
    tp = sum(1 for p, t in zip(pred.tolist(), true.tolist()) if p and t)
    fp = sum(1 for p, t in zip(pred.tolist(), true.tolist()) if p and not t)
    tn = sum(1 for p, t in zip(pred.tolist(), true.tolist())
             if not p and not t)
    fn = sum(1 for p, t in zip(pred.tolist(), true.tolist()) if not p and t)
    assert fc.prf_ref(pred, true) == [tp, fp, tn, fn]
    K = 7
    mat = torch.zeros(K, K, dtype=torch.int64)
    for p, t in zip(pred.tolist(), true.tolist()):
        if 0 <= p < K and 0 <= t < K:
            mat[t, p] += 1
    assert torch.equal(fc.confusion_ref(pred, true, K), mat)
    assert 0 < mat.sum() < 300                     # some pairs were dropped
    assert fc.prf_ref(pred[:0], true[:0]) == [0, 0, 0, 0]
    assert torch.equal(fc.confusion_ref(pred[:0], true[:0], 3),
                       torch.zeros(3, 3, dtype=torch.int64))


# --------------------------------------------------------------------- linear
@pytest.mark.parametrize('fn', ['torch', 'ops'])
@pytest.mark.parametrize('M,N,K', fc.LINEAR_SHAPES)
def test_linear_refs_match_torch_cpu(M, N, K, fn):
    # a length-L fp32 dot product is within L u of sum |a||b|; bias and
    # the final rounding add two
    x, w, b, go = fc.linear_inputs(M, N, K, torch.float32)
    lin = F.linear if fn == 'torch' else ops.linear
    absdot = float((x.abs().double() @ w.abs().double().t()).max()
                   + b.abs().max())
    for bias, relu in [(None, False), (b, False), (b, True)]:
        out = lin(x, w, bias)
        if relu:
            out = torch.relu(out) if fn == 'torch' else ops.linear(
                x, w, bias, relu=True)
        close(out, fc.linear_ref(x, w, bias, relu), K + 2, absdot)
    close(go @ w, fc.dgrad_ref(go, w), N + 1,
          float((go.abs().double() @ w.abs().double()).max()))
    close(go.t() @ x, fc.wgrad_ref(go, x), M + 1,
          float((go.abs().double().t() @ x.abs().double()).max()))


@pytest.mark.parametrize('M,N', fc.COLSUM_SHAPES)
def test_colsum_ref_matches_torch_cpu(M, N):
    g = torch.randn(M, N, generator=fc.gen(M + N))
    close(g.sum(0), fc.colsum_ref(g), M, float(g.abs().sum(0).max()))


@pytest.mark.parametrize('n,r', fc.GS_SHAPES)
def test_gram_schmidt_ref_matches_torch_cpu(n, r):
    # each of the r column passes takes length-n norms and dot products
    # (blocked sums, log2(n) roundings deep) and a Gaussian [n, r] matrix
    # with n >= 63 >> r is well conditioned (singular values within
    # sqrt(n) +- sqrt(r)), so errors are not amplified: 8 r log2(n) u of
    # the largest entry.
    a = torch.randn(n, r, generator=fc.gen(n + r))
    ref = fc.gram_schmidt_ref(a)
    out = fc.gram_schmidt_torch(a.clone())
    close(out, ref, 8 * r * math.log2(n), float(ref.abs().max()))
    # dividing by (norm + eps) leaves columns short by eps / norm, norm > 1
    gram = ref.t() @ ref - torch.eye(r, dtype=torch.float64)
    assert float(gram.abs().max()) < 2 * fc.GS_EPS + 1e-12


def test_gram_schmidt_ref_zero_column():
    a = torch.randn(63, 3, generator=fc.gen(1))
    a[:, 1] = 0
    q = fc.gram_schmidt_ref(a)
    assert torch.isfinite(q).all() and not q[:, 1].any()


def test_tables_reach_the_paths_they_name():
    assert any(n > fc.ADAM_CHUNK for n in fc.ADAM_LIST_NUMELS)
    assert fc.ADAM_FLAT_BIG // 4 > 2048 * 256           # vector loop wraps
    assert max(B for B, _ in fc.CE_SHAPES) > 2048 * 4   # row loop wraps
    assert max(C for _, C in fc.CE_SHAPES) > 64         # strided lane loop
    assert fc.PRF_BIG > 2048 * 256 * 16
    assert 128 * 128 * 4 <= 64 * 1024 < 129 * 129 * 4
    assert 202 * 202 * 4 <= 160 * 1024 < fc.CONF_TOO_LARGE ** 2 * 4
    assert (1, 1, 1) in fc.LINEAR_SHAPES and (65, 65, 65) in fc.LINEAR_SHAPES
    assert 20 <= len(set(fc.LINEAR_SHAPES)) == len(fc.LINEAR_SHAPES) <= 30
    assert len(fc.PACK_LISTS['many']) == 300
