"""First-generation kernels (adam.hip, lsnll.hip, metrics.hip, pack.hip,
linear.hip) against the float64 references of foundation_cases.py, at the
shapes where each kernel changes path: chunk and tile edges, misaligned
views, grid-stride wrap, empty inputs, ties.

Floating results obey the rule of foundation_cases.check: err_kernel <=
4 * err_torch + 1 ulp of the output dtype, torch's own implementation on
this device at the same input dtype being the yardstick. Integer results
are exact. Every "raises" case is a host check in front of the launch."""
import pytest
import torch
import torch.nn.functional as F

import foundation_cases as fc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    C = ops.require_native()


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    yield torch.device('cuda:0')
    for family, (ek, et, bound, case) in sorted(fc.MEASURED.items()):
        print(f'FOUNDATION-WORST {family}: err_kernel={ek:.3e} '
              f'err_torch={et:.3e} bound={bound:.3e} at [{case}]')


class Soft:
    """Run every check of a test, then fail with all that missed."""

    def __init__(self):
        self.failed = []

    def check(self, *args, **kw):
        try:
            fc.check(*args, **kw)
        except AssertionError as e:
            self.failed.append(str(e))

    def done(self):
        assert not self.failed, '\n'.join(self.failed)


def _launches_ok(dev):
    """A refused launch leaves its error for the next one to report."""
    assert float((torch.zeros(4, device=dev) + 1).sum()) == 4.0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- Adam / SGD
def _steps(opt, params, grads_per_step):
    for grads in grads_per_step:
        for p, g in zip(params, grads):
            p.grad = g.clone()
        opt.step()


def test_fused_adam_list_across_chunks(dev):
    g = fc.gen(0)
    p0 = [torch.randn(n, generator=g) for n in fc.ADAM_LIST_NUMELS]
    grads = [[torch.randn(n, generator=g) * (k + 1)
              for n in fc.ADAM_LIST_NUMELS] for k in range(fc.ADAM_STEPS)]
    dgrads = [[x.to(dev) for x in step] for step in grads]
    p_hip = [p.to(dev).requires_grad_(True) for p in p0]
    p_ref = [p.to(dev).requires_grad_(True) for p in p0]
    opt_hip = ops.FusedAdam(p_hip, **fc.ADAM_KW)
    opt_ref = torch.optim.Adam(p_ref, **fc.ADAM_KW)
    _steps(opt_hip, p_hip, dgrads)
    _steps(opt_ref, p_ref, dgrads)
    soft = Soft()
    for i, n in enumerate(fc.ADAM_LIST_NUMELS):
        ref, m, v = fc.adam_ref(p0[i], [s[i] for s in grads], **fc.ADAM_KW)
        soft.check('adam', f'list n={n} p', p_hip[i].detach(),
                   p_ref[i].detach(), ref)
        if n:
            soft.check('adam', f'list n={n} m',
                       opt_hip.state[p_hip[i]]['exp_avg'],
                       opt_ref.state[p_ref[i]]['exp_avg'], m)
            soft.check('adam', f'list n={n} v',
                       opt_hip.state[p_hip[i]]['exp_avg_sq'],
                       opt_ref.state[p_ref[i]]['exp_avg_sq'], v)
    soft.done()


SENTINEL = -777.0


def _arena_views(n, offs, dev):
    """Four views of n elements into one sentinel-filled arena, stream k at
    a 16-byte-aligned start plus offs[k] elements."""
    stride = (n + 8 + 3) // 4 * 4
    arena = torch.full((4 * stride + 8,), SENTINEL, device=dev)
    assert arena.data_ptr() % 16 == 0
    views = [arena[k * stride + 4 + offs[k]:k * stride + 4 + offs[k] + n]
             for k in range(4)]
    for k, view in enumerate(views):
        assert (view.data_ptr() % 16 != 0) == bool(offs[k])
    return arena, views


@pytest.mark.parametrize('n,offs,step', fc.ADAM_FLAT_CASES)
def test_fused_adam_flat_arena_views(dev, n, offs, step):
    g = fc.gen(n + step)
    p0, grad = torch.randn(n, generator=g), torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 0.1
    v0 = torch.rand(n, generator=g) * 0.1
    arena, (p, gv, m, v) = _arena_views(n, offs, dev)
    for view, src in zip((p, gv, m, v), (p0, grad, m0, v0)):
        view.copy_(src)
    outside = arena == SENTINEL
    kw = fc.ADAM_KW
    C.fused_adam_flat(p, gv, m, v, kw['lr'], kw['betas'][0], kw['betas'][1],
                      kw['eps'], kw['weight_decay'], step)
    # torch, from the same state
    pt = p0.to(dev).requires_grad_(True)
    opt = torch.optim.Adam([pt], **kw)
    opt.state[pt] = dict(step=torch.tensor(float(step - 1)),
                         exp_avg=m0.to(dev), exp_avg_sq=v0.to(dev))
    pt.grad = grad.to(dev)
    opt.step()
    ref, m_ref, v_ref = fc.adam_ref(p0, [grad], m0, v0, first_step=step, **kw)
    case = f'flat n={n} offs={offs} step={step}'
    soft = Soft()
    soft.check('adam', case + ' p', p, pt.detach(), ref)
    soft.check('adam', case + ' m', m, opt.state[pt]['exp_avg'], m_ref)
    soft.check('adam', case + ' v', v, opt.state[pt]['exp_avg_sq'], v_ref)
    soft.done()
    assert torch.equal(gv.cpu(), grad)                 # read only
    assert bool((arena[outside] == SENTINEL).all())    # nothing past a view


def test_fused_adam_flat_rejects_mismatch(dev):
    p, g, m, v = (torch.zeros(8, device=dev) for _ in range(4))
    with pytest.raises(RuntimeError, match='same numel'):
        C.fused_adam_flat(p, g[:7], m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    with pytest.raises(RuntimeError, match='contiguous'):
        C.fused_adam_flat(p[::2], g[::2], m[::2], v[:4], 1e-3, 0.9, 0.999,
                          1e-8, 0.0, 1)


def _layout_case(kind, dev):
    g = fc.gen(3)
    if kind == 'channels_last':
        p0 = torch.randn(8, 4, 3, 3, generator=g)
        grad = torch.randn(8, 4, 3, 3, generator=g)
        make_p = lambda: p0.to(dev).contiguous(  # noqa: E731
            memory_format=torch.channels_last).requires_grad_(True)
        make_g = lambda: grad.to(dev)  # noqa: E731  contiguous format
    else:
        p0 = torch.randn(64, 33, generator=g)
        grad = torch.randn(64, 33, generator=g)
        make_p = lambda: p0.to(dev).requires_grad_(True)  # noqa: E731
        make_g = lambda: grad.t().contiguous().to(dev).t()  # noqa: E731
    return p0, grad, make_p, make_g


@pytest.mark.parametrize('kind', ['channels_last', 'transposed_grad'])
def test_fused_adam_layout_is_honoured_or_refused(dev, kind):
    """A parameter and a gradient laid out differently in memory: the
    elementwise torch result, or an error in front of the launch; never
    element i of one updated with element i of the other's storage."""
    p0, grad, make_p, make_g = _layout_case(kind, dev)
    p_hip, p_ref = make_p(), make_p()
    assert p_hip.stride() != make_g().stride()
    opt_hip = ops.FusedAdam([p_hip], **fc.ADAM_KW)
    opt_ref = torch.optim.Adam([p_ref], **fc.ADAM_KW)
    grads = [[make_g() * (k + 1)] for k in range(fc.ADAM_STEPS)]
    try:
        _steps(opt_hip, [p_hip], grads)
    except RuntimeError as e:
        assert 'fused_adam' in str(e)
        assert torch.equal(p_hip.detach().cpu(), p0)
        return
    _steps(opt_ref, [p_ref], grads)
    ref, _, _ = fc.adam_ref(p0, [grad * (k + 1)
                                 for k in range(fc.ADAM_STEPS)], **fc.ADAM_KW)
    fc.check('adam', f'layout {kind}', p_hip.detach(), p_ref.detach(), ref)
    assert p_hip.stride() == p_ref.stride()


@pytest.mark.parametrize('momentum,wd,gdtype,n', fc.SGD_CASES)
def test_fused_sgd(dev, momentum, wd, gdtype, n):
    g = fc.gen(n + int(momentum * 10))
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g).to(gdtype)
             for _ in range(fc.SGD_STEPS)]
    ref = fc.sgd_ref(p0, grads, lr=fc.SGD_LR, momentum=momentum,
                     weight_decay=wd)
    p_ref = p0.to(dev).requires_grad_(True)
    opt_ref = torch.optim.SGD([p_ref], lr=fc.SGD_LR, momentum=momentum,
                              weight_decay=wd)
    # torch takes no bf16 grad for an fp32 parameter: it gets the same
    # values widened
    _steps(opt_ref, [p_ref], [[x.float().to(dev)] for x in grads])
    p_hip = p0.to(dev).requires_grad_(True)
    if gdtype == torch.float32:
        opt = ops.FusedSGD([p_hip], lr=fc.SGD_LR, momentum=momentum,
                           weight_decay=wd)
        _steps(opt, [p_hip], [[x.to(dev)] for x in grads])
    else:
        buf = torch.zeros(n, device=dev)
        for x in grads:
            gd = x.to(dev)
            # without momentum the optimizer passes the grad as placeholder
            C.fused_sgd([p_hip.detach()], [gd], [buf if momentum else gd],
                        fc.SGD_LR, momentum, wd)
    fc.check('sgd', f'momentum={momentum} wd={wd} {gdtype} n={n}',
             p_hip.detach(), p_ref.detach(), ref)
    _launches_ok(dev)


# ------------------------------------------------------ cross-entropy, argmax
def _ce_pair(x, y, dev):
    """(kernel loss, kernel grad, torch loss, torch grad), grad_out = 3.5."""
    xk = x.to(dev).requires_grad_(True)
    xt = x.to(dev).requires_grad_(True)
    yd = y.to(dev)
    lk = ops.cross_entropy(xk, yd)
    (lk * fc.CE_GRAD_OUT).backward()
    lt = F.cross_entropy(xt, yd)
    (lt * fc.CE_GRAD_OUT).backward()
    return lk.detach(), xk.grad, lt.detach(), xt.grad


@pytest.mark.parametrize('dtype', fc.CE_DTYPES, ids=str)
@pytest.mark.parametrize('B,Cc', fc.CE_SHAPES)
def test_cross_entropy_2d(dev, B, Cc, dtype):
    soft = Soft()
    name = str(dtype).split('.')[-1]
    for regime in fc.CE_REGIMES:
        made = fc.ce_inputs(B, Cc, dtype, regime)
        if made is None:
            continue
        x, y = made
        ref_loss, ref_grad = fc.ce_ref(x, y, fc.CE_GRAD_OUT)
        lk, gk, lt, gt = _ce_pair(x, y, dev)
        assert lk.dtype == torch.float32 and lk.dim() == 0
        assert gk.dtype == dtype and gk.shape == (B, Cc)
        case = f'B={B} C={Cc} {name} {regime}'
        soft.check(f'ce_loss_{name}', case, lk, lt, ref_loss)
        soft.check(f'ce_grad_{name}', case, gk, gt, ref_grad)
        assert torch.equal(ops.argmax_rows(x.to(dev)).cpu(), fc.argmax_ref(x))
    soft.done()


def test_cross_entropy_noncontiguous_logits(dev):
    g = fc.gen(9)
    wide = torch.randn(5, 200, generator=g)
    y = torch.randint(0, 129, (5,), generator=g)
    wk = wide.to(dev).requires_grad_(True)
    wt = wide.to(dev).requires_grad_(True)
    assert not wk[:, 3:132].is_contiguous()
    lk = ops.cross_entropy(wk[:, 3:132], y.to(dev))
    (lk * fc.CE_GRAD_OUT).backward()
    lt = F.cross_entropy(wt[:, 3:132], y.to(dev))
    (lt * fc.CE_GRAD_OUT).backward()
    ref_loss, ref_grad = fc.ce_ref(wide[:, 3:132], y, fc.CE_GRAD_OUT)
    full = torch.zeros(5, 200, dtype=torch.float64)
    full[:, 3:132] = ref_grad
    fc.check('ce_loss_float32', 'column slice', lk.detach(), lt.detach(),
             ref_loss)
    fc.check('ce_grad_float32', 'column slice', wk.grad, wt.grad, full)
    assert torch.equal(ops.argmax_rows(wk.detach()[:, 3:132]).cpu(),
                       fc.argmax_ref(wide[:, 3:132]))


def test_cross_entropy_target_dtypes(dev):
    x, y = fc.ce_inputs(5, 65, torch.float32, 'randn')
    xd = x.to(dev)
    ref_loss, _ = fc.ce_ref(x, y)
    tor = F.cross_entropy(xd, y.to(dev))
    grads = []
    for dt in (torch.int64, torch.int32, torch.uint8):
        xl = xd.clone().requires_grad_(True)
        loss = ops.cross_entropy(xl, y.to(dt).to(dev))
        # the wave partials fold by atomics in any order: the same loss up
        # to that, the same gradient to the bit
        fc.check('ce_loss_float32', f'target {dt}', loss.detach(), tor,
                 ref_loss)
        loss.backward()
        grads.append(xl.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    with pytest.raises(TypeError):
        ops.cross_entropy(xd, y.float().to(dev))
    with pytest.raises(RuntimeError, match='int64'):
        C.logsoftmax_nll_fwd(xd, y.int().to(dev))
    with pytest.raises(RuntimeError, match='int64'):
        C.logsoftmax_nll_fwd(xd, y[:4].to(dev))


def test_cross_entropy_empty_batch(dev):
    x = torch.empty(0, 5, device=dev, requires_grad=True)
    y = torch.empty(0, dtype=torch.int64, device=dev)
    loss = ops.cross_entropy(x, y)
    ref = F.cross_entropy(x.detach(), y)
    torch.testing.assert_close(loss.detach(), ref, equal_nan=True)
    (loss * fc.CE_GRAD_OUT).backward()
    assert x.grad.shape == (0, 5)
    out = ops.argmax_rows(x.detach())
    assert out.shape == (0,) and out.dtype == torch.int64
    _launches_ok(dev)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize('Cc', fc.ARGMAX_TIE_C)
def test_argmax_rows_ties_take_lowest_index(dev, Cc, dtype):
    x = fc.argmax_tie_rows(Cc, dtype)
    out = ops.argmax_rows(x.to(dev))
    assert out.dtype == torch.int64
    ref = fc.argmax_ref(x)
    assert torch.equal(out.cpu(), ref), (out.cpu() - ref).nonzero().tolist()


# -------------------------------------------------------------------- metrics
def _labels(n, dtype, gen, lo=-3, hi=8):
    if dtype == torch.bool:
        return torch.randint(0, 2, (n,), generator=gen).bool()
    if dtype == torch.uint8:
        lo = 0
    # half the entries zero, the rest anything: non-zero is positive
    vals = torch.randint(lo, hi, (n,), generator=gen)
    zero = torch.randint(0, 2, (n,), generator=gen).bool()
    return torch.where(zero, torch.zeros_like(vals), vals).to(dtype)


@pytest.mark.parametrize('dtype', fc.PRF_DTYPES, ids=str)
@pytest.mark.parametrize('n', fc.PRF_NS)
def test_prf1a_counts(dev, n, dtype):
    g = fc.gen(n % 1000)
    pred, true = _labels(n, dtype, g), _labels(n, dtype, g)
    got = ops.prf1a_counts(pred.to(dev), true.to(dev))
    assert list(got) == fc.prf_ref(pred, true) and sum(got) == n


@pytest.mark.parametrize('n', [1, 257])
def test_prf1a_counts_one_sided(dev, n):
    ones = torch.full((n,), 5, dtype=torch.int32, device=dev)
    zeros = torch.zeros(n, dtype=torch.int32, device=dev)
    assert ops.prf1a_counts(ones, ones) == (n, 0, 0, 0)
    assert ops.prf1a_counts(zeros, zeros) == (0, 0, n, 0)
    assert ops.prf1a_counts(ones, zeros) == (0, n, 0, 0)
    assert ops.prf1a_counts(zeros, ones) == (0, 0, 0, n)


def test_metrics_reject_numel_mismatch(dev):
    a = torch.zeros(64, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match='same numel'):
        ops.prf1a_counts(a, a[:63])
    with pytest.raises(RuntimeError, match='same numel'):
        ops.prf1a_counts(a[:63], a)
    with pytest.raises(RuntimeError, match='same numel'):
        ops.confusion_matrix(a, a[:63], 3)
    with pytest.raises(RuntimeError, match='same numel'):
        ops.confusion_matrix(a[:63], a, 3)
    with pytest.raises(RuntimeError, match='too large'):
        ops.confusion_matrix(a, a, fc.CONF_TOO_LARGE)
    _launches_ok(dev)


@pytest.mark.parametrize('dtype', [torch.int64, torch.int32, torch.uint8],
                         ids=str)
@pytest.mark.parametrize('K', fc.CONF_KS)
def test_confusion_matrix(dev, K, dtype):
    """K >= 129 asks for more than 64 KB of dynamic LDS."""
    g = fc.gen(K)
    lo, hi = (0, min(K + 3, 256)) if dtype == torch.uint8 else (-2, K + 3)
    pred = torch.randint(lo, hi, (fc.CONF_N,), generator=g).to(dtype)
    true = torch.randint(lo, hi, (fc.CONF_N,), generator=g).to(dtype)
    ref = fc.confusion_ref(pred, true, K)
    assert ref.sum() > 0
    mat = ops.confusion_matrix(pred.to(dev), true.to(dev), K)
    assert mat.dtype == torch.int64 and torch.equal(mat.cpu(), ref)
    empty = ops.confusion_matrix(pred[:0].to(dev), true[:0].to(dev), K)
    assert torch.equal(empty.cpu(), torch.zeros(K, K, dtype=torch.int64))


@pytest.mark.parametrize('K', [128, 129])
def test_seg_confusion_matrix_past_64k_lds(dev, K):
    g = fc.gen(K)
    logits = torch.randn(1, K, 4, 4, 4, generator=g)
    true = torch.randint(0, K, (1, 4, 4, 4), generator=g)
    pred = ops.argmax_lowest(logits)
    ref = fc.confusion_ref(pred, true, K)
    assert ref.sum() == 64
    mat = ops.seg_confusion_matrix(logits.to(dev), true.to(dev), K)
    assert torch.equal(mat.cpu(), ref)


# ---------------------------------------------------------------- pack/unpack
def _pack_case(name, dev):
    g = fc.gen(len(name))
    cpu = [torch.randn(s, generator=g) for s in fc.PACK_LISTS[name]]
    return cpu, [t.to(dev) for t in cpu], sum(t.numel() for t in cpu)


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('name', list(fc.PACK_LISTS))
def test_pack_tensors(dev, name, offset):
    cpu, tensors, total = _pack_case(name, dev)
    base = torch.full((total + offset + 1,), fc.PACK_SENTINEL, device=dev)
    flat = base[offset:offset + total]
    C.pack_tensors(tensors, flat)
    expect = torch.full((total + offset + 1,), fc.PACK_SENTINEL)
    expect[offset:offset + total] = torch.cat(
        [t.reshape(-1) for t in cpu] + [torch.empty(0)])
    assert torch.equal(base.cpu(), expect)
    _launches_ok(dev)


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('name', list(fc.PACK_LISTS))
def test_unpack_tensors_leaves_guards(dev, name, offset):
    cpu, _, total = _pack_case(name, dev)
    flat_cpu = torch.cat([t.reshape(-1) for t in cpu] + [torch.empty(0)])
    flat = torch.zeros(total + offset, device=dev)[offset:]
    flat.copy_(flat_cpu)
    G = fc.PACK_GUARD
    size = G + sum(t.numel() + G for t in cpu)
    buf = torch.full((size,), fc.PACK_SENTINEL, device=dev)
    expect = torch.full((size,), fc.PACK_SENTINEL)
    dsts, at = [], G
    for t in cpu:
        dsts.append(buf[at:at + t.numel()].view(t.shape))
        expect[at:at + t.numel()] = t.reshape(-1)
        at += t.numel() + G
    C.unpack_tensors(flat, dsts)
    assert torch.equal(buf.cpu(), expect)
    if cpu:
        for src, dst in zip(torch.split(flat_cpu, [t.numel() for t in cpu]),
                            dsts):
            assert torch.equal(dst.cpu().reshape(-1), src)
    _launches_ok(dev)


def test_pack_unpack_reject_bad_arguments(dev):
    tensors = [torch.ones(17, device=dev), torch.ones(5, 5, device=dev)]
    for n in (41, 43):      # the tensors hold 42
        flat = torch.full((n,), fc.PACK_SENTINEL, device=dev)
        with pytest.raises(RuntimeError, match='flat buffer holds'):
            C.pack_tensors(tensors, flat)
        with pytest.raises(RuntimeError, match='flat buffer holds'):
            C.unpack_tensors(flat, tensors)
        assert bool((flat == fc.PACK_SENTINEL).all())
    assert all(bool((t == 1).all()) for t in tensors)
    flat = torch.zeros(42, device=dev)
    half = [tensors[0].half(), tensors[1]]
    strided = [torch.ones(34, device=dev)[::2], tensors[1]]
    for bad in (half, strided):
        with pytest.raises(RuntimeError, match='contiguous fp32'):
            C.pack_tensors(bad, flat)
        with pytest.raises(RuntimeError, match='contiguous fp32'):
            C.unpack_tensors(flat, bad)
    with pytest.raises(RuntimeError):
        C.pack_tensors([], torch.zeros(1, device=dev))
    _launches_ok(dev)


# --------------------------------------------------------------------- linear
def _dev_inputs(M, N, K, dtype, dev):
    x, w, b, go = fc.linear_inputs(M, N, K, dtype)
    b = b.to(dtype).float()     # the same bias for the kernel and torch
    return (x, w, b, go), tuple(t.to(dev) for t in (x, w, b, go))


@pytest.mark.parametrize('dtype', fc.LINEAR_DTYPES, ids=str)
@pytest.mark.parametrize('M,N,K', fc.LINEAR_SHAPES)
def test_linear_kernels_at_tile_edges(dev, M, N, K, dtype):
    (x, w, b, go), (xd, wd, bd, god) = _dev_inputs(M, N, K, dtype, dev)
    name = str(dtype).split('.')[-1]
    none = torch.empty(0, device=dev)
    soft = Soft()
    for bias, relu in [(None, False), (b, False), (b, True)]:
        out = C.linear_fwd(xd, wd, none if bias is None else bd, relu)
        assert out.dtype == dtype and out.shape == (M, N)
        tor = F.linear(xd, wd, None if bias is None else bd.to(dtype))
        soft.check(f'linear_fwd_{name}',
                   f'M={M} N={N} K={K} bias={bias is not None} relu={relu}',
                   out, torch.relu(tor) if relu else tor,
                   fc.linear_ref(x, w, bias, relu))
    gx = C.linear_dgrad(god, wd)
    assert gx.dtype == dtype and gx.shape == (M, K)
    soft.check(f'linear_dgrad_{name}', f'M={M} N={N} K={K}', gx, god @ wd,
               fc.dgrad_ref(go, w))
    gw = C.linear_wgrad(god, xd)
    assert gw.dtype == torch.float32 and gw.shape == (N, K)
    soft.check(f'linear_wgrad_{name}', f'M={M} N={N} K={K}', gw,
               god.t() @ xd, fc.wgrad_ref(go, x))
    soft.done()


@pytest.mark.parametrize('dtype', fc.LINEAR_DTYPES, ids=str)
@pytest.mark.parametrize('M,N,K', fc.SPLITK_SHAPES)
def test_linear_wgrad_split_k(dev, M, N, K, dtype):
    """The contraction splits over grid.z and folds by atomics for M > 64."""
    (x, w, b, go), (xd, wd, bd, god) = _dev_inputs(M, N, K, dtype, dev)
    name = str(dtype).split('.')[-1]
    gw = C.linear_wgrad(god, xd)
    assert gw.dtype == torch.float32
    fc.check(f'linear_wgrad_{name}', f'split-K M={M} N={N} K={K}', gw,
             god.t() @ xd, fc.wgrad_ref(go, x))


def test_linear_autograd_relu_mask_at_exact_zero(dev):
    """Small integers make every product exact, so some pre-activations are
    exactly 0: like torch, ReLU passes no gradient there. x is a transposed
    (non-contiguous) view."""
    g = fc.gen(4)
    M, N, K = 70, 9, 5
    xt = torch.randint(-2, 3, (K, M), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float()
    b = torch.randint(-2, 3, (N,), generator=g).float()
    go = torch.randint(-3, 4, (M, N), generator=g).float()
    pre = fc.linear_ref(xt.t(), w, b)
    assert (pre == 0).any() and (pre > 0).any() and (pre < 0).any()
    masked = go.double() * (pre > 0)
    refs = [pre.clamp_min(0), (masked @ w.double()).t(),
            masked.t() @ xt.t().double(), masked.sum(0)]

    def run(fn):
        leaves = [t.to(dev).requires_grad_(True) for t in (xt, w, b)]
        x = leaves[0].t()
        assert not x.is_contiguous()
        out = fn(x, leaves[1], leaves[2])
        out.backward(go.to(dev))
        return [out.detach()] + [t.grad for t in leaves]

    got = run(lambda x, w_, b_: ops.linear(x, w_, b_, relu=True))
    tor = run(lambda x, w_, b_: torch.relu(F.linear(x, w_, b_)))
    soft = Soft()
    for what, a, t, r in zip(('out', 'gx', 'gw', 'gb'), got, tor, refs):
        soft.check('linear_autograd', f'relu mask {what}', a, t, r)
    soft.done()


def test_linear_empty_batch(dev):
    N, K = 33, 17
    w = torch.randn(N, K, device=dev)
    b = torch.randn(N, device=dev)
    x0, go0 = torch.empty(0, K, device=dev), torch.empty(0, N, device=dev)
    assert C.linear_fwd(x0, w, b, True).shape == (0, N)
    assert C.linear_dgrad(go0, w).shape == (0, K)
    gw = C.linear_wgrad(go0, x0)
    assert gw.shape == (N, K) and gw.dtype == torch.float32
    assert not gw.any()
    assert torch.equal(C.colsum(go0), torch.zeros(N, device=dev))
    wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xl = x0.clone().requires_grad_(True)
    out = ops.linear(xl, wl, bl, relu=True)
    out.sum().backward()
    assert out.shape == (0, N) and xl.grad.shape == (0, K)
    assert not wl.grad.any() and not bl.grad.any()
    _launches_ok(dev)


def test_linear_rejects_3d_input(dev):
    w = torch.randn(4, 6, device=dev)
    x = torch.randn(2, 6, 6, device=dev)      # size(1) == K passes the K check
    with pytest.raises(RuntimeError, match=r'must be \[M, K\]'):
        ops.linear(x, w)
    with pytest.raises(RuntimeError, match=r'\[M, N\]'):
        C.linear_dgrad(torch.randn(2, 3, 4, device=dev), w)
    with pytest.raises(RuntimeError, match=r'\[M, N\]'):
        C.linear_wgrad(torch.randn(2, 3, 4, device=dev), x)


@pytest.mark.parametrize('dtype', fc.LINEAR_DTYPES, ids=str)
@pytest.mark.parametrize('M,N', fc.COLSUM_SHAPES)
def test_colsum(dev, M, N, dtype):
    g = torch.randn(M, N, generator=fc.gen(M + N)).to(dtype)
    out = C.colsum(g.to(dev))
    assert out.dtype == torch.float32 and out.shape == (N,)
    fc.check(f'colsum_{str(dtype).split(".")[-1]}', f'M={M} N={N}', out,
             g.to(dev).sum(0), fc.colsum_ref(g))


@pytest.mark.parametrize('n,r', fc.GS_SHAPES)
def test_gram_schmidt(dev, n, r):
    a = torch.randn(n, r, generator=fc.gen(n + r))
    ref = fc.gram_schmidt_ref(a)
    q = a.to(dev)
    C.gram_schmidt(q, fc.GS_EPS)
    qt = fc.gram_schmidt_torch(a.to(dev))
    soft = Soft()
    soft.check('gram_schmidt', f'n={n} r={r} Q', q, qt, ref)
    eye = torch.eye(r, dtype=torch.float64)
    qd, qtd = q.double().cpu(), qt.double().cpu()
    # ||Q^T Q - I|| of the kernel's Q against that of torch's Q
    soft.check('gram_schmidt_orth', f'n={n} r={r}',
               qd.t() @ qd, qtd.t() @ qtd, eye, out_dtype=torch.float32)
    soft.done()


@pytest.mark.parametrize('r,zero', [(2, 0), (4, 1), (4, 3)])
def test_gram_schmidt_zero_column_stays_zero(dev, r, zero):
    a = torch.randn(257, r, generator=fc.gen(r + zero))
    a[:, zero] = 0
    ref = fc.gram_schmidt_ref(a)
    q = a.to(dev)
    C.gram_schmidt(q, fc.GS_EPS)
    assert bool(torch.isfinite(q).all()) and not bool(q[:, zero].any())
    fc.check('gram_schmidt', f'zero column {zero} of {r}', q,
             fc.gram_schmidt_torch(a.to(dev)), ref)
