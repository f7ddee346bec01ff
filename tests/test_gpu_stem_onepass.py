"""First layer (Cin = 1): epilogue BN statistics on the single-channel
forward instances, the one-pass BN-backward + wgrad kernel, and the stem
autograd node that uses both (MI355X).

The one-pass op is checked against an fp64 evaluation of

    d  = dz * [gamma*xhat + beta > 0],  xhat = (x1 - mean) * rstd
    go = gamma*rstd*(d - sum(d)/n - xhat*sum(d*xhat)/n)
    dw = sum go * x_in(tap),  dgamma = sum d*xhat,  dbeta = sum d

on the same bf16 inputs, next to the composed path (bn3d_bwd, which rounds
go to bf16, then conv3d_wgrad). The ReLU mask of the reference is the fp32
expression both kernels evaluate, so the comparison is about the sums.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    C = ops.require_native()

DEV = 'cuda:0'


# ---- A: forward + epilogue statistics --------------------------------------
# (N, Cout, D, H, W)
FWD_CASES = [
    (2, 32, 3, 16, 32),   # two row tiles
    (1, 40, 3, 12, 32),   # ragged row tile and ragged column tile
    (1, 16, 2, 16, 16),   # OWT 16
    (1, 32, 3, 8, 24),    # OWT 8
    (1, 32, 2, 8, 8),     # chunk-64 instance
]


@pytest.mark.parametrize('case', FWD_CASES)
def test_ci1_forward_stats(case):
    N, Co, D, H, W = case
    torch.manual_seed(7)
    x = (torch.randn(N, 1, D, H, W, device=DEV) + 0.5).bfloat16()
    w = (torch.randn(Co, 1, 3, 3, 3, device=DEV) * 0.3).bfloat16()
    plain = C.conv3d_fwd_spatial(x, w, 1, 1)
    out, stats = C.conv3d_fwd_ci1_stats(x, w)
    assert torch.equal(out, plain)
    assert stats.shape == (64, Co, 2)
    sums = stats.sum(0)
    o = out.float()
    # rows and columns past the tensor must not be counted
    torch.testing.assert_close(sums[:, 0], o.sum(dim=(0, 2, 3, 4)),
                               rtol=1e-3, atol=1e-1)
    torch.testing.assert_close(sums[:, 1], (o * o).sum(dim=(0, 2, 3, 4)),
                               rtol=1e-3, atol=1e-1)


# ---- B: one-pass BN-backward + wgrad ----------------------------------------
# (N, Cout, D, H, W)
BWD_CASES = [
    (2, 32, 3, 8, 32),       # base
    (1, 32, 5, 12, 32),      # odd depth, H no multiple of 8
    (2, 32, 2, 8, 64),       # wide rows (two 32-m steps per item)
    (3, 40, 4, 8, 32),       # ragged second channel tile
    (1, 16, 2, 8, 32),       # half-empty channel tile
    (16, 32, 32, 32, 32),    # n = 524288 per channel: the fold matters
]
MASKED = 2      # channel with beta = -10: every position masked
NEGATIVE = 1    # channel with gamma < 0


def _problem(case, x_mean):
    N, Co, D, H, W = case
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 + N * 131 + Co * 17 + D * 5 + H + W + int(x_mean))
    x_in = (torch.randn(N, 1, D, H, W, device=DEV, generator=g)
            + x_mean).bfloat16()
    w = (torch.randn(Co, 1, 3, 3, 3, device=DEV, generator=g)
         * 0.2).bfloat16()
    x1 = C.conv3d_fwd_spatial(x_in, w, 1, 1) if W % 8 == 0 and H * W >= 64 \
        else C.conv3d_fwd(x_in, w, 1)
    dz = ((torch.randn(x1.shape, device=DEV, generator=g) + 0.2)
          * 0.1).bfloat16()
    gamma = torch.rand(Co, device=DEV, generator=g) + 0.5
    beta = torch.randn(Co, device=DEV, generator=g) * 0.1
    gamma[NEGATIVE] = -0.7
    gamma[MASKED] = 0.5
    beta[MASKED] = -10.0
    xf = x1.float()
    mean = xf.mean(dim=(0, 2, 3, 4))
    var = xf.var(dim=(0, 2, 3, 4), unbiased=False)
    mean_rstd = torch.stack([mean, torch.rsqrt(var + 1e-5)], 1).contiguous()
    return x_in, dz, x1, mean_rstd, gamma, beta


def _reference(x_in, dz, x1, mean_rstd, gamma, beta):
    """fp64 (dw, dgamma, dbeta) of the formulas in the module docstring."""
    v = (1, -1, 1, 1, 1)
    mean32, rstd32 = mean_rstd[:, 0].view(v), mean_rstd[:, 1].view(v)
    # the mask as the kernels form it, in fp32
    z = gamma.view(v) * ((x1.float() - mean32) * rstd32) + beta.view(v)
    keep = ~(z <= 0)
    del z
    mean, rstd = mean32.double(), rstd32.double()
    d = dz.double() * keep
    xh = (x1.double() - mean) * rstd
    n = d.numel() // d.size(1)
    s = d.sum(dim=(0, 2, 3, 4))
    sx = (d * xh).sum(dim=(0, 2, 3, 4))
    go = gamma.double().view(v) * rstd * (d - s.view(v) / n
                                           - xh * sx.view(v) / n)
    del d, xh
    N, _, D, H, W = x_in.shape
    xp = torch.nn.functional.pad(x_in.double(), (1, 1, 1, 1, 1, 1))
    dw = torch.empty(go.size(1), 27, device=go.device, dtype=torch.float64)
    for tap in range(27):
        kd, kh, kw = tap // 9, (tap // 3) % 3, tap % 3
        xs = xp[:, :, kd:kd + D, kh:kh + H, kw:kw + W]
        dw[:, tap] = (go * xs).sum(dim=(0, 2, 3, 4))
    return dw.view(-1, 1, 3, 3, 3), sx, s


def _composed(x_in, dz, x1, mean_rstd, gamma, beta):
    dx, dgamma, dbeta = C.bn3d_bwd(dz, x1, mean_rstd, gamma, beta, True)
    return C.conv3d_wgrad(x_in, dx, 1), dgamma, dbeta


@pytest.mark.parametrize('x_mean', [0.0, 3.0])
@pytest.mark.parametrize('case', BWD_CASES)
def test_onepass_backward(case, x_mean):
    assert C.conv3d_wgrad_ci1_bn_fits(case[3], case[4])
    prob = _problem(case, x_mean)
    dw_r, dg_r, db_r = _reference(*prob)
    dw_c, dg_c, db_c = _composed(*prob)
    dw, dg, db = C.conv3d_wgrad_ci1_bn(*prob)
    dw2, dg2, db2 = C.conv3d_wgrad_ci1_bn(*prob)
    assert dw.shape == dw_c.shape and dw.dtype == torch.float32

    def err(a, ref):
        return (a.double() - ref).abs().max().item()

    e_dw, e_dw_c = err(dw, dw_r), err(dw_c, dw_r)
    e_dg, e_dg_c = err(dg, dg_r), err(dg_c, dg_r)
    e_db, e_db_c = err(db, db_r), err(db_c, db_r)
    print(f'onepass {case} x_mean={x_mean}: dw err {e_dw:.3g} '
          f'(composed {e_dw_c:.3g}, max|ref| {dw_r.abs().max().item():.3g})'
          f' dgamma {e_dg:.3g} ({e_dg_c:.3g}) dbeta {e_db:.3g} ({e_db_c:.3g})')
    assert e_dw <= 1.5 * e_dw_c
    assert e_dg <= max(4 * e_dg_c, 1e-5 * dg_r.abs().max().item())
    assert e_db <= max(4 * e_db_c, 1e-5 * db_r.abs().max().item())
    # the fully masked channel contributes nothing at all
    assert (dw[MASKED] == 0).all() and dg[MASKED] == 0 and db[MASKED] == 0
    # plain stores and a fixed fold order: run to run bitwise
    assert torch.equal(dw, dw2) and torch.equal(dg, dg2) \
        and torch.equal(db, db2)


def test_onepass_backward_fallback_is_composed():
    """OW % 32 != 0 runs bn3d_bwd then conv3d_wgrad. dgamma and dbeta (two
    atomic addends per channel: order-free) are bitwise the composed path's.
    dw cannot be bitwise: at this shape conv3d_wgrad takes the split-K igemm
    (M = 768 positions, chunk = 128, 6 chunks per output element), each
    chunk's fp32 partial p_i is deterministic, and the 6 are folded with fp32
    atomics in whatever order the blocks retire. Two orders of the same 6
    addends differ by at most 2 * 5 * 2^-24 * sum|p_i| (5 roundings each,
    every intermediate bounded by sum|p_i|). The partials are evaluated here
    in fp64 from the composed path's own bf16 dx, which is bitwise what the
    fallback feeds to conv3d_wgrad; 1e-6 * sum|p_i| is added for their own
    fp32 accumulation in the kernel (deterministic, but the fp64 stand-in
    does not have it)."""
    case = (2, 32, 3, 8, 16)
    N, Co, D, H, W = case
    assert not C.conv3d_wgrad_ci1_bn_fits(H, W)
    prob = _problem(case, 3.0)
    x_in, dz, x1, mean_rstd, gamma, beta = prob
    dx_c, dg_c, db_c = C.bn3d_bwd(dz, x1, mean_rstd, gamma, beta, True)
    dw_c = C.conv3d_wgrad(x_in, dx_c, 1)
    dw, dg, db = C.conv3d_wgrad_ci1_bn(*prob)
    assert torch.equal(dg, dg_c) and torch.equal(db, db_c)

    M, chunk = N * D * H * W, 128
    assert M % chunk == 0 and M // chunk == 6
    xp = torch.nn.functional.pad(x_in.double(), (1, 1, 1, 1, 1, 1))
    go = dx_c.double().permute(1, 0, 2, 3, 4).reshape(Co, M)
    sum_abs_p = torch.empty(Co, 27, device=DEV, dtype=torch.float64)
    for tap in range(27):
        kd, kh, kw = tap // 9, (tap // 3) % 3, tap % 3
        xs = xp[:, 0, kd:kd + D, kh:kh + H, kw:kw + W].reshape(1, M)
        parts = (go * xs).view(Co, M // chunk, chunk).sum(-1)
        sum_abs_p[:, tap] = parts.abs().sum(-1)
    bound = (10 * 2.0 ** -24 + 1e-6) * sum_abs_p
    diff = (dw.double() - dw_c.double()).abs().view(Co, 27)
    print(f'fallback vs composed: max diff {diff.max().item():.3g}, '
          f'bound at that element '
          f'{bound.view(-1)[diff.argmax()].item():.3g}, '
          f'max|dw| {dw_c.abs().max().item():.3g}')
    assert (diff <= bound).all()


# ---- C: the stem node end to end --------------------------------------------
def _step(net, x, y):
    for p in net.parameters():
        if p.grad is None:
            p.grad = torch.zeros_like(p, dtype=torch.float32)
        p.grad.zero_()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = net(x)
    loss = ops.cross_entropy(out.float(), y)
    loss.backward()
    return out, loss


def _stem_net(seed):
    from coinstac_dinunet_amd.models import VBMNet
    torch.manual_seed(seed)
    net = VBMNet(in_channels=1, num_class=2, widths=(32, 32)).to(DEV)
    x = torch.randn(2, 1, 32, 32, 32, device=DEV)
    return net, x


# positions per channel behind each BN of VBMNet(widths=(32, 32)) on 2 x 32^3
_BN_POSITIONS = {0: 2 * 32 ** 3, 1: 2 * 32 ** 3, 2: 2 * 16 ** 3, 3: 2 * 16 ** 3}


def _check_running_buffers(bufs_a, bufs_b, label, steps=1):
    """Running buffers of two arms that started from the initial state (mean
    0, var 1) and took `steps` steps on one batch: running = (1 - w) * init +
    w * batch with w = 1 - 0.9^steps ("momentum" below is w).

    bn0 sees bitwise the same x1 in both arms; only the order of the fp32
    sums differs (epilogue atomics + finalize against bn_reduce). running_var
    is held elementwise to 1e-6 relative. A mean of n values is defined only
    to the rounding of sums of magnitude n * rms, so running_mean is held to
    1e-6 of momentum * rms(x1) per channel plus 1e-6 of itself; the rms comes
    from the running_var the same steps left.

    bn1..bn3 sit behind convs whose normalize-on-load affine (a, b) differs
    by an fp32 rounding between the arms, which flips bf16 roundings of single
    activations (one bf16 step, 2^-9 relative, random sign). If EVERY element
    of a channel moved by one such step, the batch mean would move by
    2^-9 * rms / sqrt(n) and the batch variance by 2^-8 * sqrt(3) * var /
    sqrt(n) (Gaussian fourth moment). The buffers are held to 8x that, times
    the momentum: 6e-5 * momentum * rms at n = 65536, 1.7e-4 at n = 8192
    (largest of 7 measured arm pairs: 0.12 of it, at bn3; any error in the
    update itself, a momentum, a count or an unbiasing factor, is 1e-2 or
    more of the buffer at these layers)."""
    for k in bufs_a:
        a, b = bufs_a[k], bufs_b[k]
        if k.endswith('num_batches_tracked'):
            assert torch.equal(a, b), f'{label} {k}'
            continue
        layer = int(k.split('.')[1])
        w = 1 - 0.9 ** steps
        n = _BN_POSITIONS[layer]
        rv = bufs_b[k.replace('running_mean', 'running_var')]
        var = ((rv - (1 - w)) / w).clamp_min(0)
        rms = torch.sqrt(var + (bufs_b[k.replace('running_var',
                                                 'running_mean')]
                                / w) ** 2)
        if layer == 0:
            bound = 1e-6 * (b.abs() + w * rms) \
                if k.endswith('running_mean') else 1e-6 * b.abs()
        elif k.endswith('running_mean'):
            bound = 8 * w * 2.0 ** -9 * rms / n ** 0.5
        else:
            bound = 8 * w * 2.0 ** -8 * 3 ** 0.5 * var / n ** 0.5
        diff = (a - b).abs()
        worst = (diff / bound.clamp_min(1e-30)).max().item()
        print(f'{label} {k}: max diff {diff.max().item():.3g}, '
              f'{worst:.3g} of the bound')
        assert (diff <= bound).all(), f'{label} {k}'


def test_stem_node_matches_plain_chain(monkeypatch):
    from coinstac_dinunet_amd.models import vbm
    from coinstac_dinunet_amd.ops import conv as convmod
    base, x = _stem_net(11)
    y = torch.tensor([0, 1], device=DEV)
    blocks = list(base.features)
    assert convmod.can_fuse_stem(blocks[0].conv, blocks[0].bn,
                                 blocks[1].conv, x)

    res = {}
    for fuse in (True, False):
        monkeypatch.setattr(vbm, '_FUSE_STEM', fuse)
        net = copy.deepcopy(base)
        out, loss = _step(net, x, y)
        res[fuse] = (out.float().detach().clone(), loss.detach().clone(),
                     [p.grad.clone() for p in net.parameters()],
                     {k: v.clone() for k, v in net.named_buffers()})
    out_f, loss_f, grads_f, bufs_f = res[True]
    out_u, loss_u, grads_u, bufs_u = res[False]
    # tolerances of test_fused_backward_matches_unfused (test_gpu_fusebn.py)
    m = x.numel() ** 0.5
    torch.testing.assert_close(out_f, out_u, rtol=5e-2, atol=2e-2)
    torch.testing.assert_close(loss_f, loss_u, rtol=5e-2, atol=2e-2)
    for (name, _), a, b in zip(base.named_parameters(), grads_f, grads_u):
        torch.testing.assert_close(a, b, rtol=5e-2, atol=5e-2 * m * 0.1,
                                   msg=lambda s, n=name: f'{n}: {s}')
        # that atol (1.28) is above most gradients of this step, so also:
        # no element further from the plain chain than 5e-2 of the
        # tensor's largest entry (a wrong sign or scale is 1 or more)
        scale = b.abs().max().item()
        diff = (a - b).abs().max().item()
        print(f'grad {name}: max|g| {scale:.3g}, max diff {diff:.3g}')
        assert diff <= 5e-2 * scale, name
    _check_running_buffers(bufs_f, bufs_u, 'stem vs plain')


def _rel_spread(runs):
    """Per output: largest |a - b| between two replays over max |a|."""
    out = []
    for tensors in zip(*runs):
        scale = max(t.abs().max().item() for t in tensors)
        d = max((tensors[i] - tensors[j]).abs().max().item()
                for i in range(len(tensors)) for j in range(i))
        out.append(d / scale if scale > 0 else d)
    return out


# Largest replay-to-replay spread measured for the PLAIN chain
# (COINN_FUSE_STEM=0) over 4 seeds x 6 replays on MI355X, as max|a - b| /
# max|a| per output (profiles/stem_onepass_ab.md). Its epilogue statistics
# and wgrad folds use fp32 atomics, so replays of the chain this change
# starts from are not bitwise equal: mostly the forward repeats exactly and
# the gradients move by 1e-4, and now and then a bf16 rounding flips in the
# forward (1 of the 4 seeds), which is what these figures are. The stem node
# measured 0 / 0 / 3.9e-4 in the same job and must stay within 4x of the
# plain chain's figures.
_PLAIN_REPLAY_SPREAD = {'logits': 2.56e-3, 'loss': 1.48e-4, 'grads': 5.15e-2}


def test_stem_node_graph_replays_agree(monkeypatch):
    from coinstac_dinunet_amd.models import vbm
    monkeypatch.setattr(vbm, '_FUSE_STEM', True)
    net, x = _stem_net(12)
    y = torch.tensor([1, 0], device=DEV)
    for _ in range(3):
        _step(net, x, y)
    eager = copy.deepcopy(net)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        out, loss = _step(net, x, y)
    runs = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        runs.append([out.float().clone(), loss.clone()]
                    + [p.grad.clone() for p in net.parameters()])
    assert all(torch.isfinite(r[1]).item() for r in runs)
    spread = _rel_spread(runs)
    print(f'replay spread: logits {spread[0]:.3g} loss {spread[1]:.3g} '
          f'grads max {max(spread[2:]):.3g}')
    assert spread[0] <= 4 * _PLAIN_REPLAY_SPREAD['logits']
    assert spread[1] <= 4 * _PLAIN_REPLAY_SPREAD['loss']
    assert max(spread[2:]) <= 4 * _PLAIN_REPLAY_SPREAD['grads']
    # the state three replays leave is the state three eager steps leave:
    # counters exactly, running buffers within the bounds between two arms
    for _ in range(3):
        _step(eager, x, y)   # the three replays above, for the counters
    for m in list(net.modules()) + list(eager.modules()):
        if hasattr(m, 'running_mean'):
            m.running_mean.zero_(), m.running_var.fill_(1.0)
    for _ in range(3):
        g.replay()
        _step(eager, x, y)
    torch.cuda.synchronize()
    _check_running_buffers(dict(net.named_buffers()),
                           dict(eager.named_buffers()), 'replay vs eager',
                           steps=3)


def test_onepass_backward_graph_replays_bitwise():
    """The one-pass op alone, captured: every replay must be bitwise the
    eager result. A partials buffer that a replay reuses while it is being
    read, or a fold that depends on launch order, shows up here."""
    prob = _problem((2, 32, 3, 8, 32), 3.0)
    ref = C.conv3d_wgrad_ci1_bn(*prob)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = C.conv3d_wgrad_ci1_bn(*prob)
    for _ in range(3):
        for t in got:
            t.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
