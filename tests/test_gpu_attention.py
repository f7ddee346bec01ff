"""ops.attention (ops/csrc/attention.hip), ops.OpsMultiheadAttention and
models.ICATransformer against float64 CPU copies of the same bf16-rounded
inputs and weights.

Reference: the plain chain (matmul, scale, masked_fill, softmax, matmul) in
float64 on the CPU. Yardstick: the same chain in bfloat16 on the CPU. Bound,
as in test_gpu_lstm.py: per tensor the native path's max abs error against
float64 may be at most 2x the yardstick's (the same operand rounding in
another summation order); every yardstick must be > 0. Every ratio is
printed; profiles/attention_ab.md records them.

Cases (B, heads, Tq, Tk, Dh, causal, mask, q_scale), what each catches:
one partial tile on both axes; a second wave's row tail with batch and head
strides; two query and three key tiles with tails (cross attention); exact
tiles at the widest instance; Dh zero-filled 24 -> 32; the causal diagonal
tile and the skipped ones; two wholly masked key tiles and a mask tail; an
almost wholly masked tile with holes; scores of +-100."""
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    from coinstac_dinunet_amd.models import ICATransformer

CASES = [(1, 1, 3, 5, 32, False, None, 1),
         (2, 3, 17, 17, 32, False, None, 1),
         (1, 2, 65, 130, 64, False, None, 1),
         (2, 2, 64, 64, 128, False, None, 1),
         (1, 2, 40, 40, 24, False, None, 1),
         (2, 2, 70, 70, 32, True, None, 1),
         (2, 2, 33, 130, 64, False, 'lengths', 1),
         (1, 2, 20, 70, 32, False, 'holes', 1),
         (1, 1, 17, 70, 32, False, None, 16)]
PACKED = (1, 2, 65, 65, 64, False, 'packed', 1)
DEAD = (2, 3, 17, 17, 32, False, 'dead', 1)


def key_mask(kind, B, Tk):
    if kind in (None, 'packed'):
        return None
    k = torch.arange(Tk)
    if kind == 'lengths':
        return k[None] >= torch.tensor([3, 97])[:, None]
    if kind == 'holes':
        return (((k < 64) & (k != 5)) | ((k >= 64) & (k % 3 == 0)))[None]
    return torch.tensor([False, True])[:, None].expand(B, Tk)   # 'dead'


def chain(q, k, v, mask, causal):
    s = (q @ k.transpose(-1, -2)) * q.shape[-1] ** -0.5
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float('-inf'))
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(1),
                          float('-inf'))
    return torch.softmax(s, -1) @ v


@functools.lru_cache(maxsize=None)
def run(case, dtype, device):
    """{out, dq, dk, dv} as float64 CPU tensors: ops.attention on 'cuda',
    the chain on 'cpu', from the same seeded bf16-rounded draws."""
    B, H, Tq, Tk, Dh, causal, kind, q_scale = case
    gen = torch.Generator().manual_seed(5)

    def rand(T):
        return torch.randn(B, H, T, Dh, generator=gen).bfloat16()
    q, k, v, go = rand(Tq) * q_scale, rand(Tk), rand(Tk), rand(Tq)
    mask = key_mask(kind, B, Tk)
    q, k, v = (t.to(dtype).to(device).requires_grad_() for t in (q, k, v))
    if device == 'cpu':
        out = chain(q, k, v, mask, causal)
    else:
        a, b, c = q, k, v
        if kind == 'packed':   # views of [B, T, 3, heads, Dh], as the module
            packed = torch.stack([q, k, v], 1).permute(0, 3, 1, 2, 4)
            a, b, c = packed.contiguous().permute(0, 3, 2, 1, 4).unbind(2)
            assert not a.is_contiguous() and a.stride(-1) == 1
        out = ops.attention(a, b, c, None if mask is None else mask.cuda(),
                            causal)
        assert out.dtype == dtype and out.shape == (B, H, Tq, Dh)
    (out * go.to(dtype).to(device)).sum().backward()
    res = {'out': out, 'dq': q.grad, 'dk': k.grad, 'dv': v.grad}
    return {n: t.detach().double().cpu() for n, t in res.items()}


def check(tag, got, ref, yard, rows=slice(None)):
    worst = []
    for name, r in ref.items():
        g, r, y = got[name][rows], r[rows], yard[name][rows]
        assert g.shape == r.shape and torch.isfinite(g).all(), name
        err = (g - r).abs().max().item()
        bound = (y - r).abs().max().item()
        assert bound > 0, f'{name}: vacuous yardstick'
        print(f'attention {tag} {name}: err={err:.3e} yardstick={bound:.3e} '
              f'ratio={err / bound:.3f}')
        if err > 2 * bound:
            worst.append((name, err, bound))
    assert not worst, f'beyond 2x the bf16 yardstick: {worst}'


@pytest.mark.parametrize('case,dtype', [(c, torch.float32) for c in CASES] + [
    (PACKED, torch.float32), (CASES[3], torch.bfloat16)], ids=str)
def test_attention_matches_float64(case, dtype):
    check((case, dtype), run(case, dtype, 'cuda'),
          run(case, torch.float64, 'cpu'), run(case, torch.bfloat16, 'cpu'))


def test_fully_masked_rows_are_zero():
    got = run(DEAD, torch.float32, 'cuda')
    for name, g in got.items():
        assert (g[1] == 0).all(), name
    check(DEAD, got, run(DEAD, torch.float64, 'cpu'),
          run(DEAD, torch.bfloat16, 'cpu'), rows=slice(0, 1))


def test_attention_is_bit_identical():
    first = run(CASES[2], torch.float32, 'cuda')
    again = run.__wrapped__(CASES[2], torch.float32, 'cuda')   # uncached
    for name in first:
        assert torch.equal(first[name], again[name]), name


@functools.lru_cache(maxsize=None)
def run_module(kind, dtype, device):
    """Forward and backward of the module ('mha') or the model ('ica')."""
    gen = torch.Generator().manual_seed(9)
    torch.manual_seed(13)
    if kind == 'mha':
        cls = ops.OpsMultiheadAttention if device == 'cuda' \
            else nn.MultiheadAttention
        mod = cls(64, 4, batch_first=True)
        x = torch.randn(2, 19, 64, generator=gen)
        pad = torch.arange(19)[None] >= torch.tensor([19, 7])[:, None]
    else:
        mod = ICATransformer(num_comps=8, window_size=4, embed_dim=32,
                             num_heads=2, num_layers=2)
        x = torch.randn(3, 5, 8, 4, generator=gen)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(p.bfloat16())
    mod = mod.to(device=device, dtype=dtype)
    x = x.bfloat16().to(dtype).to(device).requires_grad_()
    if kind == 'mha':
        out, weights = mod(x, x, x, key_padding_mask=pad.to(device),
                           need_weights=False)
        assert weights is None
    else:
        out = mod(x, torch.tensor([5, 2, 4]))
    go = torch.randn(out.shape, generator=gen).bfloat16()
    (out * go.to(dtype).to(device)).sum().backward()
    res = {'out': out, 'dx': x.grad}
    if kind == 'mha':
        res.update(('d' + n, p.grad) for n, p in mod.named_parameters())
    return {n: t.detach().double().cpu() for n, t in res.items()}


@pytest.mark.parametrize('kind', ['mha', 'ica'])
def test_module_matches_float64(kind):
    check(kind, run_module(kind, torch.float32, 'cuda'),
          run_module(kind, torch.float64, 'cpu'),
          run_module(kind, torch.bfloat16, 'cpu'))


def test_need_weights_takes_the_library_path():
    mod = ops.OpsMultiheadAttention(64, 4, batch_first=True).cuda()
    x = torch.randn(2, 6, 64, device='cuda')
    out, weights = mod(x, x, x, need_weights=True)
    assert out.shape == (2, 6, 64) and weights.shape == (2, 6, 6)
