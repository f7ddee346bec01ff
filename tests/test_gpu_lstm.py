"""ops.OpsLSTM (ops/csrc/lstm.hip) and models.ICALstm against float64 CPU
copies holding the same bf16-rounded weights and inputs.

Bound. A recurrence has no tolerance elsewhere in this suite, so it is set by
a yardstick: the stock CPU module run in bfloat16 on the same case, compared
with the same float64 result. That computation rounds every intermediate to
bf16; the kernels round only the MFMA operands (h, dG, W_hh) and keep c, the
gates, the pre-activations and the accumulators in fp32. Per tensor the
native path may have at most 2x the yardstick's max abs error (the factor
allows another summation order over the same operand rounding). Every ratio
is printed; profiles/lstm_ab.md records them.

Cases (T, B, I, H, layers, bidirectional): a single step with H padded
40 -> 64 and a batch tail; the smallest Hp with two batch tiles (tail of one
row) and both directions; the largest register-stationary instance with odd
I; a streamed, padded instance (160 -> 192); the largest streamed instance;
two layers (layer 2 reads 2H inputs); 64 steps for LDS buffer parity and
drift."""
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    from coinstac_dinunet_amd.models import ICALstm

CASES = [(1, 3, 24, 40, 1, False),
         (7, 17, 24, 32, 1, True),
         (6, 16, 33, 128, 1, True),
         (5, 5, 20, 160, 1, False),
         (4, 2, 16, 256, 1, True),
         (6, 4, 16, 48, 2, True),
         (64, 2, 8, 32, 1, False)]
ICA = 'ica'   # ICALstm at B = 3, S = 5, 8 components, window 4, H = 32


@functools.lru_cache(maxsize=None)
def run(case, dtype, device, hx=False, batch_first=False, bf16_x=False):
    """Forward and backward of one case in `dtype` on `device` (the native
    module on 'cuda', the stock one on 'cpu'): {name: float64 CPU tensor} of
    the outputs and of the gradients of sum(output * fixed cotangent)."""
    gen = torch.Generator().manual_seed(7)

    def rand(*shape, grad=True):
        v = torch.randn(*shape, generator=gen).bfloat16()
        return v.to(dtype).to(device).requires_grad_(grad)

    torch.manual_seed(11)
    state = None
    if case == ICA:
        mod = ICALstm(num_comps=8, window_size=4, input_size=16,
                      hidden_size=32)
        x = rand(3, 5, 8, 4)
    else:
        T, B, I, H, layers, bidir = case
        cls = ops.OpsLSTM if device == 'cuda' else nn.LSTM
        mod = cls(I, H, num_layers=layers, bidirectional=bidir,
                  batch_first=batch_first)
        x = rand(B, T, I) if batch_first else rand(T, B, I)
        if hx:
            n = layers * (2 if bidir else 1)
            state = (rand(n, B, H), rand(n, B, H))
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(p.bfloat16())
    mod = mod.to(device=device, dtype=dtype)
    xin = x.bfloat16() if bf16_x and device == 'cuda' else x
    if case == ICA:
        out = {'logits': mod(xin)}
    else:
        y, (h, c) = mod(xin, state)
        out = {'y': y, 'h_T': h, 'c_T': c}
    sum((v.to(dtype) * rand(*v.shape, grad=False)).sum()
        for v in out.values()).backward()
    out['dx'] = x.grad
    if state is not None:
        out['dh0'], out['dc0'] = state[0].grad, state[1].grad
    for name, p in mod.named_parameters():
        out['d' + name] = p.grad
    return {k: v.detach().double().cpu() for k, v in out.items()}


@pytest.mark.parametrize('case,kw', [(c, {}) for c in CASES] + [
    (CASES[1], {'hx': True}),
    (CASES[3], {'hx': True}),
    (CASES[2], {'bf16_x': True}),
    (CASES[5], {'batch_first': True}),
    (ICA, {})], ids=str)
def test_lstm_matches_float64(case, kw):
    cpu_kw = {k: v for k, v in kw.items() if k != 'bf16_x'}
    ref = run(case, torch.float64, 'cpu', **cpu_kw)
    yard = run(case, torch.bfloat16, 'cpu', **cpu_kw)
    got = run(case, torch.float32, 'cuda', **kw)
    assert got.keys() == ref.keys()
    if kw.get('hx'):
        assert 'dh0' in got and 'dc0' in got
    worst = []
    for name, r in ref.items():
        assert got[name].shape == r.shape, name
        assert torch.isfinite(got[name]).all(), name
        err = (got[name] - r).abs().max().item()
        bound = (yard[name] - r).abs().max().item()
        print(f'lstm {case} {kw} {name}: err={err:.3e} yardstick={bound:.3e} '
              f'ratio={err / bound if bound else float(err > 0):.3f}')
        if err > 2 * bound:
            worst.append((name, err, bound))
    assert not worst, f'beyond 2x the bf16 yardstick: {worst}'


def test_lstm_forward_is_bit_identical():
    first = run(CASES[2], torch.float32, 'cuda')['y']
    again = run.__wrapped__(CASES[2], torch.float32, 'cuda')['y']   # uncached
    assert torch.equal(first, again)
