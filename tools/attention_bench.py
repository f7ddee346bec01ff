"""A/B of ops.attention (attention.hip) against
F.scaled_dot_product_attention, and of ops.OpsMultiheadAttention against
nn.MultiheadAttention(need_weights=False), through the library.

    python tools/attention_bench.py [--iters 10] [--repeats 3] \
        [--out profiles/attention_ab.md]

Attention: T in {64, 256, 1024}, Dh in {32, 64, 128}, B * heads chosen so
that the forward launches at least 256 blocks (256, 128, 32 slices), plus one
case with 32 blocks; fp32 and bf16; forward-only (no_grad) and forward +
backward (gradients to q, k, v). Module: embed 256, 4 heads (Dh = 64),
self-attention, batch_first. The two versions read the same tensors, run in
one process in alternating blocks of calls timed with device events; the
table gives the median block and the min..max spread over --repeats blocks,
per call. A second table times the four kernels of one forward + backward on
their own: the forward's share, and attn_bwd_dq against attn_bwd_dkv (the
second recomputation of S is what having no atomics costs). A run without a
GPU fails.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from coinstac_dinunet_amd import ops  # noqa: E402

# (T, B * heads): 256, 512, 512 forward blocks, then 32
SHAPES = ((64, 256), (256, 128), (1024, 32), (256, 8))
HEAD_DIMS = (32, 64, 128)
HEADS = 8
DTYPES = (torch.float32, torch.bfloat16)


def time_block(fn, iters):
    """ms per call over one block of `iters` calls (device events)."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def alternate(live, iters, repeats):
    """{name: [ms per call of each block]} of closures run in alternating
    blocks after three warm-up calls each."""
    for fn in live.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in live}
    for _ in range(repeats):
        for k, fn in live.items():
            times[k].append(time_block(fn, iters))
    return times


def cell(ts):
    return f'{statistics.median(ts):.4f} | {min(ts):.4f}..{max(ts):.4f}'


def passes(call, leaves, go):
    """(forward, forward + backward) closures of one version."""
    def fwd():
        with torch.no_grad():
            return call()

    def fwd_bwd():
        for t in leaves:
            t.grad = None
        call().backward(go)
    return fwd, fwd_bwd


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=10,
                    help='calls per timed block')
    ap.add_argument('--repeats', type=int, default=3,
                    help='alternating blocks per version')
    ap.add_argument('--out', default='profiles/attention_ab.md',
                    help='write the tables here too')
    args = ap.parse_args()
    C = ops.require_native()
    dev = torch.device('cuda:0')
    lines = []

    def emit(line=''):
        lines.append(line)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                        exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    emit(f'calls per block: {args.iters}, blocks per version: '
         f'{args.repeats}, device: {torch.cuda.get_device_name(0)}')
    emit()
    emit('ops.attention against F.scaled_dot_product_attention')
    emit()
    emit('| T | B*heads | Dh | dtype | pass | ops ms median | min..max | '
         'lib ms median | min..max | lib / ops time | max abs diff vs lib |')
    emit('|---|---|---|---|---|---|---|---|---|---|---|')
    kernels = []
    for dtype in DTYPES:
        name = str(dtype).replace('torch.', '')
        for Dh in HEAD_DIMS:
            for T, BH in SHAPES:
                gen = torch.Generator().manual_seed(T + Dh)
                q, k, v, go = (
                    torch.randn(BH // HEADS, HEADS, T, Dh, generator=gen)
                    .to(dev, dtype) for _ in range(4))
                for t in (q, k, v):
                    t.requires_grad_(True)
                live = {'ops': passes(lambda: ops.attention(q, k, v),
                                      (q, k, v), go),
                        'lib': passes(
                            lambda: F.scaled_dot_product_attention(q, k, v),
                            (q, k, v), go)}
                diff = (live['ops'][0]().float()
                        - live['lib'][0]().float()).abs().max().item()
                for p in (0, 1):
                    ts = alternate({n: f[p] for n, f in live.items()},
                                   args.iters, args.repeats)
                    ratio = (statistics.median(ts['lib'])
                             / statistics.median(ts['ops']))
                    emit(f"| {T} | {BH} | {Dh} | {name} | "
                         f"{'fwd+bwd' if p else 'fwd'} | {cell(ts['ops'])} | "
                         f"{cell(ts['lib'])} | {ratio:.2f} | {diff:.3g} |")
                # the kernels of one forward + backward, one at a time
                scale = Dh ** -0.5
                with torch.no_grad():
                    o, lse = C.attn_fwd(q, k, v, None, False, scale)
                    delta = C.attn_delta(o, go)
                    a = (q, k, v, go, None, lse, delta, False, scale)
                    ts = alternate({
                        'fwd': lambda: C.attn_fwd(q, k, v, None, False, scale),
                        'delta': lambda: C.attn_delta(o, go),
                        'dkv': lambda: C.attn_bwd_dkv(*a),
                        'dq': lambda: C.attn_bwd_dq(*a)},
                        args.iters, args.repeats)
                med = {n: statistics.median(t) for n, t in ts.items()}
                kernels.append(
                    f"| {T} | {BH} | {Dh} | {name} | {cell(ts['fwd'])} | "
                    f"{cell(ts['delta'])} | {cell(ts['dkv'])} | "
                    f"{cell(ts['dq'])} | "
                    f"{med['fwd'] / sum(med.values()):.2f} | "
                    f"{med['dq'] / med['dkv']:.2f} |")
                del live, q, k, v, go, o, lse, delta, a
        torch.cuda.empty_cache()
    emit()
    emit('Kernels of one forward + backward, each timed on its own (ms per '
         'launch, median | min..max)')
    emit()
    emit('| T | B*heads | Dh | dtype | attn_fwd | | attn_delta | | '
         'attn_bwd_dkv | | attn_bwd_dq | | fwd share | dq / dkv |')
    emit('|---|---|---|---|---|---|---|---|---|---|---|---|---|---|')
    for line in kernels:
        emit(line)
    emit()
    emit('ops.OpsMultiheadAttention against nn.MultiheadAttention '
         '(need_weights=False), embed 256, 4 heads, self-attention')
    emit()
    emit('| T | B | dtype | pass | ops ms median | min..max | '
         'lib ms median | min..max | lib / ops time | max abs diff vs lib |')
    emit('|---|---|---|---|---|---|---|---|---|---|')
    for dtype in DTYPES:
        name = str(dtype).replace('torch.', '')
        torch.manual_seed(1)
        m_ops = ops.OpsMultiheadAttention(256, 4, batch_first=True)
        m_lib = nn.MultiheadAttention(256, 4, batch_first=True)
        m_lib.load_state_dict(m_ops.state_dict())
        m_ops, m_lib = m_ops.to(dev, dtype), m_lib.to(dev, dtype)
        for T, B in ((64, 64), (256, 32), (1024, 8)):
            gen = torch.Generator().manual_seed(T)
            x = torch.randn(B, T, 256, generator=gen).to(dev, dtype)
            x.requires_grad_(True)
            go = torch.randn(B, T, 256, generator=gen).to(dev, dtype)
            live = {}
            for n, m in (('ops', m_ops), ('lib', m_lib)):
                live[n] = passes(
                    lambda m=m: m(x, x, x, need_weights=False)[0],
                    (x, *m.parameters()), go)
            diff = (live['ops'][0]().float()
                    - live['lib'][0]().float()).abs().max().item()
            for p in (0, 1):
                ts = alternate({n: f[p] for n, f in live.items()},
                               args.iters, args.repeats)
                ratio = (statistics.median(ts['lib'])
                         / statistics.median(ts['ops']))
                emit(f"| {T} | {B} | {name} | {'fwd+bwd' if p else 'fwd'} | "
                     f"{cell(ts['ops'])} | {cell(ts['lib'])} | {ratio:.2f} | "
                     f'{diff:.3g} |')
            del live, x, go


if __name__ == '__main__':
    main()
