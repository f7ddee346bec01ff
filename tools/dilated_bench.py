"""A/B of the dilated 3x3x3 conv3d (dilation == padding == d), the MeshNet
layer.

    python tools/dilated_bench.py [--iters 20] [--lib-iters 2] [--repeats 5] \
        [--out profiles/dilated_ab.md]

N = 1, bf16, channels 32 -> 32 and 64 -> 64 on 64^3 and 128^3, d in
{2, 4, 8, 16}, no bias:

  ops      OpsConv3d on conv3d_dilated.hip (sub-lattice slab kernels)
  lib      nn.Conv3d with bf16 parameters and the same dilation through the
           library: what such a layer ran on before these kernels. It gets
           --lib-iters calls per block, it can be very slow.
  dense    OpsConv3d with dilation 1 on the same shape (the dense 3x3x3
           kernels): the same FLOPs, the ceiling this code base has shown.
           Timed once per shape, repeated on every d row for comparison.

forward-only and forward + backward (gradients to x and the weight). The
versions run in one process, in alternating blocks of calls timed with device
events; the table gives the median block and the min..max spread over
--repeats blocks. TF/s is 2 * 27 * Cin * Cout * positions (x 3 for forward +
backward) over the median time, weight prep launches included. `staging` is
(32 + 2d) / 32, the slab columns staged per output column of the forward
tile. A run without a GPU fails.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from coinstac_dinunet_amd import ops  # noqa: E402
from coinstac_dinunet_amd.ops import conv as opsconv  # noqa: E402

CHANNELS = (32, 64)
SIDES = (64, 128)
DILATIONS = (2, 4, 8, 16)


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


def steps(mod, x, go):
    """(forward, forward + backward) closures of one module."""
    def fwd():
        with torch.no_grad():
            return mod(x)

    def fwd_bwd():
        x.grad = None
        mod.zero_grad(set_to_none=True)
        mod(x).backward(go)
    return fwd, fwd_bwd


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=20,
                    help='calls per timed block (ops, dense)')
    ap.add_argument('--lib-iters', type=int, default=2,
                    help='calls per timed block of the library conv')
    ap.add_argument('--repeats', type=int, default=5,
                    help='alternating blocks per version')
    ap.add_argument('--out', default='profiles/dilated_ab.md',
                    help='write the table here too')
    args = ap.parse_args()
    ops.require_native()
    dev = torch.device('cuda:0')
    iters = {'ops': args.iters, 'dense': args.iters, 'lib': args.lib_iters}

    lines = [f'calls per block: {args.iters} (lib: {args.lib_iters}), blocks '
             f'per version: {args.repeats}, device: '
             f'{torch.cuda.get_device_name(0)}', '',
             '| shape | d | pass | version | ms median | min..max | TF/s | '
             'ops / dense time | staging | lib / ops time | '
             'max abs diff vs lib |',
             '|---|---|---|---|---|---|---|---|---|---|---|']

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                        exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    def measure(live, p):
        """{name: block times} of pass p, versions alternating."""
        for k, fns in live.items():
            for _ in range(1 if k == 'lib' else 3):
                fns[p]()
        torch.cuda.synchronize()
        times = {k: [] for k in live}
        for _ in range(args.repeats):
            for k, fns in live.items():
                times[k].append(time_block(fns[p], iters[k]))
        return times

    for line in lines:
        print(line, flush=True)
    for c in CHANNELS:
        for side in SIDES:
            gen = torch.Generator().manual_seed(1000 * side + c)
            x = torch.randn(1, c, side, side, side, generator=gen)
            x = x.to(dev, torch.bfloat16).requires_grad_(True)
            go = torch.randn(1, c, side, side, side, generator=gen)
            go = go.to(dev, torch.bfloat16)
            flops = 2.0 * 27 * c * c * side ** 3
            shape = f'1x{c}->{c} {side}^3'
            dense = opsconv.OpsConv3d(c, c, 3, padding=1, bias=False).to(dev)
            dense_fns = steps(dense, x, go)
            dense_med = []
            for p in (0, 1):
                t = measure({'dense': dense_fns}, p)['dense']
                dense_med.append(statistics.median(t))
                emit(f"| {shape} | 1 | {'fwd+bwd' if p else 'fwd'} | dense | "
                     f'{dense_med[p]:.4f} | {min(t):.4f}..{max(t):.4f} | '
                     f'{flops * (3 if p else 1) / dense_med[p] / 1e9:.1f} | '
                     f'- | - | - | - |')
            for d in DILATIONS:
                m_ops = opsconv.OpsConv3d(c, c, 3, padding=d, dilation=d,
                                          bias=False).to(dev)
                m_lib = nn.Conv3d(c, c, 3, padding=d, dilation=d,
                                  bias=False).to(dev, torch.bfloat16)
                with torch.no_grad():
                    m_lib.weight.copy_(m_ops.weight)
                live = {'ops': steps(m_ops, x, go),
                        'lib': steps(m_lib, x, go)}
                try:
                    ref = live['lib'][0]().float()
                    diff = (live['ops'][0]().float() - ref).abs().max().item()
                    live['lib'][1]()
                    diff = f'{diff:.4g}'
                    del ref
                except RuntimeError as e:   # the library has no such kernel
                    print(f'{shape} d={d}: lib failed: {e}', flush=True)
                    del live['lib']
                    diff = 'lib failed'
                for p in (0, 1):
                    times = measure(live, p)
                    med = {k: statistics.median(t) for k, t in times.items()}
                    for k, t in times.items():
                        tf = flops * (3 if p else 1) / med[k] / 1e9
                        if k == 'ops':
                            extra = (f'{med[k] / dense_med[p]:.2f} | '
                                     f'{(32 + 2 * d) / 32:.2f} | '
                                     + (f"{med['lib'] / med[k]:.1f}"
                                        if 'lib' in med else '-')
                                     + f' | {diff} |')
                        else:
                            extra = '- | - | - | - |'
                        emit(f"| {shape} | {d} | {'fwd+bwd' if p else 'fwd'}"
                             f' | {k} | {med[k]:.4f} | '
                             f'{min(t):.4f}..{max(t):.4f} | {tf:.1f} | '
                             + extra)
                del live, m_ops, m_lib
                torch.cuda.empty_cache()
            del dense, dense_fns, x, go
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
