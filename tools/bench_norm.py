"""A/B of GroupNorm + ReLU: the HIP kernels against stock PyTorch.

    python tools/bench_norm.py [--iters 20] [--repeats 5] \
        [--out profiles/groupnorm_ab.md]

bf16 [N, C, D, H, W] activations, 8 groups, the norm layers of the models:
2x32x128^3 (MeshNet), 2x16x64^3 (UNet3D stem), 2x64x32^3 (UNet3D) and
16x64x32^3 (VBM).

  ops      OpsGroupNorm(8, C, relu=True) on groupnorm.hip
  stock    F.relu(F.group_norm(x, 8, w, b)) with bf16 x, w, b through the
           library: what such a layer ran on before these kernels
  bn-norm  ops' bn3d_normalize on the same tensor (forward rows only): one
           read and one write of the activation, the streaming rate this
           code base reaches on these bytes

forward-only (no_grad) and forward + backward (gradients to x, weight and
bias). The versions run in one process, in alternating blocks of calls
timed with device events; the table gives the median block and the
min..max spread over --repeats blocks. GB/s is the bytes the algorithm has
to move over the median time: forward 6 B/element (statistics read x,
normalize reads x and writes y), forward + backward 16 B/element (two more
passes read dy and x, the second writes dx), bn-norm 4 B/element; all
launches of a call are inside the time. A run without a GPU fails.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from coinstac_dinunet_amd import ops  # noqa: E402

GROUPS = 8
SHAPES = [('MeshNet', (2, 32, 128, 128, 128)),
          ('UNet3D stem', (2, 16, 64, 64, 64)),
          ('UNet3D', (2, 64, 32, 32, 32)),
          ('VBM', (16, 64, 32, 32, 32))]
BYTES = {'fwd': 6, 'fwd+bwd': 16, 'bn-norm': 4}


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


def steps(norm, params, x, go):
    """(forward, forward + backward) closures of y = norm(x)."""
    def fwd():
        with torch.no_grad():
            return norm(x)

    def fwd_bwd():
        x.grad = None
        for p in params:
            p.grad = None
        norm(x).backward(go)
    return {'fwd': fwd, 'fwd+bwd': fwd_bwd}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=20,
                    help='calls per timed block')
    ap.add_argument('--repeats', type=int, default=5,
                    help='alternating blocks per version')
    ap.add_argument('--out', default='profiles/groupnorm_ab.md',
                    help='write the table here too')
    args = ap.parse_args()
    C = ops.require_native()
    dev = torch.device('cuda:0')

    lines = [f'calls per block: {args.iters}, blocks per version: '
             f'{args.repeats}, device: {torch.cuda.get_device_name(0)}', '',
             '| layer | shape | pass | version | ms median | min..max | '
             'GB/s | stock / ops time | max abs diff vs stock |',
             '|---|---|---|---|---|---|---|---|---|']

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                        exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    for line in lines:
        print(line, flush=True)
    for layer, shape in SHAPES:
        ch = shape[1]
        gen = torch.Generator().manual_seed(ch * shape[2])
        x = torch.randn(*shape, generator=gen).to(dev, torch.bfloat16)
        x.requires_grad_(True)
        go = torch.randn(*shape, generator=gen).to(dev, torch.bfloat16)
        m_ops = ops.OpsGroupNorm(GROUPS, ch, relu=True).to(dev)
        w = torch.ones(ch, device=dev, dtype=torch.bfloat16,
                       requires_grad=True)
        b = torch.zeros(ch, device=dev, dtype=torch.bfloat16,
                        requires_grad=True)
        live = {
            'ops': steps(m_ops, list(m_ops.parameters()), x, go),
            'stock': steps(lambda t: F.relu(F.group_norm(t, GROUPS, w, b)),
                           [w, b], x, go)}
        mean_rstd = torch.tensor([0.0, 1.0], device=dev).repeat(ch, 1)
        xd = x.detach()
        live['bn-norm'] = {'fwd': lambda: C.bn3d_normalize(
            xd, mean_rstd, m_ops.weight, m_ops.bias, True)}
        diff = (live['ops']['fwd']().float()
                - live['stock']['fwd']().float()).abs().max().item()
        name = 'x'.join(str(s) for s in shape)
        for p in ('fwd', 'fwd+bwd'):
            fns = {k: v[p] for k, v in live.items() if p in v}
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in fns}
            for _ in range(args.repeats):
                for k, fn in fns.items():
                    times[k].append(time_block(fn, args.iters))
            med = {k: statistics.median(t) for k, t in times.items()}
            for k, t in times.items():
                nbytes = BYTES['bn-norm' if k == 'bn-norm' else p] * x.numel()
                extra = (f"{med['stock'] / med[k]:.2f} | {diff:.4g} |"
                         if k == 'ops' else '- | - |')
                emit(f'| {layer} | {name} | {p} | {k} | {med[k]:.4f} | '
                     f'{min(t):.4f}..{max(t):.4f} | '
                     f'{nbytes / med[k] / 1e6:.0f} | ' + extra)
        del live, m_ops, x, xd, go
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
