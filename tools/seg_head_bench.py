"""A/B of the segmentation loss+metric head: fused HIP path vs eager chain.

    python tools/seg_head_bench.py [--iters 100] [--repeats 5] \
        [--out profiles/seg_head_ab.md]

For binary dice (one logit plane) and C = 4 cross-entropy, at 2xCx128^3 and
4xCx160^3 in bf16, one "step" is loss forward + backward + metric update:

  fused   ops.dice_loss_with_logits + Prf1a.add_logits
          ops.cross_entropy (5-D)   + ConfusionMatrix.add_logits
  eager   sigmoid -> dice_loss_binary -> (prob > 0.5).long() -> Prf1a.add
          F.cross_entropy -> argmax   -> ConfusionMatrix.add

The eager chain is pure torch (plus the metric kernels both paths end in)
and does not touch segloss.hip. Both versions run in one process, in
alternating blocks of --iters steps timed with device events; the table
gives the median block and the min..max spread over --repeats blocks. Each
step ends in the metric's one device-to-host copy, in both versions. Bytes
per voxel are computed from shapes: what each fused kernel has to read and
write. Peak extra memory is max_memory_allocated over one step above what
was allocated before it. A run without a GPU fails.
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
from coinstac_dinunet_amd.metrics import ConfusionMatrix, Prf1a  # noqa: E402
from coinstac_dinunet_amd.metrics.loss import dice_loss_binary  # noqa: E402

SHAPES = [(2, 128), (4, 160)]
CE_CLASSES = 4


def make_case(kind, n, side, dev):
    gen = torch.Generator().manual_seed(1000 * side + n)
    c = 1 if kind == 'dice' else CE_CLASSES
    x = torch.randn(n, c, side, side, side, generator=gen).to(torch.bfloat16)
    x = x.to(dev).requires_grad_(True)
    if kind == 'dice':
        y = (torch.rand(n, 1, side, side, side, generator=gen) > 0.7)
        y = y.to(torch.uint8).to(dev)
    else:
        y = torch.randint(0, c, (n, side, side, side), generator=gen).to(dev)
    return x, y


def steps(kind, x, y):
    """(fused_step, eager_step) closures; each returns the loss."""
    if kind == 'dice':
        def fused():
            x.grad = None
            loss = ops.dice_loss_with_logits(x, y)
            loss.backward()
            Prf1a().add_logits(x.detach(), y)
            return loss

        def eager():
            x.grad = None
            prob = torch.sigmoid(x)
            loss = dice_loss_binary(prob, y)
            loss.backward()
            Prf1a().add((prob.detach() > 0.5).long(), y)
            return loss
    else:
        def fused():
            x.grad = None
            loss = ops.cross_entropy(x, y)
            loss.backward()
            ConfusionMatrix(num_classes=CE_CLASSES).add_logits(x.detach(), y)
            return loss

        def eager():
            x.grad = None
            loss = F.cross_entropy(x, y)
            loss.backward()
            ConfusionMatrix(num_classes=CE_CLASSES).add(
                torch.argmax(x.detach(), 1), y)
            return loss
    return fused, eager


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


def peak_extra_bytes(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del loss
    return peak


def kernel_rows(kind, x, y, iters):
    """[(kernel, bytes/voxel, ms, GB/s)] for each fused kernel on its own."""
    C = ops.require_native()
    xd = x.detach()
    nvox = y.numel()
    lb = y.element_size()
    go = torch.ones((), device=x.device)
    if kind == 'dice':
        _, sums = C.seg_dice_fwd(xd, y, None, 1.0, 1e-5)
        calls = [
            ('seg_dice_fwd', 2 + lb,
             lambda: C.seg_dice_fwd(xd, y, None, 1.0, 1e-5)),
            ('seg_dice_bwd', 2 + lb + 2,
             lambda: C.seg_dice_bwd(xd, y, None, sums, go, 1.0, 1e-5)),
            ('seg_prf1a', 2 + lb, lambda: C.seg_prf1a_counts(xd, y)),
        ]
    else:
        k = CE_CLASSES
        _, lse = C.seg_ce_fwd(xd, y)
        calls = [
            ('seg_ce_fwd', 2 * k + lb + 4, lambda: C.seg_ce_fwd(xd, y)),
            ('seg_ce_bwd', 2 * k + lb + 4 + 2 * k,
             lambda: C.seg_ce_bwd(xd, y, lse, go)),
            ('seg_confusion', 2 * k + lb,
             lambda: C.seg_confusion_matrix(xd, y, k)),
        ]
    rows = []
    for name, bpv, fn in calls:
        for _ in range(5):
            fn()
        ms = statistics.median(time_block(fn, iters) for _ in range(3))
        rows.append((name, bpv, ms, bpv * nvox / (ms * 1e-3) / 1e9))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=100,
                    help='steps per timed block')
    ap.add_argument('--repeats', type=int, default=5,
                    help='alternating blocks per version')
    ap.add_argument('--out', default=None, help='write the table here too')
    args = ap.parse_args()
    ops.require_native()
    dev = torch.device('cuda:0')

    lines = ['| head | logits | version | ms/step median | min..max | '
             'peak extra MiB | loss |', '|---|---|---|---|---|---|---|']
    klines = ['| head | logits | kernel | B/voxel | ms | GB/s |',
              '|---|---|---|---|---|---|']
    for kind in ('dice', 'ce'):
        for n, side in SHAPES:
            x, y = make_case(kind, n, side, dev)
            c = x.shape[1]
            shape = f'{n}x{c}x{side}^3 bf16'
            fused, eager = steps(kind, x, y)
            for fn in (fused, eager):          # warm up every shape
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            times = {'fused': [], 'eager': []}
            for _ in range(args.repeats):      # alternate the two versions
                times['fused'].append(time_block(fused, args.iters))
                times['eager'].append(time_block(eager, args.iters))
            mem = {'fused': peak_extra_bytes(fused),
                   'eager': peak_extra_bytes(eager)}
            val = {'fused': float(fused().detach()),
                   'eager': float(eager().detach())}
            for ver in ('fused', 'eager'):
                t = times[ver]
                lines.append(
                    f'| {kind} | {shape} | {ver} | '
                    f'{statistics.median(t):.3f} | {min(t):.3f}..{max(t):.3f}'
                    f' | {mem[ver] / 2**20:.1f} | {val[ver]:.6f} |')
            for name, bpv, ms, gbs in kernel_rows(kind, x, y, args.iters):
                klines.append(f'| {kind} | {shape} | {name} | {bpv} | '
                              f'{ms:.4f} | {gbs:.0f} |')
            del x, y, fused, eager
            torch.cuda.empty_cache()

    text = '\n'.join(
        [f'steps per block: {args.iters}, blocks per version: '
         f'{args.repeats}, device: {torch.cuda.get_device_name(0)}', '']
        + lines + ['', 'Fused kernels on their own (bytes from shapes):', '']
        + klines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
