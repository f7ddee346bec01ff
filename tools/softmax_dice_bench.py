"""A/B of the multi-class soft-dice (+CE) loss: fused HIP path vs eager chains.

    python tools/softmax_dice_bench.py [--iters 20] [--repeats 5] \
        [--out profiles/softmax_dice_ab.md]

bf16 logits at 2x4x128^3, 1x50x128^3 and 1x104x128^3, uint8 labels, one
"step" is loss forward + backward, with ce_weight 0 and 1:

  (a) fused   ops.softmax_dice_loss                       (segdice.hip)
  (b) eager   softmax -> dice_loss_multiclass (+ F.cross_entropy)
  (c) mixed   ops.cross_entropy + eager dice              (ce_weight 1 only)

All versions run in one process, in alternating blocks of --iters steps
timed with device events; the table gives the median block and the min..max
spread over --repeats blocks. Peak extra memory is max_memory_allocated over
one step above what was allocated before it. The kernel table times each
fused kernel on its own next to seg_ce_fwd / seg_ce_bwd at the same shape;
bytes per voxel are what each kernel has to read and write, from shapes
(forward: logits + labels + lse write; backward: logits + lse + labels +
gradient write). A run without a GPU fails.
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
from coinstac_dinunet_amd.metrics import dice_loss_multiclass  # noqa: E402

SHAPES = [(2, 4, 128), (1, 50, 128), (1, 104, 128)]


def make_case(n, c, side, dev):
    gen = torch.Generator(device=dev).manual_seed(1000 * c + n)
    x = torch.randn(n, c, side, side, side, generator=gen, device=dev,
                    dtype=torch.bfloat16).requires_grad_(True)
    y = torch.randint(0, c, (n, side, side, side), generator=gen, device=dev,
                      dtype=torch.uint8)
    return x, y


def steps(x, y, w):
    """{version: step} closures; each returns the loss."""
    def fused():
        x.grad = None
        loss = ops.softmax_dice_loss(x, y, ce_weight=w)
        loss.backward()
        return loss

    def probs():
        return torch.softmax(x, 1, dtype=torch.float32)

    def eager():
        x.grad = None
        loss = dice_loss_multiclass(probs(), y)
        if w:
            loss = loss + w * F.cross_entropy(x, y.long())
        loss.backward()
        return loss

    def mixed():
        x.grad = None
        loss = dice_loss_multiclass(probs(), y) + w * ops.cross_entropy(x, y)
        loss.backward()
        return loss

    out = {'a fused': fused, 'b eager': eager}
    if w:
        out['c ops.ce + eager dice'] = mixed
    return out


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


def kernel_rows(x, y, iters):
    """[(kernel, bytes/voxel, median ms, min, max, GB/s)], each on its own."""
    C = ops.require_native()
    xd = x.detach()
    k = x.shape[1]
    nvox = y.numel()
    lb = y.element_size()
    go = torch.ones((), device=x.device)
    _, lse, coef = C.seg_sdice_fwd(xd, y, 1.0, True, False, 1e-5)
    fwd_b, bwd_b = 2 * k + lb + 4, 2 * k + 4 + lb + 2 * k
    calls = [
        ('seg_sdice_fwd', fwd_b,
         lambda: C.seg_sdice_fwd(xd, y, 1.0, True, False, 1e-5)),
        ('seg_ce_fwd', fwd_b, lambda: C.seg_ce_fwd(xd, y)),
        ('seg_sdice_bwd', bwd_b,
         lambda: C.seg_sdice_bwd(xd, y, lse, coef, go, 1.0)),
        ('seg_ce_bwd', bwd_b, lambda: C.seg_ce_bwd(xd, y, lse, go)),
    ]
    for _, _, fn in calls:
        for _ in range(5):
            fn()
    times = {name: [] for name, _, _ in calls}
    for _ in range(3):                       # alternate the four kernels
        for name, _, fn in calls:
            times[name].append(time_block(fn, iters))
    rows = []
    for name, bpv, _ in calls:
        ms = statistics.median(times[name])
        rows.append((name, bpv, ms, min(times[name]), max(times[name]),
                     bpv * nvox / (ms * 1e-3) / 1e9))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=20,
                    help='steps per timed block')
    ap.add_argument('--repeats', type=int, default=5,
                    help='alternating blocks per version')
    ap.add_argument('--out', default=None, help='write the tables here too')
    args = ap.parse_args()
    ops.require_native()
    dev = torch.device('cuda:0')

    lines = ['| logits | ce_weight | version | ms/step median | min..max | '
             'peak extra MiB | loss |', '|---|---|---|---|---|---|---|']
    klines = ['| logits | kernel | B/voxel | ms median | min..max | GB/s |',
              '|---|---|---|---|---|---|']
    for n, c, side in SHAPES:
        x, y = make_case(n, c, side, dev)
        shape = f'{n}x{c}x{side}^3 bf16'
        for w in (0.0, 1.0):
            vers = steps(x, y, w)
            for fn in vers.values():           # warm up every version
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {v: [] for v in vers}
            for _ in range(args.repeats):      # alternate the versions
                for v, fn in vers.items():
                    times[v].append(time_block(fn, args.iters))
            for v, fn in vers.items():
                t = times[v]
                mem = peak_extra_bytes(fn)
                val = float(fn().detach())
                lines.append(
                    f'| {shape} | {w:g} | {v} | {statistics.median(t):.3f} | '
                    f'{min(t):.3f}..{max(t):.3f} | {mem / 2**20:.1f} | '
                    f'{val:.6f} |')
            x.grad = None
            torch.cuda.empty_cache()
        for name, bpv, ms, lo, hi, gbs in kernel_rows(x, y, args.iters):
            klines.append(f'| {shape} | {name} | {bpv} | {ms:.4f} | '
                          f'{lo:.4f}..{hi:.4f} | {gbs:.0f} |')
        del x, y
        torch.cuda.empty_cache()

    text = '\n'.join(
        [f'steps per block: {args.iters}, blocks per version: '
         f'{args.repeats}, device: {torch.cuda.get_device_name(0)}', '']
        + lines + ['', 'Kernels on their own (bytes from shapes; seg_ce_* '
                   'is the yardstick streaming the same planes):', '']
        + klines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
