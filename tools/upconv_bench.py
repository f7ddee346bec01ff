"""A/B of the UNet3D decoder step: interpolate + conv vs upsample2_conv3d.

    python tools/upconv_bench.py [--iters 50] [--repeats 5] \
        [--out profiles/upconv_ab.md]

At the default-width decoder shapes of 64^3 and 128^3 inputs (N = 2, bf16):

  A         F.interpolate(x, scale_factor=2, 'nearest') + OpsConv3d — what
            the decoder ran before upconv3d.hip
  B         ops.upsample2_conv3d on the route route_upconv3d picks
  composed  upsample2_nearest3d + the plain forward kernels, forward only:
            the other route, timed so the routing rule rests on a number

forward-only and forward + backward (gradients to x and the weight). The
versions run in one process, in alternating blocks of --iters calls timed
with device events; the table gives the median block and the min..max spread
over --repeats blocks. TF/s is MFMA FLOPs computed from shapes over event
time: 2 * M * Cout * Cin * slots with M the output positions, slots = 27
(A, composed) or 64 / 8 = 8 per output position (collapsed forward; the
backward of both versions is counted at 2 x 27). Peak extra memory is
max_memory_allocated over one forward + backward above what was allocated
before it. A run without a GPU fails.

    python tools/upconv_bench.py --bwd [--out profiles/upconv_bwd_ab.md]

times the backward instead, at the same shapes and in the same alternating
blocks: forward + backward of upsample2_conv3d with the backward on the
'composed' route (COINN_UPCONV_BWD=composed: full-resolution dgrad +
fold2_sum3d, wgrad on an upsampled temporary) and on the 'collapsed' route
(upconv3d_dgrad + upconv3d_wgrad), then each backward kernel alone against
the composed calls it replaces. Weight prep is inside the timed calls. The
table adds the max abs difference of dx and dw between the two routes and,
per row, spread = (max - min) / median over its blocks; `clear` is whether
the collapsed median beats the composed one by more than the larger of the
two spreads, the rule route_upconv3d_bwd rests on.
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
from coinstac_dinunet_amd.ops import conv as opsconv  # noqa: E402

# (N, Cin, Cout, low-res side)
SHAPES = [(2, 64, 32, 16), (2, 32, 16, 32), (2, 64, 32, 32), (2, 32, 16, 64)]


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
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def make_case(n, cin, cout, side, dev):
    gen = torch.Generator().manual_seed(1000 * side + cin)
    x = torch.randn(n, cin, side, side, side, generator=gen)
    x = x.to(dev, torch.bfloat16).requires_grad_(True)
    conv = opsconv.OpsConv3d(cin, cout, 3, padding=1, bias=False).to(dev)
    go = torch.randn(n, cout, 2 * side, 2 * side, 2 * side, generator=gen)
    return x, conv, go.to(dev, torch.bfloat16)


def versions(x, conv, go):
    """{name: (forward, forward_backward or None)} closures."""
    C = ops.require_native()
    wb = conv.weight.detach().to(torch.bfloat16)

    def fwd_a():
        return conv(F.interpolate(x, scale_factor=2, mode='nearest'))

    def fwd_b():
        return opsconv.upsample2_conv3d(x, conv.weight, None)

    def fwd_composed():
        return opsconv._fwd3d(C, C.upsample2_nearest3d(x.detach()), wb, 1)

    def with_bwd(fwd):
        def step():
            x.grad = None
            conv.weight.grad = None
            fwd().backward(go)
        return step

    def no_grad(fwd):
        def step():
            with torch.no_grad():
                return fwd()
        return step

    return {'A': (no_grad(fwd_a), with_bwd(fwd_a)),
            'B': (no_grad(fwd_b), with_bwd(fwd_b)),
            'composed': (fwd_composed, None)}


def bwd_versions(x, conv, go):
    """{group: {name: fn}}: the rows of one group are compared."""
    C = ops.require_native()
    xb = x.detach()
    wb = conv.weight.detach().to(torch.bfloat16)
    up_shape = list(xb.shape[:2]) + [2 * s for s in xb.shape[2:]]

    def step(route):
        def fn():
            os.environ['COINN_UPCONV_BWD'] = route
            x.grad = None
            conv.weight.grad = None
            opsconv.upsample2_conv3d(x, conv.weight, None).backward(go)
            return x.grad, conv.weight.grad
        return fn

    return {
        'fwd+bwd': {'composed': step('composed'),
                    'collapsed': step('collapsed')},
        'dgrad': {'composed': lambda: C.fold2_sum3d(
                      opsconv._dgrad3d(C, go, wb, up_shape, 1)),
                  'collapsed': lambda: C.upconv3d_dgrad(go, wb,
                                                        list(xb.shape))},
        'wgrad': {'composed': lambda: C.conv3d_wgrad(
                      C.upsample2_nearest3d(xb), go, 1, 0),
                  'collapsed': lambda: C.upconv3d_wgrad(xb, go)},
    }


def main_bwd(args):
    dev = torch.device('cuda:0')
    lines = ['| shape | pass | backward | ms median | min..max | spread | '
             'speed-up | clear | peak extra MiB | max abs diff dx | '
             'max abs diff dw |',
             '|---|---|---|---|---|---|---|---|---|---|---|']
    for n, cin, cout, side in SHAPES:
        x, conv, go = make_case(n, cin, cout, side, dev)
        shape = f'{n}x{cin}->{cout} {side}^3->{2 * side}^3'
        groups = bwd_versions(x, conv, go)
        gc = [g.float().clone() for g in groups['fwd+bwd']['composed']()]
        gn = [g.float().clone() for g in groups['fwd+bwd']['collapsed']()]
        diff = [(a - b).abs().max().item() for a, b in zip(gc, gn)]
        for gname, live in groups.items():
            for fn in live.values():
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in live}
            for _ in range(args.repeats):
                for k, fn in live.items():
                    times[k].append(time_block(fn, args.iters))
            med = {k: statistics.median(t) for k, t in times.items()}
            spread = {k: (max(t) - min(t)) / med[k]
                      for k, t in times.items()}
            gain = 1 - med['collapsed'] / med['composed']
            clear = gain > max(spread.values())
            for k, fn in live.items():
                t = times[k]
                new = k == 'collapsed'
                lines.append(
                    f'| {shape} | {gname} | {k} | {med[k]:.4f} | '
                    f'{min(t):.4f}..{max(t):.4f} | {spread[k]:.3f} | '
                    + (f"{med['composed'] / med[k]:.2f}x | "
                       f"{'yes' if clear else 'NO'} | " if new else '- | - | ')
                    + f'{peak_extra_bytes(fn) / 2**20:.1f} | '
                    + (f'{diff[0]:.4g} | {diff[1]:.4g} |'
                       if new and gname == 'fwd+bwd' else '- | - |'))
        os.environ.pop('COINN_UPCONV_BWD', None)
        del x, conv, go, groups, live, gc, gn
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--bwd', action='store_true',
                    help='A/B the backward routes instead '
                         '(default --out profiles/upconv_bwd_ab.md)')
    ap.add_argument('--iters', type=int, default=50,
                    help='calls per timed block')
    ap.add_argument('--repeats', type=int, default=5,
                    help='alternating blocks per version')
    ap.add_argument('--out', default=None,
                    help='write the table here too '
                         '(default profiles/upconv_ab.md)')
    args = ap.parse_args()
    if args.out is None:
        args.out = ('profiles/upconv_bwd_ab.md' if args.bwd
                    else 'profiles/upconv_ab.md')
    ops.require_native()
    dev = torch.device('cuda:0')
    if args.bwd:
        return write_table(args, main_bwd(args))

    lines = ['| shape | pass | version | route | ms median | min..max | '
             'TF/s | peak extra MiB | max abs diff vs A |',
             '|---|---|---|---|---|---|---|---|---|']
    for n, cin, cout, side in SHAPES:
        x, conv, go = make_case(n, cin, cout, side, dev)
        route = opsconv.route_upconv3d(cin, side, side)
        shape = f'{n}x{cin}->{cout} {side}^3->{2 * side}^3'
        m_out = n * 8 * side ** 3
        conv_flops = 2.0 * m_out * cout * cin * 27
        fwd_flops = {'A': conv_flops, 'composed': conv_flops,
                     'B': conv_flops * 8 / 27 if route == 'collapsed'
                     else conv_flops}
        vers = versions(x, conv, go)
        with torch.no_grad():
            ref = vers['A'][0]().float()
            diff = {k: (v[0]().float() - ref).abs().max().item()
                    for k, v in vers.items()}
        for p in (0, 1):
            live = {k: v[p] for k, v in vers.items() if v[p] is not None}
            for fn in live.values():               # warm up every shape
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in live}
            for _ in range(args.repeats):          # alternate the versions
                for k, fn in live.items():
                    times[k].append(time_block(fn, args.iters))
            for k, fn in live.items():
                t = times[k]
                med = statistics.median(t)
                flops = fwd_flops[k] + (2 * conv_flops if p else 0)
                mem = f'{peak_extra_bytes(fn) / 2**20:.1f}' if p else '-'
                lines.append(
                    f"| {shape} | {'fwd+bwd' if p else 'fwd'} | {k} | "
                    f"{route if k == 'B' else '-'} | {med:.4f} | "
                    f'{min(t):.4f}..{max(t):.4f} | '
                    f'{flops / (med * 1e-3) / 1e12:.1f} | {mem} | '
                    f'{diff[k]:.4g} |')
        del x, conv, go, vers, live
        torch.cuda.empty_cache()
    write_table(args, lines)


def write_table(args, lines):
    text = '\n'.join(
        [f'calls per block: {args.iters}, blocks per version: '
         f'{args.repeats}, device: {torch.cuda.get_device_name(0)}', '']
        + lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
