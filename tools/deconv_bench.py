"""A/B of the learned 2x decoder upsample, ConvTranspose3d(kernel 2, stride 2).

    python tools/deconv_bench.py [--iters 50] [--repeats 5] \
        [--out profiles/deconv_ab.md]

At the decoder shapes of UNet3D(widths=(16, 32, 64)) and (32, 64, 128) on a
64^3 input (N = 2, bf16, bias as nn.ConvTranspose3d defaults):

  ops      OpsConvTranspose3d on deconv3d.hip
  lib      nn.ConvTranspose3d with bf16 parameters through the library
  upconv   ops.upsample2_conv3d (nearest-2x + 3x3x3 conv, upconv3d.hip) with
           the same channels: the decoder's other mode
  stream   bn3d_normalize on a tensor sized to move the forward's byte count
           (half read, half written), forward only: what a streaming kernel
           of this code base reaches on those bytes

forward-only and forward + backward (gradients to x and the parameters). The
versions run in one process, in alternating blocks of --iters calls timed
with device events; the table gives the median block and the min..max spread
over --repeats blocks. The forward's HBM bytes are 2 * S * (Cin + 8 * Cout)
for S = N * D * H * W low-res positions (x read once, y written once); the
HBM column is those bytes over the median time as a fraction of the 8 TB/s
of ops/csrc/common.h, weight prep launch included in the time. A run without
a GPU fails.
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

HBM_BYTES_PER_S = 8e12   # ops/csrc/common.h

# (N, Cin, Cout, low-res side)
SHAPES = [(2, 64, 32, 16), (2, 32, 16, 32), (2, 128, 64, 16), (2, 64, 32, 32)]


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


def versions(n, cin, cout, side, dev):
    """{name: (forward, forward_backward or None)} closures."""
    C = ops.require_native()
    gen = torch.Generator().manual_seed(1000 * side + cin)
    x = torch.randn(n, cin, side, side, side, generator=gen)
    x = x.to(dev, torch.bfloat16).requires_grad_(True)
    go = torch.randn(n, cout, 2 * side, 2 * side, 2 * side, generator=gen)
    go = go.to(dev, torch.bfloat16)
    m_ops = opsconv.OpsConvTranspose3d(cin, cout, 2, stride=2).to(dev)
    m_lib = nn.ConvTranspose3d(cin, cout, 2, stride=2).to(dev, torch.bfloat16)
    with torch.no_grad():
        m_lib.weight.copy_(m_ops.weight)
        m_lib.bias.copy_(m_ops.bias)
    up = opsconv.OpsConv3d(cin, cout, 3, padding=1, bias=False).to(dev)
    # bn3d_normalize reads and writes numel * 2 bytes each
    sc = (cin + 8 * cout) // 2
    xs = torch.randn(n, sc, side, side, side, generator=gen)
    xs = xs.to(dev, torch.bfloat16)
    mr = torch.stack([torch.zeros(sc), torch.ones(sc)], 1).to(dev)
    gamma, beta = torch.ones(sc, device=dev), torch.zeros(sc, device=dev)

    fwds = {'ops': (lambda: m_ops(x), m_ops),
            'lib': (lambda: m_lib(x), m_lib),
            'upconv': (lambda: opsconv.upsample2_conv3d(x, up.weight, None),
                       up)}

    def with_bwd(fwd, mod):
        def step():
            x.grad = None
            mod.zero_grad(set_to_none=True)
            fwd().backward(go)
        return step

    def no_grad(fwd):
        def step():
            with torch.no_grad():
                return fwd()
        return step

    out = {k: (no_grad(f), with_bwd(f, m)) for k, (f, m) in fwds.items()}
    out['stream'] = (lambda: C.bn3d_normalize(xs, mr, gamma, beta, False),
                     None)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=50,
                    help='calls per timed block')
    ap.add_argument('--repeats', type=int, default=5,
                    help='alternating blocks per version')
    ap.add_argument('--out', default='profiles/deconv_ab.md',
                    help='write the table here too')
    args = ap.parse_args()
    ops.require_native()
    dev = torch.device('cuda:0')

    lines = ['| shape | pass | version | ms median | min..max | '
             'fwd HBM GB/s | of 8 TB/s | max abs diff vs lib |',
             '|---|---|---|---|---|---|---|---|']
    for n, cin, cout, side in SHAPES:
        vers = versions(n, cin, cout, side, dev)
        shape = f'{n}x{cin}->{cout} {side}^3->{2 * side}^3'
        fwd_bytes = 2.0 * n * side ** 3 * (cin + 8 * cout)
        try:
            with torch.no_grad():
                ref = vers['lib'][0]().float()
                diff = (vers['ops'][0]().float() - ref).abs().max().item()
            vers['lib'][1]()
            diff = f'{diff:.4g}'
        except RuntimeError as e:       # the library has no such kernel
            print(f'{shape}: lib failed: {e}', flush=True)
            del vers['lib']
            diff = 'lib failed'
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
            for k in live:
                t = times[k]
                med = statistics.median(t)
                if p == 0 and k != 'upconv':
                    rate = fwd_bytes / (med * 1e-3)
                    bw = (f'{rate / 1e9:.0f} | '
                          f'{100 * rate / HBM_BYTES_PER_S:.1f}%')
                else:
                    bw = '- | -'
                lines.append(
                    f"| {shape} | {'fwd+bwd' if p else 'fwd'} | {k} | "
                    f'{med:.4f} | {min(t):.4f}..{max(t):.4f} | {bw} | '
                    f"{diff if k == 'ops' else '-'} |")
        del vers, live
        torch.cuda.empty_cache()

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
