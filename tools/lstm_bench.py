"""A/B of ops.OpsLSTM (persistent recurrence kernels, lstm.hip) against
nn.LSTM through the library.

    python tools/lstm_bench.py [--iters 10] [--repeats 3] \
        [--out profiles/lstm_ab.md]

One layer, I = 256, T in {16, 128, 512}, B in {16, 64}, H in {64, 128, 256},
one and two directions, fp32 and bf16 (module and input in that dtype).
forward-only (no_grad) and forward + backward (gradients to x and every
parameter). The two versions hold the same weights, run in one process in
alternating blocks of calls timed with device events; the table gives the
median block and the min..max spread over --repeats blocks, per call.
H = 256 is the streamed-weight instance, H <= 128 the register-stationary
one. A run without a GPU fails.
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

STEPS = (16, 128, 512)
BATCHES = (16, 64)
HIDDEN = (64, 128, 256)
INPUT = 256


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
            return mod(x)[0]

    def fwd_bwd():
        x.grad = None
        mod.zero_grad(set_to_none=True)
        mod(x)[0].backward(go)
    return fwd, fwd_bwd


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=10,
                    help='calls per timed block')
    ap.add_argument('--repeats', type=int, default=3,
                    help='alternating blocks per version')
    ap.add_argument('--out', default='profiles/lstm_ab.md',
                    help='write the table here too')
    args = ap.parse_args()
    ops.require_native()
    dev = torch.device('cuda:0')
    lines = [f'calls per block: {args.iters}, blocks per version: '
             f'{args.repeats}, device: {torch.cuda.get_device_name(0)}', '',
             '| T | B | H | dirs | dtype | pass | ops ms median | min..max | '
             'lib ms median | min..max | lib / ops time | '
             'max abs y diff vs lib |',
             '|---|---|---|---|---|---|---|---|---|---|---|---|']

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
    for dtype in (torch.float32, torch.bfloat16):
        for dirs in (1, 2):
            for H in HIDDEN:
                torch.manual_seed(H + dirs)
                m_ops = ops.OpsLSTM(INPUT, H, bidirectional=dirs == 2)
                m_lib = nn.LSTM(INPUT, H, bidirectional=dirs == 2)
                m_lib.load_state_dict(m_ops.state_dict())
                m_ops, m_lib = m_ops.to(dev, dtype), m_lib.to(dev, dtype)
                for T in STEPS:
                    for B in BATCHES:
                        gen = torch.Generator().manual_seed(T + B)
                        x = torch.randn(T, B, INPUT, generator=gen)
                        x = x.to(dev, dtype).requires_grad_(True)
                        go = torch.randn(T, B, dirs * H, generator=gen)
                        go = go.to(dev, dtype)
                        live = {'ops': steps(m_ops, x, go),
                                'lib': steps(m_lib, x, go)}
                        diff = (live['ops'][0]().float()
                                - live['lib'][0]().float()).abs().max().item()
                        for p in (0, 1):
                            for fns in live.values():
                                for _ in range(3):
                                    fns[p]()
                            torch.cuda.synchronize()
                            times = {k: [] for k in live}
                            for _ in range(args.repeats):
                                for k, fns in live.items():
                                    times[k].append(
                                        time_block(fns[p], args.iters))
                            med = {k: statistics.median(t)
                                   for k, t in times.items()}
                            name = str(dtype).replace('torch.', '')
                            emit(f"| {T} | {B} | {H} | {dirs} | {name} | "
                                 f"{'fwd+bwd' if p else 'fwd'} | "
                                 f"{med['ops']:.4f} | "
                                 f"{min(times['ops']):.4f}.."
                                 f"{max(times['ops']):.4f} | "
                                 f"{med['lib']:.4f} | "
                                 f"{min(times['lib']):.4f}.."
                                 f"{max(times['lib']):.4f} | "
                                 f"{med['lib'] / med['ops']:.2f} | "
                                 f'{diff:.3g} |')
                        del live, x, go
                del m_ops, m_lib
                torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
