"""Flagship benchmark: VBM 3D-CNN dSGD training step (BASELINE.json).

Measures whole-node samples/sec for the decentralized-SGD training round:
per step = local fwd/bwd on synthetic 64^3 volumes (bf16 autocast) +
bucketed RCCL all-reduce(avg) of the flat gradient arena overlapped with
backward + fused-Adam update. One process per GPU "site" (weak scaling:
per-GPU batch fixed as N grows).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`;
launched via torch.distributed.run for N>1. Rank 0 prints ONE JSON line.

A plain run does only what the headline figure needs: set up, warm up,
time the K steps, optionally write the last step's outputs
(`--dump-outputs DIR`), print the result line. Secondary measurements
belong behind `--full` (off by default); there are none at present, so
`--full` currently runs the same path. Model weights and the synthetic
batch come from a fixed seed, so two runs with the same arguments see
identical inputs and their dumped outputs can be compared array by array.
"""
import argparse
import json
import os
import time

import torch

SEED = 20240917
# per-array cap for --dump-outputs (16 MB as float32, so a dump stays well
# under 64 MB); a larger array is stored as a fixed seeded sample
DUMP_MAX_ELEMS = 4 * 1024 * 1024


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    # default region ~3.5 s on 1 GPU: long enough that driver-side
    # utilization sampling lands inside it, still < minutes
    ap.add_argument('--steps', type=int, default=80)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=64,
                    help='per-GPU (per-site) batch size')
    ap.add_argument('--vol', type=int, default=64, help='volume side length')
    ap.add_argument('--local-iterations', type=int, default=1)
    ap.add_argument('--model', type=str, default='vbm',
                    choices=['vbm', 'mlp', 'resnet18'])
    ap.add_argument('--stock', action='store_true',
                    help='stock torch ops (MIOpen conv/BN) for comparison')
    ap.add_argument('--graph', type=int, default=1, choices=[0, 1],
                    help='hipGraph-capture the fwd+loss+bwd inner loop '
                         '(single-rank only; collectives and the optimizer '
                         'stay outside the capture)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps write what the last timed '
                         'step returned to its caller (logits, loss) as '
                         'DIR/<name>.npy (float32)')
    ap.add_argument('--full', action='store_true',
                    help='also run the secondary measurements (none at '
                         'present: the plain run is already headline-only)')
    return ap.parse_args()


def dump_outputs(dirname, arrays):
    """Write each tensor as float32 `dirname/<name>.npy`. Arrays above
    DUMP_MAX_ELEMS are flattened and reduced to a fixed seeded sample of
    their elements (same indices every run, ascending order)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().to(device='cpu', dtype=torch.float32).numpy()
        if a.size > DUMP_MAX_ELEMS:
            idx = np.random.RandomState(SEED % (2 ** 32)).choice(
                a.size, DUMP_MAX_ELEMS, replace=False)
            a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(dirname, name + '.npy'),
                np.ascontiguousarray(a))


def build_model(args, device):
    from coinstac_dinunet_amd.models import FreeSurferMLP, ResNet18, VBMNet
    if args.model == 'vbm':
        if args.stock:
            import coinstac_dinunet_amd.models.vbm as _vbm
            import torch.nn as _nn

            class _StockBlock(_nn.Module):
                def __init__(self, cin, cout, stride=1):
                    super().__init__()
                    self.conv = _nn.Conv3d(cin, cout, 3, stride=stride,
                                           padding=1, bias=False)
                    self.bn = _nn.BatchNorm3d(cout)
                    self.act = _nn.ReLU(inplace=True)

                def forward(self, x):
                    return self.act(self.bn(self.conv(x)))

            _orig = _vbm._ConvBlock
            _vbm._ConvBlock = _StockBlock
            net = VBMNet(in_channels=1, num_class=2)
            _vbm._ConvBlock = _orig
        else:
            net = VBMNet(in_channels=1, num_class=2)
        data = torch.randn(args.batch, 1, args.vol, args.vol, args.vol)
    elif args.model == 'mlp':
        net = FreeSurferMLP(in_features=66, num_class=2)
        data = torch.randn(args.batch, 66)
    else:
        if args.stock:
            # library-op ResNet-18 (MIOpen convs, eager BN) for comparison
            import torch.nn as _nn
            import coinstac_dinunet_amd.models.resnet as _rn

            class _StockBN(_nn.BatchNorm2d):
                def __init__(self, c, relu=False, **kw):
                    super().__init__(c, **kw)
                    self._relu = relu

                def forward(self, x):
                    y = super().forward(x)
                    return _nn.functional.relu(y) if self._relu else y

            o_conv, o_bn = _rn.OpsConv2d, _rn.OpsBatchNorm2d
            _rn.OpsConv2d, _rn.OpsBatchNorm2d = _nn.Conv2d, _StockBN
            try:
                net = ResNet18(in_channels=3, num_class=10)
            finally:
                _rn.OpsConv2d, _rn.OpsBatchNorm2d = o_conv, o_bn
        else:
            net = ResNet18(in_channels=3, num_class=10)
        data = torch.randn(args.batch, 3, 224, 224)
    labels = torch.randint(0, 2, (args.batch,))
    return net.to(device), data.to(device), labels.to(device)


def main():
    args = parse_args()
    from coinstac_dinunet_amd import ops
    from coinstac_dinunet_amd.parallel.engine import (FlatGradBuffer,
                                                      init_distributed)

    rank, world = init_distributed()
    on_gpu = torch.cuda.is_available()
    local = int(os.environ.get('LOCAL_RANK', 0))
    device = torch.device(
        f"cuda:{local % max(1, torch.cuda.device_count())}"
        if on_gpu else 'cpu')
    if on_gpu:
        torch.cuda.set_device(device)
        torch.backends.cudnn.benchmark = True

    torch.manual_seed(SEED)  # same weights + batch on every run and rank
    net, data, labels = build_model(args, device)
    comm_stream = torch.cuda.Stream() if on_gpu else None
    buf = FlatGradBuffer(net.parameters(), world_size=world,
                         comm_stream=comm_stream)
    if on_gpu and ops.native_available():
        opt = ops.FusedAdam(net.parameters(), lr=1e-3)
    else:
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)

    import torch.distributed as dist

    last = {}  # logits/loss of the most recent fwd_bwd (static under replay)

    def fwd_bwd(sync):
        buf.zero_()
        buf.begin_round(sync=sync)
        if on_gpu:
            with torch.autocast('cuda', dtype=torch.bfloat16):
                out = net(data)
            loss = ops.cross_entropy(out.float(), labels)
        else:
            out = net(data)
            loss = ops.cross_entropy(out, labels)
        last['logits'], last['loss'] = out.detach(), loss.detach()
        loss.backward()

    def one_step():
        for li in range(args.local_iterations):
            fwd_bwd(sync=(li == args.local_iterations - 1))
        buf.finish_round()
        opt.step()

    # warmup (also primes autotuners before any graph capture)
    for _ in range(args.warmup):
        one_step()

    # hipGraph capture of the launch-bound fwd+loss+bwd region: ResNet-18
    # dispatches ~1100 kernels/step, VBM ~465 — replay removes the launch
    # gaps. Single-rank + single-micro-batch only (collectives inside a
    # capture need a cooperating RCCL setup; optimizer stays eager so its
    # per-step bias correction keeps advancing).
    graphed = (args.graph and on_gpu and world == 1
               and args.local_iterations == 1)
    if graphed:
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            fwd_bwd(sync=False)

        def one_step():  # noqa: F811 — replay + eager optimizer
            g.replay()
            opt.step()

        for _ in range(3):  # graph warmup
            one_step()

    if dist.is_initialized():
        dist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    if on_gpu:
        torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
    elapsed = time.perf_counter() - t0

    # MAX over ranks (slowest rank defines the lock-step round time);
    # the tensor must live on the device for the RCCL backend
    t = torch.tensor([elapsed], dtype=torch.float64,
                     device=device if on_gpu else 'cpu')
    if dist.is_initialized() and world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())

    ms_per_step = elapsed / args.steps * 1000.0
    samples_per_sec = args.batch * world * args.steps / elapsed

    if rank == 0 and args.dump_outputs:
        # What the step hands its caller. They depend on every weight
        # update of the steps before, so they cover the whole path. The
        # weights themselves are left out: at lr 1e-3 on one fixed noise
        # batch the early VBM layers go non-finite within ~10 steps (the
        # fused ReLU masks them), which makes them useless for comparing.
        dump_outputs(args.dump_outputs, {'logits': last['logits'],
                                         'loss': last['loss']})

    if rank == 0:
        print(json.dumps({
            'metric': 'samples/sec (whole node), VBM 3D-CNN dSGD'
                      if args.model == 'vbm' else
                      f'samples/sec (whole node), {args.model} dSGD',
            'value': round(samples_per_sec, 3),
            'unit': 'samples/sec',
            'n_gpus': world,
            'steps': args.steps,
            'warmup': args.warmup,
            'ms_per_step': round(ms_per_step, 3),
            'higher_is_better': True,
            'scaling': 'weak',
            'vs_baseline': None,
            'dtype': 'bf16' if on_gpu else 'fp32',
            'data': 'synthetic',
            'config': {
                'model': args.model,
                'global_batch': args.batch * world,
                'volume': f'{args.vol}^3' if args.model == 'vbm' else None,
                'local_iterations': args.local_iterations,
                'parallelism': f'dsgd-dp{world}',
                'hipgraph': bool(graphed),
                # BASELINE.json names "wall-clock/epoch" too: derived for a
                # nominal 1024-sample per-site epoch at this step time
                'wallclock_per_epoch_s_1024spp': round(
                    -(-1024 // args.batch) * ms_per_step / 1000.0, 3),
            },
        }))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
