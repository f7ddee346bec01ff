"""End-to-end example: 3D U-Net segmentation on 2 (or N) sites.

The loss and the metrics come straight from the logits: on a GPU the loss
head is the fused HIP kernels of ops/csrc/segloss.hip (no probability or
prediction tensor is materialised), on CPU the same functions fall back to
plain torch.

  --classes 2   one logit plane, ops.dice_loss_with_logits + Prf1a.add_logits
                (binary rule: logit > 0)
  --classes K   K > 2 planes, ops.cross_entropy on the [N, K, D, H, W] logits
                + ConfusionMatrix.add_logits (argmax, lowest index on ties)

Run:
  # 2 emulated sites over the file/JSON relay (CPU, or one GPU if present):
  python examples/unet_segmentation_computation.py --mode loopback

  # N GPU-sites over RCCL, one rank per MI355X:
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 examples/unet_segmentation_computation.py \
      --mode rccl

Data is synthesized: noisy volumes holding one sphere (class 1) and, for
K > 2, an offset box per further class; labels are stored as uint8 and are
read by the kernels in that dtype.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..'))

from coinstac_dinunet_amd import (COINNDataset, COINNLocal, COINNRemote,
                                  COINNTrainer, ops)  # noqa: E402
from coinstac_dinunet_amd.config.keys import Mode  # noqa: E402
from coinstac_dinunet_amd.models import UNet3D  # noqa: E402


class SegDataset(COINNDataset):
    """One .npy record per volume: {'x': float32 [D,H,W], 'y': uint8 [D,H,W]}."""

    def load_index(self, file):
        self.indices.append(file)

    def __getitem__(self, ix):
        rec = np.load(os.path.join(self.path(), self.cache['data_dir'],
                                   self.indices[ix]), allow_pickle=True).item()
        return {'inputs': torch.from_numpy(rec['x']).unsqueeze(0),
                'labels': torch.from_numpy(rec['y'])}


class SegTrainer(COINNTrainer):
    def _init_nn_model(self):
        k = self.cache.get('num_class', 2)
        self.nn['unet'] = UNet3D(in_channels=1, num_class=1 if k == 2 else k,
                                 widths=tuple(self.cache.get('widths',
                                                             (8, 16))))

    def iteration(self, batch):
        dev = self.device['gpu']
        x = batch['inputs'].to(dev).float()
        y = batch['labels'].to(dev)               # uint8, as stored
        logits = self.nn['unet'](x)
        if logits.shape[1] == 1:
            logits = logits.squeeze(1)
            loss = ops.dice_loss_with_logits(logits, y)
        else:
            # the HIP kernel reads uint8 labels; torch's CPU loss wants int64
            loss = ops.cross_entropy(logits, y if y.is_cuda else y.long())
        avg, metrics = self.new_averages(), self.new_metrics()
        avg.add(loss.item(), len(x))
        metrics.add_logits(logits, y)
        return {'loss': loss, 'averages': avg, 'metrics': metrics,
                'output': logits.detach()}


def synthesize(base_dir, n=12, side=16, classes=2, seed=0):
    rng = np.random.RandomState(seed)
    data_dir = os.path.join(base_dir, 'data')
    os.makedirs(data_dir, exist_ok=True)
    g = np.stack(np.meshgrid(*([np.arange(float(side))] * 3), indexing='ij'))
    for i in range(n):
        y = np.zeros((side,) * 3, dtype=np.uint8)
        c = rng.uniform(0.3 * side, 0.7 * side, size=3)
        y[((g - c[:, None, None, None]) ** 2).sum(0) < (0.25 * side) ** 2] = 1
        for k in range(2, classes):
            lo = rng.randint(0, side - side // 4, size=3)
            y[tuple(slice(a, a + side // 4) for a in lo)] = k
        x = (y.astype(np.float32) / max(classes - 1, 1)
             + 0.3 * rng.randn(side, side, side).astype(np.float32))
        np.save(os.path.join(data_dir, f'vol_{i:03d}.npy'),
                {'x': x, 'y': y}, allow_pickle=True)


def local_kw(args):
    return dict(task_id='seg', mode=Mode.TRAIN, batch_size=args.batch,
                epochs=args.epochs, validation_epochs=1, local_iterations=1,
                split_ratio=(0.5, 0.25, 0.25), data_dir='data',
                num_class=args.classes, monitor_metric='f1',
                metric_direction='maximize', seed_all=True,
                patience=args.epochs, verbose=False)


def run_loopback(args):
    from coinstac_dinunet_amd.simulator import LoopbackCluster
    cluster = LoopbackCluster(
        args.root, n_sites=args.sites,
        site_data=lambda s: synthesize(s.baseDirectory, side=args.side,
                                       classes=args.classes,
                                       seed=int(s.clientId[-1])))
    kw = local_kw(args)
    success, _ = cluster.run(
        lambda cache, input, state: COINNLocal(cache=cache, input=input,
                                               state=state, **kw),
        lambda cache, input, state: COINNRemote(cache=cache, input=input,
                                                state=state),
        SegTrainer, dataset_cls=SegDataset, max_rounds=2000)
    print('SUCCESS' if success else 'DID NOT FINISH',
          '| native loss head:', ops.native_available())


def run_rccl(args):
    from coinstac_dinunet_amd.parallel.cluster import RcclCluster
    cluster = RcclCluster(args.root, local_kw=local_kw(args))
    synthesize(cluster.site.baseDirectory, side=args.side,
               classes=args.classes, seed=cluster.rank)
    success, _ = cluster.run(SegTrainer, dataset_cls=SegDataset,
                             max_rounds=2000)
    if cluster.rank == 0:
        print('SUCCESS' if success else 'DID NOT FINISH',
              '| native loss head:', ops.native_available())


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['loopback', 'rccl'],
                    default='loopback')
    ap.add_argument('--root', default='/tmp/seg_run')
    ap.add_argument('--sites', type=int, default=2)
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--side', type=int, default=16)
    ap.add_argument('--classes', type=int, default=2,
                    help='2: binary dice head; K > 2: K-plane cross-entropy')
    args = ap.parse_args()
    {'loopback': run_loopback, 'rccl': run_rccl}[args.mode](args)
