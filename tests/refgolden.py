"""Recorded outputs of the upstream coinstac-dinunet package (v2.5.3).

The differential tests (test_reference_parity.py, test_reference_e2e.py)
compare our stack against what the upstream package produced on the same
inputs. Those outputs are stored as JSON under tests/golden/ so the tests
need nothing outside the repository; tools/make_reference_golden.py
regenerates them from an upstream checkout. The case tables below are the
single source for both the generator and the tests.
"""
import json
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          'golden')

RATIO_CASES = [(20, (0.6, 0.2, 0.2)), (17, (0.7, 0.15, 0.15)),
               (9, (0.5, 0.5)), (33, (0.8, 0.1, 0.1))]
KFOLD_CASES = [(20, 4), (18, 3), (23, 5)]
PERF_CASES = [('maximize', [0.5, 0.6, 0.60005, 0.7, 0.69, 0.7001]),
              ('minimize', [1.0, 0.9, 0.89995, 0.5, 0.51, 0.4999])]
SAMPLER_CASES = [(10, 4, True, False), (13, 4, False, False),
                 (3, 8, True, False), (10, 4, True, True)]
CONFIG_KEYS = ('batch_size', 'epochs', 'learning_rate', 'local_iterations',
               'data_dir', 'num_folds', 'task_id', 'mode', 'agg_engine')

# keyword set shared by every end-to-end run (both stacks)
E2E_KW = dict(task_id='tab', batch_size=4, epochs=2, validation_epochs=1,
              local_iterations=1, split_ratio=(0.6, 0.2, 0.2),
              data_dir='data', num_class=2, seed_all=True, patience=2,
              verbose=False)


def files(n, prefix='subj'):
    return [f'{prefix}_{i:03d}.npy' for i in range(n)]


def perf_cache(direction):
    return {'metric_direction': direction, 'patience': 2, 'epochs': 10,
            'best_val_epoch': 0,
            'best_val_score': 0 if direction == 'maximize' else 1e11}


def config_spec():
    spec = {
        'task_id': 'tsk', 'mode': 'train', 'agg_engine': 'dSGD',
        'batch_size': 16,                       # platform input
        'tsk_args': {'epochs': 7, 'learning_rate': 0.005},
        'dSGD_args': {'local_iterations': 3},
        'tsk_data_conf': {'batch_size': 99,      # loses: already in input?
                          'data_dir': 'vols', 'num_folds': 4},
    }
    kw = dict(task_id='tsk', mode='train', batch_size=4, epochs=2,
              local_iterations=1, split_ratio=(0.8, 0.1, 0.1),
              data_dir='data', num_class=2, verbose=False)
    return spec, kw


def init_model():
    torch.manual_seed(42)
    return torch.nn.Sequential(
        torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8),
        torch.nn.Flatten(), torch.nn.Linear(8, 4))


def plain(x):
    """JSON-ready copy: tensors/arrays -> nested lists, numpy scalars ->
    python numbers (exact: float32/float64 widen without rounding), tuples
    -> lists, str-subclass enums -> their plain value."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().tolist()
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, str):
        return x + ''  # the value of a str-subclass enum, not its repr
    return x


def split_dir_contents(d):
    return {f: json.load(open(os.path.join(d, f)))
            for f in sorted(os.listdir(d))}


def named_params(net):
    return [[n, plain(p)] for n, p in net.named_parameters()]


def load(name):
    with open(os.path.join(GOLDEN_DIR, name + '.json')) as f:
        return json.load(f)
