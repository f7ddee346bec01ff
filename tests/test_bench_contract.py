"""Guard the driver's bench.py contract: flags, JSON line, torchrun path."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_KEYS = {'metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup',
                 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
                 'dtype', 'data', 'config'}


def _run(cmd, timeout=300, env=None):
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True,
                       timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, f'expected ONE json line, got {len(lines)}'
    return json.loads(lines[0])


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_torchrun(nproc, bench_args, timeout=420):
    """torchrun with one retry on a fresh port: many-process rendezvous is
    occasionally flaky on a loaded machine; a deterministic failure still
    fails both attempts."""
    cmd = lambda port: [sys.executable, '-m', 'torch.distributed.run',
                        '--nnodes=1', '--nproc-per-node', str(nproc),
                        '--master-addr', '127.0.0.1',
                        '--master-port', str(port), 'bench.py',
                        '--gpus', str(nproc)] + bench_args
    try:
        return _run(cmd(_free_port()), timeout=timeout)
    except (AssertionError, subprocess.TimeoutExpired):
        return _run(cmd(_free_port()), timeout=timeout)


def test_bench_single_process(tmp_path):
    out = _run([sys.executable, 'bench.py', '--steps', '2', '--warmup', '1',
                '--batch', '2', '--vol', '8'])
    assert REQUIRED_KEYS <= set(out)
    assert out['n_gpus'] == 1 and out['steps'] == 2 and out['warmup'] == 1
    assert out['scaling'] == 'weak' and out['data'] == 'synthetic'
    assert out['value'] > 0


def test_bench_torchrun_two_ranks():
    """The driver's N>1 launch shape (gloo here, RCCL on the GPU node)."""
    out = _run_torchrun(2, ['--steps', '2', '--warmup', '1',
                            '--batch', '2', '--vol', '8'])
    assert out['n_gpus'] == 2
    assert out['config']['parallelism'] == 'dsgd-dp2'
    assert out['config']['global_batch'] == 4


def test_bench_mlp_model():
    out = _run([sys.executable, 'bench.py', '--model', 'mlp', '--steps', '2',
                '--warmup', '1', '--batch', '8'])
    assert 'mlp' in out['metric']


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's arrays as float32 .npy;
    same arguments => same inputs => (on the deterministic CPU path) the
    same outputs. --full is accepted and keeps the result line's meaning."""
    import numpy as np
    args = ['--model', 'mlp', '--steps', '3', '--warmup', '1', '--batch', '8']
    # pin the CPU path (bitwise repeatable) even where a GPU is present
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    outs = []
    for sub, extra in (('a', []), ('b', ['--full'])):
        d = tmp_path / sub
        res = _run([sys.executable, 'bench.py'] + args + extra +
                   ['--dump-outputs', str(d)], env=env)
        assert res['dtype'] == 'fp32'
        assert REQUIRED_KEYS <= set(res) and res['steps'] == 3
        assert res['ms_per_step'] > 0
        files = sorted(os.listdir(d))
        assert files == ['logits.npy', 'loss.npy']
        outs.append({f: np.load(d / f) for f in files})
    a, b = outs
    assert a['logits.npy'].shape == (8, 2)
    assert a['loss.npy'].size == 1
    total = 0
    for f in a:
        assert a[f].dtype == np.float32 and np.isfinite(a[f]).all(), f
        assert np.array_equal(a[f], b[f]), f'{f} differs between runs'
        total += a[f].nbytes
    assert total <= 64 * 1024 * 1024
    assert np.abs(a['logits.npy']).max() > 0


def test_bench_dump_sampling_is_fixed():
    """Arrays above the per-array cap are stored as the same seeded sample
    of their elements on every call."""
    import numpy as np
    import tempfile
    import torch
    import bench
    big = torch.arange(bench.DUMP_MAX_ELEMS + 1000, dtype=torch.float32)
    with tempfile.TemporaryDirectory() as d:
        bench.dump_outputs(d, {'big': big, 'small': big[:10].view(2, 5)})
        first = np.load(os.path.join(d, 'big.npy'))
        bench.dump_outputs(d, {'big': big})
        again = np.load(os.path.join(d, 'big.npy'))
        small = np.load(os.path.join(d, 'small.npy'))
    assert first.shape == (bench.DUMP_MAX_ELEMS,) and small.shape == (2, 5)
    assert np.array_equal(first, again)
    assert (np.diff(first) > 0).all()  # distinct source elements, in order


def test_bench_torchrun_eight_ranks():
    """Exactly the driver's SCALE shape at N=8 (gloo on CPU; RCCL on the
    node): rendezvous, device-modulo, MAX-over-ranks, one JSON line."""
    out = _run_torchrun(8, ['--steps', '1', '--warmup', '1',
                            '--batch', '2', '--vol', '8', '--model', 'mlp'])
    assert out['n_gpus'] == 8
    assert out['config']['parallelism'] == 'dsgd-dp8'
    assert out['config']['global_batch'] == 16


def test_bench_stock_model_builders():
    """--stock builders (library-op VBM/ResNet) must keep constructing:
    they are the measured comparison baseline."""
    import argparse
    import torch
    import bench

    for model in ['vbm', 'resnet18']:
        args = argparse.Namespace(model=model, stock=True, batch=2, vol=8)
        net, data, labels = bench.build_model(args, torch.device('cpu'))
        out = net(data)
        assert out.shape[0] == 2
        # stock means NO Ops modules anywhere
        from coinstac_dinunet_amd.ops.conv import OpsConv2d, OpsConv3d
        for m in net.modules():
            assert not isinstance(m, (OpsConv2d, OpsConv3d)), type(m)
