"""Regenerate tests/golden/reference_{parity,e2e}.json.

Runs the UPSTREAM coinstac-dinunet package (v2.5.3) as a black-box oracle
on the inputs listed in tests/refgolden.py and records what it returns;
the differential tests then compare our stack against these records.

    python tools/make_reference_golden.py --reference /path/to/coinstac-dinunet

Only recorded results are written (lists of names, numbers, weights);
nothing of the upstream program text is copied.
"""
import argparse
import itertools
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

import refgolden as G  # noqa: E402


class _FakePool:
    """starmap-only stand-in for the platform's multiprocessing pool."""

    @staticmethod
    def starmap(fn, iterable):
        return list(itertools.starmap(fn, iterable))


def import_reference(root):
    if 'cv2' not in sys.modules:  # optional upstream dependency, unused here
        cv2 = types.ModuleType('cv2')
        cv2.createCLAHE = lambda **kw: None
        sys.modules['cv2'] = cv2
    if not hasattr(np, 'float'):  # upstream uses the numpy<2 alias
        np.float = float
    sys.path.insert(0, root)
    import coinstac_dinunet  # noqa: F401


# --------------------------------------------------------------- parity ----
def parity():
    from coinstac_dinunet import COINNLocal as RefLocal
    from coinstac_dinunet.data import datautils as ref_du
    from coinstac_dinunet.data.data import COINNPaddedDataSampler as RefS
    from coinstac_dinunet.metrics import (AUCROCMetrics, COINNAverages,
                                          ConfusionMatrix, Prf1a)
    from coinstac_dinunet.utils.tensorutils import initialize_weights
    from coinstac_dinunet.utils.utils import (performance_improved_,
                                              stop_training_)
    out = {}

    out['ratio_split'] = {}
    for n, ratio in G.RATIO_CASES:
        with tempfile.TemporaryDirectory() as d:
            ref_du.create_ratio_split(G.files(n), {'split_dir': d,
                                                   'split_ratio': list(ratio)})
            out['ratio_split'][str(n)] = G.split_dir_contents(d)

    out['kfold_split'] = {}
    for n, k in G.KFOLD_CASES:
        with tempfile.TemporaryDirectory() as d:
            ref_du.create_k_fold_splits(G.files(n), {'num_folds': k,
                                                     'split_dir': d})
            out['kfold_split'][f'{n}-{k}'] = G.split_dir_contents(d)

    out['performance'] = {}
    for direction, scores in G.PERF_CASES:
        cache, trace = G.perf_cache(direction), []
        for ep, sc in enumerate(scores):
            improved = performance_improved_(ep, sc, cache)
            stop = stop_training_(ep, cache)
            trace.append({'improved': improved, 'stop': stop,
                          'cache': G.plain(dict(cache))})
        out['performance'][direction] = trace

    rng = np.random.RandomState(7)
    ra, rb = Prf1a(), Prf1a()
    for m in (ra, rb):
        for _ in range(3):
            pred = torch.from_numpy(rng.randint(0, 2, 50))
            true = torch.from_numpy(rng.randint(0, 2, 50))
            m.add(pred.clone(), true.clone())
    p = {'serialize': G.plain(ra.serialize()),
         'scores': G.plain([ra.f1, ra.accuracy, ra.precision, ra.recall])}
    ra.accumulate(rb)
    p['accumulated'] = G.plain(ra.serialize())
    rr = Prf1a()
    rr.reduce_sites([[0.8, 0.7, 0.9], [0.6, 0.5, 0.4]])
    p['reduced'] = G.plain(rr.serialize())
    p['reduced_f1_acc'] = G.plain([rr.f1, rr.accuracy])
    out['prf1a'] = p

    ra = COINNAverages(num_averages=2)
    for v, n, i in [(0.5, 4, 0), (0.25, 8, 1), (1.5, 2, 0)]:
        ra.add(v, n, index=i)
    a = {'serialize': G.plain(ra.serialize()), 'get': G.plain(ra.get())}
    rred = COINNAverages(num_averages=2)
    rred.reduce_sites([ra.serialize(), [[1.0, 2.0], [3, 5]]])
    a['reduced'] = G.plain(rred.serialize())
    out['averages'] = a

    rng = np.random.RandomState(11)
    rc = ConfusionMatrix(num_classes=3)
    for _ in range(3):
        pred = torch.from_numpy(rng.randint(0, 3, 60))
        true = torch.from_numpy(rng.randint(0, 3, 60))
        rc.add(pred.clone(), true.clone())
    out['confusion'] = {
        'matrix': G.plain(rc.matrix.long()),
        'accuracy': G.plain(rc.accuracy()),
        'f1_avg': G.plain(rc.f1(average=True)),
        'precision': G.plain(rc.precision(average=False)),
        'recall': G.plain(rc.recall(average=False))}

    out['sampler'] = []
    for n, bs, shuffle, drop_last in G.SAMPLER_CASES:
        rs = RefS(list(range(n)), bs, seed=5, shuffle=shuffle,
                  drop_last=drop_last)
        seqs = []
        for epoch in range(3):
            rs.set_epoch(epoch)
            seqs.append(G.plain(list(iter(rs))))
        out['sampler'].append({'epochs': seqs, 'len': len(rs)})

    m = G.init_model()
    torch.manual_seed(99)
    initialize_weights(m)
    out['init_weights'] = [G.plain(p) for p in m.parameters()]

    spec, kw = G.config_spec()
    with tempfile.TemporaryDirectory() as d:
        cache = {}
        RefLocal(cache=cache, input=dict(spec), state={
            'clientId': 'local0', 'baseDirectory': d, 'transferDirectory': d,
            'outputDirectory': d, 'cacheDirectory': d}, **kw)
    out['config'] = {k: G.plain(cache.get(k)) for k in G.CONFIG_KEYS}

    rng = np.random.RandomState(5)
    ra = AUCROCMetrics()
    for _ in range(3):
        prob = torch.from_numpy(rng.rand(40).astype(np.float32))
        true = torch.from_numpy((rng.rand(40) > 0.4).astype(np.int64))
        ra.add(prob.clone(), true.clone())
    rr = AUCROCMetrics()
    rr.reduce_sites([0.7, 0.9])
    out['aucroc'] = {'auc': G.plain(ra.auc()),
                     'serialize': G.plain(ra.serialize()),
                     'reduced_auc': G.plain(rr.auc())}
    return out


# ------------------------------------------------------------------ e2e ----
def _reference_classes():
    """Upstream-API computation: same module arch as our TabularTrainer."""
    from coinstac_dinunet import COINNDataset as RefDataset
    from coinstac_dinunet import COINNTrainer as RefTrainer
    from coinstac_dinunet_amd.models import FreeSurferMLP

    class RefTabularDataset(RefDataset):
        def load_index(self, file):
            self.indices.append(file)

        def __getitem__(self, ix):
            rec = np.load(os.path.join(self.state['baseDirectory'],
                                       self.cache.get('data_dir', 'data'),
                                       self.indices[ix]),
                          allow_pickle=True).item()
            return {'inputs': torch.from_numpy(rec['x']),
                    'labels': torch.tensor(rec['y'], dtype=torch.long)}

    class RefTabularTrainer(RefTrainer):
        def _init_nn_model(self):
            self.nn['net'] = FreeSurferMLP(in_features=16,
                                           hidden_sizes=(32, 16),
                                           num_class=2, dropout=0.0)

        def iteration(self, batch):
            dev = self.device.get('gpu', torch.device('cpu'))
            inputs = batch['inputs'].to(dev).float()
            labels = batch['labels'].to(dev).long()
            out = self.nn['net'](inputs)
            loss = torch.nn.functional.cross_entropy(out, labels)
            pred = torch.argmax(out, 1)
            avg = self.new_averages()
            avg.add(loss.item(), len(inputs))
            metrics = self.new_metrics()
            metrics.add(pred, labels)
            return {'loss': loss, 'averages': avg, 'metrics': metrics,
                    'output': pred}

    return RefTabularTrainer, RefTabularDataset


def _run_reference(kw, seed, sizes, max_rounds):
    from coinstac_dinunet import COINNLocal as RefLocal
    from coinstac_dinunet import COINNRemote as RefRemote
    from coinstac_dinunet_amd.simulator import LoopbackCluster
    from computations import make_site_data

    rtc, rdc = _reference_classes()
    tmp = tempfile.TemporaryDirectory()
    c = LoopbackCluster(
        tmp.name, n_sites=2,
        site_data=lambda s: make_site_data(s.as_dict(),
                                           n_samples=sizes[s.clientId],
                                           seed=int(s.clientId[-1])))
    c.remote_cache['seed'] = seed
    ok, _ = c.run(
        lambda cache, input, state: RefLocal(cache=cache, input=input,
                                             state=state, mode='train', **kw),
        lambda cache, input, state: RefRemote(cache=cache, input=input,
                                              state=state),
        rtc, dataset_cls=rdc, mp_pool=_FakePool(), max_rounds=max_rounds)
    c._tmp = tmp  # keep the run directory alive with the cluster
    return bool(ok), c


def e2e():
    from coinstac_dinunet.config.keys import Phase as RefPhase
    from coinstac_dinunet_amd.config.keys import Key
    out = {}
    even = {'local0': 20, 'local1': 20}

    ok, c = _run_reference(dict(G.E2E_KW), 2024, even, 400)
    out['dsgd'] = {
        'ok': ok, 'rounds': c.rounds,
        'global_test': G.plain(c.remote_cache[Key.GLOBAL_TEST_SERIALIZABLE]),
        'params': [G.named_params(c.site_caches[i]['nn']['net'])
                   for i in range(2)]}

    kw = dict(G.E2E_KW)
    kw.update(split_ratio=None, num_folds=3, epochs=1, patience=1)
    ok, c = _run_reference(kw, 7, {'local0': 18, 'local1': 18}, 700)
    out['kfold'] = {
        'ok': ok,
        'global_test': G.plain(c.remote_cache[Key.GLOBAL_TEST_SERIALIZABLE])}

    kw = dict(G.E2E_KW)
    kw.update(pretrain_args={'epochs': 1})
    ok, c = _run_reference(kw, 7, {'local0': 12, 'local1': 28}, 60)
    out['pretrain'] = {
        'ok': ok,
        'site0_phase': G.plain(c.site_inputs[0].get('phase')),
        'phase_pre_computation': G.plain(RefPhase.PRE_COMPUTATION),
        'pretrain_flags': [c.site_caches[i].get('pretrain')
                           for i in range(2)]}

    kw = dict(G.E2E_KW)
    kw.update(agg_engine='powerSGD', matrix_approximation_rank=2,
              start_powerSGD_iter=2, epochs=2)
    ok, c = _run_reference(kw, 5, even, 500)
    out['powersgd'] = {
        'ok': ok, 'rounds': c.rounds,
        'params': [G.named_params(c.site_caches[i]['nn']['net'])
                   for i in range(2)]}

    kw = dict(G.E2E_KW)
    kw.update(agg_engine='rankDAD', dad_reduction_rank=3, epochs=1,
              patience=1)
    ok, c = _run_reference(kw, 5, even, 500)
    out['rankdad'] = {
        'ok': ok, 'rounds': c.rounds,
        'global_test': G.plain(c.remote_cache[Key.GLOBAL_TEST_SERIALIZABLE])}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reference', required=True,
                    help='checkout of upstream coinstac-dinunet v2.5.3')
    args = ap.parse_args()
    import_reference(os.path.abspath(args.reference))
    os.makedirs(G.GOLDEN_DIR, exist_ok=True)
    for name, fn in (('reference_parity', parity), ('reference_e2e', e2e)):
        path = os.path.join(G.GOLDEN_DIR, name + '.json')
        with open(path, 'w') as f:
            json.dump(fn(), f, indent=1, sort_keys=True)
            f.write('\n')
        print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
