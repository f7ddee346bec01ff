"""Differential parity: the UPSTREAM reference implementation against ours
on identical inputs, demanding identical outputs — split generation,
checkpoint-best predicates, and the metric serialize/reduce_sites protocol
are the behaviors COINSTAC computations depend on bit-for-bit.

The reference is a black-box oracle whose outputs on these inputs are
recorded in tests/golden/reference_parity.json (regenerate with
tools/make_reference_golden.py); inputs and case tables are shared through
tests/refgolden.py, so the tests run anywhere without an upstream checkout.
"""
import numpy as np
import pytest
import torch

import refgolden as G


@pytest.fixture(scope='module')
def ref():
    """What the reference package returned (read-only)."""
    return G.load('reference_parity')


@pytest.mark.parametrize('n,ratio', G.RATIO_CASES)
def test_ratio_split_bitwise(ref, tmp_path, n, ratio):
    from coinstac_dinunet_amd.data import datautils as our_du
    b = tmp_path / 'ours'
    b.mkdir()
    our_du.create_ratio_split(G.files(n), {'split_dir': str(b),
                                           'split_ratio': list(ratio)})
    want, got = ref['ratio_split'][str(n)], G.split_dir_contents(str(b))
    assert sorted(want) == sorted(got)
    for f in want:
        assert want[f] == got[f], f'{f} differs'


@pytest.mark.parametrize('n,k', G.KFOLD_CASES)
def test_kfold_split_bitwise(ref, tmp_path, n, k):
    from coinstac_dinunet_amd.data import datautils as our_du
    b = tmp_path / 'ours'
    b.mkdir()
    our_du.create_k_fold_splits(G.files(n), {'num_folds': k,
                                             'split_dir': str(b)})
    want, got = ref['kfold_split'][f'{n}-{k}'], G.split_dir_contents(str(b))
    assert sorted(want) == sorted(got) and len(got) == k
    for f in want:
        assert want[f] == got[f], f
    # every fold partitions the full set
    for f, s in got.items():
        assert sorted(s['train'] + s['validation'] + s['test']) == \
            sorted(G.files(n))


@pytest.mark.parametrize('direction,scores', G.PERF_CASES)
def test_performance_improved_matches(ref, direction, scores):
    from coinstac_dinunet_amd.utils.utils import (performance_improved_ as op,
                                                  stop_training_ as os_)
    trace = ref['performance'][direction]
    assert len(trace) == len(scores)
    cb = G.perf_cache(direction)
    for ep, sc in enumerate(scores):
        assert trace[ep]['improved'] == op(ep, sc, cb), (ep, sc)
        assert trace[ep]['stop'] == os_(ep, cb), (ep, sc)
        assert trace[ep]['cache'] == G.plain(cb)  # identical cache mutations


def test_prf1a_protocol_matches(ref):
    from coinstac_dinunet_amd.metrics import Prf1a as OurP
    want = ref['prf1a']
    rng = np.random.RandomState(7)
    oa, ob = OurP(), OurP()
    for m_our in (oa, ob):
        for _ in range(3):
            pred = torch.from_numpy(rng.randint(0, 2, 50))
            true = torch.from_numpy(rng.randint(0, 2, 50))
            m_our.add(pred.clone(), true.clone())
    assert want['serialize'] == G.plain(oa.serialize())
    assert want['scores'] == \
        G.plain([oa.f1, oa.accuracy, oa.precision, oa.recall])
    # accumulate parity
    oa.accumulate(ob)
    assert want['accumulated'] == G.plain(oa.serialize())
    # reduce_sites parity (mutates the instance; serialized site scores
    # -> floor values)
    site_scores = [[0.8, 0.7, 0.9], [0.6, 0.5, 0.4]]
    ro = OurP()
    ro.reduce_sites(site_scores)
    assert want['reduced'] == G.plain(ro.serialize())
    assert want['reduced_f1_acc'] == G.plain([ro.f1, ro.accuracy])


def test_averages_protocol_matches(ref):
    from coinstac_dinunet_amd.metrics import COINNAverages as OurA
    want = ref['averages']
    oa = OurA(num_averages=2)
    for v, n, i in [(0.5, 4, 0), (0.25, 8, 1), (1.5, 2, 0)]:
        oa.add(v, n, index=i)
    assert want['serialize'] == G.plain(oa.serialize())
    np.testing.assert_allclose(np.asarray(want['get'], dtype=float),
                               np.asarray(oa.get(), dtype=float))
    sites = [want['serialize'], [[1.0, 2.0], [3, 5]]]
    ored = OurA(num_averages=2)
    ored.reduce_sites(sites)
    assert want['reduced'] == G.plain(ored.serialize())


def test_confusion_matrix_protocol_matches(ref):
    """The reference indexes matrix[pred][true], so its precision()/
    recall() are swapped vs the standard definitions we use — accuracy and
    macro-F1 are invariant under that swap (F1 is symmetric in p<->r). Pin
    exactly that equivalence."""
    from coinstac_dinunet_amd.metrics import ConfusionMatrix as OurC
    want = ref['confusion']
    rng = np.random.RandomState(11)
    oc = OurC(num_classes=3)
    for _ in range(3):
        pred = torch.from_numpy(rng.randint(0, 3, 60))
        true = torch.from_numpy(rng.randint(0, 3, 60))
        oc.add(pred.clone(), true.clone())
    # transposed layouts
    assert torch.equal(torch.tensor(want['matrix']), oc.matrix.t())
    np.testing.assert_allclose(want['accuracy'], oc.accuracy, atol=1e-4)
    np.testing.assert_allclose(want['f1_avg'],
                               oc.f1(average=True), atol=1e-4)
    # the reference's 'precision' is the standard recall and vice versa
    np.testing.assert_allclose(want['precision'],
                               oc.recall(average=False), atol=1e-4)
    np.testing.assert_allclose(want['recall'],
                               oc.precision(average=False), atol=1e-4)


@pytest.mark.parametrize('n,bs,shuffle,drop_last', G.SAMPLER_CASES)
def test_padded_sampler_sequences_match(ref, n, bs, shuffle, drop_last):
    """Identical padded index sequences per (seed, epoch) — the property
    lock-step batch counts depend on."""
    from coinstac_dinunet_amd.data.data import COINNPaddedDataSampler as OurS
    want = ref['sampler'][G.SAMPLER_CASES.index((n, bs, shuffle, drop_last))]
    os_ = OurS(list(range(n)), bs, seed=5, shuffle=shuffle,
               drop_last=drop_last)
    for epoch in range(3):
        os_.set_epoch(epoch)
        assert want['epochs'][epoch] == G.plain(list(iter(os_))), epoch
    assert want['len'] == len(os_)


def test_initialize_weights_bitwise(ref):
    """Same torch seed => bit-identical Kaiming init on the module types
    the reference covers (Conv2d/Linear/BatchNorm2d)."""
    from coinstac_dinunet_amd.utils.tensorutils import (initialize_weights
                                                        as oi)
    mb = G.init_model()
    torch.manual_seed(99), oi(mb)
    want = ref['init_weights']
    assert len(want) == len(list(mb.parameters()))
    for pa, pb in zip(want, mb.parameters()):
        assert torch.equal(torch.tensor(pa, dtype=pb.dtype), pb)


def test_config_precedence_matches(ref, tmp_path):
    """Three-source hyperparameter resolution (platform input >
    {task}_args > {engine}_args > {task}_data_conf > ctor defaults) must
    cache identical values in both stacks."""
    from coinstac_dinunet_amd import COINNLocal as OurLocal
    spec, kw = G.config_spec()
    cache = {}
    OurLocal(cache=cache, input=dict(spec), state={
        'clientId': 'local0', 'baseDirectory': str(tmp_path),
        'transferDirectory': str(tmp_path),
        'outputDirectory': str(tmp_path),
        'cacheDirectory': str(tmp_path)}, **kw)
    for k in G.CONFIG_KEYS:
        assert ref['config'][k] == G.plain(cache.get(k)), \
            (k, ref['config'][k], cache.get(k))


def test_aucroc_protocol_matches(ref):
    from coinstac_dinunet_amd.metrics import AUCROCMetrics as OurA
    want = ref['aucroc']
    rng = np.random.RandomState(5)
    oa = OurA()
    for _ in range(3):
        prob = torch.from_numpy(rng.rand(40).astype(np.float32))
        true = torch.from_numpy((rng.rand(40) > 0.4).astype(np.int64))
        oa.add(prob.clone(), true.clone())
    # reference exposes auc() as a method; ours as a property
    assert abs(want['auc'] - oa.auc) < 1e-6
    np.testing.assert_allclose(np.asarray(want['serialize'], dtype=float),
                               np.asarray(oa.serialize(), dtype=float),
                               atol=1e-5)
    ro = OurA()
    ro.reduce_sites([0.7, 0.9])
    assert abs(want['reduced_auc'] - ro.auc) < 1e-9
