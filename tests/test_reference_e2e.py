"""Whole-protocol differential: the UPSTREAM reference package's
COINNLocal/COINNRemote driven through the in-process loopback relay on the
SAME site data, seeds and hyperparameters as our stack; the two runs must
agree — round count, reduced global scores, and final weights.

This is the strongest drop-in-compatibility statement the CPU can make:
the same user computation (module arch, iteration math) trained by both
frameworks converges to the same model through the same protocol.

The reference side of each run is recorded in
tests/golden/reference_e2e.json (tools/make_reference_golden.py drives the
upstream package and writes it); our side runs live here.
"""
import os
import sys

import numpy as np
import pytest
import torch

TESTS_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, TESTS_DIR)

import refgolden as G  # noqa: E402

_KW = G.E2E_KW


@pytest.fixture(scope='module')
def ref():
    """What the reference runs produced (read-only)."""
    return G.load('reference_e2e')


def _cluster(root, sizes, seed):
    from coinstac_dinunet_amd.simulator import LoopbackCluster
    from computations import make_site_data
    c = LoopbackCluster(
        root, n_sites=2,
        site_data=lambda s: make_site_data(s.as_dict(),
                                           n_samples=sizes[s.clientId],
                                           seed=int(s.clientId[-1])))
    c.remote_cache['seed'] = seed  # match the reference run's seed
    return c


def _run_ours(cluster, kw, max_rounds, **inject):
    from coinstac_dinunet_amd import COINNLocal, COINNRemote
    from coinstac_dinunet_amd.config.keys import Mode
    from computations import TabularDataset, TabularTrainer
    ok, _ = cluster.run(
        lambda cache, input, state: COINNLocal(cache=cache, input=input,
                                               state=state, mode=Mode.TRAIN,
                                               **kw),
        lambda cache, input, state: COINNRemote(cache=cache, input=input,
                                                state=state),
        TabularTrainer, dataset_cls=TabularDataset, max_rounds=max_rounds,
        **inject)
    return ok


def _unshuffled(base):
    """The reference's padded train loader never shuffles (its get_loader
    forces shuffle False before building the sampler); ours shuffles
    seeded by default. Align batch order for the bitwise comparison."""

    class Unshuffled(base):
        def backward(self):
            out = {}
            self.trainer.nn[self.first_model].train()
            self.trainer.optimizer[self.first_optim].zero_grad()
            its = []
            for _ in range(self.cache.get('local_iterations', 1)):
                batch, nxt = self.trainer.data_handle.next_iter(shuffle=False)
                it = self.trainer.iteration(batch)
                it['loss'].backward()
                its.append(it)
                out.update(**nxt)
            return self.trainer.reduce_iteration(its), out

    return Unshuffled


_EVEN = {'local0': 20, 'local1': 20}


def test_reference_and_ours_agree_end_to_end(ref, tmp_path):
    from coinstac_dinunet_amd.config.keys import Key
    from coinstac_dinunet_amd.distrib.learner import COINNLearner
    from coinstac_dinunet_amd.distrib.reducer import COINNReducer
    want = ref['dsgd']
    our_cluster = _cluster(str(tmp_path / 'ours'), _EVEN, 2024)
    kw = dict(_KW, agg_engine='dSGD_unshuffled')
    ok_our = _run_ours(our_cluster, kw, 400,
                       learner_cls=_unshuffled(COINNLearner),
                       reducer_cls=COINNReducer)
    assert want['ok'] and ok_our
    assert want['rounds'] == our_cluster.rounds, \
        'protocols took different numbers of rounds'

    # reduced global test scores agree
    rs = want['global_test']
    os_ = our_cluster.remote_cache[Key.GLOBAL_TEST_SERIALIZABLE]
    assert len(rs) == len(os_) == 1
    ra = np.asarray(rs[0]['averages'], dtype=float)
    oa = np.asarray(os_[0]['averages'], dtype=float)
    np.testing.assert_allclose(ra, oa, rtol=1e-5)
    np.testing.assert_allclose(np.asarray(rs[0]['metrics'], dtype=float),
                               np.asarray(os_[0]['metrics'], dtype=float),
                               atol=1e-6)

    # final site models agree parameter by parameter
    for i in range(2):
        onet = our_cluster.site_caches[i]['nn']['net']
        ours = list(onet.named_parameters())
        assert len(want['params'][i]) == len(ours)
        for (rn, rp), (on, op_) in zip(want['params'][i], ours):
            assert rn == on
            torch.testing.assert_close(torch.tensor(rp, dtype=op_.dtype),
                                       op_.detach(), rtol=1e-6, atol=1e-7)


def test_reference_and_ours_agree_kfold(ref, tmp_path):
    """Same differential under 3-fold cross-validation: fold queue order,
    per-fold re-init and the fold score table must all line up."""
    from coinstac_dinunet_amd.config.keys import Key
    kw = dict(_KW)
    kw.update(split_ratio=None, num_folds=3, epochs=1, patience=1)
    want = ref['kfold']

    co = _cluster(str(tmp_path / 'ours'), {'local0': 18, 'local1': 18}, 7)
    ok_our = _run_ours(co, kw, 700)

    assert want['ok'] and ok_our
    rs = want['global_test']
    os_ = co.remote_cache[Key.GLOBAL_TEST_SERIALIZABLE]
    assert len(rs) == len(os_) == 3  # one entry per fold, same order
    for fold_ref, fold_our in zip(rs, os_):
        ra = np.asarray(fold_ref['averages'], dtype=float)
        oa = np.asarray(fold_our['averages'], dtype=float)
        assert ra.shape == oa.shape
        np.testing.assert_allclose(ra[1], oa[1])  # same sample counts


def test_reference_and_ours_elect_same_pretrain_site(ref, tmp_path):
    """Pretraining election (max train-data site) must agree. KNOWN
    REFERENCE DEADLOCK pinned here: when the elected site's pretraining
    never improves, the reference ships no weights_file and every site
    spins in PRE_COMPUTATION forever (recorded in the golden run); our
    local proceeds to COMPUTATION instead (distrib/nodes/local.py). The
    test asserts our stack finishes and that the reference either finished
    too or was stuck in exactly that phase."""
    from coinstac_dinunet_amd.config.keys import Phase
    kw = dict(_KW)
    kw.update(pretrain_args={'epochs': 1})
    want = ref['pretrain']
    sizes = {'local0': 12, 'local1': 28}  # site 1 must win the election

    co = _cluster(str(tmp_path / 'ours'), sizes, 7)
    ok_our = _run_ours(co, kw, 500)

    assert ok_our, 'our stack must complete the pretrain path'
    if not want['ok']:
        # the reference deadlock: every site still in PRE_COMPUTATION
        assert want['site0_phase'] == want['phase_pre_computation']
        assert want['site0_phase'] == G.plain(Phase.PRE_COMPUTATION)
    ours = [co.site_caches[i].get('pretrain') for i in range(2)]
    for flags in (want['pretrain_flags'], ours):
        assert flags[1] is True, 'site 1 (more data) should pretrain'
        assert flags[0] is False


def test_reference_and_ours_agree_powersgd(ref, tmp_path):
    """PowerSGD engine differential: warmup -> two-phase P/Q compression
    with error feedback and warm-started Qs must produce the same final
    model as the reference engine on identical data/seeds.

    Seed note: seeds where validation NEVER improves crash the REFERENCE
    at test time (missing best checkpoint, a reference bug our
    test_distributed guards); seed 5 improves at least once."""
    from coinstac_dinunet_amd.distrib.powersgd import (PowerSGDLearner,
                                                       PowerSGDReducer)
    kw = dict(_KW)
    kw.update(agg_engine='powerSGD_unshuffled',  # fall through to inject
              matrix_approximation_rank=2, start_powerSGD_iter=2, epochs=2)
    want = ref['powersgd']

    co = _cluster(str(tmp_path / 'ours'), _EVEN, 5)
    ok_our = _run_ours(co, kw, 500,
                       learner_cls=_unshuffled(PowerSGDLearner),
                       reducer_cls=PowerSGDReducer)

    assert want['ok'] and ok_our
    assert want['rounds'] == co.rounds
    for i in range(2):
        ours = list(co.site_caches[i]['nn']['net'].parameters())
        assert len(want['params'][i]) == len(ours)
        for (_, rp), op_ in zip(want['params'][i], ours):
            torch.testing.assert_close(torch.tensor(rp, dtype=op_.dtype),
                                       op_.detach(), rtol=1e-5, atol=1e-6)


def test_reference_and_ours_agree_rankdad_protocol(ref, tmp_path):
    """rankDAD differential (structural): same phase trajectory and round
    count. Factor VALUES legitimately differ — our power_iteration_BC
    fixes the reference's deflation (garbage components past the true
    rank; see distrib/rankdad.py docstring) — so this pins the protocol,
    not the bits."""
    from coinstac_dinunet_amd.config.keys import Key
    kw = dict(_KW)
    kw.update(agg_engine='rankDAD', dad_reduction_rank=3, epochs=1,
              patience=1)
    want = ref['rankdad']

    co = _cluster(str(tmp_path / 'ours'), _EVEN, 5)
    ok_our = _run_ours(co, kw, 500)

    assert want['ok'] and ok_our
    assert want['rounds'] == co.rounds
    rs = want['global_test']
    os_ = co.remote_cache[Key.GLOBAL_TEST_SERIALIZABLE]
    assert len(rs) == len(os_) == 1
    # same evaluated sample counts through the same protocol
    assert rs[0]['averages'][1] == os_[0]['averages'][1]
