"""CPU side of the EM trajectory conversion over soft mixture posteriors: the numpy restatement of tests/em_cases.py on
its own -- how well conditioned every table case is, that the log-likelihood never decreases, where the scheme meets
the arg-max conversion and where it leaves it -- and the host logic around the new entry points.

The conditioning gate is a condition on the INPUTS of tests/test_em_gpu.py, not a measurement of the library: the
log-densities and conditional means of a case are perturbed by a relative 1e-13 (three seeds), and every y_k has to stay
within 3e-10 of its peak, every L_k within 3e-10 |L_k|.  The device test then holds the kernels to 1e-9 with three
orders of magnitude of room over f64 rounding.  Worst over the table: 9e-11 for y (d = 24, M = 64, T = 257, N = 1),
2e-13 for L.  A case that fails the gate gets a smaller N, never a larger cap.
"""
import sys

import numpy as np
import pytest

import convert_cases as cc
import em_cases as ec

GATE = 3e-10


def _perturbed(logp, E, v, N, seed):
    rng = np.random.default_rng([seed, logp.shape[0], logp.shape[1], E.shape[2]])
    return ec.em_from_terms(logp * (1.0 + 1e-13 * rng.standard_normal(logp.shape)),
                            E * (1.0 + 1e-13 * rng.standard_normal(E.shape)), v, N)


def _gate(logp, E, v, N, ys, Ls, what):
    worst_y = worst_l = 0.0
    for seed in range(3):
        py, pl = _perturbed(logp, E, v, N, seed)
        for k in range(N + 1):
            worst_y = max(worst_y, np.abs(py[k] - ys[k]).max() / np.abs(ys[k]).max())
            worst_l = max(worst_l, abs(pl[k] - Ls[k]) / abs(Ls[k]))
    print(f'{what}: moved by {worst_y:.2e} of the peak (y), {worst_l:.2e} (L)')
    assert worst_y <= GATE and worst_l <= GATE, what


@pytest.mark.parametrize('case', ec.CASES, ids=ec.case_id)
def test_case_is_well_conditioned_and_its_likelihood_never_decreases(case):
    d, M, s, tag, T, N = case
    outs, Ls = ec.case_reference(case)
    assert len(outs) == len(Ls) == N + 1 and all(np.isfinite(o).all() for o in outs) and np.isfinite(Ls).all()
    _gate(*ec.case_terms(d, M, s, tag, T), N, [o[:, 1:] for o in outs], Ls, ec.case_id(case))
    for k in range(N):
        assert Ls[k + 1] >= Ls[k] - 1e-9 * abs(Ls[k]), (k, Ls)
    w, mu, cov, mc = ec.inputs(d, M, s, tag, T)
    assert np.array_equal(outs[0][:, 0], mc[:, 0])
    hard = cc.ref_mcep(mc, w, mu, cov)
    peak = np.abs(hard[:, 1:]).max()
    apart = np.abs(outs[0] - hard).max() / peak
    if M == 1:
        assert apart <= 1e-12, 'one mixture: the single solve is the arg-max conversion'
    elif T >= 15 and M >= 3:
        assert apart > 1e-2, f'soft posteriors give another trajectory than the arg-max ({apart:.2e} of the peak)'


def test_batch_case_is_well_conditioned():
    d, M, s, tag, Ts, N = ec.BATCH
    for T in Ts:
        w, mu, cov, mc = ec.inputs(d, M, s, tag, T)
        logp, E, v = ec.terms(mc, w, mu, cov)
        ys, Ls = ec.em_from_terms(logp, E, v, N)
        _gate(logp, E, v, N, ys, Ls, f'batch job of {T} frames')


def test_table_covers_the_issue_and_the_frame_tile():
    by = {}
    for d, M, s, tag, T, N in ec.CASES:
        by.setdefault((d, M, s), set()).add((T, N))
    assert {(T, 4) for T in (1, 2, 3, 15, 16, 17, 33, 257, ec.FRAME_TILE - 1, ec.FRAME_TILE, ec.FRAME_TILE + 1)} \
        <= by[2, 3, 1.0]
    assert by[24, 64, 0.2] == {(33, 4), (129, 1), (257, 1)} and by[24, 64, 1.0] == {(257, 4)}
    assert by[2, 70, 1.0] == {(33, 2)} and by[27, 3, 0.2] == {(33, 2)}
    assert all(by[d, 3, 0.2] == {(33, 2)} for d in (6, 11, 16, 20))
    assert max(N for *_, N in ec.CASES) <= ec.KWY_MLPG_EM_MAX


@pytest.mark.parametrize('M', (3, 64))
def test_well_separated_mixtures_give_the_arg_max_conversion(M):
    """spread = 6: the x-means lie so far apart that the posteriors of a track built on the mixture's own x-means --
    dwelling 11 frames near the static part of one after the other -- are one-hot to the last bit of the winner, the
    others below 1e-25 (asserted: a property of this input; tag and dwell are chosen for it, the transitions between
    dwells are where a shorter dwell leaves a runner-up).  The winner changes along the track."""
    d, T, tag = 24, 33, 7
    w, mu, cov = cc.mixture(3 * d, M, tag, spread=6.0)
    rng = np.random.default_rng([cc.SEED, d, M, tag, T, 2])
    mc = np.empty((T, d + 1))
    mc[:, 0] = rng.standard_normal(T)
    mc[:, 1:] = mu[(np.arange(T) // 11) % M, :d] + 0.3 * rng.standard_normal((T, d))
    post = cc.posterior(cc.ref_logp(cc.delta_features(mc[:, 1:]), w, mu, cov))
    assert (post.max(axis=1) == 1.0).all() and np.sort(post, axis=1)[:, :-1].max() < 1e-25
    assert len(set(post.argmax(axis=1))) >= 3
    outs, _ = ec.ref_mcep_em(mc, w, mu, cov, 0)
    hard = cc.ref_mcep(mc, w, mu, cov)
    assert np.abs(outs[0] - hard).max() <= 1e-12 * np.abs(hard).max()


def test_diff_mixture_is_the_mixture_over_the_difference():
    w, mu, cov = cc.mixture(6, 2, 7)
    mu2, cov2 = ec.diff_mixture(mu, cov)
    D = 6
    J = np.block([[np.eye(D), np.zeros((D, D))], [-np.eye(D), np.eye(D)]])      # [x, y] -> [x, y - x]
    for m in range(2):
        assert np.allclose(mu2[m], J @ mu[m], rtol=0, atol=1e-14)
        assert np.allclose(cov2[m], J @ cov[m] @ J.T, rtol=0, atol=1e-14)


# ---- host logic ------------------------------------------------------------------------------------------------------
class _Gmm:
    covariance_type = 'full'

    def __init__(self, d=2, M=3):
        self.weights_, self.means_, self.covariances_ = cc.mixture(3 * d, M, 7)


def test_mlpg_em_argument_is_validated():
    from kwiiyatta_amd.backend import mlpg
    assert mlpg.EM_MAX == ec.KWY_MLPG_EM_MAX
    plain = mlpg.MLPG(_Gmm())
    assert plain.em is None and plain.loglik_ is None
    for good in (0, 1, 16, np.int64(3)):
        stage = mlpg.MLPG(_Gmm(), em=good)
        assert stage.em == int(good) and type(stage.em) is int and stage.loglik_ is None
    for bad in (True, False, 1.0, '2', -1, 17, 2.5):
        with pytest.raises(ValueError):
            mlpg.MLPG(_Gmm(), em=bad)
    static = mlpg.DELTA_WINDOWS[0:1]
    assert mlpg.MLPG(_Gmm(), windows=static).framewise
    with pytest.raises(ValueError, match='static window'):
        mlpg.MLPG(_Gmm(), windows=static, em=1)


def test_converter_hands_em_on_only_when_set(monkeypatch):
    from kwiiyatta_amd.converter import gmm as gmm_mod
    calls = []

    class Stub:
        def __init__(self, gmm, **kwargs):
            calls.append(kwargs)

        def transform(self, feature):
            return feature

    monkeypatch.setattr(gmm_mod, 'MLPG', Stub)
    conv = gmm_mod.GMMFeatureConverter.__new__(gmm_mod.GMMFeatureConverter)
    conv.gmm = object()
    x = np.zeros((3, 6))
    assert conv.convert(x) is x and conv.convert(x, diff=True, em=None) is x
    assert all('em' not in kw for kw in calls) and calls[1]['diff'] is True
    conv.convert(x, em=0)
    conv.convert(x, mlpg=True, diff=True, em=4)
    assert calls[2]['em'] == 0 and calls[3]['em'] == 4 and calls[3]['diff'] is True


def test_mlpg_em_option_parses_in_both_commands(monkeypatch):
    import kwiiyatta_amd as k
    from kwiiyatta_amd import config, evaluate_voice

    def parsed(conf, argv):
        monkeypatch.setattr(sys, 'argv', ['prog'] + argv)
        conf.parse_args()
        return conf

    def convert_conf():
        conf = k.Config()
        conf.add_gv_argument()
        conf.add_mlpg_em_argument()
        conf.add_converter_arguments()
        return conf
    assert config.MLPG_EM_OPTION[0] == '--mlpg-em' and config.MLPG_EM_OPTION[1]['default'] is None
    assert parsed(convert_conf(), []).mlpg_em is None
    assert parsed(convert_conf(), ['--mlpg-em', '0']).mlpg_em == 0
    assert parsed(convert_conf(), ['--mlpg-em', '16', '--gv']).mlpg_em == 16
    assert parsed(evaluate_voice.make_config(), []).mlpg_em is None
    assert parsed(evaluate_voice.make_config(), ['--mlpg-em', '4', '--batch']).mlpg_em == 4
    for bad in ('-1', '17', '1.5', 'x'):
        with pytest.raises(SystemExit):
            parsed(convert_conf(), ['--mlpg-em', bad])
    import inspect
    from kwiiyatta_amd import convert_voice, corpus
    assert 'add_mlpg_em_argument' in inspect.getsource(convert_voice.main)
    for fn in (corpus.convert_batch, corpus.evaluate_batch, convert_voice.convert, convert_voice.convert_synth_batch):
        assert inspect.signature(fn).parameters['mlpg_em'].default is None
    assert inspect.signature(evaluate_voice.evaluate_pair).parameters['em'].default is None
    for bad in (True, 1.5, -1, 17):
        with pytest.raises(ValueError, match='mlpg_em'):
            corpus._mlpg_em(bad)
    assert corpus._mlpg_em(None) is None and corpus._mlpg_em(np.int32(2)) == 2


def test_new_entry_points_are_in_the_ctypes_table():
    import ctypes
    from kwiiyatta_amd import _lib
    for name in ('kwy_gmm_mlpg_em', 'kwy_convert_mcep_em_dev', 'kwy_convert_mcep_em_batch_dev'):
        assert name in _lib.SIGNATURES and name not in _lib.MISSING
    assert len(_lib.SIGNATURES['kwy_gmm_mlpg_em'][1]) == 12
    assert len(_lib.SIGNATURES['kwy_convert_mcep_em_dev'][1]) == 9
    assert len(_lib.SIGNATURES['kwy_convert_mcep_em_batch_dev'][1]) == 7
    assert [n for n, _ in _lib.ConvertEmJob._fields_] == ['mc', 'T', 'mc_out', 'loglik']
    assert ctypes.sizeof(_lib.ConvertEmJob) == 32


def test_drivers_take_the_options_of_one_record_and_name_a_keyword_they_do_not_know():
    """the defaults below are those of convert_batch's signature before the options moved into ConvertOptions"""
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd._convert_options import ConvertOptions
    with pytest.raises(TypeError, match='gv_strenght'):
        corpus.convert_batch([], 16000, None, gv_strenght=1.0)
    with pytest.raises(TypeError, match='ms_strength'):
        corpus.evaluate_batch([], 16000, None, ms_strength=1.0)
    assert ConvertOptions.DEFAULTS == dict(
        f0_stats=None, transpose_key=0.0, gv_stats=None, gv_strength=0.0, ms_stats=None, ms_length=None, ms_strength=0.0,
        formant_ratio=1.0, mlpg_em=None, mlpg_gv=None, gv_var=None, gv_weight=1.0, diff_filter='mlsa', postfilter_beta=0.0,
        keep_power=False)
    assert all(type(v) is type(w) for v, w in zip(ConvertOptions.DEFAULTS.values(),
                                                  (None, 0.0, None, 0.0, None, None, 0.0, 1.0, None, None, None, 1.0, 'mlsa',
                                                   0.0, False)))
    record = ConvertOptions()
    assert all(getattr(record, name) is default for name, default in ConvertOptions.DEFAULTS.items())
