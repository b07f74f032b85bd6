"""The GV-considering trajectory generation without a device: the conditioning of every case the GPU tests compare
(tests/gvgen_cases.py), the properties of the numpy restatement, and the host logic around the new option.

Conditioning gate: the band records and y_ML of every table case are perturbed by a relative 1e-13 (three seeds); no
y_k may move by more than 3e-10 of its peak and no Q_k by more than 3e-10 of the sum of the magnitudes of its three
terms -- the EM tests' gate (tests/test_em_cases.py), a condition on the inputs checked from the restatement alone.  The
GPU tests then hold the device to 1e-9.  A case that fails here gets a smaller N, never a larger cap.
"""
import sys

import numpy as np
import pytest

import gvgen_cases as gc

GATE = 3e-10
PERTURBATION = 1e-13


def _gate(rec, y, s, mean, var, N, ref, what):
    worst_y, worst_q = gc.gate_figures(rec, y, s, mean, var, N, ref, PERTURBATION)
    print(f'{what}: a relative {PERTURBATION:g} of the inputs moves y_k by at most {worst_y:.3e} of its peak, '
          f'Q_k by {worst_q:.3e} of its terms')
    assert worst_y <= GATE and worst_q <= GATE, what


@pytest.mark.parametrize('case', gc.CASES, ids=gc.case_id)
def test_case_is_well_conditioned_and_its_objective_never_decreases(case):
    d, T, off, up, Ns = case
    rec, y, s, mean, var = gc.inputs(d, T, off, up)
    ref = gc.case_reference(case)
    ys, Qs, mags, status = ref
    assert status == 0 and np.isfinite(ys).all() and np.isfinite(Qs).all()
    assert all(Qs[k + 1] >= Qs[k] for k in range(len(Qs) - 1)), Qs
    _gate(rec, y, s, mean, var, max(Ns), ref, gc.case_id(case))
    if T > 1:
        # after the table's largest N the variance is closer to the target than at y_ML (they differ by 60 % or 100 %)
        z0, zN = (a if s is None else a + s for a in (y, ys[-1]))
        assert np.all(np.abs(zN.var(axis=0) - mean) < np.abs(z0.var(axis=0) - mean))


def test_batch_case_is_well_conditioned():
    d, Ts, off, up, N = gc.BATCH
    mean = var = None
    for T in Ts:
        rec, y, s, m, v = gc.inputs(d, T, off, up)
        mean, var = (m, v) if mean is None else (mean, var)
        _gate(rec, y, s, mean, var, N, gc.ascent(rec, y, s, mean, var, N), f'batch job of {T} frames')


@pytest.mark.parametrize('case', gc.CHAINED, ids=gc.chained_id)
def test_chained_case_is_well_conditioned(case):
    w, mu, cov, mc, s, mean, var, rec, y, ref = gc.chained_reference(case)
    assert ref[3] == 0 and all(ref[1][k + 1] >= ref[1][k] for k in range(gc.CHAINED_N))
    _gate(rec, y, s, mean, var, gc.CHAINED_N, ref, gc.chained_id(case))


def test_table_covers_the_issue_and_the_kernel_forms():
    Ts = {T for _, T, _, _, _ in gc.CASES}
    assert {1, 2, 3, 4, 5, gc.NT - 1, gc.NT, gc.NT + 1, 2 * gc.NT + 1, 2001} <= Ts
    for edge in (gc.REG_ROWS, gc.LDS_ROWS):
        assert {edge - 1, edge, edge + 1} <= Ts
    assert {d for d, _, _, _, _ in gc.CASES} == {1, 2, 24, 27}
    assert {N for c in gc.CASES for N in c[4]} == {0, 1, 2, 8, gc.LONG_N}
    assert {(off, up) for _, _, off, up, _ in gc.CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    assert gc.KWY_MLPG_GV_MAX == 256 and len(gc.BATCH[1]) == 3
    text = open(__file__.replace('tests/test_gvgen_cases.py', 'kwiiyatta_amd/csrc/kwy_gvgen.hip')).read()
    assert f'#define GVA_NT {gc.NT}\n' in text and f'#define GVA_LDS_ROWS {gc.LDS_ROWS} ' in text
    assert f'#define GVA_REG_ROWS {gc.REG_ROWS // gc.NT} ' in text


def test_no_iterations_is_the_linear_scaling():
    for up in (True, False):
        rec, y, s, mean, var = gc.inputs(2, 257, False, up)
        ys, Qs, _, _ = gc.ascent(rec, y, None, mean, var, 0)
        want = y + (np.sqrt(mean / y.var(axis=0)) - 1.0) * (y - y.mean(axis=0))
        assert np.abs(ys[0] - want).max() <= 1e-12
        assert np.allclose(ys[0].var(axis=0), mean, rtol=1e-12)


def test_a_track_that_has_the_target_variance_stays():
    rec, y, s, _, _ = gc.inputs(2, 257, False, True)
    mean = y.var(axis=0)
    ys, Qs, _, _ = gc.ascent(rec, y, None, mean, (0.3 * mean) ** 2, 8)
    assert np.abs(ys - y).max() <= 1e-12


def test_unusable_and_constant_columns():
    rec, y, s, mean, var = gc.inputs(2, 33, True, True)
    for bad_mean, bad_var in ((np.nan, 1.0), (0.0, 1.0), (1.0, 0.0), (1.0, np.inf), (-1.0, 1.0)):
        ys, Qs, mags, bad = gc.ascent_column(rec[:, 0], y[:, 0], s[:, 0], bad_mean, bad_var, 1.0, 2)
        assert bad and np.array_equal(ys, np.tile(y[:, 0], (3, 1))) and not Qs.any()
    ys, Qs, mags, bad = gc.ascent_column(rec[:, 0], np.full(33, 0.5), None, mean[0], var[0], 1.0, 2)
    assert not bad and np.array_equal(ys, np.full((3, 33), 0.5)) and not Qs.any()


def test_conversion_bands_restate_the_solvers_system():
    import convert_cases as cc
    import em_cases as ec
    d, M, T = 2, 3, 33
    w, mu, cov, mc = ec.inputs(d, M, 1.0, 7, T)
    rec, y = gc.conversion_bands(mc, w, mu, cov, -1)
    assert np.abs(y - cc.ref_mcep(mc, w, mu, cov)[:, 1:]).max() <= 1e-12 * np.abs(y).max()
    for em in (0, 2):
        rec, y = gc.conversion_bands(mc, w, mu, cov, em)
        want = ec.ref_mcep_em(mc, w, mu, cov, em)[0][em][:, 1:]
        assert np.abs(y - want).max() <= 1e-12 * np.abs(y).max()


# ---- host logic ------------------------------------------------------------------------------------------------------
class _Gmm:
    covariance_type = 'full'
    weights_ = np.ones(1)
    means_ = np.zeros((1, 12))
    covariances_ = np.eye(12)[None]


def test_mlpg_gv_arguments_are_validated():
    from kwiiyatta_amd.backend import gv, mlpg
    assert mlpg.GV_MAX == gv.ASCENT_MAX == gc.KWY_MLPG_GV_MAX
    stats = (np.ones(2), np.ones(2))
    m = mlpg.MLPG(_Gmm(), gv=stats, gv_iterations=4, em=2, diff=True)
    assert m.gv[2] == 4 and m.gv[3] == 1.0 and m.em == 2 and m.objective_ is None and m.loglik_ is None
    assert mlpg.MLPG(_Gmm()).gv is None
    for bad in (-1, 257, 1.5, True, 'x'):
        with pytest.raises(ValueError, match='iterations'):
            mlpg.MLPG(_Gmm(), gv=stats, gv_iterations=bad)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='weight'):
            mlpg.MLPG(_Gmm(), gv=stats, gv_iterations=1, gv_weight=bad)
    with pytest.raises(ValueError, match='go together'):
        mlpg.MLPG(_Gmm(), gv=stats)
    with pytest.raises(ValueError, match='go together'):
        mlpg.MLPG(_Gmm(), gv_iterations=2)
    with pytest.raises(ValueError, match='one value per column'):
        mlpg.MLPG(_Gmm(), gv=(np.ones(2), np.ones(3)), gv_iterations=1)
    with pytest.raises(ValueError, match='static window'):
        mlpg.MLPG(_Gmm(), windows=mlpg.DELTA_WINDOWS[0:1], gv=stats, gv_iterations=1)
    with pytest.raises(ValueError, match='2 static dimensions'):
        mlpg.MLPG(_Gmm(), gv=(np.ones(3), np.ones(3)), gv_iterations=1).transform(np.zeros((4, 2)))


def _converter(order=2):
    import kwiiyatta_amd as k
    conv = k.MelCepstrumConverter(use_delta=True, components=1)
    conv.order, conv.fs = order, 16000
    return conv


def _mel_cepstrum(order=2, frames=5):
    import kwiiyatta_amd as k
    return k.MelCepstrum(16000, 5.0, np.zeros((frames, order + 1)))


def test_convert_checks_its_mlpg_gv_arguments():
    conv = _converter()
    mc = _mel_cepstrum()
    with pytest.raises(ValueError, match='retrain it with gv_stats=True on two or more'):
        conv.convert(mc, mlpg_gv=4)
    conv.gv_stats = np.ones(3)
    with pytest.raises(ValueError, match='retrain it with gv_stats=True on two or more'):
        conv.convert(mc, mlpg_gv=4)                     # (a model file from before gv_var existed)
    conv.gv_var = np.array([1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match='retrain the converter with gv_stats=True on two or more'):
        conv.convert(mc, mlpg_gv=4)                     # (trained on one utterance)
    conv.gv_var = np.ones(3)
    with pytest.raises(ValueError, match='same variance twice'):
        conv.convert(mc, mlpg_gv=4, gv=1.0)
    conv.ms_stats = (np.zeros((3, 3, 3)),) * 2
    with pytest.raises(ValueError, match='left for later'):
        conv.convert(mc, mlpg_gv=4, ms=1.0)
    for bad in (-1, 257, 1.5):
        with pytest.raises(ValueError, match='iterations'):
            conv.convert(mc, mlpg_gv=bad)
    with pytest.raises(ValueError, match='weight'):
        conv.convert(mc, mlpg_gv=4, gv_weight=0.0)


def test_converter_hands_the_statistics_on_only_when_set(monkeypatch):
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
    conv.convert(x)
    conv.convert(x, diff=True, em=2)
    assert all(not any(key.startswith('gv') for key in kw) for kw in calls)
    stats = (np.ones(2), np.ones(2))
    conv.convert(x, diff=True, em=2, gv_stats=stats, gv_iterations=4, gv_weight=2.0)
    assert calls[2]['gv'] is stats and calls[2]['gv_iterations'] == 4 and calls[2]['gv_weight'] == 2.0
    assert calls[2]['em'] == 2 and calls[2]['diff'] is True


def test_model_file_carries_gv_var(tmp_path):
    conv = _converter()
    conv.gmm.weights_, conv.gmm.means_, conv.gmm.covariances_ = np.ones(1), np.zeros((1, 12)), np.eye(12)[None]
    conv.gv_stats, conv.gv_var = np.array([3.0, 2.0, 1.0]), np.array([0.3, 0.2, 0.1])
    conv.save(tmp_path / 'with.npz')
    back = _converter().load(tmp_path / 'with.npz')
    assert np.array_equal(back.gv_stats, conv.gv_stats) and np.array_equal(back.gv_var, conv.gv_var)
    assert back.gv_var.dtype == np.float64
    mean, var = back.gv_ascent_statistics()
    assert np.array_equal(mean, [2.0, 1.0]) and np.array_equal(var, [0.2, 0.1])
    conv.gv_var = None
    conv.save(tmp_path / 'without.npz')
    with np.load(tmp_path / 'without.npz') as z:
        assert 'gv_var' not in z.files and str(z['format']) == conv.MODEL_FORMAT
    old = _converter().load(tmp_path / 'without.npz')
    assert old.gv_var is None and np.array_equal(old.gv_stats, conv.gv_stats)
    assert _converter().gv_var is None


def test_mlpg_gv_option_parses_in_both_commands(monkeypatch):
    import argparse
    import inspect
    import kwiiyatta_amd as k
    from kwiiyatta_amd import config, convert_voice, corpus, evaluate_voice

    def parsed(conf, argv):
        monkeypatch.setattr(sys, 'argv', ['prog'] + argv)
        conf.parse_args()
        return conf

    def convert_conf():
        conf = k.Config()
        conf.add_gv_argument()
        conf.add_ms_argument()
        conf.add_mlpg_em_argument()
        conf.add_mlpg_gv_argument()
        conf.add_converter_arguments()
        return conf
    for good in ('0', '16', '256'):
        assert config.mlpg_gv(good) == int(good)
    for bad in ('-1', '257', '1.5', 'x'):
        with pytest.raises(argparse.ArgumentTypeError):
            config.mlpg_gv(bad)
        with pytest.raises(SystemExit):
            parsed(convert_conf(), ['--mlpg-gv', bad])
    assert config.MLPG_GV_OPTION[0] == '--mlpg-gv' and config.MLPG_GV_OPTION[1]['default'] is None
    assert parsed(convert_conf(), []).mlpg_gv is None
    assert parsed(convert_conf(), ['--mlpg-gv', '0']).mlpg_gv == 0
    both = parsed(convert_conf(), ['--mlpg-gv', '256', '--mlpg-em', '2'])
    assert both.mlpg_gv == 256 and both.mlpg_em == 2
    assert parsed(convert_conf(), ['--mlpg-gv', '4', '--gv', '0', '--ms', '0']).mlpg_gv == 4
    assert parsed(evaluate_voice.make_config(), []).mlpg_gv is None
    assert parsed(evaluate_voice.make_config(), ['--mlpg-gv', '4', '--batch', '--mlpg-em', '1']).mlpg_gv == 4
    for clash in (['--gv'], ['--gv', '0.5'], ['--ms'], ['--ms', '0.5']):
        with pytest.raises(SystemExit):
            parsed(convert_conf(), ['--mlpg-gv', '4'] + clash)
    with pytest.raises(SystemExit):
        parsed(evaluate_voice.make_config(), ['--mlpg-gv', '4', '--gv'])
    assert 'add_mlpg_gv_argument' in inspect.getsource(convert_voice.main)
    for fn in (corpus.convert_batch, corpus.evaluate_batch, convert_voice.convert, convert_voice.convert_synth_batch,
               evaluate_voice.evaluate_pair):
        assert inspect.signature(fn).parameters['mlpg_gv'].default is None
    assert inspect.signature(corpus.build_training_matrix).parameters['gv_variance'].default is False


def test_new_entry_points_are_in_the_ctypes_table():
    import ctypes
    from kwiiyatta_amd import _lib
    for name, args in (('kwy_gv_ascent', 9), ('kwy_gv_ascent_batch_dev', 9), ('kwy_gv_stats_from_moments', 6),
                       ('kwy_gv_stats_from_moments_dev', 6), ('kwy_gmm_mlpg_gv', 19), ('kwy_convert_mcep_gv_dev', 16),
                       ('kwy_convert_mcep_gv_batch_dev', 13)):
        assert name in _lib.SIGNATURES and name not in _lib.MISSING
        assert len(_lib.SIGNATURES[name][1]) == args, name
    assert [n for n, _ in _lib.GvAscentJob._fields_] == ['band', 'offset', 'y', 'T', 'objective']
    assert [n for n, _ in _lib.ConvertGvJob._fields_] == ['mc', 'T', 'mc_out', 'loglik', 'objective']
    assert ctypes.sizeof(_lib.GvAscentJob) == 40 and ctypes.sizeof(_lib.ConvertGvJob) == 40
