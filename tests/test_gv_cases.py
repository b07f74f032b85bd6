"""Global-variance postfilter, host side (no GPU): the claims of its numpy statement (tests/gv_cases.py), the --gv
option and its checks, the statistic in the converter model file, and -- on the CPU oracle backend -- that the
statistic fits the conversions: a GMM / MLPG conversion varies clearly less than the target speaker does."""
import pathlib
import shutil
import sys

import numpy as np
import pytest

import gv_cases as gc
from conftest import CLB_DIR, CLB_WAV, SLT_DIR


def _run_cli(main, argv):
    old = sys.argv
    sys.argv = ['prog'] + argv
    try:
        main()
    finally:
        sys.argv = old


def _parser_error(main, argv, capsys):
    with pytest.raises(SystemExit) as e:
        _run_cli(main, argv)
    assert e.value.code == 2
    return capsys.readouterr().err


# ---- the numpy statement's own claims -------------------------------------------------------------------------------
def _cases(seed, lengths=gc.LENGTHS, cols=25):
    rng = np.random.RandomState(seed)
    for T in lengths:
        x = gc.matrix(rng, T, cols)
        r = rng.uniform(0.5, 3.0, size=cols - 1)
        yield x, gc.gv_for_ratios(x, r), r


def test_strength_zero_returns_the_input_bit_for_bit():
    for x, gv, _ in _cases(0):
        x[0, 3] = -0.0                                        # (x + 0 would turn it into +0)
        y, status = gc.postfilter(x, gv, 0.0)
        assert status == 0 and y.tobytes() == x.tobytes() and y is not x
        d = np.random.RandomState(1).standard_normal(x.shape)
        y, _ = gc.postfilter(x, gv, 0.0, base=d)
        assert y.tobytes() == d.tobytes()


def test_full_strength_gives_the_target_variance():
    worst = 0.0
    for seed in range(4):
        for x, gv, _ in _cases(seed, lengths=[T for T in gc.LENGTHS if T >= 2]):
            y, status = gc.postfilter(x, gv, 1.0)
            assert status == 0
            for d in range(1, x.shape[1]):
                err, bound = abs(np.var(y[:, d]) / gv[d] - 1), gc.variance_claim_bound(x, d)
                worst = max(worst, err / bound)
                assert err <= bound, (len(x), d, err, bound)
    print(f'variance claim: worst error / bound = {worst:.3f}')


@pytest.mark.parametrize('s', [0.25, 0.5, 1.0])
def test_agrees_with_the_textbook_form(s):
    worst = 0.0
    for x, gv, r in _cases(5):
        y, _ = gc.postfilter(x, gv, s)
        t = gc.textbook(x, gv, s)
        for d in range(1, x.shape[1]):
            err, bound = np.abs(y[:, d] - t[:, d]).max(), gc.textbook_bound(x, r[d - 1], d)
            worst = max(worst, err / bound) if bound else worst
            assert err <= bound, (len(x), d, err, bound)
    print(f'textbook form: worst error / bound = {worst:.3f}')


def test_constant_columns_single_frames_and_c0_come_back_unchanged():
    rng = np.random.RandomState(2)
    x = gc.matrix(rng, 300, 25)
    x[:, 4] = 0.1                    # (300 copies of 0.1 do not add up to 30: the mean must not come from the sum)
    x[:, 7] = -3.75
    gv = np.full(25, 2.0)
    m = gc.column_moments(x)
    assert m[4, 1] == 0.1 and m[4, 2] == 0.0 and m[7, 1] == -3.75 and m[7, 2] == 0.0
    y, status = gc.postfilter(x, gv, 1.0)
    assert status == 0
    for d in (0, 4, 7):
        assert y[:, d].tobytes() == x[:, d].tobytes(), d
    assert not np.array_equal(y[:, 5], x[:, 5])
    one = gc.matrix(rng, 1, 25)
    y, status = gc.postfilter(one, gv, 1.0)
    assert status == 0 and y.tobytes() == one.tobytes()
    # c0 is neither filtered nor examined
    x[5, 0] = np.nan
    gv[0] = -1.0
    y, status = gc.postfilter(x, gv, 0.5)
    assert status == 0 and y[:, 0].tobytes() == x[:, 0].tobytes()


def test_unusable_coefficients_are_counted_and_left():
    rng = np.random.RandomState(3)
    x = gc.matrix(rng, 200, 25)
    gv = np.full(25, 2.0)
    x[17, 3] = np.nan
    for d, bad in ((5, 0.0), (6, -1.0), (7, np.inf), (8, np.nan)):
        gv[d] = bad
    y, status = gc.postfilter(x, gv, 1.0)
    assert status == 5
    for d in (3, 5, 6, 7, 8):
        assert y[:, d].tobytes() == x[:, d].tobytes(), d
    assert np.var(y[:, 9]) == pytest.approx(2.0, rel=1e-12)


def test_differential_form_adds_the_filters_change():
    for x, gv, _ in _cases(6, lengths=(2, 65, 1000)):
        d_conv = np.random.RandomState(7).standard_normal(x.shape) * np.abs(x).max(axis=0) * 0.1
        for s in (0.5, 1.0):
            y, _ = gc.postfilter(x, gv, s)
            out, status = gc.postfilter(x, gv, s, base=d_conv)
            assert status == 0
            assert out[:, 0].tobytes() == d_conv[:, 0].tobytes()
            want = d_conv + (y - x)
            # roundings: of y, of y - x, of either sum
            bound = 4 * gc.U * (np.abs(y).max(axis=0) + np.abs(x).max(axis=0) + np.abs(out).max(axis=0))
            assert np.all(np.abs(out - want).max(axis=0) <= bound)


def test_statistic_is_the_mean_of_the_utterance_variances():
    rng = np.random.RandomState(4)
    mats = [gc.matrix(rng, T, 25, max_offset=5.0) for T in (300, 0, 1, 777)]
    gv = gc.gv_statistic([gc.column_moments(m) for m in mats])
    want = np.mean([m.var(axis=0) for m in mats if len(m)], axis=0)
    assert np.allclose(gv, want, rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        gc.gv_statistic([gc.column_moments(mats[1])])


# ---- the command line -------------------------------------------------------------------------------------------------
def test_gv_option_parses():
    import argparse
    import kwiiyatta_amd as k
    for argv, want in ((['--gv'], 1.0), (['--gv', '0.5'], 0.5), (['--gv', '0'], 0.0), (['--gv', '1'], 1.0), ([], 0.0),
                       (['--gv', '--mcep-order', '24'], 1.0)):
        conf = k.Config(argparse.ArgumentParser())
        conf.add_gv_argument()
        conf.parser.parse_args(argv, namespace=conf)
        assert conf.gv == want, argv


@pytest.mark.parametrize('text', ['-0.1', '1.5', 'abc', 'nan'])
def test_gv_out_of_range_is_a_parser_error(text, capsys):
    import kwiiyatta_amd.convert_voice as cv
    assert '--gv' in _parser_error(cv.main, ['--gv', text, CLB_WAV], capsys)


def test_resynthesize_voice_has_no_gv_option(capsys):
    import kwiiyatta_amd.resynthesize_voice as rv
    assert '--gv' in _parser_error(rv.main, [CLB_WAV, '--gv'], capsys)


# ---- the model file ---------------------------------------------------------------------------------------------------
def _trained_stack(gv_stats=None):
    import kwiiyatta_amd as k
    conv = k.MelCepstrumConverter(components=2, random_state=0)
    rng = np.random.RandomState(0)
    gmm = conv.gmm
    gmm.weights_ = np.array([0.25, 0.75])
    gmm.means_ = rng.standard_normal((2, 6))
    gmm.covariances_ = np.stack([np.eye(6) * 0.5, np.eye(6) * 2.0])
    conv.order, conv.fs, conv.frame_period = 24, 16000, 5
    conv.gv_stats = gv_stats
    return conv


def _parent_model(path):
    """a model file as the parent commit's `save` writes it (f0 statistics, no global variance)"""
    conv = _trained_stack()
    gmm = conv.gmm
    with open(path, 'wb') as fh:
        np.savez(fh, format=conv.MODEL_FORMAT, order=24, fs=16000, frame_period=5, weights=gmm.weights_,
                 means=gmm.means_, covariances=gmm.covariances_, f0_stats=np.array([5.1, 0.21, 5.4, 0.17]))


def test_model_round_trip_keeps_gv_stats(tmp_path):
    import kwiiyatta_amd as k
    stats = np.random.RandomState(1).uniform(0.01, 2.0, size=25)
    path = tmp_path / 'model.npz'
    _trained_stack(stats).save(path)
    loaded = k.MelCepstrumConverter(components=2).load(path)
    assert loaded.gv_stats.dtype == np.float64 and loaded.gv_stats.tobytes() == stats.tobytes()
    assert loaded.f0_stats is None
    assert k.MelCepstrumConverter(components=2).gv_stats is None
    # without the statistic: no key in the file (what older readers expect), None after loading
    _trained_stack(None).save(path)
    with np.load(path) as z:
        assert 'gv_stats' not in z.files and str(z['format']) == 'kwiiyatta_amd.converter/1'
    assert k.MelCepstrumConverter(components=2).load(path).gv_stats is None


def test_parent_commits_model_loads_without_gv_stats(tmp_path):
    import kwiiyatta_amd as k
    path = tmp_path / 'parent.npz'
    _parent_model(path)
    conv = k.MelCepstrumConverter(components=2).load(path)
    assert conv.gv_stats is None and conv.f0_stats == (5.1, 0.21, 5.4, 0.17) and conv.order == 24


def test_gv_with_a_model_without_statistics_asks_to_retrain(tmp_path, capsys):
    import kwiiyatta_amd.convert_voice as cv
    path = tmp_path / 'parent.npz'
    _parent_model(path)
    err = _parser_error(cv.main, ['--gv', '--converter-model', str(path), '--result-dir', str(tmp_path / 'out'), CLB_WAV],
                        capsys)
    assert 'no global variance statistics' in err and 'retrain it with --gv' in err
    assert not (tmp_path / 'out').exists()


def test_convert_checks_strength_and_statistics():
    import kwiiyatta_amd as k
    conv = _trained_stack()

    class Mcep:
        order, fs = 24, 16000
    with pytest.raises(ValueError, match=r'outside \[0, 1\]'):
        conv.convert(Mcep(), gv=1.5)
    with pytest.raises(ValueError, match=r'outside \[0, 1\]'):
        conv.convert(Mcep(), gv=-0.1)
    with pytest.raises(ValueError, match='gv_stats=True'):
        conv.convert(Mcep(), gv=0.5)
    assert k.MelCepstrumConverter(components=2).gv_stats is None


# ---- the statistic fits the conversions (CPU oracle backend, scikit-learn's fit) ---------------------------------------------
def test_converted_trajectories_vary_less_than_the_targets(monkeypatch, tmp_path):
    """4 CLB -> SLT training files, 2 components, seed 0: for the four training inputs and two unseen ones the median
    over c1..c24 of r_d = sqrt(gv_d / var(converted c_d)) exceeds 1.25 and at least 20 of 24 coefficients have
    r_d > 1 (measured when the feature was proposed: medians 1.62 .. 1.73, 22 .. 24 coefficients).  The new kernels
    cannot run here, so the statistic and the ratios come from the numpy statement."""
    from conftest import _install_oracle_backend
    _install_oracle_backend(monkeypatch)
    import kwiiyatta_amd as k
    from kwiiyatta_amd.converter.mcep import _target_mel_cepstra
    src = tmp_path / 'src'
    src.mkdir()
    for n in range(1, 5):
        shutil.copy(pathlib.Path(CLB_DIR) / f'arctic_a{n:04}.wav', src)
    dataset = k.align(k.WavFileDataset(src, Analyzer=k.analyze_wav),
                      k.WavFileDataset(pathlib.Path(SLT_DIR), Analyzer=k.analyze_wav))
    keys = sorted(dataset.keys())[:4]
    conv = k.MelCepstrumConverter(use_delta=True, components=2, random_state=0)
    np.random.seed(0)
    conv.train(dataset, keys)
    assert conv.gv_stats is None                       # a plain train computes none
    mats = _target_mel_cepstra(dataset, keys, conv.order, conv.fs)
    assert len(mats) == 4 and all(m.shape[1] == 25 and m.dtype == np.float64 for m in mats)
    gv = gc.gv_statistic([gc.column_moments(m) for m in mats])
    assert gv.shape == (25,) and np.all(gv > 0)
    for n in (1, 2, 3, 4, 8, 9):
        mcep = k.analyze_wav(pathlib.Path(CLB_DIR) / f'arctic_a{n:04}.wav').mel_cepstrum
        r = gc.ratios(conv.convert(mcep).data, gv)
        print(f'arctic_a{n:04}: frames {len(mcep.data)} median r {np.median(r):.3f} min {r.min():.3f} max {r.max():.3f} '
              f'r > 1: {(r > 1).sum()} / {len(r)}')
        assert len(r) == 24 and np.median(r) > 1.25 and (r > 1).sum() >= 20, n
