"""f0 conversion and key transposition, host side (no GPU): the command-line options and their checks, the f0
statistics in the converter model file, and Chan's merge of voiced log-f0 moments restated in numpy."""
import sys

import numpy as np
import pytest

from conftest import CLB_WAV


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


def _trained_stack(f0_stats=None):
    import kwiiyatta_amd as k
    conv = k.MelCepstrumConverter(components=2, random_state=0)
    rng = np.random.RandomState(0)
    gmm = conv.gmm
    gmm.weights_ = np.array([0.25, 0.75])
    gmm.means_ = rng.standard_normal((2, 6))
    gmm.covariances_ = np.stack([np.eye(6) * 0.5, np.eye(6) * 2.0])
    conv.order, conv.fs, conv.frame_period = 24, 16000, 5
    conv.f0_stats = f0_stats
    return conv


def test_transpose_key_option_parses_and_checks_range():
    import argparse
    import kwiiyatta_amd as k
    for text, key in (('-5', -5.0), ('12', 12.0), ('0.5', 0.5), ('-99.99', -99.99), ('99.99', 99.99)):
        conf = k.Config(argparse.ArgumentParser())
        conf.add_transpose_key_argument()
        conf.parser.parse_args(['--transpose-key', text], namespace=conf)
        assert conf.transpose_key == key
    conf = k.Config(argparse.ArgumentParser())
    conf.add_transpose_key_argument()
    conf.parser.parse_args([], namespace=conf)
    assert conf.transpose_key == 0.0


@pytest.mark.parametrize('key', ['100', '-99.991', 'nan', 'up'])
def test_transpose_key_out_of_range_is_a_parser_error(key, capsys):
    import kwiiyatta_amd.convert_voice as cv
    import kwiiyatta_amd.resynthesize_voice as rv
    assert '--transpose-key' in _parser_error(rv.main, [CLB_WAV, '--transpose-key', key], capsys)
    assert '--transpose-key' in _parser_error(cv.main, ['--transpose-key', key, CLB_WAV], capsys)


def test_kwiieiya_diffvc_with_transpose_key_is_a_parser_error(capsys):
    import kwiiyatta_amd.resynthesize_voice as rv
    err = _parser_error(rv.main, [CLB_WAV, '--carrier', CLB_WAV, '--diffvc', '--transpose-key', '3'], capsys)
    assert '--diffvc' in err and '--transpose-key' in err


def test_model_round_trip_keeps_f0_stats(tmp_path):
    import kwiiyatta_amd as k
    stats = (5.1, 0.21, 5.4, 0.17)
    path = tmp_path / 'model.npz'
    _trained_stack(stats).save(path)
    loaded = k.MelCepstrumConverter(components=2).load(path)
    assert loaded.f0_stats == stats
    assert all(isinstance(v, float) for v in loaded.f0_stats)
    # without statistics: no key in the file, None after loading
    _trained_stack(None).save(path)
    with np.load(path) as z:
        assert 'f0_stats' not in z.files
    assert k.MelCepstrumConverter(components=2).load(path).f0_stats is None


def _old_model(path):
    """a model file as written before the f0 statistics existed"""
    conv = _trained_stack()
    gmm = conv.gmm
    with open(path, 'wb') as fh:
        np.savez(fh, format=conv.MODEL_FORMAT, order=24, fs=16000, frame_period=5, weights=gmm.weights_,
                 means=gmm.means_, covariances=gmm.covariances_)


def test_old_model_loads_without_f0_stats(tmp_path):
    import kwiiyatta_amd as k
    path = tmp_path / 'old.npz'
    _old_model(path)
    conv = k.MelCepstrumConverter(components=2).load(path)
    assert conv.f0_stats is None and conv.order == 24 and conv.fs == 16000


def test_convert_f0_with_old_model_asks_to_retrain(tmp_path, capsys):
    import kwiiyatta_amd.convert_voice as cv
    path = tmp_path / 'old.npz'
    _old_model(path)
    err = _parser_error(cv.main, ['--convert-f0', '--transpose-key', '2.5', '--converter-model', str(path),
                                  '--result-dir', str(tmp_path / 'out'), CLB_WAV], capsys)
    assert 'no f0 statistics' in err and 'retrain' in err
    assert not (tmp_path / 'out').exists()


def chan_merge(triples):
    """the device merge (kwy_logf0_moments_merge) restated: Chan's pairwise combination, a left fold in index order"""
    n, mean, m2 = 0.0, 0.0, 0.0
    for nb, mb, m2b in triples:
        if nb == 0.0:
            continue
        if n == 0.0:
            n, mean, m2 = nb, mb, m2b
            continue
        nn = n + nb
        delta = mb - mean
        mean = mean + delta * (nb / nn)
        m2 = (m2 + m2b) + delta * delta * (n * nb / nn)
        n = nn
    return n, mean, m2


def two_pass(x):
    if len(x) == 0:
        return 0.0, 0.0, 0.0
    mean = x.sum() / len(x)
    return float(len(x)), mean, float(((x - mean) ** 2).sum())


def test_chan_merge_equals_two_pass():
    rng = np.random.RandomState(3)
    for trial in range(20):
        lengths = rng.randint(0, 400, size=rng.randint(1, 12))
        lengths[rng.randint(len(lengths))] = 0            # an all-unvoiced track somewhere
        parts = [np.log(rng.uniform(70, 400, size=n)) for n in lengths]
        if trial % 5 == 0:
            parts[0] = np.log(np.array([123.0]))            # a single voiced frame
        merged = chan_merge([two_pass(p) for p in parts])
        direct = two_pass(np.concatenate(parts))
        assert merged[0] == direct[0]
        assert merged[1] == pytest.approx(direct[1], rel=1e-14, abs=0)
        assert merged[2] == pytest.approx(direct[2], rel=1e-12, abs=0)
    assert chan_merge([(0.0, 0.0, 0.0)] * 3) == (0.0, 0.0, 0.0)
