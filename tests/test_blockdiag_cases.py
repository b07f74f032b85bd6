"""Block-diagonal covariance fit: what needs no device -- the reference (masked full-covariance EM in numpy) keeps the
lower bound from falling, the constructor rules, the command-line option and the model file's key.  The kernels are
tested on the GPU (test_blockdiag_gpu.py)."""
import argparse
import sys

import numpy as np
import pytest

import blockdiag_cases as bd
from conftest import CLB_WAV
from numpy_em_stats import NumpyStats


# ---- the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,D,M,seed', bd.MONOTONE_CASES)
def test_masked_em_never_lowers_the_bound(n, D, M, seed):
    """EM in the block-diagonal family is exact (the M-step's maximum is the empirical covariance restricted to the
    pattern), so the lower bound of the masked numpy EM never falls: 25 iterations from random labels, every step at
    least -1e-12 |bound| (the worst one measured is -8.4e-15)."""
    X = bd.make_data(n, D, M, seed)
    stats, _, _, n_iter = bd.reference_fit(X, M, bd.random_labels(n, M, seed), max_iter=25, tol=0.0)
    trace = np.array(stats.trace)
    assert n_iter == 25 and len(trace) == 25 and np.isfinite(trace).all()
    steps = np.diff(trace)
    worst = (steps / np.abs(trace[1:])).min()
    print(f'n={n} D={D} M={M}: bound {trace[0]:.6f} -> {trace[-1]:.6f}, worst relative step {worst:.3e}')
    assert (steps >= -1e-12 * np.abs(trace[1:])).all()
    assert (stats.covs[:, bd.pattern_mask(D) == 0] == 0).all()


def test_at_two_dimensions_the_mask_changes_nothing():
    """D = 2: one 2 x 2 block is a full covariance, so the masked run equals the unmasked one exactly"""
    n, D, M, seed = 300, 2, 2, 3
    X = bd.make_data(n, D, M, seed)
    labels = bd.random_labels(n, M, seed)
    masked = bd.reference_fit(X, M, labels, max_iter=25, tol=0.0)
    plain = bd.reference_fit(X, M, labels, max_iter=25, tol=0.0, stats_class=NumpyStats)
    assert masked[1:] == plain[1:]
    for a, b in zip(masked[0].get_params(), plain[0].get_params()):
        assert np.array_equal(a, b)


def test_closed_form_is_the_conditional_mean_of_the_expanded_mixture():
    """the frame-wise closed form of the case file against the general formula on full matrices"""
    rng = np.random.default_rng(0)
    M, h = 3, 4
    a, b = rng.uniform(0.5, 2, (M, h)), rng.uniform(0.5, 2, (M, h))
    c = rng.uniform(-0.9, 0.9, (M, h)) * np.sqrt(a * b)
    covs = np.zeros((M, 2 * h, 2 * h))
    i = np.arange(h)
    covs[:, i, i], covs[:, h + i, h + i], covs[:, i, h + i], covs[:, h + i, i] = a, b, c, c
    means, weights = rng.standard_normal((M, 2 * h)), np.array([0.2, 0.5, 0.3])
    x = rng.standard_normal((7, h))
    from scipy.stats import multivariate_normal
    post = np.stack([w * multivariate_normal(mu[:h], S[:h, :h]).pdf(x) for w, mu, S in zip(weights, means, covs)], 1)
    post /= post.sum(1, keepdims=True)
    ref = sum(post[:, m:m + 1] * (means[m, h:] + (x - means[m, :h]) @ np.linalg.solve(covs[m, :h, :h], covs[m, :h, h:]))
              for m in range(M))
    assert np.allclose(bd.frame_wise_closed_form(weights, means, covs, x), ref, rtol=1e-12, atol=1e-12)


# ---- constructor rules -------------------------------------------------------------------------------------------------
def test_mixture_constructor_rules():
    from kwiiyatta_amd.converter.gmm_fit import GaussianMixtureHIP, fit_one_call
    g = GaussianMixtureHIP(4)
    assert g.covariance_structure == 'full' and g.covariance_type == 'full'
    g = GaussianMixtureHIP(4, covariance_structure='block_diag')
    assert g.covariance_structure == 'block_diag' and g.covariance_type == 'full'
    assert GaussianMixtureHIP.covariance_type == 'full'
    with pytest.raises(NotImplementedError, match='banded'):
        GaussianMixtureHIP(4, covariance_structure='banded')
    for other in ('diag', 'tied', 'spherical', 'block_diag'):
        with pytest.raises(NotImplementedError):
            GaussianMixtureHIP(4, covariance_type=other)
    with pytest.raises(NotImplementedError, match='block_diag'):
        fit_one_call(np.zeros((8, 4)), 2, covariance_structure='block_diag')


def test_an_odd_dimension_is_refused_before_the_device_is_touched(monkeypatch):
    from kwiiyatta_amd.converter import gmm_fit

    def no_device(*args, **kwargs):
        raise AssertionError('statistics were allocated')
    monkeypatch.setattr(gmm_fit.HipStats, '__init__', no_device)
    g = gmm_fit.GaussianMixtureHIP(2, covariance_structure='block_diag')
    with pytest.raises(ValueError, match='D = 5'):
        g.fit(np.zeros((20, 5)))


def test_converter_constructor_rules():
    import kwiiyatta_amd as k
    from kwiiyatta_amd.converter import GMMFeatureConverter
    assert GMMFeatureConverter(components=2).covariance == 'full'
    conv = GMMFeatureConverter(components=2, covariance='block_diag')
    assert conv.covariance == 'block_diag' and conv.gmm.covariance_structure == 'block_diag'
    assert conv.gmm.covariance_type == 'full'
    with pytest.raises(NotImplementedError):
        GMMFeatureConverter(components=2, covariance='diag')
    stack = k.MelCepstrumConverter(components=2, covariance='block_diag')
    assert stack.covariance == 'block_diag'
    assert k.MelCepstrumConverter(components=2).covariance == 'full'
    conv.init_gmm(3)
    assert conv.covariance == 'full'


# ---- the option --------------------------------------------------------------------------------------------------------
def _config(argv):
    import kwiiyatta_amd as k
    conf = k.Config(argparse.ArgumentParser())
    conf.add_converter_arguments()
    conf.parser.parse_args(argv, namespace=conf)
    return conf


def _parser_error(main, argv, capsys):
    old = sys.argv
    sys.argv = ['prog'] + argv
    try:
        with pytest.raises(SystemExit) as e:
            main()
    finally:
        sys.argv = old
    assert e.value.code == 2
    return capsys.readouterr().err


def test_option_parses_and_reaches_the_converter():
    assert _config([]).converter_covariance is None
    assert _config([]).create_converter().covariance == 'full'
    for word in ('full', 'block_diag'):
        conf = _config(['--converter-covariance', word, '--converter-components', '2'])
        assert conf.converter_covariance == word
        assert conf.create_converter().covariance == word


@pytest.mark.parametrize('word', ['diag', 'Full', 'block-diag', ''])
def test_other_words_are_parser_errors(word, capsys):
    import kwiiyatta_amd.convert_voice as cv
    import kwiiyatta_amd.evaluate_voice as ev
    assert '--converter-covariance' in _parser_error(cv.main, ['--converter-covariance', word, CLB_WAV], capsys)
    assert '--converter-covariance' in _parser_error(ev.main, ['--converter-covariance', word], capsys)


# ---- the model file ------------------------------------------------------------------------------------------------------
def _trained_stack(covariance):
    import kwiiyatta_amd as k
    conv = k.MelCepstrumConverter(components=2, random_state=0, covariance=covariance)
    rng = np.random.RandomState(0)
    gmm = conv.gmm
    gmm.weights_ = np.array([0.25, 0.75])
    gmm.means_ = rng.standard_normal((2, 6))
    gmm.covariances_ = np.stack([np.eye(6) * 0.5, np.eye(6) * 2.0])
    conv.order, conv.fs, conv.frame_period = 24, 16000, 5
    return conv


def test_model_file_keeps_the_structure(tmp_path):
    import kwiiyatta_amd as k
    path = tmp_path / 'bd.npz'
    _trained_stack('block_diag').save(path)
    with np.load(path) as z:
        assert str(z['covariance']) == 'block_diag'
    loaded = k.MelCepstrumConverter(components=2).load(path)
    assert loaded.covariance == 'block_diag' and loaded.gmm.covariance_structure == 'block_diag'
    assert loaded.gmm.covariance_type == 'full'
    # a full model's file has no such key, and a file without it loads as 'full' -- into any stack
    full = tmp_path / 'full.npz'
    _trained_stack('full').save(full)
    with np.load(full) as z:
        assert 'covariance' not in z.files
    for covariance in ('full', 'block_diag'):
        assert k.MelCepstrumConverter(components=2, covariance=covariance).load(full).covariance == 'full'


def test_a_structure_that_conflicts_with_the_model_is_a_parser_error(tmp_path, capsys):
    import kwiiyatta_amd.convert_voice as cv
    path = tmp_path / 'bd.npz'
    _trained_stack('block_diag').save(path)
    err = _parser_error(cv.main, ['--converter-covariance', 'full', '--converter-model', str(path), '--result-dir',
                                  str(tmp_path / 'out'), CLB_WAV], capsys)
    assert 'trained with --converter-covariance block_diag' in err and 'not full' in err and 'retrain' in err
    assert not (tmp_path / 'out').exists()
    for extra in ([], ['--converter-covariance', 'block_diag']):
        conf = _config(['--converter-model', str(path), '--converter-components', '2'] + extra)
        assert conf.train_converter(use_delta=True).covariance == 'block_diag'
