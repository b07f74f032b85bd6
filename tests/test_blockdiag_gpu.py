"""Block-diagonal covariance fit on the device (csrc/kwy_gmmfit_bd.hip): the building blocks and the whole fit against
the masked full-covariance EM in numpy (blockdiag_cases.py), the status word, the conversion of such a mixture, and the
way from the command-line option to a model file."""
import argparse
import types

import numpy as np
import pytest

import blockdiag_cases as bd
from conftest import CLB_DIR, CLB_WAV, SLT_DIR

pytestmark = pytest.mark.gpu


# ---- building blocks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,D,M', bd.BLOCK_SHAPES)
def test_statistics_match_the_masked_numpy_em(n, D, M):
    """sums, the three covariance diagonals, finalisation, expansion and the E-step against numpy, set up as
    test_gmm_fit.test_hip_statistics_match_numpy and at its tolerances"""
    import torch
    from kwiiyatta_amd.converter.gmm_fit import HipStatsBlockDiag
    X = bd.make_data(n, D, min(M, 8), seed=1)
    labels = np.random.default_rng(2).integers(0, M, n)
    labels[:M] = np.arange(M)
    h = D // 2
    i = np.arange(h)
    hs, ns = HipStatsBlockDiag(X, M), bd.MaskedNumpyStats(X, M)
    with hs.scope():
        for s in (hs, ns):
            s.set_resp_from_labels(labels)
        sh, sn = hs.sums().cpu().numpy(), ns.sums().numpy()
        assert np.allclose(sh, sn, rtol=1e-12, atol=1e-12)
        hs.means_from(hs.stats)
        ns.means_from(ns.sums())
        ch, cn = hs.cov(hs.stats).cpu().numpy(), ns.cov().numpy()
        assert ch.shape == (M, 3, h)
        want = np.stack((cn[:, i, i], cn[:, h + i, h + i], cn[:, i, h + i]), axis=1)
        assert np.allclose(ch, want, rtol=1e-10, atol=1e-10)
        assert np.array_equal(hs.cov(None).cpu().numpy(), ch)
        hs.finalize(hs.stats, hs.sbd, 1e-3)
        ns.finalize(torch.from_numpy(sn), torch.from_numpy(cn), 1e-3)
        wh, mh, covh = hs.get_params()
        assert np.allclose(wh, ns.weights, rtol=1e-12) and np.allclose(mh, ns.means, rtol=1e-10, atol=1e-12)
        assert covh.shape == (M, D, D) and bd.obeys_pattern(covh)
        assert np.allclose(covh, ns.covs, rtol=1e-9, atol=1e-10)
        packed = hs.covs_bd.cpu().numpy()
        assert np.array_equal(covh[:, i, i], packed[:, 0]) and np.array_equal(covh[:, h + i, h + i], packed[:, 1])
        assert np.array_equal(covh[:, i, h + i], packed[:, 2])
        llh, lln = float(hs.estep().item()), float(ns.estep().item())
        assert not float(hs.estep_failed().item()) and not ns.failed
        print(f'n={n} D={D} M={M}: log-likelihood {llh:.12e} vs {lln:.12e}')
        assert abs(llh - lln) <= 1e-9 * abs(lln)
        assert np.allclose(hs.resp.cpu().numpy(), ns.resp, rtol=1e-7, atol=1e-10)
        # parameters that went in as full matrices come back as they went
        hs.set_params(ns.weights, ns.means, ns.covs)
        back = hs.get_params()
        assert np.array_equal(np.triu(back[2]), np.triu(ns.covs)) and np.array_equal(back[0], ns.weights)


def test_estep_reports_an_indefinite_block_and_recovers():
    """c^2 >= a b in one block: `estep_failed()` is non-zero and nothing raises; the next E-step on valid parameters
    succeeds, clears the word and inherits nothing"""
    from kwiiyatta_amd.converter.gmm_fit import HipStatsBlockDiag
    n, D, M = 300, 6, 3
    X = bd.make_data(n, D, M, seed=4)
    ns = bd.MaskedNumpyStats(X, M)
    ns.set_resp_from_labels(bd.random_labels(n, M, 4))
    import torch
    ns.means_from(ns.sums())
    ns.finalize(ns.sums(), ns.cov(), 1e-3)
    good = ns.get_params()
    want = float(ns.estep().item())
    hs = HipStatsBlockDiag(X, M)
    for spoil in ('cross', 'variance', 'nan'):
        bad = good[2].copy()
        if spoil == 'cross':
            bad[1, 2, 5] = bad[1, 5, 2] = 1.5 * np.sqrt(bad[1, 2, 2] * bad[1, 5, 5])
        elif spoil == 'variance':
            bad[2, 0, 0] = 0.0
        else:
            bad[0, 4, 4] = np.nan
        with hs.scope():
            hs.set_params(good[0], good[1], bad)
            hs.estep()
            assert float(hs.estep_failed().item()) != 0
            assert torch.isfinite(hs.resp).all()
            hs.set_params(*good)
            ll = float(hs.estep().item())
            assert float(hs.estep_failed().item()) == 0
            assert abs(ll - want) <= 1e-9 * abs(want)
            assert np.allclose(hs.resp.cpu().numpy(), ns.resp, rtol=1e-7, atol=1e-10)


def test_entries_refuse_what_they_cannot_do():
    """an odd D, D < 2, D > 160, M outside 1..256, n < 1 and NULL pointers are KWY_EINVAL with a message"""
    import torch
    from kwiiyatta_amd import _lib
    lib, ctx = _lib.lib, _lib.default_context()
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    p = _lib.c_vp(buf.data_ptr())
    for n, D, M in ((8, 5, 2), (8, 0, 2), (8, 162, 2), (8, 4, 0), (8, 4, 257), (0, 4, 2)):
        assert lib.kwy_gmm_em_estep_bd_dev(ctx.handle, p, n, D, M, p, p, p, p, p, p) == _lib.KWY_EINVAL
        assert lib.kwy_gmm_em_cov_bd_dev(ctx.handle, p, n, D, M, p, p, None, p) == _lib.KWY_EINVAL
        assert 'gmm_em_bd' in ctx.error()
    for D, M in ((5, 2), (4, 257)):
        assert lib.kwy_gmm_em_finalize_bd_dev(ctx.handle, p, p, D, M, 1e-6, p, p) == _lib.KWY_EINVAL
        assert lib.kwy_gmm_expand_bd_dev(ctx.handle, p, D, M, p) == _lib.KWY_EINVAL
    assert lib.kwy_gmm_em_estep_bd_dev(ctx.handle, p, 8, 4, 2, p, p, None, p, p, p) == _lib.KWY_EINVAL
    assert 'null pointer' in ctx.error()
    assert lib.kwy_gmm_em_cov_bd_dev(ctx.handle, p, 8, 4, 2, p, None, None, p) == _lib.KWY_EINVAL
    assert lib.kwy_gmm_em_finalize_bd_dev(ctx.handle, p, None, 4, 2, 1e-6, p, p) == _lib.KWY_EINVAL
    assert lib.kwy_gmm_expand_bd_dev(ctx.handle, None, 4, 2, p) == _lib.KWY_EINVAL
    ctx.sync()


# ---- the whole fit -----------------------------------------------------------------------------------------------------
def _agrees(g, ref):
    stats, lower_bound, converged, n_iter = ref
    assert g.n_iter_ == n_iter and g.converged_ == converged
    print(f'n_iter {g.n_iter_}, lower bound {g.lower_bound_:.12f} vs {lower_bound:.12f}')
    assert abs(g.lower_bound_ - lower_bound) <= 1e-8 * abs(lower_bound)
    w, mu, cov = stats.get_params()
    assert np.allclose(g.weights_, w, rtol=1e-6, atol=1e-10)
    assert np.allclose(g.means_, mu, rtol=1e-6, atol=1e-8)
    assert np.allclose(g.covariances_, cov, rtol=1e-5, atol=1e-8)
    assert bd.obeys_pattern(g.covariances_)


@pytest.mark.parametrize('case,iterations', list(zip(bd.FIT_CASES, bd.FIT_ITERATIONS)))
def test_fit_matches_the_masked_numpy_em(case, iterations):
    """the fit from sklearn's k-means labels at default tol and max_iter: the reference's iteration count, bound and
    parameters"""
    from kwiiyatta_amd.converter.gmm_fit import GaussianMixtureHIP
    n, D, M, seed = case
    X, labels, ref = bd.kmeans_case(*case)
    assert ref[3] == iterations and ref[2]
    g = GaussianMixtureHIP(M, covariance_structure='block_diag').fit(X, labels=labels)
    assert g.covariance_structure == 'block_diag' and g.covariance_type == 'full'
    assert g.covariances_.shape == (M, D, D)
    _agrees(g, ref)


def test_fit_with_the_device_k_means_and_twice():
    """without `labels` the device's own k-means feeds the fit: same iteration count and bound; two fits of one input
    are equal bit for bit"""
    from kwiiyatta_amd.converter.gmm_fit import GaussianMixtureHIP
    case = bd.FIT_CASES[0]
    n, D, M, seed = case
    X, labels, ref = bd.kmeans_case(*case)
    fits = [GaussianMixtureHIP(M, random_state=seed, covariance_structure='block_diag').fit(X) for _ in range(2)]
    assert fits[0].n_iter_ == ref[3] and fits[0].converged_ == ref[2]
    assert abs(fits[0].lower_bound_ - ref[1]) <= 1e-8 * abs(ref[1])
    for name in ('weights_', 'means_', 'covariances_'):
        assert np.array_equal(getattr(fits[0], name), getattr(fits[1], name))
    assert fits[0].lower_bound_ == fits[1].lower_bound_
    again = GaussianMixtureHIP(M, covariance_structure='block_diag').fit(X, labels=labels)
    once = GaussianMixtureHIP(M, covariance_structure='block_diag').fit(X, labels=labels)
    assert np.array_equal(again.covariances_, once.covariances_) and again.lower_bound_ == once.lower_bound_


def test_at_two_dimensions_the_structures_agree():
    from kwiiyatta_amd.converter.gmm_fit import GaussianMixtureHIP
    case = bd.FIT_CASES[2]
    n, D, M, seed = case
    assert D == 2
    X, labels, ref = bd.kmeans_case(*case)
    full = GaussianMixtureHIP(M).fit(X, labels=labels)
    g = GaussianMixtureHIP(M, covariance_structure='block_diag').fit(X, labels=labels)
    assert g.n_iter_ == full.n_iter_ and g.converged_ == full.converged_
    assert abs(g.lower_bound_ - full.lower_bound_) <= 1e-8 * abs(full.lower_bound_)
    assert np.allclose(g.weights_, full.weights_, rtol=1e-6, atol=1e-10)
    assert np.allclose(g.means_, full.means_, rtol=1e-6, atol=1e-8)
    assert np.allclose(g.covariances_, full.covariances_, rtol=1e-5, atol=1e-8)


# ---- conversion ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fitted():
    from kwiiyatta_amd.converter.gmm_fit import GaussianMixtureHIP
    n, D, M, seed = bd.FIT_CASES[0]
    X, labels, _ = bd.kmeans_case(n, D, M, seed)
    return X, GaussianMixtureHIP(M, covariance_structure='block_diag').fit(X, labels=labels)


def _plain(g):
    return types.SimpleNamespace(weights_=g.weights_.copy(), means_=g.means_.copy(), covariances_=g.covariances_.copy(),
                                 covariance_type='full', n_components=len(g.weights_))


def test_frame_wise_conversion_is_the_closed_form(fitted):
    from kwiiyatta_amd.converter import GMMFeatureConverter
    X, g = fitted
    conv = GMMFeatureConverter(components=g.n_components, covariance='block_diag')
    conv.gmm = g
    x = np.ascontiguousarray(X[:500, :X.shape[1] // 2])
    got = conv.convert(x, mlpg=False)
    ref = bd.frame_wise_closed_form(g.weights_, g.means_, g.covariances_, x)
    assert got.shape == ref.shape
    print(f'frame-wise conversion: max error {np.abs(got - ref).max():.3e}')
    assert np.abs(got - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1.0)


def test_trajectory_conversion_takes_the_mixture_as_a_full_one(fitted):
    from kwiiyatta_amd.converter import GMMFeatureConverter
    X, g = fitted
    conv = GMMFeatureConverter(components=g.n_components, covariance='block_diag')
    conv.gmm = g
    x = np.ascontiguousarray(X[:500, :X.shape[1] // 2])
    got = conv.convert(x, mlpg=True)
    assert np.isfinite(got).all()
    conv.gmm = _plain(g)
    assert np.array_equal(conv.convert(x, mlpg=True), got)


# ---- stack and drivers -----------------------------------------------------------------------------------------------------
def test_corpus_fit_is_the_direct_fit():
    import torch
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd.converter.gmm_fit import GaussianMixtureHIP
    n, D, M, seed = bd.FIT_CASES[0]
    X = bd.make_data(n, D, M, seed)
    direct = GaussianMixtureHIP(n_components=4, random_state=0, covariance_structure='block_diag').fit(X)
    Xd = torch.from_numpy(X).to('cuda')
    torch.cuda.synchronize()
    g = corpus.fit_converter(Xd, components=4, seed=0, covariance='block_diag')
    assert g.covariance_structure == 'block_diag' and g.n_iter_ == direct.n_iter_
    for name in ('weights_', 'means_', 'covariances_'):
        assert np.array_equal(getattr(g, name), getattr(direct, name))
    assert bd.obeys_pattern(g.covariances_)
    assert not bd.obeys_pattern(corpus.fit_converter(Xd, components=4, seed=0).covariances_)


def _config(argv):
    import kwiiyatta_amd as k
    conf = k.Config(argparse.ArgumentParser())
    conf.add_converter_arguments()
    conf.parser.parse_args(argv, namespace=conf)
    return conf


def test_option_trains_saves_and_loads_a_block_diagonal_converter(tmp_path):
    import kwiiyatta_amd.convert_voice as cv
    model = tmp_path / 'model.npz'
    common = ['--source', CLB_DIR, '--target', SLT_DIR, '--max-files', '2', '--converter-seed', '0',
              '--converter-components', '4', '--converter-model', str(model)]
    conf = _config(common + ['--converter-covariance', 'block_diag'])
    np.random.seed(0)
    trained = conf.train_converter(use_delta=True)
    assert trained.fs == 16000 and trained.covariance == 'block_diag'
    covs = trained.gmm.covariances_
    assert covs.shape == (4, 144, 144) and bd.obeys_pattern(covs)
    with np.load(model) as z:
        assert str(z['covariance']) == 'block_diag'
    fresh = _config(common)
    loaded = fresh.train_converter(use_delta=True)
    assert loaded is not trained and loaded.covariance == 'block_diag'
    assert np.array_equal(loaded.gmm.covariances_, covs)
    a = cv.convert(conf, trained, CLB_WAV)
    b = cv.convert(fresh, loaded, CLB_WAV)
    assert a.fs == b.fs and len(a.data) > 0 and np.array_equal(a.data, b.data)
