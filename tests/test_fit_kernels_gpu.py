"""The kernels of the mixture fit (kwy_gmmfit.hip, kwy_gmmfit_bd.hip, kwy_kmeans.hip) against the longdouble references
of fit_cases.py: the covariance statistics and the sums on soft responsibilities around the skip threshold, the E-step on
given ill-conditioned parameters, the k-means blocks at the tile seams, ties between duplicate centres.

A kernel may miss the reference by fit_cases.KERNEL_MULTIPLE times what the float64 restatement (NumpyStats) misses it
by, floored at 4 ulp of the largest reference magnitude -- per mixture for the statistics, per case elsewhere; no bound
comes from a kernel's output.  Every check prints its measured error next to its bound (pytest -s); DESIGN.md section 4
has the table of the measured kernel / float64 ratios.  test_fit_cases.py proves the inputs' properties on the CPU."""
import numpy as np
import pytest

import fit_cases as fc

pytestmark = pytest.mark.gpu
LD, EPS = fc.LD, fc.EPS


@pytest.fixture(scope='module')
def ctx():
    """one context for the whole module: every call meets the scratch the calls before it left behind"""
    from kwiiyatta_amd import _lib
    return _lib.Context(0)


def _dev(hs, a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(hs.dev)


def _stats(cls, X, M, ctx):
    return cls(np.array(X), M, ctx=ctx)          # (a writable copy: the cases' arrays are read-only)


def _set_params(hs, c, covs=None):
    hs.set_params(np.array(c['weights']), np.array(c['means']), np.array(c['covs'] if covs is None else covs))


def _needed(err, err64, big):
    """the multiple of the float64 error that `err` needs: 0 where the 4 ulp floor already covers it"""
    err, err64, big = (np.asarray(a, dtype=np.float64) for a in (err, err64, big))
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(err <= 4 * EPS * big, 0.0, np.where(err64 > 0, err / err64, np.inf))


def _check(what, got, ref, err64, big):
    """max-norm: kernel error <= bound(float64 error, largest reference magnitude); prints all of it"""
    err = float(np.abs(fc.ld(got) - ref).max()) if np.size(ref) else 0.0
    b = float(fc.bound(err64, big))
    print(f'{what}: kernel error {err:.3e}, float64 error {err64:.3e}, bound {b:.3e} (needs multiple '
          f'{float(_needed(err, err64, big)):.2f} of {fc.KERNEL_MULTIPLE:g}), largest reference value {big:.3e}')
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), what
    assert err <= b, what


def _check_per_mixture(what, got, ref, err64, big, allow=None):
    """per mixture: the entries' error beyond `allow` <= bound(float64 error, largest magnitude) of that mixture"""
    M = ref.shape[0]
    miss = np.abs(fc.ld(got) - ref)
    over = np.maximum(miss - (allow if allow is not None else 0), 0).reshape(M, -1).max(1).astype(np.float64)
    b = fc.bound(err64, big)
    need = _needed(over, err64, big)
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(b > 0, over / b, np.where(over > 0, np.inf, 0.0))
    worst = int(np.argmax(rel))
    print(f'{what}: error / bound at most {rel.max():.3f}, needs multiple {need.max():.2f} of {fc.KERNEL_MULTIPLE:g} '
          f'(mixture {worst}: error{" beyond the skip allowance" if allow is not None else ""} {over[worst]:.3e}, '
          f'float64 error {err64[worst]:.3e}, bound {b[worst]:.3e}, largest reference value {big[worst]:.3e}); whole case: '
          f'kernel error {over.max():.3e}, float64 error {err64.max():.3e}')
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), what
    assert (over <= b).all(), (what, np.flatnonzero(over > b)[:8])


def _soft_stats(hs, c, ref):
    """a statistics object holding the case's rows, responsibilities and means; the reduced sums as the M-step hands
    them to the covariance kernel: [nk, sum r x] in float64"""
    hs.resp.copy_(_dev(hs, c['resp']))
    hs.means.copy_(_dev(hs, c['means']))
    st = ref['sums'].astype(np.float64)
    st[:, 0] = c['nk']
    return _dev(hs, st)


# ---- 1: covariance statistics on soft weights ------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(fc.SOFT_CASES))
def test_covariance_of_soft_weights_skips_what_it_may_and_nothing_else(name, ctx):
    """k_fit_active, k_fit_active_list, k_fit_cov, k_fit_reduce_sym without the sums (threshold 2^-200) and with them
    (max(2^-200, 2^-70 nk)): every entry within the rounding bound of the UNSKIPPED reference, plus what the frames
    below the threshold weigh there; sxx symmetric to the bit.  k_bd_cov takes the sums and skips nothing."""
    from kwiiyatta_amd.converter.gmm_fit import HipStats, HipStatsBlockDiag
    c, ref = fc.soft_case(name), fc.soft_reference(name)
    hs = _stats(HipStats, c['X'], c['M'], ctx)
    with hs.scope():
        stats = _soft_stats(hs, c, ref)
        for with_stats in (False, True):
            got = hs.cov(stats if with_stats else None).cpu().numpy()
            assert np.array_equal(got, got.transpose(0, 2, 1))
            _check_per_mixture(f'{name} sxx, sums {"given" if with_stats else "absent"}', got, ref['cov'],
                               ref['cov_err64'], ref['cov_max'], fc.skip_allowance(c, with_stats))
    if c['D'] % 2 == 0:
        hb = _stats(HipStatsBlockDiag, c['X'], c['M'], ctx)
        with hb.scope():
            stats = _soft_stats(hb, c, ref)
            for with_stats in (False, True):
                got = hb.cov(stats if with_stats else None).cpu().numpy()
                _check_per_mixture(f'{name} sbd, sums {"given" if with_stats else "absent"}', got, ref['cov_bd'],
                                   ref['cov_bd_err64'], ref['cov_bd_max'])


def test_sparse_covariance_after_a_dense_one_shows_no_stale_scratch(ctx):
    """the same object and context, the same shape: every group active, then mixtures of 0, 1 and 9 active groups over
    five splits -- splits without a tile must store zeros over the dense run's partial sums, the lists and counts must
    be the sparse run's"""
    from kwiiyatta_amd.converter.gmm_fit import HipStats
    dense, sparse = fc.soft_case('dense_d33_m3_n2049'), fc.soft_case('sparse_d33_m3_n2049')
    hs = _stats(HipStats, dense['X'], dense['M'], ctx)
    with hs.scope():
        for c in (dense, sparse, dense, sparse):
            ref = fc.soft_reference(c['name'])
            hs.X.copy_(_dev(hs, c['X']))
            stats = _soft_stats(hs, c, ref)
            for with_stats in (True, False):
                got = hs.cov(stats if with_stats else None).cpu().numpy()
                assert np.array_equal(got, got.transpose(0, 2, 1))
                _check_per_mixture(f'{c["name"]} sxx, sums {"given" if with_stats else "absent"}', got, ref['cov'],
                                   ref['cov_err64'], ref['cov_max'], fc.skip_allowance(c, with_stats))
            if c is sparse:
                none = c['types'].index('none')
                assert (got[none] <= 2.0 ** -190).all()       # (a column of 2^-201s: whatever is kept of it is tiny)


# ---- 2: sums ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(fc.SOFT_CASES))
def test_sums_of_soft_weights(name, ctx):
    """k_fit_sums / k_fit_reduce: M = 65 and 256 (a second and fourth blockIdx.y, wavefronts without a mixture),
    n = 513 and 2049 (a last chunk of one row), n < 4"""
    from kwiiyatta_amd.converter.gmm_fit import HipStats
    c, ref = fc.soft_case(name), fc.soft_reference(name)
    hs = _stats(HipStats, c['X'], c['M'], ctx)
    with hs.scope():
        _soft_stats(hs, c, ref)
        got = hs.sums().cpu().numpy()
    _check_per_mixture(f'{name} sums', got, ref['sums'], ref['sums_err64'], ref['sums_max'])


# ---- 3: the E-step ---------------------------------------------------------------------------------------------------
def _check_estep(what, c, ref, hs):
    """after hs.estep(): status, responsibilities (relative, down to the smallest normal double), twins, row sums, every
    log-likelihood part"""
    M, n = c['M'], c['n']
    assert float(hs.estep_failed().item()) == 0
    resp, parts = hs.resp.cpu().numpy(), hs.ll.cpu().numpy()
    assert np.isfinite(resp).all() and (resp >= 0).all()
    miss = np.abs(fc.ld(resp) - ref['resp'])
    normal = ref['resp'] >= fc.TINY
    rel = float((miss[normal] / ref['resp'][normal]).max())
    allowed = float(np.expm1(2 * ref['delta']))
    need = float(_needed(rel / 2, ref['wlp_err64'], ref['wlp_max']))
    print(f'{what}: resp relative error {rel:.3e} over {int(normal.sum())} normal entries (smallest '
          f'{float(ref["resp"][normal].min()):.3e}), float64 density error {ref["wlp_err64"]:.3e}, bound '
          f'e^(2 delta) - 1 = {allowed:.3e} (needs multiple {need:.2f} of {fc.KERNEL_MULTIPLE:g}); '
          f'{int((~normal).sum())} entries below the normal range, largest got '
          f'{float(resp[~normal].max()) if (~normal).any() else 0.0:.3e}')
    assert (miss <= fc.resp_bound(ref)).all(), what
    if M > 1:
        assert np.array_equal(resp[:, 0], resp[:, M - 1]), what      # equal parameters: equal bits
    off = np.abs(fc.ld(resp).sum(1) - 1).astype(np.float64)
    sb = fc.resp_sum_bound(ref, M)
    print(f'{what}: |sum resp - 1| at most {off.max() / EPS:.1f} ulp, {float((off / sb).max()):.3f} of its bound; '
          f'where |lse| < 100: {off[np.abs(ref["lse"]) < 100].max(initial=0.0) / EPS:.1f} ulp')
    assert (off <= sb).all(), what
    assert parts.shape == ((n + 255) // 256,)
    _check(f'{what} log-likelihood parts', parts, ref['parts'], ref['parts_err64'], ref['parts_max'])


@pytest.mark.parametrize('name', list(fc.ESTEP_CASES))
def test_estep_on_given_parameters(name, ctx):
    """k_fit_prec, k_fit_logprob, k_fit_resp on covariances of condition up to 1e6 and weights over twelve decades"""
    from kwiiyatta_amd.converter.gmm_fit import HipStats
    c, ref = fc.estep_case(name), fc.estep_reference(name)
    hs = _stats(HipStats, c['X'], c['M'], ctx)
    with hs.scope():
        _set_params(hs, c)
        total = hs.estep()
        _check_estep(name, c, ref, hs)
        assert float(total.item()) == float(hs.ll.sum().item())
        if c['M'] == 1 and c['n'] == 1:          # one row, one mixture: the part IS the log-density
            _check(f'{name} part = log-density', hs.ll.cpu().numpy()[0], ref['wlp'][0, 0], ref['wlp_err64'], ref['wlp_max'])


@pytest.mark.parametrize('name', list(fc.ESTEP_CASES))
def test_blockdiag_estep_on_given_parameters(name, ctx):
    """k_bd_prec, k_bd_logprob, k_fit_resp on the same list with an even D and three-diagonal parameters"""
    from kwiiyatta_amd.converter.gmm_fit import HipStatsBlockDiag
    c, ref = fc.estep_case_bd(name), fc.estep_reference_bd(name)
    hs = _stats(HipStatsBlockDiag, c['X'], c['M'], ctx)
    with hs.scope():
        _set_params(hs, c)
        assert np.array_equal(hs.covs_bd.cpu().numpy(), c['abc'])
        hs.estep()
        _check_estep(f'{name} block_diag', c, ref, hs)


@pytest.mark.parametrize('name,how', [('d17_m16_n32', 'zero'), ('d144_m17_n33', 'negative')])
def test_estep_reports_an_indefinite_covariance_and_recovers(name, how, ctx):
    """one mixture of several with a zero (a negative) pivot: the status word is set and nothing raises; the next call on
    the same object with the valid parameters clears it and gives the reference values"""
    from kwiiyatta_amd.converter.gmm_fit import HipStats
    c, ref = fc.estep_case(name), fc.estep_reference(name)
    hs = _stats(HipStats, c['X'], c['M'], ctx)
    with hs.scope():
        _set_params(hs, c, fc.indefinite_covs(c, how))
        hs.estep()
        assert float(hs.estep_failed().item()) != 0
        _set_params(hs, c)
        hs.estep()
        _check_estep(f'{name} after a {how} pivot', c, ref, hs)


# ---- 4: k-means ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(fc.KM_CASES))
def test_kmeans_blocks_at_the_seams(name, ctx):
    """km_colstats, km_begin, km_candidates, km_assign, km_sums, km_update: values against the longdouble reference,
    labels against the exact ones (every row's margin is checked in test_fit_cases.py).  A block that reads another
    block's output reads the REFERENCE's, rounded to float64."""
    import torch
    from kwiiyatta_amd.converter.gmm_fit import HipStats
    c, ref = fc.km_case(name), fc.km_reference(name)
    n, D, M = c['n'], c['D'], c['M']
    hs = _stats(HipStats, c['X'], M, ctx)
    with hs.scope():
        mean = _dev(hs, c['mean'])
        _check(f'{name} colstats', hs.km_colstats(None).cpu().numpy(), *ref['colstats'])
        _check(f'{name} colstats, shifted', hs.km_colstats(mean).cpu().numpy(), *ref['colstats_shift'])
        hs.km_begin(mean)
        assert np.array_equal(hs.Xc.cpu().numpy(), c['Xc'])              # one subtraction: the same bits
        _check(f'{name} centred rows', hs.Xc.cpu().numpy(), *ref['Xc'])
        _check(f'{name} row norms', hs.xsq.cpu().numpy(), *ref['xsq'])
        hs.xsq.copy_(_dev(hs, ref['xsq64']))
        cand = _dev(hs, c['cand'])
        L = len(c['cand'])
        pots = hs.km_candidates(cand, use_closest=False).cpu().numpy()
        _check(f'{name} candidate distances', hs.newd[:L].cpu().numpy(), *ref['newd'])
        _check(f'{name} candidate potentials', pots, *ref['pots'])
        hs.closest.copy_(_dev(hs, ref['closest64']))
        pots = hs.km_candidates(cand, use_closest=True).cpu().numpy()
        _check(f'{name} candidate distances under the closest', hs.newd[:L].cpu().numpy(), *ref['newd_closest'])
        _check(f'{name} candidate potentials under the closest', pots, *ref['pots_closest'])
        centres = _dev(hs, c['centres'])
        assert int(hs.km_assign(centres).item()) == n                    # (from -1 everywhere)
        labels = hs.labels.cpu().numpy()
        wrong = np.flatnonzero(labels != ref['labels'])
        print(f'{name} labels: {len(wrong)} of {n} differ from the reference')
        assert not len(wrong), (wrong[:8], labels[wrong[:8]], ref['labels'][wrong[:8]])
        onehot = np.zeros((n, M))
        onehot[np.arange(n), ref['labels']] = 1.0
        assert np.array_equal(hs.resp.cpu().numpy(), onehot)
        assert int(hs.km_assign(centres).item()) == 0                    # the same centres: nothing changes
        st = hs.km_sums().cpu().numpy()
        assert np.array_equal(st[:, 0], ref['sums64'][:, 0])             # counts are exact
        _check(f'{name} centroid sums', st, *ref['sums'])
        new = torch.empty((M, D), dtype=torch.float64, device=hs.dev)
        shift2 = hs.km_update(_dev(hs, ref['sums64']), centres, new).cpu().numpy()
        _check(f'{name} new centres', new.cpu().numpy(), *ref['update'])
        _check(f'{name} squared shifts', shift2, *ref['shift2'])
        empty = ref['sums64'][:, 0] == 0
        assert np.array_equal(new.cpu().numpy()[empty], c['centres'][empty]) and (shift2[empty] == 0).all()
        hs.km_end()


def test_equal_centres_give_the_lower_index(ctx):
    """duplicate centres make equal distances, the same bits: the lower index wins between two lanes of a 16-column
    block, two blocks of a lane, and two groups of 64 centres (k_km_assign's lane and row arg-min, k_km_labels)"""
    from kwiiyatta_amd.converter.gmm_fit import HipStats
    c = fc.tie_case()
    hs = _stats(HipStats, c['Xc'], c['M'], ctx)
    with hs.scope():
        hs.km_begin(_dev(hs, np.zeros(c['D'])))                         # centred on zero: Xc = X
        assert np.array_equal(hs.Xc.cpu().numpy(), c['Xc'])
        hs.km_assign(_dev(hs, c['centres']))
        labels = hs.labels.cpu().numpy()
        hs.km_end()
    for lo, hi in fc.TIE_PAIRS:
        got = labels[c['near'][lo]]
        print(f'centres {lo} = {hi}: their rows are labelled {sorted(set(got.tolist()))}')
        assert (got == lo).all(), (lo, hi, got)
    assert np.array_equal(labels, c['labels'])
