"""The inputs and references of the fit's kernel-level tests (fit_cases.py), checked without a device: the longdouble
primitives, the properties the GPU assertions rest on (threshold values on both sides, active-group counts, skipped-frame
allowances below the terms that must not be skipped, distance gaps, ties) and the float64 restatement's error against
the longdouble reference, which is what the GPU tolerances are built from (test_fit_kernels_gpu.py)."""
import numpy as np
import pytest

import fit_cases as fc
from numpy_em_stats import NumpyStats

LD, EPS = fc.LD, fc.EPS


# ---- the references themselves ---------------------------------------------------------------------------------------
def test_cholesky_and_substitution_hold_to_longdouble_precision():
    rng = np.random.default_rng(0)
    for D, cond in ((1, 1.0), (5, 1e3), (40, 1e6)):
        C = fc._spd(rng, D, cond)
        L = fc.cholesky(C)
        assert np.abs(L @ L.T - fc.ld(C)).max() <= 8 * D * np.finfo(LD).eps * np.abs(C).max()
        assert (np.triu(L, 1) == 0).all() and (np.diag(L) > 0).all()
        B = fc.ld(rng.standard_normal((D, 7)))
        Z = fc.forward_subst(L, B)
        assert np.abs(L @ Z - B).max() <= 8 * D * np.finfo(LD).eps * np.abs(L).max() * np.abs(Z).max()
        assert np.allclose(L.astype(np.float64), np.linalg.cholesky(C), rtol=1e-9 * cond ** 0.5, atol=0)
    assert fc.cholesky(np.array([[1.0, 1.0], [1.0, 1.0]])) is None          # a zero pivot
    assert fc.cholesky(np.array([[1.0, 2.0], [2.0, 1.0]])) is None          # a negative one


def test_log_density_agrees_with_scipy_where_float64_is_good():
    from scipy.stats import multivariate_normal
    rng = np.random.default_rng(1)
    D, M, n = 6, 3, 20
    w = np.array([0.2, 0.5, 0.3])
    mu = rng.standard_normal((M, D))
    C = np.stack([fc._spd(rng, D, 10.0) for _ in range(M)])
    X = rng.standard_normal((n, D))
    W = fc.weighted_log_density(X, w, mu, C)
    want = np.stack([np.log(w[m]) + multivariate_normal(mu[m], C[m]).logpdf(X) for m in range(M)], axis=1)
    assert np.abs(W.astype(np.float64) - want).max() <= 1e-12 * np.abs(want).max()
    lse = fc.log_sum_exp(W)
    assert np.abs(fc.responsibilities(W, lse).sum(1) - 1).max() <= 8 * np.finfo(LD).eps
    # the block-diagonal form is the full one on matrices of its pattern
    h = D // 2
    abc = np.stack((rng.uniform(0.5, 2, (M, h)), rng.uniform(0.5, 2, (M, h)), rng.uniform(-0.4, 0.4, (M, h))), axis=1)
    full = np.zeros((M, D, D))
    i = np.arange(h)
    full[:, i, i], full[:, h + i, h + i] = abc[:, 0], abc[:, 1]
    full[:, i, h + i] = full[:, h + i, i] = abc[:, 2]
    a, b = fc.weighted_log_density_bd(X, w, mu, abc), fc.weighted_log_density(X, w, mu, full)
    assert np.abs(a - b).max() <= 64 * np.finfo(LD).eps * np.abs(b).max()


# ---- 1, 2: soft responsibilities -------------------------------------------------------------------------------------
def _values_present(case):
    R, nk = case['resp'], case['nk']
    rel = R / np.where(nk > 0, nk, 1.0)[None, :]
    return {'0': (R == 0).any(), '2^-201': (R == 2.0 ** -201).any(), '2^-200': (R == 2.0 ** -200).any(),
            '2^-199': (R == 2.0 ** -199).any(), '2^-71 nk': (rel == 2.0 ** -71).any(),
            '2^-70 nk': (rel == 2.0 ** -70).any(), '2^-69 nk': (rel == 2.0 ** -69).any(), '1e-30': (R == 1e-30).any(),
            '1e-5': (R == 1e-5).any(), '0.3': (R == 0.3).any(), '1': (R == 1.0).any()}


@pytest.mark.parametrize('name', list(fc.SOFT_CASES))
def test_soft_case_has_the_layout_the_assertions_rest_on(name):
    c = fc.soft_case(name)
    R, nk, n, M, D = c['resp'], c['nk'], c['n'], c['M'], c['D']
    G = (n + 3) // 4
    assert R.shape == (n, M) and (R >= 0).all() and (R <= 1).all()
    # nk is the column sum as the sums kernel would hand it over
    import math
    assert all(nk[m] == math.fsum(R[:, m]) for m in range(M))              # (fsum: the correctly rounded sum)
    assert np.abs(fc.ld(R).sum(0) - nk).max() <= EPS * nk.max()
    # every value of the list, wherever the case has room for a whole cycle of column types and their huge rows
    if M >= len(fc.TYPES) and G >= 64:
        missing = [k for k, v in _values_present(c).items() if not v]
        assert not missing, missing
    # a huge row carries exactly one weight, a threshold value of its owner, and lies 2^18 .. 2^19 from the owner's mean
    for t, m in c['huge_rows'].items():
        assert np.count_nonzero(R[t]) == 1
        assert R[t, m] in (2.0 ** -200, 2.0 ** -199, nk[m] * 2.0 ** -70, nk[m] * 2.0 ** -69)
        d = np.abs(c['X'][t] - c['means'][m])
        assert (d >= fc.HUGE * (1 - 1e-9)).all() and (d <= 2 * fc.HUGE * (1 + 1e-9)).all()
    # active groups with the sums handed over: as the column's type says
    counts = fc.active_group_counts(c, True)
    for m, ty in enumerate(c['types']):
        want = G if ty == 'all' else max(1, G // 2) if ty == 'half' else min(fc.COUNT[ty], G)
        if ty == 'tiny':                 # active through its huge rows alone: as many as the case had left for it
            want = sum(1 for owner in c['huge_rows'].values() if owner == m)
        assert counts[m] == want == c['counts'][m], (m, ty, counts[m])
    # without them the threshold is 2^-200 everywhere: 'none' and 'tiny' columns keep their counts, the others gain
    free = fc.active_group_counts(c, False)
    assert (free >= counts).all()
    for m, ty in enumerate(c['types']):
        if ty in ('none', 'tiny'):
            assert free[m] == counts[m]
    print(f'{name}: active groups of {G} with sums {sorted(set(counts.tolist()))}, without {sorted(set(free.tolist()))}, '
          f'{len(c["huge_rows"])} huge rows, splits {fc.cov_splits(n, M)}')


@pytest.mark.parametrize('name', ['d144_m16_n257', 'd160_m17_n257', 'd16_m65_n513', 'd17_m17_n2049', 'd17_m128_n3601'])
def test_soft_case_groups_sit_on_both_sides_of_the_threshold(name):
    """groups all below the threshold, groups active through ONE weight that equals the threshold (its other three
    below it), a cut last group active for one column and idle for another"""
    c = fc.soft_case(name)
    R, nk, n, M = c['resp'], c['nk'], c['n'], c['M']
    G = (n + 3) // 4
    pad = np.zeros((4 * G, M))
    pad[:n] = R
    rmin = fc.r_min_of(nk, True)
    above = (pad >= rmin[None, :]).reshape(G, 4, M)
    below_nonzero = ((pad > 0) & (pad < rmin[None, :])).reshape(G, 4, M)
    at = (pad == rmin[None, :]).reshape(G, 4, M)
    assert (~above.any(1) & below_nonzero.any(1)).any()                       # idle although it holds weights
    lone = (above.sum(1) == 1) & at.any(1)
    assert lone.any() and (lone & below_nonzero.any(1)).any()                 # exactly one entry, exactly at r_min
    assert n % 4 and above[G - 1].any(0).any() and (~above[G - 1].any(0)).any()
    assert ((above.sum(1) == 1) & ~at.any(1)).any()                           # ... and one entry well above it


def test_soft_cases_cover_the_seams():
    cases = [fc.soft_case(k) for k in fc.SOFT_CASES]
    assert {c['D'] for c in cases} >= {1, 16, 17, 33, 97, 144, 160}
    assert {c['M'] for c in cases} >= {1, 3, 16, 17, 65, 128, 256}
    assert {c['n'] for c in cases} >= {1, 3, 4, 5, 31, 33, 257, 513, 2049, 3601}
    assert max(fc.cov_splits(c['n'], c['M']) for c in cases) >= 8
    counts = set()
    for c in cases:
        counts |= set(fc.active_group_counts(c, True).tolist())
    assert counts >= {0, 1, 7, 8, 9}
    for c in cases:
        assert c['M'] * c['n'] * c['D'] ** 2 <= 2e8 and c['n'] <= 4000
    # the sparse case of the stale-scratch test: splits without tiles, a mixture without a group -- after a dense
    # run of the same shape, so that what the dense run left in the scratch lies where the sparse one must write zeros
    dense, sparse = fc.soft_case('dense_d33_m3_n2049'), fc.soft_case('sparse_d33_m3_n2049')
    assert (dense['D'], dense['M'], dense['n']) == (sparse['D'], sparse['M'], sparse['n'])
    ns = fc.cov_splits(sparse['n'], sparse['M'])
    tiles = (fc.active_group_counts(sparse, True) + 7) // 8
    assert 0 in tiles.tolist() and ns >= 4 and (tiles < ns).all()
    assert ((fc.active_group_counts(dense, True) + 7) // 8 >= ns).all()


@pytest.mark.parametrize('with_stats', [True, False])
@pytest.mark.parametrize('name', list(fc.SOFT_CASES))
def test_a_frame_that_must_be_kept_outweighs_all_that_may_be_skipped(name, with_stats):
    """include/kwy.h lets the covariance sum leave out the frames below r_min = max(2^-200, 2^-70 nk) and no others.  The
    GPU test allows an entry the sum of the skippable terms plus rounding; so that dropping ANY other frame fails it, the
    term of every frame at r_min and above exceeds that allowance on some diagonal entry -- and the term of every frame
    that sits AT a threshold value (the huge rows) exceeds allowance plus rounding bound, a thousandfold."""
    c = fc.soft_case(name)
    ref = fc.soft_reference(name)
    allow = fc.skip_allowance(c, with_stats)
    rmin = fc.r_min_of(c['nk'], with_stats)
    rounding = fc.bound(ref['cov_err64'], ref['cov_max'])
    worst, worst_huge = np.inf, np.inf
    for m in range(c['M']):
        r = c['resp'][:, m]
        keep = np.flatnonzero(r >= rmin[m])
        if not len(keep):
            continue
        term = r[keep, None] * (c['X'][keep] - c['means'][m]) ** 2
        a = np.diagonal(allow[m])[None, :]
        margin = (term - a).max(1)
        assert (margin > 0).all(), (m, keep[margin <= 0])
        worst = min(worst, float((term / np.maximum(a, 1e-300)).max(1).min()))
        for k, t in enumerate(keep):
            if c['huge_rows'].get(int(t)) == m:
                ratio = float((term[k] / (a[0] + rounding[m])).max())
                worst_huge = min(worst_huge, ratio)
                assert ratio >= 1e3, (m, t, ratio)
    print(f'{name} stats={with_stats}: smallest kept term / allowance {worst:.2e}, '
          f'smallest threshold term / (allowance + rounding bound) {worst_huge:.2e}')


@pytest.mark.parametrize('name', list(fc.SOFT_CASES))
def test_float64_statistics_miss_the_reference_by_rounding_only(name):
    """the error the GPU bounds are built from: NumpyStats (float64, BLAS) against the longdouble sums and covariances,
    per mixture; a sum of n terms cannot miss by more than n eps times the sum of the terms' magnitudes"""
    c = fc.soft_case(name)
    ref = fc.soft_reference(name)
    X, R, mu = c['X'], c['resp'], c['means']
    mag_sums = np.hstack((R.sum(0)[:, None], R.T @ np.abs(X))).max(1)
    mag_cov = np.array([((np.abs(X - mu[m]) ** 2).T @ R[:, m]).max() for m in range(c['M'])])
    for what, mag in (('sums', mag_sums), ('cov', mag_cov)):
        err, big = ref[what + '_err64'], ref[what + '_max']
        assert np.isfinite(err).all() and (err <= (c['n'] + 4) * EPS * mag).all(), what
        b = fc.bound(err, big)
        assert (b >= 4 * EPS * big).all() and (b >= fc.KERNEL_MULTIPLE * err).all()
        rel = err / np.where(big > 0, big, 1.0)
        print(f'{name} {what}: float64 error / largest magnitude, worst mixture {rel.max():.2e}; '
              f'bound / largest magnitude {(b / np.where(big > 0, big, 1.0)).max():.2e}')
    if c['D'] % 2 == 0:
        assert (ref['cov_bd_err64'] <= (c['n'] + 4) * EPS * mag_cov).all()
        # the three-vector form is the three diagonals of the full one
        h = c['D'] // 2
        i = np.arange(h)
        full = ref['cov']
        three = np.stack((full[:, i, i], full[:, h + i, h + i], full[:, i, h + i]), axis=1)
        assert (np.abs(three - ref['cov_bd']) <= 64 * np.finfo(LD).eps * ref['cov_bd_max'][:, None, None] * c['n']).all()
    asym = np.abs(ref['cov'] - ref['cov'].transpose(0, 2, 1)).reshape(c['M'], -1).max(1)
    assert (asym <= (c['n'] + 4) * np.finfo(LD).eps * mag_cov).all()


# ---- 3: the E-step ---------------------------------------------------------------------------------------------------
def test_estep_cases_cover_the_seams():
    cases = [fc.estep_case(k) for k in fc.ESTEP_CASES]
    assert {c['D'] for c in cases} >= {1, 16, 17, 144, 160}
    assert {c['M'] for c in cases} >= {1, 2, 16, 17, 64, 65, 256}
    assert {c['n'] for c in cases} >= {1, 31, 32, 33, 255, 256, 257, 2047}
    assert any(c['M'] == 64 and c['n'] >= 1793 for c in cases)
    assert all(fc.estep_case_bd(k)['D'] % 2 == 0 for k in fc.ESTEP_CASES)
    near = below = 0
    for k in fc.ESTEP_CASES:
        for r in (fc.estep_reference(k)['resp'], fc.estep_reference_bd(k)['resp']):
            near += int(((r >= fc.TINY) & (r < 1e-290)).sum())
            below += int((r < fc.TINY).sum())
    assert near >= 100 and below >= 100          # posteriors next to the smallest normal double, and under it


@pytest.mark.parametrize('bd', [False, True])
@pytest.mark.parametrize('name', list(fc.ESTEP_CASES))
def test_estep_case_and_its_float64_error(name, bd):
    c = fc.estep_case_bd(name) if bd else fc.estep_case(name)
    ref = fc.estep_reference_bd(name) if bd else fc.estep_reference(name)
    M, D, n = c['M'], c['D'], c['n']
    if M > 1:
        assert np.array_equal(c['covs'][0], c['covs'][M - 1]) and np.array_equal(c['means'][0], c['means'][M - 1])
        assert c['weights'][0] == c['weights'][M - 1]
        assert np.array_equal(ref['resp'][:, 0], ref['resp'][:, M - 1])
    if M >= 16:
        assert c['weights'].max() / c['weights'].min() >= 1e11
    conds = np.array([np.linalg.cond(C) for C in c['covs']])
    assert conds.max() <= 4e6 and (D < 16 or conds.max() >= (3e4 if bd else 1e5))
    if n >= 31:
        assert {'typical', 'on-mean', 'gap', 'far'} <= set(c['kind'].tolist())
        on = np.flatnonzero(c['kind'] == 'on-mean')
        assert all((c['X'][t] == c['means']).all(1).any() for t in on)
    # the float64 restatement: these lines and NumpyStats.estep are one computation
    from scipy.special import logsumexp
    ns = NumpyStats(c['X'], M)
    ns.set_params(c['weights'], c['means'], c['covs'])
    total = float(ns.estep().item())
    assert np.array_equal(ns.resp, np.exp(ref['wlp64'] - logsumexp(ref['wlp64'], axis=1)[:, None]))
    assert total == ref['lse64'].sum()
    # its error is rounding, amplified by the conditioning at most: a bound on delta that does not come from a kernel
    assert ref['wlp_err64'] <= 4e6 * EPS * ref['wlp_max']
    assert ref['delta'] == max(fc.KERNEL_MULTIPLE * ref['wlp_err64'], 4 * EPS * ref['wlp_max'])
    # (the reference's own rounding: that of max + log(sum), eps |lse|, next to the sum of M values)
    assert (np.abs(ref['resp'].sum(1) - 1) <= np.finfo(LD).eps * (2 * M + 2 * np.abs(ref['lse']))).all()
    assert len(ref['parts']) == (n + 255) // 256 and abs(ref['parts'].sum() - ref['lse'].sum()) <= 1e-15 * abs(ref['lse'].sum())
    if M == 1:
        assert np.array_equal(ref['lse'], ref['wlp'][:, 0])          # the parts are sums of the log-densities themselves
    print(f'{name} bd={bd}: |wlp| <= {ref["wlp_max"]:.2e}, float64 error {ref["wlp_err64"]:.2e}, delta {ref["delta"]:.2e}, '
          f'resp bound e^(2 delta) - 1 = {np.expm1(2 * ref["delta"]):.2e}; parts: float64 error {ref["parts_err64"]:.2e} '
          f'of {ref["parts_max"]:.2e}')


@pytest.mark.parametrize('how', ['zero', 'negative'])
def test_spoilt_covariance_has_the_pivot_it_says(how):
    for name in ('d17_m16_n32', 'd144_m17_n33'):
        c = fc.estep_case(name)
        bad = fc.indefinite_covs(c, how)
        m, k = c['M'] // 2, c['D'] // 2
        assert fc.cholesky(bad[m]) is None
        assert all(fc.cholesky(bad[j]) is not None for j in range(c['M']) if j != m)
        # float64, left-looking as the kernel: the pivot of column k is exactly C[k][k] (the row of L before it is zero)
        L = np.linalg.cholesky(bad[m][:k, :k])
        row = np.linalg.solve(L, bad[m][:k, k])
        assert (row == 0).all() and bad[m][k, k] == (0.0 if how == 'zero' else -1.0)
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(bad[m])


# ---- 4: k-means ------------------------------------------------------------------------------------------------------
def test_km_cases_cover_the_seams():
    shapes = [fc.KM_CASES[k][:3] for k in fc.KM_CASES]
    assert {s[0] for s in shapes} >= {1, 5, 255, 256, 257, 2049}
    assert {s[1] for s in shapes} >= {1, 16, 17, 160}
    assert {s[2] for s in shapes} >= {1, 16, 17, 64, 65, 256}


@pytest.mark.parametrize('name', list(fc.KM_CASES))
def test_km_case_labels_are_decided_by_a_clear_margin(name):
    """labels are compared exactly, so EVERY row's best and second-best reference distance lie at least 1e-9 of the
    larger apart (float64 evaluations differ by 1e-13 of it at the most); the float64 restatement then agrees"""
    c, ref = fc.km_case(name), fc.km_reference(name)
    gaps = fc.distance_gaps(ref['dist'])
    assert gaps.shape == (c['n'],) and (gaps >= fc.GAP).all(), float(gaps.min())
    assert np.array_equal(ref['labels'], ref['labels64'])
    assert np.array_equal(c['Xc'], c['X'] - c['mean'])
    cnt = ref['sums64'][:, 0]
    assert cnt.sum() == c['n'] and (c['M'] == 1 or (cnt == 0).any())      # a centre without rows keeps its place
    on_centre = (np.abs(ref['dist'].min(1) + (fc.ld(c['Xc']) ** 2).sum(1)) <= 1e-15 * (c['Xc'] ** 2).sum(1)).sum()
    assert on_centre >= min(c['n'], c['M']) // 2
    for key in ('colstats', 'colstats_shift', 'Xc', 'xsq', 'newd', 'pots', 'newd_closest', 'pots_closest', 'sums',
                'update', 'shift2'):
        r, err, big = ref[key]
        assert err <= (c['n'] + c['D'] + 4) * EPS * max(big, 1e-300) * 4, key
    print(f'{name}: smallest gap {float(gaps.min()):.2e}; float64 error / largest magnitude: ' +
          ', '.join(f'{k} {ref[k][1] / max(ref[k][2], 1e-300):.1e}' for k in ('colstats', 'xsq', 'newd', 'pots', 'sums',
                                                                          'update', 'shift2')))


def test_tie_case_duplicates_are_nearest_for_their_rows():
    c = fc.tie_case()
    blocks = [(lo // 64, (lo % 64) // 16, lo % 16, hi // 64, (hi % 64) // 16, hi % 16) for lo, hi in fc.TIE_PAIRS]
    assert any(b[0] == b[3] and b[1] == b[4] and b[2] != b[5] for b in blocks)      # one block, two lanes
    assert any(b[0] == b[3] and b[1] != b[4] and b[2] == b[5] for b in blocks)      # one lane, two blocks
    assert any(b[0] != b[3] for b in blocks)                                        # two groups of 64
    for lo, hi in fc.TIE_PAIRS:
        assert lo < hi and np.array_equal(c['centres'][lo], c['centres'][hi])
        assert np.array_equal(c['dist'][:, lo], c['dist'][:, hi])                   # the same bits
        assert (c['labels'][c['near'][lo]] == lo).all()
    gaps = fc.distance_gaps(c['dist'], c['same'])
    assert (gaps >= fc.GAP).all()
