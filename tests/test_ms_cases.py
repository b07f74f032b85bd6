"""The claims of the numpy yardstick tests/ms_cases.py itself (no GPU): against an 80-bit direct transform it stays
within an eighth of the bounds the kernels are held to; identical statistics, zero strength, the spectrum the filter
leaves, the Welford fold, unusable bins and constant columns, the composition with the global-variance filter -- and
each one-line mutant of the definition breaks one of them."""
import numpy as np
import pytest

import gv_cases as gc
import ms_cases as mc

L = 512


def _long_reference(x, G, N, k, base=None):
    """(s (cols, K), y) of a (T, cols) matrix in np.longdouble throughout: a direct DFT with exact twiddle indices"""
    ld = np.longdouble
    T, cols = x.shape
    K = L // 2 + 1
    pi = 4 * np.arctan(ld(1))                                  # (np.pi is a double)
    ang = 2 * pi * ((np.arange(K)[:, None] * np.arange(L)[None, :]) % L).astype(ld) / L
    c, s_ = np.cos(ang), np.sin(ang)
    base = x if base is None else base
    S, y = np.zeros((cols, K), dtype=ld), np.array(base, dtype=ld)
    for d in range(cols):
        col = x[:, d].astype(ld)
        z = np.zeros(L, dtype=ld)
        z[:T] = col - col.sum() / T
        re, im = c @ z, -(s_ @ z)
        S[d] = np.log(np.maximum(re * re + im * im, ld(mc.DBL_MIN)) / T)
        if d == 0:
            continue
        sG, sN = np.sqrt(G[d, 1:, 2] / G[d, 1:, 0]).astype(ld), np.sqrt(N[d, 1:, 2] / N[d, 1:, 0]).astype(ld)
        sp = (1 - ld(k)) * S[d, 1:] + ld(k) * (sN / sG * (S[d, 1:] - G[d, 1:, 1]) + N[d, 1:, 1])
        g = np.ones(K, dtype=ld)
        g[1:] = np.exp((sp - S[d, 1:]) / 2)
        w = np.full(K, ld(2))
        w[0] = w[-1] = 1
        zf = ((w * g * re) @ c - (w * g * im) @ s_) / L
        y[:, d] = np.asarray(base[:, d], dtype=ld) + (zf[:T] - z[:T])
    return S, y


@pytest.mark.parametrize('offset', [0.0, 10.0, 500.0])
@pytest.mark.parametrize('T', [2, 3, 65, 257, 511, 512])
def test_numpy_is_within_an_eighth_of_the_bounds(T, offset):
    rng = np.random.RandomState(1000 + T)
    x = mc.matrix(rng, T, 3, max_offset=offset)
    G, N = mc.stats_for(x, L, rng)
    s, valid = mc.log_spectra(x, L)
    assert valid.tolist() == [1, 1, 1]
    for k in (1.0, 0.5):
        S, Y = _long_reference(x, G, N, k)
        y, status = mc.postfilter(x, G, N, k)
        assert status == 0
        bounds = mc.filter_bounds(x, G, N, k)
        for d in range(3):
            bound, usable = mc.log_spectrum_bound(x[:, d], L)
            assert usable[1:].all(), (d, int((~usable[1:]).sum()))          # no bin >= 1 is skipped
            err = np.abs((s[d] - S[d]).astype(np.float64))[1:]
            assert np.all(err <= bound[1:] / 8), (d, (err / bound[1:]).max())
            if d >= 1:
                err = np.abs((y[:, d] - Y[:, d]).astype(np.float64)).max()
                assert err <= bounds[d] / 8, (d, k, err / bounds[d])
        assert y[:, 0].tobytes() == x[:, 0].tobytes()


def _case(T=257, cols=4, seed=5, offset=1.0):
    rng = np.random.RandomState(seed)
    x = mc.matrix(rng, T, cols, max_offset=offset)
    return (x,) + mc.stats_for(x, L, rng) + (rng,)


def _identity_holds(variant=None):
    x, G, _, _ = _case()
    y, status = mc.postfilter(x, G, G, 1.0, variant=variant)
    return status == 0 and np.all(np.abs(y - x).max(axis=0) <= np.maximum(mc.filter_bounds(x, G, G, 1.0), 0))


def _spectrum_reached(variant=None):
    """at T == L the filter's output has the spectrum s' on every bin >= 1"""
    x, G, N, _ = _case(T=L)
    ok = True
    for k in (1.0, 0.5):
        y, _ = mc.postfilter(x, G, N, k, variant=variant)
        s, _ = mc.log_spectra(x, L)
        sy, _ = mc.log_spectra(y, L)
        for d in range(1, x.shape[1]):
            ratio = np.sqrt(N[d, 1:, 2] / N[d, 1:, 0]) / np.sqrt(G[d, 1:, 2] / G[d, 1:, 0])
            want = (1 - k) * s[d, 1:] + k * (ratio * (s[d, 1:] - G[d, 1:, 1]) + N[d, 1:, 1])
            bound, usable = mc.log_spectrum_bound(y[:, d], L)
            ok = ok and usable[1:].all() and bool(np.all(np.abs(sy[d, 1:] - want) <= bound[1:]))
    return ok


def _mean_kept(variant=None):
    """bin 0 untouched: at T == L (nothing of z' is cut off) every filtered column keeps its mean, to the mean's own
    error and the output bound"""
    x, G, N, _ = _case(T=L, offset=10.0)
    y, _ = mc.postfilter(x, G, N, 1.0, variant=variant)
    tol = mc.filter_bounds(x, G, N, 1.0) + 2 * 4 * len(x) * mc.U * np.abs(x).max(axis=0)
    return bool(np.all(np.abs(y.mean(axis=0) - x.mean(axis=0))[1:] <= tol[1:]))


def _learnt_statistics_give_status_zero(variant=None):
    """statistics folded by `statistics` carry nothing at bin 0, and the filter does not ask for it"""
    rng = np.random.RandomState(3)
    mats = [mc.matrix(rng, T, 3) for T in (100, 200, 300)]
    stats = mc.statistics(mats, L)
    assert np.all(stats[:, 0] == 0) and np.all(stats[:, 1:, 0] == 3)
    return mc.postfilter(mats[0], stats, stats, 1.0, first_col=0, variant=variant)[1] == 0


def _periodogram_comparable(variant=None):
    """/ T: white noise of one variance has the same mean log-spectrum whatever its length"""
    rng = np.random.RandomState(9)
    means = [mc.log_spectra(rng.standard_normal((T, 8)), L, variant=variant)[0][:, 1:].mean() for T in (128, 512)]
    return abs(means[0] - means[1]) <= 0.2          # (log 4 = 1.39 apart without the division; s.e. of a mean of 2048 bins: 0.03)


CLAIMS = (_identity_holds, _spectrum_reached, _mean_kept, _learnt_statistics_give_status_zero, _periodogram_comparable)


@pytest.mark.parametrize('claim', CLAIMS, ids=lambda c: c.__name__)
def test_claim(claim):
    assert claim()


@pytest.mark.parametrize('variant', mc.MUTANTS)
def test_every_mutant_breaks_a_claim(variant):
    broken = [c.__name__ for c in CLAIMS if not c(variant)]
    print(variant, '->', broken)
    assert broken, variant


def test_zero_strength_and_untouched_columns_are_base_bit_for_bit():
    x, G, N, rng = _case()
    base = x + rng.standard_normal(x.shape)
    for b in (None, base):
        y, status = mc.postfilter(x, G, N, 0.0, base=b)
        assert status == 0 and y.tobytes() == (x if b is None else b).tobytes()
        y, _ = mc.postfilter(x, G, N, 1.0, base=b, first_col=2)
        assert y[:, :2].tobytes() == np.ascontiguousarray((x if b is None else b)[:, :2]).tobytes()
        assert np.all(y[:, 2:] != (x if b is None else b)[:, 2:])
    # the differential form is the plain filter's change on another base
    y0, _ = mc.postfilter(x, G, N, 1.0)
    y1, _ = mc.postfilter(x, G, N, 1.0, base=base)
    assert np.abs((y1 - base) - (y0 - x)).max() <= 4 * mc.U * (np.abs(y0).max() + np.abs(y1).max() + np.abs(x).max())


def test_welford_fold_against_two_passes_and_invalid_columns():
    rng = np.random.RandomState(21)
    mats = [mc.matrix(rng, T, 5) for T in (1, 40, 77, 300, 2, 512, 129)]
    mats[3][:, 2] = 0.1                                       # a constant column: skipped for that utterance only
    spectra, valid = zip(*(mc.log_spectra(m, L) for m in mats))
    spectra, valid = np.stack(spectra), np.stack(valid)
    assert valid[0].tolist() == [0] * 5 and valid[3].tolist() == [1, 1, 0, 1, 1]
    assert np.all(spectra[0] == 0) and np.all(spectra[3, 2] == 0)
    acc = mc.stats_update(mc.new_accumulator(5, L), spectra, valid)
    assert acc.tobytes() == mc.statistics(mats, L).tobytes()
    # one utterance at a time, or in two blocks: the same bits
    two = mc.stats_update(mc.stats_update(mc.new_accumulator(5, L), spectra[:3], valid[:3]), spectra[3:], valid[3:])
    assert two.tobytes() == acc.tobytes()
    assert np.all(acc[:, 0] == 0)
    for d in range(5):
        rows = spectra[valid[:, d] == 1, d, 1:]
        n = len(rows)
        assert n == (5 if d == 2 else 6) and np.all(acc[d, 1:, 0] == n)
        # sums of n terms of size max|s| (the mean) and sum s^2 (M2: no algorithm's terms are larger)
        scale = np.abs(rows).max(axis=0)
        assert np.all(np.abs(acc[d, 1:, 1] - rows.mean(axis=0)) <= 8 * n * mc.U * scale)
        m2 = ((rows - rows.mean(axis=0)) ** 2).sum(axis=0)
        assert np.all(np.abs(acc[d, 1:, 2] - m2) <= 8 * n * mc.U * (rows ** 2).sum(axis=0))
        assert np.all(np.abs(np.sqrt(acc[d, 1:, 2] / n) - rows.std(axis=0)) <= 8 * n * mc.U * (rows ** 2).sum(axis=0)
                      / (2 * n * rows.std(axis=0)) + 4 * mc.U * rows.std(axis=0))


def test_unusable_bins_constant_columns_and_short_matrices():
    x, G, N, rng = _case(cols=6)
    x[:, 4] = -2.5
    G, N = G.copy(), N.copy()
    G[1, 3, 1] = np.nan                  # a mean that is not finite
    G[1, 4, 2] = 0.0                     # sigmaG == 0
    N[2, 5, 0] = 1.0                     # n < 2
    G[2, 6, 2] = np.inf                  # sigmaG not finite
    N[3, 7, 2] = -1.0                    # sigmaN not a number
    N[3, 8, 2] = 0.0                     # sigmaN == 0 is usable: the bin is flattened onto muN
    N[5, 9, 1] = 1e4                     # a gain that overflows
    G[4, 10, 1] = np.nan                 # in the constant column: never looked at
    y, status = mc.postfilter(x, G, N, 1.0)
    assert status == 6
    assert y[:, 4].tobytes() == x[:, 4].tobytes() and y[:, 0].tobytes() == x[:, 0].tobytes()
    s, valid = mc.log_spectra(x, L)
    assert valid.tolist() == [1, 1, 1, 1, 0, 1]
    g, bad = mc.gains(s[1], G[1], N[1], 1.0)
    assert bad.nonzero()[0].tolist() == [3, 4] and g[3] == g[4] == 1.0 and g[0] == 1.0
    g, bad = mc.gains(s[3], G[3], N[3], 1.0)
    assert bad.nonzero()[0].tolist() == [7] and g[8] == np.exp((N[3, 8, 1] - s[3, 8]) / 2)
    for T in (0, 1):
        short = x[:T]
        y, status = mc.postfilter(short, G, N, 1.0)
        assert status == 0 and y.tobytes() == short.tobytes()
        assert mc.log_spectra(short, L)[1].tolist() == [0] * 6
    with pytest.raises(ValueError, match='T = 513.*L = 512'):
        mc.postfilter(np.zeros((513, 6)), G, N, 1.0)


@pytest.mark.parametrize('diff', [False, True])
def test_composition_with_the_global_variance_filter(diff):
    x, G, N, rng = _case(cols=5)
    b = x + 0.1 * rng.standard_normal(x.shape) if diff else None
    gv = gc.gv_for_ratios(x, np.full(4, 1.5))
    p1, _ = mc.postfilter(x, G, N, 1.0)
    b1 = mc.postfilter(x, G, N, 1.0, base=b)[0] if diff else p1
    want, _ = gc.postfilter(p1, gv, 1.0, base=b1)
    got = mc.convert_chain(x, b, G, N, 1.0, gv, 1.0)
    assert got.tobytes() == want.tobytes()
    # the moments are those of the modulation-spectrum filter's output, not of the conversion
    other, _ = gc.postfilter(x, gv, 1.0, base=b1)
    assert np.abs(got - other).max() > 1e-6 * np.abs(x).max()
    # either filter alone
    assert mc.convert_chain(x, b, G, N, 1.0, gv, 0.0).tobytes() == b1.tobytes()
    assert mc.convert_chain(x, b, G, N, 0.0, gv, 1.0).tobytes() == gc.postfilter(x, gv, 1.0, base=b)[0].tobytes()
    if not diff:           # at strength 1 the variance is the statistic's, whatever the first filter did
        for d in range(1, 5):
            assert abs(np.var(got[:, d]) / gv[d] - 1) <= gc.variance_claim_bound(p1, d)
