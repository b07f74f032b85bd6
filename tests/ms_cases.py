"""The modulation-spectrum postfilter stated in numpy -- the yardstick of tests/test_ms_cases.py (its own claims) and of
tests/test_ms_gpu.py (the kernels of kwy_ms.hip against it) -- with the generators of their inputs and the bounds.

For one column x[0..T-1] of a (T, cols) matrix and a transform length L >= T:

    m    = mean(x)                     (gv_cases.column_moments: a constant column's mean is its value)
    z[t] = x[t] - m (t < T), 0 (T <= t < L);   Z = rfft(z);   s[f] = log(max(|Z[f]|^2, DBL_MIN) / T)
    s'[f] = (1 - k) s[f] + k (sigmaN[f] / sigmaG[f] (s[f] - muG[f]) + muN[f]);   g[f] = exp((s'[f] - s[f]) / 2), g[0] = 1
    y[t] = base[t] + (irfft(g Z)[t] - z[t])

Statistics are (n, mean, M2) per (column, bin >= 1), folded by Welford's step one utterance at a time; bin 0 has none.
Functions take `variant`, the name of a one-line mutation (MUTANTS), so that test_ms_cases.py can show that its claims
tell the definition from its near misses; nothing else passes it."""
import numpy as np

import gv_cases

U = 2.0 ** -53            # unit roundoff of float64
DBL_MIN = np.finfo(np.float64).tiny

TRANSFORM_LENGTHS = (512, 1024, 2048, 4096, 8192)
LENGTHS_512 = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512)
SHAPES = tuple((T, 512) for T in LENGTHS_512) + ((513, 1024), (1000, 1024), (1024, 1024), (2201, 4096), (8192, 8192))
COLS = (1, 25, 41, 64)
MUTANTS = ('no_over_T', 'ratio_inverted', 'bin0_filtered', 'mean_not_restored', 'gain_without_half')


def centred(col, length):
    """(z, mean, valid): the zero-padded deviations of one column, its mean, and whether it has a spectrum at all
    (T >= 2 and M2 != 0)"""
    col = np.asarray(col, dtype=np.float64)
    T = len(col)
    z = np.zeros(length)
    if T > length:
        raise ValueError(f'T = {T} rows are longer than the transform length L = {length}')
    if T == 0:
        return z, 0.0, False
    mean = col[0] if np.all(col == col[0]) else col.sum() / T
    z[:T] = col - mean
    return z, mean, bool(T >= 2 and (z * z).sum() != 0)


def log_power(Z, T, variant=None):
    p = np.maximum(Z.real * Z.real + Z.imag * Z.imag, DBL_MIN)
    return np.log(p if variant == 'no_over_T' else p / T)


def log_spectra(x, length, variant=None):
    """(spectra (cols, L/2 + 1), valid (cols,) int32); the row of an invalid column is zero"""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((x.shape[1], length // 2 + 1))
    valid = np.zeros(x.shape[1], dtype=np.int32)
    for d in range(x.shape[1]):
        z, _, ok = centred(x[:, d], length)
        if ok:
            out[d] = log_power(np.fft.rfft(z), len(x), variant)
            valid[d] = 1
    return out, valid


def new_accumulator(cols, length):
    return np.zeros((cols, length // 2 + 1, 3))


def stats_update(acc, spectra, valid):
    """Welford's step over the utterances of spectra (count, cols, K) in index order, in place; bin 0 is left alone"""
    for s, v in zip(spectra, valid):
        for d in np.flatnonzero(v):
            n = acc[d, 1:, 0] + 1.0
            delta = s[d, 1:] - acc[d, 1:, 1]
            mean = acc[d, 1:, 1] + delta / n
            acc[d, 1:, 2] += delta * (s[d, 1:] - mean)
            acc[d, 1:, 1] = mean
            acc[d, 1:, 0] = n
    return acc


def statistics(mats, length):
    acc = new_accumulator(np.asarray(mats[0]).shape[1], length)
    for m in mats:
        s, v = log_spectra(m, length)
        stats_update(acc, s[None], v[None])
    return acc


def gains(s, g3, n3, k, variant=None):
    """(g, bad) of one column: s (K,), g3 / n3 its (K, 3) statistics.  bad marks the bins >= 1 that keep g = 1 because
    their statistics or their gain are unusable"""
    K = len(s)
    g = np.ones(K)
    bad = np.zeros(K, dtype=bool)
    with np.errstate(all='ignore'):
        sG, sN = np.sqrt(g3[:, 2] / g3[:, 0]), np.sqrt(n3[:, 2] / n3[:, 0])
        ok = ((g3[:, 0] >= 2) & (n3[:, 0] >= 2) & np.isfinite(g3[:, 1]) & np.isfinite(n3[:, 1])
              & np.isfinite(sG) & (sG > 0) & np.isfinite(sN) & (sN >= 0))
        ratio = sG / sN if variant == 'ratio_inverted' else sN / sG
        sp = (1.0 - k) * s + k * (ratio * (s - g3[:, 1]) + n3[:, 1])
        gain = np.exp(sp - s) if variant == 'gain_without_half' else np.exp((sp - s) / 2.0)
    ok &= np.isfinite(gain)
    first = 0 if variant == 'bin0_filtered' else 1
    g[first:] = np.where(ok, gain, 1.0)[first:]
    bad[first:] = ~ok[first:]
    return g, bad


def postfilter(x, stats_g, stats_n, k=1.0, base=None, first_col=1, variant=None):
    """(y, status): status counts the bins that kept g = 1 for unusable statistics or gain.  Columns below first_col,
    invalid columns (T < 2, M2 == 0) and everything at k == 0 are base, bit for bit."""
    x = np.asarray(x, dtype=np.float64)
    base = x if base is None else np.asarray(base, dtype=np.float64)
    length = 2 * (stats_g.shape[1] - 1)
    T = len(x)
    y = base.copy()
    status = 0
    if T > length:
        raise ValueError(f'T = {T} rows are longer than the transform length L = {length}')
    if k == 0:
        return y, status
    for d in range(first_col, x.shape[1]):
        z, mean, ok = centred(x[:, d], length)
        if not ok:
            continue
        Z = np.fft.rfft(z)
        g, bad = gains(log_power(Z, T, variant), stats_g[d], stats_n[d], k, variant)
        status += int(bad.sum())
        zf = np.fft.irfft(g * Z, n=length)[:T]
        y[:, d] = base[:, d] + (zf - z[:T])
        if variant == 'mean_not_restored':
            y[:, d] -= mean
    return y, status


def convert_chain(plain, diff_base, stats_g, stats_n, ms, gv, gv_strength, first_col=1):
    """the converter's composition: the modulation-spectrum filter first, then the global-variance filter on its
    output with that output's moments.  diff_base None: the plain conversion."""
    p1 = postfilter(plain, stats_g, stats_n, ms, first_col=first_col)[0] if ms > 0 else plain
    b1 = p1 if diff_base is None else (postfilter(plain, stats_g, stats_n, ms, base=diff_base, first_col=first_col)[0]
                                       if ms > 0 else diff_base)
    if gv_strength > 0:
        return gv_cases.postfilter(p1, gv, gv_strength, base=b1, first_col=first_col)[0]
    return b1


# ---- bounds (reasoned from the number format, not measured) -------------------------------------------------------
def column_scale(col, length):
    """(||z||_2, dm, BZ): the deviations' norm, the mean error 4 T u max|x| any summation order may have, and the bin
    error u (4 log2 L + 8) ||z||_2 + T dm (a transform of L points rounds log2 L butterfly levels; the mean's error is
    a constant over T samples, so at most T dm in a bin)"""
    z, _, _ = centred(col, length)
    T = len(col)
    norm = np.sqrt((z * z).sum())
    dm = 4 * T * U * np.abs(col).max() if T else 0.0
    return norm, dm, U * (4 * np.log2(length) + 8) * norm + T * dm


def log_spectrum_bound(col, length):
    """(bound (K,), usable (K,)): |ds[f]| <= 2.5 BZ / |Z[f]| where BZ / |Z[f]| <= 0.1 (d log |Z|^2 = 2 d|Z| / |Z|, and
    a quarter more for the second order); the other bins are not comparable"""
    z, _, _ = centred(col, length)
    _, _, bz = column_scale(col, length)
    with np.errstate(divide='ignore'):
        rel = bz / np.abs(np.fft.rfft(z))
    return 2.5 * rel, rel <= 0.1


def output_bound(col, length, gmax, k, rdev):
    """|dy| <= gmax (1 + k rdev) (16 u log2 L ||z||_2 + 2 sqrt(T) dm): two transforms' roundings scaled by the largest
    gain, the gain's own sensitivity to the error of s (d s'/ds = 1 + k (ratio - 1)), and the mean's error through both"""
    norm, dm, _ = column_scale(col, length)
    return gmax * (1 + k * rdev) * (16 * U * np.log2(length) * norm + 2 * np.sqrt(len(col)) * dm)


def filter_bounds(x, stats_g, stats_n, k, first_col=1):
    """the output bound per column (cols,), from the yardstick's own gains; 0 for the columns that are copied"""
    x = np.asarray(x, dtype=np.float64)
    length = 2 * (stats_g.shape[1] - 1)
    out = np.zeros(x.shape[1])
    for d in range(first_col, x.shape[1]):
        z, _, ok = centred(x[:, d], length)
        if not ok or k == 0:
            continue
        g, bad = gains(log_power(np.fft.rfft(z), len(x)), stats_g[d], stats_n[d], k)
        use = ~bad
        use[0] = False
        with np.errstate(all='ignore'):
            ratio = np.sqrt(stats_n[d][:, 2] / stats_n[d][:, 0]) / np.sqrt(stats_g[d][:, 2] / stats_g[d][:, 0])
        rdev = np.abs(ratio[use] - 1).max() if use.any() else 0.0
        out[d] = output_bound(x[:, d], length, g.max(), k, rdev)
    return out


# ---- generators ---------------------------------------------------------------------------------------------------
def matrix(rng, rows, cols, max_offset=1.0):
    """gv_cases.matrix with offsets of at most `max_offset` standard deviations"""
    return gv_cases.matrix(rng, rows, cols, max_offset=max_offset)


def stats_for(x, length, rng):
    """(G, N), each (cols, L/2 + 1, 3), around the matrix's own log-spectra s: muG = s + N(0, 0.5), sigmaG in
    [0.8, 1.5], sigmaN / sigmaG in [0.5, 2], muN = muG + N(0, 0.5), n = 8, bin 0 without statistics.  Arbitrary
    statistics give gains of 1e50 and would test overflow only: the gains of these are at most e^3 (asserted)."""
    s, _ = log_spectra(x, length)
    shape = s.shape
    mu_g = s + 0.5 * rng.standard_normal(shape)
    sigma_g = rng.uniform(0.8, 1.5, size=shape)
    sigma_n = sigma_g * 2.0 ** rng.uniform(-1, 1, size=shape)
    mu_n = mu_g + 0.5 * rng.standard_normal(shape)
    G = np.stack([np.full(shape, 8.0), mu_g, 8.0 * sigma_g ** 2], axis=-1)
    N = np.stack([np.full(shape, 8.0), mu_n, 8.0 * sigma_n ** 2], axis=-1)
    G[:, 0] = 0.0
    N[:, 0] = 0.0
    for d in range(shape[0]):
        assert gains(s[d], G[d], N[d], 1.0)[0].max() <= np.exp(3.0)
    return np.ascontiguousarray(G), np.ascontiguousarray(N)
