"""The formant shift of include/kwy.h ("formant shift") stated in numpy, and the cases its tests share.  This module is
the reference of tests/test_formant_cases.py and tests/test_formant_gpu.py and never imports the product.

    u_k = k / rho (one IEEE division),  j = floor(u_k),  a = u_k - j,  l = log(sp[t])
    out[t, k] = sp[t, K-1]                          if j >= K-1
              = sp[t, j]                            if a == 0
              = exp(l[j] + a * (l[j+1] - l[j]))     otherwise
"""
import numpy as np

U = 2.0 ** -53                          # unit roundoff of float64
EPS = 2.0 ** -52
RATIO_RANGE = (0.5, 2.0)
MAX_K = 2049                            # the envelope width of the longest transform CheapTrick accepts (4096 points)
WIDTHS = (2, 3, 65, 513, 1025, MAX_K)
ROWS = (0, 1, 3, 67)
RATIOS = (0.5, 2.0 ** (-3 / 12), 1.0, 2.0 ** (1 / 12), 1.5, 2.0)
BAD_VALUES = (0.0, -1.0, np.nan, np.inf)


def taps(K, ratio):
    """(j, a, copied) per output bin: the lower tap, its weight's complement and whether the definition copies sp[j]
    there (the held band included, with j = K-1).  They depend on (k, ratio) alone."""
    u = np.arange(K, dtype=np.float64) / np.float64(ratio)
    j = np.floor(u)
    a = u - j
    held = j >= K - 1
    j = np.where(held, K - 1, j).astype(np.int64)
    a = np.where(held, 0.0, a)
    return j, a, a == 0.0


def usable(sp):
    """per row: every value finite and > 0"""
    sp = np.asarray(sp)
    return np.all(np.isfinite(sp) & (sp > 0), axis=1) if sp.shape[0] else np.zeros(0, dtype=bool)


def shift(sp, ratio):
    """(out, status): the warped matrix and the number of rows that were copied because they are unusable"""
    sp = np.asarray(sp, dtype=np.float64)
    if not (np.isfinite(ratio) and RATIO_RANGE[0] <= ratio <= RATIO_RANGE[1]):
        raise ValueError(f'ratio {ratio!r} is outside [0.5, 2]')
    out = sp.copy()
    if ratio == 1 or sp.shape[0] == 0:
        return out, 0
    K = sp.shape[1]
    j, a, copied = taps(K, ratio)
    good = usable(sp)
    rows = sp[good]
    with np.errstate(all='ignore'):
        l = np.log(rows)
        lo, hi = l[:, j], l[:, np.minimum(j + 1, K - 1)]
        warped = np.exp(lo + a * (hi - lo))
    out[good] = np.where(copied, rows[:, j], warped)
    return out, int((~good).sum())


def envelope(rng, rows, K):
    """positive values over the whole range an envelope takes, and beyond: exp(uniform(-30, 2))"""
    return np.exp(rng.uniform(-30.0, 2.0, size=(rows, K)))


def bump(K, centre, width, floor=-9.0, height=7.0):
    """one row: a Gaussian bump in the log domain, centred at the (real) bin `centre`"""
    k = np.arange(K, dtype=np.float64)
    return np.exp(floor + height * np.exp(-0.5 * ((k - centre) / width) ** 2))[None, :]


def bump_cases():
    """(K, semitones, centre): the grid the claim about the maximum was stated on, wherever centre * rho < K - 2"""
    for K in (65, 257, 513, 1025):
        for semitones in (1, 3, 7, 12, -1, -3, -7, -12):
            for share in (0.08, 0.2, 0.35):
                centre = share * (K - 1)
                if centre * 2.0 ** (semitones / 12) < K - 2:
                    yield K, semitones, centre


def plant(sp, rng, count):
    """`count` distinct rows of sp (in place) get one unusable value each, cycling through BAD_VALUES: -> their indices"""
    rows = sorted(rng.choice(len(sp), size=count, replace=False).tolist())
    for n, r in enumerate(rows):
        sp[r, rng.randint(sp.shape[1])] = BAD_VALUES[n % len(BAD_VALUES)]
    return rows


def range_slack(sp):
    """relative slack of `min <= out <= max` per row: the interpolated logarithm lies between two rounded logarithms up
    to its own three roundings, each at most U * max|l|, and exp adds its own rounding (1 ulp allowed)"""
    with np.errstate(all='ignore'):
        big = np.abs(np.log(sp)).max(axis=1)
    return (3 * big + 2) * EPS
