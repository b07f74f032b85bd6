"""The global-variance postfilter stated in numpy -- the yardstick of tests/test_gv_cases.py (its own claims) and of
tests/test_gv_gpu.py (the kernels of kwy_gv.hip against it) -- and the generators of their inputs.

    m_d = mean(x[:, d]),  v_d = var(x[:, d]) (ddof 0),  r_d = sqrt(gv_d / v_d)
    y[t, d] = base[t, d] + s * (r_d - 1) * (x[t, d] - m_d)         for d >= first_col, other columns copied

Three operations: `column_moments` (n, mean, M2 per column, two passes), `gv_statistic` (the mean over utterances of
M2 / n, a left fold) and `postfilter` (returns the matrix and the status word)."""
import numpy as np

U = 2.0 ** -53            # unit roundoff of float64

LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 1000, 2049, 4097, 5000)
COLS = (1, 25, 41, 64)


def column_moments(x):
    """(cols, 3): n, mean and M2 = sum of squared deviations from that mean, per column.  A column that repeats one
    value has that value as its mean (T copies of it need not add up to T times it), hence M2 == 0 exactly."""
    x = np.asarray(x, dtype=np.float64)
    rows, cols = x.shape
    out = np.zeros((cols, 3))
    for d in range(cols):
        col = x[:, d]
        if rows == 0:
            continue
        mean = col[0] if np.all(col == col[0]) else col.sum() / rows
        dev = col - mean
        out[d] = rows, mean, (dev * dev).sum()
    return out


def gv_statistic(moments):
    """moments: (count, cols, 3).  Per column the mean over the matrices with n > 0 of M2 / n, a left fold in order"""
    moments = np.asarray(moments, dtype=np.float64)
    cols = moments.shape[1]
    total, used = np.zeros(cols), 0
    for m in moments:
        if m[0, 0] > 0:
            total = total + m[:, 2] / m[:, 0]
            used += 1
    if used == 0:
        raise ValueError('no utterance has frames')
    return total / used


def ratios(x, gv, first_col=1):
    """r_d = sqrt(gv_d / v_d) for d >= first_col (as an array over those d)"""
    m = column_moments(x)[first_col:]
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.sqrt(np.asarray(gv, dtype=np.float64)[first_col:] / (m[:, 2] / m[:, 0]))


def postfilter(x, gv, s=1.0, base=None, first_col=1):
    """(y, status): status counts the columns >= first_col left as they are because v_d is not finite or gv_d is not
    finite or <= 0; columns with v_d == 0 or s * (r_d - 1) == 0 are left as they are without a count"""
    x = np.asarray(x, dtype=np.float64)
    base = x if base is None else np.asarray(base, dtype=np.float64)
    y = base.copy()
    status = 0
    m = column_moments(x)
    for d in range(first_col, x.shape[1]):
        n, mean, m2 = m[d]
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            v = m2 / n if n > 0 else 0.0
        if not np.isfinite(v) or not (np.isfinite(gv[d]) and gv[d] > 0):
            status += 1
            continue
        if v == 0:
            continue
        k = s * (np.sqrt(gv[d] / v) - 1.0)
        if k == 0:
            continue
        y[:, d] = base[:, d] + k * (x[:, d] - mean)
    return y, status


def textbook(x, gv, s=1.0, first_col=1):
    """the usual way to write the plain filter: s (r (x - m) + m) + (1 - s) x"""
    x = np.asarray(x, dtype=np.float64)
    y = x.copy()
    m = column_moments(x)
    for d in range(first_col, x.shape[1]):
        n, mean, m2 = m[d]
        if n == 0 or m2 == 0:
            continue
        r = np.sqrt(gv[d] / (m2 / n))
        y[:, d] = s * (r * (x[:, d] - mean) + mean) + (1 - s) * x[:, d]
    return y


# ---- bounds (reasoned from the number format, not measured) -------------------------------------------------------
def variance_claim_bound(x, d):
    """at s = 1: |var(y[:, d]) / gv_d - 1| <= 2^-53 (16 T + 32 max|x_d| / sigma_d) -- the rounding of y (relative to
    its offset) and of sums of T terms"""
    col = x[:, d]
    return U * (16 * len(col) + 32 * np.abs(col).max() / col.std())


def textbook_bound(x, r, d):
    return 8 * U * max(1.0, r) * np.abs(x[:, d]).max()


def moments_bounds(x, d):
    """(bound of |mean error|, relative bound of the M2 error): the worst case of any summation order over T terms"""
    T = len(x)
    return 4 * T * U * np.abs(x[:, d]).max(), 4 * T * U


def apply_bound(x, r, d):
    """|y error| of the kernel's filter: the moment bounds carried through r_d and m_d plus the elementwise roundings"""
    return (8 * len(x) + 16) * U * max(1.0, r) * np.abs(x[:, d]).max()


# ---- generators ---------------------------------------------------------------------------------------------------
def matrix(rng, rows, cols, max_offset=500.0):
    """(rows, cols) float64, C-contiguous: per column a scale within 1e-3 .. 1e3 and an offset of up to `max_offset`
    standard deviations.  The deviations are standardised per column, so max|x_d| / sigma_d <= max_offset + sqrt(rows)
    <= 1e3 and the error of the mean does not show in M2."""
    z = rng.standard_normal((rows, cols))
    if rows >= 2:
        z = z - z.mean(axis=0)
        z = z / z.std(axis=0)
    else:
        z = np.zeros((rows, cols))
    scale = 10.0 ** rng.uniform(-3, 3, size=cols)
    offset = rng.uniform(-max_offset, max_offset, size=cols)
    return np.ascontiguousarray((z + offset) * scale)


def gv_for_ratios(x, r, first_col=1):
    """the gv vector that makes the ratios of x's columns >= first_col the given r (entries below first_col: 1)"""
    m = column_moments(x)
    gv = np.ones(x.shape[1])
    v = m[first_col:, 2] / np.maximum(m[first_col:, 0], 1)
    gv[first_col:] = np.where(v > 0, np.asarray(r) ** 2 * v, 1.0)
    return gv
