"""The mel-cepstral energy and the postfilter built on it, stated in numpy -- the yardstick of tests/test_power_cases.py
(its own claims against closed forms) and of tests/test_power_gpu.py (the kernels of kwy_mcpower.hip against it) -- and
the generators of their inputs.  include/kwy.h, "mel-cepstral energy", is the contract:

    w_k = 2 pi k / N,   w~_k = w_k + 2 atan2(alpha sin w_k, 1 - alpha cos w_k)
    L_k = sum_{m = 0 .. order} c[m] cos(m w~_k),   m ascending
    E(c) = ( exp(2 L_0) + exp(2 L_{N/2}) + 2 sum_{k = 1 .. N/2 - 1} exp(2 L_k) ) / N

    b[order] = x[order];  b[m] = x[m] - alpha b[m+1]
    if order >= 2:  b[1] = b[1] - (beta alpha) b[2];   b[m] = b[m] (1 + beta),  m = 2 .. order
    y[order] = b[order];  y[m] = b[m] + alpha b[m+1]
    y[0] = y[0] + log(E(ref) / E(y)) / 2

`energy` and `postfilter` work on (rows, order + 1) matrices, every row on its own."""
import numpy as np

U = 2.0 ** -53            # unit roundoff of float64
EPS = 2.0 ** -52

CONFIGS = ((1, 512, 0.0), (24, 1024, 0.41), (24, 2048, 0.554), (62, 4096, 0.63))      # (order, N, alpha)
ROWS = 67


def warped(N, alpha):
    """w~_k, k = 0 .. N/2"""
    w = 2.0 * np.pi * np.arange(N // 2 + 1, dtype=np.float64) / float(N)
    return w + 2.0 * np.arctan2(alpha * np.sin(w), 1.0 - alpha * np.cos(w))


def cos_table(order, N, alpha):
    """(order + 1, N/2 + 1): cos(m w~_k)"""
    return np.cos(np.arange(order + 1, dtype=np.float64)[:, None] * warped(N, alpha)[None, :])


def energy(c, alpha, N, table=None):
    """E of every row of c (rows, order + 1)"""
    c = np.asarray(c, dtype=np.float64)
    rows, cols = c.shape
    tab = cos_table(cols - 1, N, alpha) if table is None else table
    H = N // 2
    L = np.zeros((rows, H + 1))
    with np.errstate(all='ignore'):
        for m in range(cols):
            L = L + c[:, m:m + 1] * tab[m][None, :]
        p = np.exp(2.0 * L)
        return (p[:, 0] + p[:, H] + 2.0 * p[:, 1:H].sum(axis=1)) / float(N)


def emphasis(x, alpha, beta):
    """y before its c0 is corrected; x itself at beta == 0 (no b is formed)"""
    x = np.asarray(x, dtype=np.float64)
    if beta == 0:
        return x.copy(), np.abs(x).max(axis=1, initial=0.0)
    order = x.shape[1] - 1
    with np.errstate(all='ignore'):
        b = x.copy()
        for m in range(order - 1, -1, -1):
            b[:, m] = x[:, m] - alpha * b[:, m + 1]
        bmax = np.abs(b).max(axis=1, initial=0.0)
        if order >= 2:
            b[:, 1] = b[:, 1] - (beta * alpha) * b[:, 2]
            b[:, 2:] = b[:, 2:] * (1.0 + beta)
        y = b.copy()
        for m in range(order - 1, -1, -1):
            y[:, m] = b[:, m] + alpha * b[:, m + 1]
    return y, bmax


def postfilter(x, alpha, N, beta=0.0, ref=None, base=None):
    """(out, status): status counts the rows left as they are (copied from base, or from x without one) because E(ref)
    or E(y) is not finite or not > 0 or the correction is not finite.  beta == 0 without ref copies every row, uncounted"""
    x = np.asarray(x, dtype=np.float64)
    if (beta == 0 and ref is None) or len(x) == 0:
        return (x if base is None else np.asarray(base, dtype=np.float64)).copy(), 0
    return compose(x, *filtered(x, alpha, N, beta, ref), base)


def filtered(x, alpha, N, beta, ref=None, table=None):
    """(y, ok): the filtered rows with their corrected c0, and which of them are usable"""
    x = np.asarray(x, dtype=np.float64)
    tab = cos_table(x.shape[1] - 1, N, alpha) if table is None else table
    y, _ = emphasis(x, alpha, beta)
    e_ref = energy(x if ref is None else ref, alpha, N, tab)
    e_y = energy(y, alpha, N, tab)
    with np.errstate(all='ignore'):
        corr = np.log(e_ref / e_y) / 2.0
        ok = np.isfinite(e_ref) & (e_ref > 0) & np.isfinite(e_y) & (e_y > 0) & np.isfinite(corr)
        y[:, 0] = y[:, 0] + corr
    return y, ok


def compose(x, y, ok, base=None):
    """(out, status) of `filtered`'s result: out = y, or base + (y - x); the unusable rows copied and counted"""
    keep = x if base is None else np.asarray(base, dtype=np.float64)
    with np.errstate(all='ignore'):
        out = y if base is None else keep + (y - x)
    return np.where(ok[:, None], out, keep), int((~ok).sum())


def kernel_ceiling(x, ref, order):
    """the derived ceiling of the kernel's deviation from this statement, per row: 32 eps (order + 2)(1 + sum|x| +
    sum|ref|) -- the rounding of m w~ before the cosine, carried through the sums"""
    x = np.asarray(x, dtype=np.float64)
    r = np.zeros_like(x) if ref is None else np.asarray(ref, dtype=np.float64)
    with np.errstate(all='ignore'):
        return 32 * EPS * (order + 2) * (1.0 + np.abs(x).sum(axis=1) + np.abs(r).sum(axis=1))


# ---- inputs ------------------------------------------------------------------------------------------------
def rows_like_speech(rng, rows, order, c0=-8.0):
    """mel-cepstra with the decay of speech: c0 around `c0`, c1 up to about 2, the rest falling off with the index"""
    scale = np.concatenate(([1.0], 1.5 / (1.0 + np.arange(order)) ** 0.9))
    x = rng.standard_normal((rows, order + 1)) * scale
    x[:, 0] += c0
    return np.ascontiguousarray(x)


BAD_KINDS = ('nan', 'overflow', 'ref_inf')


def spoil(x, ref, kind, row):
    """one bad row of the given kind put into copies of (x, ref)"""
    x, ref = x.copy(), ref.copy()
    if kind == 'nan':
        x[row, min(3, x.shape[1] - 1)] = np.nan
    elif kind == 'overflow':
        x[row, 0] = 400.0
    else:
        ref[row, 1] = np.inf
    return x, ref
