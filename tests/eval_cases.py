"""The objective evaluation measures stated in numpy -- the yardstick of tests/test_eval_cases.py (its own claims)
and of tests/test_eval_gpu.py (the kernels of kwy_eval.hip against it) -- and the generators of their inputs.

    mcd[t] = (10 / ln 10) * sqrt(2 * sum_{d = first_col .. cols-1} (a[ia[t], d] - b[ib[t], d]) ** 2)       dB
    cents  = 1200 * log2(fa[ia[t]] / fb[ib[t]])       over the rows where both tracks are voiced (f0 > 0)

Row t reads row ia[t] - off_a of a and row ib[t] - off_b of b (no list: row t); the mask is addressed by the
unshifted ib[t].  Four operations: `mcd_rows` (per-row values and the status word), `moments` ((n, mean, M2) in two
passes), `f0_error` (confusion counts, the moments of the cents, the status word) and `merge` (Chan's combination,
a left fold)."""
import numpy as np

U = 2.0 ** -53            # unit roundoff of float64
DB = 10.0 / np.log(10.0)

LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 1000, 2049, 4097, 5000)
COLS = (1, 25, 41, 64)


def _rows(n_a, n_b, ia, ib):
    if ia is None and ib is None:
        assert n_a == n_b
        return n_a
    return len(ia if ia is not None else ib)


def mcd_rows(a, b, ia=None, ib=None, off_a=0, off_b=0, mask=None, first_col=1):
    """(values, status): values[t] the distortion of row t, NaN where the row does not count -- an index points outside
    a, b or the mask, its mask entry is not > 0, or one of the measured coefficients is not finite; status counts the
    rows of the last kind (a row whose mask is clear is not examined)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = _rows(len(a), len(b), ia, ib)
    out = np.full(n, np.nan)
    status = 0
    for t in range(n):
        ja = int(ia[t]) if ia is not None else t
        jb = int(ib[t]) if ib is not None else t
        ra, rb = ja - off_a, jb - off_b
        if not (0 <= ra < len(a) and 0 <= rb < len(b)) or (mask is not None and not 0 <= jb < len(mask)):
            continue
        if mask is not None and not mask[jb] > 0:
            continue
        x, y = a[ra, first_col:], b[rb, first_col:]
        if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
            status += 1
            continue
        d = x - y
        out[t] = DB * np.sqrt(2.0 * (d * d).sum())
    return out, status


def moments(values):
    """(n, mean, M2) over the values that are not NaN: M2 = the sum of squared deviations from that mean"""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    if len(v) == 0:
        return np.zeros(3)
    mean = v.sum() / len(v)
    dev = v - mean
    return np.array([len(v), mean, (dev * dev).sum()])


def cents(fa, fb):
    return 1200.0 * np.log2(fa / fb)


def f0_error(fa, fb, ia=None, ib=None, off_a=0, off_b=0):
    """(counts VV VU UV UU as int64, (n, mean, M2) of the cents over the VV rows, status, the cents themselves).
    status: rows left out of everything because an f0 is negative or not finite; a row whose index lies outside its
    track is passed over"""
    fa, fb = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
    n = _rows(len(fa), len(fb), ia, ib)
    counts = np.zeros(4, dtype=np.int64)
    status, vals = 0, []
    for t in range(n):
        ra = (int(ia[t]) if ia is not None else t) - off_a
        rb = (int(ib[t]) if ib is not None else t) - off_b
        if not (0 <= ra < len(fa) and 0 <= rb < len(fb)):
            continue
        x, y = fa[ra], fb[rb]
        if not (np.isfinite(x) and np.isfinite(y) and x >= 0 and y >= 0):
            status += 1
            continue
        counts[(0 if x > 0 else 2) + (0 if y > 0 else 1)] += 1
        if x > 0 and y > 0:
            vals.append(cents(x, y))
    return counts, moments(vals), status, np.array(vals)


def rmse(m):
    """sqrt(M2 / n + mean ** 2): the root mean square of the values behind a triple"""
    return np.sqrt(m[2] / m[0] + m[1] * m[1]) if m[0] > 0 else np.nan


def merge(ms):
    """Chan et al.'s pairwise combination, a left fold over the triples in order, skipping n == 0"""
    n = mean = m2 = 0.0
    for nb, mb, m2b in np.asarray(ms, dtype=np.float64).reshape(-1, 3):
        if nb == 0:
            continue
        if n == 0:
            n, mean, m2 = nb, mb, m2b
            continue
        nn, delta = n + nb, mb - mean
        mean = mean + delta * (nb / nn)
        m2 = (m2 + m2b) + delta * delta * (n * nb / nn)
        n = nn
    return np.array([n, mean, m2])


# ---- bounds (reasoned from the number format, not measured) -------------------------------------------------------
def row_bound(values, k):
    """|error| of a per-row distortion over k coefficients.  The differences and their squares are single correctly
    rounded operations on the same inputs, hence the same bits on both sides.  A sum of k non-negative terms in any
    order is within (k - 1) U of the exact sum, so two orders differ by 2 (k - 1) U of it; the doubling is exact; the
    square root halves that and adds its own rounding on either side (2 U); the product with 10 / ln 10 adds U on
    either side and at most U for a constant that is one unit off: relative (k - 1) + 2 + 3 <= (k + 4) U."""
    return (k + 4) * U * np.abs(values)


def moments_bounds(values, eps):
    """(|mean error|, |M2 error|) of the two-pass moments of n values known to within eps each, for any summation
    order: the mean is a sum of n terms (4 n U of max|v| covers either side's sum and quotient) plus eps; M2 is a sum
    of n squares (4 n U relative) of deviations that are off by e = eps + the mean's error + a rounding of the
    deviation, which moves sum d^2 by at most 2 sqrt(n M2) e + n e^2 (Cauchy-Schwarz)."""
    v = np.asarray(values, dtype=np.float64)
    n = len(v)
    if n == 0:
        return 0.0, 0.0
    top = np.abs(v).max()
    mean_bound = 4 * n * U * top + eps
    m2 = ((v - v.mean()) ** 2).sum()
    e = eps + mean_bound + 2 * U * top
    return mean_bound, 4 * n * U * m2 + 2 * np.sqrt(n * m2) * e + n * e * e


def cents_bound(values):
    """|error| of one cents value: the quotient is one correctly rounded operation (the same bits on both sides);
    log2 is within one unit in the last place of the true value in either library (2 U relative each, 4 U between
    them), the product with 1200 adds U on either side: 6 U relative, stated as 8 U"""
    v = np.asarray(values, dtype=np.float64)
    return 8 * U * (np.abs(v).max() if len(v) else 0.0)


def merge_bound(parts):
    """(|mean error|, |M2 error|) of merging the two-pass triples of `parts` (a list of value vectors) against the
    two-pass moments of their concatenation of N values.  Chan's combination is exact in real numbers, so only
    roundings count.  A part's mean is within e = 4 n_i U max|v| (moments_bounds); a fold step forms a convex
    combination of two means, which passes their errors on without growth and adds at most 4 U max|v| of its own;
    the other side's mean carries 4 N U max|v|.  The parts' M2 are within 4 n_i U of themselves and sum to at most the
    total M2; a step's delta is off by at most 2 e + 2 U max|v|, which moves delta^2 n nb / nn by at most
    spread * that * N (n nb / nn <= N / 4, delta <= spread, twice for the square); its roundings are 6 U of terms
    bounded by M2 + N spread^2; the other side's M2 carries 4 N U M2."""
    allv = np.concatenate([np.asarray(p, dtype=np.float64) for p in parts] + [np.zeros(0)])
    N, steps = len(allv), len(parts)
    if N == 0:
        return 0.0, 0.0
    top, spread = np.abs(allv).max(), allv.max() - allv.min()
    m2 = ((allv - allv.mean()) ** 2).sum()
    longest = max(len(p) for p in parts)
    e = 4 * longest * U * top
    mean_bound = e + 4 * steps * U * top + 4 * N * U * top
    m2_bound = 4 * longest * U * m2 + steps * (spread * (2 * e + 2 * U * top) * N + 6 * U * (m2 + N * spread * spread)) \
        + 4 * N * U * m2
    return mean_bound, m2_bound


# ---- generators ---------------------------------------------------------------------------------------------------
def matrices(rng, rows_a, rows_b, cols):
    """two float64 matrices in the range of mel-cepstra: c0 about -5 +- 3, the others shrinking with the index"""
    scale = np.concatenate(([3.0], 1.0 / (1.0 + np.arange(1, cols)) ** 0.7))
    a = rng.standard_normal((rows_a, cols)) * scale
    b = rng.standard_normal((rows_b, cols)) * scale
    a[:, 0] -= 5.0
    b[:, 0] -= 5.0
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def index_lists(rng, n, rows_a, rows_b, off_a=0, off_b=0):
    """int32 lists as an alignment leaves them, made harder: mostly rising with repeats, then some entries swapped so
    that they are not monotone either.  Values are within [off, off + rows)"""
    def one(rows, off):
        if rows == 0 or n == 0:
            return np.zeros(n, dtype=np.int32) + off
        idx = np.sort(rng.randint(0, rows, size=n))
        swaps = rng.randint(0, n, size=(max(1, n // 8), 2))
        for i, j in swaps:
            idx[i], idx[j] = idx[j], idx[i]
        return (idx + off).astype(np.int32)
    return one(rows_a, off_a), one(rows_b, off_b)


def mask_vector(rng, rows, kind):
    """kind: 'set' (all 9.4, the DTW feature's power weight), 'clear' (all 0) or 'mixed'"""
    if kind == 'set':
        return np.full(rows, 9.4)
    if kind == 'clear':
        return np.zeros(rows)
    return np.where(rng.uniform(size=rows) < 0.6, 9.4, 0.0)


def f0_tracks(rng, rows_a, rows_b):
    """two f0 tracks: voiced stretches of 80 .. 400 Hz between unvoiced ones (0)"""
    def one(rows):
        f = np.exp(rng.uniform(np.log(80.0), np.log(400.0), size=rows))
        voiced = np.repeat(rng.uniform(size=rows // 16 + 1) < 0.65, 16)[:rows]
        return np.ascontiguousarray(np.where(voiced, f, 0.0))
    return one(rows_a), one(rows_b)
