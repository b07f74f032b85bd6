"""numpy reference of the nearest-neighbour search (include/kwy.h, "non-parallel training") and the inputs its tests
share.  Everything is formed in np.longdouble (64-bit mantissa on x86: products of doubles are exact in it, sums of
D <= 160 of them good to 2^-60 relative) and ties go to the lowest index."""
import numpy as np

LD = np.longdouble
CHUNK = 512          # queries per block of the all-pairs matrices


def scores(Q, C):
    """s(t, j) = |c_j|^2 - 2 <q_t, c_j> in longdouble, (nq, nc)"""
    Q, C = np.asarray(Q, dtype=LD), np.asarray(C, dtype=LD)
    return (C * C).sum(axis=1)[None, :] - 2 * (Q @ C.T)


def distances(Q, C):
    """|q_t - c_j|^2 formed directly in longdouble, (nq, nc)"""
    Q, C = np.asarray(Q, dtype=LD), np.asarray(C, dtype=LD)
    out = np.empty((len(Q), len(C)), dtype=LD)
    rows = max(1, (1 << 22) // max(1, C.size))        # blocks of at most 64 MB
    for t0 in range(0, len(Q), rows):
        d = Q[t0:t0 + rows, None, :] - C[None, :, :]
        out[t0:t0 + rows] = (d * d).sum(axis=2)
    return out


def nearest(Q, C):
    """(idx int32, dist2 longdouble): the lowest index of the least score, and that pair's direct distance.  A query
    without a finite score gets -1 and NaN, as the library has it; a score that is not finite never wins."""
    Q, C = np.asarray(Q, dtype=np.float64), np.asarray(C, dtype=np.float64)
    idx = np.empty(len(Q), dtype=np.int32)
    dist2 = np.empty(len(Q), dtype=LD)
    for t0 in range(0, len(Q), CHUNK):
        with np.errstate(invalid='ignore', over='ignore'):
            s = scores(Q[t0:t0 + CHUNK], C)
        s = np.where(np.isfinite(s), s, np.inf)
        j = np.argmin(s, axis=1)                      # the first of equal minima
        none = ~np.isfinite(s[np.arange(len(j)), j])
        d = np.asarray(Q[t0:t0 + CHUNK], dtype=LD) - np.asarray(C[j], dtype=LD)
        idx[t0:t0 + CHUNK] = np.where(none, -1, j)
        dist2[t0:t0 + CHUNK] = np.where(none, np.nan, (d * d).sum(axis=1))
    return idx, dist2


def integer_rows(seed, n, D, low=-8, high=8):
    """rows of integers in [low, high]: every product and every sum of the search is exact in float64"""
    return np.random.RandomState(seed).randint(low, high + 1, size=(n, D)).astype(np.float64)


def normal_rows(seed, n, D, offset=0.0):
    return np.random.RandomState(seed).standard_normal((n, D)) + offset


def slice_length(nc, splits):
    """the library's slice of the candidate range (kwy_nn_slice): ceil(nc / splits) up to a multiple of 64"""
    per = -(-nc // splits)
    return -(-per // 64) * 64
