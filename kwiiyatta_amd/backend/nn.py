"""All-pairs nearest-neighbour search on the device (include/kwy.h, "non-parallel training")

    idx[t]   = argmin_j |c_j|^2 - 2 <q_t, c_j>          of equal scores the lower j
    dist2[t] = sum_k (q[t, k] - c[idx[t], k]) ** 2      recomputed directly for the winner

the search of INCA (`MelCepstrumFeatureConverter.train_nonparallel`): every source frame is paired with its nearest
target frame and every target frame with its nearest source frame.  The reference trains on parallel data only and has
no counterpart.  The product runs on the f64 matrix cores with the candidates streamed through LDS; the result does not
depend on `splits`, the number of slices the candidate range is cut into (0: the library chooses).
A query without a finite score (a NaN or an infinity in its row, or in every candidate) gets idx = -1 and
dist2 = NaN and is counted in the status word.
Inputs follow the other shims' contract: float64, C-contiguous (the same ValueError otherwise)."""
import numpy as np

from .. import _lib
from .._lib import lib, ptr

MAX_COLS = 160
MAX_SPLITS = 64


def _matrix(a, what):
    a = _lib.as_f64(a)
    if a.ndim != 2 or not 1 <= a.shape[1] <= MAX_COLS:
        raise ValueError(f'{what}: a (rows, columns) matrix of 1 .. {MAX_COLS} columns is expected, not shape {a.shape}')
    return a


def slice_length(nc, splits):
    """rows of a slice when `splits` slices are forced on nc candidates: slice s is [s L, min(nc, (s + 1) L))"""
    return int(lib.kwy_nn_slice(int(nc), int(splits)))


def scratch_bytes(nq, splits=0):
    """bytes of context scratch `nearest_dev` takes for nq queries (splits = 0: the bound for whatever it chooses)"""
    return int(lib.kwy_nn_scratch_bytes(int(nq), int(splits)))


def nearest(queries, candidates, splits=0, center=True, strict=True, ctx=None):
    """(idx int32, dist2 float64) of every row of `queries` among the rows of `candidates`.
    center: the column mean of the candidates (of those rows that are finite) is subtracted from both sides first.
    Distances do not change under it, and the rounding error of the score, which grows with |q|^2 + |c|^2, is that of
    the centred rows.  dist2 is then formed here, on the host, from the rows AS GIVEN, in the kernel's order (k
    ascending, no contraction): the same definition, but the kernel's own value only with center=False (and from
    `nearest_dev`).
    strict: ValueError when a query has no finite score (`check_status`)."""
    q, c = _matrix(queries, 'queries'), _matrix(candidates, 'candidates')
    if q.shape[1] != c.shape[1]:
        raise ValueError(f'queries and candidates differ in columns: {q.shape[1]} and {c.shape[1]}')
    if len(q) and not len(c):
        raise ValueError('nearest: no candidates')
    given = q, c
    if center and len(c):
        finite = np.isfinite(c).all(axis=1)        # a row that is not finite cannot win and must not spoil the mean
        if finite.any():
            mean = c[finite].mean(axis=0)
            q, c = q - mean, c - mean
    idx = np.empty(len(q), dtype=np.int32)
    dist2 = np.empty(len(q))
    status = np.zeros(1, dtype=np.int32)
    ctx = ctx or _lib.default_context()
    _lib.check(ctx, lib.kwy_nn_search(ctx.handle, ptr(q), len(q), ptr(c), len(c), q.shape[1], int(splits), ptr(idx),
                                      ptr(dist2), ptr(status)))
    if strict:
        check_status(status, 'nearest')
    if q is not given[0]:
        # the distance is that of the rows as given: the centred ones carry the rounding of the subtraction.  Summed
        # as the kernel sums it, column after column in ascending order
        found = idx >= 0
        d = given[0][found] - given[1][idx[found]]
        total = np.zeros(len(d))
        for k in range(d.shape[1]):
            total += d[:, k] * d[:, k]
        dist2[found] = total
    return idx, dist2


def nearest_dev(ctx, Q, C, idx, dist2, status=None, splits=0):
    """Q (nq, D), C (nc, D): contiguous float64 device tensors; idx (nq) int32, dist2 (nq) float64, status one int32
    word or None: written.  Enqueued on the context's stream, not synchronised; no centring (the caller's rows as
    they are)."""
    if Q.dim() != 2 or C.dim() != 2 or Q.shape[1] != C.shape[1] or not Q.is_contiguous() or not C.is_contiguous():
        raise ValueError('nearest_dev: contiguous (rows, D) matrices of one column count are expected')
    if idx.numel() < Q.shape[0] or dist2.numel() < Q.shape[0]:
        raise ValueError('nearest_dev: idx and dist2 need an entry per query')
    _lib.check(ctx, lib.kwy_nn_search_dev(ctx.handle, Q.data_ptr(), Q.shape[0], C.data_ptr(), C.shape[0], Q.shape[1],
                                          int(splits), idx.data_ptr(), dist2.data_ptr(),
                                          None if status is None else status.data_ptr()))


def check_status(status, what='nearest-neighbour search'):
    """raise for a non-zero status word (host array / device tensor, read back here)"""
    n = int(sum(int(s) for s in (status.tolist() if hasattr(status, 'tolist') else status)))
    if n:
        raise ValueError(f'{what}: {n} quer{"y has" if n == 1 else "ies have"} no finite score '
                         f'(a value of the rows is not finite)')
