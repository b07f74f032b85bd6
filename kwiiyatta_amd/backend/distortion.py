"""Objective evaluation on the device (include/kwy.h, "objective evaluation"): mel-cepstral distortion, f0 and
voicing error along an alignment, and the merge of per-utterance moments into corpus totals

    mcd[t] = (10 / ln 10) * sqrt(2 * sum_{d >= first_col} (a[ia[t], d] - b[ib[t], d]) ** 2)          dB
    cents  = 1200 * log2(fa[ia[t]] / fb[ib[t]])       over the rows where both tracks are voiced (f0 > 0)

Row t of an utterance reads row ia[t] - off_a of a and ib[t] - off_b of b (no index list: row t), so the lists of
an alignment over padded features address unpadded matrices; the kernels gather themselves.  The reference has no
counterpart: it compares features only in its tests.
Inputs follow the other shims' contract: float64, C-contiguous (the same ValueError otherwise); index lists int32."""
import math

import numpy as np

from .. import _lib
from .._lib import lib, ptr

MAX_COLS = 64


def rmse(moments):
    """root mean square of the values behind an (n, mean, M2) triple: sqrt(M2 / n + mean ** 2); nan when n == 0.
    The one place where the finishing step of the f0 error is stated"""
    n, mean, m2 = (float(v) for v in moments)
    return math.sqrt(m2 / n + mean * mean) if n > 0 else math.nan


def vuv_error(counts):
    """share of the frames on which the two tracks disagree in voicing: (VU + UV) / all; nan without frames"""
    vv, vu, uv, uu = (int(v) for v in counts)
    total = vv + vu + uv + uu
    return (vu + uv) / total if total else math.nan


def _matrix(a):
    a = _lib.as_f64(a)
    if a.ndim != 2 or not 1 <= a.shape[1] <= MAX_COLS:
        raise ValueError(f'a (frames, columns) matrix of 1 .. {MAX_COLS} columns is expected, not shape {a.shape}')
    return a


def _index(idx, what):
    if idx is None:
        return None
    idx = np.asarray(idx)
    if idx.ndim != 1 or idx.dtype != np.int32 or not idx.flags['C_CONTIGUOUS']:
        raise ValueError(f'{what} must be a C-contiguous int32 vector')
    return idx


def _rows(a_rows, b_rows, ia, ib, what):
    """the row count of an utterance: the lists' common length; without lists the two sides must agree"""
    if ia is not None and ib is not None and len(ia) != len(ib):
        raise ValueError(f'{what}: the index lists differ in length')
    if ia is not None or ib is not None:
        return len(ia if ia is not None else ib)
    if a_rows != b_rows:
        raise ValueError(f'{what}: without index lists both sides must have the same number of rows')
    return a_rows


def _addr(a):
    return None if a is None else a.ctypes.data


def _listed(v, n):
    return list(v) if isinstance(v, (list, tuple)) else [v] * n


def _raise_status(status, what):
    bad = [i for i, s in enumerate(status) if s]
    if bad:
        raise ValueError(f'{what}: {int(sum(status[i] for i in bad))} row(s) of utterance(s) {bad} were left out: a '
                         f'value is not finite (or an f0 negative)')


def mcd(a, b, idx_a=None, idx_b=None, off_a=0, off_b=0, mask=None, first_col=1, per_row=False, strict=True, ctx=None):
    """(moments, status[, per-row values]) of the mel-cepstral distortion of a against b: moments (n, mean, M2) in dB
    over the rows that count, status the number of rows left out for a coefficient that is not finite
    (a row whose index falls outside a or b is passed over: it is not a row of the measure).
    mask: a float64 vector or a column view of a matrix (its stride is kept), addressed by the UNSHIFTED idx_b[t]:
    a row counts when its entry is > 0.  a, b (and the other arguments) may be lists of utterances: one call, arrays
    with a row per utterance back ((count, 3), (count,), list of vectors).  per_row=True: also mcd[t] per row, NaN
    where the row does not count.  strict: ValueError when a status word is not zero."""
    single = not isinstance(a, (list, tuple))
    As = [_matrix(m) for m in ([a] if single else a)]
    Bs = [_matrix(m) for m in ([b] if single else b)]
    n = len(As)
    if not As:
        return (np.zeros((0, 3)), np.zeros(0, dtype=np.int32)) + (([],) if per_row else ())
    cols = As[0].shape[1]
    if len(Bs) != n or any(m.shape[1] != cols for m in As + Bs):
        raise ValueError('mcd: a and b must be as many matrices of one column count')
    if not 0 <= int(first_col) <= cols:
        raise ValueError(f'first_col {first_col!r} is outside [0, {cols}]')
    wrap = (lambda v: [v]) if single else (lambda v: _listed(v, n))
    ias, ibs = ([_index(i, 'an index list') for i in wrap(v)] for v in (idx_a, idx_b))
    offs_a, offs_b, masks = wrap(off_a), wrap(off_b), wrap(mask)
    rows, outs, jobs, held = [], [], [], []
    for k in range(n):
        r = _rows(len(As[k]), len(Bs[k]), ias[k], ibs[k], 'mcd')
        m, m_stride, m_rows = masks[k], 0, 0
        if m is not None:
            m = np.asarray(m)
            if m.ndim != 1 or m.dtype != np.float64 or m.strides[0] % 8 or m.strides[0] <= 0:
                raise ValueError('mcd: the mask must be a float64 vector (a column view of a matrix will do)')
            m_stride, m_rows = m.strides[0] // 8, len(m)
            held.append(m)
        out = np.empty(r) if per_row else None
        rows.append(r)
        outs.append(out)
        jobs.append((As[k].ctypes.data, len(As[k]), cols, Bs[k].ctypes.data, len(Bs[k]), cols, _addr(ias[k]), _addr(ibs[k]),
                     int(offs_a[k]), int(offs_b[k]), r, None, _addr(m), m_stride, m_rows, _addr(out)))
    ctx = ctx or _lib.default_context()
    moments = np.empty((n, 3))
    status = np.zeros(n, dtype=np.int32)
    _lib.check(ctx, lib.kwy_mcd(ctx.handle, _lib.job_array(_lib.McdJob, jobs), n, cols, int(first_col), ptr(moments),
                                ptr(status)))
    if strict:
        _raise_status(status, 'mcd')
    res = (moments[0], int(status[0])) if single else (moments, status)
    if per_row:
        res += (outs[0] if single else outs,)
    return res


def f0_error(f0_a, f0_b, idx_a=None, idx_b=None, off_a=0, off_b=0, strict=True, ctx=None):
    """(counts, moments, status) of f0_a against f0_b: the int64 confusion counts (VV, VU, UV, UU; voiced: f0 > 0),
    (n, mean, M2) of 1200 log2(f0_a / f0_b) cents over the VV rows, and the number of rows left out (f0 negative or not
    finite; rows whose index falls outside a track are passed over, so counts + status = the rows inside both).
    Lists of tracks: one call, (count, 4), (count, 3) and (count,) arrays back"""
    single = not isinstance(f0_a, (list, tuple))
    As = [_lib.as_f64(f) for f in ([f0_a] if single else f0_a)]
    Bs = [_lib.as_f64(f) for f in ([f0_b] if single else f0_b)]
    n = len(As)
    if not As:
        return np.zeros((0, 4), dtype=np.int64), np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
    if len(Bs) != n or any(f.ndim != 1 for f in As + Bs):
        raise ValueError('f0 error: f0_a and f0_b must be as many one-dimensional tracks')
    wrap = (lambda v: [v]) if single else (lambda v: _listed(v, n))
    ias, ibs = ([_index(i, 'an index list') for i in wrap(v)] for v in (idx_a, idx_b))
    offs_a, offs_b = wrap(off_a), wrap(off_b)
    jobs = [(As[k].ctypes.data, len(As[k]), Bs[k].ctypes.data, len(Bs[k]), _addr(ias[k]), _addr(ibs[k]), int(offs_a[k]),
             int(offs_b[k]), _rows(len(As[k]), len(Bs[k]), ias[k], ibs[k], 'f0 error'), None) for k in range(n)]
    ctx = ctx or _lib.default_context()
    counts = np.zeros((n, 4), dtype=np.int64)
    moments = np.empty((n, 3))
    status = np.zeros(n, dtype=np.int32)
    _lib.check(ctx, lib.kwy_f0_error(ctx.handle, _lib.job_array(_lib.F0ErrorJob, jobs), n, ptr(counts), ptr(moments),
                                     ptr(status)))
    if strict:
        _raise_status(status, 'f0 error')
    return (counts[0], moments[0], int(status[0])) if single else (counts, moments, status)


def merge_moments(m, ctx=None):
    """(count, 3) -> (3,), or (count, width, 3) -> (width, 3): per column of triples the (n, mean, M2) of the
    concatenation of what the rows stand for (Chan's combination, a left fold in row order; n == 0 skipped)"""
    m = _lib.as_f64(m)
    flat = m.ndim == 2
    if flat:
        m = m.reshape(len(m), 1, 3) if m.shape[1:] == (3,) else m
    if m.ndim != 3 or m.shape[2] != 3 or len(m) == 0 or not 1 <= m.shape[1] <= MAX_COLS:
        raise ValueError(f'moments must be a non-empty (count, 3) or (count, width <= {MAX_COLS}, 3) array')
    ctx = ctx or _lib.default_context()
    out = np.empty((m.shape[1], 3))
    _lib.check(ctx, lib.kwy_moments_merge(ctx.handle, ptr(m), len(m), m.shape[1], ptr(out)))
    return out[0] if flat else out


# ---- device tensors (enqueued on the context's stream, not synchronised) ---------------------------------------------
def mcd_job(a, b, idx_a=None, idx_b=None, off_a=0, off_b=0, rows=None, n_dev=None, mask=None, per_row=None):
    """one row for `mcd_batch_dev`.  a, b: (rows, cols) float64 device tensors whose rows may be strided (the
    values of a row are contiguous); idx_a / idx_b: int32
    device tensors or None; rows: the row count, or with n_dev (an int64 device word) the capacity of the lists;
    mask: a one-dimensional float64 view (its stride is kept), addressed by the unshifted idx_b; per_row: a float64
    device tensor of `rows` values to write, or None"""
    if rows is None:
        rows = (idx_a if idx_a is not None else idx_b if idx_b is not None else a).shape[0]
    return (a, a.shape[0], a.stride(0), b, b.shape[0], b.stride(0), idx_a, idx_b, int(off_a), int(off_b), int(rows), n_dev,
            mask, 0 if mask is None else mask.stride(0), 0 if mask is None else mask.shape[0], per_row)


def mcd_batch_dev(ctx, jobs, cols, moments, status=None, first_col=1):
    """jobs: rows made by `mcd_job`; moments: a (len(jobs), 3) float64 device tensor, written; status: an int32 device
    tensor with a word per job, or None"""
    _lib.check(ctx, lib.kwy_mcd_batch_dev(ctx.handle, _lib.job_array(_lib.McdJob, jobs), len(jobs), int(cols),
                                          int(first_col), moments.data_ptr(),
                                          None if status is None else status.data_ptr()))


def f0_error_job(f0_a, f0_b, idx_a=None, idx_b=None, off_a=0, off_b=0, rows=None, n_dev=None):
    """one row for `f0_error_batch_dev` (arguments as in `mcd_job`; the tracks are contiguous device tensors)"""
    if rows is None:
        rows = (idx_a if idx_a is not None else idx_b if idx_b is not None else f0_a).shape[0]
    return (f0_a, f0_a.numel(), f0_b, f0_b.numel(), idx_a, idx_b, int(off_a), int(off_b), int(rows), n_dev)


def f0_error_batch_dev(ctx, jobs, counts, moments, status=None):
    """counts: a (len(jobs), 4) int64 device tensor; moments: (len(jobs), 3) float64; status: int32 words or None"""
    _lib.check(ctx, lib.kwy_f0_error_batch_dev(ctx.handle, _lib.job_array(_lib.F0ErrorJob, jobs), len(jobs),
                                               counts.data_ptr(), moments.data_ptr(),
                                               None if status is None else status.data_ptr()))


def merge_moments_dev(ctx, moments, out):
    """moments: a contiguous (count, width, 3) device tensor; out: (width, 3) on the device, written"""
    _lib.check(ctx, lib.kwy_moments_merge_dev(ctx.handle, moments.data_ptr(), moments.shape[0], moments.shape[1],
                                              out.data_ptr()))


def check_status(status, what='evaluation'):
    """raise for the non-zero words of a status (host array / device tensor, read back here)"""
    _raise_status([int(s) for s in (status.tolist() if hasattr(status, 'tolist') else status)], what)
