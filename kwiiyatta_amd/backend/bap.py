"""Band-aperiodicity conversion on the device (include/kwy.h, "aperiodicity conversion"; kwy_bap.hip): the aperiodic
component as one more stream of the joint-density GMM conversion (Ohtani et al. 2006; sprocket's `codeap` mixture).

    track(ap, fs)          ap (T, K) -> S (T, B + 1): column 0 the voicing flag of the band codec's decoder, columns
                           1..B the coded bands in dB, unvoiced frames holding the nearest voiced frame's row
    rows(...)              the joint rows [gx, dgx, ddgx | gy, dgy, ddgy] of the cells of an aligned pair that are voiced
                           on both sides, appended behind a cursor
    apply(src, conv, ap)   the converted bands, clamped to [-60, -1e-12] dB, decoded over the voiced rows of ap
    error(a, b, ...)       (n, mean, M2) of sqrt(sum_b (a - b)^2 / B) dB over the cells voiced on both sides

B = bands(fs) must be at least 1 (fs >= 12 kHz): `check_rate` raises ValueError otherwise, and so does the library.
The reference has no counterpart: it renders a converted voice with the source's aperiodicity.
Inputs follow the other shims' contract: float64, C-contiguous (the same ValueError otherwise); index lists int32."""
import numpy as np

from .. import _lib
from .._lib import lib, ptr

FLOOR, CEILING = -60.0, -1e-12          # what a converted band is clamped to before it is decoded (dB)
PASS_FRAMES = 256                       # frames per pass of the track kernel (BAP_PASS, kwy_bap.hip)


def bands(fs):
    return int(lib.kwy_aperiodicity_bands(int(fs)))


def check_rate(fs):
    """the band count B of the sampling rate; ValueError for a rate without a band (below 12 kHz)"""
    B = bands(fs)
    if B < 1:
        raise ValueError(f'aperiodicity conversion needs a sampling rate of 12 kHz or more: {fs} Hz has no '
                         f'aperiodicity band')
    return B


def _matrix(a, what):
    a = _lib.as_f64(a)
    if a.ndim != 2:
        raise ValueError(f'{what} is expected to be a (frames, columns) matrix, not of shape {a.shape}')
    return a


def _tracks(items, B, what):
    out = [_matrix(m, what) for m in items]
    if any(m.shape[1] != B + 1 for m in out):
        raise ValueError(f'{what} is expected to have {B + 1} columns (voicing flag and {B} bands)')
    return out


def _index(idx, what):
    idx = np.asarray(idx)
    if idx.ndim != 1 or idx.dtype != np.int32 or not idx.flags['C_CONTIGUOUS']:
        raise ValueError(f'{what} must be a C-contiguous int32 vector')
    return idx


def _addr(a):
    return None if a is None else a.ctypes.data


def _fft_size(aps):
    K = aps[0].shape[1]
    if K < 3 or any(m.shape[1] != K for m in aps):
        raise ValueError('the aperiodicity matrices must share one bin count of at least 3')
    return 2 * (K - 1)


def track(ap, fs, ctx=None):
    """the band track(s) (T, B + 1) of one aperiodicity matrix (T, K) or of a list of them (one call)"""
    B = check_rate(fs)
    single = not isinstance(ap, (list, tuple))
    aps = [_matrix(m, 'aperiodicity') for m in ([ap] if single else ap)]
    if not aps:
        return []
    fft_size = _fft_size(aps)
    outs = [np.empty((len(m), B + 1)) for m in aps]
    live = [(m, o) for m, o in zip(aps, outs) if len(m)]
    if live:
        ctx = ctx or _lib.default_context()
        jobs = [(m.ctypes.data, len(m), o.ctypes.data) for m, o in live]
        _lib.check(ctx, lib.kwy_bap_track(ctx.handle, _lib.job_array(_lib.BapTrackJob, jobs), len(jobs), int(fs), fft_size))
    return outs[0] if single else outs


def rows(track_x, track_y, idx_x, idx_y, joint=None, cursor=0, ctx=None):
    """(joint, cursor, n_rows) of aligned pairs: track_x / track_y / idx_x / idx_y one pair or lists of them.  joint: a
    (capacity, 6 B) matrix that is appended to behind `cursor` (default: one that holds every cell); n_rows per pair
    the rows kept, or -1 - rows for a pair that did not fit (dropped whole)"""
    single = not isinstance(track_x, (list, tuple))
    xs, ys = ([m] if single else list(m) for m in (track_x, track_y))
    ixs, iys = ([m] if single else list(m) for m in (idx_x, idx_y))
    if not xs or not len({len(xs), len(ys), len(ixs), len(iys)}) == 1:
        raise ValueError('band rows: as many tracks and index lists are expected on both sides (at least one pair)')
    B = np.shape(xs[0])[1] - 1
    xs, ys = _tracks(xs, B, 'a band track'), _tracks(ys, B, 'a band track')
    ixs, iys = ([_index(i, 'an index list') for i in v] for v in (ixs, iys))
    if B < 1:
        raise ValueError('band rows: the tracks have no band')
    for x, y, ix, iy in zip(xs, ys, ixs, iys):
        if len(ix) != len(iy):
            raise ValueError('band rows: the index lists of a pair differ in length')
        if len(ix) and (len(x) == 0 or len(y) == 0):
            raise ValueError('band rows: cells into an empty track')
    if joint is None:
        joint = np.zeros((sum(len(i) for i in ixs), 6 * B))
    joint = _matrix(joint, 'the joint matrix')
    if joint.shape[1] != 6 * B:
        raise ValueError(f'the joint matrix is expected to have {6 * B} columns')
    cur = np.array([int(cursor)], dtype=np.int64)
    n_rows = np.zeros(len(xs), dtype=np.int64)
    jobs = [(_addr(x), len(x), _addr(y), len(y), _addr(ix), _addr(iy), None, len(ix), n_rows[k:].ctypes.data)
            for k, (x, y, ix, iy) in enumerate(zip(xs, ys, ixs, iys))]
    ctx = ctx or _lib.default_context()
    _lib.check(ctx, lib.kwy_bap_rows(ctx.handle, _lib.job_array(_lib.BapRowsJob, jobs), len(jobs), B, ptr(joint),
                                     len(joint), ptr(cur)))
    return joint, int(cur[0]), (int(n_rows[0]) if single else n_rows)


def apply(track_src, track_conv, ap, fs, ctx=None):
    """ap (T, K) -- or a list of them -- rewritten IN PLACE: the rows that are voiced in track_src become the decode of
    track_conv's bands; returns ap"""
    B = check_rate(fs)
    single = not isinstance(ap, (list, tuple))
    aps = [_matrix(m, 'aperiodicity') for m in ([ap] if single else ap)]
    srcs = _tracks([track_src] if single else track_src, B, 'a band track')
    convs = _tracks([track_conv] if single else track_conv, B, 'a band track')
    if not aps:
        return ap
    if not len(aps) == len(srcs) == len(convs) or any(not len(a) == len(s) == len(c) for a, s, c in zip(aps, srcs, convs)):
        raise ValueError('band apply: the tracks and the aperiodicity must agree in number and in frames')
    if any(not m.flags['WRITEABLE'] for m in aps):
        raise ValueError('band apply: the aperiodicity is rewritten in place and must be writeable')
    fft_size = _fft_size(aps)
    jobs = [(s.ctypes.data, c.ctypes.data, len(a), a.ctypes.data) for a, s, c in zip(aps, srcs, convs) if len(a)]
    if jobs:
        ctx = ctx or _lib.default_context()
        _lib.check(ctx, lib.kwy_bap_apply(ctx.handle, _lib.job_array(_lib.BapApplyJob, jobs), len(jobs), int(fs), fft_size))
    return ap


def error(a, b, idx_a=None, idx_b=None, off_a=0, off_b=0, per_row=False, ctx=None):
    """moments (n, mean, M2) [, per-cell values] of the band error of track a against track b in dB, over the cells
    voiced on both sides; cell t reads row idx_a[t] - off_a of a and idx_b[t] - off_b of b (no list: row t), a cell
    outside either track is passed over.  Lists of tracks: one call, a (count, 3) array back"""
    single = not isinstance(a, (list, tuple))
    As, Bs = ([m] if single else list(m) for m in (a, b))
    if not As:
        return (np.zeros((0, 3)),) + (([],) if per_row else ())
    B = np.shape(As[0])[1] - 1
    As, Bs = _tracks(As, B, 'a band track'), _tracks(Bs, B, 'a band track')
    n = len(As)
    if B < 1 or len(Bs) != n:
        raise ValueError('band error: as many tracks of at least one band are expected on both sides')
    wrap = (lambda v: [v]) if single else (lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n)
    ias, ibs = ([None if i is None else _index(i, 'an index list') for i in wrap(v)] for v in (idx_a, idx_b))
    offs_a, offs_b = wrap(off_a), wrap(off_b)
    jobs, outs = [], []
    for k in range(n):
        ia, ib = ias[k], ibs[k]
        if ia is not None and ib is not None and len(ia) != len(ib):
            raise ValueError('band error: the index lists differ in length')
        if ia is None and ib is None and len(As[k]) != len(Bs[k]):
            raise ValueError('band error: without index lists both sides must have the same number of rows')
        r = len(ia if ia is not None else ib if ib is not None else As[k])
        out = np.empty(r) if per_row else None
        outs.append(out)
        jobs.append((As[k].ctypes.data, len(As[k]), Bs[k].ctypes.data, len(Bs[k]), _addr(ia), _addr(ib), int(offs_a[k]),
                     int(offs_b[k]), r, None, _addr(out)))
    ctx = ctx or _lib.default_context()
    moments = np.empty((n, 3))
    _lib.check(ctx, lib.kwy_bap_error(ctx.handle, _lib.job_array(_lib.BapErrorJob, jobs), n, B, ptr(moments)))
    res = (moments[0] if single else moments,)
    if per_row:
        res += (outs[0] if single else outs,)
    return res if per_row else res[0]


def clamp(bands_db):
    """what `apply` decodes of a converted band value"""
    return np.clip(bands_db, FLOOR, CEILING)


# ---- device tensors (enqueued on the context's stream, not synchronised) ---------------------------------------------
def track_batch_dev(ctx, jobs, fs, fft_size):
    """jobs: (ap, track) device tensors per utterance, (T, K) and (T, B + 1) float64"""
    rows_ = [(ap, ap.shape[0], tr) for ap, tr in jobs]
    _lib.check(ctx, lib.kwy_bap_track_batch_dev(ctx.handle, _lib.job_array(_lib.BapTrackJob, rows_), len(rows_), int(fs),
                                                int(fft_size)))


def rows_job(track_x, track_y, idx_x, idx_y, n_rows, n_dev=None, capacity=None):
    """one row for `rows_batch_dev`: the tracks and int32 index lists of a pair (device tensors), n_rows an int64 device
    word that is written; n_dev: an int64 device word with the cell count (default: all `capacity` cells, the lists'
    length)"""
    return (track_x, track_x.shape[0], track_y, track_y.shape[0], idx_x, idx_y, n_dev,
            int(idx_x.shape[0] if capacity is None else capacity), n_rows)


def rows_batch_dev(ctx, jobs, bands, joint, cursor):
    """jobs: rows made by `rows_job`; joint: a (capacity, 6 B) float64 device tensor appended to behind cursor[0] (an
    int64 device word, advanced)"""
    _lib.check(ctx, lib.kwy_bap_rows_batch_dev(ctx.handle, _lib.job_array(_lib.BapRowsJob, jobs), len(jobs), int(bands),
                                               joint.data_ptr(), joint.shape[0], cursor.data_ptr()))


def apply_batch_dev(ctx, jobs, fs, fft_size):
    """jobs: (track_src, track_conv, ap) device tensors per utterance; ap (T, K) is rewritten in place"""
    rows_ = [(s, c, ap.shape[0], ap) for s, c, ap in jobs]
    _lib.check(ctx, lib.kwy_bap_apply_batch_dev(ctx.handle, _lib.job_array(_lib.BapApplyJob, rows_), len(rows_), int(fs),
                                                int(fft_size)))


def error_job(a, b, idx_a=None, idx_b=None, off_a=0, off_b=0, rows=None, n_dev=None, per_row=None):
    """one row for `error_batch_dev` (arguments as in distortion.mcd_job; the tracks are contiguous device tensors)"""
    if rows is None:
        rows = (idx_a if idx_a is not None else idx_b if idx_b is not None else a).shape[0]
    return (a, a.shape[0], b, b.shape[0], idx_a, idx_b, int(off_a), int(off_b), int(rows), n_dev, per_row)


def error_batch_dev(ctx, jobs, bands, moments):
    """jobs: rows made by `error_job`; moments: a (len(jobs), 3) float64 device tensor, written"""
    _lib.check(ctx, lib.kwy_bap_error_batch_dev(ctx.handle, _lib.job_array(_lib.BapErrorJob, jobs), len(jobs), int(bands),
                                                moments.data_ptr()))
