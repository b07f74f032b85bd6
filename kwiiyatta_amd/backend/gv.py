"""Global-variance postfilter on the device (include/kwy.h, "global variance"): the column moments of mel-cepstrum
matrices, the target speaker's statistic gv_d (the mean over utterances of the per-utterance variance of coefficient
d) and the filter of Toda et al. (2007) that stretches each converted trajectory about its own mean

    m_d = mean(x[:, d]),  v_d = var(x[:, d]) (ddof 0),  r_d = sqrt(gv_d / v_d)
    y[t, d] = base[t, d] + strength * (r_d - 1) * (x[t, d] - m_d)            for d >= first_col

with base = x (the plain filter: at strength 1 the variance of y[:, d] is gv_d) or base = the differential conversion
of the same input.  The reference has no counterpart: it synthesises the converter's output as it is.
`gv_statistics` and `ascent` serve the parameter generation that considers the global variance instead of filtering
afterwards (kwy_gv_ascent, include/kwy.h: conjugate-gradient steps on the joint likelihood of a trajectory and of its
global variance; the conversion with it behind is backend.mlpg.MLPG(gv=...)).
Inputs follow the other shims' contract: float64, C-contiguous (the same ValueError otherwise)."""
import numpy as np

from .. import _lib
from .._lib import lib, ptr

MAX_COLS = 64


def _matrix(a):
    a = _lib.as_f64(a)
    if a.ndim != 2 or not 1 <= a.shape[1] <= MAX_COLS:
        raise ValueError(f'a (frames, columns) matrix of 1 .. {MAX_COLS} columns is expected, not shape {a.shape}')
    return a


def _strength(strength):
    strength = float(strength)
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f'global variance: strength {strength!r} is outside [0, 1]')
    return strength


def column_moments(mats, ctx=None):
    """(len(mats), cols, 3) array: (n, mean, M2) of every column of every (frames, cols) matrix"""
    mats = [_matrix(m) for m in mats]
    if not mats:
        return np.zeros((0, 0, 3))
    cols = mats[0].shape[1]
    if any(m.shape[1] != cols for m in mats):
        raise ValueError('column moments: the matrices differ in their number of columns')
    ctx = ctx or _lib.default_context()
    out = np.empty((len(mats), cols, 3))
    jobs = _lib.job_array(_lib.GvMatrix, [(m.ctypes.data, len(m)) for m in mats])
    _lib.check(ctx, lib.kwy_column_moments(ctx.handle, jobs, len(mats), cols, ptr(out)))
    return out


def gv_from_moments(moments, ctx=None):
    """the statistic: per column the mean, over the matrices that have frames, of M2 / n (a left fold in row order).
    ValueError when no matrix has frames"""
    moments = _lib.as_f64(moments)
    if moments.ndim != 3 or moments.shape[2] != 3 or not 1 <= moments.shape[1] <= MAX_COLS:
        raise ValueError('moments must be a (count, cols, 3) array')
    if len(moments) == 0 or not (moments[:, 0, 0] > 0).any():
        raise ValueError('global variance statistics: no utterance has frames')
    ctx = ctx or _lib.default_context()
    out = np.empty(moments.shape[1])
    _lib.check(ctx, lib.kwy_gv_from_moments(ctx.handle, ptr(moments), len(moments), moments.shape[1], ptr(out)))
    return out


def gv_statistics(moments, ctx=None):
    """(mean, var): per column the mean and the variance (ddof 0), over the matrices that have frames, of M2 / n -- the
    statistics of the GV ascent (kwy_gv_ascent, include/kwy.h).  The mean is gv_from_moments' value bit for bit; with
    fewer than two such matrices the variance is 0.  ValueError when no matrix has frames"""
    moments = _lib.as_f64(moments)
    if moments.ndim != 3 or moments.shape[2] != 3 or not 1 <= moments.shape[1] <= MAX_COLS:
        raise ValueError('moments must be a (count, cols, 3) array')
    if len(moments) == 0 or not (moments[:, 0, 0] > 0).any():
        raise ValueError('global variance statistics: no utterance has frames')
    ctx = ctx or _lib.default_context()
    mean, var = np.empty(moments.shape[1]), np.empty(moments.shape[1])
    _lib.check(ctx, lib.kwy_gv_stats_from_moments(ctx.handle, ptr(moments), len(moments), moments.shape[1], ptr(mean),
                                                  ptr(var)))
    return mean, var


ASCENT_MAX = 256     # KWY_MLPG_GV_MAX (include/kwy.h)


def ascent_arguments(mean, var, iterations, weight, cols=None):
    """(mean, var, iterations, weight) checked: ValueError for a count outside [0, ASCENT_MAX], a weight that is not
    positive and finite, or statistics of the wrong shape"""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or \
            not 0 <= iterations <= ASCENT_MAX:
        raise ValueError(f'GV ascent: iterations must be an integer within [0, {ASCENT_MAX}], not {iterations!r}')
    weight = float(weight)
    if not (weight > 0.0 and np.isfinite(weight)):
        raise ValueError(f'GV ascent: weight {weight!r} must be positive and finite')
    mean, var = _lib.as_f64(mean), _lib.as_f64(var)
    if mean.ndim != 1 or mean.shape != var.shape or (cols is not None and mean.shape != (cols,)):
        raise ValueError(f'GV ascent: mean and var must hold one value per column'
                         f'{"" if cols is None else f" ({cols})"}, not shapes {mean.shape} and {var.shape}')
    return mean, var, int(iterations), weight


def ascent(bands, y, mean, var, iterations, offset=None, weight=1.0, ctx=None):
    """the GV ascent on caller data (kwy_gv_ascent): bands (T, d, 4) records {P[t][t], P[t][t-1], P[t][t-2], b[t]},
    y (T, d) the solution of P y = b, offset (T, d) or None.  Returns (y_N, [Q_0 .. Q_N], status); bands, y and offset
    may be lists of utterances: one call, lists back"""
    single = not isinstance(y, (list, tuple))
    ys = [_matrix(a) for a in ([y] if single else y)]
    bs = [_lib.as_f64(b) for b in ([bands] if single else bands)]
    offs = [None] * len(ys) if offset is None else [_matrix(o) for o in ([offset] if single else offset)]
    if not ys:
        return []
    d = ys[0].shape[1]
    mean, var, iterations, weight = ascent_arguments(mean, var, iterations, weight, d)
    if len(bs) != len(ys) or len(offs) != len(ys) or any(
            a.shape[1] != d or len(a) < 1 or b.shape != a.shape + (4,) or (o is not None and o.shape != a.shape)
            for a, b, o in zip(ys, bs, offs)):
        raise ValueError('GV ascent: y (T, d), bands (T, d, 4) and offset (T, d) must agree, T >= 1')
    ctx = ctx or _lib.default_context()
    outs = [a.copy() for a in ys]
    objs = [np.empty(iterations + 1) for _ in ys]
    status = np.zeros(len(ys), dtype=np.int32)
    jobs = _lib.job_array(_lib.GvAscentJob, [(b.ctypes.data, None if o is None else o.ctypes.data, a.ctypes.data, len(a),
                                              q.ctypes.data) for b, o, a, q in zip(bs, offs, outs, objs)])
    _lib.check(ctx, lib.kwy_gv_ascent(ctx.handle, jobs, len(ys), d, ptr(mean), ptr(var), weight, iterations,
                                      ptr(status)))
    res = [(a, q.tolist(), int(s)) for a, q, s in zip(outs, objs, status)]
    return res[0] if single else res


def _raise_status(status):
    bad = [i for i, s in enumerate(status) if s]
    if bad:
        raise ValueError(f'global variance: {int(sum(status[i] for i in bad))} coefficient(s) of utterance(s) {bad} '
                         f'were left unfiltered: their variance is not finite, or the statistic is not finite or not '
                         f'positive there')


def postfilter(x, gv, strength=1.0, base=None, first_col=1, ctx=None):
    """a new matrix: `base` (default: x itself) plus strength * (r - 1) * (x - mean) on the columns from `first_col`
    on, the others copied.  x (and base) may be lists of matrices: one call, a list back.  ValueError when a
    coefficient cannot be filtered (its variance not finite, gv not finite or <= 0), naming the utterances."""
    single = not isinstance(x, (list, tuple))
    xs = [_matrix(a) for a in ([x] if single else x)]
    bases = xs if base is None else [_matrix(b) for b in ([base] if single else base)]
    strength = _strength(strength)
    if not xs:
        return []
    cols = xs[0].shape[1]
    if len(bases) != len(xs) or any(a.shape[1] != cols or b.shape != a.shape for a, b in zip(xs, bases)):
        raise ValueError('global variance: x and base must be matrices of the same shapes and column count')
    gv = _lib.as_f64(gv)
    if gv.shape != (cols,):
        raise ValueError(f'gv must hold one value per column ({cols}), not shape {gv.shape}')
    if not 0 <= int(first_col) <= cols:
        raise ValueError(f'first_col {first_col!r} is outside [0, {cols}]')
    ctx = ctx or _lib.default_context()
    outs = [np.empty_like(a) for a in xs]
    status = np.zeros(len(xs), dtype=np.int32)
    jobs = _lib.job_array(_lib.GvJob, [(a.ctypes.data, len(a), None, b.ctypes.data, o.ctypes.data)
                                       for a, b, o in zip(xs, bases, outs)])
    _lib.check(ctx, lib.kwy_gv_postfilter(ctx.handle, jobs, len(xs), cols, int(first_col), ptr(gv), strength,
                                          ptr(status)))
    _raise_status(status)
    return outs[0] if single else outs


# ---- device tensors (enqueued on the context's stream, not synchronised) ---------------------------------------------
def column_moments_batch_dev(ctx, mats, moments):
    """mats: (frames, cols) float64 device tensors; moments: a (len(mats), cols, 3) device tensor, written"""
    jobs = _lib.job_array(_lib.GvMatrix, [(m, m.shape[0]) for m in mats])
    _lib.check(ctx, lib.kwy_column_moments_batch_dev(ctx.handle, jobs, len(mats), moments.shape[1], moments.data_ptr()))


def gv_from_moments_dev(ctx, moments, gv):
    """moments: (count, cols, 3) device tensor; gv: cols doubles on the device, written"""
    _lib.check(ctx, lib.kwy_gv_from_moments_dev(ctx.handle, moments.data_ptr(), moments.shape[0], moments.shape[1],
                                                gv.data_ptr()))


def postfilter_batch_dev(ctx, xs, moments, gv, strength, outs, bases=None, first_col=1, status=None):
    """xs / bases / outs: device tensors per utterance (bases default to xs; outs[i] may be bases[i]); moments: the
    (len(xs), cols, 3) device tensor of xs; gv: cols doubles on the device; status: an int32 device tensor with a word
    per utterance, or None"""
    bases = xs if bases is None else bases
    jobs = _lib.job_array(_lib.GvJob, [(x, x.shape[0], moments[i], b, o)
                                       for i, (x, b, o) in enumerate(zip(xs, bases, outs))])
    _lib.check(ctx, lib.kwy_gv_postfilter_batch_dev(ctx.handle, jobs, len(xs), moments.shape[1], int(first_col),
                                                    gv.data_ptr(), _strength(strength),
                                                    None if status is None else status.data_ptr()))


def gv_statistics_dev(ctx, moments, mean, var):
    """moments: (count, cols, 3) device tensor; mean, var: cols doubles each on the device, written"""
    _lib.check(ctx, lib.kwy_gv_stats_from_moments_dev(ctx.handle, moments.data_ptr(), moments.shape[0], moments.shape[1],
                                                      mean.data_ptr(), var.data_ptr()))


def ascent_batch_dev(ctx, bands, ys, mean, var, iterations, offsets=None, weight=1.0, objectives=None, status=None):
    """bands (T, d, 4) / ys (T, d, in place) / offsets (T, d or None) / objectives (iterations + 1 doubles or None):
    device tensors per utterance; mean, var: d doubles on the device; status: an int32 device tensor with a word per
    utterance, or None"""
    n = len(ys)
    offsets = offsets or [None] * n
    objectives = objectives or [None] * n
    jobs = _lib.job_array(_lib.GvAscentJob, [(b, o, y, y.shape[0], q)
                                             for b, o, y, q in zip(bands, offsets, ys, objectives)])
    _lib.check(ctx, lib.kwy_gv_ascent_batch_dev(ctx.handle, jobs, n, ys[0].shape[1] if n else 1, mean.data_ptr(),
                                                var.data_ptr(), float(weight), int(iterations),
                                                None if status is None else status.data_ptr()))


def check_status(status):
    """raise for the non-zero words of a filter's status (host array / device tensor, read back here)"""
    _raise_status([int(s) for s in (status.tolist() if hasattr(status, 'tolist') else status)])
