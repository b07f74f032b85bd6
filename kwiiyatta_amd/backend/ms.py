"""Modulation-spectrum postfilter on the device (include/kwy.h, "modulation spectrum"): the log modulation spectra of
mel-cepstrum matrices, their running statistics, and the utterance-level filter of Takamichi et al. (2016), which
moves every modulation-frequency bin of a converted trajectory from the statistics G of converted speech to the
statistics N of the target speaker's natural speech and keeps the phase

    z = x[:, d] - mean, zero-padded to L;  Z = rfft(z);  s[f] = log(max(|Z[f]|^2, DBL_MIN) / T)
    s'[f] = (1 - k) s[f] + k (sigmaN[f] / sigmaG[f] (s[f] - muG[f]) + muN[f]);  g[f] = exp((s'[f] - s[f]) / 2), g[0] = 1
    y[t, d] = base[t, d] + (irfft(g Z)[t] - z[t])                              for d >= first_col

with base = x (the plain filter) or base = the differential conversion of the same input.  Statistics are
(cols, L/2 + 1, 3) arrays of (n, mean, M2) per column and bin; bin 0 carries none.  The global-variance filter
(backend/gv.py) is the one-bin case.  The reference has no counterpart: it synthesises the converter's output as it is.
Inputs follow the other shims' contract: float64, C-contiguous (the same ValueError otherwise)."""
import numpy as np

from .. import _lib
from .._lib import lib, ptr

MAX_COLS = 64
LENGTHS = (512, 1024, 2048, 4096, 8192)
GROUP = 64               # matrices per call of `statistics`


def _matrix(a):
    a = _lib.as_f64(a)
    if a.ndim != 2 or not 1 <= a.shape[1] <= MAX_COLS:
        raise ValueError(f'a (frames, columns) matrix of 1 .. {MAX_COLS} columns is expected, not shape {a.shape}')
    return a


def _length(length):
    length = int(length)
    if length not in LENGTHS:
        raise ValueError(f'modulation spectrum: the transform length must be one of {LENGTHS}, not {length!r}')
    return length


def _strength(strength):
    strength = float(strength)
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f'modulation spectrum: strength {strength!r} is outside [0, 1]')
    return strength


def _fits(rows, length):
    for T in rows:
        if T > length:
            raise ValueError(f'modulation spectrum: an utterance of T = {T} frames is longer than the transform length '
                             f'L = {length}')


def _stats(stats, cols, name):
    stats = _lib.as_f64(stats)
    if stats.ndim != 3 or stats.shape[0] != cols or stats.shape[2] != 3 or 2 * (stats.shape[1] - 1) not in LENGTHS:
        raise ValueError(f'{name} must be a ({cols}, L/2 + 1, 3) array with L one of {LENGTHS}, not shape {stats.shape}')
    return stats


def _same_cols(mats, what):
    cols = mats[0].shape[1]
    if any(m.shape[1] != cols for m in mats):
        raise ValueError(f'{what}: the matrices differ in their number of columns')
    return cols


def log_spectra(mats, length, ctx=None):
    """(spectra (len(mats), cols, L/2 + 1), valid (len(mats), cols) int32) of (frames, cols) matrices; a column with
    fewer than two frames or without any variation has valid 0 and a row of zeros"""
    mats = [_matrix(m) for m in mats]
    length = _length(length)
    if not mats:
        return np.zeros((0, 0, length // 2 + 1)), np.zeros((0, 0), dtype=np.int32)
    cols = _same_cols(mats, 'log spectra')
    _fits([len(m) for m in mats], length)
    ctx = ctx or _lib.default_context()
    spectra = np.empty((len(mats), cols, length // 2 + 1))
    valid = np.empty((len(mats), cols), dtype=np.int32)
    jobs = _lib.job_array(_lib.GvMatrix, [(m.ctypes.data, len(m)) for m in mats])
    _lib.check(ctx, lib.kwy_ms_logspectra(ctx.handle, jobs, len(mats), cols, length, ptr(spectra), ptr(valid)))
    return spectra, valid


def new_accumulator(cols, length):
    return np.zeros((int(cols), _length(length) // 2 + 1, 3))


def stats_update(acc, spectra, valid, ctx=None):
    """folds the rows of `spectra` into the (cols, L/2 + 1, 3) accumulator `acc` by Welford's step, in index order and
    in place; returns acc"""
    spectra = _lib.as_f64(spectra)
    valid = np.asarray(valid)
    if not (acc.dtype == np.float64 and acc.flags['C_CONTIGUOUS'] and acc.flags['WRITEABLE']):
        raise ValueError('the accumulator must be a writeable C-contiguous float64 array')
    if spectra.ndim != 3 or acc.shape != spectra.shape[1:] + (3,) or valid.shape != spectra.shape[:2] \
            or valid.dtype != np.int32 or not valid.flags['C_CONTIGUOUS']:
        raise ValueError('stats update: acc (cols, K, 3), spectra (count, cols, K) and valid (count, cols) int32 '
                         'must agree')
    if len(spectra) == 0:
        return acc
    length = _length(2 * (spectra.shape[2] - 1))
    ctx = ctx or _lib.default_context()
    _lib.check(ctx, lib.kwy_ms_stats_update(ctx.handle, ptr(acc), ptr(spectra), ptr(valid), len(spectra),
                                            spectra.shape[1], length))
    return acc


def statistics(mats, length, ctx=None):
    """the (cols, L/2 + 1, 3) statistics of a list of matrices, GROUP at a time"""
    mats = [_matrix(m) for m in mats]
    if not mats:
        raise ValueError('modulation spectrum statistics: no utterance')
    acc = new_accumulator(_same_cols(mats, 'statistics'), length)
    for i in range(0, len(mats), GROUP):
        stats_update(acc, *log_spectra(mats[i:i + GROUP], length, ctx), ctx=ctx)
    return acc


def _raise_status(status):
    bad = [i for i, s in enumerate(status) if s]
    if bad:
        raise ValueError(f'modulation spectrum: {int(sum(status[i] for i in bad))} bin(s) of utterance(s) {bad} were '
                         f'left unfiltered: their statistics or their gain are not usable')


def postfilter(x, stats_g, stats_n, strength=1.0, base=None, first_col=1, length=None, ctx=None):
    """a new matrix: `base` (default: x itself) plus the change the filter makes to x on the columns from `first_col`
    on, the others copied.  x (and base) may be lists of matrices: one call, a list back.  `length` defaults to the
    statistics' own.  ValueError when bins cannot be filtered, naming the utterances, and for an utterance longer than
    the transform."""
    single = not isinstance(x, (list, tuple))
    xs = [_matrix(a) for a in ([x] if single else x)]
    bases = xs if base is None else [_matrix(b) for b in ([base] if single else base)]
    strength = _strength(strength)
    if not xs:
        return []
    cols = xs[0].shape[1]
    if len(bases) != len(xs) or any(a.shape[1] != cols or b.shape != a.shape for a, b in zip(xs, bases)):
        raise ValueError('modulation spectrum: x and base must be matrices of the same shapes and column count')
    stats_g, stats_n = _stats(stats_g, cols, 'stats_g'), _stats(stats_n, cols, 'stats_n')
    own = 2 * (stats_g.shape[1] - 1)
    if stats_n.shape != stats_g.shape or (length is not None and _length(length) != own):
        raise ValueError(f'modulation spectrum: the statistics are of length {own} and {2 * (stats_n.shape[1] - 1)}, '
                         f'the call asks for {length}')
    if not 0 <= int(first_col) <= cols:
        raise ValueError(f'first_col {first_col!r} is outside [0, {cols}]')
    _fits([len(a) for a in xs], own)
    ctx = ctx or _lib.default_context()
    outs = [np.empty_like(a) for a in xs]
    status = np.zeros(len(xs), dtype=np.int32)
    jobs = _lib.job_array(_lib.MsJob, [(a.ctypes.data, len(a), b.ctypes.data, o.ctypes.data)
                                       for a, b, o in zip(xs, bases, outs)])
    _lib.check(ctx, lib.kwy_ms_postfilter(ctx.handle, jobs, len(xs), cols, int(first_col), own, ptr(stats_g),
                                          ptr(stats_n), strength, ptr(status)))
    _raise_status(status)
    return outs[0] if single else outs


# ---- device tensors (enqueued on the context's stream, not synchronised) ---------------------------------------------
def log_spectra_batch_dev(ctx, mats, length, spectra, valid):
    """mats: (frames, cols) float64 device tensors; spectra: (len(mats), cols, L/2 + 1) float64 and valid:
    (len(mats), cols) int32 device tensors, written"""
    _fits([m.shape[0] for m in mats], _length(length))
    jobs = _lib.job_array(_lib.GvMatrix, [(m, m.shape[0]) for m in mats])
    _lib.check(ctx, lib.kwy_ms_logspectra_batch_dev(ctx.handle, jobs, len(mats), spectra.shape[1], length,
                                                    spectra.data_ptr(), valid.data_ptr()))


def stats_update_dev(ctx, acc, spectra, valid):
    """acc: (cols, L/2 + 1, 3) device tensor, updated; spectra / valid as log_spectra_batch_dev wrote them"""
    _lib.check(ctx, lib.kwy_ms_stats_update_dev(ctx.handle, acc.data_ptr(), spectra.data_ptr(), valid.data_ptr(),
                                                spectra.shape[0], spectra.shape[1], 2 * (spectra.shape[2] - 1)))


def postfilter_batch_dev(ctx, xs, stats_g, stats_n, strength, outs, bases=None, first_col=1, status=None):
    """xs / bases / outs: device tensors per utterance (bases default to xs; outs[i] may be bases[i] or xs[i]);
    stats_g / stats_n: (cols, L/2 + 1, 3) device tensors; status: an int32 device tensor with a word per utterance, or
    None"""
    bases = xs if bases is None else bases
    length = 2 * (stats_g.shape[1] - 1)
    _fits([x.shape[0] for x in xs], length)
    jobs = _lib.job_array(_lib.MsJob, [(x, x.shape[0], b, o) for x, b, o in zip(xs, bases, outs)])
    _lib.check(ctx, lib.kwy_ms_postfilter_batch_dev(ctx.handle, jobs, len(xs), stats_g.shape[0], int(first_col), length,
                                                    stats_g.data_ptr(), stats_n.data_ptr(), _strength(strength),
                                                    None if status is None else status.data_ptr()))


def check_status(status):
    """raise for the non-zero words of a filter's status (host array / device tensor, read back here)"""
    _raise_status([int(s) for s in (status.tolist() if hasattr(status, 'tolist') else status)])
