"""f0 conversion on the device (include/kwy.h, "f0 conversion"): the voiced log-f0 moments of f0 tracks, their merge
into corpus statistics, and the per-frame map

    log f0' = (log f0 - mu_src) * sigma_tgt / sigma_src + mu_tgt          (voiced frames)
    f0'     = f0' * 2 ** (key / 12)

whose key ratio is the reference dialog's transposition (/root/reference/kwiiyatta/view/qt/kwiieiya.py:152-155).
Inputs follow the other shims' contract: float64, C-contiguous (the same ValueError otherwise)."""
import numpy as np

from .. import _lib
from .._lib import lib, ptr

KEY_RANGE = 99.99      # the dialog's QDoubleSpinBox (view/qt/ui/kwiieiya.ui:262-280)


def key_ratio(key):
    """the dialog's factor, formed on the host exactly as it does"""
    return 2.0 ** (key / 12)


def f0_limit(fs):
    """the highest f0 (exclusive) a mapped track may reach: the synthesis plan holds y_length / 8 + 16 pulses"""
    return fs / 8


def logf0_moments(tracks, ctx=None):
    """(len(tracks), 3) array: (n, mean, M2) of log f0 over the voiced frames (f0 > 0) of every track"""
    tracks = [_lib.as_f64(f) for f in tracks]
    if not tracks:
        return np.zeros((0, 3))
    ctx = ctx or _lib.default_context()
    out = np.empty((len(tracks), 3))
    jobs = _lib.job_array(_lib.F0Track, [(f.ctypes.data, len(f)) for f in tracks])
    _lib.check(ctx, lib.kwy_logf0_moments(ctx.handle, jobs, len(tracks), ptr(out)))
    return out


def merge_moments(m, ctx=None):
    """(n, mean, M2) of the concatenation of the tracks whose triples are the rows of `m` (Chan's combination, a left
    fold in row order)"""
    m = _lib.as_f64(m)
    if m.ndim != 2 or m.shape[1] != 3 or len(m) == 0:
        raise ValueError('moments must be a non-empty (count, 3) array')
    ctx = ctx or _lib.default_context()
    out = np.empty(3)
    _lib.check(ctx, lib.kwy_logf0_moments_merge(ctx.handle, ptr(m), len(m), ptr(out)))
    return out


def stats_from_moments(source, target):
    """(mu_src, sigma_src, mu_tgt, sigma_tgt) of the two sides' merged moments; sigma with ddof 0"""
    stats = []
    for side, (n, mean, m2) in (('source', source), ('target', target)):
        n, mean, m2 = float(n), float(mean), float(m2)
        if n <= 0:
            raise ValueError(f'f0 statistics: the {side} side has no voiced frames')
        sigma = float(np.sqrt(m2 / n))
        if not sigma > 0:
            raise ValueError(f'f0 statistics: the voiced log-f0 of the {side} side has zero variance')
        stats += [mean, sigma]
    return tuple(stats)


def _raise_status(status, fs):
    bad = [i for i, s in enumerate(status) if s]
    if bad:
        raise ValueError(f'f0 map: {int(sum(status[i] for i in bad))} frame(s) of track(s) {bad} are negative, not '
                         f'finite or mapped to f0 >= fs/8 = {f0_limit(fs):g} Hz (the limit of the synthesis plan)')


def map_f0(f0, fs, stats=None, key=0.0, ctx=None):
    """a new track: voiced frames through the normalised log-Gaussian transform of `stats` (a 4-tuple, or None for
    none) and times 2 ** (key / 12); unvoiced frames stay 0.  ValueError when a frame is negative or not finite or
    its result reaches fs/8 Hz."""
    f0 = _lib.as_f64(f0)
    ctx = ctx or _lib.default_context()
    out = np.empty_like(f0)
    st = None if stats is None else np.ascontiguousarray(stats, dtype=np.float64)
    if st is not None and st.shape != (4,):
        raise ValueError('stats must be (mu_src, sigma_src, mu_tgt, sigma_tgt)')
    status = np.zeros(1, dtype=np.int32)
    jobs = _lib.job_array(_lib.F0MapJob, [(f0.ctypes.data, len(f0), out.ctypes.data)])
    _lib.check(ctx, lib.kwy_f0_map(ctx.handle, jobs, 1, int(fs), None if st is None else ptr(st),
                                   float(key_ratio(key)), ptr(status)))
    _raise_status(status, fs)
    return out


# ---- device tensors (enqueued on the context's stream, not synchronised) ---------------------------------------------
def logf0_moments_batch_dev(ctx, tracks, moments):
    """moments: a (len(tracks), 3) float64 device tensor, written"""
    jobs = _lib.job_array(_lib.F0Track, [(f, f.numel()) for f in tracks])
    _lib.check(ctx, lib.kwy_logf0_moments_batch_dev(ctx.handle, jobs, len(tracks), moments.data_ptr()))


def merge_moments_dev(ctx, moments, out):
    """moments: (count, 3) device tensor; out: 3 doubles on the device, written"""
    _lib.check(ctx, lib.kwy_logf0_moments_merge_dev(ctx.handle, moments.data_ptr(), moments.shape[0], out.data_ptr()))


def map_f0_batch_dev(ctx, f0_in, f0_out, fs, stats=None, key=0.0, status=None):
    """f0_in / f0_out: device tensors per track (f0_out[i] may be f0_in[i]); stats: 4 doubles on the device or None;
    status: an int32 device tensor with a word per track, or None"""
    jobs = _lib.job_array(_lib.F0MapJob, [(a, a.numel(), b) for a, b in zip(f0_in, f0_out)])
    _lib.check(ctx, lib.kwy_f0_map_batch_dev(ctx.handle, jobs, len(f0_in), int(fs),
                                             None if stats is None else stats.data_ptr(), float(key_ratio(key)),
                                             None if status is None else status.data_ptr()))


def check_status(status, fs):
    """raise for the non-zero words of a map's status (host array / device tensor, read back here)"""
    _raise_status([int(s) for s in (status.tolist() if hasattr(status, 'tolist') else status)], fs)
