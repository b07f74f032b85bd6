"""Formant shift on the device (include/kwy.h, "formant shift"): a frequency-axis warp of spectral envelopes that
moves every formant by the ratio rho -- the apparent vocal-tract length -- and leaves pitch and aperiodicity alone

    u_k = k / rho,  j = floor(u_k),  a = u_k - j,  l = log(sp[t])
    out[t, k] = sp[t, K-1]                          if j >= K-1     (the band nothing maps to holds the edge value)
              = sp[t, j]                            if a == 0
              = exp(l[j] + a * (l[j+1] - l[j]))     otherwise

The reference has no counterpart: its dialog transposes the key only.
Inputs follow the other shims' contract: float64, C-contiguous (the same ValueError otherwise)."""
import math

import numpy as np

from .. import _lib
from .._lib import lib, ptr

RATIO_RANGE = (0.5, 2.0)
SEMITONE_RANGE = 12.0    # 2 ** (+-12 / 12): the ends of RATIO_RANGE
MAX_K = 2049             # KWY_FORMANT_MAX_K: the envelope width of the longest transform CheapTrick accepts


def semitone_ratio(semitones):
    """rho of a shift by so many semitones, formed on the host as the key transposition's factor is"""
    return 2.0 ** (semitones / 12)


def check_ratio(ratio):
    """the ratio as a float; ValueError unless it is finite and within [0.5, 2]"""
    try:
        rho = float(ratio)
    except (TypeError, ValueError):
        raise ValueError(f'formant shift: the ratio {ratio!r} is not a number') from None
    lo, hi = RATIO_RANGE
    if not (math.isfinite(rho) and lo <= rho <= hi):
        raise ValueError(f'formant shift: the ratio {ratio!r} is outside [{lo}, {hi}]')
    return rho


def _matrix(a):
    a = _lib.as_f64(a)
    if a.ndim != 2 or not 2 <= a.shape[1] <= MAX_K:
        raise ValueError(f'a (frames, bins) envelope matrix of 2 .. {MAX_K} bins is expected, not shape {a.shape}')
    return a


def _raise_status(status, what='matrix / matrices'):
    bad = [i for i, s in enumerate(status) if s]
    if bad:
        raise ValueError(f'formant shift: {int(sum(status[i] for i in bad))} row(s) of {what} {bad} were left '
                         f'as they are: they hold values that are not finite or not positive')


def shift_formants(sp, ratio, ctx=None):
    """a new matrix: the envelope rows of `sp` warped by `ratio` (> 1: formants up).  sp may be a list of matrices of
    one width: one call, a list back.  ValueError when a row cannot be warped (a value not finite or <= 0), naming the
    matrices."""
    rho = check_ratio(ratio)
    single = not isinstance(sp, (list, tuple))
    mats = [_matrix(a) for a in ([sp] if single else sp)]
    if not mats:
        return []
    K = mats[0].shape[1]
    if any(a.shape[1] != K for a in mats):
        raise ValueError('formant shift: the matrices differ in their number of bins')
    ctx = ctx or _lib.default_context()
    outs = [np.empty_like(a) for a in mats]
    status = np.zeros(len(mats), dtype=np.int32)
    jobs = _lib.job_array(_lib.FormantJob, [(a.ctypes.data, len(a), o.ctypes.data) for a, o in zip(mats, outs)])
    _lib.check(ctx, lib.kwy_formant_shift(ctx.handle, jobs, len(mats), K, rho, ptr(status)))
    _raise_status(status)
    return outs[0] if single else outs


# ---- device tensors (enqueued on the context's stream, not synchronised) ---------------------------------------------
def shift_formants_batch_dev(ctx, mats, outs, ratio, status=None):
    """mats / outs: (frames, bins) float64 device tensors of one width (outs[i] may be mats[i]); status: an int32
    device tensor with a word per matrix, or None"""
    jobs = _lib.job_array(_lib.FormantJob, [(a, a.shape[0], o) for a, o in zip(mats, outs)])
    _lib.check(ctx, lib.kwy_formant_shift_batch_dev(ctx.handle, jobs, len(mats), mats[0].shape[1], check_ratio(ratio),
                                                    None if status is None else status.data_ptr()))


def check_status(status, what='matrix / matrices'):
    """raise for the non-zero words of a shift's status (host array / device tensor, read back here); `what` names
    what a word stands for"""
    _raise_status([int(s) for s in (status.tolist() if hasattr(status, 'tolist') else status)], what)
