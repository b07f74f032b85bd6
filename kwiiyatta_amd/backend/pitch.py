"""Waveform pitch shift on the device (include/kwy.h, "waveform pitch shift"): a WSOLA time stretch by `rate` -- every
10 ms frame is taken from the input position whose waveform best continues the previous frame -- resampled back to
the input's length, which multiplies every frequency by `rate` and keeps the duration

    y = resample(wsola(x, rate), len(x))                    rate within [0.5, 2.0]; rate 1 returns x bit for bit

The reference has no counterpart: its differential output keeps the source's pitch.  GMM voice-conversion recipes
shift the source recordings this way before training and conversion, so that the MLSA filter of the differential
conversion runs on a waveform that already has the target's pitch.
Inputs follow the other shims' contract: float64, C-contiguous (the same ValueError otherwise)."""
import math

import numpy as np

from .. import _lib
from .._lib import lib, ptr

RATE_RANGE = (0.5, 2.0)


def check_rate(rate):
    rate = float(rate)
    if not (math.isfinite(rate) and RATE_RANGE[0] <= rate <= RATE_RANGE[1]):
        raise ValueError(f'pitch shift: rate {rate!r} is outside [{RATE_RANGE[0]}, {RATE_RANGE[1]}]')
    return rate


def stretched_length(n, rate):
    """M: the length of the stretched signal"""
    return int(lib.kwy_pitch_stretched_length(int(n), check_rate(rate)))


def frames(n, fs, rate):
    """K: the number of 10 ms frames of the stretched signal (positions the chain chooses)"""
    k = int(lib.kwy_pitch_frames(int(n), int(fs), check_rate(rate)))
    if k < 0:
        raise ValueError(f'pitch shift: bad length {n!r} or sampling rate {fs!r}')
    return k


def shift_pitch(x, fs, rate, positions=False, ctx=None):
    """a new waveform of len(x) samples whose pitch is `rate` times that of x; positions=True: (y, p) with the int32
    input positions the frames were taken from"""
    x = _lib.as_f64(x)
    if x.ndim != 1:
        raise ValueError(f'a waveform (one axis) is expected, not shape {x.shape}')
    rate = check_rate(rate)
    p = np.zeros(frames(len(x), fs, rate), dtype=np.int32)
    ctx = ctx or _lib.default_context()
    y = np.empty_like(x)
    _lib.check(ctx, lib.kwy_pitch_shift(ctx.handle, ptr(x), len(x), int(fs), rate, ptr(y), ptr(p)))
    return (y, p) if positions else y


# ---- device tensors (enqueued on the context's stream, not synchronised) ---------------------------------------------
def shift_pitch_batch_dev(ctx, xs, ys, fs, rate, positions=None):
    """xs / ys: float64 device tensors per waveform (ys[i] as long as xs[i], not the same memory); positions: None, or
    per waveform an int32 device tensor of frames(len, fs, rate) values (or None).  One grid over all waveforms."""
    rate = check_rate(rate)
    if not xs:
        return
    positions = [None] * len(xs) if positions is None else positions
    jobs = _lib.job_array(_lib.PitchJob, [(x, x.numel(), y, p) for x, y, p in zip(xs, ys, positions)])
    _lib.check(ctx, lib.kwy_pitch_shift_batch_dev(ctx.handle, jobs, len(xs), int(fs), rate))
