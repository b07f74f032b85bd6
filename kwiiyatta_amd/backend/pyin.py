"""Probabilistic YIN (Mauch & Dixon 2014) on the device: the second f0 estimator beside DIO (include/kwy.h, "probabilistic
YIN", states the algorithm step by step).

    f0, t = pyin(x, fs)                  the coarse track on DIO's frame grid, like `world.dio`
    f0 = world.stonemask(x, f0, t, fs)   refined exactly as DIO's is

`observe` (the per-frame log probabilities L) and `decode` (the Viterbi pass over a caller's L) are the two stages on
their own.  The reference has no counterpart.  Inputs follow the other shims' contract: float64, C-contiguous.
A signal with a non-finite sample is a ValueError."""
import math

import numpy as np

from .. import _lib
from .._lib import lib, ptr

BINS_PER_OCTAVE = 120
F0_ESTIMATORS = ('dio', 'pyin')         # the coarse f0 estimators of the analysis: the one list of their names
default_frame_period = 5.0
default_f0_floor = 71.0
default_f0_ceil = 800.0
default_p_a = 0.01
default_switch_prob = 0.01
default_max_rate = 35.92          # octaves per second


def check_estimator(estimator):
    if estimator not in F0_ESTIMATORS:
        raise ValueError(f'f0 estimator: {estimator!r} is not one of {F0_ESTIMATORS}')
    return estimator


def frames(fs, x_length, frame_period=default_frame_period):
    if not (int(fs) > 0 and float(frame_period) > 0):
        raise ValueError('pyin: bad argument')
    return int(lib.kwy_dio_frames(int(fs), int(x_length), float(frame_period)))


def fft_size(fs, f0_floor=default_f0_floor):
    """length of the frame transform (supported: up to 4096)"""
    return int(lib.kwy_pyin_fft_size(int(fs), float(f0_floor)))


def bins(f0_floor=default_f0_floor, f0_ceil=default_f0_ceil):
    """pitch bins nb of the range; L has nb + 1 columns, the decoder 2 nb states"""
    nb = int(lib.kwy_pyin_bins(float(f0_floor), float(f0_ceil)))
    if nb < 1:
        raise ValueError('pyin: bad f0 range')
    return nb


def radius(frame_period=default_frame_period, max_rate=default_max_rate):
    """bins R the pitch may move between two frames"""
    r = int(lib.kwy_pyin_radius(float(frame_period), float(max_rate)))
    if r < 0:
        raise ValueError('pyin: bad pitch rate')
    return r


def scratch_bytes(n_frames, nb, count=1):
    """bytes of context scratch the device entries take for `count` utterances of up to n_frames frames"""
    return int(lib.kwy_pyin_scratch_bytes(int(n_frames), int(nb), int(count)))


def transition_table(R, switch_prob=default_switch_prob):
    """the 2 (2 R + 1) log transition values [voicing kept | voicing changed][k + R] the decoder adds"""
    k = np.abs(np.arange(-R, R + 1))
    w = (R + 1 - k) / float((R + 1) * (R + 1))
    return np.ascontiguousarray(np.concatenate([np.log(w * (1.0 - switch_prob)), np.log(w * switch_prob)]))


def bin_frequencies(nb, f0_floor=default_f0_floor):
    """the track's value for voiced bin b: the bin's centre f0_floor 2^((b + 1/2) / 120)"""
    return np.array([f0_floor * math.pow(2.0, (b + 0.5) / BINS_PER_OCTAVE) for b in range(nb)])


def pyin(x, fs, f0_floor=default_f0_floor, f0_ceil=default_f0_ceil, frame_period=default_frame_period,
         p_a=default_p_a, switch_prob=default_switch_prob, max_rate=default_max_rate, ctx=None):
    """(f0, t) like `world.dio`: the coarse pYIN track and the frame times"""
    x = _lib.as_f64(x)
    ctx = ctx or _lib.default_context()
    T = frames(fs, len(x), frame_period)
    f0 = np.empty(T)
    t = np.empty(T)
    _lib.check(ctx, lib.kwy_pyin(ctx.handle, ptr(x), len(x), int(fs), float(f0_floor), float(f0_ceil),
                                 float(frame_period), float(p_a), float(switch_prob), float(max_rate), ptr(t), ptr(f0)))
    return f0, t


def observe(x, fs, f0_floor=default_f0_floor, f0_ceil=default_f0_ceil, frame_period=default_frame_period,
            p_a=default_p_a, ctx=None):
    """L (frames, nb + 1): the log probabilities of the pitch bins and, last, of an unvoiced state"""
    x = _lib.as_f64(x)
    ctx = ctx or _lib.default_context()
    L = np.empty((frames(fs, len(x), frame_period), bins(f0_floor, f0_ceil) + 1))
    _lib.check(ctx, lib.kwy_pyin_observe(ctx.handle, ptr(x), len(x), int(fs), float(f0_floor), float(f0_ceil),
                                         float(frame_period), float(p_a), ptr(L)))
    return L


def decode(L, trans, freq, ctx=None):
    """the Viterbi track over L (T, nb + 1) with `transition_table` values and `bin_frequencies`"""
    L, trans, freq = _lib.as_f64(L), _lib.as_f64(trans), _lib.as_f64(freq)
    if L.ndim != 2 or L.shape[0] < 1 or L.shape[1] != len(freq) + 1 or len(trans) % 2 != 0 or (len(trans) // 2) % 2 != 1:
        raise ValueError('decode: L (T, nb + 1), trans 2 (2 R + 1) values and freq nb values are expected')
    ctx = ctx or _lib.default_context()
    f0 = np.empty(L.shape[0])
    _lib.check(ctx, lib.kwy_pyin_decode(ctx.handle, ptr(L), L.shape[0], len(freq), ptr(trans), len(trans) // 4,
                                        ptr(freq), ptr(f0)))
    return f0


def pyin_batch_dev(ctx, waves, fs, t_out, f0_out, status=None, f0_floor=default_f0_floor, f0_ceil=default_f0_ceil,
                   frame_period=default_frame_period, p_a=default_p_a, switch_prob=default_switch_prob,
                   max_rate=default_max_rate):
    """`pyin` for every waveform of `waves` (float64 device tensors), enqueued on the context's stream and not
    synchronised: the drop-in for `world.dio_batch_dev`.  status: an int32 device tensor with one word per utterance
    (non-zero afterwards: a non-finite sample, the track is all zero; see `check_status`), or None."""
    rows = [(x, x.numel(), t, f, (status[i:i + 1] if status is not None else 0))
            for i, (x, t, f) in enumerate(zip(waves, t_out, f0_out))]
    jobs = _lib.job_array(_lib.F0Job, rows)
    _lib.check(ctx, lib.kwy_pyin_batch_dev(ctx.handle, jobs, len(rows), int(fs), float(f0_floor), float(f0_ceil),
                                           float(frame_period), float(p_a), float(switch_prob), float(max_rate)))


def check_status(status, what='pyin'):
    """raise for a non-zero status word (host array / device tensor, read back here)"""
    words = status.tolist() if hasattr(status, 'tolist') else list(status)
    bad = [i for i, s in enumerate(words) if int(s)]
    if bad:
        raise ValueError(f'{what}: a sample of the signal is not finite (utterance {bad[0]} of the batch)')
