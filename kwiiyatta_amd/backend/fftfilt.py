"""Frame-parallel FFT form of the differential mel-cepstral filter (include/kwy.h, "frame-parallel FFT form of the
differential filter"): every frame of the waveform is filtered through the closed frequency response of its
mel-cepstrum

    H_i[k] = exp( sum_{m >= m0} mc[i][m] exp(-j m w~_k) )      w~: the frequency axis warped by the all-pass of alpha

by a transform of its own (overlap-save), and the outputs of the filter of the frame before and of the frame's own
are crossfaded across the frame.  All frames run side by side, where the MLSA filter (backend.sptk) is serial in the
sample.  Inputs follow the other shims' contract: float64, C-contiguous (the same ValueError otherwise)."""
import numpy as np

from .. import _lib
from .._lib import lib, ptr

FFT_SIZES = (1024, 2048, 4096, 8192)


def fft_filter_size(fs, hopsize):
    """the transform length for sampling rate fs and hop `hopsize`: a power of two that leaves 25 ms behind the hop
    for the impulse response to die in, 1024 at least; ValueError when that is more than 8192"""
    n = int(lib.kwy_mcep_filter_fft_size(int(fs), int(hopsize)))
    if n == 0:
        raise ValueError(f'fft filter: no transform length for fs {fs!r} and hopsize {hopsize!r} (8192 is the longest)')
    return n


def mcep_fft_filter(x, mc, alpha, hopsize, fft_size, ignore_c0=True, ctx=None):
    """x (n samples) filtered frame by frame with the mel-cepstra mc (T, order+1); a new array"""
    x = _lib.as_f64(np.asarray(x, dtype=np.float64))
    if x.ndim != 1:
        raise ValueError(f'a waveform (one axis) is expected, not shape {x.shape}')
    mc = np.ascontiguousarray(mc, dtype=np.float64)
    if mc.ndim != 2:
        raise ValueError(f'mel-cepstra (frames, order + 1) are expected, not shape {mc.shape}')
    ctx = ctx or _lib.default_context()
    y = np.empty_like(x)
    _lib.check(ctx, lib.kwy_mcep_filter_fft(ctx.handle, ptr(x), len(x), ptr(mc), mc.shape[0], mc.shape[1] - 1,
                                            float(alpha), int(hopsize), int(fft_size), int(bool(ignore_c0)), ptr(y)))
    return y


# ---- device tensors (enqueued on the context's stream, not synchronised) ---------------------------------------------
def mcep_fft_filter_batch_dev(ctx, xs, mcs, ys, alpha, hopsize, fft_size, ignore_c0=True):
    """xs / ys: float64 device tensors per waveform (ys[i] as long as xs[i], not the same memory); mcs: (T, order+1)
    float64 device tensors of one order.  One grid over all frames of all waveforms."""
    if not xs:
        return
    order = mcs[0].shape[1] - 1
    if any(m.shape[1] - 1 != order for m in mcs):
        raise ValueError('fft filter: the mel-cepstra of a batch share one order')
    jobs = _lib.job_array(_lib.MlsaJob, [(x, x.numel(), m, m.shape[0], y) for x, m, y in zip(xs, mcs, ys)])
    _lib.check(ctx, lib.kwy_mcep_filter_fft_batch_dev(ctx.handle, jobs, len(xs), order, float(alpha), int(hopsize),
                                                      int(fft_size), int(bool(ignore_c0))))
