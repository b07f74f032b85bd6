"""Mel-cepstral energy on the device (include/kwy.h, "mel-cepstral energy"): the energy of every frame of a
mel-cepstrum without its spectrum

    L_k = sum_m c[m] cos(m w~_k),   E(c) = (exp 2 L_0 + exp 2 L_{N/2} + 2 sum_{0 < k < N/2} exp 2 L_k) / N

and the filter built on it: the formant-emphasis postfilter of strength beta (mc2b, b[1] -= beta alpha b[2],
b[2..] *= 1 + beta, and back) whose c0 is shifted by log(E(ref) / E(y)) / 2, so that the filtered frame has the energy
of the reference frame -- its own input when there is none.  beta = 0 with a reference is the power-preserving shift
alone: c1.. stay, c0 becomes the one at which the frame is as loud as the reference's.  With `base` the filter's change
is added to another matrix (out = base + (y - x), the differential form of the GV and MS filters).  The reference has
no counterpart.  Inputs follow the other shims' contract: float64, C-contiguous (the same ValueError otherwise)."""
import numpy as np

from .. import _lib
from .._lib import lib, ptr

MAX_ORDER = 63
FFT_SIZES = (512, 1024, 2048, 4096, 8192)


def energy_fft_size(fs):
    """the transform length the energies of a mel-cepstrum at `fs` are taken over: that of the vocoder's spectrum,
    2 (fs_spectrum_len(fs) - 1) -- 1024 at 16 and 22.05 kHz, 2048 at 44.1 and 48 kHz, 4096 at 96 kHz"""
    import kwiiyatta_amd as k
    return 2 * (k.Synthesizer.fs_spectrum_len(fs) - 1)


def _matrix(a):
    a = _lib.as_f64(a)
    if a.ndim != 2 or not 2 <= a.shape[1] <= MAX_ORDER + 1:
        raise ValueError(f'mel-cepstra (frames, order + 1) of order 1 .. {MAX_ORDER} are expected, not shape {a.shape}')
    return a


def beta_argument(beta):
    beta = float(beta)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f'postfilter: beta {beta!r} is outside [0, 1]')
    return beta


def _fft_size(fft_size):
    if fft_size not in FFT_SIZES:
        raise ValueError(f'mel-cepstral energy: fft_size {fft_size!r} is not one of {FFT_SIZES}')
    return int(fft_size)


def frame_energy(mc, alpha, fft_size, ctx=None):
    """E of every row of mc (frames, order + 1): a new array of `frames` doubles"""
    mc = _matrix(mc)
    ctx = ctx or _lib.default_context()
    out = np.empty(len(mc))
    _lib.check(ctx, lib.kwy_mcep_energy(ctx.handle, ptr(mc), len(mc), mc.shape[1] - 1, float(alpha), _fft_size(fft_size),
                                        ptr(out)))
    return out


def _raise_status(status):
    bad = [i for i, s in enumerate(status) if s]
    if bad:
        raise ValueError(f'postfilter: {int(sum(status[i] for i in bad))} frame(s) of utterance(s) {bad} were left '
                         f'unfiltered: their energy, or that of their reference, is not finite or not positive')


def postfilter(mc, beta=0.0, ref=None, base=None, alpha=0.0, fft_size=1024, ctx=None):
    """a new matrix: the rows of `mc` through the formant emphasis of strength beta, their c0 shifted to the energy of
    the rows of `ref` (default: of mc itself); with `base`, base plus the filter's change of mc.  mc (and ref, base)
    may be lists of matrices: one call, a list back.  ValueError when a row cannot be filtered (an energy that is not
    finite or not positive), naming the utterances."""
    single = not isinstance(mc, (list, tuple))
    wrap = (lambda a: None if a is None else [a]) if single else (lambda a: a)
    xs = [_matrix(a) for a in wrap(mc)]
    refs = [None] * len(xs) if ref is None else [_matrix(a) for a in wrap(ref)]
    bases = [None] * len(xs) if base is None else [_matrix(a) for a in wrap(base)]
    beta, fft_size = beta_argument(beta), _fft_size(fft_size)
    if not xs:
        return []
    cols = xs[0].shape[1]
    if len(refs) != len(xs) or len(bases) != len(xs) or any(
            a.shape[1] != cols or any(o is not None and o.shape != a.shape for o in (r, b))
            for a, r, b in zip(xs, refs, bases)):
        raise ValueError('postfilter: mc, ref and base must be matrices of the same shapes and one order')
    ctx = ctx or _lib.default_context()
    outs = [np.empty_like(a) for a in xs]
    status = np.zeros(len(xs), dtype=np.int32)
    at = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    jobs = _lib.job_array(_lib.McPowerJob, [(at(a), at(r), at(b), at(o), len(a))
                                            for a, r, b, o in zip(xs, refs, bases, outs)])
    _lib.check(ctx, lib.kwy_mcep_postfilter(ctx.handle, jobs, len(xs), cols - 1, float(alpha), fft_size, beta,
                                            ptr(status)))
    _raise_status(status)
    return outs[0] if single else outs


# ---- device tensors (enqueued on the context's stream, not synchronised) ---------------------------------------------
def frame_energy_batch_dev(ctx, mcs, energies, alpha, fft_size):
    """mcs: (frames, order + 1) float64 device tensors of one order; energies: `frames` doubles each, written"""
    if not mcs:
        return
    jobs = _lib.job_array(_lib.EnergyJob, [(m, m.shape[0], e) for m, e in zip(mcs, energies)])
    _lib.check(ctx, lib.kwy_mcep_energy_batch_dev(ctx.handle, jobs, len(mcs), mcs[0].shape[1] - 1, float(alpha),
                                                  int(fft_size)))


def postfilter_batch_dev(ctx, xs, outs, alpha, fft_size, beta=0.0, refs=None, bases=None, status=None):
    """xs / refs / bases / outs: device tensors per utterance (refs, bases: None, or lists whose items may be None;
    outs[i] may be xs[i] or bases[i]); status: an int32 device tensor with a word per utterance, or None"""
    if not xs:
        return
    refs = refs or [None] * len(xs)
    bases = bases or [None] * len(xs)
    jobs = _lib.job_array(_lib.McPowerJob, [(x, r, b, o, x.shape[0]) for x, r, b, o in zip(xs, refs, bases, outs)])
    _lib.check(ctx, lib.kwy_mcep_postfilter_batch_dev(ctx.handle, jobs, len(xs), xs[0].shape[1] - 1, float(alpha),
                                                      int(fft_size), beta_argument(beta),
                                                      None if status is None else status.data_ptr()))


def check_status(status):
    """raise for the non-zero words of a filter's status (host array / device tensor, read back here)"""
    _raise_status([int(s) for s in (status.tolist() if hasattr(status, 'tolist') else status)])
