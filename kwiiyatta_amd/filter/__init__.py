"""Differential-spectrum filtering: a waveform is passed through the MLSA filter described by a mel-cepstrum (for
voice conversion: the difference between target and source mel-cepstra), which changes its spectral envelope
without re-synthesising it.  API of kwiiyatta.filter (/root/reference/kwiiyatta/filter/mlsa.py:9-30).  mc2b and the
filter itself are HIP kernels behind the pysptk-shaped classes of kwiiyatta_amd.backend.sptk.
`apply_diff_filter(wav, mcep, method=)` chooses between that filter ('mlsa', serial in the sample) and the
frame-parallel FFT form of the same mel-cepstral filter ('fft', backend.fftfilt)."""
import numpy as np

from ..backend import sptk

DIFF_FILTERS = ('mlsa', 'fft')


def _at_waveform_rate(mcep, fs):
    """the mel-cepstrum re-expressed at the waveform's sampling rate"""
    import kwiiyatta_amd as k
    if mcep.fs > fs:
        return k.resample(mcep, fs)
    if mcep.fs == fs:
        return mcep
    # lower rate: its spectrum covers only the lower band of the waveform's; the band above is held at the level of
    # the last bin the mel-cepstrum knows about (a flat continuation of the filter's gain)
    wide = k.Synthesizer.resample_spectrum_envelope(mcep.extract_spectrum(), mcep.fs, fs)
    known = mcep.fs * wide.shape[1] // fs
    wide[:, known:] = wide[:, known - 1:known]
    out = k.MelCepstrum(fs, mcep.frame_period)
    out.extract(wide)
    return out


def _shape_only(wav, mcep, use_c0=False):
    """what both filters run on: the mel-cepstrum at the waveform's rate, its coefficients with c0 = 0 (the filter
    changes the envelope's shape, not its power) unless use_c0, alpha and the hop in samples"""
    mcep = _at_waveform_rate(mcep, wav.fs)
    shape_only = np.array(mcep.data, dtype=np.float64)
    if not use_c0:
        shape_only[:, 0] = 0.0
    return mcep, shape_only, mcep.alpha(), int(mcep.fs * (mcep.frame_period * 0.001))


def apply_mlsa_filter(wav, mcep, use_c0=False):
    """`wav` (Wavdata or anything with .fs / .data) filtered frame by frame with `mcep` (c0 ignored; with use_c0
    column 0 takes part: the filter scales its input by exp(b0), which is how a differential c0 -- the power correction
    of converter.convert(diff=True, keep_power=True) -- reaches the waveform)"""
    import kwiiyatta_amd as k
    mcep, shape_only, alpha, hop = _shape_only(wav, mcep, use_c0)
    engine = sptk.Synthesizer(sptk.MLSADF(order=mcep.order, alpha=alpha), hopsize=hop)
    return k.Wavdata(wav.fs, engine.synthesis(wav.data, sptk.mc2b(shape_only, alpha=alpha)))


def apply_diff_filter(wav, mcep, method='mlsa', use_c0=False):
    """`wav` through the differential filter of `mcep` (c0 ignored unless use_c0): method 'mlsa' is apply_mlsa_filter;
    'fft' filters every frame through the frequency response of its mel-cepstrum and crossfades the outputs of
    neighbouring frames' filters where the MLSA filter interpolates their coefficients -- all frames at once instead of
    sample by sample"""
    if method not in DIFF_FILTERS:
        raise ValueError(f'differential filter: {method!r} is not one of {DIFF_FILTERS}')
    if method == 'mlsa':
        return apply_mlsa_filter(wav, mcep, use_c0=True) if use_c0 else apply_mlsa_filter(wav, mcep)
    import kwiiyatta_amd as k
    from ..backend import fftfilt
    mcep, shape_only, alpha, hop = _shape_only(wav, mcep, use_c0)
    size = fftfilt.fft_filter_size(wav.fs, hop)
    return k.Wavdata(wav.fs, fftfilt.mcep_fft_filter(wav.data, shape_only, alpha, hop, size, ignore_c0=not use_c0))


__all__ = ['apply_mlsa_filter', 'apply_diff_filter']
