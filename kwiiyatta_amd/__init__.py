"""kwiiyatta_amd -- MI355X-native implementation of kwiiyatta's per-utterance
conversion hot path (WORLD analysis, mel-cepstrum, FastDTW alignment, GMM/MLPG
conversion, WORLD synthesis) behind the reference's own Python API
(same export list as /root/reference/kwiiyatta/__init__.py:1-22; the host-side
feature model, converter stack and CLIs are this package's own code written
to that API).

The numerics run in hand-written gfx950 HIP kernels (``libkwy.so``, C ABI in
``include/kwy.h``) reached through the pyworld / pysptk / fastdtw / nnmnkwii
shaped modules in ``kwiiyatta_amd.backend``; there is no CPU fallback.
"""
from . import wavfile
from .wavfile import Wavdata, load_wav
from .vocoder import (Analyzer, Feature, MelCepstrum, Synthesizer, align_even, analyze_wav,
                      feature, pad_silence, resample, reshape)
from .converter import MelCepstrumConverter, ParallelDataset, WavFileDataset, align_dataset
from .filter import apply_diff_filter, apply_mlsa_filter
from .align import align
from .config import Config
from .evaluate_voice import evaluate, evaluate_pair


def shift_pitch(wavdata, rate):
    """a new Wavdata of the same length and sampling rate whose pitch is `rate` (within [0.5, 2.0]) times the
    input's: a WSOLA time stretch resampled back to the input's length (backend.pitch, kwy_pitch.hip)"""
    import numpy as np
    from .backend import pitch
    return Wavdata(wavdata.fs, pitch.shift_pitch(np.ascontiguousarray(wavdata.data, dtype=np.float64), wavdata.fs, rate))


def shift_formants(feature_set, ratio):
    """a materialised copy of the feature set whose formants are `ratio` (within [0.5, 2.0]) times the input's: the
    spectral envelope warped along frequency (MutableFeature.shift_formants, backend.formant, kwy_formant.hip); f0 and
    aperiodicity are the input's"""
    warped = feature(feature_set)
    warped.shift_formants(ratio)
    return warped


def mcep_energy(mcep):
    """the energy of every frame of a MelCepstrum record: the mean of |H|^2 over the vocoder's transform length at its
    sampling rate, without the spectrum (backend.power, kwy_mcpower.hip); one double per frame"""
    import numpy as np
    from .backend import power
    return power.frame_energy(np.ascontiguousarray(mcep.data, dtype=np.float64), mcep.alpha(),
                              power.energy_fft_size(mcep.fs))


def postfilter_mcep(mcep, beta=0.0, power_of=None):
    """a new MelCepstrum: `mcep` through the mel-cepstral formant emphasis of strength beta (within [0, 1]), every
    frame's c0 shifted until the frame has the energy of the same frame of `power_of` (a MelCepstrum of the same shape
    and rate; default: of `mcep` itself, which the emphasis alone would make louder)"""
    import numpy as np
    from .backend import power
    if power_of is not None and (power_of.fs != mcep.fs or np.shape(power_of.data) != np.shape(mcep.data)):
        raise ValueError('postfilter_mcep: power_of must have the sampling rate and the shape of mcep')
    ref = None if power_of is None else np.ascontiguousarray(power_of.data, dtype=np.float64)
    data = power.postfilter(np.ascontiguousarray(mcep.data, dtype=np.float64), beta, ref=ref, alpha=mcep.alpha(),
                            fft_size=power.energy_fft_size(mcep.fs))
    return MelCepstrum(mcep.fs, mcep.frame_period, data)


def band_track(feature_or_ap, fs=None):
    """the band track (frames, B + 1) of a feature set's aperiodicity, or of an aperiodicity matrix (frames, bins) at
    the sampling rate `fs` (a feature set brings its own): column 0 the voicing flag of the band codec's decoder,
    columns 1..B the coded bands in dB, unvoiced frames holding the row of the nearest voiced frame (backend.bap,
    kwy_bap.hip) -- what the converter's band mixture is trained on and converts.  ValueError below 12 kHz"""
    import numpy as np
    from .backend import bap
    if hasattr(feature_or_ap, 'aperiodicity'):
        if fs is not None and fs != feature_or_ap.fs:
            raise ValueError(f'band_track: the feature set is at {feature_or_ap.fs} Hz, not at {fs} Hz')
        fs = feature_or_ap.fs
        bap.check_rate(fs)
        feature_or_ap = feature_or_ap.aperiodicity
    elif fs is None:
        raise ValueError('band_track: an aperiodicity matrix needs its sampling rate')
    bap.check_rate(fs)
    return bap.track(np.ascontiguousarray(feature_or_ap, dtype=np.float64), fs)


name = "kwiiyatta_amd"

__all__ = ['align', 'Config', 'MelCepstrumConverter', 'ParallelDataset', 'WavFileDataset',
           'align_dataset', 'apply_mlsa_filter', 'apply_diff_filter', 'Analyzer', 'Feature', 'MelCepstrum',
           'Synthesizer', 'align_even', 'analyze_wav', 'feature', 'pad_silence', 'resample',
           'reshape', 'Wavdata', 'load_wav',
           # additions to the reference's names: objective evaluation of a trained converter (evaluate_voice.py)
           'evaluate_pair', 'evaluate',
           # ... and the waveform pitch shifter in front of a differential conversion across genders (backend/pitch.py)
           'shift_pitch',
           # ... and the formant shift beside it: the envelope of a feature set warped along frequency (backend/formant.py)
           'shift_formants',
           # ... and the energy of a mel-cepstrum with the postfilter that renormalises by it (backend/power.py)
           'mcep_energy', 'postfilter_mcep',
           # ... and the band track the aperiodicity conversion works on (backend/bap.py)
           'band_track']
