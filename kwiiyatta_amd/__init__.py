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
           'shift_formants']
