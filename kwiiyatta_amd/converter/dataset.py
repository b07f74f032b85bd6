"""Datasets of the training path: wav directories, parallel pairs, trimming, alignment, and the stacking of a
dataset into the matrix the converter is fitted on.  API of kwiiyatta.converter.dataset
(/root/reference/kwiiyatta/converter/dataset.py).  `kwiiyatta_amd.corpus` is the device-resident counterpart of
this chain for whole corpora; this module is the per-item Python path (and the definition the other is tested
against)."""
import numpy as np

from . import abc

FRAME_EPS = 1e-7        # nnmnkwii: a frame whose L1 norm is below this is "zero"


def _pkg():
    import kwiiyatta_amd
    return kwiiyatta_amd


def _frame_mass(x, eps):
    mass = np.abs(x).sum(axis=1)
    mass[mass < eps] = 0.
    return mass


def trim_zeros_frames(x, eps=FRAME_EPS):
    """nnmnkwii.preprocessing.trim_zeros_frames: the zero frames at BOTH ends are counted off, but the remaining
    length is taken from the FRONT (x[:n]) -- behaviour the reference inherits and documents with a strict xfail
    (tests/kwiiyatta/test_dataset.py:78-99)"""
    return x[:len(np.trim_zeros(_frame_mass(x, eps)))]


def remove_zeros_frames(x, eps=FRAME_EPS):
    """nnmnkwii.preprocessing.remove_zeros_frames: all zero frames are dropped"""
    return x[_frame_mass(x, eps) > 0]


class WavFileDataset(abc.Dataset):
    """the *.wav files of a directory, analysed (lazily) on access; keys are paths relative to the directory"""

    def __init__(self, data_dir, Analyzer=None):
        if not data_dir.exists():
            raise FileNotFoundError(f'wav files dir "{data_dir!s}" is not found')
        if not data_dir.is_dir():
            raise NotADirectoryError(f'wav files dir "{data_dir!s}" is not directory')
        self.data_dir = data_dir
        self.Analyzer = Analyzer or _pkg().analyze_wav
        self.files = frozenset(path.relative_to(data_dir) for path in data_dir.glob('*.wav'))

    def keys(self):
        return self.files

    def get_data(self, key):
        return self.Analyzer(self.data_dir / key)


class ParallelDataset(abc.Dataset):
    """(item of dataset1, item of dataset2) for the keys both have"""

    def __init__(self, dataset1, dataset2):
        self.dataset1, self.dataset2 = dataset1, dataset2
        self.common_keys = dataset1.keys() & dataset2.keys()

    def keys(self):
        return self.common_keys

    def get_data(self, key):
        return self.dataset1[key], self.dataset2[key]


@abc.map_dataset()
def TrimmedDataset(feature):
    """a feature set without its silent end frames (see trim_zeros_frames for which ones exactly)"""
    return feature[:len(trim_zeros_frames(feature.spectrum_envelope))]


@abc.map_dataset(expand_tuple=False)
def AlignedDataset(features, **kwargs):
    """a parallel pair, both sides along their common warping path"""
    return _pkg().align_even(*features, **kwargs)


class PaddedSide:
    """What re-alignment needs of one padded side of a pair, and nothing else: its mel-cepstrum (frames, order + 1) and
    its voicing decision -- no envelopes.  It answers the questions `vocoder.align.make_feature` asks of a feature set"""

    def __init__(self, feature, bands=False):
        record = feature.mel_cepstrum
        self.fs, self.frame_period, self.order = feature.fs, feature.frame_period, record.order
        self.mel_cepstrum_data = np.ascontiguousarray(record.data, dtype=np.float64)
        self.is_voiced = np.array(feature.is_voiced, dtype=bool)
        self.frame_len = len(self.is_voiced)
        # bands=True: also the band track of its aperiodicity (frames, bands + 1), for the band mixture's rows
        self.band_track = _pkg().band_track(feature) if bands else None

    def resample_mel_cepstrum(self, fs):
        if fs != self.fs:
            raise ValueError(f'align_iterations: a side at {self.fs} Hz cannot be re-aligned at {fs} Hz '
                             f'(only its mel-cepstrum at its own sampling rate is kept)')
        return self

    data = property(lambda self: self.mel_cepstrum_data)


class PaddedDataset(abc.MapDataset):
    """a parallel pair with `pad_len` frames of the vocoder's silence around both sides -- drawn ONCE per key, in
    align_even's order (source head, source tail, target head, target tail), when the key is first read.  An
    AlignedDataset on top (with padded=True) therefore gives what one on the unpadded pairs gives, draw for draw.
    `sides[key]` keeps the pair's `PaddedSide`s: later alignments of the same pads (MelCepstrumFeatureConverter
    .train(align_iterations=...)) read those; the padded envelopes themselves are not kept"""
    expand_tuple = False
    with_key = True

    def __init__(self, base, pad_len=100, bands=False):
        super().__init__(base)
        self.pad_len = pad_len
        self.bands = bands           # keep the sides' band tracks too (`PaddedSide.band_track`)
        self.sides = {}

    def function(self, features, key):
        if key in self.sides:
            raise ValueError(f'PaddedDataset: "{key}" was padded before; its pads are drawn once (read `sides`)')
        pad = _pkg().pad_silence
        pair = tuple(pad(f, self.pad_len) for f in features)
        self.sides[key] = tuple(PaddedSide(f, bands=self.bands) for f in pair)
        return pair


def make_dataset_to_array(dataset, keys=None):
    """rows of all items under `keys` (default: all, sorted), zero rows removed; a tuple item contributes its
    members side by side.  None for no keys."""
    blocks = []
    for key in (sorted(dataset.keys()) if keys is None else keys):
        item = dataset[key]
        blocks.append(remove_zeros_frames(np.hstack(item) if isinstance(item, tuple) else item))
    return np.concatenate(blocks) if blocks else None
