"""Converter layer: datasets of the training path and the converter stack
(mel-cepstrum stage > delta stage > joint GMM).  Export list of kwiiyatta.converter."""
from . import abc
from .dataset import (AlignedDataset, PaddedDataset, ParallelDataset, TrimmedDataset, WavFileDataset,
                      make_dataset_to_array)
from .delta import DELTA_WINDOWS, DeltaFeatureConverter, DeltaFeatureDataset
from .exemplar import ExemplarFeatureConverter
from .gmm import GMMFeatureConverter
from .mcep import MelCepstrumDataset, MelCepstrumFeatureConverter


CONVERTERS = ('gmm', 'exemplar')


def MelCepstrumConverter(use_delta=True, mcep_fs=None, Converter=GMMFeatureConverter, converter='gmm', exemplars=None,
                         exemplar_iterations=None, exemplar_sparsity=None, exemplar_fft=None, **kwargs):
    """the stack the CLIs use; kwargs go to the innermost converter.
    converter='exemplar' (an addition): the exemplar converter in the place of delta stage and mixture
    (converter.exemplar; `exemplars` atoms at the most, `exemplar_iterations` activation updates of sparsity
    `exemplar_sparsity` on `exemplar_fft` / 2 + 1 bins, None: its defaults).  It has no dynamic features, no
    components and no random state: use_delta, components, max_iter and random_state are ignored, any other keyword of
    the mixture is a TypeError."""
    if converter not in CONVERTERS:
        raise ValueError(f'converter must be one of {CONVERTERS}, not {converter!r}')
    if converter == 'exemplar':
        unknown = sorted(set(kwargs) - {'components', 'max_iter', 'random_state'})
        if unknown:
            raise TypeError(f'the exemplar converter takes no {", ".join(unknown)}')
        return MelCepstrumFeatureConverter(ExemplarFeatureConverter(
            exemplars=exemplars, iterations=exemplar_iterations, sparsity=exemplar_sparsity, fft=exemplar_fft),
            mcep_fs=mcep_fs)
    given = {name: v for name, v in dict(exemplars=exemplars, exemplar_iterations=exemplar_iterations,
                                         exemplar_sparsity=exemplar_sparsity, exemplar_fft=exemplar_fft).items()
             if v is not None}
    if given:
        raise TypeError(f'{", ".join(sorted(given))}: options of converter=\'exemplar\'')
    stack = Converter(**kwargs)
    if use_delta:
        stack = DeltaFeatureConverter(stack)
    return MelCepstrumFeatureConverter(stack, mcep_fs=mcep_fs)


def align_dataset(parallel_dataset):
    """a parallel dataset -> trimmed and aligned pairs (the training set of the converter)"""
    return AlignedDataset(TrimmedDataset(parallel_dataset))


__all__ = ['MelCepstrumConverter', 'align_dataset', 'AlignedDataset', 'ParallelDataset', 'TrimmedDataset',
           'WavFileDataset', 'PaddedDataset', 'make_dataset_to_array', 'GMMFeatureConverter', 'ExemplarFeatureConverter', 'DELTA_WINDOWS',
           'DeltaFeatureConverter', 'DeltaFeatureDataset', 'MelCepstrumDataset', 'MelCepstrumFeatureConverter']
