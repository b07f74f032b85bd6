"""The options of the device-resident conversion drivers (corpus.convert_batch, resynthesize_batch, evaluate_batch,
ConvertWave), in one record: their names and defaults, the one check of their values on the host, the one upload of what
the kernels read, and the one answer to which of them need the lockstep driver.  (torch is imported where a value is
looked at, not with the module: the commands import it for the names alone.)"""
import inspect
from types import SimpleNamespace

import numpy as np


def filled(options, table):
    """`options` over the defaults of `table`; a name that `table` does not have is a TypeError, as a signature's"""
    for name in options:
        if name not in table:
            raise TypeError(f'got an unexpected keyword argument {name!r}')
    return {**table, **options}


class ConvertOptions:
    """What a driver is asked to do to the utterances it converts, besides converting them (all need the lockstep
    driver; the converter-side ones do nothing without a GMM):

    f0_stats, transpose_key   (mu_src, sigma_src, mu_tgt, sigma_tgt: a 4-tuple or 4 doubles on the device) and / or a
                    key != 0 in semitones: the synthesis runs on the analysed f0 mapped by kwy_f0_map_batch_dev (CheapTrick
                    and D4C keep the analysed track); a frame out of the map's range is a ValueError after the batch.
    gv_stats, gv_strength   gv_strength > 0 (within [0, 1]; gv_stats: the order + 1 values of
                    MelCepstrumFeatureConverter.gv_stats, an array or on the device): the converted mel-cepstra of both
                    outputs through the global-variance postfilter (kwy_column_moments_batch_dev,
                    kwy_gv_postfilter_batch_dev on c1..cN, in place); a coefficient it cannot filter is a ValueError after
                    the batch.
    ms_stats, ms_length, ms_strength   ms_strength > 0 (within [0, 1]; ms_stats: the (G, N) pair of
                    MelCepstrumFeatureConverter.ms_stats, (order + 1, ms_length / 2 + 1, 3) each): the modulation-spectrum
                    postfilter in front of the global-variance one (kwy_ms_postfilter_batch_dev); a bin it cannot filter
                    is a ValueError after the batch, an utterance of more than ms_length frames one before it.
    formant_ratio   a ratio other than 1 (within [0.5, 2]): the envelopes the rendering reads -- the converted ones,
                    without a GMM the analysed ones -- warped along frequency (kwy_formant_shift_dev, one in-place call
                    per wave); the differential outputs are not touched; a row it cannot warp is a ValueError after the
                    batch.
    mlpg_em         None, or N within [0, 16]: both conversions, plain and differential, as EM trajectory conversions over
                    soft mixture posteriors with N re-estimations (kwy_convert_mcep_em_batch_dev) instead of one arg-max
                    mixture per frame.
    mlpg_gv, gv_var, gv_weight   mlpg_gv None, or N within [0, 256], with gv_stats and gv_var (the converter's): both
                    conversions with the GV ascent behind them (kwy_convert_mcep_gv_batch_dev; N conjugate-gradient steps,
                    gv_weight weighs the GV term), the differential one on the variance of differential + source.  It goes
                    with mlpg_em, not with gv_strength or ms_strength; a coefficient it cannot process is a ValueError
                    after the batch.
    diff_filter     (with diff=True) 'mlsa', the MLSA recursions -- which wait for the last wave of a batch and run side
                    by side, one wavefront per file --, or 'fft': the frame-parallel FFT form of the differential filter
                    (kwy_mcep_filter_fft_batch_dev, one grid over all frames of a wave's files, launched with the wave).
    postfilter_beta, keep_power   beta > 0 (within [0, 1]) and / or keep_power: the absolute converted mel-cepstra through
                    kwy_mcep_postfilter_batch_dev after every other filter -- the formant emphasis, c0 shifted to the
                    energy of the source frame (keep_power) or of the unfiltered converted frame; the differential filters
                    then take c0 into account (ignore_c0 = 0: column 0 of the coefficients is the change of c0).  A frame
                    whose energy is unusable is a ValueError after the batch."""

    DEFAULTS = dict(f0_stats=None, transpose_key=0.0, gv_stats=None, gv_strength=0.0, ms_stats=None, ms_length=None,
                    ms_strength=0.0, formant_ratio=1.0, mlpg_em=None, mlpg_gv=None, gv_var=None, gv_weight=1.0,
                    diff_filter='mlsa', postfilter_beta=0.0, keep_power=False)

    def __init__(self, only=None, **options):
        """only: the part of DEFAULTS a driver takes, when it does not take them all"""
        self.__dict__.update(self.DEFAULTS, **filled(options, only or self.DEFAULTS))

    def check(self, order, converting=True):
        """every check of the values, on the host, before anything is put on a device: -> self.  converting=False (no
        GMM): the converter-side options are off and only their ranges are checked"""
        from .backend import formant
        from .filter import DIFF_FILTERS
        if self.diff_filter not in DIFF_FILTERS:
            raise ValueError(f'differential filter: {self.diff_filter!r} is not one of {DIFF_FILTERS}')
        self.postfilter_beta, self.keep_power = float(self.postfilter_beta), bool(self.keep_power)
        if not 0.0 <= self.postfilter_beta <= 1.0:
            raise ValueError(f'postfilter: beta {self.postfilter_beta!r} is outside [0, 1]')
        self.formant_ratio = formant.check_ratio(self.formant_ratio)
        if converting and self.mlpg_em is not None:
            if isinstance(self.mlpg_em, bool) or int(self.mlpg_em) != self.mlpg_em or not 0 <= self.mlpg_em <= 16:
                raise ValueError(f'mlpg_em must be None or an integer within [0, 16], not {self.mlpg_em!r}')     # (KWY_MLPG_EM_MAX)
            self.mlpg_em = int(self.mlpg_em)
        self._ascent = self._check_ascent(order) if converting and self.mlpg_gv is not None else None
        if not 0.0 <= float(self.gv_strength) <= 1.0:
            raise ValueError(f'global variance: strength {self.gv_strength!r} is outside [0, 1]')
        if converting and self.gv_strength > 0:
            if self.gv_stats is None:
                raise ValueError('global variance: gv_strength > 0 needs gv_stats')
            if _shape(self.gv_stats) != (order + 1,) or not _is_f64(self.gv_stats):
                raise ValueError(f'global variance: gv_stats must be {order + 1} float64 values')
        if not 0.0 <= float(self.ms_strength) <= 1.0:
            raise ValueError(f'modulation spectrum: strength {self.ms_strength!r} is outside [0, 1]')
        if converting and self.ms_strength > 0:
            if self.ms_stats is None or len(self.ms_stats) != 2:
                raise ValueError('modulation spectrum: ms_strength > 0 needs ms_stats, the (G, N) pair of a trained converter')
            first = _shape(self.ms_stats[0])
            length = 2 * (first[1] - 1) if len(first) == 3 else None
            if self.ms_length is not None and int(self.ms_length) != length:
                raise ValueError(f'modulation spectrum: ms_stats are of length {length}, not ms_length = {self.ms_length}')
            for v in self.ms_stats:
                if _shape(v) != (order + 1, (length or 0) // 2 + 1, 3) or not _is_f64(v):
                    raise ValueError(f'modulation spectrum: ms_stats must be two ({order + 1}, L/2 + 1, 3) float64 arrays')
        return self

    def _check_ascent(self, order):
        """-> (mean, var, iterations, weight) of the GV ascent: the statistics of c1..cN as host arrays"""
        import torch
        from .backend import gv as gvgen
        if self.gv_strength:
            raise ValueError('mlpg_gv does not go with gv_strength > 0: the postfilter would repair the same variance twice')
        if self.ms_strength:
            raise ValueError('mlpg_gv does not go with ms_strength > 0: composing it with the modulation-spectrum filter is '
                             'left for later')
        if self.gv_stats is None or self.gv_var is None:
            raise ValueError('mlpg_gv needs gv_stats and gv_var (retrain the converter with gv_stats=True on two or more '
                             'utterances)')
        host = [v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)
                for v in (self.gv_stats, self.gv_var)]
        if any(v.shape != (order + 1,) for v in host):
            raise ValueError(f'mlpg_gv: gv_stats and gv_var must be {order + 1} float64 values each')
        if not (host[1][1:] > 0).all():
            raise ValueError('mlpg_gv: the variance of the global variance is not positive everywhere (retrain the '
                             'converter with gv_stats=True on two or more utterances)')
        return gvgen.ascent_arguments(np.ascontiguousarray(host[0][1:]), np.ascontiguousarray(host[1][1:]), self.mlpg_gv,
                                      self.gv_weight, order)

    def upload(self, dev, converting=True):
        """(after `check`) what the kernels read, put on `dev` once per batch: -> the resolved options, which every wave
        takes as they are.  f0_stats: 4 doubles or None; f0_map: whether the f0 is mapped; gv: the order + 1 statistics or
        None (no filter); ms: the (G, N) pair or None; gvgen: None or dict(iterations, weight, mean, var) of the GV
        ascent, the statistics those of c1..cN; power: whether kwy_mcep_postfilter_batch_dev runs; the scalars as
        checked.  converting=False (no GMM): every converter-side option is off"""
        import torch
        from ._blocks import to_device

        put = lambda v: to_device(v, dev, dtype=np.float64).to(dev)  # noqa: E731 (.to: a tensor may come from the host)
        stats, ascent = self.f0_stats, self._ascent if converting else None
        return SimpleNamespace(
            transpose_key=float(self.transpose_key), f0_map=stats is not None or float(self.transpose_key) != 0,
            f0_stats=None if stats is None else torch.as_tensor(stats if torch.is_tensor(stats) else list(stats),
                                                                dtype=torch.float64, device=dev),
            gv_strength=float(self.gv_strength), gv=put(self.gv_stats) if converting and self.gv_strength > 0 else None,
            ms_strength=float(self.ms_strength),
            ms=tuple(put(v).contiguous() for v in self.ms_stats) if converting and self.ms_strength > 0 else None,
            formant_ratio=self.formant_ratio, diff_filter=self.diff_filter, mlpg_em=self.mlpg_em if converting else None,
            postfilter_beta=self.postfilter_beta, keep_power=self.keep_power,
            power=converting and (self.postfilter_beta > 0 or self.keep_power),
            gvgen=None if ascent is None else dict(iterations=ascent[2], weight=ascent[3], mean=put(ascent[0]),
                                                   var=put(ascent[1])))

    def need_lockstep(self):
        """the active options that only the lockstep driver knows, each as the opening of a driver's rejection:
        '<who>: <this> the lockstep driver'"""
        asked = (('postfilter_beta and keep_power need', self.postfilter_beta or self.keep_power),
                 ('formant_ratio needs', self.formant_ratio != 1),
                 ('mlpg_gv needs', self.mlpg_gv is not None),
                 ('f0_stats and transpose_key need', self.f0_stats is not None or self.transpose_key != 0),
                 ('gv_stats and gv_strength need', self.gv_stats is not None or self.gv_strength != 0),
                 ('ms_stats and ms_strength need', self.ms_stats is not None or self.ms_strength != 0),
                 ('mlpg_em needs', self.mlpg_em is not None))
        return [what for what, on in asked if on]


def _shape(v):
    return tuple(v.shape) if hasattr(v, 'data_ptr') else np.asarray(v).shape


def _is_f64(v):
    return str(v.dtype) == 'torch.float64' if hasattr(v, 'data_ptr') else True       # (an array is converted on its way up)


def takes_options(defaults=ConvertOptions.DEFAULTS):
    """marks fn(..., **options) as taking ConvertOptions' keywords (defaults: a part of them, or another table of names
    and defaults): help() and inspect.signature show them, keyword-only, with the table's defaults"""
    def mark(fn):
        sig = inspect.signature(fn)
        own = [q for q in sig.parameters.values() if q.kind is not inspect.Parameter.VAR_KEYWORD]
        fn.__signature__ = sig.replace(parameters=own + [
            inspect.Parameter(name, inspect.Parameter.KEYWORD_ONLY, default=default)
            for name, default in defaults.items()])
        return fn
    return mark
