"""Mel-cepstrum stage of the converter stack: feature sets become coefficient matrices c1..cN at one common order
and sampling rate for training; at conversion the power coefficient c0 is set aside and re-attached.  API of
kwiiyatta.converter.mcep (/root/reference/kwiiyatta/converter/mcep.py)."""
import copy

import numpy as np

from . import abc


def _pkg():
    import kwiiyatta_amd
    return kwiiyatta_amd


class MelCepstrumDataset(abc.MapDataset):
    """c1..cN of every item.  The first item fixes the order and (unless `mcep_fs` is given) the sampling rate;
    later items are truncated / resampled to them."""
    with_key = True

    def __init__(self, base, mcep_fs=None):
        super().__init__(base)
        self.fs, self.order = mcep_fs, None

    def function(self, feature, key):
        snap = _pkg().feature(feature)
        if self.order is None:
            self.order = snap.mel_cepstrum_order
        if self.fs is None:
            self.fs = snap.fs
        snap.mel_cepstrum_order = self.order
        record = snap.mel_cepstrum if snap.fs == self.fs else snap.resample_mel_cepstrum(self.fs)
        return record.data[:, 1:]


def _trimmed_stage(dataset):
    """the TrimmedDataset of the dataset's chain (the dataset itself when its chain has none)"""
    from .dataset import TrimmedDataset
    stage = dataset
    while not isinstance(stage, TrimmedDataset) and isinstance(stage, abc.MapDataset):
        stage = stage.base
    return stage if isinstance(stage, TrimmedDataset) else dataset


def _f0_tracks(dataset, keys):
    """(source tracks, target tracks) of `keys` in sorted order: the f0 of the frames TrimmedDataset keeps, before
    alignment (the items of the dataset itself when its chain has no TrimmedDataset)"""
    stage = _trimmed_stage(dataset)
    sides = ([], [])
    for key in sorted(keys):
        for side, feature in zip(sides, stage[key]):
            side.append(np.ascontiguousarray(feature.f0, dtype=np.float64))
    return sides


def _side_mel_cepstra(dataset, keys, order, fs, side):
    """one side's (0: source, 1: target) MelCepstrum records of `keys` in sorted order, at the given order and sampling
    rate: the frames `_f0_tracks` takes, c0 included"""
    stage = _trimmed_stage(dataset)
    records = []
    for key in sorted(keys):
        snap = _pkg().feature(stage[key][side])
        snap.mel_cepstrum_order = order
        records.append(snap.mel_cepstrum if snap.fs == fs else snap.resample_mel_cepstrum(fs))
    return records


def _target_mel_cepstra(dataset, keys, order, fs):
    """the target side's mel-cepstra (frames, order + 1) of `keys` in sorted order"""
    return [np.ascontiguousarray(r.data, dtype=np.float64) for r in _side_mel_cepstra(dataset, keys, order, fs, 1)]


class MelCepstrumFeatureConverter(abc.MapFeatureConverter):
    def __init__(self, base, mcep_fs=None):
        super().__init__(base)
        self.mcep_fs = mcep_fs
        self.f0_stats = None
        self.gv_stats = None
        self.gv_var = None
        self.ms_stats, self.ms_length = None, None
        # the pitch ratio the source waveforms were (and are to be) shifted by before analysis (backend.pitch): set by
        # whoever prepares the training set (Config.train_converter), kept in the model file; 1: no shift
        self.source_f0_rate = 1.0
        # the re-alignment passes the training ran (`train(align_iterations=...)`) and its record, a dict per fit
        self.align_iterations = 0
        self.align_history = []
        # the band-aperiodicity stack (`train(ap_model=True)`: delta stage > joint GMM on the band rows of the aligned
        # pairs, used by `convert_aperiodicity`) and the rows its fit saw; None / 0 without one
        self.ap_converter = None
        self.ap_rows = 0
        # the INCA iterations of a non-parallel training (`train_nonparallel(iterations=...)`; None: trained on
        # parallel data) and its record, a dict per fit
        self.nonparallel = None
        self.nonparallel_history = []
        # the f0 estimator behind the training set's tracks ('dio' or 'pyin': the voicing term of the alignment and the
        # f0 statistics were learnt on them): set by whoever prepares the training set, kept in the model file
        self.f0_estimator = 'dio'

    def train(self, dataset, keys, f0_stats=False, gv_stats=False, align_iterations=0, ms_stats=False, ms_length=4096,
              ap_model=False, ap_components=16, **kwargs):
        """f0_stats=True: also the voiced log-f0 statistics of both sides (`f0_stats`, used by `convert_f0`).
        gv_stats=True: also the target side's global variance (`gv_stats`, order + 1 values: per coefficient the mean
        over the training utterances of its variance within the utterance; used by `convert(gv=...)`) and `gv_var`, the
        variance over the training utterances of the same quantity (0 everywhere when trained on one utterance; used,
        with `gv_stats`, by `convert(mlpg_gv=...)`).
        align_iterations=N > 0: iterative re-alignment of the training set, see `_train_realigned`
        ms_stats=True: also the modulation-spectrum statistics (`ms_stats` = (G, N), each (order + 1, ms_length / 2 + 1,
        3): per coefficient and modulation-frequency bin the count, mean and M2 over the training utterances of the log
        modulation spectrum -- N of the target side's mel-cepstra, G of the source side's converted by the mixture just
        fitted (`convert(..., diff=False)`); used by `convert(ms=...)`).  ms_length: the transform length, which no
        utterance may exceed (`ms_length`)
        ap_model=True: also a mixture of `ap_components` components (the converter's covariance structure, random
        state and stopping rule) on the band aperiodicity of the same aligned pairs (`ap_converter`, used by
        `convert_aperiodicity`; include/kwy.h, "aperiodicity conversion"): the rows pair the two sides' band tracks along
        the kept cells that are voiced on both sides -- with align_iterations > 0 along the LAST alignment.  It takes the
        padded-pair path of the re-alignment for any align_iterations (an aligned dataset that pads its pairs itself,
        both sides at the converter's sampling rate, which must be 12 kHz or more: ValueError otherwise)"""
        if isinstance(align_iterations, bool) or int(align_iterations) != align_iterations or align_iterations < 0:
            raise ValueError(f'align_iterations must be a non-negative integer, not {align_iterations!r}')
        self.align_iterations, self.align_history = int(align_iterations), []
        self.nonparallel, self.nonparallel_history = None, []
        if ms_stats:
            self._check_ms_lengths(dataset, keys, ms_length)          # (before the fit is paid for)
        self.ap_converter, self.ap_rows = None, 0
        if ap_model:
            if isinstance(ap_components, bool) or int(ap_components) != ap_components or ap_components < 1:
                raise ValueError(f'ap_components must be a positive integer, not {ap_components!r}')
            if self.mcep_fs is not None:
                from ..backend import bap
                bap.check_rate(self.mcep_fs)                           # (before a file is read)
        if self.align_iterations > 0 or ap_model:
            self._train_realigned(dataset, list(keys), self.align_iterations, kwargs,
                                  ap_components=int(ap_components) if ap_model else None)
        else:
            coefficients = MelCepstrumDataset(dataset, mcep_fs=self.mcep_fs)
            self.base.train(coefficients, keys, **kwargs)
            self.order, self.fs = coefficients.order, coefficients.fs
            self._bind_rate()
        self.f0_stats = None
        if f0_stats:
            from ..backend import f0 as f0map
            source, target = _f0_tracks(dataset, keys)
            if not source:
                raise ValueError('f0 statistics: no training files')
            self.f0_stats = f0map.stats_from_moments(f0map.merge_moments(f0map.logf0_moments(source)),
                                                     f0map.merge_moments(f0map.logf0_moments(target)))
        self.gv_stats, self.gv_var = None, None
        if gv_stats:
            from ..backend import gv as gvfilter
            mats = _target_mel_cepstra(dataset, keys, self.order, self.fs)
            if not mats:
                raise ValueError('global variance statistics: no training files')
            moments = gvfilter.column_moments(mats)
            self.gv_stats = gvfilter.gv_from_moments(moments)
            self.gv_var = gvfilter.gv_statistics(moments)[1]
        self.ms_stats, self.ms_length = None, None
        if ms_stats:
            self._train_ms(dataset, keys, ms_length)

    @staticmethod
    def _check_ms_lengths(dataset, keys, length):
        """what the modulation-spectrum statistics need of the training set, as far as frame counts tell: no utterance
        of either side longer than the transform (the converted source has the source's frames), two of two frames"""
        from ..backend import ms as msfilter
        stage = _trimmed_stage(dataset)
        usable = 0
        for key in sorted(keys):
            frames = [len(feature.f0) for feature in stage[key]]
            msfilter._fits(frames, msfilter._length(length))
            usable += min(frames) >= 2
        if usable < 2:
            raise ValueError('modulation spectrum statistics: fewer than two usable training utterances (of at least '
                             'two frames)')

    def _train_ms(self, dataset, keys, length):
        self._train_ms_sides(lambda: _side_mel_cepstra(dataset, keys, self.order, self.fs, 0),
                             _target_mel_cepstra(dataset, keys, self.order, self.fs), length)

    def _train_ms_sides(self, sources, natural, length):
        """sources: a callable that gives the source side's MelCepstrum records (called after the target's statistics
        are made); natural: the target side's (frames, order + 1) matrices"""
        from ..backend import ms as msfilter
        as_f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        if not natural:
            raise ValueError('modulation spectrum statistics: no training files')
        stats_n = msfilter.statistics(natural, length)
        converted = [as_f64(self.convert(source, diff=False).data) for source in sources()]
        stats_g = msfilter.statistics(converted, length)
        for name, stats in (('target', stats_n), ('converted source', stats_g)):
            if stats[1:, 1:, 0].min() < 2:
                raise ValueError(f'modulation spectrum statistics: fewer than two usable {name} utterances (of at least '
                                 f'two frames and with every coefficient varying)')
        self.ms_stats, self.ms_length = (stats_g, stats_n), int(length)

    def _band_stack(self, components):
        """an untrained band stack: delta stage > joint GMM of `components` components with this converter's covariance
        structure, random state and iteration limit"""
        from .delta import DeltaFeatureConverter
        from .gmm import GMMFeatureConverter
        main = self.gmm
        return DeltaFeatureConverter(GMMFeatureConverter(
            components=components, max_iter=getattr(main, 'max_iter', 100), random_state=getattr(main, 'random_state', None),
            covariance=getattr(main, 'covariance_structure', 'full')))

    def convert_aperiodicity(self, feature):
        """the aperiodicity (frames, bins) for synthesising a converted voice: a copy of the feature set's whose voiced
        frames are the decode of its band track converted by the band mixture (arg-max MLPG, no EM / GV / MS; the bands
        clamped to [-60, -1e-12] dB); unvoiced frames are the feature set's own.  The feature set must be at the
        converter's sampling rate and frame period"""
        from ..backend import bap
        ap = np.array(feature.aperiodicity, dtype=np.float64, order='C')
        if not len(ap):
            return ap
        source, converted = self.convert_band_track(feature, ap=ap)
        return bap.apply(source, converted, ap, self.fs)

    def convert_band_track(self, feature, ap=None):
        """(the band track of the feature set's aperiodicity, the converted band track): (frames, B + 1) each, column 0
        -- the voicing flag -- the same in both, the converted bands clamped to [-60, -1e-12] dB"""
        from ..backend import bap
        if self.ap_converter is None:
            raise ValueError('convert_aperiodicity: the converter has no band mixture (train it with ap_model=True)')
        if feature.fs != self.fs:
            raise ValueError(f'convert_aperiodicity: the feature set is at {feature.fs} Hz, the converter at {self.fs} Hz')
        B = bap.check_rate(self.fs)
        if self.ap_converter.gmm.means_.shape[1] != 6 * B:
            raise ValueError(f'convert_aperiodicity: the band mixture does not have the {B} band(s) of {self.fs} Hz')
        if ap is None:
            ap = np.ascontiguousarray(feature.aperiodicity, dtype=np.float64)
        source = bap.track(ap, self.fs)
        bands = self.ap_converter.convert(np.ascontiguousarray(source[:, 1:]), raw=feature, diff=False)
        return source, np.ascontiguousarray(np.hstack((source[:, :1], bap.clamp(bands))), dtype=np.float64)

    def _train_realigned(self, dataset, keys, iterations, fit_options, ap_components=None):
        """Iterative re-alignment of the training set (Toda et al.'s joint-feature iterations): fit 0 is the training
        of align_iterations=0 on the same rows -- every pair trimmed, padded (the pads are drawn ONCE, here, in
        today's order) and aligned on the two speakers' own DTW features.  Then, `iterations` times over, every pair
        is aligned again: the same padded pair, the source's DTW features carrying its mel-cepstrum CONVERTED by the
        mixture fitted last (`convert(..., diff=False)`: deltas, mixture, MLPG; no GV, no f0) in columns 2.. while its
        power and voicing terms stay its own; the joint rows pair the ORIGINAL source coefficients with the target's
        along the new path, and the mixture is fitted on them from scratch (same components, random_state, stopping
        rule).  `align_history` gets one record per fit: rows, em_iterations and mcd, the monitor -- the mean
        distortion in dB over c1..cN, along the kept path of all pairs, between the target and the source coefficients
        the path was found with (fit 0: the source's own; fit k: converted by fit k - 1).
        The dataset must be an AlignedDataset chain with silence pads; pairs whose alignment would not run at the
        converter's sampling rate raise ValueError (nothing is resampled here)."""
        from ..backend import bap, distortion as dist
        from ..backend.mlpg import DELTA_WINDOWS, delta_features
        from ..vocoder.align import even_indices
        from .dataset import AlignedDataset, PaddedDataset, remove_zeros_frames
        from .delta import DeltaFeatureConverter
        stage = dataset
        while not isinstance(stage, AlignedDataset) and isinstance(stage, abc.MapDataset):
            stage = stage.base
        who = 'align_iterations > 0' if iterations > 0 else 'ap_model=True'     # (whichever brought the caller here)
        if not isinstance(stage, AlignedDataset):
            raise ValueError(f'{who} needs an aligned dataset (kwiiyatta_amd.align / align_dataset)')
        options = dict(stage.kwargs)
        if not options.pop('pad_silence', True) or options.pop('padded', False):
            raise ValueError(f'{who} needs an alignment that pads its pairs with silence itself')
        padded = PaddedDataset(stage.base, pad_len=options.pop('pad_len', 100), bands=ap_components is not None)
        delta_stage = self.base
        while not isinstance(delta_stage, DeltaFeatureConverter) and isinstance(delta_stage, abc.MapFeatureConverter):
            delta_stage = delta_stage.base
        if not isinstance(delta_stage, DeltaFeatureConverter):
            delta_stage = None
        k = _pkg()
        self.order, self.fs = None, self.mcep_fs
        for it in range(iterations + 1):
            blocks, triples, band_blocks = [], [], []
            for key in keys:
                if it == 0:
                    padded[key]                      # draws the pair's pads and keeps its `sides`
                x, y = padded.sides[key]
                if it == 0:
                    if self.order is None:
                        self.order = x.order
                    if self.fs is None:
                        self.fs = x.fs
                    if x.order != self.order or y.order != self.order:
                        raise ValueError(f'align_iterations: "{key}" has mel-cepstra of order {x.order} and {y.order}, '
                                         f'the converter of order {self.order}')
                    if ap_components is not None and key == keys[0]:
                        bap.check_rate(self.fs)
                    if not x.fs == y.fs == self.fs:
                        raise ValueError(f'align_iterations: "{key}" is aligned at {min(x.fs, y.fs)} Hz (source {x.fs} Hz, '
                                         f'target {y.fs} Hz) but the converter works at {self.fs} Hz; re-alignment does '
                                         f'not resample')
                    if delta_stage is not None:
                        if key == keys[0]:
                            delta_stage.frame_period = x.frame_period
                        for side in (x, y):
                            if side.frame_period != delta_stage.frame_period:
                                raise ValueError(f'frame_period of "{key}" is {side.frame_period!r} but others are '
                                                 f'{delta_stage.frame_period!r}')
                    mapped = x.data
                else:
                    source = k.MelCepstrum(x.fs, x.frame_period, x.data)
                    mapped = np.ascontiguousarray(self.convert(source, diff=False).data, dtype=np.float64)
                xs, ys = even_indices(x, y, padded.pad_len, **options,
                                      **({} if it == 0 else dict(x_mapped=mapped[:, 1:])))
                sides = [np.ascontiguousarray(side.data[idx][:, 1:]) for side, idx in ((x, xs), (y, ys))]
                if delta_stage is not None:
                    sides = [delta_features(m, DELTA_WINDOWS) for m in sides]
                blocks.append(remove_zeros_frames(np.hstack(sides)))
                lists = [np.ascontiguousarray(v, dtype=np.int32) for v in (xs, ys)]
                triples.append(dist.mcd(mapped, y.data, idx_a=lists[0], idx_b=lists[1])[0])
                if ap_components is not None and it == iterations:        # the band rows follow the last alignment
                    joint, n, _ = bap.rows(x.band_track, y.band_track, lists[0], lists[1])
                    band_blocks.append(joint[:n])
            matrix = np.concatenate(blocks)
            self._bind_rate()
            self._train(matrix, **fit_options)
            if band_blocks:
                band_matrix = np.concatenate(band_blocks)
                if len(band_matrix) < ap_components:
                    raise ValueError(f'ap_model: the aligned pairs have {len(band_matrix)} cell(s) voiced on both sides, '
                                     f'fewer than the {ap_components} components of the band mixture')
                stack = self._band_stack(ap_components)
                stack.frame_period = getattr(delta_stage, 'frame_period', x.frame_period)
                stack._train(band_matrix, **fit_options)
                self.ap_converter, self.ap_rows = stack, len(band_matrix)
            cells = float(sum(t[0] for t in triples))
            total = 0.0
            for t in triples:
                total += float(t[0]) * float(t[1])
            self.align_history.append(dict(rows=len(matrix), mcd=total / cells if cells > 0 else float('nan'),
                                           em_iterations=int(getattr(self.gmm, 'n_iter_', 0))))
        if ap_components is not None and self.ap_converter is None:
            raise ValueError(f'ap_model: the band rows follow the last alignment (fit {iterations}), which this training '
                             f'did not reach: no band mixture was fitted')

    NONPARALLEL_RANGE = (0, 64)
    NONPARALLEL_DEFAULT = 6

    def train_nonparallel(self, source, target, source_keys, target_keys, iterations=None, f0_stats=False,
                          gv_stats=False, ms_stats=False, ms_length=4096, ap_model=False, **fit_options):
        """Training without parallel data: INCA (Erro, Moreno, Bonafonte 2010).  `source` and `target` are datasets of
        feature sets (WavFileDataset) that need no common keys; `source_keys` / `target_keys` name the utterances of
        each, in the order their frames take in the matrices.
        Of every utterance the SPEECH frames take part: those whose power term `vocoder.align.make_feature` sets with
        its defaults (what --frames speech means); an utterance without one contributes nothing.  Its delta features
        are `delta_features(c1..cN, DELTA_WINDOWS)` over ALL its frames, the rows selected afterwards, and the search
        row of a speech frame is [voicing term of make_feature | c1..cN | delta c1..cN]: D = 2 order + 1.
        Fit i = 0 .. iterations: the source search rows take their static and delta columns from X' -- fit 0: the
        source's own mel-cepstra; fit i: `convert(utterance, diff=False)` by fit i - 1, the deltas recomputed from it;
        the voicing term stays the source's own.  p = nearest(S, T), q = nearest(T, S) (backend.nn); the joint matrix is
        [x_k | y_p(k)] for k in source order followed by [x_q(j) | y_j] for j in target order, x ALWAYS the original
        source delta features; the mixture is fitted on it from scratch (same components, random_state, stopping rule,
        covariance structure).  `nonparallel_history` gets one record per fit: rows, em_iterations and mcd, the
        monitor -- the mean distortion in dB over c1..cN across all joint rows between the static columns the search
        used.  Order, sampling rate and frame period are checked as `_train_realigned` checks them (nothing is
        resampled).  f0_stats / gv_stats / ms_stats as in `train`, each side's statistics over its own utterances;
        ap_model raises ValueError: band rows along the nearest-neighbour pairs are left for later."""
        from ..backend import distortion as dist, nn
        from ..backend.mlpg import DELTA_WINDOWS, delta_features
        from ..vocoder.align import make_feature
        from .delta import DeltaFeatureConverter
        if ap_model:
            raise ValueError('ap_model: non-parallel training pairs no band-aperiodicity rows (left for later)')
        if iterations is None:
            iterations = self.NONPARALLEL_DEFAULT
        lo, hi = self.NONPARALLEL_RANGE
        if isinstance(iterations, bool) or int(iterations) != iterations or not lo <= iterations <= hi:
            raise ValueError(f'iterations must be an integer within [{lo}, {hi}], not {iterations!r}')
        iterations = int(iterations)
        delta_stage = self.base
        while not isinstance(delta_stage, DeltaFeatureConverter) and isinstance(delta_stage, abc.MapFeatureConverter):
            delta_stage = delta_stage.base
        if not isinstance(delta_stage, DeltaFeatureConverter):
            raise ValueError('non-parallel training searches on delta features: the stack needs a delta stage '
                             '(use_delta=True)')
        if ms_stats:
            from ..backend import ms as msfilter
            msfilter._length(ms_length)
        as_f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        k = _pkg()
        self.order, self.fs = None, self.mcep_fs
        sides = []
        for name, dataset, keys in (('source', source, list(source_keys)), ('target', target, list(target_keys))):
            utterances = []
            for key in keys:
                feature = dataset[key]
                record = feature.mel_cepstrum
                if self.order is None:
                    self.order = record.order
                if self.fs is None:
                    self.fs = record.fs
                if not utterances and name == 'source':
                    delta_stage.frame_period = record.frame_period
                if record.order != self.order:
                    raise ValueError(f'nonparallel: {name} "{key}" has mel-cepstra of order {record.order}, the converter '
                                     f'of order {self.order}')
                if record.fs != self.fs:
                    raise ValueError(f'nonparallel: {name} "{key}" is at {record.fs} Hz but the converter works at '
                                     f'{self.fs} Hz; non-parallel training does not resample')
                if record.frame_period != delta_stage.frame_period:
                    raise ValueError(f'frame_period of {name} "{key}" is {record.frame_period!r} but others are '
                                     f'{delta_stage.frame_period!r}')
                terms = make_feature(feature, record.fs)[:, :2]
                if ms_stats:
                    msfilter._fits([len(terms)], msfilter._length(ms_length))
                speech = np.flatnonzero(terms[:, 0] > 0)
                data = as_f64(record.data)
                utterances.append(dict(record=k.MelCepstrum(record.fs, record.frame_period, data), speech=speech,
                                       voicing=terms[speech, 1], f0=as_f64(feature.f0),
                                       delta=delta_features(as_f64(data[:, 1:]), DELTA_WINDOWS)[speech]))
            if not utterances:
                raise ValueError(f'nonparallel: no {name} files')
            sides.append(utterances)
        order = self.order
        xd, yd = (np.concatenate([u['delta'] for u in side]) for side in sides)
        vx, vy = (np.concatenate([u['voicing'] for u in side]) for side in sides)
        if not len(xd) or not len(yd):
            raise ValueError(f'nonparallel: no speech frames ({len(xd)} on the source side, {len(yd)} on the target side)')
        T = as_f64(np.hstack((vy[:, None], yd[:, :2 * order])))
        self.align_iterations, self.align_history = 0, []
        self.ap_converter, self.ap_rows = None, 0
        self.nonparallel, self.nonparallel_history = iterations, []
        for it in range(iterations + 1):
            if it == 0:
                mapped = xd[:, :2 * order]
            else:
                mapped = np.concatenate([
                    delta_features(as_f64(self.convert(u['record'], diff=False).data[:, 1:]),
                                   DELTA_WINDOWS)[u['speech'], :2 * order] for u in sides[0]])
            S = as_f64(np.hstack((vx[:, None], mapped)))
            # (the rows as they are, as the device driver searches them, corpus.train_converter_nonparallel: with a
            # voicing term of 9 and mel-cepstra of a few units the bound of the search, 4 (D + 1) 2^-53 (|q|^2 + |c|^2),
            # is some 1e-12 on squared distances of order 1 -- centring has nothing to repair here)
            p, q = nn.nearest(S, T, center=False)[0], nn.nearest(T, S, center=False)[0]
            matrix = np.vstack((np.hstack((xd, yd[p])), np.hstack((xd[q], yd))))
            self._train(matrix, **fit_options)
            own = np.arange(len(S), dtype=np.int32), np.arange(len(T), dtype=np.int32)
            moments = dist.mcd(as_f64(S[:, 1:order + 1]), as_f64(T[:, 1:order + 1]),
                               idx_a=np.concatenate((own[0], q)), idx_b=np.concatenate((p, own[1])), first_col=0)[0]
            self.nonparallel_history.append(dict(rows=len(matrix), mcd=float(moments[1]),
                                                 em_iterations=int(getattr(self.gmm, 'n_iter_', 0))))
        self.f0_stats = None
        if f0_stats:
            from ..backend import f0 as f0map
            self.f0_stats = f0map.stats_from_moments(*(
                f0map.merge_moments(f0map.logf0_moments([u['f0'] for u in side])) for side in sides))
        self.gv_stats, self.gv_var = None, None
        if gv_stats:
            from ..backend import gv as gvfilter
            moments = gvfilter.column_moments([u['record'].data for u in sides[1]])
            self.gv_stats = gvfilter.gv_from_moments(moments)
            self.gv_var = gvfilter.gv_statistics(moments)[1]
        self.ms_stats, self.ms_length = None, None
        if ms_stats:
            self._train_ms_sides(lambda: [u['record'] for u in sides[0]], [u['record'].data for u in sides[1]],
                                 ms_length)

    @property
    def kind(self):
        """'gmm', or 'exemplar' for a stack on an ExemplarFeatureConverter: what a model file's `converter` names"""
        try:
            return self.base.kind
        except AttributeError:
            return 'gmm'

    def _bind_rate(self):
        """hand the sampling rate to an innermost stage that works on spectra (the exemplar converter needs the
        all-pass constant); the mixture stages have no use for it"""
        bind = getattr(self.base, 'bind_rate', None)
        if bind is not None:
            bind(self.fs)

    def convert_f0(self, f0, key=0.0, fs=None):
        """the f0 track for synthesising a converted voice: voiced frames through the log-Gaussian transform of
        `f0_stats` (when trained with them), then transposed by `key` semitones; unvoiced frames stay 0.  fs: the
        sampling rate it will be synthesised at (default: the converter's), which bounds the result below fs/8"""
        from ..backend import f0 as f0map
        return f0map.map_f0(np.ascontiguousarray(f0, dtype=np.float64), self.fs if fs is None else fs,
                            stats=self.f0_stats, key=key)

    # ---- trained state on disk (an addition: the reference retrains on every run) ---------------------------------
    MODEL_FORMAT = 'kwiiyatta_amd.converter/1'

    def save(self, path):
        """the trained stack as one .npz: the mixture's parameters and what the outer stages learnt from the
        training set (mel-cepstrum order, sampling rate, frame period; the f0 statistics, the global variance and the
        modulation-spectrum statistics when there are any; the pitch ratio of the source waveforms; the re-alignment passes of the training as
        `align_iterations` with the monitor and row count of every fit as `align_mcd` / `align_rows`; the structure of
        the covariances as `covariance` when it is not 'full'; the band-aperiodicity mixture as `ap_weights`, `ap_means`,
        `ap_covariances` and `ap_covariance` when there is one; for a converter trained by `train_nonparallel` the
        iterations as `nonparallel` and a row (rows, monitor, EM iterations) per fit as `nonparallel_history`).
        A stack on the exemplar converter writes `converter: 'exemplar'` and, in the mixture's place, its dictionaries
        and settings: `exemplar_source`, `exemplar_target`, `exemplar_fft`, `exemplar_iterations`, `exemplar_sparsity`
        (and `exemplar_rows`); a file without `converter` is a mixture's"""
        gmm = self.gmm
        with open(path, 'wb') as fh:        # a file object: np.savez would append '.npz' to a bare name
            extra = {} if self.f0_stats is None else dict(f0_stats=np.array(self.f0_stats, dtype=np.float64))
            if self.kind == 'exemplar':     # the dictionaries in the mixture's place (a mixture's file has no `converter`)
                model = dict(converter='exemplar', **self.base.model_arrays())
            else:
                model = dict(weights=gmm.weights_, means=gmm.means_, covariances=gmm.covariances_)
            if self.gv_stats is not None:
                extra['gv_stats'] = np.array(self.gv_stats, dtype=np.float64)
            if self.gv_var is not None:
                extra['gv_var'] = np.array(self.gv_var, dtype=np.float64)
            if self.ms_stats is not None:
                extra.update(ms_stats_g=np.array(self.ms_stats[0], dtype=np.float64),
                             ms_stats_n=np.array(self.ms_stats[1], dtype=np.float64), ms_length=int(self.ms_length))
            structure = getattr(gmm, 'covariance_structure', 'full')
            if structure != 'full':          # (a full model's file is what it was before structures existed)
                extra['covariance'] = structure
            if self.ap_converter is not None:      # (a model without the band mixture has none of these keys)
                band = self.ap_converter.gmm
                extra.update(ap_weights=band.weights_, ap_means=band.means_, ap_covariances=band.covariances_,
                             ap_covariance=getattr(band, 'covariance_structure', 'full'))
            if self.nonparallel is not None:       # (a model trained on parallel data has neither key)
                extra.update(nonparallel=int(self.nonparallel), nonparallel_history=np.array(
                    [[r['rows'], r['mcd'], -1 if r['em_iterations'] is None else r['em_iterations']]
                     for r in self.nonparallel_history], dtype=np.float64).reshape(-1, 3))
            if self.f0_estimator != 'dio':         # (a model trained on DIO's tracks has no such key)
                extra['f0_estimator'] = str(self.f0_estimator)
            np.savez(fh, format=self.MODEL_FORMAT, order=self.order, fs=self.fs,
                     frame_period=getattr(self, 'frame_period', -1),     # (forwarded to the delta stage)
                     source_f0_rate=float(self.source_f0_rate),
                     align_iterations=int(self.align_iterations),
                     align_mcd=np.array([r['mcd'] for r in self.align_history], dtype=np.float64),
                     align_rows=np.array([r['rows'] for r in self.align_history], dtype=np.int64),
                     **model, **extra)

    def load(self, path):
        """the state written by `save` into this (untrained) stack; component count and dimensions come from
        the file.  `f0_stats` / `gv_stats` / `ms_stats` are None for a file without them (written without these statistics, or before
        they existed); `source_f0_rate` is 1.0 for a file without it, `align_iterations` 0 and `align_history` empty,
        the mixture's `covariance_structure` 'full', `nonparallel` None and `nonparallel_history` empty, `f0_estimator`
        'dio'"""
        with np.load(path, allow_pickle=False) as z:
            if str(z['format']) != self.MODEL_FORMAT:
                raise ValueError(f'{path!s}: not a converter model of format {self.MODEL_FORMAT}')
            kind = str(z['converter']) if 'converter' in z.files else 'gmm'
            if kind != self.kind:
                raise ValueError(f'{path!s}: a model of the {kind} converter, not of the {self.kind} converter')
            self.order, self.fs = int(z['order']), int(z['fs'])
            from .delta import DeltaFeatureConverter
            stage = self.base
            while isinstance(stage, abc.MapFeatureConverter):
                if isinstance(stage, DeltaFeatureConverter):       # it keeps the training set's frame period
                    period = float(z['frame_period'])
                    stage.frame_period = int(period) if period.is_integer() else period
                stage = stage.base
            if kind == 'exemplar':
                self.base.load_arrays(z)
                self._bind_rate()
            else:
                gmm = self.gmm
                gmm.weights_ = np.array(z['weights'], dtype=np.float64)
                gmm.means_ = np.array(z['means'], dtype=np.float64)
                gmm.covariances_ = np.array(z['covariances'], dtype=np.float64)
                gmm.n_components = len(gmm.weights_)
                gmm.covariance_structure = str(z['covariance']) if 'covariance' in z.files else 'full'
                gmm.converged_ = True
            self.f0_stats = tuple(float(v) for v in z['f0_stats']) if 'f0_stats' in z.files else None
            self.gv_stats = np.array(z['gv_stats'], dtype=np.float64) if 'gv_stats' in z.files else None
            self.gv_var = np.array(z['gv_var'], dtype=np.float64) if 'gv_var' in z.files else None
            has_ms = 'ms_stats_g' in z.files
            self.ms_stats = tuple(np.array(z[n], dtype=np.float64)
                                  for n in ('ms_stats_g', 'ms_stats_n')) if has_ms else None
            self.ms_length = int(z['ms_length']) if has_ms else None
            self.source_f0_rate = float(z['source_f0_rate']) if 'source_f0_rate' in z.files else 1.0
            self.ap_converter, self.ap_rows = None, 0
            if 'ap_weights' in z.files:
                stack = self._band_stack(len(z['ap_weights']))
                band = stack.gmm
                band.weights_ = np.array(z['ap_weights'], dtype=np.float64)
                band.means_ = np.array(z['ap_means'], dtype=np.float64)
                band.covariances_ = np.array(z['ap_covariances'], dtype=np.float64)
                band.covariance_structure = str(z['ap_covariance']) if 'ap_covariance' in z.files else 'full'
                band.converged_ = True
                period = float(z['frame_period'])
                stack.frame_period = int(period) if period.is_integer() else period
                self.ap_converter = stack
            self.align_iterations = int(z['align_iterations']) if 'align_iterations' in z.files else 0
            mcd = z['align_mcd'] if 'align_mcd' in z.files else ()
            rows = z['align_rows'] if 'align_rows' in z.files else [None] * len(mcd)
            self.align_history = [dict(rows=None if n is None else int(n), mcd=float(v), em_iterations=None)
                                  for n, v in zip(rows, mcd)]
            self.nonparallel = int(z['nonparallel']) if 'nonparallel' in z.files else None
            self.f0_estimator = str(z['f0_estimator']) if 'f0_estimator' in z.files else 'dio'
            history = z['nonparallel_history'] if 'nonparallel_history' in z.files else ()
            self.nonparallel_history = [dict(rows=int(n), mcd=float(v), em_iterations=None if e < 0 else int(e))
                                        for n, v, e in history]
        return self

    def gv_ascent_statistics(self):
        """(mean, var) of c1..cN for `convert(mlpg_gv=...)`; ValueError when the converter has none, or when a variance
        is not positive (a converter trained on one utterance)"""
        if self.gv_stats is None or self.gv_var is None:
            raise ValueError('mlpg_gv: the converter has no global-variance statistics with their variance (retrain it '
                             'with gv_stats=True on two or more utterances)')
        mean, var = (np.ascontiguousarray(a[1:], dtype=np.float64) for a in (self.gv_stats, self.gv_var))
        if not (var > 0).all():
            raise ValueError('mlpg_gv: the variance of the global variance is not positive everywhere (retrain the '
                             'converter with gv_stats=True on two or more utterances)')
        return mean, var

    def convert(self, mel_cepstrum, gv=0.0, ms=0.0, mlpg_gv=None, gv_weight=1.0, postfilter=0.0, keep_power=False,
                **kwargs):
        """a MelCepstrum at the converter's sampling rate: c0 of the input, c1..cN converted.
        gv > 0 (a strength within [0, 1]; needs `gv_stats`): the converted c1..cN through the global-variance
        postfilter, each trajectory stretched about its own mean towards the target's variance.  With diff=True the
        filter's change of the NON-differential conversion is added to the differential one, which costs one more
        conversion (MLPG) of the same input.
        ms > 0 (a strength within [0, 1]; needs `ms_stats`): the converted c1..cN through the modulation-spectrum
        postfilter, every modulation-frequency bin of each trajectory moved from the statistics of converted speech
        towards the target's; it composes with diff=True as gv does.  With both, the modulation-spectrum filter comes
        first and the global-variance filter takes its moments from that filter's output.
        em=N (an integer within [0, 16], through **kwargs down to the mixture stage): EM trajectory conversion over
        soft mixture posteriors instead of one arg-max mixture per frame, N re-estimations of the posteriors
        (backend.mlpg.MLPG).  It composes with diff, gv and ms as the arg-max conversion does -- with diff=True the
        non-differential conversion the filters look at is an EM conversion too.  `ms_stats` are learnt from ARG-MAX
        conversions of the training set (as re-alignment uses them), whatever `em` is given here.
        mlpg_gv=N (an integer within [0, 256]; needs `gv_stats` and `gv_var`): parameter generation considering the
        global variance instead of the postfilter -- N conjugate-gradient steps on the joint objective of trajectory
        and GV likelihood, from the linearly scaled track (backend.mlpg.MLPG(gv=...)); gv_weight > 0 weighs the GV
        term.  c0 is kept; with diff=True the variance is that of the converted spectrum (differential + source).  It
        goes with em=N, and with neither gv > 0 (the same repair twice) nor ms > 0 (not composed yet).
        postfilter > 0 (beta within [0, 1]) / keep_power=True run last, after ms, gv and mlpg_gv, on the ABSOLUTE
        converted rows -- c0 of the input with the converted c1..cN; with diff=True input + differential, one addition
        -- through backend.power.postfilter: the mel-cepstral formant emphasis of strength beta, then c0 shifted until
        the frame has the energy of the input's frame (keep_power) or of the unfiltered converted frame (postfilter
        alone).  c0 is not the power: converting c1.. at a fixed c0 moves a frame's energy by several dB.  Column 0 of
        the result is then the corrected c0 -- with diff=True its DIFFERENCE from the input's c0, for a filter that
        takes c0 into account (apply_diff_filter(use_c0=True)).  With both neutral nothing changes and
        backend.power is not imported."""
        if mel_cepstrum.order != self.order:
            raise ValueError(f'order is expected to {self.order!s} but {mel_cepstrum.order!s}')
        if not 0.0 <= postfilter <= 1.0:
            raise ValueError(f'postfilter: beta {postfilter!r} is outside [0, 1]')
        if mlpg_gv is not None:
            if gv > 0:
                raise ValueError('mlpg_gv does not go with gv > 0: the postfilter would repair the same variance twice')
            if ms > 0:
                raise ValueError('mlpg_gv does not go with ms > 0: composing it with the modulation-spectrum filter is '
                                 'left for later')
            from ..backend import gv as gvgen
            mean, var, mlpg_gv, gv_weight = gvgen.ascent_arguments(*self.gv_ascent_statistics(), mlpg_gv, gv_weight)
            kwargs = dict(kwargs, gv_stats=(mean, var), gv_iterations=mlpg_gv, gv_weight=gv_weight)
        if not 0.0 <= gv <= 1.0:
            raise ValueError(f'global variance: strength {gv!r} is outside [0, 1]')
        if gv > 0 and self.gv_stats is None:
            raise ValueError('global variance: the converter has no statistics (train it with gv_stats=True)')
        if not 0.0 <= ms <= 1.0:
            raise ValueError(f'modulation spectrum: strength {ms!r} is outside [0, 1]')
        if ms > 0 and self.ms_stats is None:
            raise ValueError('modulation spectrum: the converter has no statistics (train it with ms_stats=True)')
        out = copy.copy(mel_cepstrum) if mel_cepstrum.fs == self.fs else _pkg().resample(mel_cepstrum, self.fs)
        power, shape = out.data[:, :1], out.data[:, 1:]
        converted = super().convert(shape, raw=mel_cepstrum, **kwargs)
        if gv > 0 or ms > 0:
            as_f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
            converted = as_f64(converted)
            diff = bool(kwargs.get('diff'))
            plain = as_f64(super().convert(shape, raw=mel_cepstrum, **dict(kwargs, diff=False))) if diff else converted
            if ms > 0:
                from ..backend import ms as msfilter
                stats_g, stats_n = (as_f64(s[1:]) for s in self.ms_stats)
                if diff:
                    plain, converted = msfilter.postfilter([plain, plain], stats_g, stats_n, ms, base=[plain, converted],
                                                           first_col=0)
                else:
                    plain = converted = msfilter.postfilter(plain, stats_g, stats_n, ms, first_col=0)
            if gv > 0:
                from ..backend import gv as gvfilter
                converted = gvfilter.postfilter(plain, as_f64(self.gv_stats[1:]), gv, base=converted, first_col=0)
        if postfilter > 0 or keep_power:
            from ..backend import power as powerfilter
            source = np.ascontiguousarray(out.data, dtype=np.float64)
            options = dict(ref=source if keep_power else None, alpha=out.alpha(),
                           fft_size=powerfilter.energy_fft_size(self.fs))
            if kwargs.get('diff'):
                base = np.hstack((np.zeros_like(source[:, :1]), converted)).astype(np.float64, copy=False)
                out.data = powerfilter.postfilter(source + base, postfilter, base=base, **options)
            else:
                absolute = np.hstack((source[:, :1], converted)).astype(np.float64, copy=False)
                out.data = powerfilter.postfilter(absolute, postfilter, **options)
            return out
        out.data = np.hstack((power, converted))
        return out
