"""`evaluate_voice`: objective evaluation of a trained converter on parallel utterances it was not trained on.
An addition to the reference's commands (it measures a conversion only in its tests): for every evaluated pair the
three measures voice-conversion work reports, taken along the DTW alignment of the pair (the alignment training would
use for it: silence pads, DTW features, FastDTW, strict filter, cut to the stretch between the pads)

    MCD           mel-cepstral distortion in dB of the CONVERTED source against the target, c0 left out, beside the
                  distortion of the UNCONVERTED source along the same alignment (the baseline a conversion must beat)
    f0 RMSE       root mean square of 1200 log2(f0_source / f0_target) cents over the frames both sides voice;
                  with --convert-f0 / --transpose-key the source f0 is mapped first, as convert_voice would map it
    V/UV error    share of the aligned frames on which the two sides disagree in voicing

The conversion runs on the source's own time axis -- what a listener would hear from convert_voice, `--gv` included --
and is compared frame by frame through the index lists of the alignment.  frames='speech' (default) takes the aligned
frames whose TARGET-side binarised power term is set (column 0 of the DTW feature: c0 within 1.636 of its maximum);
frames='all' every aligned frame that lies inside both utterances.  The frame selection applies to the distortion;
the f0 and voicing figures always take every aligned frame (their own voicing decision selects).
With --align-iterations N the converter is trained with N re-alignment passes (Config), and the report starts with the
training record: one line per fit with the rows of its joint matrix and the monitor distortion of its alignment.
The numbers come from the kernels of kwy_eval.hip (backend.distortion); this module is the bookkeeping around them."""
import json
import math
import pathlib
import sys
from types import SimpleNamespace

import numpy as np

from ._convert_options import filled, takes_options
from .convert_voice import COMMAND_OPTIONS, _stages, driver_options

PAD_LEN = 100             # align_even's silence pads
FRAMES = ('speech', 'all')


def _nan_to_none(v):
    return None if isinstance(v, float) and math.isnan(v) else v


class Result:
    """the figures of one pair (or the pooled figures of several): built from the (n, mean, M2) triples of the
    distortion, of the unconverted source's distortion and of the f0 error in cents, and the voicing counts

        frames            distortion frames (the selected aligned frames)
        mcd, mcd_source   mean distortion in dB over them: converted / unconverted source against the target
        f0_rmse_cents     over the frames both sides voice;  vuv_error: (VU + UV) / all aligned frames
        vv, vu, uv, uu    source voiced / target voiced, source voiced / target unvoiced, ...
        aligned           aligned frames (the alignment's length);  outside: those of them beyond either utterance
        bap, bap_source   with convert_ap: mean band-aperiodicity error in dB (sqrt of the mean squared difference over
                          the bands) of the converted / unconverted source's band track against the target's, over the
                          bap_frames aligned frames that both sides voice; nan / 0 without convert_ap
    A figure without frames is nan.  idx_x / idx_y (frame indices into the two utterances) and mcd_frames
    (per aligned frame, nan where not selected) are kept when they were asked for."""

    def __init__(self, mcd_moments, source_moments, f0_moments, counts, aligned, outside=0, idx_x=None, idx_y=None,
                 mcd_frames=None, bap_moments=None, bap_source_moments=None):
        self.bap_moments, self.bap_source_moments = (None if m is None else tuple(float(v) for v in m)
                                                     for m in (bap_moments, bap_source_moments))
        self.mcd_moments, self.source_moments, self.f0_moments = (tuple(float(v) for v in m) for m in
                                                                  (mcd_moments, source_moments, f0_moments))
        self.vv, self.vu, self.uv, self.uu = (int(v) for v in counts)
        self.aligned, self.outside = int(aligned), int(outside)
        self.idx_x, self.idx_y, self.mcd_frames = idx_x, idx_y, mcd_frames

    frames = property(lambda self: int(self.mcd_moments[0]))
    mcd = property(lambda self: self.mcd_moments[1] if self.mcd_moments[0] > 0 else math.nan)
    mcd_source = property(lambda self: self.source_moments[1] if self.source_moments[0] > 0 else math.nan)
    counts = property(lambda self: (self.vv, self.vu, self.uv, self.uu))
    convert_ap = property(lambda self: self.bap_moments is not None)
    bap_frames = property(lambda self: int(self.bap_moments[0]) if self.convert_ap else 0)
    bap = property(lambda self: self.bap_moments[1] if self.bap_frames > 0 else math.nan)
    bap_source = property(lambda self: self.bap_source_moments[1] if self.convert_ap and self.bap_source_moments[0] > 0
                          else math.nan)

    @property
    def f0_rmse_cents(self):
        from .backend.distortion import rmse
        return rmse(self.f0_moments)

    @property
    def vuv_error(self):
        from .backend.distortion import vuv_error
        return vuv_error(self.counts)

    def as_dict(self):
        """the JSON form: numbers, nan as null"""
        d = dict(frames=self.frames, aligned=self.aligned, outside=self.outside, mcd=self.mcd, mcd_source=self.mcd_source,
                 f0_rmse_cents=self.f0_rmse_cents, f0_frames=int(self.f0_moments[0]), vuv_error=self.vuv_error,
                 counts=dict(vv=self.vv, vu=self.vu, uv=self.uv, uu=self.uu))
        if self.convert_ap:
            d.update(bap=self.bap, bap_source=self.bap_source, bap_frames=self.bap_frames)
        return {k: _nan_to_none(v) for k, v in d.items()}

    def line(self, name):
        band = f' band aperiodicity {self.bap:.3f} dB (source {self.bap_source:.3f} dB, {self.bap_frames} frames)' \
            if self.convert_ap else ''
        return (f'{name}: frames {self.frames} MCD {self.mcd:.3f} dB (source {self.mcd_source:.3f} dB) '
                f'f0 RMSE {self.f0_rmse_cents:.1f} cents V/UV error {100 * self.vuv_error:.2f} %' + band)


def pool(results):
    """the figures of all frames of `results` together: the triples merged on the device (backend.distortion
    .merge_moments, in the order given; a pair without frames contributes nothing), the counts added"""
    from .backend import distortion as dist
    results = list(results)
    if not results:
        zero = (0.0, 0.0, 0.0)
        return Result(zero, zero, zero, (0, 0, 0, 0), 0)
    bands = all(r.convert_ap for r in results)          # (the band error is pooled when every pair has one)
    triples = np.array([[r.mcd_moments, r.source_moments, r.f0_moments] +
                        ([r.bap_moments, r.bap_source_moments] if bands else []) for r in results], dtype=np.float64)
    merged = dist.merge_moments(np.ascontiguousarray(triples))
    return Result(merged[0], merged[1], merged[2], [sum(r.counts[i] for r in results) for i in range(4)],
                  sum(r.aligned for r in results), sum(r.outside for r in results),
                  **(dict(bap_moments=merged[3], bap_source_moments=merged[4]) if bands else {}))


def _check_options(gv, transpose_key, frames):
    if frames not in FRAMES:
        raise ValueError(f'frames must be one of {FRAMES}, not {frames!r}')
    if not 0.0 <= gv <= 1.0:
        raise ValueError(f'global variance: strength {gv!r} is outside [0, 1]')
    from .backend.f0 import KEY_RANGE
    if not -KEY_RANGE <= transpose_key <= KEY_RANGE:
        raise ValueError(f'transpose_key {transpose_key!r} is outside [-{KEY_RANGE}, {KEY_RANGE}]')


PAIR_OPTIONS = dict(gv=0.0, convert_f0=False, transpose_key=0.0, frames='speech', per_frame=False, em=None, mlpg_gv=None,
                    convert_ap=False)


@takes_options(defaults=PAIR_OPTIONS)
def evaluate_pair(converter, source, target, **options):
    """The figures of one parallel pair: two unaligned feature sets (trimmed as training trims them, if the alignment
    is to be the one training would use).  Both are padded and aligned as `align_even` does -- the same pad draws in
    the same order, so a seeded run reproduces training's alignment -- `source.mel_cepstrum` is converted on its own
    time axis through `converter.convert(..., gv=gv)` (which resamples a source of another sampling rate to the
    converter's; the comparison then runs at the converter's rate), and the kernels measure along the index lists.
    convert_f0 / transpose_key: the source f0 through the converter's f0 map first (convert_voice's options).
    per_frame=True keeps the index lists and the per-frame distortion in the result.
    em=N: the conversion is the EM trajectory conversion over soft mixture posteriors with N re-estimations
    (`converter.convert(..., em=N)`, convert_voice's --mlpg-em); None: one arg-max mixture per frame.
    mlpg_gv=N: parameter generation considering the global variance behind it, N steps
    (`converter.convert(..., mlpg_gv=N)`, --mlpg-gv); it does not go with gv > 0.
    convert_ap: also the band-aperiodicity error (`Result.bap`, `bap_source`, `bap_frames`) of the source's band track
    converted by the converter's band mixture -- clamped as the rendering clamps it -- and of the unconverted one
    against the target's, along the same index lists over the frames both sides voice (backend.bap.error); both
    feature sets must be at the converter's sampling rate (12 kHz or more)."""
    import kwiiyatta_amd as k
    from .backend import distortion as dist
    from .backend import f0 as f0map
    from .vocoder.align import even_indices, make_feature
    o = SimpleNamespace(**filled(options, PAIR_OPTIONS))
    gv, convert_f0, transpose_key, frames = o.gv, o.convert_f0, o.transpose_key, o.frames
    _check_options(gv, transpose_key, frames)
    if convert_f0 and converter.f0_stats is None:
        raise ValueError('f0 conversion: the converter has no statistics (train it with f0_stats=True)')
    if o.convert_ap:
        from .convert_voice import check_convert_ap
        check_convert_ap(converter)
        if not source.fs == target.fs == converter.fs:
            raise ValueError(f'convert_ap: the pair is at {source.fs} Hz and {target.fs} Hz, the converter at '
                             f'{converter.fs} Hz (the band tracks are not resampled)')
    a, b = k.pad_silence(source, PAD_LEN), k.pad_silence(target, PAD_LEN)
    xs, ys = even_indices(a, b, PAD_LEN, strict=True)
    idx_x, idx_y = (np.ascontiguousarray(v, dtype=np.int32) for v in (xs, ys))
    # converter.convert's keywords: (value, whether it is on) -- an option that is off is not handed over
    stages = dict(gv=(gv, gv > 0), em=(o.em, o.em is not None), mlpg_gv=(o.mlpg_gv, o.mlpg_gv is not None))
    converted = converter.convert(source.mel_cepstrum, **{name: v for name, (v, on) in stages.items() if on})
    fs = converted.fs

    def coefficients(f):
        record = f.mel_cepstrum if f.fs == fs else f.resample_mel_cepstrum(fs)
        return np.ascontiguousarray(record.data, dtype=np.float64)
    conv, src, tgt = np.ascontiguousarray(converted.data, dtype=np.float64), coefficients(source), coefficients(target)
    mask = None
    if frames == 'speech':
        # the target side's DTW feature as dtw_feature made it: column 0 is the binarised power term
        mask = np.ascontiguousarray(make_feature(b, min(a.fs, b.fs), vuv='voiced', power='binalize')[:, 0])
    lists = dict(idx_a=[idx_x, idx_x], idx_b=[idx_y, idx_y], off_a=PAD_LEN, off_b=PAD_LEN)
    m, _, rows = dist.mcd([conv, src], [tgt, tgt], mask=[mask, mask], per_row=True, **lists)
    f0_src = np.ascontiguousarray(source.f0, dtype=np.float64)
    if convert_f0 or transpose_key != 0:
        f0_src = f0map.map_f0(f0_src, source.fs, stats=converter.f0_stats if convert_f0 else None, key=transpose_key)
    counts, f0_m, _ = dist.f0_error(f0_src, np.ascontiguousarray(target.f0, dtype=np.float64), idx_a=idx_x, idx_b=idx_y,
                                    off_a=PAD_LEN, off_b=PAD_LEN)
    # the cut of align_even ends where BOTH sides are in their trailing pads: cells with one side in its pad remain,
    # and the kernels pass them over (the f0 kernel counts every other aligned frame)
    outside = len(idx_x) - int(counts.sum())
    keep = dict(idx_x=idx_x - PAD_LEN, idx_y=idx_y - PAD_LEN, mcd_frames=rows[0]) if o.per_frame else {}
    if o.convert_ap:
        from .backend import bap
        own, mapped = converter.convert_band_track(source)
        theirs = k.band_track(target)
        band = bap.error([mapped, own], [theirs, theirs], idx_a=[idx_x, idx_x], idx_b=[idx_y, idx_y], off_a=PAD_LEN,
                         off_b=PAD_LEN)
        keep.update(bap_moments=band[0], bap_source_moments=band[1])
    return Result(m[0], m[1], f0_m, counts, len(idx_x), outside, **keep)


def evaluate(converter, pairs_or_dataset, keys=None, **options):
    """(results, total): `evaluate_pair` for every key, in the order given (default: sorted), and their pooled figures.
    pairs_or_dataset: a mapping / list of (source, target) feature sets, or the aligned parallel dataset training
    takes (`kwiiyatta_amd.align(source_dataset, target_dataset)`): then the pairs are its trimmed, unaligned items.
    A pair without frames stays in `results` and adds nothing to the total."""
    from .converter import abc
    from .converter.mcep import _trimmed_stage
    items = _trimmed_stage(pairs_or_dataset) if isinstance(pairs_or_dataset, abc.Dataset) else pairs_or_dataset
    if keys is None:
        keys = sorted(items.keys()) if hasattr(items, 'keys') else range(len(items))
    results = [evaluate_pair(converter, *items[key], **options) for key in keys]
    return results, pool(results)


# ---- command line --------------------------------------------------------------------------------------------------------
def _count(least):
    def parse(text):
        import argparse
        try:
            n = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f'invalid file count: {text!r}') from None
        if n < least:
            raise argparse.ArgumentTypeError(f'{text} is below {least}')
        return n
    return parse


def make_config():
    """the command's options, unparsed: Config's vocoder and converter options unchanged, plus its own"""
    import kwiiyatta_amd as k
    conf = k.Config()
    conf.add_argument('--eval-skip-files', type=_count(0), default=0,
                      help='Skip file num of the sorted common files before the evaluated ones (default 0)')
    conf.add_argument('--eval-max-files', type=_count(1), default=None,
                      help='File num to evaluate (default: all that remain)')
    conf.add_argument('--frames', choices=FRAMES, default='speech',
                      help='Frames the distortion is taken over: aligned frames whose target-side power term is set, '
                           'or all aligned frames')
    conf.add_argument('--convert-f0', action='store_true',
                      help='Measure the f0 error of the source f0 mapped to the target speaker, as convert_voice '
                           '--convert-f0 synthesises it')
    conf.add_argument('--batch', action='store_true',
                      help='Evaluate all pairs through the GPU-resident batch path')
    conf.add_argument('--json', type=str, metavar='PATH', help='Write per-file and pooled figures to this file')
    conf.add_transpose_key_argument()
    conf.add_gv_argument()
    conf.add_mlpg_em_argument()
    conf.add_mlpg_gv_argument()
    conf.add_aperiodicity_arguments()
    conf.add_converter_arguments()
    return conf


def file_slice(keys, skip, count):
    """`count` (None: all) of the sorted keys behind the first `skip` (None: 0): how Config picks the training files
    (--skip-files / --max-files) and this command the evaluated ones (--eval-skip-files / --eval-max-files)"""
    return sorted(keys)[slice(skip, None)][:count]


def overlap_warning(trained, evaluated):
    """one line naming the files that were both trained on and evaluated, or None"""
    both = sorted(set(trained) & set(evaluated))
    if not both:
        return None
    return (f'warning: {len(both)} evaluated file(s) were also trained on, their figures flatter the converter: '
            + ', '.join(str(key) for key in both))


def training_record_lines(converter):
    """the record of a training with --align-iterations, a line per fit: the rows of its joint matrix and the monitor,
    the mean distortion along the training alignment between the target and the source coefficients that alignment was
    found with (fit 0: the source's own, fit k: converted by fit k - 1).  Nothing for a converter aligned once.
    For a training with --nonparallel: a line per fit of `nonparallel_history` instead"""
    if getattr(converter, 'kind', 'gmm') == 'exemplar':
        stage = converter.base
        size = [f'exemplar dictionary: {len(stage.source)} exemplars of {stage.rows} training rows, '
                f'{stage.fft // 2 + 1} bins, {stage.iterations} iterations, sparsity {stage.sparsity:g}']
        history = getattr(converter, 'align_history', None) or []
        if not getattr(converter, 'align_iterations', 0):
            return size
        return size + [f'training alignment {it}: rows {"?" if r["rows"] is None else r["rows"]} monitor MCD '
                       f'{r["mcd"]:.3f} dB' for it, r in enumerate(history)]
    if getattr(converter, 'nonparallel', None) is not None:
        # a training with --nonparallel: the rows are the speech frames of both sides, the monitor runs across the
        # nearest-neighbour pairs of the fit
        return [f'non-parallel fit {it}: rows {r["rows"]} monitor MCD {r["mcd"]:.3f} dB'
                for it, r in enumerate(converter.nonparallel_history)]
    history = getattr(converter, 'align_history', None) or []
    if not getattr(converter, 'align_iterations', 0):
        return []
    return [f'training alignment {it}: rows {"?" if r["rows"] is None else r["rows"]} monitor MCD {r["mcd"]:.3f} dB'
            for it, r in enumerate(history)]


def report(names, results, total, options):
    """the --json document: the options that shape the figures, a record per file, the pooled record"""
    return dict(options=dict(options),
                files=[dict(name=str(name), **r.as_dict()) for name, r in zip(names, results)],
                total=dict(files=sum(1 for r in results if r.frames > 0), **total.as_dict()))


def _evaluate_batched(conf, converter, dataset, keys, options):
    """the pairs at the converter's sampling rate, order and frame period through corpus.evaluate_batch, the others
    one by one (the batch path has no resampling stage).  For a converter trained on pitch-shifted sources the source
    waveforms of the batch go through the shifter in one call and are analysed from there on the device"""
    import kwiiyatta_amd as k
    from . import corpus
    from .converter.delta import DeltaFeatureConverter
    if options.get('convert_ap'):
        from .convert_voice import check_convert_ap
        check_convert_ap(converter)               # (raises before any file is read)
    period = next((s.frame_period for s in _stages(converter) if isinstance(s, DeltaFeatureConverter)), None)
    sides = [pathlib.Path(conf.source), pathlib.Path(conf.target)]
    results, batch = {}, []
    for key in keys:
        pair = [conf.create_analyzer(d / key, Analyzer=k.analyze_wav) for d in sides]
        if any(a.fs != converter.fs or a.mel_cepstrum_order != converter.order or
               (period is not None and a.frame_period != period) for a in pair):
            results[key] = evaluate_pair(converter, *_trimmed(dataset)[key], **options)
        else:
            # (the source's f0 track is taken from the shifted waveform below when there is a shift)
            source = _triple(pair[0]) if getattr(converter, 'source_f0_rate', 1.0) == 1 else \
                (np.ascontiguousarray(pair[0].wavdata.data, dtype=np.float64),)
            batch.append((key, (source, _triple(pair[1])), float(pair[0].frame_period)))
    rate = getattr(converter, 'source_f0_rate', 1.0)
    if batch and rate != 1:
        sources = _shifted_triples([pair[0][0] for _, pair, _ in batch], converter.fs, rate, batch[0][2],
                                   f0_estimator=getattr(conf, 'f0_estimator', 'dio'))
        batch = [(key, (src, pair[1]), period) for (key, pair, period), src in zip(batch, sources)]
    if batch:
        asked = SimpleNamespace(**dict(COMMAND_OPTIONS, gv=options['gv'], convert_f0=options['convert_f0'],
                                       transpose_key=options['transpose_key'], mlpg_em=options.get('em'),
                                       mlpg_gv=options.get('mlpg_gv')))
        records, _ = corpus.evaluate_batch(
            [p for _, p, _ in batch], converter.fs, converter.gmm, order=converter.order, frame_period=batch[0][2],
            frames=options['frames'], ap_gmm=converter.ap_converter.gmm if options.get('convert_ap') else None,
            **driver_options(converter, asked))
        for (key, _, _), rec in zip(batch, records):
            band = {name: rec[name] for name in ('bap_moments', 'bap_source_moments') if name in rec}
            results[key] = Result(rec['mcd_moments'], rec['source_moments'], rec['f0_moments'], rec['counts'],
                                  rec['aligned'], rec['outside'], **band)
    return [results[key] for key in keys]


def _shifted_triples(waves, fs, rate, frame_period, group=16, f0_estimator='dio'):
    """(x, f0, t) device tensors per waveform: the waveforms through ONE kwy_pitch_shift_batch_dev call
    (convert_voice.shift_waves_dev), then DIO (or, with f0_estimator='pyin', pYIN) + StoneMask on the device, as
    Analyzer.extract_f0 runs them"""
    import torch
    from . import _lib
    from .backend import world
    from .convert_voice import shift_waves_dev
    xs = shift_waves_dev(waves, fs, rate)
    ctx = _lib.default_context()
    frames = [world.dio_frames(fs, x.numel(), frame_period) for x in xs]
    ts, coarse, f0 = ([torch.empty(n, dtype=torch.float64, device=xs[0].device) for n in frames] for _ in range(3))
    status = torch.zeros(len(xs), dtype=torch.int32, device=xs[0].device)
    torch.cuda.current_stream(xs[0].device).synchronize()
    from .pipeline import check_f0_status, coarse_f0_batch_dev, f0_jobs
    for g in range(0, len(xs), group):
        sl = slice(g, g + group)
        jobs, _ = f0_jobs(xs[sl], ts[sl], coarse[sl], f0[sl], status[sl])
        coarse_f0_batch_dev(ctx, f0_estimator, jobs, len(xs[sl]), int(fs), float(frame_period))
        world.stonemask_batch_dev(ctx, xs[sl], ts[sl], coarse[sl], fs, f0[sl])
    ctx.sync()
    check_f0_status(f0_estimator, status.cpu().numpy())
    return list(zip(xs, f0, ts))


def _trimmed(dataset):
    from .converter.mcep import _trimmed_stage
    return _trimmed_stage(dataset)


def _triple(analyzer):
    """(waveform, f0, frame times) of an analysed file, as the corpus drivers take an utterance"""
    f0, t = analyzer._frame_grid()
    return tuple(np.ascontiguousarray(v, dtype=np.float64) for v in (analyzer.wavdata.data, f0, t))


def main():
    conf = make_config()
    conf.parse_args()
    model = conf.converter_model
    training = model is None or not pathlib.Path(model).is_file()
    dataset = conf.load_dataset()              # (--source / --target name the evaluated files, trained or not)
    keys = file_slice(dataset.keys(), conf.eval_skip_files, conf.eval_max_files)
    if not keys:
        conf.parser.error('no files to evaluate: --eval-skip-files / --eval-max-files leave none of the '
                          f'{len(dataset.keys())} common files of --source and --target')
    if training:
        if conf.nonparallel is not None:           # either side's training files, picked per directory
            trained = set().union(*(file_slice(side.keys(), conf.skip_files, conf.max_files)
                                    for side in conf.nonparallel_sides(1.0)))
        else:
            trained = file_slice(dataset.keys(), conf.skip_files, conf.max_files)
        warning = overlap_warning(trained, keys)
        if warning:
            print(warning, file=sys.stderr)
    converter = conf.train_converter(use_delta=True, f0_stats=conf.convert_f0, gv_stats=conf.gv > 0,
                                     **(dict(gv_var=True) if conf.mlpg_gv is not None else {}),
                                     **(dict(ap_model=True) if conf.convert_aperiodicity else {}))
    options = dict(gv=conf.gv, convert_f0=conf.convert_f0, transpose_key=conf.transpose_key, frames=conf.frames)
    if conf.convert_aperiodicity:
        options['convert_ap'] = True
        print(f'band-aperiodicity mixture: {converter.ap_converter.gmm.n_components} components'
              + (f', fitted on {converter.ap_rows} rows' if converter.ap_rows else ''))
    # (--mlpg-em, --mlpg-gv: EM trajectory conversion, GV-considering parameter generation, as convert_voice runs them)
    options.update({name: v for name, v in dict(em=conf.mlpg_em, mlpg_gv=conf.mlpg_gv).items() if v is not None})
    if conf.batch:
        results = _evaluate_batched(conf, converter, dataset, keys, options)
        total = pool(results)
    else:
        results, total = evaluate(converter, dataset, keys, **options)
    for line in training_record_lines(converter):
        print(line)
    for key, r in zip(keys, results):
        print(r.line(key))
    if total.frames == 0:
        conf.parser.error(f'none of the {len(keys)} evaluated file(s) has a selected frame')
    print(total.line(f'total ({sum(1 for r in results if r.frames > 0)} of {len(keys)} files)'))
    if conf.json is not None:
        out = pathlib.Path(conf.json)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(report(keys, results, total, options), indent=1) + '\n')


if __name__ == '__main__':
    main()
