"""`kwiiyatta`: train a converter on a parallel corpus (--source / --target directories with equally named wav
files) and convert wav files with it.  Command line and outputs of the reference's kwiiyatta/convert_voice.py:
for every input <name>.wav a <name>.diff.wav (the input waveform through the differential MLSA filter) and a
<name>.synth.wav (WORLD synthesis from the converted mel-cepstrum).  Additions: `--no-diffvc` skips the first;
`--converter-model FILE` keeps the trained converter between runs; `--batch` renders the .synth.wav outputs of all
input files -- and the .diff.wav outputs -- through the HBM-resident batch path (kwiiyatta_amd.corpus.convert_batch:
waves of 16 files in lockstep, wav in -> 16-bit PCM out on the device) instead of file by file; `--convert-f0`
synthesises the .synth.wav outputs on the source f0 mapped to the target speaker's voiced log-f0 statistics (trained
with the converter and kept in its model file), `--transpose-key` transposes them by so many semitones.  Neither
reaches the .diff.wav output: the MLSA filter runs on a waveform, whose pitch it keeps.
`--source-f0-rate RATE|auto` changes the pitch of that waveform instead: every source waveform -- the training set's
and the files to convert -- goes through the pitch shifter (WSOLA + resampling, backend.pitch) before anything else
runs, the converter is trained from the shifted source to the target (the shift moves the formants too; the mixture
learns that), and both outputs start from the shifted waveform.  `auto` takes the ratio of the two speakers' mean
voiced log-f0 over the training files.  The rate is kept in the converter model; at 1 (the default) the shifter is
never called.  `--convert-f0` and `--gv` compose with it unchanged: their statistics are those of the shifted source.
`--gv [STRENGTH]` runs the global-variance postfilter on the converted mel-cepstrum of both outputs: a GMM conversion
averages, its trajectories vary about 0.6 times as much as the target speaker's and the voice sounds muffled; the
filter stretches every coefficient's trajectory about its own mean until its variance is the one the target's training
utterances have (learnt with the converter, kept in its model file), or STRENGTH of the way there.
`--ms [STRENGTH]` runs the modulation-spectrum postfilter on the converted mel-cepstrum of both outputs, before `--gv`
where both are given: the smoothing of GMM + MLPG removes the fast movement of a trajectory (10 - 50 Hz of modulation
frequency) far more than the slow, which one variance ratio cannot undo; the filter takes the log power spectrum of
every coefficient's trajectory along time and moves every bin from the statistics of converted speech to those of the
target speaker's natural speech (both learnt with the converter at `--ms-length` frames and kept in its model file),
or STRENGTH of the way there, keeping the phase.  No utterance may be longer than that length.
`--align-iterations N` trains with iterative re-alignment: after the first fit every training pair is aligned again, N
times over, with the source mel-cepstrum converted by the converter fitted so far in its DTW features (the reference
aligns once, on the two speakers' own coefficients), the joint matrix is rebuilt along the new paths and the mixture
refitted.  The count is kept in the converter model; 0 (the default) is the reference's training.
`--formant-shift SEMITONES` warps the CONVERTED spectral envelope along frequency by 2 ** (SEMITONES / 12) before the
synthesis (Feature.shift_formants, `convert(..., formant_shift=)`; with `--batch` on the device, one launch over a wave's
frames).  Like `--transpose-key` it reaches the .synth.wav output only: the .diff.wav output is the input waveform
filtered by the converter's difference, which this option leaves alone.
`--mlpg-em N` converts the spectrum, for both outputs, by EM over soft mixture posteriors (Toda et al. 2007) instead
of with one arg-max mixture per frame: every mixture of a frame weighs in with its posterior, and the posteriors are
re-estimated N times from the source frame and the trajectory solved last (`convert(..., em=N)`; with `--batch`
kwy_convert_mcep_em_batch_dev).  The statistics of `--ms` and the re-alignment of `--align-iterations` keep the arg-max
conversion.
`--diff-filter fft` writes the .diff.wav outputs through the frame-parallel FFT form of the differential filter instead
of the MLSA filter (`convert(..., diff_filter='fft')`, kwiiyatta_amd.apply_diff_filter; with `--batch`
kwy_mcep_filter_fft_batch_dev over all frames of a wave's files): the mel-cepstral filter the MLSA filter approximates,
applied to every frame through its frequency response, the outputs of neighbouring frames' filters crossfaded where the
MLSA filter interpolates their coefficients.  Its time shrinks with the GPU where the MLSA recursion's does not (about
0.5 us per sample of the longest file, whatever runs beside it).  The default, `mlsa`, is the reference's filter,
unchanged; the .synth.wav outputs do not depend on the option.
`--keep-power` repairs the loudness of both outputs: the conversion keeps the source's c0, but c0 is not the power --
a frame's energy is the mean of |H|^2, and the converted c1.. move it by several dB -- so c0 of every converted frame
is shifted until the frame has the energy of the source frame (`convert(..., keep_power=True)`, backend.power,
kwy_mcpower.hip; with `--batch` kwy_mcep_postfilter_batch_dev inside the wave).  `--postfilter BETA` (within [0, 1])
sharpens the over-smoothed envelope frame by frame with the mel-cepstral formant emphasis of the HTS vocoder and SPTK's
mcpf and keeps the frame's energy -- the source's with `--keep-power`, its own otherwise.  Both run after `--ms`, `--gv`
and `--mlpg-gv`.  For the .diff.wav output the corrected c0 travels as its difference from the source's c0 in column 0
of the differential mel-cepstrum, and the differential filter takes that column into account
(`apply_diff_filter(..., use_c0=True)`).  Neither option writes anything to the converter model.
`--convert-aperiodicity` renders the .synth.wav outputs on the source's aperiodicity converted to the target speaker's:
training fits a second mixture (`--ap-components`, kept in the converter model) on the band aperiodicity of the voiced
frames of the same aligned pairs, and `convert(..., convert_ap=True)` decodes the converted bands over the voiced frames
of the analysed aperiodicity (converter.convert_aperiodicity, backend.bap, kwy_bap.hip).  It needs a sampling rate of
12 kHz or more and does not reach the .diff.wav output (a filtered waveform); with `--batch` the three calls run on
the wave's side stream behind D4C (corpus.convert_batch(ap_gmm=...))."""
import pathlib
from types import SimpleNamespace

import numpy as np

from ._convert_options import ConvertOptions, filled, takes_options

OUTPUTS = (('diff', True), ('synth', False))          # suffix, differential?

# what a command can ask of a conversion, under the names of its arguments (Config), and what it asks by default
COMMAND_OPTIONS = dict(convert_f0=False, transpose_key=0.0, gv=0.0, ms=0.0, formant_shift=0.0, mlpg_em=None, mlpg_gv=None,
                       diff_filter='mlsa', postfilter=0.0, keep_power=False, convert_ap=False)


def driver_options(converter, asked):
    """the keywords of the device drivers (corpus.ConvertOptions) for what a command `asked` of this converter: its
    statistics where an option needs them, and of the others those that are not the drivers' defaults"""
    plain = dict(formant_ratio=2.0 ** (asked.formant_shift / 12), mlpg_em=asked.mlpg_em, mlpg_gv=asked.mlpg_gv,
                 diff_filter=asked.diff_filter, postfilter_beta=asked.postfilter, keep_power=asked.keep_power)
    on = {name: v for name, v in plain.items() if v != ConvertOptions.DEFAULTS[name]}
    on.update(f0_stats=converter.f0_stats if asked.convert_f0 else None, transpose_key=asked.transpose_key)
    if asked.gv > 0:
        on.update(gv_stats=converter.gv_stats, gv_strength=asked.gv)
    if asked.ms > 0:
        on.update(ms_stats=converter.ms_stats, ms_length=converter.ms_length, ms_strength=asked.ms)
    if asked.mlpg_gv is not None:
        on.update(gv_stats=converter.gv_stats, gv_var=converter.gv_var)
    return on


@takes_options(defaults=COMMAND_OPTIONS)
def convert(conf, converter, src_path, diffvc=True, **options):
    """one converted waveform.  The file is analysed afresh per call, as the reference does.  convert_f0 /
    transpose_key: the f0 of the synthesised output through converter.convert_f0 (the differential output is the
    input waveform filtered, its pitch stays the source's).  gv > 0: the converted mel-cepstrum through the
    global-variance postfilter of that strength (converter.convert(gv=...), either output); ms > 0: through the
    modulation-spectrum postfilter first (converter.convert(ms=...)).  A converter trained on
    pitch-shifted sources (converter.source_f0_rate != 1) gets the file's waveform shifted the same way.
    formant_shift != 0 (semitones): the converted envelope of the synthesised output warped along frequency by
    2 ** (formant_shift / 12) (Feature.shift_formants); the differential output ignores it.
    mlpg_em=N: the EM trajectory conversion with N re-estimations (converter.convert(em=N), either output).
    mlpg_gv=N: parameter generation considering the global variance, N steps (converter.convert(mlpg_gv=N), either
    output).
    diff_filter: the filter of the differential output, 'mlsa' (apply_mlsa_filter) or 'fft'
    (apply_diff_filter(method='fft')); the synthesised output ignores it.
    postfilter > 0 / keep_power: the formant emphasis of that beta and / or the source's frame energies on the converted
    mel-cepstrum (converter.convert(postfilter=..., keep_power=...), either output); the differential filter then runs
    with use_c0=True, on the change of c0 the conversion hands over in column 0.
    convert_ap: the synthesised output on the aperiodicity converted by the converter's band mixture
    (converter.convert_aperiodicity; needs a converter trained with ap_model=True at 12 kHz or more); the differential
    output is a filtered waveform and keeps the source's aperiodic component."""
    import kwiiyatta_amd as k
    o = SimpleNamespace(**filled(options, COMMAND_OPTIONS))
    if not 0.0 <= o.postfilter <= 1.0:          # (raises before the file is read)
        raise ValueError(f'postfilter: beta {o.postfilter!r} is outside [0, 1]')
    if o.convert_ap:                            # (raises before the file is read)
        check_convert_ap(converter)
    power = o.postfilter > 0 or o.keep_power
    # converter.convert's keywords: (value, whether it is on) -- an option that is off is not handed over
    stages = dict(gv=(o.gv, o.gv > 0), ms=(o.ms, o.ms > 0), em=(o.mlpg_em, o.mlpg_em is not None),
                  mlpg_gv=(o.mlpg_gv, o.mlpg_gv is not None), postfilter=(o.postfilter, power),
                  keep_power=(o.keep_power, power))
    source = analyze_source(conf, converter, src_path)
    converted = converter.convert(source.mel_cepstrum, diff=diffvc, **{name: v for name, (v, on) in stages.items() if on})
    if diffvc:
        use_c0 = dict(use_c0=True) if power else {}
        if o.diff_filter == 'mlsa':
            return k.apply_mlsa_filter(source, converted, **use_c0)
        return k.apply_diff_filter(source, converted, method=o.diff_filter, **use_c0)
    rendered = k.feature(source)
    rendered.mel_cepstrum = converted                   # takes over from the analysed envelope
    if o.convert_f0 or o.transpose_key != 0:
        from .backend import f0 as f0map
        stats = converter.f0_stats if o.convert_f0 else None          # (converter.convert_f0 without the statistics)
        rendered.f0 = f0map.map_f0(np.ascontiguousarray(source.f0, dtype=np.float64), rendered.fs, stats=stats,
                                   key=o.transpose_key)
    if o.formant_shift != 0:
        rendered.shift_formants(2.0 ** (o.formant_shift / 12))
    if o.convert_ap:
        rendered.aperiodicity = converter.convert_aperiodicity(source)
    return rendered.synthesize()


def check_convert_ap(converter):
    """what convert_ap needs of a converter, without reading a file: a sampling rate with an aperiodicity band and the
    band mixture (ValueError otherwise)"""
    from .backend import bap
    bap.check_rate(converter.fs)
    if getattr(converter, 'ap_converter', None) is None:
        raise ValueError('convert_ap: the converter has no band-aperiodicity mixture (train it with ap_model=True)')


def analyze_source(conf, converter, path):
    """the analyzer of a file to convert: the file as it is, or -- for a converter trained on pitch-shifted sources --
    its waveform through the shifter at the converter's rate (Config.analyze_source, which training uses too)"""
    import kwiiyatta_amd as k
    rate = getattr(converter, 'source_f0_rate', 1.0)
    if rate == 1:
        return conf.create_analyzer(path, Analyzer=k.analyze_wav)
    return conf.analyze_source(path, rate)


def shift_waves_dev(waves, fs, rate, device_index=0):
    """the waveforms of a batch (numpy arrays) through ONE kwy_pitch_shift_batch_dev call: float64 device tensors, which
    the corpus drivers take as they are"""
    import torch
    from . import _lib
    from .backend import pitch
    dev = torch.device('cuda', device_index)
    xs = [torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(dev) for w in waves]
    ys = [torch.empty_like(x) for x in xs]
    torch.cuda.current_stream(dev).synchronize()          # (the uploads, before the library's own stream reads them)
    ctx = _lib.default_context()
    pitch.shift_pitch_batch_dev(ctx, xs, ys, fs, rate)
    ctx.sync()                                            # (the drivers run on streams of their own)
    return ys


class _Pcm16:
    """the 16-bit samples of a finished waveform as the batch path hands them over: `save` writes them as they are
    (what Wavdata.save(normalize=True) would write for the waveform -- kwy_finish_pcm16_batch_dev)"""

    def __init__(self, fs, pcm):
        self.fs, self.pcm = fs, pcm

    def save(self, wav):
        from scipy.io import wavfile
        wavfile.write(wav, self.fs, self.pcm)


@takes_options(defaults=COMMAND_OPTIONS)
def convert_synth_batch(conf, converter, paths, diffvc=False, **options):
    """{(path, differential?): object with .save(file)} of the .synth.wav outputs -- with diffvc=True of the .diff.wav
    outputs too.  Files whose sampling rate or frame period differ from the converter's go through `convert` one by
    one (the batch path has no resampling stage).  The others go through the device WAV IN -> PCM OUT: the pitch shift of
    a converter trained on shifted sources (all files of the batch in one call, the shifted waveforms stay on the
    device), f0 (DIO +
    StoneMask), analysis, conversion, synthesis / the MLSA filter of the differential conversion, the post-step of
    `synthesize` and `save`'s normalisation and 16-bit truncation all run on the GPU
    (corpus.convert_batch(pcm=True, diff=...)); the host reads the wav files and writes 2 bytes per sample.
    convert_f0 / transpose_key: the .synth.wav outputs on the mapped f0 (as `convert` does), mapped on the device.
    gv > 0 / ms > 0: both outputs from the postfiltered mel-cepstra (as `convert` does), filtered on the device; a file
    longer than the converter's ms_length goes through `convert`, which names it.
    formant_shift != 0: the .synth.wav outputs from the warped converted envelopes (as `convert` does), warped on the
    device (corpus.convert_batch(formant_ratio=...)).
    mlpg_em=N: both outputs from EM trajectory conversions (as `convert` does; corpus.convert_batch(mlpg_em=N)).
    mlpg_gv=N: both outputs from GV-considering parameter generation (as `convert` does;
    corpus.convert_batch(mlpg_gv=N)).
    diff_filter='fft': the .diff.wav outputs through the frame-parallel FFT filter instead of the MLSA filter
    (corpus.convert_batch(diff_filter='fft'): all frames of a wave's files in one launch).
    postfilter > 0 / keep_power: both outputs from the emphasised / power-corrected mel-cepstra (as `convert` does;
    corpus.convert_batch(postfilter_beta=..., keep_power=...)).
    convert_ap: the .synth.wav outputs on the converted aperiodicity (as `convert` does; corpus.convert_batch(ap_gmm=...))."""
    import kwiiyatta_amd as k
    from . import corpus
    o = SimpleNamespace(**filled(options, COMMAND_OPTIONS))
    corpus._postfilter_beta(o.postfilter)          # (raises before any file is read)
    if o.convert_ap:
        check_convert_ap(converter)               # (raises before any file is read)
    if o.mlpg_gv is not None:
        converter.gv_ascent_statistics()          # (raises before any file is read)
    from ._lib import lib
    from .converter.delta import DeltaFeatureConverter
    out, batch = {}, []
    period = next((s.frame_period for s in _stages(converter) if isinstance(s, DeltaFeatureConverter)), None)
    for path in paths:
        a = conf.create_analyzer(path, Analyzer=k.analyze_wav)
        # (the frame count ConvertWave itself takes for a bare waveform -- the same call on the same number of samples,
        # which the pitch shifter keeps -- so a file that passes here fits there)
        too_long = o.ms > 0 and converter.ms_length is not None and \
            lib.kwy_dio_frames(int(a.fs), len(a.wavdata.data), float(a.frame_period)) > converter.ms_length
        if a.fs != converter.fs or a.mel_cepstrum_order != converter.order or too_long or \
                (period is not None and a.frame_period != period):
            out[path, False] = convert(conf, converter, path, diffvc=False, **options)
        else:
            batch.append((path, a))
    if batch:
        fs = batch[0][1].fs
        waves = [a.wavdata.data for _, a in batch]
        rate = getattr(converter, 'source_f0_rate', 1.0)
        if rate != 1:
            waves = shift_waves_dev(waves, fs, rate)
        res = corpus.convert_batch(waves, fs, converter.gmm, order=converter.order,
                                   frame_period=float(batch[0][1].frame_period), pcm=True, diff=diffvc,
                                   ap_gmm=converter.ap_converter.gmm if o.convert_ap else None,
                                   f0_estimator=getattr(conf, 'f0_estimator', 'dio'), **driver_options(converter, o))
        for k, (path, a) in enumerate(batch):
            out[path, False] = _Pcm16(fs, res[1][k].cpu().numpy())
            if diffvc:
                out[path, True] = _Pcm16(fs, res[3][k].cpu().numpy())
    return out


def _stages(converter):
    stage = converter
    while stage is not None:
        yield stage
        stage = getattr(stage, '__dict__', {}).get('base')


def main():
    import kwiiyatta_amd as k
    conf = k.Config()
    conf.add_argument('--result-dir', type=str, help='Path to write result wav files')
    conf.add_argument('files', type=str, nargs='+', help='Wav files to convert voice')
    conf.add_argument('--no-diffvc', action='store_true', help='Write only the .synth.wav outputs')
    conf.add_argument('--batch', action='store_true',
                      help='Render the outputs of all files through the GPU-resident batch path')
    conf.add_argument('--convert-f0', action='store_true',
                      help='Map the f0 of the .synth.wav outputs to the target speaker (log-f0 mean and deviation of '
                           'the training data, kept in the converter model)')
    conf.add_transpose_key_argument()
    conf.add_formant_shift_argument()
    conf.add_gv_argument()
    conf.add_ms_argument()
    conf.add_mlpg_em_argument()
    conf.add_mlpg_gv_argument()
    conf.add_diff_filter_argument()
    conf.add_power_arguments()
    conf.add_aperiodicity_arguments()
    conf.add_converter_arguments()          # (--source-f0-rate among them)
    conf.parse_args()
    conf.convert_ap = conf.convert_aperiodicity
    converter = conf.train_converter(use_delta=True, f0_stats=conf.convert_f0, gv_stats=conf.gv > 0,
                                     ms_stats=conf.ms > 0, **(dict(gv_var=True) if conf.mlpg_gv is not None else {}),
                                     **(dict(ap_model=True) if conf.convert_ap else {}))
    asked = {name: getattr(conf, name) for name in COMMAND_OPTIONS}
    batched = convert_synth_batch(conf, converter, [pathlib.Path(n) for n in conf.files], diffvc=not conf.no_diffvc,
                                  **asked) if conf.batch else {}
    for name in conf.files:
        wav_path = pathlib.Path(name)
        stem = wav_path if conf.result_dir is None else pathlib.Path(conf.result_dir) / wav_path.name
        stem.parent.mkdir(parents=True, exist_ok=True)
        for suffix, differential in OUTPUTS:
            if differential and conf.no_diffvc:
                continue
            out = stem.with_suffix(f'.{suffix}.wav')
            print(f'{suffix} MLPG: {out!s}')
            if (wav_path, differential) in batched:
                batched[wav_path, differential].save(out)
            else:
                convert(conf, converter, wav_path, diffvc=differential, **asked).save(out)


if __name__ == '__main__':
    main()
