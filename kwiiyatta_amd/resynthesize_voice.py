"""`kwiieiya`: analyse a wav file and synthesise it again -- optionally through its mel-cepstrum (--mcep), at another
sampling rate (--result-fs), or on the timing and f0 of a second recording (--carrier; with --diffvc the carrier's
own waveform is filtered towards the source's spectrum instead of being re-synthesised).  Command line of the
reference's kwiiyatta/resynthesize_voice.py; its Qt dialog (started when no source file is given) is not part of
this build, but its key transposition is: --transpose-key SEMITONES multiplies the f0 by 2 ** (SEMITONES / 12)
after the carrier and --mcep steps (kwiiyatta/view/qt/kwiieiya.py:152-155).  --diffvc returns before that step in
the dialog, so the two together are refused.
An addition to the reference's options: --formant-shift SEMITONES warps the spectral envelope along frequency by
2 ** (SEMITONES / 12) (Feature.shift_formants: above 0 the formants move up, a shorter vocal tract; the pitch and the
aperiodicity stay), after the carrier and --mcep steps, beside the transposition and before --result-fs.  With
--diffvc the shift composes in two ways.  --carrier --diffvc: the source's envelope on the carrier's frames is warped
BEFORE the difference to the carrier's mel-cepstrum is taken, so the carrier's waveform is filtered towards the shifted
spectrum.  --diffvc without a carrier (ignored at shift 0, as it always was): the source's OWN waveform goes through the
MLSA filter of mel-cepstrum(warped envelope) - mel-cepstrum(envelope) -- a formant shift with no resynthesis at all.
--diff-filter fft runs every --diffvc path above -- with and without --carrier, the --formant-shift difference
included -- through the frame-parallel FFT form of the filter (kwiiyatta_amd.apply_diff_filter(method='fft')) instead
of the MLSA recursion: the same mel-cepstral filter, every frame filtered by a transform of its own and neighbouring
frames' outputs crossfaded, in milliseconds for a file of minutes.  The default, mlsa, is the reference's filter."""
import copy
import pathlib


def _diff_filter(conf, wav, difference):
    """the --diffvc filter the options ask for: the MLSA filter unless --diff-filter names another"""
    import kwiiyatta_amd as k
    method = getattr(conf, 'diff_filter', 'mlsa')
    if method == 'mlsa':
        return k.apply_mlsa_filter(wav, difference)
    return k.apply_diff_filter(wav, difference, method=method)


def render(conf, source):
    """the result waveform for the parsed options"""
    import kwiiyatta_amd as k
    shift = getattr(conf, 'formant_shift', 0.0)
    ratio = 2.0 ** (shift / 12)
    if conf.carrier is None:
        picture = k.feature(source)
        if conf.diffvc and shift != 0:                   # the source's own waveform filtered by the warp's difference
            plain = picture.mel_cepstrum.data
            picture.shift_formants(ratio)
            difference = copy.copy(picture.mel_cepstrum)
            difference.data = difference.data - plain
            return _diff_filter(conf, source.wavdata, difference)
    else:
        carrier = conf.create_analyzer(conf.carrier, Analyzer=k.analyze_wav)
        picture = k.align(source, carrier)               # the source's features on the carrier's frames
        if conf.diffvc:
            if shift != 0:
                picture.shift_formants(ratio)
            difference = copy.copy(picture.mel_cepstrum)
            difference.data -= carrier.mel_cepstrum.data
            return _diff_filter(conf, carrier.wavdata, difference)
        picture.f0 = carrier.f0
    if conf.mcep:
        picture.extract_mel_cepstrum()
        picture.spectrum_envelope = None                 # from here on the mel-cepstrum is the envelope
    if shift != 0:
        picture.shift_formants(ratio)
    if conf.transpose_key != 0:
        import numpy as np
        from .backend import f0 as f0map
        fs = conf.result_fs if conf.result_fs is not None else picture.fs
        picture.f0 = f0map.map_f0(np.ascontiguousarray(picture.f0, dtype=np.float64), fs, key=conf.transpose_key)
    if conf.result_fs is not None:
        picture.resample(conf.result_fs)
    return picture.synthesize()


def main():
    import kwiiyatta_amd as k
    conf = k.Config()
    conf.add_argument('source', type=str, default=None, nargs='?', help='Source wav file of voice resynthesis')
    conf.add_argument('--result-dir', type=str, help='Path to write result wav files')
    conf.add_argument('--mcep', action='store_true', help='Use mel-cepstrum to resynthesize')
    conf.add_argument('--play', action='store_true', help='Play result wavform')
    conf.add_argument('--no-save', action='store_true', help='Not to write result wav file, and play wavform')
    conf.add_argument('--carrier', type=str, help='Wav file to use for carrier')
    conf.add_argument('--diffvc', action='store_true', help='Use difference MelCepstrum synthesis')
    conf.add_argument('--result-fs', type=int, help='Result waveform sampling rate')
    conf.add_transpose_key_argument()
    conf.add_formant_shift_argument()
    conf.add_diff_filter_argument()
    conf.parse_args()
    if conf.source is None:
        conf.parser.error('a source wav file is required (the Qt dialog of the reference is not part of this build)')
    if conf.diffvc and conf.transpose_key != 0:
        conf.parser.error('--transpose-key cannot be combined with --diffvc (the carrier waveform is filtered, not '
                          're-synthesised: its pitch stays)')
    source_path = pathlib.Path(conf.source).resolve()
    wav = render(conf, conf.create_analyzer(source_path, Analyzer=k.analyze_wav))
    if not conf.no_save:
        target = (source_path.with_suffix('.resynth.wav') if conf.result_dir is None
                  else pathlib.Path(conf.result_dir) / source_path.name)
        target.parent.mkdir(parents=True, exist_ok=True)
        wav.save(target)
    if conf.play or conf.no_save:
        wav.play()


if __name__ == '__main__':
    main()
