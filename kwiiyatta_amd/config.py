"""Options shared by the command-line tools, and the factories that apply them.  API of kwiiyatta.config.Config
(/root/reference/kwiiyatta/config.py): the options are parsed INTO the Config object (it is the argparse namespace),
analyzers and converters are created through it so that frame period, mel-cepstrum order, component count and seed
follow the command line."""
import argparse
import functools
import math
import pathlib
import sys

import numpy as np

from .backend.ms import LENGTHS as MS_LENGTHS

class _Unset(int):
    """the default of an option whose presence on the command line matters: the number it stands for, told apart
    from a typed one by its class"""


VOCODER_OPTIONS = (
    ('--frame-period', dict(type=int, default=5, help='Frame period milli-seconds of vocoder')),
    ('--mcep-order', dict(type=int, default=24, help='Mel-cepstrum order for spectrum envelope')),
    # an addition to the reference's options: the coarse f0 track that StoneMask refines
    ('--f0-estimator', dict(choices=('dio', 'pyin'), default='dio',
                            help='Coarse f0 estimator of the analysis: dio (WORLD\'s), or pyin, probabilistic YIN with '
                                 'a Viterbi pass over the utterance; a converter model keeps the one it was trained with')),
)
CONVERTER_OPTIONS = (
    ('--source', dict(type=str, help='Source data-set path of voice conversion')),
    ('--target', dict(type=str, help='Target data-set path of voice conversion')),
    ('--max-files', dict(type=int, help='File num to train feature converter')),
    ('--skip-files', dict(type=int, help='Skip file num to train feature converter')),
    ('--mcep-fs', dict(type=int, help='Sampling rate of training mel cepstrum')),
    ('--converter-components', dict(type=int, default=_Unset(64), help='Components num for feature converter')),
    ('--converter-seed', dict(type=int, help='Random seed for feature converter')),
    # an addition to the reference's options: keep the trained converter between runs
    ('--converter-model', dict(type=str, help='File of the trained converter: loaded when it exists (no training, '
                                              '--source/--target not needed), written after training otherwise')),
)

SOURCE_F0_RATE_RANGE = (0.5, 2.0)


def source_f0_rate(text):
    """--source-f0-rate: 'auto', or a ratio within the pitch shifter's range"""
    if text == 'auto':
        return text
    try:
        rate = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid f0 ratio: {text!r} (a number or 'auto')") from None
    lo, hi = SOURCE_F0_RATE_RANGE
    if not lo <= rate <= hi:                # (false for nan)
        raise argparse.ArgumentTypeError(f'{text} is outside [{lo}, {hi}]')
    return rate


# an addition to the reference's options, among the converter's: it shapes the training set as well as the conversion
CONVERTER_OPTIONS += (
    ('--source-f0-rate', dict(type=source_f0_rate, default=None, metavar='RATE|auto',
                              help='Shift the pitch of every source waveform by this ratio (WSOLA + resampling, '
                                   'within [0.5, 2.0]) before it is analysed, in training and in conversion, so that '
                                   'the differential output takes the target\'s pitch as well; auto: the ratio of the '
                                   'two speakers\' mean voiced log-f0 over the training files; kept in the converter '
                                   'model (default 1: no shift)')),
)


ALIGN_ITERATIONS_RANGE = (0, 10)


def align_iterations(text):
    """--align-iterations: how often the training set is aligned again, an integer within [0, 10]"""
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'invalid iteration count: {text!r}') from None
    lo, hi = ALIGN_ITERATIONS_RANGE
    if not lo <= n <= hi:
        raise argparse.ArgumentTypeError(f'{text} is outside [{lo}, {hi}]')
    return n


# an addition to the reference's options (it aligns its training set once)
CONVERTER_OPTIONS += (
    ('--align-iterations', dict(type=align_iterations, default=None, metavar='N',
                                help='Align the training set again N times (within [0, 10]): each time every pair is '
                                     'aligned with the source mel-cepstrum converted by the converter fitted so far, '
                                     'the joint matrix is rebuilt along the new paths and the mixture refitted; kept '
                                     'in the converter model (default 0: aligned once, as the reference does)')),
)


NONPARALLEL_RANGE = (0, 64)      # MelCepstrumFeatureConverter.NONPARALLEL_RANGE
NONPARALLEL_DEFAULT = 6          # MelCepstrumFeatureConverter.NONPARALLEL_DEFAULT


def nonparallel(text):
    """--nonparallel: the INCA iterations of a training without parallel data, an integer within [0, 64]"""
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'invalid iteration count: {text!r}') from None
    lo, hi = NONPARALLEL_RANGE
    if not lo <= n <= hi:
        raise argparse.ArgumentTypeError(f'{text} is outside [{lo}, {hi}]')
    return n


# an addition to the reference's options (it trains on parallel data only)
CONVERTER_OPTIONS += (
    ('--nonparallel', dict(type=nonparallel, nargs='?', const=NONPARALLEL_DEFAULT, default=None, metavar='N',
                           help='Train without parallel data (INCA, Erro et al. 2010): --source and --target need no '
                                'common file names, --skip-files / --max-files pick the training files of each '
                                'directory on its own.  Every speech frame of one side is paired with its nearest '
                                'frame of the other (static and delta mel-cepstrum, voicing), the mixture fitted on '
                                'the pairs, the source converted and the search repeated N times (within [0, 64], '
                                f'{NONPARALLEL_DEFAULT} when omitted); kept in the converter model.  Goes with neither '
                                '--align-iterations nor --convert-aperiodicity')),
)


COVARIANCE_STRUCTURES = ('full', 'block_diag')

# an addition to the reference's options (its mixtures have full covariances)
CONVERTER_OPTIONS += (
    ('--converter-covariance', dict(choices=COVARIANCE_STRUCTURES, default=None,
                                    help='Structure of the mixture\'s covariances: full matrices, or block_diag -- '
                                         'diagonal source, target and cross blocks (Toda et al. 2007), 3 D / 2 numbers '
                                         'per component instead of D (D + 1) / 2, for training sets of a few '
                                         'sentences; kept in the converter model (default full, as the reference '
                                         'does)')),
)


# an addition to the reference's options (it has no postfilter)
CONVERTER_OPTIONS += (
    ('--ms-length', dict(type=int, choices=MS_LENGTHS, default=None, metavar='L',
                         help='Transform length of the modulation-spectrum statistics learnt with --ms, in frames (one '
                              f'of {", ".join(map(str, MS_LENGTHS))}; default 4096); no training or converted utterance '
                              'may be longer; kept in the converter model, which decides when one is loaded; only '
                              'convert_voice --ms uses it')),
)


def transpose_key(text):
    """--transpose-key: semitones, within the reference dialog's spin box range (view/qt/ui/kwiieiya.ui:262-280)"""
    try:
        key = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'invalid semitone value: {text!r}') from None
    if not -99.99 <= key <= 99.99:
        raise argparse.ArgumentTypeError(f'{text} semitones is outside [-99.99, 99.99]')
    return key


TRANSPOSE_KEY_OPTION = ('--transpose-key', dict(type=transpose_key, default=0.0, metavar='SEMITONES',
                                                help='Transpose the synthesised voice by this many semitones '
                                                     '(f0 * 2 ** (SEMITONES / 12); [-99.99, 99.99])'))


FORMANT_SHIFT_RANGE = (-12.0, 12.0)


def formant_shift(text):
    """--formant-shift: semitones within [-12, 12], the range of the envelope warp (a ratio within [0.5, 2])"""
    try:
        semitones = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'invalid semitone value: {text!r}') from None
    lo, hi = FORMANT_SHIFT_RANGE
    if not lo <= semitones <= hi:           # (false for nan)
        raise argparse.ArgumentTypeError(f'{text} semitones is outside [{lo:g}, {hi:g}]')
    return semitones


FORMANT_SHIFT_OPTION = ('--formant-shift', dict(type=formant_shift, default=0.0, metavar='SEMITONES',
                                                help='Move the formants of the synthesised voice by this many semitones '
                                                     '(the spectral envelope warped along frequency by 2 ** (SEMITONES '
                                                     '/ 12): above 0 a shorter vocal tract; [-12, 12]); the pitch '
                                                     'stays'))


def gv_strength(text):
    """--gv: the strength of the global-variance postfilter, within [0, 1]"""
    try:
        strength = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'invalid strength: {text!r}') from None
    if not 0.0 <= strength <= 1.0:
        raise argparse.ArgumentTypeError(f'{text} is outside [0, 1]')
    return strength


GV_OPTION = ('--gv', dict(type=gv_strength, nargs='?', const=1.0, default=0.0, metavar='STRENGTH',
                          help='Global-variance postfilter on the converted mel-cepstrum: stretch every trajectory '
                               'about its mean towards the variance of the target speaker (kept in the converter '
                               'model); STRENGTH within [0, 1], 1 when omitted'))


MS_OPTION = ('--ms', dict(type=gv_strength, nargs='?', const=1.0, default=0.0, metavar='STRENGTH',
                          help='Modulation-spectrum postfilter on the converted mel-cepstrum: move every modulation '
                               'frequency of every trajectory from the statistics of converted speech to those of the '
                               'target speaker (both kept in the converter model); runs before --gv; STRENGTH within '
                               '[0, 1], 1 when omitted'))


MLPG_EM_RANGE = (0, 16)      # KWY_MLPG_EM_MAX (include/kwy.h)


def mlpg_em(text):
    """--mlpg-em: the re-estimations of the mixture posteriors, an integer within [0, 16]"""
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'invalid iteration count: {text!r}') from None
    lo, hi = MLPG_EM_RANGE
    if not lo <= n <= hi:
        raise argparse.ArgumentTypeError(f'{text} is outside [{lo}, {hi}]')
    return n


MLPG_EM_OPTION = ('--mlpg-em', dict(type=mlpg_em, default=None, metavar='N',
                                    help='EM trajectory conversion over soft mixture posteriors: weigh every mixture '
                                         'of a frame by its posterior instead of picking the likeliest one, and '
                                         're-estimate the posteriors N times from the source frame and the trajectory '
                                         'solved last (Toda et al. 2007); N within [0, 16], 0: one solve under the '
                                         'source-only posteriors (default: one arg-max mixture per frame, as the '
                                         'reference does)'))


MLPG_GV_RANGE = (0, 256)     # KWY_MLPG_GV_MAX (include/kwy.h)


def mlpg_gv(text):
    """--mlpg-gv: the conjugate-gradient steps of the GV-considering parameter generation, an integer within [0, 256]"""
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'invalid iteration count: {text!r}') from None
    lo, hi = MLPG_GV_RANGE
    if not lo <= n <= hi:
        raise argparse.ArgumentTypeError(f'{text} is outside [{lo}, {hi}]')
    return n


MLPG_GV_OPTION = ('--mlpg-gv', dict(type=mlpg_gv, default=None, metavar='N',
                                    help='Parameter generation considering the global variance: maximise the '
                                         'likelihood of the trajectory and of its global variance jointly (Toda et '
                                         'al. 2007) by N conjugate-gradient steps from the linearly scaled '
                                         'trajectory; N within [0, 256], 0: that scaled trajectory (what --gv 1 '
                                         'gives).  Uses the global-variance statistics of the converter model; goes '
                                         'with --mlpg-em, not with --gv or --ms'))


DIFF_FILTER_OPTION = ('--diff-filter', dict(choices=('mlsa', 'fft'), default='mlsa',
                                            help='The filter of the differential outputs: mlsa, the MLSA filter of the '
                                                 'reference (serial in the sample), or fft, the same mel-cepstral '
                                                 'filter applied frame by frame through its frequency response, all '
                                                 'frames in parallel, neighbouring frames crossfaded'))


POWER_OPTIONS = (
    ('--postfilter', dict(type=gv_strength, default=0.0, metavar='BETA',
                          help='Mel-cepstral formant-emphasis postfilter on the converted mel-cepstrum, frame by frame '
                               '(the beta of the HTS vocoder and of SPTK mcpf), the frame energy kept; BETA within '
                               '[0, 1], 0 (the default) is off; runs after --ms, --gv and --mlpg-gv')),
    ('--keep-power', dict(action='store_true',
                          help='Shift c0 of every converted frame until the frame has the energy of the source frame: '
                               'c0 is not the power, converting c1.. at a fixed c0 moves it by several dB')),
)


def ap_components(text):
    """--ap-components: the components of the band-aperiodicity mixture, a positive integer"""
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'invalid component count: {text!r}') from None
    if n < 1:
        raise argparse.ArgumentTypeError(f'{text} is not a positive component count')
    return n


# an addition to the reference's options (it renders a converted voice with the source's aperiodicity)
APERIODICITY_OPTIONS = (
    ('--convert-aperiodicity', dict(action='store_true',
                                    help='Convert the aperiodicity as well: a second joint-density mixture on the band '
                                         'aperiodicity of the voiced frames of the same aligned pairs (Ohtani et al. 2006), '
                                         'kept in the converter model; the converted bands replace the voiced frames of '
                                         'the analysed aperiodicity.  Needs a sampling rate of 12 kHz or more.  Only the '
                                         'synthesised output (.synth.wav) changes: the differential output (.diff.wav) is '
                                         'a filtered waveform and keeps the source\'s aperiodic component')),
    ('--ap-components', dict(type=ap_components, default=16, metavar='N',
                             help='Components of the band-aperiodicity mixture trained with --convert-aperiodicity '
                                  '(default 16); a loaded converter model decides')),
)


CONVERTERS = ('gmm', 'exemplar')
EXEMPLAR_FFT_SIZES = (256, 512, 1024, 2048, 4096)        # converter.exemplar.FFT_SIZES
EXEMPLARS_RANGE = (1, 8192)                              # backend.nmf.MAX_ATOMS
EXEMPLAR_ITERATIONS_RANGE = (0, 1000)                    # backend.nmf.MAX_ITERATIONS


def _int_within(lo, hi, what):
    def parse(text):
        try:
            n = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f'invalid {what}: {text!r}') from None
        if not lo <= n <= hi:
            raise argparse.ArgumentTypeError(f'{text} is outside [{lo}, {hi}]')
        return n
    return parse


def exemplar_sparsity(text):
    """--exemplar-sparsity: the weight of the L1 term of the activations, finite and >= 0"""
    try:
        value = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'invalid sparsity: {text!r}') from None
    if not (value >= 0 and math.isfinite(value)):
        raise argparse.ArgumentTypeError(f'{text} is not a finite sparsity >= 0')
    return value


# an addition to the reference's options (its converter is the joint-density mixture)
CONVERTER_OPTIONS += (
    ('--converter', dict(choices=CONVERTERS, default='gmm',
                         help='The spectral converter: gmm, the joint-density mixture with MLPG of the reference, or '
                              'exemplar -- the aligned training frames themselves as two coupled dictionaries, a source '
                              'frame explained as a sparse non-negative combination of source exemplars (KL-NMF '
                              'activations) and the same activations applied to the paired target exemplars; nothing '
                              'is fitted, there is no component count; kept in the converter model.  exemplar goes '
                              'with none of --mlpg-em, --mlpg-gv, --converter-covariance, --converter-components, '
                              '--convert-aperiodicity, --nonparallel and --batch')),
    ('--exemplars', dict(type=_int_within(*EXEMPLARS_RANGE, 'exemplar count'), default=None, metavar='A',
                         help='Exemplars the dictionary keeps at the most (within [1, 8192]): of R > A aligned training '
                              'rows the rows floor(i R / A); a loaded converter model decides')),
    ('--exemplar-iterations', dict(type=_int_within(*EXEMPLAR_ITERATIONS_RANGE, 'iteration count'), default=None,
                                   metavar='N', help='Multiplicative updates of the activations (within [0, 1000]); a '
                                                     'loaded converter model decides')),
    ('--exemplar-sparsity', dict(type=exemplar_sparsity, default=None, metavar='L',
                                 help='Weight of the L1 term on the activations (>= 0); a loaded converter model '
                                      'decides')),
    ('--exemplar-fft', dict(type=int, choices=EXEMPLAR_FFT_SIZES, default=None,
                            help='Transform length of the envelopes the activations work on (FFT / 2 + 1 bins); a '
                                 'loaded converter model decides')),
)

# what does not go with --converter exemplar: (attribute, whether it is asked for, flag, why)
EXEMPLAR_CONFLICTS = (
    ('mlpg_em', lambda v: v is not None, '--mlpg-em', 'it re-estimates the posteriors of a mixture'),
    ('mlpg_gv', lambda v: v is not None, '--mlpg-gv', 'it ascends the likelihood of a mixture\'s trajectory'),
    ('converter_covariance', lambda v: v is not None, '--converter-covariance', 'there are no covariances'),
    ('converter_components', lambda v: v is not None and not isinstance(v, _Unset), '--converter-components',
     'there are no components'),
    ('convert_aperiodicity', bool, '--convert-aperiodicity', 'the band conversion is a mixture'),
    ('nonparallel', lambda v: v is not None, '--nonparallel', 'its search runs on the delta features of a mixture stack'),
    ('batch', bool, '--batch', 'the lockstep drivers take a mixture; the exemplar stage is not wired into them yet'),
)
EXEMPLAR_OPTIONS = ('exemplars', 'exemplar_iterations', 'exemplar_sparsity', 'exemplar_fft')


def _pkg():
    import kwiiyatta_amd
    return kwiiyatta_amd


class Config:
    def __init__(self, argparser=None):
        self.parser = argparser or argparse.ArgumentParser()
        self._declare(VOCODER_OPTIONS)

    def _declare(self, options):
        for flag, spec in options:
            self.parser.add_argument(flag, **spec)

    def add_converter_arguments(self):
        self._declare(CONVERTER_OPTIONS)

    def add_transpose_key_argument(self):
        self._declare((TRANSPOSE_KEY_OPTION,))

    def add_formant_shift_argument(self):
        self._declare((FORMANT_SHIFT_OPTION,))

    @property
    def formant_ratio(self):
        """the warp ratio --formant-shift asks for (1 when the option is not declared)"""
        return 2.0 ** (getattr(self, 'formant_shift', 0.0) / 12)

    def add_gv_argument(self):
        self._declare((GV_OPTION,))

    def add_ms_argument(self):
        self._declare((MS_OPTION,))

    def add_mlpg_em_argument(self):
        self._declare((MLPG_EM_OPTION,))

    def add_mlpg_gv_argument(self):
        self._declare((MLPG_GV_OPTION,))

    def add_diff_filter_argument(self):
        self._declare((DIFF_FILTER_OPTION,))

    def add_power_arguments(self):
        self._declare(POWER_OPTIONS)

    def add_aperiodicity_arguments(self):
        self._declare(APERIODICITY_OPTIONS)

    def add_argument(self, *args, **kwargs):
        self.parser.add_argument(*args, **kwargs)

    def parse_args(self, args=None):
        """`args` come BEFORE the process arguments, which therefore win (the reference's order)"""
        self.parser.parse_args(args=list(args or []) + sys.argv[1:], namespace=self)
        if getattr(self, 'mlpg_gv', None) is not None:
            if getattr(self, 'gv', 0.0) > 0:
                self.parser.error('--mlpg-gv does not go with --gv: the postfilter would repair the same variance twice')
            if getattr(self, 'ms', 0.0) > 0:
                self.parser.error('--mlpg-gv does not go with --ms: composing it with the modulation-spectrum filter is '
                                  'left for later')
        if getattr(self, 'converter', 'gmm') == 'exemplar':
            for name, asked, flag, why in EXEMPLAR_CONFLICTS:
                if asked(getattr(self, name, None)):
                    self.parser.error(f'{flag} does not go with --converter exemplar: {why}')
        else:
            for name in EXEMPLAR_OPTIONS:
                if getattr(self, name, None) is not None:
                    self.parser.error(f'--{name.replace("_", "-")} needs --converter exemplar')
        if getattr(self, 'nonparallel', None) is not None:
            if getattr(self, 'align_iterations', None) is not None:
                self.parser.error('--nonparallel does not go with --align-iterations: there are no pairs to align '
                                  'again')
            if getattr(self, 'convert_aperiodicity', False):
                self.parser.error('--nonparallel does not go with --convert-aperiodicity: band rows along the '
                                  'nearest-neighbour pairs are left for later')

    # ---- factories --------------------------------------------------------------------------------------
    def create_analyzer(self, *args, Analyzer=None, **kwargs):
        make = Analyzer or _pkg().Analyzer
        if getattr(self, 'f0_estimator', 'dio') != 'dio':       # (the analyzers of the default take what they always took)
            kwargs = dict(kwargs, f0_estimator=self.f0_estimator)
        return make(*args, **dict(kwargs, frame_period=self.frame_period, mcep_order=self.mcep_order))

    def create_converter(self, Converter=None, **kwargs):
        make = Converter or _pkg().MelCepstrumConverter
        if getattr(self, 'converter', 'gmm') == 'exemplar':
            chosen = dict(converter='exemplar', **{name: getattr(self, name, None) for name in EXEMPLAR_OPTIONS})
            if self.mcep_fs is not None:
                chosen['mcep_fs'] = self.mcep_fs
            return make(**dict(chosen, **kwargs))
        chosen = dict(random_state=self.converter_seed, components=int(self.converter_components))
        if self.mcep_fs is not None:
            chosen['mcep_fs'] = self.mcep_fs
        if getattr(self, 'converter_covariance', None) is not None:
            chosen['covariance'] = self.converter_covariance
        return make(**dict(chosen, **kwargs))

    def _required_dir(self, flag):
        # the reference tests `source` for both flags (config.py:79); kept, since it decides when --target alone errors
        if self.source is None:
            self.parser.error(f'the following arguments are required: --{flag}')
        return pathlib.Path(getattr(self, flag))

    source_path = property(lambda self: self._required_dir('source'))
    target_path = property(lambda self: self._required_dir('target'))

    # ---- the source side's pitch shift (--source-f0-rate) ----------------------------------------------------------------
    def analyze_source(self, path, rate):
        """the analyzer of a SOURCE-side wav file -- a training file, a file to convert, the source of an evaluated
        pair -- for a converter of that `source_f0_rate`: at 1 the file as it is, otherwise its waveform through the
        pitch shifter first"""
        k = _pkg()
        if rate == 1:
            return self.create_analyzer(path, Analyzer=k.analyze_wav)
        return self.create_analyzer(k.shift_pitch(k.load_wav(path), rate), Analyzer=k.vocoder.Analyzer)

    def _training_keys(self, keys):
        return sorted(keys)[slice(self.skip_files, None)][:self.max_files]

    def auto_source_f0_rate(self):
        """exp(mean voiced log-f0 of the target - that of the source) over the training files, from the f0 tracks of
        the unshifted waveforms (DIO + StoneMask only); a parser error outside the shifter's range"""
        from .backend import f0 as f0map
        k = _pkg()
        dirs = (self.source_path, self.target_path)
        sides = [k.WavFileDataset(path, Analyzer=functools.partial(self.create_analyzer, Analyzer=k.analyze_wav))
                 for path in dirs]
        keys = self._training_keys(sides[0].keys() & sides[1].keys())
        means = []
        for flag, side in zip(('source', 'target'), sides):
            if getattr(self, 'nonparallel', None) is not None:       # each side's own training files
                keys = self._training_keys(side.keys())
            tracks = [np.ascontiguousarray(side[key].f0, dtype=np.float64) for key in keys]
            n, mean, _ = f0map.merge_moments(f0map.logf0_moments(tracks)) if tracks else (0, 0, 0)
            if not n > 0:
                self.parser.error(f'--source-f0-rate auto: the training files of --{flag} have no voiced frames')
            means.append(float(mean))
        rate = math.exp(means[1] - means[0])
        lo, hi = SOURCE_F0_RATE_RANGE
        if not lo <= rate <= hi:
            self.parser.error(f'--source-f0-rate auto: the speakers\' f0 ratio {rate:.4f} is outside [{lo}, {hi}]')
        return rate

    def resolve_source_f0_rate(self):
        """the rate the command line asks for, as a number (`auto` is measured once and remembered)"""
        asked = getattr(self, 'source_f0_rate', None)
        if asked is None:
            return 1.0
        if asked == 'auto':
            if getattr(self, '_auto_f0_rate', None) is None:
                self._auto_f0_rate = self.auto_source_f0_rate()
            return self._auto_f0_rate
        return float(asked)

    def load_dataset(self, source_f0_rate=None):
        """the aligned parallel training set of --source / --target; the source side through `analyze_source` at
        `source_f0_rate` (default: what the command line asks for, resolved when the first file is analysed -- a
        converter loaded from a model file in between decides, see train_converter)"""
        k = _pkg()

        def source(path):
            rate = source_f0_rate if source_f0_rate is not None else getattr(self, '_model_f0_rate', None)
            return self.analyze_source(path, self.resolve_source_f0_rate() if rate is None else rate)
        analyze = functools.partial(self.create_analyzer, Analyzer=k.analyze_wav)
        sides = [k.WavFileDataset(self.source_path, Analyzer=source), k.WavFileDataset(self.target_path, Analyzer=analyze)]
        return k.align(*sides)

    def nonparallel_sides(self, source_f0_rate=None):
        """(source, target): the two directories as data sets of their own for --nonparallel, which pairs no files;
        the source side through `analyze_source` as in `load_dataset`"""
        k = _pkg()
        rate = self.resolve_source_f0_rate() if source_f0_rate is None else source_f0_rate
        analyze = functools.partial(self.create_analyzer, Analyzer=k.analyze_wav)
        return (k.WavFileDataset(self.source_path, Analyzer=lambda path: self.analyze_source(path, rate)),
                k.WavFileDataset(self.target_path, Analyzer=analyze))

    def train_converter(self, f0_stats=False, gv_stats=False, ms_stats=False, gv_var=False, ap_model=False, **kwargs):
        """f0_stats=True / gv_stats=True / ms_stats=True: training also computes the f0 statistics / the target's global
        variance / the modulation-spectrum statistics at --ms-length (and the model file keeps them); a loaded model
        without them is a parser error.  gv_var=True (--mlpg-gv): gv_stats, and a loaded model must also hold the
        variance of the global variance.  ap_model=True (--convert-aperiodicity): training also fits the band-aperiodicity
        mixture of --ap-components components; a loaded model without it is a parser error, and so is a --mcep-fs below
        12 kHz (no band), before a file is read"""
        gv_stats = gv_stats or gv_var
        if ap_model and self.mcep_fs is not None:
            from .backend import bap
            if bap.bands(self.mcep_fs) < 1:
                self.parser.error(f'--convert-aperiodicity needs a sampling rate of 12 kHz or more: --mcep-fs '
                                  f'{self.mcep_fs} has no aperiodicity band')
        converter = self.create_converter(**kwargs)
        model = getattr(self, 'converter_model', None)
        if model is not None and pathlib.Path(model).is_file():
            with np.load(model, allow_pickle=False) as z:
                kind = str(z['converter']) if 'converter' in z.files else 'gmm'
            mine = getattr(converter, 'kind', 'gmm')
            if kind != mine:
                self.parser.error(f'{model}: the converter model was trained with --converter {kind}, not {mine}; '
                                  f'retrain it with --converter {mine} (a new --converter-model file)')
            converter.load(model)
            asked = getattr(self, 'source_f0_rate', None)
            if isinstance(asked, float) and asked != converter.source_f0_rate:
                self.parser.error(f'{model}: the converter model was trained with --source-f0-rate '
                                  f'{converter.source_f0_rate:g}, not {asked:g}; retrain it with --source-f0-rate '
                                  f'{asked:g} (a new --converter-model file)')
            self._model_f0_rate = converter.source_f0_rate          # (a loaded model decides, `auto` included)
            asked = getattr(self, 'align_iterations', None)
            if asked is not None and asked != converter.align_iterations:
                self.parser.error(f'{model}: the converter model was trained with --align-iterations '
                                  f'{converter.align_iterations}, not {asked}; retrain it with --align-iterations '
                                  f'{asked} (a new --converter-model file)')
            asked = getattr(self, 'nonparallel', None)
            if asked is not None and asked != converter.nonparallel:
                was = ('on parallel data' if converter.nonparallel is None
                       else f'with --nonparallel {converter.nonparallel}')
                self.parser.error(f'{model}: the converter model was trained {was}, not with --nonparallel {asked}; '
                                  f'retrain it with --nonparallel {asked} (a new --converter-model file)')
            asked = getattr(self, 'f0_estimator', 'dio')
            if asked != converter.f0_estimator:
                self.parser.error(f'{model}: the converter model was trained with --f0-estimator '
                                  f'{converter.f0_estimator}, not {asked}: its voicing term and f0 statistics were learnt '
                                  f'on the other tracks; retrain it with --f0-estimator {asked} (a new --converter-model '
                                  f'file)')
            asked = getattr(self, 'converter_covariance', None)
            if asked is not None and asked != converter.covariance:
                self.parser.error(f'{model}: the converter model was trained with --converter-covariance '
                                  f'{converter.covariance}, not {asked}; retrain it with --converter-covariance '
                                  f'{asked} (a new --converter-model file)')
            if f0_stats and converter.f0_stats is None:
                self.parser.error(f'{model}: the converter model has no f0 statistics; retrain it with '
                                  f'--convert-f0 (a new --converter-model file)')
            if gv_stats and converter.gv_stats is None:
                self.parser.error(f'{model}: the converter model has no global variance statistics; retrain it with '
                                  f'--gv (a new --converter-model file)')
            if gv_var and converter.gv_var is None:
                self.parser.error(f'{model}: the converter model has no variance of the global variance; retrain it '
                                  f'with --mlpg-gv (a new --converter-model file)')
            if ms_stats and converter.ms_stats is None:
                self.parser.error(f'{model}: the converter model has no modulation spectrum statistics; retrain it '
                                  f'with --ms (a new --converter-model file)')
            if ap_model and converter.ap_converter is None:
                self.parser.error(f'{model}: the converter model has no band-aperiodicity mixture; retrain it with '
                                  f'--convert-aperiodicity (a new --converter-model file)')
            return converter
        converter = self._train(converter, f0_stats=f0_stats, gv_stats=gv_stats, ms_stats=ms_stats, ap_model=ap_model)
        if model is not None:
            converter.save(model)
        return converter

    def _train(self, converter, f0_stats=False, gv_stats=False, ms_stats=False, ap_model=False):
        converter.source_f0_rate = self._model_f0_rate = self.resolve_source_f0_rate()
        converter.f0_estimator = getattr(self, 'f0_estimator', 'dio')
        extra = dict(f0_stats=True) if f0_stats else {}
        if gv_stats:
            extra['gv_stats'] = True
        if ms_stats:
            extra.update(ms_stats=True, ms_length=getattr(self, 'ms_length', None) or 4096)
        if getattr(self, 'nonparallel', None) is not None:
            sides = self.nonparallel_sides(converter.source_f0_rate)
            converter.train_nonparallel(*sides, *(self._training_keys(side.keys()) for side in sides),
                                        iterations=self.nonparallel, **extra, **(dict(ap_model=True) if ap_model else {}))
            return converter
        dataset = self.load_dataset(converter.source_f0_rate)
        keys = sorted(dataset.keys())[slice(self.skip_files, None)]
        if getattr(self, 'align_iterations', None):
            extra['align_iterations'] = self.align_iterations
        if ap_model:
            extra.update(ap_model=True, ap_components=getattr(self, 'ap_components', None) or 16)
        converter.train(dataset, keys[:self.max_files], **extra)
        return converter
