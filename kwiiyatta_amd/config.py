"""Options shared by the command-line tools, and the factories that apply them.  API of kwiiyatta.config.Config
(/root/reference/kwiiyatta/config.py): the options are parsed INTO the Config object (it is the argparse namespace),
analyzers and converters are created through it so that frame period, mel-cepstrum order, component count and seed
follow the command line."""
import argparse
import functools
import pathlib
import sys

VOCODER_OPTIONS = (
    ('--frame-period', dict(type=int, default=5, help='Frame period milli-seconds of vocoder')),
    ('--mcep-order', dict(type=int, default=24, help='Mel-cepstrum order for spectrum envelope')),
)
CONVERTER_OPTIONS = (
    ('--source', dict(type=str, help='Source data-set path of voice conversion')),
    ('--target', dict(type=str, help='Target data-set path of voice conversion')),
    ('--max-files', dict(type=int, help='File num to train feature converter')),
    ('--skip-files', dict(type=int, help='Skip file num to train feature converter')),
    ('--mcep-fs', dict(type=int, help='Sampling rate of training mel cepstrum')),
    ('--converter-components', dict(type=int, default=64, help='Components num for feature converter')),
    ('--converter-seed', dict(type=int, help='Random seed for feature converter')),
    # an addition to the reference's options: keep the trained converter between runs
    ('--converter-model', dict(type=str, help='File of the trained converter: loaded when it exists (no training, '
                                              '--source/--target not needed), written after training otherwise')),
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

    def add_gv_argument(self):
        self._declare((GV_OPTION,))

    def add_argument(self, *args, **kwargs):
        self.parser.add_argument(*args, **kwargs)

    def parse_args(self, args=None):
        """`args` come BEFORE the process arguments, which therefore win (the reference's order)"""
        self.parser.parse_args(args=list(args or []) + sys.argv[1:], namespace=self)

    # ---- factories --------------------------------------------------------------------------------------
    def create_analyzer(self, *args, Analyzer=None, **kwargs):
        make = Analyzer or _pkg().Analyzer
        return make(*args, **dict(kwargs, frame_period=self.frame_period, mcep_order=self.mcep_order))

    def create_converter(self, Converter=None, **kwargs):
        make = Converter or _pkg().MelCepstrumConverter
        chosen = dict(random_state=self.converter_seed, components=self.converter_components)
        if self.mcep_fs is not None:
            chosen['mcep_fs'] = self.mcep_fs
        return make(**dict(chosen, **kwargs))

    def _required_dir(self, flag):
        # the reference tests `source` for both flags (config.py:79); kept, since it decides when --target alone errors
        if self.source is None:
            self.parser.error(f'the following arguments are required: --{flag}')
        return pathlib.Path(getattr(self, flag))

    source_path = property(lambda self: self._required_dir('source'))
    target_path = property(lambda self: self._required_dir('target'))

    def load_dataset(self):
        """the aligned parallel training set of --source / --target"""
        k = _pkg()
        analyze = functools.partial(self.create_analyzer, Analyzer=k.analyze_wav)
        sides = [k.WavFileDataset(path, Analyzer=analyze) for path in (self.source_path, self.target_path)]
        return k.align(*sides)

    def train_converter(self, f0_stats=False, gv_stats=False, **kwargs):
        """f0_stats=True / gv_stats=True: training also computes the f0 statistics / the target's global variance (and
        the model file keeps them); a loaded model without them is a parser error"""
        converter = self.create_converter(**kwargs)
        model = getattr(self, 'converter_model', None)
        if model is not None and pathlib.Path(model).is_file():
            converter.load(model)
            if f0_stats and converter.f0_stats is None:
                self.parser.error(f'{model}: the converter model has no f0 statistics; retrain it with '
                                  f'--convert-f0 (a new --converter-model file)')
            if gv_stats and converter.gv_stats is None:
                self.parser.error(f'{model}: the converter model has no global variance statistics; retrain it with '
                                  f'--gv (a new --converter-model file)')
            return converter
        converter = self._train(converter, f0_stats=f0_stats, gv_stats=gv_stats)
        if model is not None:
            converter.save(model)
        return converter

    def _train(self, converter, f0_stats=False, gv_stats=False):
        dataset = self.load_dataset()
        keys = sorted(dataset.keys())[slice(self.skip_files, None)]
        extra = dict(f0_stats=True) if f0_stats else {}
        if gv_stats:
            extra['gv_stats'] = True
        converter.train(dataset, keys[:self.max_files], **extra)
        return converter
