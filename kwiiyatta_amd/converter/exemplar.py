"""Exemplar-based innermost stage of the converter stack, beside the joint-density mixture (Takashima et al. 2012; Wu,
Virtanen, Chng, Li 2014).  The reference has no counterpart.

The aligned training frames themselves are the model: two coupled dictionaries, the source and the target side of
the joint matrix [source c1..cN | target c1..cN] the mixture would be fitted on, and nothing is fitted.  A source
frame is explained as a sparse non-negative combination of source exemplars (KL-NMF activations, backend.nmf on
the f64 matrix cores), and the same activations applied to the paired target exemplars give the converted frame.

The dictionaries are kept as mel-cepstra.  The activations work on amplitude envelopes: with c0 = 0 the envelope
exp(sum_m c_m cos(m w~)) on exemplar_fft / 2 + 1 bins (the square root of `sptk.mc2sp` at the converter's all-pass
constant), every row scaled to unit sum.  The converted envelope goes back to order N through `sptk.sp2mc` of its
square, c0 dropped: the scale of a row moves c0 alone.

It takes the place of DeltaFeatureConverter(GMMFeatureConverter) beneath MelCepstrumFeatureConverter, which sets c0
aside, re-attaches it, and runs every stage that works on the converted mel-cepstrum (gv, ms, postfilter,
keep_power) unchanged."""
import numpy as np

from ..backend import nmf, sptk
from . import abc

FFT_SIZES = (256, 512, 1024, 2048, 4096)
# the cheapest setting (exemplars x iterations) within 0.02 dB of the best held-out distortion of
# profiles/exemplar_quality.json (README.md).  The sparsity does not move c1..cN at all: see README.md
DEFAULTS = dict(exemplars=512, iterations=200, sparsity=0.0, fft=512)


def select_rows(rows, exemplars):
    """the training rows a dictionary of at most `exemplars` atoms keeps of `rows`: all of them, or rows
    floor(i rows / exemplars), i = 0 .. exemplars - 1"""
    if rows <= exemplars:
        return np.arange(rows)
    return np.arange(exemplars, dtype=np.int64) * rows // exemplars


class ExemplarFeatureConverter(abc.FeatureConverter):
    kind = 'exemplar'
    gmm = None          # (the outer stage asks a mixture for its EM iterations; there is none)

    def __init__(self, exemplars=None, iterations=None, sparsity=None, fft=None):
        pick = lambda v, name: DEFAULTS[name] if v is None else v  # noqa: E731
        self.exemplars, self.iterations = pick(exemplars, 'exemplars'), pick(iterations, 'iterations')
        self.sparsity, self.fft = pick(sparsity, 'sparsity'), pick(fft, 'fft')
        if isinstance(self.exemplars, bool) or int(self.exemplars) != self.exemplars or \
                not 1 <= self.exemplars <= nmf.MAX_ATOMS:
            raise ValueError(f'exemplars must be an integer within [1, {nmf.MAX_ATOMS}], not {self.exemplars!r}')
        if isinstance(self.iterations, bool) or int(self.iterations) != self.iterations or \
                not 0 <= self.iterations <= nmf.MAX_ITERATIONS:
            raise ValueError(f'exemplar_iterations must be an integer within [0, {nmf.MAX_ITERATIONS}], not '
                             f'{self.iterations!r}')
        if not (self.sparsity >= 0 and np.isfinite(self.sparsity)):
            raise ValueError(f'exemplar_sparsity must be finite and >= 0, not {self.sparsity!r}')
        if self.fft not in FFT_SIZES:
            raise ValueError(f'exemplar_fft must be one of {FFT_SIZES}, not {self.fft!r}')
        self.exemplars, self.iterations = int(self.exemplars), int(self.iterations)
        self.sparsity, self.fft = float(self.sparsity), int(self.fft)
        self.source = self.target = None        # (atoms, N) mel-cepstra c1..cN
        self.rows = 0                           # training rows the atoms were picked from
        self.fs = None
        self._spectra = None

    # ---- training -----------------------------------------------------------------------------------------------------
    def _train(self, dataarray, **fit_options):
        if fit_options:
            raise TypeError(f'the exemplar converter fits nothing: unexpected {sorted(fit_options)}')
        joint = np.asarray(dataarray, dtype=np.float64)
        if joint.ndim != 2 or joint.shape[1] % 2 or not len(joint):
            raise ValueError(f'exemplar dictionary: a joint matrix [source | target] with rows is expected, not shape '
                             f'{joint.shape}')
        keep = select_rows(len(joint), self.exemplars)
        order = joint.shape[1] // 2
        self.source = np.ascontiguousarray(joint[keep, :order])
        self.target = np.ascontiguousarray(joint[keep, order:])
        self.rows = len(joint)
        self._spectra = None

    def bind_rate(self, fs):
        """the sampling rate the mel-cepstra belong to (the outer stage knows it): it gives the all-pass constant"""
        if fs != self.fs:
            self.fs, self._spectra = fs, None

    # ---- the state a model file keeps (MelCepstrumFeatureConverter.save / load) ---------------------------------------
    def model_arrays(self):
        return dict(exemplar_source=self.source, exemplar_target=self.target, exemplar_fft=self.fft,
                    exemplar_iterations=self.iterations, exemplar_sparsity=self.sparsity, exemplar_rows=self.rows)

    def load_arrays(self, z):
        self.source = np.array(z['exemplar_source'], dtype=np.float64, order='C')
        self.target = np.array(z['exemplar_target'], dtype=np.float64, order='C')
        self.fft, self.iterations = int(z['exemplar_fft']), int(z['exemplar_iterations'])
        self.sparsity = float(z['exemplar_sparsity'])
        self.rows = int(z['exemplar_rows']) if 'exemplar_rows' in z.files else len(self.source)
        self.exemplars = max(self.exemplars, len(self.source))
        self._spectra = None

    # ---- conversion ---------------------------------------------------------------------------------------------------
    def prepare(self, coefficients):
        """(rows, N) mel-cepstra c1..cN -> (rows, fft / 2 + 1) amplitude envelopes of unit sum, c0 taken as 0"""
        if self.fs is None:
            raise ValueError('exemplar converter: the sampling rate is not known yet (bind_rate)')
        c = np.asarray(coefficients, dtype=np.float64)
        mc = np.ascontiguousarray(np.hstack((np.zeros((len(c), 1)), c)))
        power = sptk.mc2sp(mc, alpha=sptk.mcepalpha(self.fs), fftlen=self.fft)
        return nmf.unit_sum(np.sqrt(power))

    def dictionaries(self):
        """(S, Tg): the prepared source and target atoms, made on first use and kept"""
        if self.source is None:
            raise ValueError('exemplar converter: not trained')
        if self._spectra is None:
            self._spectra = self.prepare(self.source), self.prepare(self.target)
        return self._spectra

    def convert(self, feature, mlpg=True, diff=False, return_h=False, **mixture_options):
        """(T, N) c1..cN -> (T, N); diff=True: minus the input.  `mlpg` has no meaning here (there are no dynamic
        features); the mixture's options (em, gv_stats, gv_iterations) raise ValueError."""
        asked = sorted(name for name, v in mixture_options.items() if v is not None and name != 'gv_weight')
        if asked:
            raise ValueError(f'the exemplar converter has no mixture: {", ".join(asked)} cannot be used with it')
        feature = np.ascontiguousarray(feature, dtype=np.float64)
        S, Tg = self.dictionaries()
        order = self.source.shape[1]
        if feature.ndim != 2 or feature.shape[1] != order:
            raise ValueError(f'exemplar converter: (frames, {order}) coefficients are expected, not shape {feature.shape}')
        if not len(feature):
            return (feature.copy(), np.empty((0, len(S)))) if return_h else feature.copy()
        out = nmf.convert(S, Tg, self.prepare(feature), self.iterations, self.sparsity, return_h=return_h)
        Y, H = out if return_h else (out, None)
        converted = np.ascontiguousarray(sptk.sp2mc(Y * Y, order=order, alpha=sptk.mcepalpha(self.fs))[:, 1:])
        if diff:
            converted = converted - feature
        return (converted, H) if return_h else converted
