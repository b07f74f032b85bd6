"""A numpy INCA (Erro, Moreno, Bonafonte 2010) on given feature matrices and a given conversion, the synthetic set
its tests share, and stand-ins for feature sets whose mel-cepstra are given.  Reference of
MelCepstrumFeatureConverter.train_nonparallel: every source row is paired with its nearest target row and every
target row with its nearest source row, the map is fitted on the pairs, the source converted, the search repeated."""
import math

import numpy as np

import nn_cases

ORDER = 8
DB = 10.0 / math.log(10.0)


def ar_track(rs, frames, dims, coefficient=0.95, noise=0.3):
    """an AR(1) track per column, started from its stationary distribution"""
    x = np.empty((frames, dims))
    x[0] = rs.standard_normal(dims) * noise / math.sqrt(1.0 - coefficient ** 2)
    for t in range(1, frames):
        x[t] = coefficient * x[t - 1] + noise * rs.standard_normal(dims)
    return x


def synthetic(seed, dims=ORDER):
    """(source tracks, target tracks): three AR(1) tracks of 300 x dims, and three OTHER such tracks of 280 x dims
    times 1.25 plus a ramp from 0.5 to -0.5 over the columns -- two speakers that never say the same thing"""
    rs = np.random.RandomState(seed)
    source = [ar_track(rs, 300, dims) for _ in range(3)]
    ramp = np.linspace(0.5, -0.5, dims)
    target = [1.25 * ar_track(rs, 280, dims) + ramp for _ in range(3)]
    return source, target


def mcd_db(a, b):
    """mean over the rows of (10 / ln 10) sqrt(2 sum_d (a - b)^2), dB"""
    return float(np.mean(DB * np.sqrt(2.0 * ((a - b) ** 2).sum(axis=1))))


def gaussian_map(joint):
    """one Gaussian on the joint rows [x | y] with its conditional mean: x -> mu_y + S_yx S_xx^-1 (x - mu_x)"""
    d = joint.shape[1] // 2
    mean = joint.mean(axis=0)
    cov = np.cov(joint.T, bias=True)
    gain = np.linalg.solve(cov[:d, :d], cov[:d, d:]).T
    return lambda x: mean[d:] + (x - mean[:d]) @ gain.T


def nearest(Q, C):
    return nn_cases.nearest(Q, C)[0]


def joint_rows(xs, ys, p, q):
    """[x_k | y_p(k)] for k in source order, then [x_q(j) | y_j] for j in target order"""
    return np.vstack((np.hstack((xs, ys[p])), np.hstack((xs[q], ys))))


def inca(source, target, iterations, fit=gaussian_map, search=nearest):
    """source (ns, d), target (nt, d) feature rows -> (history, joint matrices, last map).  Fit i searches with the
    source mapped by fit i - 1 (fit 0: as it is); the joint rows always carry the ORIGINAL source rows; the monitor is
    the mean distortion across all joint rows between the rows the search used."""
    history, matrices, convert = [], [], None
    for it in range(iterations + 1):
        mapped = source if convert is None else convert(source)
        p, q = search(mapped, target), search(target, mapped)
        joint = joint_rows(source, target, p, q)
        monitor = mcd_db(np.vstack((mapped, mapped[q])), np.vstack((target[p], target)))
        convert = fit(joint)
        history.append(dict(rows=len(joint), mcd=monitor))
        matrices.append(joint)
    return history, matrices, convert


class Utterance:
    """what train_nonparallel reads of a feature set, for mel-cepstra that are given: c0 is constant, so every frame
    carries the power term (a speech frame) unless `quiet` names frames to sink 10 below the others"""

    def __init__(self, coefficients, fs=16000, frame_period=5, voiced=None, quiet=()):
        import kwiiyatta_amd as kw
        frames = len(coefficients)
        c0 = np.full((frames, 1), 2.0)
        c0[list(quiet)] = -8.0
        self.fs, self.frame_period = fs, frame_period
        self.mel_cepstrum = kw.MelCepstrum(fs, frame_period, np.ascontiguousarray(np.hstack((c0, coefficients))))
        self.mel_cepstrum_order = coefficients.shape[1]
        self.is_voiced = np.ones(frames, dtype=bool) if voiced is None else np.asarray(voiced, dtype=bool)
        self.f0 = np.where(self.is_voiced, 120.0 * (1.0 + 0.1 * np.sin(np.arange(frames) / 7.0)), 0.0)

    def resample_mel_cepstrum(self, fs):
        assert fs == self.fs
        return self.mel_cepstrum


def datasets(source, target, **kwargs):
    """({key: Utterance}, {key: Utterance}) with keys that the two sides do not share"""
    return ({f's{i}': Utterance(m, **kwargs) for i, m in enumerate(source)},
            {f't{i}': Utterance(m, **kwargs) for i, m in enumerate(target)})


def recording_converter(kw, **kwargs):
    from kwiiyatta_amd.converter import GMMFeatureConverter

    class Recording(GMMFeatureConverter):
        def _train(self, dataarray, **options):
            self.matrices = getattr(self, 'matrices', []) + [np.array(dataarray)]
            super()._train(dataarray, **options)
    return kw.MelCepstrumConverter(use_delta=True, Converter=Recording, **kwargs)


def recorded_matrices(conv):
    """the matrices the innermost stage of a `recording_converter` stack was fitted on, in order"""
    stage = conv
    while not hasattr(stage, 'matrices'):
        stage = stage.base
    return stage.matrices


def small_set(quiet=False):
    source, target = synthetic(3)
    source, target = [m[:60] for m in source], [m[:50] for m in target]
    src, tgt = datasets(source, target)
    if quiet:                                              # frames that are not speech, and an unvoiced stretch
        src['s1'] = Utterance(source[1], quiet=(0, 1, 30), voiced=np.arange(60) % 7 > 1)
        tgt['t2'] = Utterance(target[2], quiet=(49,), voiced=np.arange(50) % 5 > 0)
    return src, tgt


def expected_fit0(src, tgt, source_keys, target_keys):
    """the joint matrix of fit 0 from the definition: delta features over whole utterances, speech rows selected
    afterwards, search rows [voicing | c | delta c], nearest rows both ways"""
    from kwiiyatta_amd.backend.mlpg import DELTA_WINDOWS, delta_features
    from kwiiyatta_amd.vocoder.align import make_feature
    sides = []
    for dataset, keys in ((src, source_keys), (tgt, target_keys)):
        rows, deltas = [], []
        for key in keys:
            u = dataset[key]
            terms = make_feature(u, u.fs)
            speech = terms[:, 0] > 0
            d = delta_features(np.ascontiguousarray(u.mel_cepstrum.data[:, 1:]), DELTA_WINDOWS)
            deltas.append(d[speech])
            rows.append(np.hstack((terms[speech, 1:2], d[speech, :2 * ORDER])))
        sides.append((np.concatenate(rows), np.concatenate(deltas)))
    (S, xd), (T, yd) = sides
    p, q = nn_cases.nearest(S, T)[0], nn_cases.nearest(T, S)[0]
    return joint_rows(xd, yd, p, q), S, T, p, q
