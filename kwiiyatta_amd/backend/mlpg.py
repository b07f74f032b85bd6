"""nnmnkwii-shaped front-end of the HIP converter-apply kernels
(reference call sites /root/reference/kwiiyatta/converter/delta.py:30,46 and
gmm.py:28-34): ``MLPG(gmm, windows, diff).transform(X)`` with the reference's
fixed DELTA_WINDOWS."""
import numpy as np

from .. import _lib
from .._lib import lib, ptr

EM_MAX = 16      # KWY_MLPG_EM_MAX (include/kwy.h)
GV_MAX = 256     # KWY_MLPG_GV_MAX

DELTA_WINDOWS = [
    (0, 0, np.array([1.0])),
    (1, 1, np.array([-0.5, 0.0, 0.5])),
    (1, 1, np.array([1.0, -2.0, 1.0])),
]


def _is_delta_windows(windows):
    return (len(windows) == 3 and
            all(w[0] == r[0] and w[1] == r[1] and np.array_equal(np.asarray(w[2]), r[2])
                for w, r in zip(windows, DELTA_WINDOWS)))


def _is_static_window(windows):
    w = DELTA_WINDOWS[0]
    return len(windows) == 1 and windows[0][0] == w[0] and windows[0][1] == w[1] and \
        np.array_equal(np.asarray(windows[0][2]), w[2])


def delta_features(x, windows):
    """static -> static|delta|delta2 (np.correlate(..., 'same') per column).
    Host-side helper for dataset preparation (the fit path); the conversion
    kernel computes the same features on the device."""
    x = np.asarray(x)
    T, D = x.shape
    y = np.zeros((T, D * len(windows)), dtype=x.dtype)
    for i, (_, _, w) in enumerate(windows):
        for c in range(D):
            y[:, D * i + c] = np.correlate(x[:, c], w, mode='same')
    return y


class MLPG:
    """Maximum-likelihood parameter generation from a joint GMM
    (sklearn.mixture.GaussianMixture-like object with weights_, means_,
    covariances_ and covariance_type == 'full').

    em=None: one arg-max mixture per frame and a single trajectory solve, what nnmnkwii does.  em=N, an integer within
    [0, EM_MAX] (an addition): every mixture weighs in with its posterior, and the posteriors are re-estimated N times
    from the source frame and the trajectory solved last (kwy_gmm_mlpg_em, include/kwy.h); `loglik_` then holds
    L_0 .. L_N of the last `transform`, which never decrease.

    gv=(mean, var) (an addition; static_dim values each: mean and variance over the training utterances of the target's
    per-utterance variance of every coefficient) with gv_iterations=N, an integer within [0, GV_MAX]: parameter
    generation considering the global variance (kwy_gmm_mlpg_gv) -- after the posteriors are fixed (arg-max, or em=),
    N conjugate-gradient steps on the joint objective from the linearly scaled track; gv_weight > 0 weighs the GV term.
    With diff=True the variance is taken of trajectory + source statics.  `objective_` then holds Q_0 .. Q_N of the
    last `transform`, which never decrease."""

    def __init__(self, gmm, windows=None, swap=False, diff=False, ctx=None, em=None, gv=None, gv_iterations=None,
                 gv_weight=1.0):
        if windows is None:
            windows = DELTA_WINDOWS
        self.framewise = _is_static_window(windows)     # DELTA_WINDOWS[0:1]: conversion without trajectory smoothing
        if not self.framewise and not _is_delta_windows(windows):
            raise NotImplementedError('only the reference DELTA_WINDOWS (or their static part alone) are implemented '
                                      'on the GPU')
        if swap:
            raise NotImplementedError('swap=True is not used by the reference and not implemented')
        if em is not None:
            if isinstance(em, bool) or not isinstance(em, (int, np.integer)):
                raise ValueError(f'em must be None or an integer within [0, {EM_MAX}], not {em!r}')
            if not 0 <= em <= EM_MAX:
                raise ValueError(f'em = {em} is outside [0, {EM_MAX}]')
            if self.framewise:
                raise ValueError('em needs the trajectory solve: it does not go with the static window alone '
                                 '(mlpg=False)')
            em = int(em)
        self.em = em
        self.loglik_ = None
        self.objective_ = None
        if (gv is None) != (gv_iterations is None):
            raise ValueError('gv=(mean, var) and gv_iterations go together')
        if gv is not None:
            from . import gv as gvgen
            if self.framewise:
                raise ValueError('gv needs the trajectory solve: it does not go with the static window alone '
                                 '(mlpg=False)')
            if len(gv) != 2:
                raise ValueError('gv must be the pair (mean, var)')
            gv = gvgen.ascent_arguments(gv[0], gv[1], gv_iterations, gv_weight)
        self.gv = gv
        assert gmm.covariance_type == 'full'
        self.weights = np.ascontiguousarray(gmm.weights_, dtype=np.float64)
        self.means = np.ascontiguousarray(gmm.means_, dtype=np.float64)
        self.covs = np.ascontiguousarray(gmm.covariances_, dtype=np.float64)
        self.diff = bool(diff)
        self.windows = windows
        self.num_mixtures = len(self.weights)
        self.static_dim = self.means.shape[1] // 2 // len(windows)
        self.ctx = ctx

    def transform(self, src):
        """src: (T, 3*d) static+delta features (as produced by delta_features) or
        (T, d) static features.  Returns (T, 3*d) with the generated static
        trajectory in the first d columns (nnmnkwii returns (T, d); the
        reference truncates to d either way: converter/delta.py:48-49)."""
        src = np.ascontiguousarray(src, dtype=np.float64)
        d = self.static_dim
        if self.framewise:
            # nnmnkwii: feature_dim == static_dim -> MLPGBase.transform, the posterior-weighted conditional mean of
            # every frame on its own (all of the mixture's dimensions, dynamic features included, are "static" here)
            if src.shape[1] != d:
                raise ValueError(f'feature dimension {src.shape[1]} does not match the GMM ({d})')
            ctx = self.ctx or _lib.default_context()
            y = np.empty_like(src)
            if len(src):
                _lib.check(ctx, lib.kwy_gmm_convert_frames(ctx.handle, ptr(src), src.shape[0], d, self.num_mixtures,
                                                           ptr(self.weights), ptr(self.means), ptr(self.covs),
                                                           int(self.diff), ptr(y)))
            return y
        if src.shape[1] not in (d, 3 * d):
            raise ValueError(f'feature dimension {src.shape[1]} does not match the GMM ({d})')
        x = np.ascontiguousarray(src[:, :d])
        if self.gv is not None and self.gv[0].shape != (d,):
            raise ValueError(f'gv statistics hold {self.gv[0].shape[0]} values, the GMM has {d} static dimensions')
        ctx = self.ctx or _lib.default_context()
        y = np.empty((x.shape[0], d))
        if self.gv is not None:
            mean, var, iterations, weight = self.gv
            em = -1 if self.em is None else self.em
            loglik, objective = np.empty(max(em, 0) + 1), np.empty(iterations + 1)
            status = np.zeros(1, dtype=np.int32)
            _lib.check(ctx, lib.kwy_gmm_mlpg_gv(ctx.handle, ptr(x), x.shape[0], d, self.num_mixtures, ptr(self.weights),
                                                ptr(self.means), ptr(self.covs), int(self.diff), em, int(self.diff),
                                                ptr(mean), ptr(var), weight, iterations, ptr(y),
                                                ptr(loglik) if em >= 0 else None, ptr(objective), ptr(status)))
            if status[0]:
                raise ValueError(f'GV ascent: {int(status[0])} coefficient(s) were left at the maximum-likelihood track: '
                                 f'their variance is not finite, or a statistic is not finite or not positive there')
            self.loglik_ = loglik.tolist() if em >= 0 else None
            self.objective_ = objective.tolist()
            return y
        if self.em is not None:
            loglik = np.empty(self.em + 1)
            _lib.check(ctx, lib.kwy_gmm_mlpg_em(ctx.handle, ptr(x), x.shape[0], d, self.num_mixtures, ptr(self.weights),
                                                ptr(self.means), ptr(self.covs), int(self.diff), self.em, ptr(y),
                                                ptr(loglik)))
            self.loglik_ = loglik.tolist()
            return y
        _lib.check(ctx, lib.kwy_gmm_mlpg(ctx.handle, ptr(x), x.shape[0], d, self.num_mixtures,
                                         ptr(self.weights), ptr(self.means), ptr(self.covs),
                                         int(self.diff), ptr(y)))
        return y
