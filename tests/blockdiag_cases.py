"""Block-diagonal covariance fit (`covariance_structure='block_diag'`): what its CPU and GPU tests share.

The reference is the masked full-covariance EM: `NumpyStats` (numpy_em_stats.py) whose `finalize` multiplies the
covariances by the pattern mask, driven by `gmm_fit._em_fit`.  Its E-step is a Cholesky of the expanded D x D matrix,
independent of the 2 x 2 formula of the HIP kernels (csrc/kwy_gmmfit_bd.hip)."""
import numpy as np

from numpy_em_stats import NumpyStats

# (n, D, M, seed) of test_gmm_fit.make_data
MONOTONE_CASES = [(3000, 12, 4, 0), (2500, 20, 8, 2), (300, 2, 2, 3), (257, 6, 3, 4), (2000, 30, 64, 2),
                  (1000, 144, 16, 5)]
BLOCK_SHAPES = [(1, 4, 1), (300, 2, 2), (257, 6, 3), (3000, 12, 4), (2000, 30, 64), (5000, 144, 8), (1500, 160, 3),
                (1000, 144, 256)]
FIT_CASES = [(3000, 12, 4, 0), (2500, 20, 8, 2), (300, 2, 2, 3), (257, 6, 3, 4), (2000, 30, 64, 2), (4000, 144, 8, 1)]
FIT_ITERATIONS = [2, 6, 2, 2, 6, 6]          # where the reference stops, at least 4e-5 away from `tol`


def pattern_mask(D):
    """1.0 on the diagonals of the xx, yy, xy and yx blocks"""
    h = D // 2
    eye = np.eye(h)
    return np.block([[eye, eye], [eye, eye]])


def obeys_pattern(covs):
    """exactly zero off the pattern and exactly symmetric"""
    D = covs.shape[-1]
    off = covs[:, pattern_mask(D) == 0]
    return bool((off == 0).all()) and np.array_equal(covs, covs.transpose(0, 2, 1))


class MaskedNumpyStats(NumpyStats):
    """the masked full-covariance EM; `trace` collects the lower bound of every E-step"""

    def __init__(self, X, n_components):
        super().__init__(X, n_components)
        self.mask = pattern_mask(self.D)
        self.trace = []

    def estep(self):
        ll = super().estep()
        self.trace.append(float(ll.item()) / self.n)
        return ll

    def finalize(self, stats, sxx, reg_covar):
        super().finalize(stats, sxx, reg_covar)
        self.covs = self.covs * self.mask


def make_data(n, D, M, seed):
    from test_gmm_fit import make_data as make
    return make(n, D, M, seed)


def random_labels(n, M, seed):
    labels = np.random.default_rng(seed + 100).integers(0, M, n)
    labels[:M] = np.arange(M)
    return labels


def reference_fit(X, M, labels, max_iter=100, tol=1e-3, reg_covar=1e-6, stats_class=MaskedNumpyStats):
    """-> (stats, lower bound, converged, n_iter): gmm_fit._em_fit over the numpy statistics from `labels`"""
    from kwiiyatta_amd.converter import gmm_fit
    stats = stats_class(X, M)
    stats.set_resp_from_labels(labels)
    lower_bound, converged, n_iter = gmm_fit._em_fit(stats, float(len(X)), max_iter, tol, reg_covar, False)
    return stats, lower_bound, converged, n_iter


_kmeans_cache = {}


def kmeans_case(n, D, M, seed):
    """(X, sklearn's k-means labels, the reference fit from them), computed once per case"""
    key = (n, D, M, seed)
    if key not in _kmeans_cache:
        from test_gmm_fit import kmeans_labels
        X = make_data(n, D, M, seed)
        labels = kmeans_labels(X, M, seed)[0]
        _kmeans_cache[key] = (X, labels, reference_fit(X, M, labels))
    return _kmeans_cache[key]


def frame_wise_closed_form(weights, means, covs, x):
    """sum_m P(m|x) (muy_m + (c_m / a_m)(x - mux_m)) with P(m|x) from the diagonal source marginals: the conditional
    mean of a block-diagonal mixture, frame by frame"""
    h = means.shape[1] // 2
    i = np.arange(h)
    a, c = covs[:, i, i], covs[:, i, h + i]
    mux, muy = means[:, :h], means[:, h:]
    d = x[:, None, :] - mux[None]                                        # (T, M, h)
    logp = np.log(weights)[None] - 0.5 * (np.log(2 * np.pi * a)[None] + d * d / a[None]).sum(2)
    logp -= logp.max(1, keepdims=True)
    post = np.exp(logp)
    post /= post.sum(1, keepdims=True)
    return (post[:, :, None] * (muy[None] + (c / a)[None] * d)).sum(1)
