"""Innermost stage of the converter stack: a joint-density Gaussian mixture over [source | target] dynamic features.
API of kwiiyatta.converter.gmm (/root/reference/kwiiyatta/converter/gmm.py): the mixture object sits in `.gmm`,
`_train` fits it, `convert` runs maximum-likelihood parameter generation.  Both run on the GPU: the fit is
GaussianMixtureHIP (k-means + EM kernels, scikit-learn's GaussianMixture.fit semantics), the conversion the MLPG
kernels behind kwiiyatta_amd.backend.mlpg (nnmnkwii's MLPG call signature)."""
from ..backend.mlpg import MLPG
from . import abc, delta
from .gmm_fit import GaussianMixtureHIP as GaussianMixture


class GMMFeatureConverter(abc.FeatureConverter):
    def __init__(self, components=64, max_iter=100, random_state=None, covariance='full', **kwargs):
        # covariance (an addition): 'full', or 'block_diag' -- diagonal source, target and cross blocks, the
        # structure of Toda et al.'s mixtures, for training sets too small for 64 full matrices (gmm_fit)
        self.init_gmm(components, max_iter, random_state, covariance=covariance, **kwargs)

    def init_gmm(self, components, max_iter=100, random_state=None, covariance='full', **kwargs):
        options = dict(verbose=1, covariance_type='full')
        if covariance not in (None, 'full'):       # (handed on only when asked for: a mixture class without the
            options['covariance_structure'] = covariance       # argument, scikit-learn's, keeps working)
        options.update(kwargs)
        self.gmm = GaussianMixture(n_components=components, max_iter=max_iter, random_state=random_state, **options)

    @property
    def covariance(self):
        """the structure of the mixture's covariances: 'full' or 'block_diag'"""
        return getattr(self.gmm, 'covariance_structure', 'full')

    def _train(self, dataarray, **kwargs):
        self.gmm.fit(dataarray, **kwargs)

    def convert(self, feature, mlpg=True, diff=False, em=None, gv_stats=None, gv_iterations=None, gv_weight=1.0):
        # mlpg=False: the static window alone -- every frame converted on its own (posterior-weighted conditional mean)
        # em=N: EM trajectory conversion over soft mixture posteriors, N re-estimations (backend.mlpg.MLPG); the keyword
        # is handed on only when set
        # gv_stats=(mean, var) with gv_iterations=N: the GV ascent behind the conversion (MLPG(gv=...)); `mlpg_`
        # keeps the MLPG object of the last conversion (its loglik_ and objective_)
        windows = delta.DELTA_WINDOWS if mlpg else delta.DELTA_WINDOWS[0:1]
        options = {} if em is None else dict(em=em)
        if gv_stats is not None or gv_iterations is not None:
            options.update(gv=gv_stats, gv_iterations=gv_iterations, gv_weight=gv_weight)
        self.mlpg_ = MLPG(self.gmm, windows=windows, diff=diff, **options)
        return self.mlpg_.transform(feature)
