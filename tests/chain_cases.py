"""The filter chain of the device conversion driver (`corpus.ConvertWave`: modulation spectrum, then global variance,
then power / emphasis; plain and differential rows) composed by hand and stated in numpy -- the inputs, the table of
option combinations, the composite of the three statements (ms_cases, gv_cases, power_cases), its one-line mutants and
its bound.  The yardstick of tests/test_chain_cases.py (the composite's own claims) and of
tests/test_convert_chain_gpu.py (the driver and `MelCepstrumConverter.convert` against it).

The composite, for one utterance with source rows `src`, plain conversion `plain` and differential conversion `diff`
(all (T, order + 1)):

    p1 = MS(plain)                          b1 = diff + (MS(plain) - plain)           (c1.., ms_cases.postfilter)
    p2 = p1 + s (r - 1)(p1 - mean p1)       b2 = b1 + s (r - 1)(p1 - mean p1)         (r from the moments of p1)
    P  = POWER(p2; ref)                     a = src + [0 | b2[:, 1:]];  D = [0 | b2[:, 1:]] + (POWER(a; ref) - a)

The bound is put together from what the single filters' tests state, see `bounds`."""
from types import SimpleNamespace

import numpy as np

import convert_cases as cc
import gv_cases as gc
import ms_cases as mc
import power_cases as pc

U = 2.0 ** -53
FS, ORDER, FRAME_PERIOD, MS_LENGTH, FFT = 16000, 24, 5.0, 512, 1024
SECONDS = (0.25, 0.4, 0.3)                  # 51, 81 and 61 frames: ragged offsets
FRAMES = (51, 81, 61)
MS_STRENGTH, GV_STRENGTH, BETA = 0.5, 0.75, 0.25
KERNEL_BOUND = 2e-14                        # test_power_gpu.KERNEL_BOUND (test_chain_cases.py holds the two together)
MUTANTS = ('gv_first', 'moments_before_ms', 'base_not_updated')


# ---- inputs ------------------------------------------------------------------------------------------------------------
def utterances(n=3, seconds=SECONDS, seed=70):
    """n synthetic (x, f0, t) triples of the given lengths (cycled), f0 around 140 and 190 Hz in turn"""
    from kwiiyatta_amd.synthetic import make_utterance
    return [make_utterance(seed=seed + i, fs=FS, seconds=seconds[i % len(seconds)], f0_base=(140.0, 190.0)[i % 2])
            for i in range(n)]


def mixture(tag=7):
    w, mu, cov = cc.mixture(3 * ORDER, 2, tag)
    return SimpleNamespace(weights_=w, means_=mu, covariances_=cov)


def band_mixture(bands, tag=8):
    w, mu, cov = cc.mixture(3 * bands, 2, tag)
    return SimpleNamespace(weights_=w, means_=mu, covariances_=cov)


def host_rows(seed=0, frames=FRAMES):
    """per utterance (src, plain, diff) as a wave leaves them, made on the host: rows with the decay of speech smoothed
    along time (a trajectory MLPG made moves slowly), the plain conversion with the source's c0, the differential one
    plain - src in c1.. with the source's c0 in column 0"""
    rng = np.random.default_rng([seed, 41])
    out = []
    for T in frames:
        def smooth(c0):
            x = pc.rows_like_speech(rng, T + 4, ORDER, c0=c0)
            return np.ascontiguousarray((x[:-4] + 2 * x[1:-3] + 3 * x[2:-2] + 2 * x[3:-1] + x[4:]) / 9.0)
        src, plain = smooth(-8.0), smooth(0.0)
        plain[:, 0] = src[:, 0]
        diff = plain - src
        diff[:, 0] = src[:, 0]
        out.append((src, plain, np.ascontiguousarray(diff)))
    return out


def statistics(plain_rows, seed=3):
    """the statistics of a table run, from the plain wave's own converted rows (a list of (T, order + 1) arrays):
    gv_stats by gv_cases.gv_for_ratios with ratios within [0.7, 1.6] and ms_stats by ms_cases.stats_for, both around the
    longest utterance; gv_var a positive vector"""
    rng = np.random.RandomState(seed)
    x = max(plain_rows, key=len)
    gv = gc.gv_for_ratios(x, rng.uniform(0.7, 1.6, x.shape[1] - 1))
    G, N = mc.stats_for(x, MS_LENGTH, rng)
    return SimpleNamespace(gv=gv, gv_var=(0.05 * gv) ** 2, ms=(G, N))


def options(stats, ms=False, gv=False, beta=0.0, keep_power=False):
    """the ConvertOptions keywords of one filter subset"""
    out = {}
    if ms:
        out.update(ms_stats=stats.ms, ms_length=MS_LENGTH, ms_strength=MS_STRENGTH)
    if gv:
        out.update(gv_stats=stats.gv, gv_strength=GV_STRENGTH)
    if beta or keep_power:
        out.update(postfilter_beta=beta, keep_power=keep_power)
    return out


BOTH = dict(beta=BETA, keep_power=True)
# name -> (filters, diff, the conversion's own options: mlpg_em, mlpg_gv); a filter subset is dict(ms, gv, beta, keep_power)
TABLE = {
    'none': (dict(), True, {}),
    'ms': (dict(ms=True), True, {}),
    'gv': (dict(gv=True), True, {}),
    'ms+gv': (dict(ms=True, gv=True), True, {}),
    'beta': (dict(beta=BETA), True, {}),
    'keep': (dict(keep_power=True), True, {}),
    'power': (dict(BOTH), True, {}),
    'ms+power': (dict(ms=True, **BOTH), True, {}),
    'gv+power': (dict(gv=True, **BOTH), True, {}),
    'ms+gv+power': (dict(ms=True, gv=True, **BOTH), True, {}),
    'ms+gv+power, plain only': (dict(ms=True, gv=True, **BOTH), False, {}),
    'none, plain only': (dict(), False, {}),
    'em: ms+gv+power': (dict(ms=True, gv=True, **BOTH), True, dict(mlpg_em=1)),
    'em: gv': (dict(gv=True), True, dict(mlpg_em=1)),
    'em: none': (dict(), True, dict(mlpg_em=1)),
    'gvgen: power': (dict(BOTH), True, dict(mlpg_em=1, mlpg_gv=3, gv_weight=2.0)),
    'gvgen: none': (dict(), True, dict(mlpg_em=1, mlpg_gv=3, gv_weight=2.0)),
}
NUMERIC = ('ms+gv+power', 'ms+gv+power, plain only', 'gv+power')        # the entries held against the composite
PLAIN_ONLY_OF = {'ms+gv+power, plain only': 'ms+gv+power', 'none, plain only': 'none'}


# ---- the composite -----------------------------------------------------------------------------------------------------
def early(plain, base, stats, ms, gv, variant=None):
    """MS -> GV on c1..cN of the plain rows (base None) or with the differential rows as `base`.  variant: a mutant --
    'gv_first': GV before MS; 'moments_before_ms': GV's ratio and mean from the rows MS has not filtered yet;
    'base_not_updated': the differential rows miss MS's change"""
    G, N = stats.ms
    k, s = (MS_STRENGTH if ms else 0.0), (GV_STRENGTH if gv else 0.0)
    if variant is None:
        return mc.convert_chain(plain, base, G, N, k, stats.gv, s)
    assert ms and gv and variant in MUTANTS
    if variant == 'gv_first':
        p1 = gc.postfilter(plain, stats.gv, s)[0]
        b1 = p1 if base is None else gc.postfilter(plain, stats.gv, s, base=base)[0]
        return mc.postfilter(p1, G, N, k, base=b1)[0]
    p1 = mc.postfilter(plain, G, N, k)[0]
    b1 = p1 if base is None else mc.postfilter(plain, G, N, k, base=base)[0]
    if variant == 'base_not_updated':
        return gc.postfilter(p1, stats.gv, s, base=p1 if base is None else base)[0]
    m = gc.column_moments(plain)                             # 'moments_before_ms'
    y = b1.copy()
    for d in range(1, plain.shape[1]):
        r = np.sqrt(stats.gv[d] / (m[d, 2] / m[d, 0]))
        y[:, d] = b1[:, d] + s * (r - 1.0) * (p1[:, d] - m[d, 1])
    return y


def composite(src, plain, diff, stats, alpha, ms=False, gv=False, beta=0.0, keep_power=False, variant=None):
    """(P, D): the filtered plain and differential rows of one utterance in float64 numpy; D is None without `diff`"""
    p2 = early(plain, None, stats, ms, gv, variant) if (ms or gv) else plain.copy()
    b2 = None if diff is None else (early(plain, diff, stats, ms, gv, variant) if (ms or gv) else diff.copy())
    if not (beta or keep_power):
        return p2, b2
    ref = src if keep_power else None
    P, status = pc.postfilter(p2, alpha, FFT, beta, ref=ref)
    assert status == 0
    D = None
    if b2 is not None:
        base = np.hstack((np.zeros_like(b2[:, :1]), b2[:, 1:]))
        D, status = pc.postfilter(src + base, alpha, FFT, beta, ref=ref, base=base)
        assert status == 0
    return P, D


def bounds(src, plain, diff, stats, ms=False, gv=False, beta=0.0, keep_power=False):
    """(bound of P, bound of D) per column, from the numbers the single filters' tests state:
    MS     ms_cases.filter_bounds(plain) per column, for the plain and the differential rows alike (test_ms_gpu.py);
    GV     an error B of p1 and b1 comes through y = b1 + (r - 1)(p1 - m) as B (1 + |r - 1|) directly and as
           r B max|p1 - m| / sigma through the ratio, plus the filter's own gv_cases.apply_bound (test_ms_gpu.py,
           test_converter_composition_against_the_yardstick; stated there at strength 1, an upper bound below it);
    power  the kernel's own KERNEL_BOUND plus 4 (order + 1) times the largest incoming error (test_power_gpu.py: the
           emphasis carries a difference with a gain below 4 per coefficient, the c0 correction with one below 1 per
           coefficient); the differential rows enter as src + [0 | b2], one more rounding of that sum."""
    cols = plain.shape[1]
    G, N = stats.ms
    err = mc.filter_bounds(plain, G, N, MS_STRENGTH) if ms else np.zeros(cols)
    p1 = mc.postfilter(plain, G, N, MS_STRENGTH)[0] if ms else plain
    if gv:
        r = np.concatenate(([1.0], gc.ratios(p1, stats.gv)))
        dev = np.abs(p1 - p1.mean(axis=0)).max(axis=0) / p1.std(axis=0)
        err = err * (1 + np.abs(r - 1) + r * dev) + np.array([gc.apply_bound(p1, r[d], d) for d in range(cols)])
        err[0] = 0.0
    if not (beta or keep_power):
        return err, err
    carried = KERNEL_BOUND + 4 * cols * err.max()
    b2 = composite(src, plain, diff, stats, 0.0, ms, gv)[1] if diff is not None else None
    summed = 0.0 if b2 is None else 2 * U * np.abs(src + b2).max()
    return np.full(cols, carried), np.full(cols, KERNEL_BOUND + 4 * cols * (err.max() + summed))


def one_ulp(rng, a):
    """`a` with every element moved by one unit in its last place, up or down at random"""
    return np.where(rng.integers(0, 2, a.shape) == 1, np.nextafter(a, np.inf), np.nextafter(a, -np.inf))
