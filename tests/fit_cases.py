"""Inputs and high-precision references for the kernel-level tests of the mixture fit (kwy_gmmfit.hip,
kwy_gmmfit_bd.hip, kwy_kmeans.hip): soft responsibilities laid out around the covariance kernel's skip threshold,
E-step parameters given directly (ill-conditioned covariances, weights over twelve decades, far rows, twin mixtures),
k-means blocks at the tile seams, and duplicate centres for the tie rules.

The references are plain numpy in np.longdouble (64-bit mantissa), start from the raw inputs and share nothing with
numpy_em_stats.py: a hand-written Cholesky and forward substitution, log-sum-exp, the weighted sums and the
|c|^2 - 2 <x, c> distances.  numpy_em_stats.NumpyStats is the FLOAT64 restatement: its error against these references
is what the GPU tolerances are built from (`bound`), never the kernels' own output.

test_fit_cases.py checks the inputs and references on the CPU; test_fit_kernels_gpu.py runs the kernels.  Section 5 holds
the calls whose output BYTES tools/record_fit_bits.py records and test_fit_bits_gpu.py compares."""
import functools
import math

import numpy as np
import pytest

LD = np.longdouble
if not np.finfo(LD).eps <= 2.0 ** -63:
    pytest.skip('fit_cases: np.longdouble has no 64-bit mantissa on this platform (eps > 2^-63), so there is no '
                'reference more precise than the float64 restatement', allow_module_level=True)

EPS = float(np.finfo(np.float64).eps)
TINY = float(np.finfo(np.float64).tiny)           # smallest normal double
R_MIN = 2.0 ** -200                               # include/kwy.h: the covariance sum may skip weights below
R_REL = 2.0 ** -70                                #   max(2^-200, 2^-70 nk) and no others
# The kernels sum in another order (4-wide MFMA steps, DPP trees, chunk partials) than BLAS: they may miss the
# longdouble reference by this multiple of the float64 restatement's own miss (measured: DESIGN.md, section 4, "The
# fit kernels against a longdouble reference").  A wrong fragment, tile or lane is wrong by orders of magnitude.
KERNEL_MULTIPLE = 16.0


def ld(a):
    return np.asarray(a, dtype=LD)


def bound(err64, ref_max, multiple=None):
    """what a kernel may miss the reference by: `multiple` times the float64 restatement's error, floored at 4 ulp
    of the largest reference magnitude (arrays broadcast: one bound per mixture where the statistics are per mixture)"""
    multiple = KERNEL_MULTIPLE if multiple is None else multiple
    return np.maximum(multiple * np.asarray(err64, dtype=np.float64), 4 * EPS * np.asarray(ref_max, dtype=np.float64))


# ---- longdouble references -------------------------------------------------------------------------------------------
LOG_2PI = np.log(LD(8) * np.arctan(LD(1)))


def cholesky(C):
    """lower-triangular L with L L' = C, column by column; None as soon as a pivot is not positive"""
    C = ld(C)
    D = C.shape[0]
    L = np.zeros((D, D), dtype=LD)
    for j in range(D):
        piv = C[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not piv > 0:
            return None
        L[j, j] = np.sqrt(piv)
        if j + 1 < D:
            L[j + 1:, j] = (C[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def forward_subst(L, B):
    """Z with L Z = B; B: (D, n)"""
    Z = np.empty_like(B)
    for i in range(L.shape[0]):
        Z[i] = (B[i] - L[i, :i] @ Z[:i]) / L[i, i]
    return Z


def weighted_log_density(X, weights, means, covs):
    """(n, M): log w_m + log N(x_t; mu_m, C_m)"""
    X = ld(X)
    n, D = X.shape
    M = len(weights)
    out = np.empty((n, M), dtype=LD)
    for m in range(M):
        L = cholesky(covs[m])
        assert L is not None, f'mixture {m}: covariance not positive definite'
        Z = forward_subst(L, (X - ld(means[m])).T)
        out[:, m] = np.log(ld(weights[m])) - (D * LOG_2PI + (Z * Z).sum(0)) / 2 - np.log(np.diag(L)).sum()
    return out


def weighted_log_density_bd(X, weights, means, abc):
    """the same for block-diagonal covariances given as (M, 3, h) = [a | b | c]: h independent 2 x 2 blocks
    [[a, c], [c, b]] pairing feature i with feature h + i, each through its own 2 x 2 Cholesky"""
    X = ld(X)
    n, D = X.shape
    h = D // 2
    M = len(weights)
    out = np.empty((n, M), dtype=LD)
    for m in range(M):
        a, b, c = (ld(abc[m, k]) for k in range(3))
        l11 = np.sqrt(a)
        l21 = c / l11
        l22 = np.sqrt(b - l21 * l21)
        d = X - ld(means[m])
        z1 = d[:, :h] / l11
        z2 = (d[:, h:] - l21 * z1) / l22
        out[:, m] = (np.log(ld(weights[m])) - (D * LOG_2PI + (z1 * z1).sum(1) + (z2 * z2).sum(1)) / 2
                     - np.log(l11).sum() - np.log(l22).sum())
    return out


def log_sum_exp(W):
    mx = W.max(1)
    return mx + np.log(np.exp(W - mx[:, None]).sum(1))


def responsibilities(W, lse):
    return np.exp(W - lse[:, None])


def block_sums(v, block=256):
    """sums of consecutive `block` entries (the log-likelihood parts)"""
    return np.array([v[i:i + block].sum() for i in range(0, len(v), block)], dtype=LD)


def weighted_sums(X, R):
    """(M, 1 + D): [sum_t r, sum_t r x]"""
    X, R = ld(X), ld(R)
    return np.hstack((R.sum(0)[:, None], R.T @ X))


def weighted_cov(X, R, means):
    """(M, D, D): sum_t r (x - mu)(x - mu)' over EVERY frame (a weight of exactly zero adds exactly nothing and is
    left out of the product for speed; nothing else is)"""
    n, D = X.shape
    M = R.shape[1]
    out = np.zeros((M, D, D), dtype=LD)
    for m in range(M):
        nz = R[:, m] != 0
        if nz.any():
            d = ld(X[nz]) - ld(means[m])
            out[m] = (d.T * ld(R[nz, m])) @ d
    return out


def weighted_cov_bd(X, R, means):
    """(M, 3, h): [sum r dx^2 | sum r dy^2 | sum r dx dy], dx = x_i - mu_i, dy = x_{h+i} - mu_{h+i}"""
    n, D = X.shape
    h = D // 2
    M = R.shape[1]
    out = np.zeros((M, 3, h), dtype=LD)
    for m in range(M):
        d = ld(X) - ld(means[m])
        r = ld(R[:, m])[:, None]
        dx, dy = d[:, :h], d[:, h:]
        out[m, 0], out[m, 1], out[m, 2] = (r * dx * dx).sum(0), (r * dy * dy).sum(0), (r * dx * dy).sum(0)
    return out


def centre_distances(Xc, C):
    """(n, M): |c_j|^2 - 2 <x_t, c_j> (what sklearn's Lloyd iteration minimises over j)"""
    Xc, C = ld(Xc), ld(C)
    return (C * C).sum(1)[None, :] - 2 * (Xc @ C.T)


# ---- 1, 2: soft responsibilities around the skip threshold ----------------------------------------------------------
HUGE = 2.0 ** 18           # |x - mu| of the rows that carry a threshold weight: r |d|^2 then clears the rounding bound
BIG = (1e-5, 0.3, 1.0)
# what a mixture's column looks like: the count of ACTIVE groups of four frames (a group is active when one of its
# weights reaches r_min) with the sums handed over; 'tiny' columns hold only 0 and 2^-201 .. 2^-199, so their r_min is
# 2^-200 with and without the sums
TYPES = ('all', 'none', 'one', 'seven', 'eight', 'nine', 'tiny', 'half')
COUNT = {'none': 0, 'one': 1, 'seven': 7, 'eight': 8, 'nine': 9, 'tiny': 3}

# name: (D, M, n, seed, types or None for the cycle of TYPES)
SOFT_CASES = {
    'd1_m1_n1': (1, 1, 1, 1, None),
    'd16_m3_n3': (16, 3, 3, 2, None),
    'd17_m16_n4': (17, 16, 4, 3, None),
    'd33_m17_n5': (33, 17, 5, 4, None),
    'd1_m65_n31': (1, 65, 31, 5, None),
    'd97_m3_n33': (97, 3, 33, 6, ('all', 'seven', 'tiny')),
    'd144_m16_n257': (144, 16, 257, 7, None),
    'd160_m17_n257': (160, 17, 257, 8, None),
    'd16_m65_n513': (16, 65, 513, 9, None),
    'd17_m17_n2049': (17, 17, 2049, 10, None),
    'd17_m128_n3601': (17, 128, 3601, 111, None),          # fit_cov_splits = 8: the XCD-aware numbering
    'd16_m256_n33': (16, 256, 33, 12, None),
    # one shape twice on one context: every group active, then five splits for mixtures of 0, 1 and 9 active groups
    'dense_d33_m3_n2049': (33, 3, 2049, 13, ('all', 'all', 'all')),
    'sparse_d33_m3_n2049': (33, 3, 2049, 14, ('none', 'one', 'nine')),
}


def cov_splits(n, M):
    """fit_cov_splits of kwy_gmmfit.hip"""
    s = (1024 + M - 1) // M
    s = (s + 7) & ~7
    return max(1, min(s, (n + 511) // 512, 64))


def r_min_of(nk, with_stats):
    nk = np.asarray(nk, dtype=np.float64)
    return np.maximum(R_MIN, nk * R_REL) if with_stats else np.full(nk.shape, R_MIN)


@functools.lru_cache(maxsize=None)
def soft_case(name):
    """X (n, D), means (M, D), resp (n, M), nk (M,): the column sums to pass as stats[:, 0], types (M,)

    Rows come in groups of four (one matrix instruction of k_fit_cov).  A 'huge' row lies 2^18 from every mean and
    carries ONE non-zero weight, a threshold value of the mixture that owns it (2^-70 nk, 2^-69 nk; 2^-200, 2^-199
    for a tiny column): dropping it moves the covariance by far more than rounding and the skippable weights can.
    Where a mixture has three active groups or more, the first two are active through their huge row ALONE."""
    D, M, n, seed, types = SOFT_CASES[name]
    rng = np.random.default_rng(seed)
    G = (n + 3) // 4
    X = rng.standard_normal((n, D)) * 1.5 + 0.7
    means = rng.standard_normal((M, D)) * 0.5 + 0.7
    types = tuple((types or TYPES)[m % len(types or TYPES)] for m in range(M))
    R = np.zeros((n, M))
    nk = np.zeros(M)
    rows_of = lambda g: np.arange(4 * g, min(n, 4 * g + 4))      # noqa: E731
    # groups that may hold a huge row: two rows at least (an 'all' column stays active there through another row),
    # one huge row per group; the owners are dealt out before any column is filled
    free = [int(g) for g in rng.permutation(G) if len(rows_of(g)) >= 2]
    counts, owned = [], []
    huge_rows = {}                                               # row -> owner
    for m in range(M):
        ty = types[m]
        k = G if ty == 'all' else max(1, G // 2) if ty == 'half' else min(COUNT[ty], G)
        own = []                                                 # (group, huge row) of this column
        # (a tiny column is active through huge rows alone: 2^-200 on an ordinary row would not outweigh the 2^-201s)
        for _ in range(0 if ty == 'none' else min(3 if ty == 'tiny' else 2, k, len(free))):
            g = free.pop()
            t = int(rng.choice(rows_of(g)))
            own.append((g, t))
            huge_rows[t] = m
        counts.append(len(own) if ty == 'tiny' else k)
        owned.append(own)
    is_huge = np.zeros(n, dtype=bool)
    is_huge[list(huge_rows)] = True
    for m in range(M):
        ty, k, own = types[m], counts[m], owned[m]
        tiny = ty in ('none', 'tiny')
        own_groups = [g for g, _ in own]
        rest = [int(g) for g in rng.permutation(G) if g not in own_groups]
        if ty in ('one', 'nine') and (m // len(TYPES)) % 2 == 0 and G - 1 in rest and k > len(own):
            rest.remove(G - 1)                                   # the last group, cut where n is no multiple of 4
            rest.insert(0, G - 1)
        active = own_groups + rest[:k - len(own)]
        lone = own_groups if ty == 'tiny' or len(active) >= 3 else []   # groups active through their huge row alone
        col = R[:, m]
        for g in active:
            rows = [t for t in rows_of(g) if not is_huge[t]]
            if g in lone or not rows:
                continue
            vals = rng.choice((2.0 ** -200, 2.0 ** -199) if tiny else BIG, len(rows))
            keep = rng.random(len(rows)) < 0.7
            keep[rng.integers(len(rows))] = True                 # one weight at least counts
            col[rows] = np.where(keep, vals, 0.0)
        # the values that are multiples of the column sum nk, as (row, factor): nk is the sum of the whole column
        # rounded to float64 -- what the sums kernel hands the covariance kernel -- so it is settled by iteration
        # (the small values move it by less than 2^-60 of itself: one more round at the most)
        scaled = [(t, f) for (g, t), f in zip(own, (2.0 ** -70, 2.0 ** -69))] if not tiny else []
        for (g, t), v in zip(own, (2.0 ** -200, 2.0 ** -199, 2.0 ** -199) if tiny else (0.0, 0.0)):
            col[t] = v
        # below the threshold: in the zeros of the active groups and all over the others, a fifth of the rows
        fill = np.flatnonzero((col == 0.0) & ~is_huge & (rng.random(n) < 0.2))
        which = rng.integers(1 if tiny else 3, size=len(fill))
        col[fill[which == 0]] = 2.0 ** -201
        col[fill[which == 1]] = 1e-30
        scaled += [(int(t), 2.0 ** -71) for t in fill[which == 2]]
        for _ in range(4):
            nk[m] = math.fsum(col)                               # the correctly rounded sum
            for t, f in scaled:
                col[t] = nk[m] * f
            if math.fsum(col) == nk[m]:
                break
        else:
            raise AssertionError(f'{name}: the sum of column {m} sits on a rounding tie and does not settle: '
                                 f'take another seed')
    for t, m in huge_rows.items():
        X[t] = means[m] + HUGE * (1.0 + rng.random(D)) * rng.choice((-1.0, 1.0), D)
    for a in (X, means, R, nk):
        a.setflags(write=False)
    return dict(name=name, D=D, M=M, n=n, X=X, means=means, resp=R, nk=nk, types=types, counts=tuple(counts),
                huge_rows=dict(huge_rows))


def active_group_counts(case, with_stats):
    """per mixture: groups of four frames holding a weight >= r_min (what k_fit_active_list counts)"""
    R, n, M = case['resp'], case['n'], case['M']
    G = (n + 3) // 4
    pad = np.zeros((4 * G, M))
    pad[:n] = R
    hit = pad >= r_min_of(case['nk'], with_stats)[None, :]
    return hit.reshape(G, 4, M).any(1).sum(0)


def skip_allowance(case, with_stats):
    """(M, D, D): sum over the frames with 0 < r < r_min of r |d_i| |d_j| -- what leaving out every frame the
    contract lets a kernel leave out can change an entry by (float64 is ample: the terms are all positive)"""
    X, R, means = case['X'], case['resp'], case['means']
    rmin = r_min_of(case['nk'], with_stats)
    out = np.zeros((case['M'], case['D'], case['D']))
    for m in range(case['M']):
        sk = (R[:, m] > 0) & (R[:, m] < rmin[m])
        if sk.any():
            d = np.abs(X[sk] - means[m])
            out[m] = (d.T * R[sk, m]) @ d
    return out


def _numpy_stats(X, M):
    from numpy_em_stats import NumpyStats
    return NumpyStats(X, M)


@functools.lru_cache(maxsize=None)
def soft_reference(name):
    """longdouble sums and covariances of a soft case, the float64 restatement's values, and per mixture the largest
    reference magnitude and the restatement's error"""
    c = soft_case(name)
    X, R, means = c['X'], c['resp'], c['means']
    ns = _numpy_stats(X, c['M'])
    ns.resp = R.copy()
    ns.means = means.copy()
    out = {}
    for what, ref, f64 in (('sums', weighted_sums(X, R), ns.sums().numpy()),
                           ('cov', weighted_cov(X, R, means), ns.cov().numpy())):
        flat = ref.reshape(c['M'], -1)
        out[what] = ref
        out[what + '_max'] = np.abs(flat).max(1).astype(np.float64)
        out[what + '_err64'] = np.abs(ld(f64).reshape(c['M'], -1) - flat).max(1).astype(np.float64)
    if c['D'] % 2 == 0:
        ref = weighted_cov_bd(X, R, means)
        mask_h = np.arange(c['D'] // 2)
        full = ns.cov().numpy()
        f64 = np.stack((full[:, mask_h, mask_h], full[:, mask_h + c['D'] // 2, mask_h + c['D'] // 2],
                        full[:, mask_h, mask_h + c['D'] // 2]), axis=1)
        out['cov_bd'] = ref
        out['cov_bd_max'] = np.abs(ref.reshape(c['M'], -1)).max(1).astype(np.float64)
        out['cov_bd_err64'] = np.abs(ld(f64) - ref).reshape(c['M'], -1).max(1).astype(np.float64)
    return out


# ---- 3: the E-step on given parameters -------------------------------------------------------------------------------
# name: (D, M, n, seed)
ESTEP_CASES = {
    'd1_m1_n1': (1, 1, 1, 21),
    'd16_m2_n31': (16, 2, 31, 22),
    'd17_m16_n32': (17, 16, 32, 23),
    'd144_m17_n33': (144, 17, 33, 24),
    'd160_m2_n255': (160, 2, 255, 25),
    'd16_m65_n256': (16, 65, 256, 26),
    'd17_m256_n257': (17, 256, 257, 27),
    'd16_m64_n2047': (16, 64, 2047, 28),                  # fit_lp_splits = 8 over exactly 8 tiles
    'd144_m1_n33': (144, 1, 33, 29),
    'd160_m16_n257': (160, 16, 257, 30),
    'd1_m17_n2047': (1, 17, 2047, 31),
    'd144_m65_n31': (144, 65, 31, 32),
}
LOG_GAPS = (40.0, 300.0, 650.0, 700.0, 706.0)             # log-density deficits that put posteriors next to 2^-1022


def _spd(rng, D, cond):
    """random symmetric positive definite matrix with eigenvalues log-spaced over `cond`, about 1 in the middle"""
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    lam = np.sqrt(cond) ** np.linspace(-1.0, 1.0, D) if D > 1 else np.array([cond ** 0.25])
    C = (Q * lam) @ Q.T
    return (C + C.T) / 2


def _estep_rows(rng, n, M, means, far_of):
    """rows: typical ones, one exactly on a mean, some far from every mean (by a chosen log-density deficit of
    their own mixture, and by 30 to 60 units -- dozens of standard deviations of a mixture with unit variances, hundreds
    along the short axes of an ill-conditioned one)"""
    D = means.shape[1]
    X = np.empty((n, D))
    kind = np.empty(n, dtype='U8')
    for t in range(n):
        m = int(rng.integers(M))
        z = rng.standard_normal(D)
        sel = t % 8
        if sel == 1:
            X[t], kind[t] = means[m], 'on-mean'
        elif sel == 3:
            gap = LOG_GAPS[(t // 8) % len(LOG_GAPS)]
            X[t], kind[t] = far_of(m, z * np.sqrt(2 * gap / (z @ z))), 'gap'
        elif sel == 5:
            X[t], kind[t] = means[m] + z * (30.0 + 30.0 * rng.random()) / np.sqrt(z @ z), 'far'
        else:
            X[t], kind[t] = far_of(m, z), 'typical'
    return X, kind


@functools.lru_cache(maxsize=None)
def estep_case(name):
    """weights spanning 1e-12 .. 1, covariances of condition up to 1e6, the first mixture an exact copy of the last"""
    D, M, n, seed = ESTEP_CASES[name]
    rng = np.random.default_rng(seed)
    weights = 10.0 ** -np.linspace(0.0, 12.0, M)[rng.permutation(M)] if M > 1 else np.ones(1)
    weights /= weights.sum()
    means = rng.standard_normal((M, D)) * 2.0
    covs = np.stack([_spd(rng, D, 10.0 ** (6.0 * (m + 1) / M)) for m in range(M)])
    if M > 1:
        weights[0], means[0], covs[0] = weights[M - 1], means[M - 1], covs[M - 1]
    chol = np.linalg.cholesky(covs)
    X, kind = _estep_rows(rng, n, M, means, lambda m, z: means[m] + chol[m] @ z)
    for a in (X, weights, means, covs):
        a.setflags(write=False)
    return dict(name=name, D=D, M=M, n=n, X=X, weights=weights, means=means, covs=covs, kind=kind)


@functools.lru_cache(maxsize=None)
def estep_case_bd(name):
    """the same list with an even D (1 -> 2, 17 -> 18) and covariances of the block-diagonal pattern: per pair
    a, b spread over up to five decades, c up to 0.99 sqrt(a b): conditions up to about 1e6.  `covs` are the full matrices that
    HipStatsBlockDiag.set_params reads, `abc` the (M, 3, h) form."""
    D, M, n, seed = ESTEP_CASES[name]
    D += D % 2
    h = D // 2
    rng = np.random.default_rng(seed + 100)
    weights = 10.0 ** -np.linspace(0.0, 12.0, M)[rng.permutation(M)] if M > 1 else np.ones(1)
    weights /= weights.sum()
    means = rng.standard_normal((M, D)) * 2.0
    abc = np.empty((M, 3, h))
    for m in range(M):
        spread = 10.0 ** (2.5 * (m + 1) / M)                       # a, b in [1/spread, spread]
        abc[m, 0] = spread ** rng.uniform(-1.0, 1.0, h)
        abc[m, 1] = spread ** rng.uniform(-1.0, 1.0, h)
        abc[m, 2] = rng.uniform(-0.99, 0.99, h) * np.sqrt(abc[m, 0] * abc[m, 1])
    if M > 1:
        weights[0], means[0], abc[0] = weights[M - 1], means[M - 1], abc[M - 1]
    covs = np.zeros((M, D, D))
    i = np.arange(h)
    covs[:, i, i], covs[:, h + i, h + i] = abc[:, 0], abc[:, 1]
    covs[:, i, h + i] = covs[:, h + i, i] = abc[:, 2]
    chol = np.linalg.cholesky(covs)
    X, kind = _estep_rows(rng, n, M, means, lambda m, z: means[m] + chol[m] @ z)
    for a in (X, weights, means, covs, abc):
        a.setflags(write=False)
    return dict(name=name, D=D, M=M, n=n, X=X, weights=weights, means=means, covs=covs, abc=abc, kind=kind)


def f64_weighted_log_density(X, weights, means, covs):
    """the float64 restatement's weighted log-density: NumpyStats.estep keeps only the responsibilities, so its lines
    are repeated here (test_fit_cases.py holds the two together: exp(this - logsumexp) IS NumpyStats.resp)"""
    n, D = X.shape
    wlp = np.empty((n, len(weights)))
    for m in range(len(weights)):
        L = np.linalg.cholesky(covs[m])
        z = np.linalg.solve(L, (X - means[m]).T)
        wlp[:, m] = (-0.5 * (D * np.log(2 * np.pi) + (z ** 2).sum(0)) - np.log(np.diag(L)).sum()
                     + np.log(weights[m]))
    return wlp


def _estep_reference(c, W):
    from scipy.special import logsumexp
    lse = log_sum_exp(W)
    w64 = f64_weighted_log_density(c['X'], c['weights'], c['means'], c['covs'])
    lse64 = logsumexp(w64, axis=1)
    parts = block_sums(lse)
    parts64 = np.array([lse64[i:i + 256].sum() for i in range(0, c['n'], 256)])
    wmax = float(np.abs(W).max())
    delta = float(bound(float(np.abs(ld(w64) - W).max()), wmax))
    return dict(wlp=W, lse=lse, resp=responsibilities(W, lse), parts=parts, wlp64=w64, lse64=lse64,
                wlp_max=wmax, wlp_err64=float(np.abs(ld(w64) - W).max()), delta=delta,
                parts_max=float(np.abs(parts).max()), parts_err64=float(np.abs(ld(parts64) - parts).max()))


@functools.lru_cache(maxsize=None)
def estep_reference(name):
    """wlp, lse, resp, parts in longdouble; delta: the case's bound on a weighted log-density (`bound` of the float64
    restatement's error), from which resp is allowed resp (e^{2 delta} - 1): delta on the density, delta on the
    log-sum-exp it is taken from"""
    c = estep_case(name)
    return _estep_reference(c, weighted_log_density(c['X'], c['weights'], c['means'], c['covs']))


@functools.lru_cache(maxsize=None)
def estep_reference_bd(name):
    c = estep_case_bd(name)
    return _estep_reference(c, weighted_log_density_bd(c['X'], c['weights'], c['means'], c['abc']))


def resp_bound(ref):
    """entrywise bound on |resp - reference|: relative e^{2 delta} - 1 down to the smallest normal double; a reference
    below it may come out as anything from 0 to the smallest normal (times the same factor)"""
    r = ref['resp']
    rel = np.expm1(LD(2) * LD(ref['delta']))
    return np.where(r >= TINY, r * rel, LD(TINY) * (1 + rel)).astype(LD)


def resp_sum_bound(ref, M):
    """|sum_m resp - 1| per row.  The kernel forms lse = max + log(sum exp(v - max)) and resp = exp(v - lse): rounding
    max + log(.) moves every responsibility of the row by the same factor, up to eps |lse| / 2; log and its argument
    add 3 eps, exp and the subtraction v - lse (weighted by resp: at most log M eps / 2) 2 + log M / 2, the float64
    sum of the M values in the test log2(M) / 2 + 1.  A few ulp of 1 wherever |lse| is moderate."""
    return EPS * (np.abs(ref['lse']).astype(np.float64) / 2 + 6 + np.log(M) / 2 + np.log2(M) / 2)


def indefinite_covs(case, how):
    """the case's covariances with mixture M // 2 spoilt at feature k = D // 2: row and column k zero, so that the
    kernel's k-th pivot is exactly zero ('zero') or -1 ('negative')"""
    covs = case['covs'].copy()
    m, k = case['M'] // 2, case['D'] // 2
    covs[m, k, :] = 0.0
    covs[m, :, k] = 0.0
    covs[m, k, k] = 0.0 if how == 'zero' else -1.0
    return covs


# ---- 4: k-means blocks -----------------------------------------------------------------------------------------------
# name: (n, D, M, seed)
KM_CASES = {
    'n1_d1_m1': (1, 1, 1, 41),
    'n5_d16_m16': (5, 16, 16, 42),
    'n255_d17_m17': (255, 17, 17, 43),
    'n256_d160_m64': (256, 160, 64, 44),
    'n257_d16_m65': (257, 16, 65, 45),
    'n2049_d17_m256': (2049, 17, 256, 46),
    'n2049_d160_m16': (2049, 160, 16, 47),
    'n256_d1_m17': (256, 1, 17, 48),
    'n5_d17_m256': (5, 17, 256, 49),
}
GAP = 1e-9     # best and second-best distance of every row differ by this much of the larger: labels compare exactly


@functools.lru_cache(maxsize=None)
def km_case(name):
    """rows, their float64 mean (what the driver hands km_begin), M centres (rows where there are enough, so that
    some rows lie exactly on a centre), L <= 8 candidate rows"""
    n, D, M, seed = KM_CASES[name]
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) * rng.uniform(0.5, 3.0, D) + rng.uniform(-2.0, 2.0, D)
    mean = (ld(X).sum(0) / n).astype(np.float64)
    Xc = X - mean                                               # one correctly rounded subtraction: the kernel's bits
    centres = rng.standard_normal((M, D)) * 2.0
    pick = rng.choice(n, min(n, M) // 2 + (n == 1 and M == 1), replace=False)
    centres[:len(pick)] = Xc[pick]
    centres = centres[rng.permutation(M)]
    L = min(8, n)
    cand = Xc[rng.choice(n, L, replace=False)].copy()
    for a in (X, mean, Xc, centres, cand):
        a.setflags(write=False)
    return dict(name=name, n=n, D=D, M=M, X=X, mean=mean, Xc=Xc, centres=centres, cand=cand)


def _err(f64, ref):
    return float(np.abs(ld(f64) - ref).max()), float(np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def km_reference(name):
    """per block: (longdouble reference, float64 restatement's error, largest reference magnitude).  Blocks that take
    another block's output take it from HERE, rounded to float64: xsq and closest for the candidates, the one-hot
    labels for the sums, the sums for the update."""
    import torch
    c = km_case(name)
    X, Xc, mean, n, D, M = c['X'], c['Xc'], c['mean'], c['n'], c['D'], c['M']
    ns = _numpy_stats(X, M)
    t = torch.from_numpy
    out = {}
    for key, shift in (('colstats', None), ('colstats_shift', mean)):
        x = ld(X) - (ld(shift) if shift is not None else 0)
        ref = np.stack((x.sum(0), (x * x).sum(0)))
        out[key] = (ref,) + _err(ns.km_colstats(None if shift is None else t(mean.copy())).numpy(), ref)
    ns.km_begin(t(mean.copy()))
    xc = ld(X) - ld(mean)
    out['Xc'] = (xc,) + _err(ns.Xc, xc)
    xsq = (ld(Xc) * ld(Xc)).sum(1)                               # of the float64 rows the later blocks read
    out['xsq'] = (xsq,) + _err(ns.xsq, xsq)
    xsq64 = xsq.astype(np.float64)
    ns.xsq = xsq64.copy()
    y = ld(c['cand'])
    d = np.maximum((-2 * (y @ ld(Xc).T) + (y * y).sum(1)[:, None]) + ld(xsq64)[None, :], 0)
    pots = ns.km_candidates(t(c['cand'].copy()), use_closest=False).numpy()
    out['newd'] = (d,) + _err(ns.newd, d)
    out['pots'] = (d.sum(1),) + _err(pots, d.sum(1))
    closest64 = d[min(2, len(d) - 1)].astype(np.float64)
    ns.closest = closest64.copy()
    d2 = np.minimum(ld(closest64)[None, :], d)
    pots = ns.km_candidates(t(c['cand'].copy()), use_closest=True).numpy()
    out['newd_closest'] = (d2,) + _err(ns.newd, d2)
    out['pots_closest'] = (d2.sum(1),) + _err(pots, d2.sum(1))
    out['closest64'], out['xsq64'] = closest64, xsq64
    dist = centre_distances(Xc, c['centres'])
    labels = dist.argmin(1).astype(np.int32)
    out['dist'], out['labels'] = dist, labels
    ns.km_assign(t(c['centres'].copy()))
    out['labels64'] = ns.labels.copy()
    onehot = np.zeros((n, M))
    onehot[np.arange(n), labels] = 1.0
    ns.resp = onehot
    st = weighted_sums(Xc, onehot)
    out['sums'] = (st,) + _err(ns.km_sums().numpy(), st)
    st64 = st.astype(np.float64)
    has = st64[:, 0] > 0
    new = ld(c['centres']).copy()
    new[has] = ld(st64[has, 1:]) / ld(st64[has, :1])
    shift2 = ((new - ld(c['centres'])) ** 2).sum(1)
    new64 = np.empty((M, D))
    sh64 = ns.km_update(t(st64.copy()), t(c['centres'].copy()), t(new64)).numpy()
    out['update'] = (new,) + _err(new64, new)
    out['shift2'] = (shift2,) + _err(sh64, shift2)
    out['sums64'] = st64
    return out


def distance_gaps(dist, same=None):
    """per row: (second-best - best) / max(|best|, |second-best|); `same[j]`: centres that are copies of centre j
    do not count as its rivals"""
    n, M = dist.shape
    if M == 1:
        return np.full(n, np.inf, dtype=LD)
    if same is None:
        two = np.sort(dist, axis=1)[:, :2]
        return (two[:, 1] - two[:, 0]) / np.abs(two).max(1)
    order = np.argsort(dist, axis=1, kind='stable')
    best = dist[np.arange(n), order[:, 0]]
    gaps = np.empty(n, dtype=LD)
    for t in range(n):
        rivals = [j for j in order[t, 1:] if same is None or same[j] != same[order[t, 0]]]
        if not rivals:
            gaps[t] = np.inf
            continue
        second = dist[t, rivals[0]]
        gaps[t] = (second - best[t]) / max(abs(second), abs(best[t]))
    return gaps


# duplicate centres: equal distances, the same bits -- the lower index has to win in each arrangement
TIE_PAIRS = ((2, 9),        # two lanes of one 16-column block
             (3, 19),       # two blocks of one lane
             (5, 70),       # two groups of 64 centres
             (40, 129))     # ... and the last, partly filled group
TIE_SHAPE = (300, 17, 130, 51)      # n, D, M, seed


@functools.lru_cache(maxsize=None)
def tie_case():
    """centres with the copies of TIE_PAIRS; rows 10 i .. 10 i + 9 lie next to pair i, so a copy is their nearest
    centre; `same[j]` names the lowest index among the copies of centre j"""
    n, D, M, seed = TIE_SHAPE
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((M, D)) * 2.0
    same = np.arange(M)
    for lo, hi in TIE_PAIRS:
        centres[hi] = centres[lo]
        same[hi] = lo
    Xc = rng.standard_normal((n, D)) * 2.0
    near = {}
    for i, (lo, hi) in enumerate(TIE_PAIRS):
        rows = np.arange(10 * i, 10 * i + 10)
        Xc[rows] = centres[lo] + 0.05 * rng.standard_normal((10, D))
        near[lo] = rows
    dist = centre_distances(Xc, centres)
    for a in (Xc, centres):
        a.setflags(write=False)
    return dict(n=n, D=D, M=M, Xc=Xc, centres=centres, same=same, near=near, dist=dist,
                labels=dist.argmin(1).astype(np.int32))


# ---- 5: the bits of the fit and k-means entries (tests/golden/fit_bits_parent.npz) ------------------------------------
# tools/record_fit_bits.py records what the functions below return on the build the bits are held to;
# test_fit_bits_gpu.py calls them on the build under test and compares bytes.  The cases sit on the seams of one, two,
# nine and ten column blocks, of the 16 / 32 / 256-row tiles and of the 64-centre groups.
BITS_ESTEP = ('d1_m1_n1', 'd16_m2_n31', 'd17_m16_n32', 'd144_m17_n33', 'd160_m2_n255', 'd16_m65_n256')
BITS_STATS = ('d1_m1_n1', 'd16_m3_n3', 'd17_m16_n4', 'd33_m17_n5', 'd97_m3_n33')      # kept as arrays
BITS_STATS_DIGEST = ('d144_m16_n257', 'd160_m17_n257')                               # megabytes: SHA-256 only
BITS_KM = ('n1_d1_m1', 'n5_d16_m16', 'n255_d17_m17', 'n256_d160_m64', 'n257_d16_m65', 'n5_d17_m256')


def digest(a):
    """SHA-256 of an array's bytes, as a string array an .npz holds"""
    import hashlib
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def tril_pack(sxx):
    """(M, D, D) -> (M, D (D + 1) / 2): the lower triangles, row by row (the fixture keeps these: the covariance
    statistics are symmetric to the bit, and `tril_unpack` gives the whole array back)"""
    i, j = np.tril_indices(sxx.shape[1])
    return np.ascontiguousarray(sxx[:, i, j])


def tril_unpack(packed, D):
    i, j = np.tril_indices(D)
    out = np.empty((packed.shape[0], D, D), dtype=packed.dtype)
    out[:, i, j] = packed
    out[:, j, i] = packed
    return out


def _hip_stats(X, M, ctx):
    from kwiiyatta_amd.converter.gmm_fit import HipStats
    return HipStats(np.array(X), M, ctx=ctx)


def _to(hs, a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(hs.dev)


def bits_estep(ctx, name):
    """kwy_gmm_em_estep_dev (k_fit_prec, k_fit_logprob, k_fit_resp) on estep_case(name):
    responsibilities (n, M), log-likelihood parts, status word"""
    c = estep_case(name)
    hs = _hip_stats(c['X'], c['M'], ctx)
    with hs.scope():
        hs.set_params(np.array(c['weights']), np.array(c['means']), np.array(c['covs']))
        hs.estep()
        return hs.resp.cpu().numpy(), hs.ll.cpu().numpy(), hs.status.cpu().numpy()[:1]


def bits_stats(ctx, name):
    """kwy_gmm_em_sums_dev (k_fit_sums, k_fit_reduce) and kwy_gmm_em_cov_dev (k_fit_active .. k_fit_cov,
    k_fit_reduce_sym) on soft_case(name): sums (M, 1 + D), sxx (M, D, D) without the sums (what kwy_gmm_em_cov_dev
    computes), sxx with the case's sums handed over (kwy_gmm_em_cov_stats_dev)"""
    c = soft_case(name)
    hs = _hip_stats(c['X'], c['M'], ctx)
    with hs.scope():
        hs.resp.copy_(_to(hs, c['resp']))
        hs.means.copy_(_to(hs, c['means']))
        sums = hs.sums().cpu().numpy()
        cov = hs.cov(None).cpu().numpy()
        st = sums.copy()
        st[:, 0] = c['nk']
        cov_stats = hs.cov(_to(hs, st)).cpu().numpy()
    return sums, cov, cov_stats


def _bits_assign(ctx, X, mean, centres, M):
    hs = _hip_stats(X, M, ctx)
    with hs.scope():
        hs.km_begin(_to(hs, mean))
        cd = _to(hs, centres)
        first = int(hs.km_assign(cd).item())               # from -1 everywhere
        labels = hs.labels.cpu().numpy()
        again = int(hs.km_assign(cd).item())               # the same centres
        hs.km_end()
    return labels, np.array([first, again], dtype=np.int64)


def bits_km(ctx, name):
    """kwy_km_assign_dev (k_km_assign, k_km_labels) on km_case(name): labels, [changed from -1, changed again]"""
    c = km_case(name)
    return _bits_assign(ctx, c['X'], c['mean'], c['centres'], c['M'])


def bits_tie(ctx):
    """... on tie_case(), centred on zero"""
    c = tie_case()
    return _bits_assign(ctx, c['Xc'], np.zeros(c['D']), c['centres'], c['M'])
