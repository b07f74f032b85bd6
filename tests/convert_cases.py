"""Inputs of tests/test_convert_kernels_gpu.py and of the recorder of its fixture (tools/record_convert_bits.py): joint
Gaussian mixtures, feature rows and mel-cepstra on the seams of the conversion kernels' maps, and the calls through
the C ABI that both make.  A plain module, so the recorder and the tests see the same arrays.

Seams: k_gmm_logp takes 16 frames per MFMA sub-tile, 32 per wavefront and 256 per workgroup tile; it has one code
path per 16-column block count of the feature dimension D (D = 3 d for a mel-cepstrum of order d), and its last block
ends after ceil(D / 4) k-steps.  k_gmm_cond takes four frames per wavefront, sixteen per workgroup, and 64 mixtures per
pass of its arg-max (lane l looks at mixtures l, l + 64, ...).
"""
import ctypes

import numpy as np

SEED = 20
T_SEAMS = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257)
T_SHORT = (1, 15, 16, 17, 31, 32, 33)
MIXTURES = (1, 3, 64)

# frame-wise conversion (kwy_gmm_convert_frames_dev) of the first T rows of one matrix per (D, M): (D, M, the T values).
# D = 82 is the widest mixture the preparation kernel takes (six column blocks, one k-step in the last); 18, 33, 48 and
# 60 fill in two, three (ragged and full) and four blocks.
FRAMES = tuple((6, M, T_SEAMS) for M in MIXTURES) + ((72, 1, T_SHORT), (72, 3, T_SHORT), (72, 64, T_SEAMS),
                                                      (82, 3, T_SHORT)) + tuple((D, 3, T_SHORT) for D in (18, 33, 48, 60))
# mel-cepstrum conversion (kwy_convert_mcep_dev: deltas, hard arg-max, conditional means, MLPG): (d, M, the T values).
# d = 6, 11, 16, 20, 27: two, three (ragged and full), four and six column blocks.
MCEP = tuple((2, M, T_SEAMS) for M in MIXTURES) + ((24, 3, T_SEAMS), (24, 1, (17, 33)), (24, 64, (17, 33, 257)),
                                                    (27, 3, (17, 33))) + tuple((d, 3, (33,)) for d in (6, 11, 16, 20))
# D = 144 and D = 150, nine column blocks and more: wider than any mixture the library prepares.  k_gmm_prep holds three
# D x D matrices in LDS (D <= 82, six column blocks -- all the log-density kernel is built for), so the library refuses
# both (KWY_EINVAL) before any kernel runs, in every build so far.  The fixture records that return code, and the tests
# hold the tree to it.
REFUSED = ((48, 3, 17), (50, 3, 17))
BATCH = (24, 3, (17, 256, 33))
MC2SP = ((2048, (1, 16, 17)), (1024, (1, 16, 17)))       # K = 1025 and K = 513
MC2SP_ORDER, MC2SP_ALPHA, MC2SP_BIN_STEP = 24, 0.55, 4   # the fixture keeps every 4th bin and the last one


def mixture(D, M, tag, equal_x=False, spread=1.0, low=0):
    """weights (M), means (M, 2 D), covariances (M, 2 D, 2 D) of a joint mixture over [x, y]; well conditioned, means a
    few standard deviations apart (spread scales the x-means: small values make neighbours overlap).  equal_x: every
    mixture shares mixture 0's x-mean and x-covariance and differs in mu_y and in the y rows and columns of the covariance;
    the first `low` mixtures have half the weight of the others, which all weigh the same, so the log-densities of a frame
    are one number for mixtures low .. M - 1 and a smaller one below."""
    rng = np.random.default_rng([SEED, D, M, tag])
    w = rng.uniform(0.5, 1.5, M)
    if equal_x:
        w[:] = 1.0
        w[:low] = 0.5
    w /= w.sum()
    mu = rng.standard_normal((M, 2 * D))
    mu[:, :D] *= spread
    cov = np.empty((M, 2 * D, 2 * D))
    for m in range(M):
        B = rng.standard_normal((2 * D, 2 * D)) / np.sqrt(2 * D)
        cov[m] = 0.3 * (B @ B.T) + 0.2 * np.eye(2 * D)
    if equal_x:     # y = C_m x + noise of covariance R_m over mixture 0's x: positive definite by construction
        mu[:, :D] = mu[0, :D]
        Sxx = cov[0, :D, :D].copy()
        for m in range(M):
            C = rng.standard_normal((D, D)) / np.sqrt(D)
            R = cov[m, D:, D:].copy()
            cov[m, :D, :D] = Sxx
            cov[m, D:, :D] = C @ Sxx
            cov[m, :D, D:] = (C @ Sxx).T
            cov[m, D:, D:] = C @ Sxx @ C.T + R
            cov[m, D:, D:] = 0.5 * (cov[m, D:, D:] + cov[m, D:, D:].T)
    return w, mu, cov


def frames_case(D, M):
    """(weights, means, covariances, rows) of a frame-wise conversion: the x-means lie so close together that several
    mixtures share the posterior of a row, so the output moves with every bit of their log-densities"""
    w, mu, cov = mixture(D, M, 3, spread=1.0 / np.sqrt(D))
    T = max(max(Ts) for D_, M_, Ts in FRAMES if (D_, M_) == (D, M))
    rng = np.random.default_rng([SEED, D, M, 3, 1])
    return w, mu, cov, np.ascontiguousarray(mu[np.arange(T) % M, :D] + 0.4 * rng.standard_normal((T, D)))


def posterior(lp):
    p = np.exp(lp - lp.max(axis=1, keepdims=True))
    return p / p.sum(axis=1, keepdims=True)


def mcep(T, d, M, tag):
    """T x (d + 1) mel-cepstra: column 0 (power) is passed through, columns 1.. are a track that dwells near the static
    part of one x-mean after the other of the mixture over D = 3 d, so the arg-max changes along the utterance"""
    _, mu, _ = mixture(3 * d, M, tag)
    rng = np.random.default_rng([SEED, d, M, tag, T, 2])
    mc = np.empty((T, d + 1))
    mc[:, 0] = rng.standard_normal(T)
    mc[:, 1:] = mu[(np.arange(T) // 5) % M, :d] + 0.3 * rng.standard_normal((T, d))
    return mc


def delta_features(x):
    """static, delta and delta-delta rows (windows [1], [-0.5, 0, 0.5], [1, -2, 1], zeros outside the utterance)"""
    xp = np.pad(x, ((1, 1), (0, 0)))
    return np.concatenate([x, 0.5 * (xp[2:] - xp[:-2]), xp[2:] - 2.0 * x + xp[:-2]], axis=1)


def mc2sp_rows(T):
    rng = np.random.default_rng([SEED, T, 3])
    mc = 0.3 * rng.standard_normal((T, MC2SP_ORDER + 1)) / (1.0 + np.arange(MC2SP_ORDER + 1))
    mc[:, 0] -= 5.0
    return np.ascontiguousarray(mc)


def mc2sp_sample(sp):
    return np.ascontiguousarray(np.concatenate([sp[:, ::MC2SP_BIN_STEP], sp[:, -1:]], axis=1))


# ---- the calls (device pointers through the C ABI) ---------------------------------------------------------------
def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def convert_frames(ctx, x, w, mu, cov, diff=0):
    """kwy_gmm_convert_frames_dev: the posterior-weighted conditional mean of every row of x"""
    import torch
    from kwiiyatta_amd import _lib
    T, D = x.shape
    dx, dw, dmu, dcov = _dev(x, w, mu, cov)
    y = torch.full((T, D), np.nan, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    _lib.check(ctx, _lib.lib.kwy_gmm_convert_frames_dev(ctx.handle, dx.data_ptr(), T, D, len(w), dw.data_ptr(),
                                                        dmu.data_ptr(), dcov.data_ptr(), diff, y.data_ptr()))
    ctx.sync()
    return y.cpu().numpy()


def prepare(ctx, d, w, mu, cov, diff=0):
    """kwy_gmm_prepare_dev: (return code, the model's device buffer)"""
    import torch
    from kwiiyatta_amd import _lib
    dw, dmu, dcov = _dev(w, mu, cov)
    model = torch.zeros(_lib.lib.kwy_gmm_model_doubles(d, len(w)), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    rc = _lib.lib.kwy_gmm_prepare_dev(ctx.handle, dw.data_ptr(), dmu.data_ptr(), dcov.data_ptr(), d, len(w), diff,
                                      model.data_ptr())
    return rc, model


def convert_mcep(ctx, model, M, mcs):
    """kwy_convert_mcep_dev for one matrix, kwy_convert_mcep_batch_dev for a list of them"""
    import torch
    from kwiiyatta_amd import _lib
    lib = _lib.lib
    batch = isinstance(mcs, (list, tuple))
    d = (mcs[0] if batch else mcs).shape[1] - 1
    ins = _dev(*(mcs if batch else [mcs]))
    outs = [torch.full(tuple(a.shape), np.nan, dtype=torch.float64, device='cuda') for a in ins]
    torch.cuda.synchronize()
    if batch:
        jobs = _lib.job_array(_lib.ConvertJob, [(a, a.shape[0], o) for a, o in zip(ins, outs)])
        _lib.check(ctx, lib.kwy_convert_mcep_batch_dev(ctx.handle, ctypes.cast(jobs, ctypes.c_void_p), len(ins), d, M,
                                                       model.data_ptr()))
    else:
        _lib.check(ctx, lib.kwy_convert_mcep_dev(ctx.handle, ins[0].data_ptr(), ins[0].shape[0], d, M, model.data_ptr(),
                                                 outs[0].data_ptr()))
    ctx.sync()
    res = [o.cpu().numpy() for o in outs]
    return res if batch else res[0]


def mc2sp(ctx, mc, fft):
    import torch
    from kwiiyatta_amd import _lib
    dmc, = _dev(mc)
    sp = torch.full((mc.shape[0], fft // 2 + 1), np.nan, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    _lib.check(ctx, _lib.lib.kwy_mc2sp_dev(ctx.handle, dmc.data_ptr(), mc.shape[0], mc.shape[1] - 1, MC2SP_ALPHA, fft,
                                           sp.data_ptr()))
    ctx.sync()
    return sp.cpu().numpy()


def frames_key(D, M):
    return f'frames_{D}_{M}'


def mcep_key(d, M, T):
    return f'mcep_{d}_{M}_{T}'


# ---- float64 numpy references from the raw mixture parameters ------------------------------------------------------
def ref_logp(X, w, mu, cov):
    """weighted log-densities log w_m + log N(x_t; mu_x,m, S_xx,m): (T, M)"""
    T, D = X.shape
    out = np.empty((T, len(w)))
    for m in range(len(w)):
        L = np.linalg.cholesky(cov[m, :D, :D])
        z = np.linalg.solve(L, (X - mu[m, :D]).T)
        out[:, m] = np.log(w[m]) - 0.5 * D * np.log(2 * np.pi) - np.log(np.diag(L)).sum() - 0.5 * (z * z).sum(axis=0)
    return out


def ref_cond(X, mu, cov, m):
    """conditional mean of y given the rows of X under mixture m"""
    D = X.shape[1]
    return mu[m, D:] + np.linalg.solve(cov[m, :D, :D], (X - mu[m, :D]).T).T @ cov[m, :D, D:]


def logp_gap(lp):
    """smallest distance over the frames between the best and the second-best log-density"""
    if lp.shape[1] < 2:
        return np.inf
    s = np.sort(lp, axis=1)
    return float((s[:, -1] - s[:, -2]).min())


def ref_frames(X, w, mu, cov):
    post = posterior(ref_logp(X, w, mu, cov))
    return sum(post[:, m:m + 1] * ref_cond(X, mu, cov, m) for m in range(len(w)))


def ref_mcep(mc, w, mu, cov, mix=None):
    """hard arg-max mixture per frame (or the given one), conditional means and diagonal variances, then per static
    dimension the trajectory that solves W' P W y = W' P E densely"""
    T, d = mc.shape[0], mc.shape[1] - 1
    D = 3 * d
    X = delta_features(mc[:, 1:])
    pick = ref_logp(X, w, mu, cov).argmax(axis=1) if mix is None else np.full(T, mix)
    E, Dv = np.empty((T, D)), np.empty((T, D))
    for m in np.unique(pick):
        sel = pick == m
        E[sel] = ref_cond(X[sel], mu, cov, m)
        sxx, syy = np.diag(cov[m, :D, :D]), np.diag(cov[m, D:, D:])
        Dv[sel] = syy - np.diag(cov[m, D:, :D]) / sxx * np.diag(cov[m, :D, D:])
    eye = np.eye(T)
    up, dn = np.eye(T, k=1), np.eye(T, k=-1)
    W = np.concatenate([eye, 0.5 * (up - dn), up - 2.0 * eye + dn])        # (3 T, T)
    out = mc.copy()
    for c in range(d):
        P = 1.0 / np.concatenate([Dv[:, w_ * d + c] for w_ in range(3)])
        mean = np.concatenate([E[:, w_ * d + c] for w_ in range(3)])
        out[:, 1 + c] = np.linalg.solve(W.T @ (P[:, None] * W), W.T @ (P * mean))
    return out
