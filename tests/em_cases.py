"""Inputs, numpy restatement and C ABI calls of the EM trajectory conversion over soft mixture posteriors
(kwy_gmm_mlpg_em, kwy_convert_mcep_em_dev, kwy_convert_mcep_em_batch_dev; the arithmetic is written out in
include/kwy.h).  A plain module shared by tests/test_em_cases.py (CPU) and tests/test_em_gpu.py.

The E-step kernel takes 16 frames per wavefront and 64 per workgroup (ML_EM_TILE in kwy_mlpg.hip), has one code path
per 16-column block count of D = 3 d (d = 2, 6, 11, 16, 20 / 24, 27: one to six blocks), and walks any number of
mixtures serially (M = 70: beyond the 64 lanes the other conversion kernels spread mixtures over).
"""
import ctypes
import functools

import numpy as np

import convert_cases as cc

KWY_MLPG_EM_MAX = 16
FRAME_TILE = 64
KWY_BATCH_MAX = 16

# (d, M, spread, tag, the T values, N).  T = FRAME_TILE - 1, FRAME_TILE, FRAME_TILE + 1 join the (2, 3) row.
TABLE = (
    (2, 1, 1.0, 7, (1, 2, 3, 17), 2),
    (2, 3, 1.0, 7, (1, 2, 3, 15, 16, 17, 33, 63, 64, 65, 257), 4),
    (2, 64, 1.0, 7, (33, 257), 4),
    (2, 70, 1.0, 7, (33,), 2),
    (24, 3, 0.2, 8, (17, 33, 257), 4),
    (24, 64, 0.2, 8, (33,), 4),
    (24, 64, 0.2, 8, (129, 257), 1),
    (24, 64, 1.0, 7, (257,), 4),
    (27, 3, 0.2, 8, (33,), 2),
) + tuple((d, 3, 0.2, 8, (33,), 2) for d in (6, 11, 16, 20))
CASES = tuple((d, M, s, tag, T, N) for d, M, s, tag, Ts, N in TABLE for T in Ts)
BATCH = (24, 3, 0.2, 8, (17, 256, 33), 2)


def case_id(case):
    d, M, s, tag, T, N = case
    return f'd{d}-M{M}-s{s}-T{T}-N{N}'


def inputs(d, M, s, tag, T):
    w, mu, cov = cc.mixture(3 * d, M, tag, spread=s)
    return w, mu, cov, cc.mcep(T, d, M, tag)


def diff_mixture(mu, cov):
    """the joint mixture over [x, y - x]: what a model prepared with diff = 1 stands for"""
    D = mu.shape[1] // 2
    mu2, cov2 = mu.copy(), cov.copy()
    mu2[:, D:] = mu[:, D:] - mu[:, :D]
    sxx, sxy, syx, syy = cov[:, :D, :D], cov[:, :D, D:], cov[:, D:, :D], cov[:, D:, D:]
    cov2[:, :D, D:] = sxy - sxx
    cov2[:, D:, :D] = np.swapaxes(sxy - sxx, 1, 2)
    cov2[:, D:, D:] = sxx + syy - sxy - syx
    return mu2, cov2


# ---- the numpy restatement ------------------------------------------------------------------------------------------
def terms(mc, w, mu, cov):
    """(logp (T, M), E (M, T, D), v (M, D)) of a mel-cepstrum matrix under a joint mixture"""
    D = 3 * (mc.shape[1] - 1)
    X = cc.delta_features(mc[:, 1:])
    logp = cc.ref_logp(X, w, mu, cov)
    E = np.stack([cc.ref_cond(X, mu, cov, m) for m in range(len(w))])
    v = np.stack([np.diag(cov[m, D:, D:]) - np.diag(cov[m, D:, :D]) / np.diag(cov[m, :D, :D]) * np.diag(cov[m, :D, D:])
                  for m in range(len(w))])
    return logp, E, v


def _logsumexp(l):
    mx = l.max(axis=1)
    return mx + np.log(np.exp(l - mx[:, None]).sum(axis=1))


def em_from_terms(logp, E, v, N):
    """([y_0 .. y_N] (T, d) each, [L_0 .. L_N]) from the log-densities, conditional means and variances"""
    M, T, D = E.shape
    d = D // 3
    eye, up, dn = np.eye(T), np.eye(T, k=1), np.eye(T, k=-1)
    W = np.concatenate([eye, 0.5 * (up - dn), up - 2.0 * eye + dn])        # (3 T, T)
    g = cc.posterior(logp)
    ys, Ls = [], []
    for k in range(N + 1):
        pbar = np.zeros((T, D))
        r = np.zeros((T, D))
        for m in range(M):
            pbar += g[:, m:m + 1] / v[m]
            r += g[:, m:m + 1] * E[m] / v[m]
        P = np.stack([np.concatenate([pbar[:, w_ * d + c] for w_ in range(3)]) for c in range(d)])     # (d, 3 T)
        R = np.stack([np.concatenate([r[:, w_ * d + c] for w_ in range(3)]) for c in range(d)])
        lhs = (W.T[None] * P[:, None, :]) @ W                                                          # (d, T, T)
        y = np.linalg.solve(lhs, (R @ W)[:, :, None])[:, :, 0].T                                       # (T, d)
        Y = cc.delta_features(y)
        l = np.stack([logp[:, m] - 0.5 * (np.log(2 * np.pi * v[m]) + (Y - E[m]) ** 2 / v[m]).sum(axis=1)
                      for m in range(M)], axis=1)
        ys.append(y)
        Ls.append(float(_logsumexp(l).sum()))
        g = cc.posterior(l)
    return ys, Ls


def ref_mcep_em(mc, w, mu, cov, N):
    """([mc_out_0 .. mc_out_N], [L_0 .. L_N]): column 0 kept, columns 1.. the trajectory after k re-estimations"""
    ys, Ls = em_from_terms(*terms(mc, w, mu, cov), N)
    return [np.concatenate([mc[:, :1], y], axis=1) for y in ys], Ls


@functools.lru_cache(maxsize=None)
def case_terms(d, M, s, tag, T):
    w, mu, cov, mc = inputs(d, M, s, tag, T)
    return terms(mc, w, mu, cov)


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """the restatement of a table case, computed once per session and not to be modified"""
    d, M, s, tag, T, N = case
    ys, Ls = em_from_terms(*case_terms(d, M, s, tag, T), N)
    mc = inputs(d, M, s, tag, T)[3]
    outs = [np.concatenate([mc[:, :1], y], axis=1) for y in ys]
    for o in outs:
        o.setflags(write=False)
    return outs, Ls


# ---- the calls (device pointers through the C ABI) ------------------------------------------------------------------
def convert_em(ctx, model, M, mc, N, loglik=True, check=True):
    """kwy_convert_mcep_em_dev: (mc_out, [L_0 .. L_N] or None); with check=False (return code, mc_out, loglik)"""
    import torch
    from kwiiyatta_amd import _lib
    d = mc.shape[1] - 1
    din, = cc._dev(mc)
    out = torch.full(tuple(din.shape), np.nan, dtype=torch.float64, device='cuda')
    lik = torch.full((max(N, 0) + 1,), np.nan, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    rc = _lib.lib.kwy_convert_mcep_em_dev(ctx.handle, din.data_ptr(), din.shape[0], d, M, model.data_ptr(), N,
                                          out.data_ptr(), lik.data_ptr() if loglik else None)
    if check:
        _lib.check(ctx, rc)
    ctx.sync()
    res = out.cpu().numpy(), (lik.cpu().numpy().tolist() if loglik else None)
    return res if check else (rc,) + res


def convert_em_batch(ctx, model, M, mcs, N, loglik=True):
    """kwy_convert_mcep_em_batch_dev: ([mc_out per job], [[L_0 .. L_N] per job])"""
    import torch
    from kwiiyatta_amd import _lib
    d = mcs[0].shape[1] - 1
    ins = cc._dev(*mcs)
    outs = [torch.full(tuple(a.shape), np.nan, dtype=torch.float64, device='cuda') for a in ins]
    liks = [torch.full((N + 1,), np.nan, dtype=torch.float64, device='cuda') for _ in ins]
    torch.cuda.synchronize()
    jobs = _lib.job_array(_lib.ConvertEmJob, [(a, a.shape[0], o, l if loglik else None)
                                              for a, o, l in zip(ins, outs, liks)])
    _lib.check(ctx, _lib.lib.kwy_convert_mcep_em_batch_dev(ctx.handle, ctypes.cast(jobs, ctypes.c_void_p), len(ins), d, M,
                                                           model.data_ptr(), N))
    ctx.sync()
    return [o.cpu().numpy() for o in outs], [l.cpu().numpy().tolist() for l in liks]


def mlpg_em_host(ctx, x, w, mu, cov, N, diff=0):
    """kwy_gmm_mlpg_em with host pointers: (y (T, d), [L_0 .. L_N])"""
    from kwiiyatta_amd import _lib
    x, w, mu, cov = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, w, mu, cov))
    y = np.full(x.shape, np.nan)
    lik = np.full(N + 1, np.nan)
    _lib.check(ctx, _lib.lib.kwy_gmm_mlpg_em(ctx.handle, _lib.ptr(x), x.shape[0], x.shape[1], len(w), _lib.ptr(w),
                                             _lib.ptr(mu), _lib.ptr(cov), diff, N, _lib.ptr(y), _lib.ptr(lik)))
    return y, lik.tolist()
