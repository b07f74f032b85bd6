"""Inputs, numpy restatement and C ABI calls of the GV-considering trajectory generation (kwy_gv_ascent,
kwy_gmm_mlpg_gv, kwy_convert_mcep_gv_dev, kwy_convert_mcep_gv_batch_dev; the arithmetic is written out in
include/kwy.h).  A plain module shared by tests/test_gvgen_cases.py (CPU), tests/test_gvgen_gpu.py and
tests/test_gvgen_drivers_gpu.py.

The restatement works on the dense P of a column's records, takes y_ML from np.linalg.solve where it makes its own
inputs, and the line search's step from np.roots.
"""
import ctypes
import functools

import numpy as np

import convert_cases as cc
import em_cases as ec

KWY_MLPG_GV_MAX = 256
KWY_BATCH_MAX = 16
# constants of k_gv_ascent (kwy_gvgen.hip)
NT = 256                 # GVA_NT: threads of a workgroup; thread i owns the rows i, i + NT, ...
REG_ROWS = 8 * NT        # GVA_NT * GVA_REG_ROWS: beyond this many rows the records are streamed in every pass
LDS_ROWS = 6800          # GVA_LDS_ROWS: beyond this many rows the tracks live in global memory
SEED = 31

ALL_N = (0, 1, 2, 8)
# (d, T, offset, target above the track's own variance, the iteration counts).  Every y_k of a case comes from one run
# of the restatement; the device is called once per count.
# The conditioning gate of tests/test_gvgen_cases.py cut two counts: a track of 2 or 3 frames is at its optimum after
# as many steps, and further steps there divide rounding noise by rounding noise (a relative 1e-13 of the inputs moved
# y_4 by up to 2.7e-9 of its peak), so these stop at N = 2; and the long case, meant for N = 64, moved by 8.3e-10 at
# y_64 (6.7e-11 at y_60, 2.1e-11 at y_48) and runs N = 48.
_SMALL_T = (1, 2, 3, 4, 5, NT - 1, NT, NT + 1, 2 * NT + 1)


def _counts(T):
    return (0, 1, 2) if T in (2, 3) else ALL_N


LONG_N = 48
CASES = tuple((2, T, bool(i % 2), bool(i % 2), _counts(T)) for i, T in enumerate(_SMALL_T)) + \
    tuple((2, T, not bool(i % 2), bool(i % 2), _counts(T)) for i, T in enumerate(_SMALL_T)) + \
    tuple((d, T, off, up, ALL_N) for d in (1, 24, 27) for T, off, up in ((33, True, True), (257, False, False))) + \
    tuple((2, REG_ROWS + k, k != 0, k != 1, ALL_N) for k in (-1, 0, 1)) + \
    tuple((1, LDS_ROWS + k, k != 0, k != 1, (2,)) for k in (-1, 0, 1)) + \
    ((24, 2001, True, True, (LONG_N,)),)
BATCH = (24, (17, 256, 33), True, True, 2)


def case_id(case):
    d, T, off, up, Ns = case
    return f'd{d}-T{T}-{"offset" if off else "plain"}-{"above" if up else "below"}-N{max(Ns)}'


# ---- inputs -----------------------------------------------------------------------------------------------------------
_COEF = ({0: 1.0}, {-1: -0.5, 1: 0.5}, {-1: 1.0, 0: -2.0, 1: 1.0})     # window w: the coefficient at offset k


def band_records(pbar, r):
    """(T, d, 4) records {P[t][t], P[t][t-1], P[t][t-2], b[t]} of W' diag(pbar) W and W' r; pbar, r: (T, 3 d) in the
    layout of the delta features (static | delta | delta-delta)"""
    T, d = pbar.shape[0], pbar.shape[1] // 3
    rec = np.zeros((T, d, 4))
    for w, coef in enumerate(_COEF):
        p, q = pbar[:, w * d:(w + 1) * d], r[:, w * d:(w + 1) * d]
        for k1, c1 in coef.items():                      # row a = t + k1
            a = np.arange(T) + k1
            ok = (a >= 0) & (a < T)
            rec[a[ok], :, 3] += c1 * q[ok]
            for k2, c2 in coef.items():                  # column a - o = t + k2
                o = k1 - k2
                ok2 = ok & (np.arange(T) + k2 >= 0) & (np.arange(T) + k2 < T)
                if 0 <= o <= 2:
                    rec[a[ok2], :, o] += c1 * c2 * p[ok2]
    return rec


def dense(rec):
    """(P (T, T), b (T)) of one column's records (T, 4)"""
    T = len(rec)
    P = np.diag(rec[:, 0])
    for o in (1, 2):
        if T > o:
            P += np.diag(rec[o:, o], -o) + np.diag(rec[o:, o], o)
    return P, rec[:, 3].copy()


@functools.lru_cache(maxsize=None)
def inputs(d, T, off, up):
    """(records (T, d, 4), y_ML (T, d), offset (T, d) or None, gv_mean (d), gv_var (d)) of a case: random precisions,
    target means that wander, the target GV 2.5 x or 0.5 x the variance of y_ML + offset, its deviation 0.3 x itself"""
    rng = np.random.default_rng([SEED, d, T, int(off), int(up)])
    pbar = np.exp(rng.standard_normal((T, 3 * d)))
    t = np.arange(T)[:, None]
    E = np.concatenate([np.sin(0.05 * t * (1.0 + np.arange(d)) + rng.uniform(0, 6, d)) + 0.3 * rng.standard_normal((T, d)),
                        0.1 * rng.standard_normal((T, 2 * d))], axis=1)
    rec = band_records(pbar, pbar * E)
    y = np.empty((T, d))
    for c in range(d):
        if T <= REG_ROWS + 1:
            y[:, c] = np.linalg.solve(*dense(rec[:, c]))
        else:      # y_ML is an input of the ascent: at the longest tracks a banded solver makes it in a fraction of the time
            from scipy.linalg import solveh_banded
            ab = np.zeros((3, T))
            for o in range(3):
                ab[o, :T - o] = rec[o:, c, o]
            y[:, c] = solveh_banded(ab, rec[:, c, 3], lower=True)
    s = 0.5 * np.cos(0.03 * t * (1.0 + np.arange(d))) + 0.1 * rng.standard_normal((T, d)) if off else None
    z = y if s is None else y + s
    v = z.var(axis=0)
    mean = np.where(v > 0, (2.5 if up else 0.5) * v, 1.0)
    var = (0.3 * mean) ** 2
    for a in (rec, y, mean, var) + (() if s is None else (s,)):
        a.setflags(write=False)
    return rec, y, s, mean, var


# ---- the numpy restatement --------------------------------------------------------------------------------------------
def _parts(P, b, y, s, mu, var, weight):
    """(Q, the sum of the magnitudes of its three terms, v, z - zbar)"""
    T = len(y)
    om = 1.0 / (3.0 * T)
    z = y + s
    zc = z - z.sum() / T
    v = (zc * zc).sum() / T
    t1, t2, t3 = om * 0.5 * (y @ (P @ y)), om * (b @ y), 0.5 * weight * (v - mu) ** 2 / var
    return -t1 + t2 - t3, abs(t1) + abs(t2) + abs(t3), v, zc


def ascent_column(rec, y_ml, s, mu, var, weight, N):
    """one column: (ys (N + 1, T), Qs (N + 1), magnitudes (N + 1), unusable).  A column that is not processed (unusable,
    or a constant track) has y_ML in every row of ys and zeros in Qs"""
    T = len(y_ml)
    s = np.zeros(T) if s is None else s
    same = (np.tile(y_ml, (N + 1, 1)), np.zeros(N + 1), np.zeros(N + 1))
    if not (np.isfinite(mu) and mu > 0 and np.isfinite(var) and var > 0):
        return same + (True,)
    P, b = dense(rec)
    om = 1.0 / (3.0 * T)
    Q, mag, v, zc = _parts(P, b, y_ml, s, mu, var, weight)
    if not np.isfinite(v):
        return same + (True,)
    if v == 0:
        return same + (False,)
    y = y_ml.copy()
    z = y + s
    y0 = np.sqrt(mu / v) * zc + z.sum() / T - s
    Q0, mag0, v0, zc0 = _parts(P, b, y0, s, mu, var, weight)
    if Q0 >= Q:
        y, Q, mag, v, zc = y0, Q0, mag0, v0, zc0
    ys, Qs, mags = [y.copy()], [Q], [mag]
    frozen, p, g_prev = False, None, None
    for k in range(1, N + 1):
        if not frozen:
            resid = b - P @ y
            g = om * resid - weight * (v - mu) / var * (2.0 / T) * zc
            if k == 1:
                p = g
            else:
                p = g + max(0.0, g @ (g - g_prev) / (g_prev @ g_prev)) * p
                if g @ p <= 0:
                    p = g
            alpha = None
            if g @ p > 0:
                pc = p - p.sum() / T
                A, B, cov, vp = p @ (P @ p), p @ resid, (zc @ pc) / T, (pc @ pc) / T
                kap, e = weight / var, v - mu
                roots = np.roots([-2.0 * kap * vp * vp, -6.0 * kap * cov * vp,
                                  -om * A - kap * (4.0 * cov * cov + 2.0 * e * vp), om * B - 2.0 * kap * e * cov])
                roots = roots[np.isreal(roots)].real
                if (roots > 0).any():
                    alpha = roots[roots > 0].min()
            if alpha is None:
                frozen = True
            else:
                y1 = y + alpha * p
                Q1, mag1, v1, zc1 = _parts(P, b, y1, s, mu, var, weight)
                if Q1 >= Q:
                    y, Q, mag, v, zc, g_prev = y1, Q1, mag1, v1, zc1, g
                else:
                    frozen = True
        ys.append(y.copy())
        Qs.append(Q)
        mags.append(mag)
    return np.array(ys), np.array(Qs), np.array(mags), False


def ascent(rec, y_ml, s, mean, var, N, weight=1.0):
    """an utterance: (ys (N + 1, T, d), Qs (N + 1), magnitudes (N + 1), status): Q_k and the magnitudes summed over the
    columns in ascending order"""
    T, d = y_ml.shape
    ys, Qs, mags, status = np.empty((N + 1, T, d)), np.zeros(N + 1), np.zeros(N + 1), 0
    for c in range(d):
        yc, qc, mc, bad = ascent_column(rec[:, c], y_ml[:, c], None if s is None else s[:, c], mean[c], var[c], weight, N)
        ys[:, :, c] = yc
        Qs += qc
        mags += mc
        status += int(bad)
    return ys, Qs, mags, status


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """the restatement of a table case up to its largest N, computed once per session and not to be modified"""
    d, T, off, up, Ns = case
    rec, y, s, mean, var = inputs(d, T, off, up)
    ys, Qs, mags, status = ascent(rec, y, s, mean, var, max(Ns))
    for a in (ys, Qs, mags):
        a.setflags(write=False)
    return ys, Qs, mags, status


def gate_figures(rec, y, s, mean, var, N, ref, perturbation=1e-13, seeds=3):
    """the conditioning gate: (the largest move of any y_k over its peak, of any Q_k over its term magnitudes) when the
    records and y_ML are perturbed by a relative `perturbation`; ref: `ascent`'s result on the unperturbed inputs"""
    ys, Qs, mags, _ = ref
    worst_y = worst_q = 0.0
    for seed in range(seeds):
        rng = np.random.default_rng([SEED, seed, len(y)])
        rec2, y2 = (a * (1.0 + perturbation * rng.uniform(-1.0, 1.0, a.shape)) for a in (rec, y))
        ys2, Qs2, _, _ = ascent(rec2, y2, s, mean, var, N)
        for k in range(N + 1):
            worst_y = max(worst_y, np.abs(ys2[k] - ys[k]).max() / np.abs(ys[k]).max())
            if mags[k] > 0:
                worst_q = max(worst_q, abs(Qs2[k] - Qs[k]) / mags[k])
    return worst_y, worst_q


# the ascent chained behind the numpy conversions of em_cases / convert_cases: (d, M, spread, tag, T) of the mixture and
# the mel-cepstra, diff, em_iterations; CHAINED_N steps towards 2 x the converted track's own variance
CHAINED_SIZES = ((2, 3, 1.0, 7, 33), (24, 64, 0.2, 8, 257))
CHAINED = tuple(size + (diff, em) for size in CHAINED_SIZES for diff in (0, 1) for em in (-1, 0, 2))
CHAINED_N = 4


def chained_id(case):
    d, M, s, tag, T, diff, em = case
    return f'd{d}-M{M}-T{T}-diff{diff}-em{em}'


@functools.lru_cache(maxsize=None)
def chained_reference(case):
    """(w, mu, cov, mc, offset or None, gv_mean, gv_var, records, y_ML, the restatement's result) of a chained case; for
    diff = 1 the numpy conversion runs on the mixture over [x, y - x] and the offset is the source's statics"""
    d, M, spread, tag, T, diff, em = case
    w, mu, cov, mc = ec.inputs(d, M, spread, tag, T)
    mu2, cov2 = ec.diff_mixture(mu, cov) if diff else (mu, cov)
    rec, y = conversion_bands(mc, w, mu2, cov2, em)
    s = np.ascontiguousarray(mc[:, 1:]) if diff else None
    mean = 2.0 * (y if s is None else y + s).var(axis=0)
    var = (0.3 * mean) ** 2
    return w, mu, cov, mc, s, mean, var, rec, y, ascent(rec, y, s, mean, var, CHAINED_N)


# the conversion in front of the ascent: the posteriors are fixed first (one arg-max mixture per frame for em = -1, the
# EM posteriors after their em re-estimations otherwise), then the records of the last solve and its y
def conversion_bands(mc, w, mu, cov, em):
    """(records (T, d, 4), y_ML (T, d)) of kwy_convert_mcep_dev (em = -1) / kwy_convert_mcep_em_dev (em >= 0)"""
    logp, E, v = ec.terms(mc, w, mu, cov)
    M, T, D = E.shape
    if em < 0:
        g = np.zeros((T, M))
        g[np.arange(T), logp.argmax(axis=1)] = 1.0
    else:
        g = cc.posterior(logp)
    for k in range(max(em, 0) + 1):
        pbar, r = np.zeros((T, D)), np.zeros((T, D))
        for m in range(M):
            pbar += g[:, m:m + 1] / v[m]
            r += g[:, m:m + 1] * E[m] / v[m]
        rec = band_records(pbar, r)
        y = np.stack([np.linalg.solve(*dense(rec[:, c])) for c in range(D // 3)], axis=1)
        Y = cc.delta_features(y)
        g = cc.posterior(np.stack([logp[:, m] - 0.5 * (np.log(2 * np.pi * v[m]) + (Y - E[m]) ** 2 / v[m]).sum(axis=1)
                                   for m in range(M)], axis=1))
    return rec, y


# ---- the calls --------------------------------------------------------------------------------------------------------
def ascent_dev(ctx, jobs, mean, var, N, weight=1.0, objective=True, check=True):
    """kwy_gv_ascent_batch_dev on jobs of (records, offset or None, y_ML): ([y_N per job], [[Q_0 .. Q_N] per job],
    [status per job]); with check=False the return code in front"""
    import torch
    from kwiiyatta_amd import _lib
    d = jobs[0][2].shape[1]
    recs = cc._dev(*[np.array(j[0]) for j in jobs])          # (copies: the cached inputs are read-only)
    offs = [None if j[1] is None else cc._dev(np.array(j[1]))[0] for j in jobs]
    ys = cc._dev(*[np.array(j[2]) for j in jobs])
    objs = [torch.full((max(N, 0) + 1,), np.nan, dtype=torch.float64, device='cuda') for _ in jobs]
    dm, dv = cc._dev(np.array(mean, dtype=np.float64), np.array(var, dtype=np.float64))
    status = torch.full((len(jobs),), -1, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    arr = _lib.job_array(_lib.GvAscentJob, [(r, o, y, y.shape[0], q if objective else None)
                                            for r, o, y, q in zip(recs, offs, ys, objs)])
    rc = _lib.lib.kwy_gv_ascent_batch_dev(ctx.handle, ctypes.cast(arr, ctypes.c_void_p), len(jobs), d, dm.data_ptr(),
                                          dv.data_ptr(), weight, N, status.data_ptr())
    if check:
        _lib.check(ctx, rc)
    ctx.sync()
    res = [y.cpu().numpy() for y in ys], [q.cpu().numpy() for q in objs], status.cpu().numpy().tolist()
    return res if check else (rc,) + res


def ascent_host(ctx, rec, s, y_ml, mean, var, N, weight=1.0):
    """kwy_gv_ascent with host pointers, one job: (y_N, [Q_0 .. Q_N], status)"""
    from kwiiyatta_amd import _lib
    rec, y = np.ascontiguousarray(rec), np.array(y_ml)
    s = None if s is None else np.ascontiguousarray(s)
    mean, var = (np.ascontiguousarray(a, dtype=np.float64) for a in (mean, var))
    obj = np.full(N + 1, np.nan)
    status = np.full(1, -1, dtype=np.int32)
    arr = _lib.job_array(_lib.GvAscentJob, [(rec.ctypes.data, None if s is None else s.ctypes.data, y.ctypes.data,
                                             len(y), obj.ctypes.data)])
    _lib.check(ctx, _lib.lib.kwy_gv_ascent(ctx.handle, ctypes.cast(arr, ctypes.c_void_p), 1, y.shape[1], _lib.ptr(mean),
                                           _lib.ptr(var), weight, N, _lib.ptr(status)))
    return y, obj, int(status[0])


def convert_gv(ctx, model, M, mcs, em, offset, mean, var, N, weight=1.0, check=True):
    """kwy_convert_mcep_gv_dev for one matrix, kwy_convert_mcep_gv_batch_dev for a list: (mc_out, loglik, objective,
    status) per matrix; with check=False the return code in front (one matrix only)"""
    import torch
    from kwiiyatta_amd import _lib
    single = not isinstance(mcs, (list, tuple))
    ins = cc._dev(*[np.array(m) for m in ([mcs] if single else mcs)])
    d = ins[0].shape[1] - 1
    outs = [torch.full(tuple(a.shape), np.nan, dtype=torch.float64, device='cuda') for a in ins]
    liks = [torch.full((max(em, 0) + 1,), np.nan, dtype=torch.float64, device='cuda') for _ in ins]
    objs = [torch.full((max(N, 0) + 1,), np.nan, dtype=torch.float64, device='cuda') for _ in ins]
    status = torch.full((len(ins),), -1, dtype=torch.int32, device='cuda')
    dm, dv = cc._dev(np.array(mean, dtype=np.float64), np.array(var, dtype=np.float64))
    torch.cuda.synchronize()
    if single:
        rc = _lib.lib.kwy_convert_mcep_gv_dev(ctx.handle, ins[0].data_ptr(), ins[0].shape[0], d, M, model.data_ptr(), em,
                                              int(offset), dm.data_ptr(), dv.data_ptr(), weight, N, outs[0].data_ptr(),
                                              liks[0].data_ptr(), objs[0].data_ptr(), status.data_ptr())
    else:
        arr = _lib.job_array(_lib.ConvertGvJob, [(a, a.shape[0], o, l, q) for a, o, l, q in zip(ins, outs, liks, objs)])
        rc = _lib.lib.kwy_convert_mcep_gv_batch_dev(ctx.handle, ctypes.cast(arr, ctypes.c_void_p), len(ins), d, M,
                                                    model.data_ptr(), em, int(offset), dm.data_ptr(), dv.data_ptr(),
                                                    weight, N, status.data_ptr())
    if check:
        _lib.check(ctx, rc)
    ctx.sync()
    res = [(o.cpu().numpy(), l.cpu().numpy(), q.cpu().numpy(), int(s))
           for o, l, q, s in zip(outs, liks, objs, status.cpu().numpy())]
    if single:
        return res[0] if check else (rc,) + res[0]
    return res


def mlpg_gv_host(ctx, x, w, mu, cov, diff, em, offset, mean, var, N, weight=1.0):
    """kwy_gmm_mlpg_gv with host pointers: (y (T, d), loglik, objective, status)"""
    from kwiiyatta_amd import _lib
    x, w, mu, cov, mean, var = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, w, mu, cov, mean, var))
    y = np.full(x.shape, np.nan)
    lik, obj = np.full(max(em, 0) + 1, np.nan), np.full(N + 1, np.nan)
    status = np.full(1, -1, dtype=np.int32)
    _lib.check(ctx, _lib.lib.kwy_gmm_mlpg_gv(ctx.handle, _lib.ptr(x), x.shape[0], x.shape[1], len(w), _lib.ptr(w),
                                             _lib.ptr(mu), _lib.ptr(cov), diff, em, int(offset), _lib.ptr(mean),
                                             _lib.ptr(var), weight, N, _lib.ptr(y), _lib.ptr(lik), _lib.ptr(obj),
                                             _lib.ptr(status)))
    return y, lik, obj, int(status[0])
