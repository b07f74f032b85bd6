"""The numpy model of the exemplar (NMF) converter's arithmetic (include/kwy.h, "exemplar-based conversion"), its
input generators, and the tolerance rule of the kernel tests.

The model takes a dtype: the same code runs in float64 and in np.longdouble, and the deviation between the two (and
between two summation orders of the float64 model) is what the kernel's tolerance is computed from."""
import numpy as np

DBL_MIN = np.finfo(np.float64).tiny


def nmf_updates(S, X, iterations, sparsity, h0=None, dtype=np.float64):
    """H after `iterations` multiplicative updates from ones (or h0)"""
    S, X = np.asarray(S, dtype=dtype), np.asarray(X, dtype=dtype)
    H = np.ones((len(X), len(S)), dtype=dtype) if h0 is None else np.array(h0, dtype=dtype)
    tiny, scale = dtype(DBL_MIN), dtype(1) + dtype(sparsity)
    for _ in range(iterations):
        R = H @ S
        Q = X / np.maximum(R, tiny)
        G = Q @ S.T
        H = H * G / scale
    return H


def nmf_objective(S, X, H, sparsity, dtype=np.float64):
    """per frame: KL(X || H S) + sparsity * sum H (the generalised divergence: sum x log(x / r) - x + r)"""
    S, X, H = (np.asarray(a, dtype=dtype) for a in (S, X, H))
    R = np.maximum(H @ S, dtype(DBL_MIN))
    return (X * np.log(X / R) - X + (H @ S)).sum(axis=1) + dtype(sparsity) * H.sum(axis=1)


def nmf_convert(S, Tg, X, iterations, sparsity, h0=None, dtype=np.float64):
    """(Y, H, objective) of the contract"""
    H = nmf_updates(S, X, iterations, sparsity, h0, dtype)
    return H @ np.asarray(Tg, dtype=dtype), H, nmf_objective(S, X, H, sparsity, dtype)


def unit_sum(rows):
    return rows / rows.sum(axis=1, keepdims=True)


def select_rows(R, A):
    """the rows an exemplar dictionary of at most A atoms keeps of R training rows"""
    if R <= A:
        return np.arange(R)
    return np.array([i * R // A for i in range(A)])


def smooth_spectra(rng, n, B):
    """n smooth positive spectra on B bins: sums of three Gaussians plus 1e-4, scaled to unit sum"""
    b = np.arange(B)[None, :]
    out = np.full((n, B), 1e-4)
    for _ in range(3):
        centre = rng.uniform(0, B, size=(n, 1))
        width = rng.uniform(B / 40 + 0.5, B / 6 + 1.0, size=(n, 1))
        out += rng.uniform(0.2, 1.0, size=(n, 1)) * np.exp(-0.5 * ((b - centre) / width) ** 2)
    return unit_sum(out)


def make_case(B, A, T, seed=0):
    """(S, Tg, X): smooth dictionaries and frames; every other frame is an exact sparse mixture of source atoms
    (at most three of them, convex weights, so its sum stays 1)"""
    rng = np.random.default_rng(seed + 1000 * B + 10 * A + T)
    S, Tg, X = smooth_spectra(rng, A, B), smooth_spectra(rng, A, B), smooth_spectra(rng, T, B)
    for t in range(0, T, 2):
        atoms = rng.choice(A, size=min(3, A), replace=False)
        w = rng.uniform(0.1, 1.0, size=len(atoms))
        X[t] = (w / w.sum()) @ S[atoms]
    return np.ascontiguousarray(S), np.ascontiguousarray(Tg), np.ascontiguousarray(unit_sum(X))


def frame_rel(a, ref):
    """per frame: max |a - ref| over the frame's entries / max |ref| of that frame"""
    a, ref = np.asarray(a, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    return np.float64((np.abs(a - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())


def vector_rel(a, ref):
    """max |a - ref| / max |ref|: for the objective, one number per frame.  A frame's objective is a difference of
    sums of size 1 (the frames have unit sum), so its error is absolute on that scale, not relative to its own value,
    which an exact mixture drives towards 0; the scale of the call is its largest objective."""
    a, ref = np.asarray(a, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    return np.float64(np.abs(a - ref).max() / np.abs(ref).max())


def reference(S, Tg, X, iterations, sparsity, h0=None):
    """the float64 model and the deviations d_Y, d_H, d_objective of the references among themselves: the larger of
    float64 against long double, and float64 against float64 with the atoms permuted (another summation order)"""
    A = len(S)
    Y, H, obj = nmf_convert(S, Tg, X, iterations, sparsity, h0)
    Yl, Hl, objl = nmf_convert(S, Tg, X, iterations, sparsity, h0, dtype=np.longdouble)
    perm = np.random.default_rng(A).permutation(A)
    Yp, Hp, objp = nmf_convert(S[perm], Tg[perm], X, iterations, sparsity, None if h0 is None else h0[:, perm])
    Hp_back = np.empty_like(Hp)
    Hp_back[:, perm] = Hp
    d = {'Y': max(frame_rel(Y, Yl), frame_rel(Yp, Y)),
         'H': max(frame_rel(H, Hl), frame_rel(Hp_back, H)),
         'objective': max(vector_rel(obj, objl), vector_rel(objp, obj))}
    return {'Y': Y, 'H': H, 'objective': obj, 'd': d}


def bound(d, A):
    """what the kernel may deviate from the float64 model: 64 d -- the factor covers the matrix cores' different
    association and the build without contraction -- and never less than A 2^-52"""
    return max(64.0 * d, A * 2.0 ** -52)
