"""KL-NMF activations over coupled exemplar dictionaries on the device (include/kwy.h, "exemplar-based conversion")

    H starts at ones (or h0); `iterations` times:  R = H S,  Q = X / max(R, DBL_MIN),  G = Q S^T,
                                                   H <- (H * G) / (1 + sparsity)
    Y = H Tg;   objective[t] = KL(X[t] || R[t]) + sparsity * sum(H[t]), R of the final H

the hot path of `ExemplarFeatureConverter`.  S, Tg (atoms x bins) and X (frames x bins) are strictly positive with
unit row sums (`unit_sum` is the preparation).  Frames never interact, the result after n updates does not depend on
how many were asked for, and a call is bit-reproducible; the products run on the f64 matrix cores.
An entry that is not finite and positive is counted in the status word: `check_status` raises for it.
Inputs follow the other shims' contract: float64, C-contiguous (the same ValueError otherwise)."""
import numpy as np

from .. import _lib
from .._lib import lib, ptr

MAX_ATOMS = 8192
MAX_BINS = 2049
MAX_ITERATIONS = 1000


def unit_sum(rows):
    """every row scaled to unit sum over its bins (a new array): the preparation of atoms and frames"""
    rows = _lib.as_f64(rows)
    return np.ascontiguousarray(rows / rows.sum(axis=1, keepdims=True))


def _matrix(a, what, cols=None):
    a = _lib.as_f64(a)
    if a.ndim != 2 or (cols is not None and a.shape[1] != cols):
        raise ValueError(f'{what}: a (rows, {"columns" if cols is None else cols}) matrix is expected, not shape {a.shape}')
    return a


def _check_sizes(A, B, iterations, sparsity):
    if not 1 <= A <= MAX_ATOMS:
        raise ValueError(f'nmf: 1 .. {MAX_ATOMS} atoms are expected, not {A}')
    if not 2 <= B <= MAX_BINS:
        raise ValueError(f'nmf: 2 .. {MAX_BINS} bins are expected, not {B}')
    if int(iterations) != iterations or not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f'nmf: 0 .. {MAX_ITERATIONS} iterations are expected, not {iterations}')
    if not (sparsity >= 0 and np.isfinite(sparsity)):
        raise ValueError(f'nmf: the sparsity must be finite and >= 0, not {sparsity}')


def scratch_bytes(A, B, T):
    """bytes of device scratch `convert_dev` needs for T frames against A atoms of B bins (0 for T = 0)"""
    return int(lib.kwy_nmf_scratch_bytes(int(A), int(B), int(T)))


def _run(S, Tg, X, iterations, sparsity, h0, want_y, want_h, want_objective, strict, ctx):
    S, X = _matrix(S, 'S'), _matrix(X, 'X')
    A, B = S.shape
    _check_sizes(A, B, iterations, sparsity)
    X = _matrix(X, 'X', B)
    T = len(X)
    if Tg is not None:
        Tg = _matrix(Tg, 'Tg', B)
        if Tg.shape != S.shape:
            raise ValueError(f'S and Tg differ in shape: {S.shape} and {Tg.shape}')
    if h0 is not None:
        h0 = _matrix(h0, 'h0', A)
        if len(h0) != T:
            raise ValueError(f'h0: {T} rows are expected, not {len(h0)}')
    Y = np.empty((T, B)) if want_y else None
    H = np.empty((T, A)) if want_h else None
    objective = np.empty(T) if want_objective else None
    status = np.zeros(1, dtype=np.int32)
    if T:
        ctx = ctx or _lib.default_context()
        opt = lambda a: None if a is None else ptr(a)
        _lib.check(ctx, lib.kwy_nmf_convert(ctx.handle, ptr(S), opt(Tg), ptr(X), A, B, T, int(iterations), float(sparsity),
                                            opt(h0), opt(Y), opt(H), opt(objective), ptr(status)))
        if strict:
            check_status(status)
    return Y, H, objective


def activations(S, X, iterations, sparsity, h0=None, strict=True, ctx=None):
    """H (frames x atoms) after `iterations` updates from ones, or from h0"""
    return _run(S, None, X, iterations, sparsity, h0, False, True, False, strict, ctx)[1]


def convert(S, Tg, X, iterations, sparsity, return_h=False, return_objective=False, h0=None, strict=True, ctx=None):
    """Y = H Tg (frames x bins); with return_h / return_objective a tuple (Y[, H][, objective])"""
    if Tg is None:
        raise ValueError('convert: the target atoms are needed')
    Y, H, objective = _run(S, Tg, X, iterations, sparsity, h0, True, return_h, return_objective, strict, ctx)
    if not (return_h or return_objective):
        return Y
    return (Y,) + ((H,) if return_h else ()) + ((objective,) if return_objective else ())


def convert_dev(ctx, S, Tg, X, iterations, sparsity, scratch, Y=None, H=None, objective=None, status=None, h0=None):
    """S, Tg (A, B), X (T, B), h0 (T, A): contiguous float64 device tensors (Tg, h0 may be None); Y (T, B), H (T, A),
    objective (T) float64 and status (one int32 word): written where given.  scratch: a device tensor of at least
    scratch_bytes(A, B, T) bytes.  Enqueued on the context's stream, not synchronised, nothing allocated."""
    if S.dim() != 2 or X.dim() != 2 or S.shape[1] != X.shape[1] or not S.is_contiguous() or not X.is_contiguous():
        raise ValueError('convert_dev: contiguous (atoms, bins) and (frames, bins) matrices of one bin count are expected')
    A, B, T = S.shape[0], S.shape[1], X.shape[0]
    _check_sizes(A, B, iterations, sparsity)
    for t, shape, what in ((Tg, (A, B), 'Tg'), (h0, (T, A), 'h0'), (Y, (T, B), 'Y'), (H, (T, A), 'H'), (objective, (T,), 'objective')):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f'convert_dev: {what} must be contiguous of shape {shape}')
    if (Tg is None) != (Y is None):
        raise ValueError('convert_dev: Tg and Y go together')
    size = scratch.numel() * scratch.element_size()
    if T and size < scratch_bytes(A, B, T):
        raise ValueError(f'convert_dev: the scratch holds {size} bytes, {scratch_bytes(A, B, T)} are needed')
    dp = lambda t: None if t is None else t.data_ptr()
    _lib.check(ctx, lib.kwy_nmf_convert_dev(ctx.handle, S.data_ptr(), dp(Tg), X.data_ptr(), A, B, T, int(iterations),
                                            float(sparsity), dp(h0), dp(Y), dp(H), dp(objective), dp(status),
                                            scratch.data_ptr(), size))


def check_status(status, what='nmf'):
    """raise for a non-zero status word (host array / device tensor, read back here)"""
    n = int(sum(int(s) for s in (status.tolist() if hasattr(status, 'tolist') else status)))
    if n:
        raise ValueError(f'{what}: {n} entr{"y is" if n == 1 else "ies are"} not finite and positive '
                         f'(atoms and frames must be > 0, starting activations >= 0)')
