"""The inputs of the band-aperiodicity conversion's tests and a numpy restatement of its contract (include/kwy.h,
"aperiodicity conversion"): voicing flags, hold fill, row selection, clamp and band error.  What the CPU check
(test_bap_cases.py) and the GPU tests (test_bap_gpu.py) share.  The checker is the CPU oracle (ko.code_aperiodicity,
ko.decode_aperiodicity, ko.gmm_mlpg, ko.delta_features); nothing here imports the product.

Bounds, derived (none is measured):
* coded values against the oracle: codec_cases.CODE_ABS.
* flags, fill, selected rows, decoded rows: the contract asks for bit-equality with the existing kernels' arithmetic,
  so the tests compare bits against the device's own coder, decoder and delta features.
* the band error's per-cell value sqrt(sum_b d^2 / B): the restatement does the same operations in the same order;
  only sqrt may round differently: 2 ulp, ERROR_CELL_REL = 2^-51.  Its mean and M2 are sums of up to a few hundred such
  values in another order: n ulp of the largest partial sum, ERROR_SUM_REL = 1e-12 for n <= 1000.
* end to end: MLPG_REL is the bound of the project's MLPG parity tests (test_backends_gpu.py::test_gmm_mlpg and
  ::test_mlpg_solve_partition_edges: |kwy_gmm_mlpg - ko.gmm_mlpg| <= 1e-10 * max(|ref|, 1)) at this data's scale of
  60 dB: E2E_DB = 6e-9 dB; decoded values then agree within DECODE_REL + ln 10 / 20 * E2E_DB relative (10^(v / 20))."""
import numpy as np

import codec_cases as cc

PASS_FRAMES = 256                            # BAP_PASS (kwy_bap.hip): frames per pass of the track kernel
TABLE_JOBS = 16                              # BAP_GROUP: jobs a by-value table holds
FLOOR, CEILING = -60.0, -1e-12               # what a converted band is clamped to
ERROR_CELL_REL = 2.0 ** -51
ERROR_SUM_REL = 1e-12
MLPG_REL = 1e-10
SCALE_DB = 60.0
E2E_DB = MLPG_REL * SCALE_DB
E2E_DECODED_REL = cc.DECODE_REL + np.log(10.0) / 20.0 * E2E_DB

PAIRS = tuple(p for p in cc.PAIRS if cc.bands(p[0]) >= 1)
FRAMES = (1, 2, PASS_FRAMES, PASS_FRAMES + 1, 2 * PASS_FRAMES + 1)


# ---- voicing patterns ------------------------------------------------------------------------------------------------
def patterns(T):
    """name -> boolean voicing (T,) for every named pattern that exists at T frames"""
    P = PASS_FRAMES
    out = {'all voiced': np.ones(T, dtype=bool), 'none voiced': np.zeros(T, dtype=bool)}
    last = np.zeros(T, dtype=bool)
    last[-1] = True
    out['one voiced frame, last'] = last
    if T >= 2:
        run = max(1, T // 3)
        lead = np.ones(T, dtype=bool)
        lead[:run] = False
        out['leading run'] = lead
        out['trailing run'] = lead[::-1].copy()
        out['alternating'] = np.arange(T) % 2 == 0
    if T >= 2 * P + 1:
        v = np.ones(T, dtype=bool)
        v[P - 1:2 * P] = False                 # frames P - 1 .. 2 P - 1: the whole second pass and the frame before it
        out['unvoiced run over a pass'] = v
    return out


def ap_for(voiced, fs, fft_size, seed=0):
    """(T, K) aperiodicity with the given voicing: voiced rows 10 ** -U(0.5, 3) (coded at most -10 dB: far below the
    -0.5 dB threshold), unvoiced rows what D4C writes for f0 = 0, 1 - 1e-12"""
    rng = np.random.default_rng([fs, fft_size, len(voiced), seed])
    ap = 10.0 ** -rng.uniform(0.5, 3.0, (len(voiced), fft_size // 2 + 1))
    ap[~np.asarray(voiced)] = cc.UNVOICED
    return ap


def threshold_ap(fft_size=1024, n=129):
    """(n, K) constant rows at 16 kHz whose one coded band 20 log10(a) steps through -0.5 dB: a runs over n consecutive
    doubles around 10 ** (-0.5 / 20), 9 ulp of the coded value apart"""
    a = np.float64(10.0 ** (-0.5 / 20.0))
    for _ in range(n // 2):
        a = np.nextafter(a, 0.0)
    rows = np.empty((n, fft_size // 2 + 1))
    for i in range(n):
        rows[i] = a
        a = np.nextafter(a, 1.0)
    return rows


# ---- the contract, restated ------------------------------------------------------------------------------------------
def flags(coded):
    """1.0 where (sum_b c[t, b]) / B <= -0.5, the sum a left fold with b ascending, compared with > -0.5"""
    coded = np.asarray(coded, dtype=np.float64)
    B = coded.shape[1]
    tmp = np.zeros(len(coded))
    for b in range(B):
        tmp = tmp + coded[:, b]
    return np.where(tmp / B > -0.5, 0.0, 1.0)


def fill(coded):
    """the band track (T, B + 1) of coded values (T, B)"""
    coded = np.asarray(coded, dtype=np.float64)
    v = flags(coded)
    S = np.hstack((v[:, None], coded))
    voiced = np.flatnonzero(v == 1.0)
    if len(voiced) == 0:
        return S
    for t in range(len(coded)):
        if v[t] == 1.0:
            continue
        before = voiced[voiced < t]
        src = before[-1] if len(before) else voiced[voiced > t][0]
        S[t, 1:] = coded[src]
    return S


def kept_cells(X, Y, ix, iy):
    """boolean (n,): the cells voiced on both sides"""
    ix, iy = np.asarray(ix, dtype=np.int64), np.asarray(iy, dtype=np.int64)
    return (X[ix, 0] == 1.0) & (Y[iy, 0] == 1.0) if len(ix) else np.zeros(0, dtype=bool)


def joint_rows(X, Y, ix, iy, delta):
    """the training rows of a pair: delta(g) -> (n, 3 B) is the delta-feature routine under which the rows are stated"""
    keep = kept_cells(X, Y, ix, iy)
    B = X.shape[1] - 1
    if not len(keep):
        return np.zeros((0, 6 * B))
    gx = np.ascontiguousarray(X[np.asarray(ix, dtype=np.int64), 1:])
    gy = np.ascontiguousarray(Y[np.asarray(iy, dtype=np.int64), 1:])
    return np.hstack((delta(gx), delta(gy)))[keep]


def clamp(bands_db):
    return np.clip(bands_db, FLOOR, CEILING)


def band_error(A, Bt, ia=None, ib=None):
    """(moments (n, mean, M2), per-cell values with NaN where the cell does not count)"""
    ia = np.arange(len(A)) if ia is None else np.asarray(ia, dtype=np.int64)
    ib = np.arange(len(Bt)) if ib is None else np.asarray(ib, dtype=np.int64)
    nb = A.shape[1] - 1
    cells = np.full(len(ia), np.nan)
    for t in range(len(ia)):
        a, b = A[ia[t]], Bt[ib[t]]
        if a[0] == 1.0 and b[0] == 1.0:
            s = 0.0
            for k in range(nb):
                d = a[1 + k] - b[1 + k]
                s += d * d
            cells[t] = np.sqrt(s / nb)
    vals = cells[~np.isnan(cells)]
    if not len(vals):
        return np.zeros(3), cells
    mean = vals.sum() / len(vals)
    return np.array([len(vals), mean, ((vals - mean) ** 2).sum()]), cells


# ---- synthetic tracks and mixtures -----------------------------------------------------------------------------------
def random_track(T, B, seed, voiced_share=0.6):
    """a band track as `fill` leaves it: smooth bands between -45 and -5 dB, random voicing"""
    rng = np.random.default_rng([T, B, seed])
    walk = np.cumsum(rng.standard_normal((T, B)), axis=0)
    coded = -25.0 + 15.0 * np.tanh(walk / 6.0) + rng.uniform(-3, 3, B)
    coded[rng.random(T) > voiced_share] = 20 * np.log10(cc.UNVOICED)
    return fill(coded)


def random_lists(n, Tx, Ty, seed):
    """two non-decreasing int32 index lists of n cells, as a warping path's are"""
    rng = np.random.default_rng([n, Tx, Ty, seed])
    return (np.sort(rng.integers(0, Tx, n)).astype(np.int32), np.sort(rng.integers(0, Ty, n)).astype(np.int32))


class BandGMM:
    """a well-conditioned joint mixture over 6 B dimensions on the dB scale: static means tens of dB apart between the
    components (the arg-max sequence is decided by a wide margin), target statics about 8 dB below the source's"""
    covariance_type = 'full'

    def __init__(self, B, M=2, seed=0):
        rng = np.random.default_rng([B, M, seed])
        D = 3 * B
        self.weights_ = np.full(M, 1.0 / M)
        self.means_ = np.zeros((M, 2 * D))
        for m in range(M):
            src = -12.0 - 22.0 * m + rng.uniform(-1, 1, B)
            self.means_[m, :B] = src
            self.means_[m, D:D + B] = src - 8.0 + rng.uniform(-1, 1, B)
        a = rng.standard_normal((M, 2 * D, 2 * D)) * 0.5
        self.covariances_ = a @ a.transpose(0, 2, 1) + np.eye(2 * D) * rng.uniform(4.0, 9.0, (M, 1, 1))
        self.n_components = M
