"""Inputs, references and assertions for the stand-alone mel-cepstrum entries kwy_sp2mc[_dev] and kwy_mc2sp[_dev]
(kwiiyatta_amd/csrc/kwy_mcep.hip): tests/test_mcep_edges_gpu.py runs them on the device, tests/test_mcep_cases.py
proves the cases and the references on the CPU.

References.  sp2mc_ref and mc2sp_ref restate pysptk's two conversions in np.longdouble: the transform as a direct
cosine sum (index reduced mod N before the cosine is taken), SPTK's freqt recursion vectorised over the frames,
c[0] /= 2 before the warp, c[0] *= 2 and the mirror after it.  sp2mc_ref warps all N points of the cepstrum, the
mirrored half included, as pysptk does.  The GPU tests compare with the float64 oracle (oracle.sp2mc, oracle.mc2sp),
which test_mcep_cases.py holds within ORACLE_MC_REL / ORACLE_SP_LOG of the long-double reference on every case.

Bounds.  The caps are the project's own (tests/test_backends_gpu.py): 1e-12 of max |ref| per call for sp2mc, 1e-11 on
|log got - log ref| of every bin for mc2sp.  MC_REL and SP_LOG are 8 x the largest error of each kernel against the
long-double reference (not against the oracle, and not against the kernels' own earlier output), measured on an
MI355X over every case of the tables below; the margin covers inputs other than the ones measured.

    kernel          worst case                  error against the long-double reference   8 x
    --------------  --------------------------  ----------------------------------------  ---------
    k_sp2mc<LOG2N>  K 257 order 63 alpha 0.95   1.376e-15 of max |ref|                    1.101e-14  = MC_REL
    k_sp2mc_dense   K 4096 order 24 alpha 0.41  1.272e-15 of max |ref|                    1.018e-14  (<= MC_REL)
      (its three fallback cases: 9.7e-16, 6.1e-16, 1.2e-15)
    k_mc2sp_mfma    K 65 order 63 alpha 0.41    1.483e-14 in log / max(1, max |log| / 15)  1.186e-13  = SP_LOG
      (unscaled 1.536e-14; the range rows: 4.786e-13 in log at |log| = 700, 1.024e-14 after scaling)

Both are two orders below the caps, as a float64 emulation of the kernels' sums predicts (1.7e-15 for sp2mc).  The
oracle itself lies 3e-16 (sp2mc) and 8e-15 in log (mc2sp) from the long-double reference on these cases.

For mc2sp rows built to reach |log sp| of about 700 the bound scales with the magnitude of the sum,
SP_LOG * max(1, max |log ref| / SP_LOG_SCALE): a sum's rounding error grows with its terms, and 15 is the magnitude of
the ordinary cases.
"""
import functools
from collections import namedtuple

import numpy as np

LD = np.longdouble

# ---- constants of kwy_mcep.hip, for the seam arithmetic of test_mcep_cases.py -------------------------------------
MC_MAX_ORDER = 63            # kwy_mcep.hip:31   #define MC_MAX_ORDER 63
MC_FR = 4                    # kwy_mcep.hip:60   #define MC_FR 4            frames per workgroup of k_sp2mc
MCD_FR = 4                   # kwy_mcep.hip:128  #define MCD_FR 4           frames per workgroup of k_sp2mc_dense
MC_PARTS = 4                 # kwy_mcep.hip:95   q = tid >> 6: four strided partial sums
MC2_FRAMES = 16              # kwy_mcep.hip:183  t0 = blockIdx.x * 16       frames per MFMA tile
MC2_TILE_BINS = 16           # kwy_mcep.hip:191  ntile = (K + 15) / 16
MC2_TILES = 4                # kwy_mcep.hip:176  #define MC2_TILES 4        16 x 4 = 64 bins per wavefront step
MC2_KSTEP = 4                # kwy_mcep.hip:184  ksteps = (order + 4) / 4   coefficients per k-step
KWY_WAVES = 4                # kwy_internal.hpp  256 threads, four wavefronts
NCUT_EPS = 1e-40             # kwy_mcep.hip:246  if (mx > 1e-40) break;
LDS_MAX = 160 * 1024         # kwy_mcep.hip:262  #define KWY_SP2MC_LDS_MAX (160 * 1024)
K_MAX = 4097                 # kwy_mcep.hip:386  K > 4097 refused
FFT_LOG2 = (9, 10, 11, 12, 13)   # kwy_mcep.hip:393  l >= 9 && l <= 13


def sp2mc_lds(N, ncut):
    """kwy_mcep.hip:263-266 (sp2mc_lds): bytes of LDS of k_sp2mc"""
    H = N // 2
    return 16 * ((H + 1) + max(H // 8, 1)) + 8 * MC_FR * (256 + ncut)


def sp2mc_dense_lds(K):
    """kwy_mcep.hip:365 (launch_sp2mc_dense): bytes of LDS of k_sp2mc_dense"""
    return 8 * (MCD_FR * K + MCD_FR * 256)


def mc2sp_gy(T):
    """kwy_mcep.hip:375-376 (launch_mc2sp_dense): gx = (T + 15) / 16; gy = gx >= 512 ? 1 : (gx >= 256 ? 2 : 4)"""
    gx = (T + 15) // 16
    return 1 if gx >= 512 else (2 if gx >= 256 else 4)


GY_SWITCHES = (4081, 8177)   # the smallest T with gx = 256 and gx = 512


def ncut_of(N, order, alpha):
    """The host recursion that sizes k_sp2mc's matrix (kwy_mcep.hip:35-52, 243-248: freqt_step0, freqt_matrix and the
    cut): the number of cepstral indices whose column of the freqt matrix has an entry above NCUT_EPS, in double."""
    a, b = float(alpha), 1.0 - float(alpha) * float(alpha)
    g, d = [0.0] * (order + 1), [0.0] * (order + 1)
    g[0] = 1.0
    nc = 1
    for n in range(N):
        if max(abs(v) for v in g) > NCUT_EPS:
            nc = n + 1
        d[0] = g[0]
        g[0] = a * d[0]
        d[1] = g[1]
        g[1] = b * d[0] + a * d[1]
        for j in range(2, order + 1):
            d[j] = g[j]
            g[j] = d[j - 1] + a * (d[j] - g[j - 1])
    return nc


def sp2mc_form(K, order, alpha):
    """'fft' or 'dense': the kernel kwy_sp2mc_dev takes (kwy_mcep.hip:393, 405-407)"""
    N = 2 * (K - 1)
    if N & (N - 1) or N.bit_length() - 1 not in FFT_LOG2:
        return 'dense'
    return 'fft' if sp2mc_lds(N, ncut_of(N, order, alpha)) <= LDS_MAX else 'dense'


# ---- bounds ----------------------------------------------------------------------------------------------------------
MC_CAP, SP_CAP = 1e-12, 1e-11            # tests/test_backends_gpu.py
SP_LOG_SCALE = 15.0
MC_REL = min(MC_CAP, 8 * 1.376e-15)      # 8 x the worst of k_sp2mc and k_sp2mc_dense (table above)
SP_LOG = min(SP_CAP, 8 * 1.483e-14)      # 8 x the worst of k_mc2sp_mfma
ORACLE_MC_REL, ORACLE_SP_LOG = 1e-14, 1e-13   # the oracle against the long-double reference (test_mcep_cases.py)
F64_MAX = LD(np.finfo(np.float64).max)
F64_ZERO = LD(2.0) ** -1075              # below it a double rounds to 0


# ---- long-double references ------------------------------------------------------------------------------------------
def _cos_table(N):
    """cos(2 pi m / N), m < N, in long double"""
    two_pi = LD(8) * np.arctan(LD(1))
    return np.cos(two_pi * np.arange(N, dtype=LD) / LD(N))


def _cos_product(N, rows, cols, weights, x, block=256):
    """out[t, r] = sum_c weights[c] * cos(2 pi rows[r] cols[c] / N) * x[t, c], the cosine matrix built `block` rows at
    a time (K = 4097: 17 MB a block instead of 540 MB)"""
    tab = _cos_table(N)
    xw = np.ascontiguousarray((x * weights[None, :]).T)           # (cols, T)
    out = np.empty((x.shape[0], len(rows)), LD)
    cols = np.asarray(cols, np.int64)
    for r0 in range(0, len(rows), block):
        r = np.asarray(rows[r0:r0 + block], np.int64)
        out[:, r0:r0 + block] = (tab[(r[:, None] * cols[None, :]) % N] @ xw).T
    return out


def freqt_ref(c1, m2, alpha):
    """SPTK freqt on the rows of c1 (T, m1 + 1) -> (T, m2 + 1), in long double"""
    c1 = np.asarray(c1, LD)
    T, m1 = c1.shape[0], c1.shape[1] - 1
    a = LD(alpha)
    b = LD(1) - a * a
    g = np.zeros((m2 + 1, T), LD)
    d = np.zeros((m2 + 1, T), LD)
    c1t = np.ascontiguousarray(c1.T)
    for i in range(m1, -1, -1):
        d[0] = g[0]
        g[0] = c1t[i] + a * d[0]
        if m2 >= 1:
            d[1] = g[1]
            g[1] = b * d[0] + a * d[1]
        for j in range(2, m2 + 1):
            d[j] = g[j]
            g[j] = d[j - 1] + a * (d[j] - g[j - 1])
    return np.ascontiguousarray(g.T)


SP2MC_MUTANTS = ('half only', 'nyquist twice', 'c0 not halved')
MC2SP_MUTANTS = ('c[H] twice', 'last bin repeats', 'partial tile from zeros')


def sp2mc_ref(sp, order, alpha, mutant=None):
    """pysptk.sp2mc in long double: c = irfft(log P) (all N points), c[0] /= 2, freqt(c, order, alpha).
    mutant: one of SP2MC_MUTANTS, the wrong kernels test_mcep_cases.py must see rejected."""
    with np.errstate(all='ignore'):
        L = np.log(np.asarray(sp, LD))
        T, K = L.shape
        H, N = K - 1, 2 * (K - 1)
        w = np.full(K, LD(2), LD)
        w[0] = 1
        w[H] = 2 if mutant == 'nyquist twice' else 1
        if H == 0:
            raise ValueError('K >= 2')
        c = _cos_product(N, np.arange(N), np.arange(K), w / LD(N), L)
        if mutant != 'c0 not halved':
            c[:, 0] /= 2
        if mutant == 'half only':
            c = c[:, :H + 1]
        return freqt_ref(c, order, alpha)


def mc2sp_ref(mc, alpha, fftlen, mutant=None):
    """pysptk.mc2sp in long double: c = freqt(mc, fftlen/2, -alpha), c[0] *= 2, mirror, exp(real(rfft(c))).
    The result stays in long double, whose exponent range holds what overflows or vanishes in double."""
    with np.errstate(all='ignore'):
        mc = np.asarray(mc, LD)
        N, H = int(fftlen), int(fftlen) // 2
        K = H + 1
        c = freqt_ref(mc, H, -alpha)
        # rfft of the mirrored sequence: S[k] = 2 c0 + 2 sum_{0<i<H} c_i cos(2 pi i k / N) + c_H cos(pi k)
        w = np.full(K, LD(2), LD)
        w[H] = 2 if mutant == 'c[H] twice' else 1
        S = _cos_product(N, np.arange(K), np.arange(K), w, c)
        if mutant == 'last bin repeats':
            S[:, K - 1] = S[:, K - 2]
        if mutant == 'partial tile from zeros' and len(S) % MC2_FRAMES:
            S[-1] = 0
        return np.exp(S)


# ---- inputs ----------------------------------------------------------------------------------------------------------
SEED = 20261
Case = namedtuple('Case', 'K order alpha T')


def _seed(K, order, alpha, extra=0):
    return [SEED, K, order, int(round(abs(alpha) * 1e6)), int(alpha < 0), extra]


def spectra(K, order, alpha, T, extra=0):
    """The smooth-plus-rough spectra of test_backends_gpu.py::test_mcep_any_length, seeded per case: (T, K)"""
    rng = np.random.default_rng(_seed(K, order, alpha, extra))
    f = np.linspace(0, 1, K)
    return np.ascontiguousarray(np.exp(-6 * f[None, :] + 2 * np.cos(9 * f[None, :] + rng.uniform(0, 6, (T, 1)))
                                       + 0.3 * rng.standard_normal((T, K))) * 1e-3)


def mcep(ko, K, order, alpha, T, extra=0):
    """speech-like coefficients for mc2sp: the oracle's sp2mc of spectra(): (T, order + 1)"""
    return np.ascontiguousarray(ko.sp2mc(spectra(K, order, alpha, T, extra), order, alpha))


# k_sp2mc<LOG2N>
FFT_KS = (257, 513, 1025, 2049, 4097)
SP2MC_FFT_CASES = (
    [Case(K, 24, 0.41, 5) for K in FFT_KS]                           # every instance, one frame in the last workgroup
    + [Case(4097, 63, 0.77, 5)]                                      # ncut 1084 beside the 4096-point transform
    + [Case(257, 24, 0.41, T) for T in (1, 3, 4, 8, 9)]              # (T = 5 above)
    + [Case(257, o, 0.41, 5) for o in (1, 2, 3, 4, 62, 63)]
    + [Case(257, 63, a, 5) for a in (0.0, -0.41, 0.77, 0.9, 0.95, -0.9)]   # ncut saturates, the mirrored half matters
    + [Case(257, 1, 0.0, 5)]                                         # ncut 2: two of the four strides have no term
    + [Case(2049, 63, 0.9, 5)])                                      # the largest LDS that fits
# the settings k_sp2mc has no LDS for: the dense form takes them
SP2MC_FALLBACK_CASES = [Case(2049, 63, 0.95, 5), Case(4097, 63, 0.9, 5), Case(4097, 24, 0.97, 5)]
# k_sp2mc_dense
SP2MC_DENSE_CASES = (
    [Case(2, 1, 0.41, 5), Case(3, 2, 0.41, 5), Case(4, 3, 0.41, 5), Case(17, 16, 0.41, 5), Case(3, 1, 0.3, 5),
     Case(17, 8, 0.41, 5), Case(100, 24, 0.41, 5), Case(372, 24, 0.41, 5), Case(4096, 24, 0.41, 5)]
    + [Case(100, 24, 0.41, T) for T in (1, 3, 4)]
    + [Case(100, 40, a, 5) for a in (0.0, -0.41, 0.8)])
# k_mc2sp_mfma
MC2SP_KS = (2, 3, 16, 17, 63, 64, 65, 501, 2049, 4097)
MC2SP_CASES = (
    [Case(K, min(24, K - 1), 0.41, 17) for K in MC2SP_KS]
    + [Case(65, o, 0.41, 17) for o in (1, 2, 3, 4, 7, 8, 63)]        # (24 above)
    + [Case(65, 3, 0.41, T) for T in (1, 15, 16, 33)]                # (17 above)
    + [Case(17, 8, a, 17) for a in (0.0, 0.41, -0.41, 0.9, -0.9)])
# across the grid's gy switches: DISTINCT rows, tiled down the matrix
DISTINCT = 37
MC2SP_GRID_CASES = [Case(65, 24, 0.41, T) for T in (4080, 4081, 8176, 8177)] + [Case(1025, 24, 0.41, 8177)]
# rows whose c0 puts the log-spectrum near these values: finite, +inf, normal (1e-304), 0
RANGE_TARGETS = (690.0, 720.0, -700.0, -800.0)
RANGE_CASE = Case(65, 24, 0.41, len(RANGE_TARGETS))


def range_mcep(ko):
    """RANGE_CASE's coefficients: a quarter of a speech-like row's shape, c0 = target / 2 (log P = 2 c0 + shape)"""
    mc = mcep(ko, *RANGE_CASE)
    mc[:, 1:] *= 0.25
    mc[:, 0] = np.array(RANGE_TARGETS) / 2
    return mc


def range_class(ref):
    """(over, under) masks of a reference spectrum: bins a double holds as +inf, as 0"""
    ref = np.asarray(ref, LD)
    return ref > F64_MAX, ref < F64_ZERO


def case_id(c):
    return f'K{c.K}-o{c.order}-a{c.alpha:g}-T{c.T}'


# ---- assertions ------------------------------------------------------------------------------------------------------
def mc_error(got, ref):
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def assert_mc_close(got, ref, label, bound=None):
    """max |got - ref| <= MC_REL max |ref| over the call; every value finite"""
    bound = MC_REL if bound is None else bound
    assert got.shape == ref.shape, f'{label}: shape {got.shape}, expected {ref.shape}'
    assert np.isfinite(np.asarray(got, np.float64)).all(), f'{label}: non-finite coefficients'
    e = mc_error(got, ref)
    print(f'{label}: mc error {e:.3e} of max |ref| (bound {bound:.1e})')
    assert e <= bound, f'{label}: mc error {e:.3e} of max |ref| exceeds {bound:.1e}'
    return e


def sp_error(got, ref):
    """(max |log got - log ref| over the bins finite and non-zero in double, the bound's scale
    max(1, max |log ref| / 15)) after checking that got is +inf exactly where ref overflows a double and 0 exactly
    where it vanishes"""
    got, ref = np.asarray(got), np.asarray(ref, LD)
    over, under = range_class(ref)
    assert np.array_equal(np.isposinf(got), over), 'the +inf bins differ from the reference'
    assert np.array_equal(got == 0, under), 'the zero bins differ from the reference'
    live = ~(over | under)
    if not live.any():
        return 0.0, 1.0
    assert (np.isfinite(got[live]) & (got[live] > 0)).all(), 'a non-positive or non-finite bin'
    lr = np.log(ref[live])
    e = float(np.abs(np.log(got[live].astype(LD)) - lr).max())
    return e, max(1.0, float(np.abs(lr).max()) / SP_LOG_SCALE)


def assert_sp_close(got, ref, label, bound=None):
    """|log got - log ref| <= SP_LOG max(1, max |log ref| / 15) on every bin; the overflowed and vanished bins exact"""
    bound = SP_LOG if bound is None else bound
    assert got.shape == ref.shape, f'{label}: shape {got.shape}, expected {ref.shape}'
    try:
        e, scale = sp_error(got, ref)
    except AssertionError as err:
        raise AssertionError(f'{label}: {err}') from None
    print(f'{label}: sp log error {e:.3e} (bound {bound:.1e} x {scale:.3g})')
    assert e <= bound * scale, f'{label}: sp log error {e:.3e} exceeds {bound:.1e} x {scale:.3g}'
    return e


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- device calls ----------------------------------------------------------------------------------------------------
GUARD_DOUBLES = 64


def _guarded(ctx, call, T, width):
    """call(pointer) writes (T, width) doubles; they lie in a NaN-filled buffer with guard rows in front and behind
    (at least GUARD_DOUBLES each), which must stay NaN.  -> (return code, the (T, width) interior)"""
    import torch
    g = -(-GUARD_DOUBLES // width)
    buf = torch.full((T + 2 * g, width), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    rc = call(buf[g].data_ptr())
    ctx.sync()
    h = buf.cpu().numpy()
    assert np.isnan(h[:g]).all() and np.isnan(h[T + g:]).all(), 'a write outside the output'
    return rc, h[g:T + g]


def run_sp2mc(ctx, sp, order, alpha, check=True):
    """kwy_sp2mc_dev on sp (T, K): (T, order + 1) doubles, the guards checked"""
    import torch
    from kwiiyatta_amd import _lib
    T, K = sp.shape
    d = torch.from_numpy(np.ascontiguousarray(sp, dtype=np.float64)).cuda()
    rc, out = _guarded(ctx, lambda p: _lib.lib.kwy_sp2mc_dev(ctx.handle, d.data_ptr(), T, K, order, alpha, p), T,
                       order + 1)
    if check:
        _lib.check(ctx, rc)
        return out
    return rc, out


def run_mc2sp(ctx, mc, alpha, fftlen, check=True):
    """kwy_mc2sp_dev on mc (T, order + 1): (T, fftlen / 2 + 1) doubles, the guards checked"""
    import torch
    from kwiiyatta_amd import _lib
    T, order = mc.shape[0], mc.shape[1] - 1
    d = torch.from_numpy(np.ascontiguousarray(mc, dtype=np.float64)).cuda()
    rc, out = _guarded(ctx, lambda p: _lib.lib.kwy_mc2sp_dev(ctx.handle, d.data_ptr(), T, order, alpha, fftlen, p), T,
                       fftlen // 2 + 1)
    if check:
        _lib.check(ctx, rc)
        return out
    return rc, out


# ---- references shared by the tests of one process -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sp2mc_long(case, mutant=None):
    return sp2mc_ref(spectra(*case), case.order, case.alpha, mutant)


@functools.lru_cache(maxsize=None)
def sp2mc_oracle(case):
    from oracle import oracle as ko
    return ko.sp2mc(spectra(*case), case.order, case.alpha)


@functools.lru_cache(maxsize=None)
def mc2sp_input(case):
    """the coefficients of a mc2sp case; of a grid case, its DISTINCT rows (tile with tiled())"""
    from oracle import oracle as ko
    if case == RANGE_CASE:
        return range_mcep(ko)
    return mcep(ko, case.K, case.order, case.alpha, min(case.T, DISTINCT))


@functools.lru_cache(maxsize=None)
def mc2sp_long(case, mutant=None):
    return mc2sp_ref(mc2sp_input(case), case.alpha, 2 * (case.K - 1), mutant)


@functools.lru_cache(maxsize=None)
def mc2sp_oracle(case):
    from oracle import oracle as ko
    return ko.mc2sp(mc2sp_input(case), case.alpha, 2 * (case.K - 1))


def tiled(rows, T):
    return np.ascontiguousarray(rows[np.arange(T) % len(rows)])
