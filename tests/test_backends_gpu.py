"""GPU parity of the remaining hot-path kernels against the CPU oracle, through
the C ABI: mel-cepstrum (sp2mc/mc2sp), FastDTW, GMM+MLPG conversion, and the
f0 front-end (DIO, StoneMask).

Tolerances: mel-cepstrum 1e-12 relative (same algorithm, different summation
order); FastDTW path and distance bit-exact (integer path, identical distance
arithmetic); MLPG 1e-10 relative; DIO and StoneMask by tests/f0_cases.py
(identical voicing decisions and F0_ABS in Hz; F0_REL per frame)."""
import os

import numpy as np
import pytest
from scipy.io import wavfile

from conftest import CLB_WAV, SLT_WAV, clb_variant
from f0_cases import all_frames, assert_f0_close, assert_refined_close

pytestmark = pytest.mark.gpu


def load(path):
    fs, d = wavfile.read(path)
    return fs, np.ascontiguousarray(d.astype(np.float64) / 2 ** 15)


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def clb(ko):
    fs, x = load(CLB_WAV)
    f0, t = ko.dio(x, fs)
    f0 = ko.stonemask(x, f0, t, fs)
    sp = ko.cheaptrick(x, f0, t, fs) / fs
    return dict(fs=fs, x=x, f0=f0, t=t, sp=sp)


@pytest.mark.parametrize('order', [24, 36, 48])
def test_sp2mc_mc2sp(ko, clb, order):
    from kwiiyatta_amd.backend import sptk
    alpha = sptk.mcepalpha(clb['fs'])
    assert alpha == pytest.approx(ko.mcepalpha(clb['fs']), abs=1e-12)
    ref = ko.sp2mc(clb['sp'], order, alpha)
    got = sptk.sp2mc(clb['sp'], order, alpha)
    assert got.shape == ref.shape == (len(clb['f0']), order + 1)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    fftlen = (clb['sp'].shape[1] - 1) * 2
    ref2 = ko.mc2sp(ref, alpha, fftlen)
    got2 = sptk.mc2sp(ref, alpha, fftlen)
    assert np.max(np.abs(got2 - ref2) / ref2) <= 1e-11
    # 1-D input is handled like pysptk's apply-along-last-axis
    assert np.allclose(sptk.sp2mc(clb['sp'][5], order, alpha), got[5], rtol=0, atol=0)


def test_mcep_48k(ko):
    from kwiiyatta_amd.backend import sptk
    fs, x = load(clb_variant('48'))
    f0, t = ko.dio(x, fs)
    sp = ko.cheaptrick(x, f0, t, fs) / fs
    alpha = sptk.mcepalpha(fs)
    assert abs(alpha - 0.554) < 1e-9
    ref = ko.sp2mc(sp, 24, alpha)
    got = sptk.sp2mc(sp, 24, alpha)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.max(np.abs(sptk.mc2sp(ref, alpha, 2048) / ko.mc2sp(ref, alpha, 2048) - 1)) <= 1e-11


@pytest.mark.parametrize('K,order,alpha', [(372, 24, 0.41), (1024, 24, 0.554), (3078, 36, 0.63), (129, 24, 0.31)])
def test_mcep_any_length(ko, K, order, alpha):
    """Spectral lengths that are not 2^n + 1 (the reference's resampled spectra, vocoder/mcep.py:31-45):
    the dense form of sp2mc / mc2sp against numpy's irfft / rfft + freqt."""
    from kwiiyatta_amd.backend import sptk
    rng = np.random.default_rng(K)
    f = np.linspace(0, 1, K)
    sp = np.exp(-6 * f[None, :] + 2 * np.cos(9 * f[None, :] + rng.uniform(0, 6, (37, 1)))
                + 0.3 * rng.standard_normal((37, K))) * 1e-3
    ref = ko.sp2mc(sp, order, alpha)
    got = sptk.sp2mc(sp, order, alpha)
    assert got.shape == ref.shape == (37, order + 1)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    ref2 = ko.mc2sp(ref, alpha, 2 * (K - 1))
    got2 = sptk.mc2sp(ref, alpha, 2 * (K - 1))
    assert got2.shape == ref2.shape == (37, K)
    assert np.max(np.abs(got2 / ref2 - 1)) <= 1e-11


def _series(rng, T, dim, warp):
    t = np.linspace(0, 1, T) ** warp
    base = np.stack([np.sin(2 * np.pi * (k + 1) * t * 3 + k) for k in range(dim)], 1)
    return base + 0.05 * rng.standard_normal((T, dim))


@pytest.mark.parametrize('Tx,Ty,dim,radius', [
    (1, 1, 2, 1), (2, 5, 3, 1), (20, 17, 3, 32), (33, 34, 4, 32), (35, 70, 4, 32), (70, 90, 5, 1),
    (300, 350, 26, 32), (737, 801, 25, 1), (2201, 2401, 26, 32), (2401, 2201, 26, 32),
    (4700, 5300, 3, 8),     # boundary rows too long for LDS (the global-memory variant of the recurrence)
    (40, 9000, 2, 32), (9000, 40, 2, 32),   # windows wider than a strip's LDS (the back-trace in one piece) / 141 strips
    (1500, 1400, 2, 300), (900, 1000, 3, 100),    # wide bands: some strips keep their entry columns, some do not
    (130, 150, 70, 32)])   # more dimensions than one LDS tile of the distances
def test_fastdtw_bit_exact(ko, Tx, Ty, dim, radius):
    from kwiiyatta_amd.backend import dtw
    rng = np.random.default_rng(Tx * 7919 + Ty)
    x, y = _series(rng, Tx, dim, 1.0), _series(rng, Ty, dim, 1.3)
    d_ref, p_ref = ko.fastdtw(x, y, radius=radius, dist=2)
    d_got, p_got = dtw.fastdtw(x, y, radius=radius, dist=2)
    assert p_got == p_ref
    assert d_got == d_ref
    # path properties: monotone, unit steps, end points
    p = np.array(p_got)
    assert tuple(p[0]) == (0, 0) and tuple(p[-1]) == (Tx - 1, Ty - 1)
    dp = np.diff(p, axis=0)
    assert ((dp >= 0) & (dp <= 1)).all() and (dp.sum(axis=1) >= 1).all()


def test_fastdtw_rejects_radius_zero(ko):
    """radius 0 leaves the last row of an odd-length series without window cells: fastdtw 0.3.2 raises a KeyError
    there; the library and the oracle refuse the call."""
    from kwiiyatta_amd.backend import dtw
    x, y = np.zeros((5, 2)), np.ones((7, 2))
    with pytest.raises(ValueError):
        dtw.fastdtw(x, y, radius=0, dist=2)
    with pytest.raises(ValueError):
        ko.fastdtw(x, y, radius=0, dist=2)


def test_fastdtw_fuzz(ko):
    """Random shapes, radii and kinds of series (smooth, quantised with many exact ties, piecewise constant with long
    plateaux, steep local slopes): path and distance bit-exact.  The kernels take different routes with the size
    (number of levels, strips per level, single-strip levels in one fused launch, windows computed by the previous
    level's trace from a table or by binary searches, entry columns per strip or the path walked in one piece,
    predecessor planes staged in LDS or read from memory)."""
    from kwiiyatta_amd.backend import dtw
    rng = np.random.default_rng(20261004)
    kinds = ('smooth', 'ties', 'plateaux', 'steep')
    for case in range(40):
        Tx, Ty = (int(v) for v in rng.integers(1, 700, 2))
        if case % 8 == 0:
            Tx, Ty = int(rng.integers(900, 1500)), int(rng.integers(900, 1500))
        dim = int(rng.integers(1, 4))
        radius = int(rng.choice([1, 2, 5, 32]))
        kind = kinds[case % len(kinds)]
        if kind == 'smooth':
            x, y = _series(rng, Tx, dim, 1.0), _series(rng, Ty, dim, 1.3)
        elif kind == 'ties':
            x = np.round(_series(rng, Tx, dim, 1.0) * 2.0) / 2.0
            y = np.round(_series(rng, Ty, dim, 1.3) * 2.0) / 2.0
        elif kind == 'plateaux':
            x = np.repeat(rng.integers(0, 4, (Tx // 17 + 1, dim)).astype(np.float64), 17, axis=0)[:Tx]
            y = np.repeat(rng.integers(0, 4, (Ty // 29 + 1, dim)).astype(np.float64), 29, axis=0)[:Ty]
        else:       # the same curve traversed at very different local speeds
            base = _series(rng, 2000, dim, 1.0)
            ix = np.sort(rng.integers(0, 2000, Tx))
            iy = np.sort((2000 * rng.random(Ty) ** 3).astype(int).clip(0, 1999))
            x, y = np.ascontiguousarray(base[ix]), np.ascontiguousarray(base[iy])
        ref = ko.fastdtw(x, y, radius=radius, dist=2)
        got = dtw.fastdtw(x, y, radius=radius, dist=2)
        assert got[1] == ref[1], (case, kind, Tx, Ty, dim, radius)
        assert got[0] == ref[0], (case, kind, Tx, Ty, dim, radius)


@pytest.mark.parametrize('Tx,Ty,radius', [(5300, 5100, 1), (4900, 5600, 32)])
def test_fastdtw_long_series(ko, Tx, Ty, radius):
    """More than 4 798 target frames: the strips' boundary rows no longer fit the LDS and travel through global
    memory (the kernel's other instantiation); 25 s and 28 s at a 5 ms hop."""
    from kwiiyatta_amd.backend import dtw
    rng = np.random.default_rng(Tx + Ty)
    x, y = _series(rng, Tx, 3, 1.0), _series(rng, Ty, 3, 1.2)
    assert dtw.fastdtw(x, y, radius=radius, dist=2) == ko.fastdtw(x, y, radius=radius, dist=2)


def test_fastdtw_ties_and_1d(ko):
    """Exact ties (integer-valued, repeated frames) exercise the predecessor order."""
    from kwiiyatta_amd.backend import dtw
    x = np.array([0, 0, 1, 1, 2, 2, 2, 3, 0, 0, 5, 5, 5, 1], dtype=np.float64)
    y = np.array([0, 1, 1, 1, 2, 3, 3, 0, 5, 1, 1], dtype=np.float64)
    for r in (1, 2, 32):
        assert dtw.fastdtw(x, y, radius=r, dist=2) == ko.fastdtw(x, y, radius=r, dist=2)
    xx = np.tile(x, 20)[:, None] * np.ones((1, 3))
    yy = np.tile(y, 23)[:, None] * np.ones((1, 3))
    assert dtw.fastdtw(xx, yy, radius=1, dist=2) == ko.fastdtw(xx, yy, radius=1, dist=2)


@pytest.mark.parametrize('M', [1, 4, 16])
@pytest.mark.parametrize('diff', [False, True])
def test_gmm_mlpg(ko, clb, M, diff):
    from sklearn.mixture import GaussianMixture
    from kwiiyatta_amd.backend import mlpg
    alpha = ko.mcepalpha(clb['fs'])
    mc = ko.sp2mc(clb['sp'], 24, alpha)[:, 1:]
    rng = np.random.default_rng(0)
    X = ko.delta_features(mc, ko.DELTA_WINDOWS)
    assert np.array_equal(mlpg.delta_features(mc, mlpg.DELTA_WINDOWS), X)
    Y = X @ (np.eye(72) + 0.05 * rng.standard_normal((72, 72))) + 0.1 * rng.standard_normal(X.shape)
    gmm = GaussianMixture(n_components=M, covariance_type='full', max_iter=15, random_state=0,
                          reg_covar=1e-4).fit(np.hstack([X, Y]))
    ref, mix_ref = ko.gmm_mlpg(mc, gmm.weights_, gmm.means_, gmm.covariances_, diff=diff, return_mix=True)
    got = mlpg.MLPG(gmm, windows=mlpg.DELTA_WINDOWS, diff=diff).transform(X)
    assert got.shape == ref.shape == mc.shape
    assert np.abs(got - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1.0)
    if M > 1:
        assert len(np.unique(mix_ref)) > 1   # the selection step is exercised


class _RandomGMM:
    """joint GMM with random SPD covariances (no fit: any static dimension, any size)"""
    covariance_type = 'full'

    def __init__(self, d, M, seed):
        rng = np.random.default_rng(seed)
        D2 = 6 * d
        self.weights_ = rng.dirichlet(np.ones(M))
        self.means_ = rng.standard_normal((M, D2))
        a = rng.standard_normal((M, D2, D2)) * 0.2
        self.covariances_ = a @ a.transpose(0, 2, 1) + np.eye(D2) * rng.uniform(0.5, 2.0, (M, 1, 1))


@pytest.mark.parametrize('d', [1, 3, 24, 27])       # 27: the largest static dimension whose model fits the LDS
@pytest.mark.parametrize('T', [1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 47, 48, 64, 100, 255, 256, 257, 520, 1031])
def test_mlpg_solve_partition_edges(ko, T, d):
    """The pentadiagonal solve is partitioned into up to 8 * (64 // d) chunks of >= 16 rows with two-row
    separators (kwy_mlpg.hip): every chunk count from 1 up, chunks of unequal length, two to 64 chunks per
    wavefront, against the serial CPU elimination."""
    from kwiiyatta_amd.backend import mlpg
    gmm = _RandomGMM(d, 2, seed=7 * d + T)
    rng = np.random.default_rng(T)
    x = np.cumsum(rng.standard_normal((T, d)) * 0.3, axis=0)
    for diff in (False, True):
        ref = ko.gmm_mlpg(x, gmm.weights_, gmm.means_, gmm.covariances_, diff=diff)
        got = mlpg.MLPG(gmm, windows=mlpg.DELTA_WINDOWS, diff=diff).transform(x)
        assert got.shape == ref.shape == (T, d)
        assert np.abs(got - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1.0), (T, d, diff)


@pytest.mark.parametrize('M', [1, 4, 16])
@pytest.mark.parametrize('diff', [False, True])
def test_gmm_frame_wise_conversion(ko, clb, M, diff):
    """GMMFeatureConverter.convert(mlpg=False): windows[0:1] -> nnmnkwii's MLPGBase.transform, the
    posterior-weighted conditional mean of every frame (kwiiyatta/converter/gmm.py:28-34), through the package's
    converter object against the restated upstream routine (posteriors from scikit-learn's predict_proba)."""
    from sklearn.mixture import GaussianMixture
    from kwiiyatta_amd.converter.gmm import GMMFeatureConverter
    alpha = ko.mcepalpha(clb['fs'])
    mc = ko.sp2mc(clb['sp'], 24, alpha)[:, 1:]
    rng = np.random.default_rng(1)
    X = ko.delta_features(mc, ko.DELTA_WINDOWS)
    Y = X @ (np.eye(72) + 0.05 * rng.standard_normal((72, 72))) + 0.1 * rng.standard_normal(X.shape)
    conv = GMMFeatureConverter(components=M)
    conv.gmm = GaussianMixture(n_components=M, covariance_type='full', max_iter=15, random_state=0,
                               reg_covar=1e-4).fit(np.hstack([X, Y]))
    got = conv.convert(X, mlpg=False, diff=diff)
    ref = ko.gmm_convert_frames(X, conv.gmm.weights_, conv.gmm.means_, conv.gmm.covariances_, diff=diff)
    assert got.shape == ref.shape == X.shape
    assert np.abs(got - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1.0)
    # and the trajectory-smoothed conversion of the same object still goes the MLPG way
    assert conv.convert(X, mlpg=True, diff=diff).shape == (len(X), 24)


def test_gmm_mlpg_errors(clb):
    from kwiiyatta_amd.backend import mlpg

    class G:  # indefinite source covariance -> ValueError, not garbage
        covariance_type = 'full'
        weights_ = np.array([1.0])
        means_ = np.zeros((1, 12))
        covariances_ = -np.eye(12)[None]
    with pytest.raises(ValueError):
        mlpg.MLPG(G()).transform(np.zeros((5, 2)))


@pytest.mark.parametrize('path', [CLB_WAV, SLT_WAV, clb_variant('22'), clb_variant('48'), clb_variant('96')])
@pytest.mark.parametrize('frame_period', [5.0, 3.0])
def test_dio_stonemask(ko, path, frame_period):
    from kwiiyatta_amd.backend import world
    fs, x = load(path)
    label = f'{os.path.basename(os.path.dirname(os.path.dirname(path)))} {fs} period {frame_period}'
    f0_ref, t_ref = ko.dio(x, fs, frame_period=frame_period)
    assert_f0_close(world.dio(x, fs, frame_period=frame_period), (f0_ref, t_ref), all_frames(f0_ref), label)
    s_ref = ko.stonemask(x, f0_ref, t_ref, fs)
    assert_refined_close(world.stonemask(x, f0_ref, t_ref, fs), s_ref, label, f0_in=f0_ref)


def test_dio_short_and_silent(ko):
    from kwiiyatta_amd.backend import world
    fs = 16000
    x = np.zeros(3000)
    f0, t = world.dio(x, fs)
    f0r, tr = ko.dio(x, fs)
    assert_f0_close((f0, t), (f0r, tr), all_frames(f0r), 'silence', f0_abs=0.0)
    assert np.array_equal(f0, f0r) and np.array_equal(t, tr) and not f0.any()
    rng = np.random.default_rng(1)
    x = rng.standard_normal(800) * 0.1      # shorter than the voiced-range minimum
    f0, t = world.dio(x, fs)
    f0r, tr = ko.dio(x, fs)
    assert_f0_close((f0, t), (f0r, tr), all_frames(f0r), '800 samples of noise', f0_abs=0.0)
    assert np.array_equal(t, tr) and np.array_equal(f0, f0r)
    s, sr = world.stonemask(x, f0, t, fs), ko.stonemask(x, f0r, tr, fs)
    assert_refined_close(s, sr, '800 samples of noise', f0_in=f0r, f0_rel=0.0)
    assert np.array_equal(s, sr)


# ---------------------------------------------------------------- spectral-axis stretch (reshape), SURVEY 8f-3
@pytest.mark.parametrize('bins,new_bins', [(513, 1025), (1025, 513), (1025, 2049), (2049, 1025), (2049, 513),
                                           (372, 513), (1024, 1025), (3078, 4097), (513, 372), (65, 129), (129, 130),
                                           (1025, 1025)])
def test_stretch_log_matches_resample_poly(bins, new_bins):
    """kwy_stretch_log against the reference's own call chain (np.log -> edge replication -> scipy.signal.resample_poly
    -> trim -> np.exp) on spectra with a 120 dB range; relative 1e-12."""
    from oracle import oracle as ko
    from kwiiyatta_amd.backend import resample
    rng = np.random.default_rng(bins * 7 + new_bins)
    T = 37
    rows = np.exp(np.cumsum(rng.standard_normal((T, bins)), axis=1) * 0.35 + rng.uniform(-8, 2, (T, 1)))
    got = resample.stretch_log(rows, new_bins)
    want = ko.stretch_log(rows, new_bins)
    assert got.shape == want.shape == (T, new_bins)
    assert np.abs(got / want - 1).max() <= 1e-12


def test_stretch_log_device_rows_and_tiles():
    """device-pointer entry on a row count that is not a multiple of the rows per workgroup, and aperiodicity-like
    values in (0, 1)"""
    import torch
    from oracle import oracle as ko
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, c_vp
    ctx = _lib.Context(0)
    rng = np.random.default_rng(5)
    for T, bins, new_bins in ((1, 1025, 513), (13, 513, 1025), (2201, 513, 1025)):
        rows = 1.0 / (1.0 + np.exp(-np.cumsum(rng.standard_normal((T, bins)), axis=1) * 0.2))
        d_in = torch.from_numpy(rows).cuda()
        d_out = torch.empty((T, new_bins), dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        _lib.check(ctx, lib.kwy_stretch_log_dev(ctx.handle, c_vp(d_in.data_ptr()), T, bins, new_bins,
                                                c_vp(d_out.data_ptr())))
        ctx.sync()
        sel = slice(None) if T < 100 else slice(0, T, 97)
        assert np.abs(d_out.cpu().numpy()[sel] / ko.stretch_log(rows[sel], new_bins) - 1).max() <= 1e-12
