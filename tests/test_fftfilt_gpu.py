"""The frame-parallel FFT differential filter on the GPU (csrc/kwy_fftfilt.hip) against the numpy restatement of its
contract (tests/fftfilt_cases.py): <= 1e-11 of the reference's peak, the bar the MLSA kernel is held to
(test_hip_mlsa_matches_oracle); the batch entry against single calls bit for bit; every KWY_EINVAL of the contract;
and corpus.convert_batch(diff_filter='fft') against the per-file path."""
import numpy as np
import pytest

import fftfilt_cases as fc
from conftest import CLB_WAV, SLT_WAV

pytestmark = pytest.mark.gpu

TOL = 1e-11


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(n):
    import torch
    return torch.full((n,), float('nan'), dtype=torch.float64, device='cuda')


def _single_dev(ctx, x, mc, y, alpha, hop, N, ignore):
    """kwy_mcep_filter_fft_dev on device tensors, synchronised; the return code"""
    import torch
    from kwiiyatta_amd._lib import lib, c_vp
    torch.cuda.synchronize()          # (torch filled the tensors on ITS stream; the library runs on the context's)
    rc = lib.kwy_mcep_filter_fft_dev(ctx.handle, c_vp(x.data_ptr()), x.numel(), c_vp(mc.data_ptr()), mc.shape[0],
                                     mc.shape[1] - 1, alpha, hop, N, ignore, c_vp(y.data_ptr()))
    ctx.sync()
    return rc


def _check(got, ref, nproc, hop):
    assert got.shape == ref.shape
    assert np.isfinite(got).all(), f'{np.count_nonzero(~np.isfinite(got))} samples not written'
    peak = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f'max difference {err:.3e}, peak {peak:.3e}, relative {err / peak if peak else 0.0:.3e}')
    assert err <= TOL * peak, err / peak
    assert np.all(got[nproc * hop:] == 0.0)


@pytest.mark.parametrize('ignore_c0', [1, 0])
@pytest.mark.parametrize('fs,order,N,hop', fc.RATES, ids=[f'{r[0]}-{r[1]}-{r[2]}' for r in fc.RATES])
def test_kernel_matches_restatement(gpu_ctx, fs, order, N, hop, ignore_c0):
    """n = T hop - 37: the first N / hop frames read before sample 0, the last frame is unprocessed; the output starts
    as NaN, so every sample the kernel leaves out shows; the host entry gives the same bits"""
    from oracle import oracle as ko
    from kwiiyatta_amd.backend import fftfilt
    rng = np.random.default_rng(30)
    T = fc.FRAMES
    alpha = ko.mcepalpha(fs)
    mc = fc.frames(rng, T, order, 0.4, c0=0.3)
    x = fc.signal(rng, T * hop - 37)
    ref = fc.fft_filter(x, mc, alpha, hop, N, ignore_c0=bool(ignore_c0))
    assert ignore_c0 or np.abs(ref - fc.fft_filter(x, mc, alpha, hop, N, True)).max() > 1e-3 * np.abs(ref).max()
    y = _nan(len(x))
    assert _single_dev(gpu_ctx, _dev(x), _dev(mc), y, alpha, hop, N, ignore_c0) == 0
    got = y.cpu().numpy()
    _check(got, ref, T - 1, hop)
    host = fftfilt.mcep_fft_filter(x, mc, alpha, hop, N, ignore_c0=bool(ignore_c0), ctx=gpu_ctx)
    assert host.tobytes() == got.tobytes()


@pytest.mark.parametrize('name,n_of,T', fc.EDGES, ids=[e[0] for e in fc.EDGES])
def test_processed_frames_rule(gpu_ctx, name, n_of, T):
    from oracle import oracle as ko
    fs, order, N, hop = fc.RATES[0]
    alpha = ko.mcepalpha(fs)
    rng = np.random.default_rng(31)
    n = n_of(hop)
    mc = fc.frames(rng, T, order, 0.4, c0=0.2)
    x = fc.signal(rng, n) + 0.5
    ref = fc.fft_filter(x, mc, alpha, hop, N, ignore_c0=False)
    y = _nan(n)
    assert _single_dev(gpu_ctx, _dev(x), _dev(mc), y, alpha, hop, N, 0) == 0
    nproc = min(T, (n - 1) // hop)
    got = y.cpu().numpy()
    _check(got, ref, nproc, hop)
    assert np.all(got[:nproc * hop] != 0.0)
    if n <= hop:
        assert not got.any()


def test_long_zero_tail_is_written_in_pieces(gpu_ctx):
    """T far shorter than the signal: the tail is longer than one workgroup's piece of it"""
    fs, order, N, hop = fc.RATES[0]
    rng = np.random.default_rng(32)
    n, T = 40000, 2
    mc = fc.frames(rng, T, order)
    x = fc.signal(rng, n)
    y = _nan(n)
    assert _single_dev(gpu_ctx, _dev(x), _dev(mc), y, 0.41, hop, N, 1) == 0
    _check(y.cpu().numpy(), fc.fft_filter(x, mc, 0.41, hop, N), T, hop)


def test_batch_equals_single_calls_bit_for_bit():
    """70 signals of different lengths: more than one launch holds (64).  Every job equals its single call, and two
    runs of the batch give the same bits."""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import fftfilt
    rng = np.random.default_rng(33)
    order, alpha, hop, N = 24, 0.55, 240, 2048
    ctx = _lib.Context(0)
    xs, mcs = [], []
    for i in range(70):
        T = int(rng.integers(1, 14))
        n = max(1, T * hop + int(rng.integers(-hop + 1, 2 * hop)))
        xs.append(_dev(fc.signal(rng, n)))
        mcs.append(_dev(rng.standard_normal((T, order + 1)) * 0.05))
    for ignore in (True, False):
        runs = []
        for _ in range(2):
            ys = [_nan(x.numel()) for x in xs]
            torch.cuda.synchronize()
            fftfilt.mcep_fft_filter_batch_dev(ctx, xs, mcs, ys, alpha, hop, N, ignore_c0=ignore)
            ctx.sync()
            runs.append(ys)
        for a, b in zip(*runs):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
        for i in list(range(0, 70, 6)) + [63, 64, 69]:
            y1 = _nan(xs[i].numel())
            assert _single_dev(ctx, xs[i], mcs[i], y1, alpha, hop, N, int(ignore)) == 0
            assert torch.equal(runs[0][i], y1), i
    # one job against the restatement: the batch is the same filter, not just the same bits
    ref = fc.fft_filter(xs[5].cpu().numpy(), mcs[5].cpu().numpy(), alpha, hop, N, ignore_c0=False)
    _check(runs[0][5].cpu().numpy(), ref, min(mcs[5].shape[0], (xs[5].numel() - 1) // hop), hop)
    torch.cuda.synchronize()
    fftfilt.mcep_fft_filter_batch_dev(ctx, [], [], [], alpha, hop, N)


def test_every_einval_leaves_the_output_untouched(gpu_ctx):
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, c_vp
    from kwiiyatta_amd.backend import fftfilt
    ctx = gpu_ctx
    rng = np.random.default_rng(34)
    hop, T = 80, 6
    n = T * hop + 9
    x = _dev(fc.signal(rng, n))
    mcs = {order: _dev(rng.standard_normal((T, order + 1)) * 0.05) for order in (1, 24, 63)}
    y = torch.full((n,), 9.0, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()

    def single(x_=x, order=24, alpha=0.41, hop_=hop, N=1024, y_=y, mc_=True, n_=n, T_=T):
        mc = mcs[order].data_ptr() if mc_ else None
        return lib.kwy_mcep_filter_fft_dev(ctx.handle, c_vp(x_.data_ptr()) if x_ is not None else None, n_, c_vp(mc), T_,
                                           order, alpha, hop_, N, 1, c_vp(y_.data_ptr()) if y_ is not None else None)

    def batch(**kw):
        """the same call as the middle job of three"""
        bad = dict(x=x, n=n, mc=mcs[kw.get('order', 24)], T=T, y=y)
        bad.update({k: v for k, v in kw.items() if k in bad})
        others = [torch.full((n,), 9.0, dtype=torch.float64, device='cuda') for _ in range(2)]
        torch.cuda.synchronize()
        order = kw.get('order', 24)
        rows = [(x, n, mcs[order], T, others[0]),
                tuple(0 if bad[k] is None else bad[k] for k in ('x', 'n', 'mc', 'T', 'y')),
                (x, n, mcs[order], T, others[1])]
        rc = lib.kwy_mcep_filter_fft_batch_dev(ctx.handle, _lib.job_array(_lib.MlsaJob, rows), 3, order,
                                               kw.get('alpha', 0.41), kw.get('hop_', hop), kw.get('N', 1024), 1)
        ctx.sync()
        assert all(bool((o == 9.0).all()) for o in others)
        return rc

    assert single() == 0                                     # (the call the bad ones are variations of)
    ctx.sync()
    assert bool(torch.isfinite(y).all()) and not bool((y == 9.0).any())
    y.fill_(9.0)
    torch.cuda.synchronize()
    overlap = torch.full((n + 10,), 9.0, dtype=torch.float64, device='cuda')
    cases = [dict(N=512), dict(N=1000), dict(N=1536), dict(N=16384), dict(N=0),      # fft_size outside the four
             dict(N=1024, hop_=1024), dict(N=1024, hop_=2000), dict(N=2048, hop_=2048),   # fft_size <= hopsize
             dict(hop_=0), dict(hop_=-80),
             dict(order=1), dict(order=63),
             dict(alpha=1.0),
             dict(n_=0), dict(T_=0)]
    for kw in cases:
        assert single(**kw) == _lib.KWY_EINVAL, kw
        assert 'mcep_filter_fft' in ctx.error()
    for kw in (dict(N=512), dict(N=1024, hop_=1024), dict(hop_=0), dict(order=1), dict(order=63)):
        assert batch(**kw) == _lib.KWY_EINVAL, kw
    for kw in (dict(x_=None), dict(mc_=False), dict(y_=None)):
        assert single(**kw) == _lib.KWY_EINVAL, kw
    for kw in (dict(x=None), dict(mc=None), dict(y=None), dict(n=0), dict(T=0), dict(y=x)):
        assert batch(**kw) == _lib.KWY_EINVAL, kw
    # y aliasing x: the same buffer, and buffers that overlap either way
    assert single(y_=x) == _lib.KWY_EINVAL and 'alias' in ctx.error()
    assert single(x_=overlap[:n], y_=overlap[10:]) == _lib.KWY_EINVAL
    assert single(x_=overlap[10:], y_=overlap[:n]) == _lib.KWY_EINVAL
    assert lib.kwy_mcep_filter_fft_batch_dev(ctx.handle, None, 3, 24, 0.41, hop, 1024, 1) == _lib.KWY_EINVAL
    assert lib.kwy_mcep_filter_fft_batch_dev(ctx.handle, None, -1, 24, 0.41, hop, 1024, 1) == _lib.KWY_EINVAL
    ctx.sync()
    assert bool((y == 9.0).all()) and bool((overlap == 9.0).all())
    assert np.array_equal(x.cpu().numpy(), fc.signal(np.random.default_rng(34), n))
    # count == 0 is not an error
    assert lib.kwy_mcep_filter_fft_batch_dev(ctx.handle, None, 0, 24, 0.41, hop, 1024, 1) == _lib.KWY_OK
    # the host entry: the same checks, as ValueError
    xh = fc.signal(rng, n)
    for kw in (dict(fft_size=512), dict(fft_size=1024, hopsize=1024), dict(hopsize=0)):
        with pytest.raises(ValueError, match='mcep_filter_fft'):
            fftfilt.mcep_fft_filter(xh, np.zeros((T, 25)), 0.41, **{**dict(hopsize=hop, fft_size=1024), **kw}, ctx=ctx)
    with pytest.raises(ValueError, match='mcep_filter_fft'):
        fftfilt.mcep_fft_filter(xh, np.zeros((T, 2)), 0.41, hop, 1024, ctx=ctx)


@pytest.fixture(scope='module')
def two_files():
    import kwiiyatta_amd as k
    from kwiiyatta_amd import pipeline as pl
    an = [k.analyze_wav(p) for p in (CLB_WAV, SLT_WAV)]
    gmm = pl.synthetic_gmm(order=24, components=4, seed=2, n_frames=4000)
    return an, gmm


def test_convert_batch_fft_diff_outputs(two_files):
    """corpus.convert_batch(diff=True, diff_filter='fft'): the differential output of every file equals
    apply_diff_filter(method='fft') of the differential conversion through the Python API's stages (same kernels,
    single calls) -- test_convert_batch_diff_outputs' comparison and bound -- and its int16 samples equal Wavdata.save's"""
    import torch
    import kwiiyatta_amd as k
    from kwiiyatta_amd import _lib, corpus, pipeline as pl
    from kwiiyatta_amd._lib import lib, c_vp
    an, gmm = two_files
    fs = an[0].fs
    waves_in = [np.ascontiguousarray(a.wavdata.data) for a in an]
    wav, pcm, dwav, dpcm = corpus.convert_batch(waves_in, fs, gmm, pcm=True, diff=True, diff_filter='fft')
    assert all(w is not None for w in wav) and all(p.dtype == torch.int16 for p in pcm)
    dg = pl.DeviceGMM(gmm.weights_, gmm.means_, gmm.covariances_, 'cuda:0')
    ctx = _lib.Context(0)
    for i, a in enumerate(an):
        mc = torch.from_numpy(np.ascontiguousarray(a.mel_cepstrum.data)).cuda()
        out = torch.empty_like(mc)
        torch.cuda.synchronize()
        _lib.check(ctx, lib.kwy_convert_mcep_dev(ctx.handle, c_vp(mc.data_ptr()), len(mc), 24, dg.M,
                                                 c_vp(dg.model(diff=True).data_ptr()), c_vp(out.data_ptr())))
        ctx.sync()
        rec = k.feature(a).mel_cepstrum
        rec.data = out.cpu().numpy()
        ref = k.apply_diff_filter(a.wavdata, rec, method='fft')
        got = dwav[i].cpu().numpy()
        assert got.shape == ref.data.shape
        assert np.abs(got - ref.data).max() <= 1e-12 * max(1.0, np.abs(ref.data).max())
        assert np.array_equal(dpcm[i].cpu().numpy(), k.Wavdata(fs, got.copy())._pcm16(True, {}))


def test_convert_batch_mlsa_is_the_default_bit_for_bit(two_files):
    import torch
    from kwiiyatta_amd import corpus
    an, gmm = two_files
    fs = an[0].fs
    waves_in = [np.ascontiguousarray(a.wavdata.data) for a in an]
    default = corpus.convert_batch(waves_in, fs, gmm, pcm=True, diff=True)
    named = corpus.convert_batch(waves_in, fs, gmm, pcm=True, diff=True, diff_filter='mlsa')
    for a, b in zip(default, named):
        assert all(torch.equal(u, v) for u, v in zip(a, b))
