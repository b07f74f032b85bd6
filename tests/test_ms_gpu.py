"""Modulation-spectrum postfilter on the MI355X: the log-spectrum, statistics and filter kernels of kwy_ms.hip through
the C ABI against their numpy statement (tests/ms_cases.py) within its bounds, their determinism and input edges, the
converter's statistics and composition, the batch path against the filter applied by hand, and what
`convert_voice --ms` writes.  Every test prints its worst error as a fraction of the bound."""
import pathlib
import shutil
import sys

import numpy as np
import pytest

import gv_cases as gc
import ms_cases as mc
from conftest import CLB_DIR, SLT_DIR

pytestmark = pytest.mark.gpu


def _run_cli(main, argv):
    old = sys.argv
    sys.argv = ['prog'] + argv
    try:
        main()
    finally:
        sys.argv = old


def _device():
    """device, stream, context: the tests upload from pageable memory (complete on return), launch on the stream,
    synchronise it and read back"""
    import torch
    from kwiiyatta_amd import _lib
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    return dev, stream, _lib.Context(0, stream=stream.cuda_stream)


def _up(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- the cases: every shape x every column count, computed once -------------------------------------------------------
@pytest.fixture(scope='module')
def cases():
    """{(L, cols): [dict(x, G, N)]} over ms_cases.SHAPES x COLS, plus T = 0 at L = 512; every third matrix with a
    constant last column.  The statistics are around each matrix's own spectra (ms_cases.stats_for)."""
    out = {}
    for q, (T, L) in enumerate(mc.SHAPES + ((0, 512),)):
        for cols in mc.COLS:
            rng = np.random.RandomState(7919 * q + cols)
            x = mc.matrix(rng, T, cols)
            if q % 3 == 0 and T >= 2 and cols >= 2:
                x[:, cols - 1] = 0.1
            G, N = mc.stats_for(x, L, rng)
            out.setdefault((L, cols), []).append(dict(x=x, G=G, N=N, base=x + rng.standard_normal(x.shape)))
    return out


def _check_spectra(x, L, got, valid):
    """worst error / bound over the bins >= 1 of one matrix; asserts that no bin is skipped"""
    want, ok = mc.log_spectra(x, L)
    assert valid.tolist() == ok.tolist()
    worst = 0.0
    for d in range(x.shape[1]):
        if not ok[d]:
            assert np.all(got[d] == 0)
            continue
        bound, usable = mc.log_spectrum_bound(x[:, d], L)
        assert usable[1:].all(), (x.shape, d, int((~usable[1:]).sum()))
        frac = np.abs(got[d, 1:] - want[d, 1:]) / bound[1:]
        assert np.all(frac <= 1), (x.shape, L, d, frac.max())
        worst = max(worst, frac.max())
    return worst


def test_log_spectra_against_numpy(cases):
    import torch
    from kwiiyatta_amd.backend import ms
    dev, stream, ctx = _device()
    worst = 0.0
    for (L, cols), group in cases.items():
        mats = [c['x'] for c in group]
        spectra, valid = ms.log_spectra(mats, L)
        assert spectra.shape == (len(mats), cols, L // 2 + 1) and valid.dtype == np.int32
        for x, s, v in zip(mats, spectra, valid):
            worst = max(worst, _check_spectra(x, L, s, v))
        d_mats = [_up(m, dev) for m in mats]
        d_s = torch.full(spectra.shape, np.nan, dtype=torch.float64, device=dev)
        d_v = torch.full(valid.shape, -1, dtype=torch.int32, device=dev)
        with torch.cuda.stream(stream):
            ms.log_spectra_batch_dev(ctx, d_mats, L, d_s, d_v)
        stream.synchronize()
        assert d_s.cpu().numpy().tobytes() == spectra.tobytes() and d_v.cpu().numpy().tobytes() == valid.tobytes()
    print(f'log-spectra: worst error / bound = {worst:.3e}')
    short = [c['x'] for c in cases[512, 25] if len(c['x']) < 2]
    assert sorted(len(m) for m in short) == [0, 1]
    assert not ms.log_spectra(short, 512)[1].any()


def test_stats_update_chunks_numpy_and_determinism():
    import torch
    from kwiiyatta_amd.backend import ms
    L, cols = 512, 25
    rng = np.random.RandomState(70)
    mats = [mc.matrix(rng, int(T), cols) for T in rng.randint(2, L + 1, size=70)]
    mats[5] = mats[5][:1]
    for m in mats[::9]:
        m[:, 3] = -1.5
    spectra, valid = ms.log_spectra(mats, L)                  # (70 matrices: more than one launch of 64)
    whole = ms.stats_update(ms.new_accumulator(cols, L), spectra, valid)
    by_64 = ms.new_accumulator(cols, L)
    for a, b in ((0, 64), (64, 70)):
        ms.stats_update(by_64, spectra[a:b], valid[a:b])
    by_10 = ms.new_accumulator(cols, L)
    for a in range(0, 70, 10):
        ms.stats_update(by_10, spectra[a:a + 10], valid[a:a + 10])
    again = ms.stats_update(ms.new_accumulator(cols, L), spectra, valid)
    for other in (by_64, by_10, again, ms.statistics(mats, L)):
        assert other.tobytes() == whole.tobytes()
    dev, stream, ctx = _device()
    d_acc = torch.zeros(whole.shape, dtype=torch.float64, device=dev)
    d_s, d_v = _up(spectra, dev), _up(valid, dev)
    with torch.cuda.stream(stream):
        ms.stats_update_dev(ctx, d_acc, d_s, d_v)
    stream.synchronize()
    assert d_acc.cpu().numpy().tobytes() == whole.tobytes()
    # against numpy: the yardstick's fold of the same rows, and the two-pass mean / M2 (sums of n terms of size max|s|
    # resp. sum s^2, tests/test_ms_cases.py)
    want = mc.stats_update(mc.new_accumulator(cols, L), spectra, valid)
    assert np.all(whole[:, 0] == 0) and np.all(whole[:, 1:, 0] == want[:, 1:, 0])
    assert whole[3, 1, 0] == 70 - 1 - len(mats[::9]) + (1 if 5 % 9 == 0 else 0) and whole[0, 1, 0] == 69
    worst = 0.0
    for d in range(cols):
        rows = spectra[valid[:, d] == 1, d, 1:]
        n = len(rows)
        for col, ref, scale in ((1, rows.mean(axis=0), np.abs(rows).max(axis=0)),
                                (2, ((rows - rows.mean(axis=0)) ** 2).sum(axis=0), (rows ** 2).sum(axis=0))):
            for other in (want[d, 1:, col], ref):
                frac = np.abs(whole[d, 1:, col] - other) / (8 * n * mc.U * scale)
                assert np.all(frac <= 1), (d, col, frac.max())
                worst = max(worst, frac.max())
    print(f'statistics: worst error / bound = {worst:.3e}')


CONFIGS = (dict(k=1.0, based=False, first_col=1), dict(k=0.5, based=True, first_col=0),
           dict(k=1.0, based=True, first_col=1), dict(k=0.5, based=False, first_col=0))


def _check_filter(c, k, based, first_col, got):
    base = c['base'] if based else None
    want, status = mc.postfilter(c['x'], c['G'], c['N'], k, base=base, first_col=first_col)
    assert status == 0
    bounds = mc.filter_bounds(c['x'], c['G'], c['N'], k, first_col=first_col)
    worst = 0.0
    for d in range(c['x'].shape[1]):
        if bounds[d] == 0:
            assert got[:, d].tobytes() == np.ascontiguousarray((c['x'] if base is None else base)[:, d]).tobytes()
            continue
        frac = np.abs(got[:, d] - want[:, d]).max() / bounds[d]
        assert frac <= 1, (c['x'].shape, d, k, frac)
        worst = max(worst, frac)
    return worst


@pytest.mark.parametrize('config', CONFIGS, ids=lambda c: f"k{c['k']}-base{int(c['based'])}-first{c['first_col']}")
def test_filter_against_numpy(cases, config):
    from kwiiyatta_amd.backend import ms
    k, based, first_col = config['k'], config['based'], config['first_col']
    worst = 0.0
    for (L, cols), group in cases.items():
        for c in group:              # (the statistics differ per matrix: one call each)
            got = ms.postfilter(c['x'], c['G'], c['N'], k, base=c['base'] if based else None, first_col=first_col,
                                length=L)
            worst = max(worst, _check_filter(c, k, based, first_col, got))
    print(f'filter {config}: worst error / bound = {worst:.3e}')


def test_filter_with_offsets_of_500_sigma():
    from kwiiyatta_amd.backend import ms
    rng = np.random.RandomState(500)
    x = mc.matrix(rng, 257, 25, max_offset=500.0)
    G, N = mc.stats_for(x, 512, rng)
    c = dict(x=x, G=G, N=N, base=None)
    for k in (1.0, 0.5):
        frac = _check_filter(c, k, False, 1, ms.postfilter(x, G, N, k))
        print(f'500 sigma, k = {k}: worst error / bound = {frac:.3e}')
    spectra, valid = ms.log_spectra([x], 512)
    print(f'500 sigma log-spectra: worst error / bound = {_check_spectra(x, 512, spectra[0], valid[0]):.3e}')


def test_aliasing_batches_determinism_and_untouched_columns():
    import torch
    from kwiiyatta_amd.backend import ms
    dev, stream, ctx = _device()
    L, cols = 512, 25
    rng = np.random.RandomState(71)
    xs = [mc.matrix(rng, int(T), cols) for T in rng.randint(0, L + 1, size=70)]
    xs[2][:, 7] = 4.0
    G, N = mc.stats_for(xs[0] if len(xs[0]) > 1 else xs[1], L, rng)     # (any statistics of bounded gain will do)
    bases = [x + rng.standard_normal(x.shape) for x in xs]
    d_G, d_N = _up(G, dev), _up(N, dev)

    def run(first_col, k, alias=None, single=False):
        """the 70 ragged jobs in one call (or one call each); out: fresh, or aliasing `base` / `x`"""
        d_x, d_b = [_up(x, dev) for x in xs], [_up(b, dev) for b in bases]
        d_o = d_b if alias == 'base' else d_x if alias == 'x' else [torch.full_like(x, np.nan) for x in d_x]
        status = torch.full((70,), -1, dtype=torch.int32, device=dev)
        with torch.cuda.stream(stream):
            if single:
                for i in range(70):
                    ms.postfilter_batch_dev(ctx, d_x[i:i + 1], d_G, d_N, k, d_o[i:i + 1], bases=d_b[i:i + 1],
                                            first_col=first_col, status=status[i:i + 1])
            else:
                ms.postfilter_batch_dev(ctx, d_x, d_G, d_N, k, d_o, bases=d_b, first_col=first_col, status=status)
        stream.synchronize()
        assert not status.cpu().numpy().any()
        return [o.cpu().numpy() for o in d_o]

    first = run(1, 1.0)
    for other in (run(1, 1.0), run(1, 1.0, single=True), run(1, 1.0, alias='base'), run(1, 1.0, alias='x')):
        for a, b in zip(first, other):
            assert a.tobytes() == b.tobytes()
    host = ms.postfilter(xs, G, N, 1.0, base=bases)
    for a, b, x, base in zip(first, host, xs, bases):
        assert a.tobytes() == b.tobytes()
        assert a[:, 0].tobytes() == np.ascontiguousarray(base[:, 0]).tobytes()
        if len(x) >= 2:
            assert np.all(a[:, 1] != base[:, 1])
    assert first[2][:, 7].tobytes() == np.ascontiguousarray(bases[2][:, 7]).tobytes()      # the constant column
    for a, base in zip(run(0, 0.0), bases):
        assert a.tobytes() == base.tobytes()
    for a, base in zip(run(cols, 1.0), bases):
        assert a.tobytes() == base.tobytes()
    want, _ = mc.postfilter(xs[3], G, N, 1.0, base=bases[3])
    assert np.all(np.abs(first[3] - want).max(axis=0) <= np.maximum(mc.filter_bounds(xs[3], G, N, 1.0), 0))


def test_status_counts_unusable_bins_and_the_host_entry_raises():
    import torch
    from kwiiyatta_amd.backend import ms
    dev, stream, ctx = _device()
    rng = np.random.RandomState(72)
    xs = [mc.matrix(rng, T, 6) for T in (257, 300, 1)]
    xs[1][:, 4] = -2.5
    G, N = mc.stats_for(xs[0], 512, rng)
    G[1, 3, 1] = np.nan                  # a mean that is not finite
    G[1, 4, 2] = 0.0                     # sigmaG == 0
    N[2, 5, 0] = 1.0                     # n < 2
    G[2, 6, 2] = np.inf                  # sigmaG not finite
    N[3, 7, 2] = -1.0                    # sigmaN not a number
    N[3, 8, 2] = 0.0                     # sigmaN == 0 is usable
    N[5, 9, 1] = 1e4                     # a gain that overflows
    G[4, 10, 1] = np.nan                 # column 4: constant in the second matrix
    want = [mc.postfilter(x, G, N, 1.0) for x in xs]
    assert [w[1] for w in want] == [7, 6, 0]
    d_x = [_up(x, dev) for x in xs]
    d_o = [torch.empty_like(x) for x in d_x]
    status = torch.full((3,), -1, dtype=torch.int32, device=dev)
    with torch.cuda.stream(stream):
        ms.postfilter_batch_dev(ctx, d_x, _up(G, dev), _up(N, dev), 1.0, d_o, status=status)
    stream.synchronize()
    assert status.cpu().tolist() == [7, 6, 0]
    with pytest.raises(ValueError, match=r'13 bin\(s\) of utterance\(s\) \[0, 1\]'):
        ms.check_status(status)
    for (y, _), o, x in zip(want, d_o, xs):
        got = o.cpu().numpy()
        bound = np.maximum(mc.filter_bounds(x, G, N, 1.0), 0)
        finite = np.isfinite(y).all(axis=0)
        assert np.all(np.abs(got - y).max(axis=0, initial=0)[finite] <= bound[finite])
    with pytest.raises(ValueError, match=r'7 bin\(s\) of utterance\(s\) \[0\]'):
        ms.postfilter(xs[0], G, N, 1.0)


def test_a_matrix_longer_than_the_transform_is_rejected_unwritten():
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import ms
    dev, stream, ctx = _device()
    rng = np.random.RandomState(73)
    x = mc.matrix(rng, 513, 4)
    G, N = mc.stats_for(x[:512], 512, rng)
    for call in (lambda: ms.postfilter(x, G, N, 1.0), lambda: ms.log_spectra([x], 512),
                 lambda: ms.postfilter([x[:10], x], G, N, 1.0)):
        with pytest.raises(ValueError, match=r'T = 513.*L = 512'):
            call()
    d_x, d_G, d_N = _up(x, dev), _up(G, dev), _up(N, dev)
    d_o = torch.full_like(d_x, 7.0)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    rc = _lib.lib.kwy_ms_postfilter_dev(ctx.handle, d_x.data_ptr(), 513, 4, 1, 512, d_G.data_ptr(), d_N.data_ptr(), 1.0,
                                        d_x.data_ptr(), d_o.data_ptr(), status.data_ptr())
    stream.synchronize()
    assert rc == _lib.KWY_EINVAL and 'T = 513' in ctx.error() and 'L = 512' in ctx.error()
    assert bool((d_o == 7.0).all()) and status.cpu().tolist() == [-1]
    out = np.full((513, 4), 7.0)
    jobs = _lib.job_array(_lib.MsJob, [(x.ctypes.data, 513, x.ctypes.data, out.ctypes.data)])
    rc = _lib.lib.kwy_ms_postfilter(ctx.handle, jobs, 1, 4, 1, 512, _lib.ptr(G), _lib.ptr(N), 1.0, None)
    assert rc == _lib.KWY_EINVAL and np.all(out == 7.0)
    for bad in (dict(length=500), dict(strength=1.5), dict(first_col=5)):
        with pytest.raises(ValueError):
            ms.postfilter(x[:100], G, N, **dict(dict(strength=1.0), **bad))
    with pytest.raises(ValueError, match='C-contiguous'):
        ms.postfilter(x[:100, ::2], G[:2], N[:2], 1.0)


# ---- converter, batch path, command line --------------------------------------------------------------------------------
NAMES = [f'arctic_a{n:04}' for n in range(1, 10)]
MS_LENGTH = 2048


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """a converter of 2 components trained on CLB -> SLT a0001 .. a0009 with modulation-spectrum and global-variance
    statistics; its model file, and one of the same mixture without the modulation-spectrum statistics"""
    import kwiiyatta_amd as k
    root = tmp_path_factory.mktemp('ms')
    src = root / 'src'
    src.mkdir()
    for name in NAMES:
        shutil.copy(pathlib.Path(CLB_DIR) / f'{name}.wav', src)
    dataset = k.align(k.WavFileDataset(src), k.WavFileDataset(pathlib.Path(SLT_DIR)))
    keys = sorted(dataset.keys())[:len(NAMES)]
    conv = k.MelCepstrumConverter(use_delta=True, components=2, random_state=0)
    np.random.seed(0)
    conv.train(dataset, keys, gv_stats=True, ms_stats=True, ms_length=MS_LENGTH)
    conv.save(root / 'model.npz')
    stats, conv.ms_stats, conv.ms_length = (conv.ms_stats, conv.ms_length), None, None
    conv.save(root / 'plain.npz')
    conv.ms_stats, conv.ms_length = stats
    return root, conv, dataset, keys


def test_trained_statistics_and_the_model_file(trained):
    import kwiiyatta_amd as k
    from kwiiyatta_amd.backend import ms
    from kwiiyatta_amd.converter import mcep
    root, conv, dataset, keys = trained
    assert conv.ms_length == MS_LENGTH and len(conv.ms_stats) == 2
    natural = mcep._target_mel_cepstra(dataset, keys, conv.order, conv.fs)
    assert len(natural) == 9 and all(m.shape[1] == 25 for m in natural)
    converted = [np.ascontiguousarray(conv.convert(r, diff=False).data)
                 for r in mcep._side_mel_cepstra(dataset, keys, conv.order, conv.fs, 0)]
    for got, mats in zip(conv.ms_stats, (converted, natural)):
        assert got.shape == (25, MS_LENGTH // 2 + 1, 3)
        assert got.tobytes() == ms.statistics(mats, MS_LENGTH).tobytes()
        assert np.all(got[:, 1:, 0] == 9) and np.all(got[:, 0] == 0)
        want = mc.statistics(mats, MS_LENGTH)
        scale = np.abs(np.stack([mc.log_spectra(m, MS_LENGTH)[0] for m in mats])).max(axis=0)[:, 1:]
        assert np.all(np.abs(got[:, 1:, 1] - want[:, 1:, 1]) <= 1e-9 * scale)        # (spectra of real trajectories: the
        # kernel's and numpy's differ by the log-spectrum bound, far below this; the bits are checked above)
    # the smoothing this filter is for: converted trajectories move less than natural ones, the more the faster
    fast = slice(MS_LENGTH // 8, None)
    assert (conv.ms_stats[1][1:, fast, 1] - conv.ms_stats[0][1:, fast, 1]).mean() > 1.0
    loaded = k.MelCepstrumConverter(use_delta=True, components=2).load(root / 'model.npz')
    assert loaded.ms_length == MS_LENGTH
    for a, b in zip(loaded.ms_stats, conv.ms_stats):
        assert a.tobytes() == b.tobytes()
    assert loaded.gv_stats.tobytes() == conv.gv_stats.tobytes()
    old = k.MelCepstrumConverter(use_delta=True, components=2).load(root / 'plain.npz')
    assert old.ms_stats is None and old.ms_length is None and old.gv_stats is not None
    mcep_in = k.analyze_wav(pathlib.Path(CLB_DIR) / 'arctic_a0001.wav').mel_cepstrum
    with pytest.raises(ValueError, match='ms_stats=True'):
        old.convert(mcep_in, ms=1.0)
    with pytest.raises(ValueError, match='outside'):
        conv.convert(mcep_in, ms=1.5)
    short = k.MelCepstrumConverter(use_delta=True, components=2).load(root / 'model.npz')
    short.ms_stats = tuple(np.ascontiguousarray(s[:, :257]) for s in short.ms_stats)
    with pytest.raises(ValueError, match=rf'T = {len(mcep_in.data)}.*L = 512'):
        short.convert(mcep_in, ms=1.0)
    fresh = k.MelCepstrumConverter(use_delta=True, components=2, random_state=0)
    with pytest.raises(ValueError, match=r'T = \d+.*L = 512'):
        fresh.train(dataset, keys[:2], ms_stats=True, ms_length=512)
    with pytest.raises(ValueError, match='fewer than two usable'):
        fresh.train(dataset, keys[:1], ms_stats=True, ms_length=MS_LENGTH)


@pytest.mark.parametrize('name', ['arctic_a0001', 'arctic_a0009'])
def test_converter_composition_against_the_yardstick(trained, name):
    import kwiiyatta_amd as k
    _, conv, _, _ = trained
    G, N = conv.ms_stats
    gv = conv.gv_stats
    mcep_in = k.analyze_wav(pathlib.Path(CLB_DIR) / f'{name}.wav').mel_cepstrum
    x = conv.convert(mcep_in).data
    b = conv.convert(mcep_in, diff=True).data
    assert conv.convert(mcep_in, ms=0.0).data.tobytes() == x.tobytes()
    for diff in (False, True):
        base = b if diff else None
        for k_ms in (1.0, 0.5):
            got = conv.convert(mcep_in, ms=k_ms, diff=diff).data
            want, status = mc.postfilter(x, G, N, k_ms, base=base)
            assert status == 0 and got[:, 0].tobytes() == mcep_in.data[:, 0].tobytes()
            bound = mc.filter_bounds(x, G, N, k_ms)
            frac = (np.abs(got - want).max(axis=0)[1:] / bound[1:]).max()
            print(f'{name} diff={diff} ms={k_ms}: worst error / bound = {frac:.3e}')
            assert frac <= 1
        # with the global-variance filter behind it: y = b1 + (r - 1) (p1 - m).  An error B of p1 and b1 comes through
        # as B (1 + |r - 1|) directly and as r B max|p1 - m| / sigma through the ratio (dv <= 2 sigma B, dr / r =
        # dv / 2v); the filter's own rounding is gv_cases.apply_bound
        got = conv.convert(mcep_in, ms=1.0, gv=1.0, diff=diff).data
        want = mc.convert_chain(x, base, G, N, 1.0, gv, 1.0)
        p1, _ = mc.postfilter(x, G, N, 1.0)
        r = np.concatenate(([1.0], gc.ratios(p1, gv)))
        dev = np.abs(p1 - p1.mean(axis=0)).max(axis=0) / p1.std(axis=0)
        bound = mc.filter_bounds(x, G, N, 1.0) * (1 + np.abs(r - 1) + r * dev) \
            + np.array([gc.apply_bound(p1, r[d], d) for d in range(25)])
        frac = (np.abs(got - want).max(axis=0)[1:] / bound[1:]).max()
        print(f'{name} diff={diff} ms=1 gv=1: worst error / bound = {frac:.3e}')
        assert frac <= 1 and got[:, 0].tobytes() == mcep_in.data[:, 0].tobytes()
        if not diff:
            for d in range(1, 25):
                assert abs(np.var(got[:, d]) / gv[d] - 1) <= gc.variance_claim_bound(p1, d)
    # what the filter is for: the spectrum of the filtered trajectories is nearer the natural mean than the plain one's
    y = conv.convert(mcep_in, ms=1.0).data
    far = [np.abs(mc.log_spectra(m, MS_LENGTH)[0][1:, 1:] - N[1:, 1:, 1]).mean() for m in (x, y)]
    print(f'{name}: mean |s - muN| plain {far[0]:.3f}, filtered {far[1]:.3f}')
    assert far[1] < far[0]


def test_batch_path_equals_the_filter_by_hand(trained):
    import torch
    import kwiiyatta_amd as k
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd.backend import ms
    root, conv, _, _ = trained
    waves = [k.analyze_wav(root / 'src' / f'{n}.wav').wavdata.data for n in NAMES[:3]]
    dev = torch.device('cuda', 0)
    gmm = conv.gmm
    dg = corpus.DeviceGMM(gmm.weights_, gmm.means_, gmm.covariances_, dev)
    ls = corpus._Lockstep(0)
    options = dict(gmm=dg, order=conv.order, frame_period=5.0, pcm=True, diff=True)
    filtered = corpus.ConvertWave(ls, 16000, waves, ms_stats=conv.ms_stats, ms_length=MS_LENGTH, ms_strength=1.0, **options)
    filtered.run()
    plain = corpus.ConvertWave(ls, 16000, waves, **options)
    plain.run()
    ls.sync()
    assert filtered.ms_status.cpu().tolist() == [0, 0, 0] and plain.ms_status is None
    rows = corpus.Ragged(plain.T)
    p, b = rows.views(plain.mc_conv.clone()), rows.views(plain.mc_diff.clone())
    d_G, d_N = (_up(s, dev) for s in conv.ms_stats)
    torch.cuda.synchronize()
    with torch.cuda.stream(ls.main):
        ms.postfilter_batch_dev(ls.ctx, p, d_G, d_N, 1.0, b, bases=b)
        ms.postfilter_batch_dev(ls.ctx, p, d_G, d_N, 1.0, p)
    ls.sync()
    for i, (got_p, got_b) in enumerate(zip(rows.views(filtered.mc_conv), rows.views(filtered.mc_diff))):
        assert got_p.cpu().numpy().tobytes() == p[i].cpu().numpy().tobytes(), i
        assert got_b.cpu().numpy().tobytes() == b[i].cpu().numpy().tobytes(), i
        assert got_p.cpu().numpy().tobytes() != rows.views(plain.mc_conv)[i].cpu().numpy().tobytes()
    opts = dict(order=conv.order, frame_period=5.0, pcm=True, diff=True)
    res = corpus.convert_batch(waves, 16000, gmm, ms_stats=conv.ms_stats, ms_length=MS_LENGTH, ms_strength=1.0, **opts)
    for i in range(3):
        assert res[1][i].cpu().numpy().tobytes() == filtered.pcm[i].cpu().numpy().tobytes()
        assert res[3][i].cpu().numpy().tobytes() == filtered.pcm_diff[i].cpu().numpy().tobytes()
    res0 = corpus.convert_batch(waves, 16000, gmm, ms_stats=conv.ms_stats, ms_strength=0.0, **opts)
    for i in range(3):
        assert res0[1][i].cpu().numpy().tobytes() == plain.pcm[i].cpu().numpy().tobytes()
    with pytest.raises(ValueError, match='needs ms_stats'):
        corpus.convert_batch(waves, 16000, gmm, ms_strength=1.0, **opts)
    short = tuple(np.ascontiguousarray(s[:, :257]) for s in conv.ms_stats)
    with pytest.raises(ValueError, match=r'T = \d+.*L = 512'):
        corpus.convert_batch(waves, 16000, gmm, ms_stats=short, ms_strength=1.0, **opts)
    bad = tuple(s.copy() for s in conv.ms_stats)
    bad[0][5, 9, 2] = 0.0
    with pytest.raises(ValueError, match=r'3 bin\(s\) of utterance\(s\) \[0, 1, 2\]'):
        corpus.convert_batch(waves, 16000, gmm, ms_stats=bad, ms_strength=1.0, **opts)
    triples = []
    for n in NAMES[:2]:
        a = k.analyze_wav(root / 'src' / f'{n}.wav')
        f0, t = a._frame_grid()
        triples.append((np.ascontiguousarray(a.wavdata.data), np.ascontiguousarray(f0), np.ascontiguousarray(t)))
    with pytest.raises(ValueError, match='lockstep driver'):
        corpus.convert_batch(triples, 16000, gmm, driver='streams', streams=2, ms_stats=conv.ms_stats, ms_strength=1.0)


def test_convert_voice_ms(trained, capsys):
    import kwiiyatta_amd.convert_voice as cv
    from scipy.io import wavfile as sio
    root, _, _, _ = trained
    inputs = [str(root / 'src' / f'{n}.wav') for n in NAMES[:2]]
    common = ['--converter-components', '2', '--converter-model', str(root / 'model.npz')] + inputs
    _run_cli(cv.main, ['--result-dir', str(root / 'plain')] + common)
    _run_cli(cv.main, ['--result-dir', str(root / 'ms'), '--ms'] + common)
    _run_cli(cv.main, ['--result-dir', str(root / 'zero'), '--ms', '0'] + common)
    _run_cli(cv.main, ['--result-dir', str(root / 'batch'), '--batch', '--ms'] + common)
    _run_cli(cv.main, ['--result-dir', str(root / 'both'), '--ms', '0.5', '--gv', '--batch'] + common)
    _run_cli(cv.main, ['--result-dir', str(root / 'both1'), '--ms', '0.5', '--gv'] + common)
    for name in NAMES[:2]:
        for kind in ('synth', 'diff'):
            where = (name, kind)
            plain = (root / 'plain' / f'{name}.{kind}.wav').read_bytes()
            assert (root / 'ms' / f'{name}.{kind}.wav').read_bytes() != plain, where
            assert (root / 'zero' / f'{name}.{kind}.wav').read_bytes() == plain, where
            for one, batch in (('ms', 'batch'), ('both1', 'both')):
                _, a = sio.read(root / one / f'{name}.{kind}.wav')
                _, c = sio.read(root / batch / f'{name}.{kind}.wav')
                assert a.shape == c.shape and np.abs(a.astype(np.int64) - c.astype(np.int64)).max() <= 1, where
    capsys.readouterr()
    with pytest.raises(SystemExit):
        _run_cli(cv.main, ['--result-dir', str(root / 'none'), '--ms', '--converter-components', '2', '--converter-model',
                           str(root / 'plain.npz')] + inputs)
    assert 'no modulation spectrum statistics; retrain it with --ms' in capsys.readouterr().err
