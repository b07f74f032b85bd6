"""Global-variance postfilter on the MI355X: the column moment, statistic and filter kernels of kwy_gv.hip through the
C ABI against their numpy statement (tests/gv_cases.py), their determinism and input edges, the converter and the
training-matrix path against the API path, and what `convert_voice --gv` writes."""
import pathlib
import shutil
import sys

import numpy as np
import pytest

import gv_cases as gc
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
    stream = torch.cuda.Stream(device=dev)       # (a stream of its own: the context would make one for the null stream)
    return dev, stream, _lib.Context(0, stream=stream.cuda_stream)


# ---- moments and the statistic ---------------------------------------------------------------------------------------
def _matrices(seed, cols):
    rng = np.random.RandomState(seed)
    mats = [gc.matrix(rng, T, cols) for T in gc.LENGTHS]
    for m in mats[::3]:
        m[:, cols - 1] = 0.1                                 # a constant column (T copies of 0.1 do not add up to T / 10)
    return mats


def test_moments_against_numpy():
    from kwiiyatta_amd.backend import gv as gvf
    worst_mean = worst_m2 = 0.0
    for cols in gc.COLS:
        mats = _matrices(cols, cols)
        got = gvf.column_moments(mats)
        assert got.shape == (len(mats), cols, 3)
        for x, g in zip(mats, got):
            want = gc.column_moments(x)
            for d in range(cols):
                where = (len(x), cols, d)
                mean_bound, m2_rel = gc.moments_bounds(x, d)
                assert g[d, 0] == len(x), where
                e_mean, e_m2 = abs(g[d, 1] - want[d, 1]), abs(g[d, 2] - want[d, 2])
                worst_mean = max(worst_mean, e_mean / mean_bound)
                assert e_mean <= mean_bound, where
                assert e_m2 <= m2_rel * want[d, 2] + 1e-300, where
                if want[d, 2] > 0:
                    worst_m2 = max(worst_m2, e_m2 / (m2_rel * want[d, 2]))
                if np.all(x[:, d] == x[0, d]):
                    assert g[d, 1] == x[0, d] and g[d, 2] == 0.0, where
    print(f'column moments: worst error / bound: mean {worst_mean:.4f}, M2 {worst_m2:.4f}')
    # no rows: zeros; the statistic skips such a matrix
    empty = gvf.column_moments([np.zeros((0, 25)), mats_25()[3]])
    assert not empty[0].any()
    assert gvf.gv_from_moments(empty).tobytes() == gvf.gv_from_moments(empty[1:]).tobytes()
    with pytest.raises(ValueError, match='no utterance has frames'):
        gvf.gv_from_moments(empty[:1])


def mats_25(seed=11):
    return _matrices(seed, 25)


def test_statistic_against_numpy():
    from kwiiyatta_amd.backend import gv as gvf
    for cols in gc.COLS:
        mats = _matrices(20 + cols, cols)
        m = gvf.column_moments(mats)
        gv = gvf.gv_from_moments(m)
        assert gv.tobytes() == gc.gv_statistic(m).tobytes(), cols            # the same fold of the same moments
        want = gc.gv_statistic([gc.column_moments(x) for x in mats])
        # (4 T u per utterance variance, as for M2, and the roundings of the quotients and of the fold)
        assert np.all(np.abs(gv - want) <= (4 * max(gc.LENGTHS) + 2 * len(mats) + 4) * gc.U * want + 1e-300), cols


def test_moments_bit_reproducible_and_group_independent():
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    from kwiiyatta_amd.backend import gv as gvf
    mats = mats_25(1) + mats_25(2) + mats_25(3)            # 39 matrices: more than one launch group
    a = gvf.column_moments(mats)
    b = gvf.column_moments(mats)
    assert a.tobytes() == b.tobytes()
    stat = gvf.gv_from_moments(a)
    for groups in (1, 3, 7):
        bounds = np.linspace(0, len(mats), groups + 1).astype(int)
        parts = [gvf.column_moments(mats[lo:hi]) for lo, hi in zip(bounds[:-1], bounds[1:])]
        assert np.concatenate(parts).tobytes() == a.tobytes(), groups
        assert gvf.gv_from_moments(np.concatenate(parts)).tobytes() == stat.tobytes(), groups
    # the device entries: batched in groups of 5, and one matrix at a time
    dev, stream, ctx = _device()
    d_mats = [torch.from_numpy(m).to(dev) for m in mats]
    d_m = torch.empty((len(mats), 25, 3), dtype=torch.float64, device=dev)
    d_one = torch.empty_like(d_m)
    d_gv = torch.empty(25, dtype=torch.float64, device=dev)
    for lo in range(0, len(mats), 5):
        gvf.column_moments_batch_dev(ctx, d_mats[lo:lo + 5], d_m[lo:lo + 5])
    for i, m in enumerate(d_mats):
        _lib.check(ctx, lib.kwy_column_moments_dev(ctx.handle, m.data_ptr(), m.shape[0], 25, d_one[i].data_ptr()))
    gvf.gv_from_moments_dev(ctx, d_m, d_gv)
    stream.synchronize()
    assert d_m.cpu().numpy().tobytes() == a.tobytes()
    assert d_one.cpu().numpy().tobytes() == a.tobytes()
    assert d_gv.cpu().numpy().tobytes() == stat.tobytes()


# ---- the filter ------------------------------------------------------------------------------------------------------
def _filter_cases(seed, cols=25, lengths=gc.LENGTHS):
    rng = np.random.RandomState(seed)
    for T in lengths:
        x = gc.matrix(rng, T, cols)
        r = rng.uniform(0.5, 3.0, size=cols - 1)
        yield x, gc.gv_for_ratios(x, r), r


@pytest.mark.parametrize('s', [0.25, 0.5, 1.0])
def test_filter_against_numpy(s):
    from kwiiyatta_amd.backend import gv as gvf
    worst = worst_var = 0.0
    for cols in (25, 41, 64):
        cases = list(_filter_cases(30 + cols, cols))
        got = gvf.postfilter([x for x, _, _ in cases[:3]], cases[0][1], s)       # (a list: one call)
        assert len(got) == 3
        for x, gv, r in cases:
            y = gvf.postfilter(x, gv, s)
            want, status = gc.postfilter(x, gv, s)
            assert status == 0 and y.shape == x.shape and y is not x
            assert y[:, 0].tobytes() == x[:, 0].tobytes()
            for d in range(1, cols):
                err, bound = np.abs(y[:, d] - want[:, d]).max(), gc.apply_bound(x, r[d - 1], d)
                assert err <= bound, (len(x), cols, d, err, bound)
                worst = max(worst, err / bound) if bound else worst
                if s == 1.0 and len(x) >= 2:
                    verr, vbound = abs(np.var(y[:, d]) / gv[d] - 1), gc.variance_claim_bound(x, d)
                    assert verr <= vbound, (len(x), cols, d, verr, vbound)
                    worst_var = max(worst_var, verr / vbound)
    print(f'filter s={s}: worst error / bound {worst:.4f}; variance claim {worst_var:.4f}')


def test_strength_zero_in_place_and_the_differential_form():
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    from kwiiyatta_amd.backend import gv as gvf
    cases = list(_filter_cases(40, lengths=(1, 2, 65, 256, 1000, 5000)))
    rng = np.random.RandomState(41)
    for x, gv, _ in cases:
        x[0, 3] = -0.0
        assert gvf.postfilter(x, gv, 0.0).tobytes() == x.tobytes()
        base = rng.standard_normal(x.shape)
        assert gvf.postfilter(x, gv, 0.0, base=base).tobytes() == base.tobytes()
    dev, stream, ctx = _device()
    for s in (0.5, 1.0):
        xs = [torch.from_numpy(x).to(dev) for x, _, _ in cases]
        bases = [torch.from_numpy(rng.standard_normal(x.shape) * np.abs(x).max(axis=0) * 0.1).to(dev) for x, _, _ in cases]
        gv = cases[2][1]
        d_gv = torch.from_numpy(gv).to(dev)
        moments = torch.empty((len(xs), 25, 3), dtype=torch.float64, device=dev)
        gvf.column_moments_batch_dev(ctx, xs, moments)
        outs = [torch.empty_like(x) for x in xs]
        status = torch.full((len(xs),), -1, dtype=torch.int32, device=dev)
        gvf.postfilter_batch_dev(ctx, xs, moments, d_gv, s, outs, status=status)
        # the differential form out of place, then in place; one matrix through the single entry; the plain form in place
        d_outs = [torch.empty_like(x) for x in xs]
        gvf.postfilter_batch_dev(ctx, xs, moments, d_gv, s, d_outs, bases=bases)
        d_in = [b.clone() for b in bases]
        gvf.postfilter_batch_dev(ctx, xs, moments, d_gv, s, d_in, bases=d_in)
        one = torch.empty_like(xs[4])
        _lib.check(ctx, lib.kwy_gv_postfilter_dev(ctx.handle, xs[4].data_ptr(), xs[4].shape[0], 25, 1,
                                                  moments[4].data_ptr(), d_gv.data_ptr(), s, bases[4].data_ptr(),
                                                  one.data_ptr(), None))
        in_place = [x.clone() for x in xs]
        gvf.postfilter_batch_dev(ctx, in_place, moments, d_gv, s, in_place)
        stream.synchronize()
        assert status.cpu().tolist() == [0] * len(xs)
        assert one.cpu().numpy().tobytes() == d_outs[4].cpu().numpy().tobytes()
        for (x, _, _), b, o, do, di, ip in zip(cases, bases, outs, d_outs, d_in, in_place):
            host = gvf.postfilter(x, gv, s)
            assert o.cpu().numpy().tobytes() == host.tobytes() and ip.cpu().numpy().tobytes() == host.tobytes()
            host_d = gvf.postfilter(x, gv, s, base=b.cpu().numpy())
            assert do.cpu().numpy().tobytes() == host_d.tobytes() and di.cpu().numpy().tobytes() == host_d.tobytes()
            want, _ = gc.postfilter(x, gv, s, base=b.cpu().numpy())
            assert host_d[:, 0].tobytes() == want[:, 0].tobytes()
            r = gc.ratios(x, gv)
            for d in range(1, 25):
                if len(x) >= 2:
                    assert np.abs(host_d[:, d] - want[:, d]).max() <= gc.apply_bound(x, r[d - 1], d), (len(x), d)


def test_status_counts_unusable_coefficients_and_the_host_entry_raises():
    import torch
    from kwiiyatta_amd.backend import gv as gvf
    rng = np.random.RandomState(50)
    good = gc.matrix(rng, 200, 25)
    nan3 = good.copy()
    nan3[17, 3] = np.nan
    flat = good.copy()
    flat[:, 6] = 0.1
    one = gc.matrix(rng, 1, 25)
    gv = np.full(25, 2.0)
    # zero variance and a single frame: copied, no status
    assert gvf.postfilter(flat, gv)[:, 6].tobytes() == flat[:, 6].tobytes()
    assert gvf.postfilter(one, gv).tobytes() == one.tobytes()
    # column 0 is never examined
    c0 = good.copy()
    c0[5, 0] = np.nan
    gv0 = gv.copy()
    gv0[0] = -1.0
    assert gvf.postfilter(c0, gv0)[:, 0].tobytes() == c0[:, 0].tobytes()
    with pytest.raises(ValueError, match=r'1 coefficient\(s\) of utterance\(s\) \[1\]'):
        gvf.postfilter([good, nan3], gv)
    bad_gv = gv.copy()
    bad_gv[[5, 6, 7]] = 0.0, -1.0, np.inf
    with pytest.raises(ValueError, match=r'6 coefficient\(s\) of utterance\(s\) \[0, 1\]'):
        gvf.postfilter([good, flat], bad_gv)
    for s in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError, match=r'outside \[0, 1\]'):
            gvf.postfilter(good, gv, s)
    with pytest.raises(ValueError, match='C-contiguous'):
        gvf.postfilter(good[:, ::2], gv[::2])
    with pytest.raises(ValueError, match='dtype mismatch'):
        gvf.postfilter(good.astype(np.float32), gv)
    with pytest.raises(ValueError, match='C-contiguous'):
        gvf.column_moments([good[::2, ::2]])
    with pytest.raises(ValueError, match='dtype mismatch'):
        gvf.column_moments([good.astype(np.float32)])
    with pytest.raises(ValueError, match='columns'):
        gvf.column_moments([np.zeros((10, 65))])
    with pytest.raises(ValueError, match='one value per column'):
        gvf.postfilter(good, gv[:24])
    # the device entry leaves the words to be read back; the coefficients come back as they went in
    dev, stream, ctx = _device()
    mats = [good, nan3, flat, one]
    xs = [torch.from_numpy(m).to(dev) for m in mats]
    moments = torch.empty((4, 25, 3), dtype=torch.float64, device=dev)
    gvf.column_moments_batch_dev(ctx, xs, moments)
    for vec, words in ((gv, [0, 1, 0, 0]), (bad_gv, [3, 4, 3, 3])):
        outs = [torch.empty_like(x) for x in xs]
        status = torch.full((4,), -1, dtype=torch.int32, device=dev)
        gvf.postfilter_batch_dev(ctx, xs, moments, torch.from_numpy(vec).to(dev), 1.0, outs, status=status)
        stream.synchronize()
        assert status.cpu().tolist() == words
        want, _ = gc.postfilter(nan3, vec, 1.0)
        got = outs[1].cpu().numpy()
        for d in (3, 5, 6, 7) if vec is bad_gv else (3,):
            assert got[:, d].tobytes() == nan3[:, d].tobytes(), d
        assert np.abs(got[:, 9] - want[:, 9]).max() <= gc.apply_bound(good, gc.ratios(good, vec)[8], 9)
        with pytest.raises(ValueError, match='unfiltered'):
            gvf.check_status(status)


# ---- converter, training matrix, command line ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """convert_voice trained on 4 CLB -> SLT files with 2 components and seed 0, without and with --gv; the model file
    of the second"""
    import kwiiyatta_amd.convert_voice as cv
    root = tmp_path_factory.mktemp('gv')
    src = root / 'src'
    src.mkdir()
    for n in range(1, 5):
        shutil.copy(pathlib.Path(CLB_DIR) / f'arctic_a{n:04}.wav', src)
    inputs = [str(src / f'arctic_a{n:04}.wav') for n in range(1, 5)]
    common = ['--source', str(src), '--target', SLT_DIR, '--converter-seed', '0', '--converter-components', '2',
              '--max-files', '4']
    np.random.seed(0)
    _run_cli(cv.main, common + ['--result-dir', str(root / 'plain')] + inputs)
    np.random.seed(0)
    _run_cli(cv.main, common + ['--result-dir', str(root / 'gv'), '--gv', '--converter-model', str(root / 'model.npz')]
             + inputs)
    return root, inputs, common


def _names():
    return [f'arctic_a{n:04}' for n in range(1, 5)]


def _target_mel_cepstra():
    """the trimmed target mel-cepstra of the API path"""
    import kwiiyatta_amd as k
    from kwiiyatta_amd.converter.dataset import trim_zeros_frames
    ds = k.WavFileDataset(pathlib.Path(SLT_DIR))
    out = []
    for name in _names():
        f = ds[pathlib.Path(f'{name}.wav')]
        out.append(np.ascontiguousarray(f.mel_cepstrum.data[:len(trim_zeros_frames(f.spectrum_envelope))]))
    return out


def _gv_bound(mats, want):
    """the project's 1e-9 max|mc| agreement between mel-cepstrum paths carried through a variance"""
    return 4e-9 * max(np.abs(m).max() for m in mats) * np.sqrt(want)


def test_trained_statistic_equals_the_numpy_statement(trained):
    import kwiiyatta_amd as k
    root, _, _ = trained
    conv = k.MelCepstrumConverter(components=2).load(root / 'model.npz')
    assert conv.gv_stats is not None and conv.gv_stats.shape == (25,) and conv.f0_stats is None
    mats = _target_mel_cepstra()
    want = gc.gv_statistic([gc.column_moments(m) for m in mats])
    err, bound = np.abs(conv.gv_stats - want), _gv_bound(mats, want)
    print(f'gv statistic: worst error / bound = {(err / bound).max():.3e}')
    assert np.all(err <= bound), (err / bound).max()
    plain = k.MelCepstrumConverter(use_delta=True, components=2)
    assert plain.gv_stats is None


def test_training_matrix_statistic_equals_the_converters(trained):
    import kwiiyatta_amd as k
    from kwiiyatta_amd import corpus
    root, _, _ = trained
    conv = k.MelCepstrumConverter(components=2).load(root / 'model.npz')
    mats = _target_mel_cepstra()
    want = gc.gv_statistic([gc.column_moments(m) for m in mats])
    pairs = []
    for name in _names():
        pair = []
        for d in (root / 'src', pathlib.Path(SLT_DIR)):
            a = k.analyze_wav(d / f'{name}.wav')
            f0, t = a._frame_grid()                       # (DIO + StoneMask, as the training path analyses)
            pair.append((np.ascontiguousarray(a.wavdata.data), np.ascontiguousarray(f0), np.ascontiguousarray(t)))
        pairs.append(tuple(pair))
    for kw in (dict(driver='lockstep', wave_pairs=3), dict(driver='streams', streams=2)):
        np.random.seed(0)
        X, frames, gv = corpus.build_training_matrix(pairs, 16000, gv_moments=True, **kw)
        np.random.seed(0)
        X0, frames0 = corpus.build_training_matrix(pairs, 16000, **kw)
        assert frames == frames0 and X.cpu().numpy().tobytes() == X0.cpu().numpy().tobytes()
        assert gv.shape == (25,) and gv.dtype == np.float64
        assert np.all(np.abs(gv - want) <= _gv_bound(mats, want)), kw
        assert np.all(np.abs(gv - conv.gv_stats) <= _gv_bound(mats, want)), kw
    np.random.seed(0)
    X, frames, f0m, gv2 = corpus.build_training_matrix(pairs, 16000, f0_moments=True, gv_moments=True, **kw)
    assert f0m.shape == (2, 3) and gv2.tobytes() == gv.tobytes() and X.cpu().numpy().tobytes() == X0.cpu().numpy().tobytes()


def test_converter_gv_reaches_the_target_variance(trained):
    import kwiiyatta_amd as k
    root, _, _ = trained
    conv = k.MelCepstrumConverter(use_delta=True, components=2).load(root / 'model.npz')
    gv = conv.gv_stats
    for n in (1, 2, 3, 4, 8, 9):
        mcep = k.analyze_wav(pathlib.Path(CLB_DIR) / f'arctic_a{n:04}.wav').mel_cepstrum
        x = conv.convert(mcep).data
        assert conv.convert(mcep, gv=0.0).data.tobytes() == x.tobytes()
        r = gc.ratios(x, gv)
        print(f'arctic_a{n:04}: frames {len(x)} median r {np.median(r):.3f} min {r.min():.3f} max {r.max():.3f} '
              f'r > 1: {(r > 1).sum()} / {len(r)}')
        assert np.median(r) > 1.25 and (r > 1).sum() >= 20, n
        y = conv.convert(mcep, gv=1.0).data
        assert y[:, 0].tobytes() == x[:, 0].tobytes() == mcep.data[:, 0].tobytes()
        for d in range(1, 25):
            assert abs(np.var(y[:, d]) / gv[d] - 1) <= gc.variance_claim_bound(x, d), (n, d)
        # half strength, and the differential form: the plain filter's change added to the differential conversion
        half, _ = gc.postfilter(x, gv, 0.5)
        got = conv.convert(mcep, gv=0.5).data
        for d in range(1, 25):
            assert np.abs(got[:, d] - half[:, d]).max() <= gc.apply_bound(x, r[d - 1], d), (n, d)
        d_conv = conv.convert(mcep, diff=True).data
        d_gv = conv.convert(mcep, gv=1.0, diff=True).data
        assert d_gv[:, 0].tobytes() == d_conv[:, 0].tobytes()
        # (the same moments and ratio on the device, so only the roundings of y, of y - x and of either sum differ)
        bound = 4 * gc.U * (np.abs(y).max(axis=0) + np.abs(x).max(axis=0) + np.abs(d_gv).max(axis=0))
        assert np.all(np.abs(d_gv - (d_conv + (y - x))).max(axis=0) <= bound), n
    fresh = k.MelCepstrumConverter(use_delta=True, components=2)
    fresh.load(root / 'model.npz').gv_stats = None
    with pytest.raises(ValueError, match='gv_stats=True'):
        fresh.convert(mcep, gv=1.0)


def test_convert_voice_gv(trained):
    import kwiiyatta_amd.convert_voice as cv
    from scipy.io import wavfile as sio
    root, inputs, common = trained
    model = ['--converter-model', str(root / 'model.npz')]
    _run_cli(cv.main, ['--result-dir', str(root / 'again'), '--gv'] + model + inputs)
    _run_cli(cv.main, ['--result-dir', str(root / 'zero'), '--gv', '0'] + model + inputs)
    _run_cli(cv.main, ['--result-dir', str(root / 'batch'), '--gv', '--batch'] + model + inputs)
    np.random.seed(0)
    _run_cli(cv.main, common + ['--result-dir', str(root / 'pitch'), '--gv', '--convert-f0', '--transpose-key', '2']
             + inputs)
    for name in _names():
        for kind in ('synth', 'diff'):
            where = (name, kind)
            plain = (root / 'plain' / f'{name}.{kind}.wav').read_bytes()
            first = (root / 'gv' / f'{name}.{kind}.wav').read_bytes()
            assert plain != first, where                                       # the filter changes both outputs
            assert (root / 'again' / f'{name}.{kind}.wav').read_bytes() == first, where
            assert (root / 'zero' / f'{name}.{kind}.wav').read_bytes() == plain, where
            _, a = sio.read(root / 'gv' / f'{name}.{kind}.wav')
            _, c = sio.read(root / 'batch' / f'{name}.{kind}.wav')
            assert a.shape == c.shape and np.abs(a.astype(np.int64) - c.astype(np.int64)).max() <= 1, where
            pitched = (root / 'pitch' / f'{name}.{kind}.wav').read_bytes()
            assert (pitched == first) == (kind == 'diff'), where


def test_convert_batch_without_the_filter_changes_nothing(trained):
    import kwiiyatta_amd as k
    from kwiiyatta_amd import corpus
    root, inputs, _ = trained
    conv = k.MelCepstrumConverter(components=2).load(root / 'model.npz')
    waves = [k.analyze_wav(p).wavdata.data for p in inputs[:2]]
    opts = dict(order=conv.order, frame_period=5.0, pcm=True, diff=True)
    r0 = corpus.convert_batch(waves, 16000, conv.gmm, **opts)
    r1 = corpus.convert_batch(waves, 16000, conv.gmm, gv_stats=None, gv_strength=0.0, **opts)
    r2 = corpus.convert_batch(waves, 16000, conv.gmm, gv_stats=conv.gv_stats, gv_strength=0.0, **opts)
    for other in (r1, r2):
        for xs, ys in zip(r0, other):
            for a, b in zip(xs, ys):
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    r3 = corpus.convert_batch(waves, 16000, conv.gmm, gv_stats=conv.gv_stats, gv_strength=1.0, **opts)
    for xs, ys in zip(r0, r3):
        for a, b in zip(xs, ys):
            assert a.cpu().numpy().tobytes() != b.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match='needs gv_stats'):
        corpus.convert_batch(waves, 16000, conv.gmm, gv_strength=1.0, **opts)
    bad = conv.gv_stats.copy()
    bad[5] = 0.0
    with pytest.raises(ValueError, match=r'2 coefficient\(s\) of utterance\(s\) \[0, 1\]'):
        corpus.convert_batch(waves, 16000, conv.gmm, gv_stats=bad, gv_strength=1.0, **opts)
    triples = []
    for p in inputs[:2]:
        a = k.analyze_wav(p)
        f0, t = a._frame_grid()
        triples.append((np.ascontiguousarray(a.wavdata.data), np.ascontiguousarray(f0), np.ascontiguousarray(t)))
    with pytest.raises(ValueError, match='lockstep driver'):
        corpus.convert_batch(triples, 16000, conv.gmm, driver='streams', streams=2, gv_stats=conv.gv_stats,
                             gv_strength=1.0)
