"""f0 conversion and key transposition on the MI355X: the log-f0 moment, merge and map kernels against numpy, their
determinism, the batch path against the per-file path, and the pitch of what the two CLIs write."""
import pathlib
import shutil
import sys

import numpy as np
import pytest

from conftest import CLB_DIR, CLB_WAV, CLB_WAV2, SLT_DIR

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 1000, 2049, 4097, 5000)


def _run_cli(main, argv):
    old = sys.argv
    sys.argv = ['prog'] + argv
    try:
        main()
    finally:
        sys.argv = old


def _tracks(seed=0):
    rng = np.random.RandomState(seed)
    out = []
    for n in LENGTHS:
        f0 = rng.uniform(70.0, 500.0, size=n)
        f0[rng.uniform(size=n) < 0.3] = 0.0
        out.append(f0)
    out.append(np.zeros(300))                              # all unvoiced
    single = np.zeros(777)
    single[411] = 187.5
    out.append(single)                                     # one voiced frame
    return out


def _numpy_moments(f0):
    v = np.log(f0[f0 > 0])
    if len(v) == 0:
        return 0.0, 0.0, 0.0
    mean = v.mean()
    return float(len(v)), mean, float(((v - mean) ** 2).sum())


def test_moments_against_numpy():
    from kwiiyatta_amd.backend import f0 as f0map
    tracks = _tracks()
    got = f0map.logf0_moments(tracks)
    assert got.shape == (len(tracks), 3)
    for f0, (n, mean, m2) in zip(tracks, got):
        wn, wmean, wm2 = _numpy_moments(f0)
        assert n == wn, len(f0)
        assert mean == pytest.approx(wmean, rel=1e-13, abs=0), len(f0)
        assert m2 == pytest.approx(wm2, rel=1e-13, abs=1e-300), len(f0)
    assert tuple(got[-2]) == (0.0, 0.0, 0.0)
    assert got[-1][0] == 1.0 and got[-1][2] == 0.0 and got[-1][1] == pytest.approx(np.log(187.5), rel=1e-15)


def test_moments_bit_reproducible_and_group_independent():
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import f0 as f0map
    tracks = _tracks(1) + _tracks(2)
    a = f0map.logf0_moments(tracks)
    b = f0map.logf0_moments(tracks)
    assert np.array_equal(a, b)
    merged = f0map.merge_moments(a)
    for groups in (1, 3, 7):
        bounds = np.linspace(0, len(tracks), groups + 1).astype(int)
        parts = [f0map.logf0_moments(tracks[lo:hi]) for lo, hi in zip(bounds[:-1], bounds[1:])]
        assert np.array_equal(np.concatenate(parts), a), groups
        assert np.array_equal(f0map.merge_moments(np.concatenate(parts)), merged), groups
    # the device entries: the same triples, the same merge
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev)
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    d_tracks = [torch.from_numpy(f).to(dev) for f in tracks]
    d_m = torch.empty((len(tracks), 3), dtype=torch.float64, device=dev)
    d_out = torch.empty(3, dtype=torch.float64, device=dev)
    for lo in range(0, len(tracks), 5):
        f0map.logf0_moments_batch_dev(ctx, d_tracks[lo:lo + 5], d_m[lo:lo + 5])
    f0map.merge_moments_dev(ctx, d_m, d_out)
    stream.synchronize()
    assert np.array_equal(d_m.cpu().numpy(), a)
    assert np.array_equal(d_out.cpu().numpy(), merged)
    # Chan's merge agrees with the moments of the concatenation
    whole = _numpy_moments(np.concatenate(tracks))
    assert merged[0] == whole[0]
    assert merged[1] == pytest.approx(whole[1], rel=1e-13) and merged[2] == pytest.approx(whole[2], rel=1e-12)


def test_transpose_only_map_is_the_dialogs_product():
    from kwiiyatta_amd.backend import f0 as f0map
    f0 = np.concatenate(_tracks(4))
    for key in list(range(-24, 25)) + [0.37, -7.5]:
        got = f0map.map_f0(f0, 48000, key=key)
        assert np.array_equal(got, f0 * (2.0 ** (key / 12))), key
    same = f0map.map_f0(f0, 48000, key=0.0)
    assert np.array_equal(same, f0) and same is not f0


def _clb_training_f0():
    import kwiiyatta_amd as k
    return [np.ascontiguousarray(k.analyze_wav(str(pathlib.Path(CLB_DIR) / f'arctic_a{n:04}.wav')).f0)
            for n in range(1, 5)]


def test_stats_map_moves_the_source_onto_the_target_statistics():
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import f0 as f0map
    src = _clb_training_f0()
    m_src = f0map.merge_moments(f0map.logf0_moments(src))
    stats = (m_src[1], np.sqrt(m_src[2] / m_src[0]), np.log(190.0), 0.12)
    mapped = [f0map.map_f0(f, 16000, stats=stats) for f in src]
    for f, g in zip(src, mapped):
        assert np.array_equal(g == 0, f == 0)                 # unvoiced frames exactly 0, voiced stay voiced
        assert np.all(g[f == 0] == 0.0)
        want = np.exp((np.log(f[f > 0]) - stats[0]) * stats[3] / stats[1] + stats[2])
        assert np.allclose(g[f > 0], want, rtol=1e-13, atol=0)
    v = np.log(np.concatenate([g[g > 0] for g in mapped]))
    assert abs(v.mean() - stats[2]) < 1e-12
    assert abs(v.std() - stats[3]) < 1e-12
    n, mean, m2 = f0map.merge_moments(f0map.logf0_moments(mapped))
    assert abs(mean - stats[2]) < 1e-12 and abs(np.sqrt(m2 / n) - stats[3]) < 1e-12
    # the device form: batch == single, in place == out of place; with a key on top
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev)
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    d_stats = torch.tensor(stats, dtype=torch.float64, device=dev)
    d_in = [torch.from_numpy(f).to(dev) for f in src]
    d_out = [torch.empty_like(t) for t in d_in]
    d_inplace = [t.clone() for t in d_in]
    status = torch.full((len(src),), -1, dtype=torch.int32, device=dev)
    f0map.map_f0_batch_dev(ctx, d_in, d_out, 16000, stats=d_stats, key=3.0, status=status)
    f0map.map_f0_batch_dev(ctx, d_inplace, d_inplace, 16000, stats=d_stats, key=3.0)
    stream.synchronize()
    assert status.cpu().tolist() == [0] * len(src)
    for f, a, b in zip(src, d_out, d_inplace):
        single = f0map.map_f0(f, 16000, stats=stats, key=3.0)
        assert np.array_equal(a.cpu().numpy(), single) and np.array_equal(b.cpu().numpy(), single)


def test_out_of_range_sets_the_status_and_raises():
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import f0 as f0map
    fs = 16000
    ok = np.array([0.0, 100.0, 1999.0, 0.0])          # fs/8 = 2000
    hot = np.array([0.0, 100.0, 1000.0, 0.0])         # one octave up: 2000 Hz, at the limit
    f0map.map_f0(ok, fs)
    with pytest.raises(ValueError, match='fs/8 = 2000 Hz'):
        f0map.map_f0(hot, fs, key=12)
    with pytest.raises(ValueError, match='fs/8'):
        f0map.map_f0(np.array([100.0, -1.0]), fs)
    with pytest.raises(ValueError, match='fs/8'):
        f0map.map_f0(np.array([100.0, np.nan, np.inf]), fs)
    with pytest.raises(ValueError, match='C-contiguous'):
        f0map.map_f0(np.zeros(10)[::2], fs)
    with pytest.raises(ValueError, match='dtype mismatch'):
        f0map.map_f0(np.zeros(10, dtype=np.float32), fs)
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev)
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    tracks = [torch.from_numpy(a).to(dev) for a in (ok, hot, np.array([3000.0, 2500.0, 0.0]))]
    out = [torch.empty_like(t) for t in tracks]
    status = torch.full((3,), -1, dtype=torch.int32, device=dev)
    f0map.map_f0_batch_dev(ctx, tracks, out, fs, key=12, status=status)
    stream.synchronize()
    assert status.cpu().tolist() == [1, 1, 2]


F0M_GROUP = 32               # tracks per launch (kwy_f0map.hip)


def test_one_track_more_than_a_launch_holds():
    """kwy_logf0_moments_batch_dev and kwy_f0_map_batch_dev on F0M_GROUP + 1 tiny tracks of unequal length in ONE call
    each, the track that falls into the second launch without frames: every track equals the same track through the
    single call, bit for bit, and the words of the last track are written"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import f0 as f0map
    rng = np.random.RandomState(17)
    tracks = [rng.uniform(70.0, 500.0, size=1 + i % 5) for i in range(F0M_GROUP)] + [np.zeros(0)]
    for f0 in tracks[::3]:
        f0[:1] = 0.0
    stats = (np.log(140.0), 0.2, np.log(190.0), 0.12)
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev)
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    d_in = [torch.from_numpy(f).to(dev) for f in tracks]
    d_out = [torch.full_like(t, -1.0) for t in d_in]
    d_m = torch.full((len(tracks), 3), -1.0, dtype=torch.float64, device=dev)
    status = torch.full((len(tracks),), -1, dtype=torch.int32, device=dev)
    f0map.logf0_moments_batch_dev(ctx, d_in, d_m)
    f0map.map_f0_batch_dev(ctx, d_in, d_out, 16000, stats=torch.tensor(stats, dtype=torch.float64, device=dev), key=3.0,
                           status=status)
    stream.synchronize()
    assert status.cpu().tolist() == [0] * len(tracks)
    for i, f0 in enumerate(tracks):
        assert np.array_equal(d_m[i].cpu().numpy(), f0map.logf0_moments([f0])[0]), i
        assert np.array_equal(d_out[i].cpu().numpy(), f0map.map_f0(f0, 16000, stats=stats, key=3.0)), i
    assert d_m[-1].tolist() == [0.0, 0.0, 0.0]


# ---- the CLIs and the batch path ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """convert_voice --convert-f0 trained on 4 CLB -> SLT files with 2 components, the same without the option; the
    model file of the first"""
    import kwiiyatta_amd.convert_voice as cv
    root = tmp_path_factory.mktemp('f0conv')
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
    _run_cli(cv.main, common + ['--result-dir', str(root / 'f0'), '--convert-f0',
                                '--converter-model', str(root / 'model.npz')] + inputs)
    return root, inputs


def _names():
    return [f'arctic_a{n:04}' for n in range(1, 5)]


def test_convert_voice_convert_f0(trained):
    import kwiiyatta_amd as k
    import kwiiyatta_amd.convert_voice as cv
    from kwiiyatta_amd.backend import f0 as f0map
    root, inputs = trained
    conv = k.MelCepstrumConverter(components=2).load(root / 'model.npz')
    assert conv.f0_stats is not None and len(conv.f0_stats) == 4
    mu_s, sigma_s, mu_t, sigma_t = conv.f0_stats
    # the statistics are those of the trimmed training tracks of both sides
    for side_dir, mu, sigma in ((root / 'src', mu_s, sigma_s), (pathlib.Path(SLT_DIR), mu_t, sigma_t)):
        ds = k.WavFileDataset(side_dir)
        feats = [ds[pathlib.Path(f'{name}.wav')] for name in _names()]
        from kwiiyatta_amd.converter.dataset import trim_zeros_frames
        tracks = [np.ascontiguousarray(f.f0[:len(trim_zeros_frames(f.spectrum_envelope))]) for f in feats]
        n, mean, m2 = f0map.merge_moments(f0map.logf0_moments(tracks))
        assert mean == pytest.approx(mu, rel=1e-12) and np.sqrt(m2 / n) == pytest.approx(sigma, rel=1e-12)
    assert mu_t > mu_s            # SLT speaks higher than CLB
    voiced = []
    for name in _names():
        a = (root / 'plain' / f'{name}.diff.wav').read_bytes()
        b = (root / 'f0' / f'{name}.diff.wav').read_bytes()
        assert a == b, name       # the differential output keeps the source's pitch
        f = k.analyze_wav(root / 'f0' / f'{name}.synth.wav').f0
        voiced.append(np.log(f[f > 0]))
    assert abs(np.concatenate(voiced).mean() - mu_t) < 0.05
    # from the saved model: the same outputs bit for bit; the batch path: the same samples within one LSB
    _run_cli(cv.main, ['--result-dir', str(root / 'again'), '--convert-f0', '--converter-model',
                       str(root / 'model.npz')] + inputs)
    _run_cli(cv.main, ['--result-dir', str(root / 'batch'), '--convert-f0', '--batch', '--converter-model',
                       str(root / 'model.npz')] + inputs)
    from scipy.io import wavfile as sio
    for name in _names():
        for kind in ('synth', 'diff'):
            assert (root / 'f0' / f'{name}.{kind}.wav').read_bytes() == \
                (root / 'again' / f'{name}.{kind}.wav').read_bytes(), (name, kind)
            _, a = sio.read(root / 'f0' / f'{name}.{kind}.wav')
            _, c = sio.read(root / 'batch' / f'{name}.{kind}.wav')
            assert a.shape == c.shape and np.abs(a.astype(np.int64) - c.astype(np.int64)).max() <= 1, (name, kind)


def test_convert_batch_key_zero_changes_nothing_and_matches_per_file(trained):
    import kwiiyatta_amd as k
    import kwiiyatta_amd.convert_voice as cv
    from kwiiyatta_amd import corpus
    from scipy.io import wavfile as sio
    root, inputs = trained
    conv = k.MelCepstrumConverter(components=2).load(root / 'model.npz')
    waves = [k.analyze_wav(p).wavdata.data for p in inputs[:2]]
    opts = dict(order=conv.order, frame_period=5.0, pcm=True)
    w0, p0 = corpus.convert_batch(waves, 16000, conv.gmm, **opts)
    w1, p1 = corpus.convert_batch(waves, 16000, conv.gmm, f0_stats=None, transpose_key=0.0, **opts)
    for a, b, c, d in zip(w0, w1, p0, p1):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert c.cpu().numpy().tobytes() == d.cpu().numpy().tobytes()
    w2, p2 = corpus.convert_batch(waves, 16000, conv.gmm, f0_stats=conv.f0_stats, transpose_key=-2.0, **opts)
    _run_cli(cv.main, ['--result-dir', str(root / 'key'), '--no-diffvc', '--convert-f0', '--transpose-key', '-2',
                       '--converter-model', str(root / 'model.npz')] + inputs[:2])
    for i, name in enumerate(_names()[:2]):
        _, a = sio.read(root / 'key' / f'{name}.synth.wav')
        got = p2[i].cpu().numpy()
        assert a.shape == got.shape and np.abs(a.astype(np.int64) - got.astype(np.int64)).max() <= 1, name
        assert not np.array_equal(got, p0[i].cpu().numpy())


def test_training_matrix_moments_equal_the_converters(trained):
    import kwiiyatta_amd as k
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd.backend import f0 as f0map
    root, _ = trained
    conv = k.MelCepstrumConverter(components=2).load(root / 'model.npz')
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
        X, frames, m = corpus.build_training_matrix(pairs, 16000, f0_moments=True, **kw)
        np.random.seed(0)
        X0, frames0 = corpus.build_training_matrix(pairs, 16000, **kw)
        assert frames == frames0 and np.array_equal(X.cpu().numpy(), X0.cpu().numpy())
        assert m.shape == (2, 3)
        assert f0map.stats_from_moments(m[0], m[1]) == pytest.approx(conv.f0_stats, rel=1e-12)


def _pitch_ratio(reference_f0, out_wav):
    import kwiiyatta_amd as k
    g = k.analyze_wav(out_wav).f0
    n = min(len(reference_f0), len(g))
    f, g = reference_f0[:n], g[:n]
    both = (f > 0) & (g > 0)
    assert both.sum() > 50
    return float(np.median(g[both] / f[both]))


@pytest.mark.parametrize('key', [-5, 5, 12])
def test_kwiieiya_transpose_key(key, tmp_path):
    import kwiiyatta_amd as k
    import kwiiyatta_amd.resynthesize_voice as rv
    want = 2.0 ** (key / 12)
    _run_cli(rv.main, ['--result-dir', str(tmp_path / 'plain'), '--transpose-key', str(key), CLB_WAV])
    ratio = _pitch_ratio(k.analyze_wav(CLB_WAV).f0, tmp_path / 'plain' / 'arctic_a0001.wav')
    assert abs(ratio / want - 1) < 0.02, (key, ratio)
    _run_cli(rv.main, ['--result-dir', str(tmp_path / 'carrier'), '--transpose-key', str(key), '--carrier', CLB_WAV2,
                       CLB_WAV])
    ratio = _pitch_ratio(k.analyze_wav(CLB_WAV2).f0, tmp_path / 'carrier' / 'arctic_a0001.wav')
    assert abs(ratio / want - 1) < 0.02, (key, ratio)
