"""The pYIN kernels (kwiiyatta_amd/csrc/kwy_pyin.hip) against the numpy model of tests/pyin_cases.py.

Observation bound (the convention of k_nmf_gemm's test): 64 d on exp(L), d the larger of the float64 model's deviation
from its long-double form and from itself with the FFT form of the difference function, never below 2^-52 tau_max.
A frame is left out only where one of the model's own decisions lies closer to its edge than that bound (or the three
model forms already decide differently), and at most 2 % of a case's frames may be."""
import functools

import numpy as np
import pytest

import pyin_cases as pc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, Params) of a named input"""
    if name.startswith('glide'):
        fs = int(name[5:])
        return pc.glide(fs)[0], pc.Params(fs)
    if name == 'speech16':
        x, fs = pc.speech()
        return x, pc.Params(fs)
    if name == 'speech96':
        x, fs = pc.speech('96')                           # N = 4096
        return x, pc.Params(fs)
    return pc.edge_cases()[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 model's frames and probabilities, the bound, and the frames that are compared"""
    x, p = case(name)
    a = pc.observe(x, p)
    # (at N = 4096 the direct sums in long double take 80 ms a frame: that deviation is measured on every fourth frame;
    # the kernel is held to the float64 model on ALL frames)
    stride = 4 if p.N >= 4096 else 1
    b = pc.observe(x, p, dtype=pc.LD, stride=stride)
    c = pc.observe(x, p, form='fft')
    agree = np.array([(fb is None or pc.same_decisions(fa, fb)) and pc.same_decisions(fa, fc)
                      for fa, fb, fc in zip(a, b, c)])
    Pa, Pc = pc.probabilities(a, p), pc.probabilities(c, p)
    had = np.array([fb is not None for fb in b])
    Pb = pc.probabilities([fb for fb in b if fb is not None], p)
    d = 2.0 ** -52 * p.tau_max
    if agree.any():
        d = max(d, np.abs(Pa - Pc)[agree].max())
    if (agree & had).any():
        d = max(d, np.abs(Pa[had] - Pb)[agree[had]].max())
    bound = 64 * d
    keep = agree & np.array([f.margin >= bound for f in a])
    return a, Pa, d, bound, keep


OBSERVE_CASES = ['glide16000', 'glide48000', 'speech16', 'speech96'] + sorted(pc.edge_cases())


@pytest.mark.parametrize('name', OBSERVE_CASES)
def test_observe_matches_the_model(name, gpu_ctx):
    from kwiiyatta_amd.backend import pyin
    x, p = case(name)
    frames, P, d, bound, keep = reference(name)
    left_out = int((~keep).sum())
    assert left_out <= 0.02 * len(keep), f'the model itself leaves out {left_out} of {len(keep)} frames'
    L = pyin.observe(np.ascontiguousarray(x), p.fs, ctx=gpu_ctx, **p.kwargs())
    assert L.shape == (len(frames), p.nb + 1) and np.isfinite(L).all()
    dev = np.abs(np.exp(L) - np.maximum(P, pc.TINY))[keep]
    worst = dev.max() if dev.size else 0.0
    print(f'{name}: frames {len(keep)}, left out {left_out}, d {d:.3e}, bound {bound:.3e}, kernel {worst:.3e}')
    assert worst <= bound


def random_rows(T, nb, seed, ties):
    rng = np.random.default_rng(seed)
    if ties:
        return np.ascontiguousarray(rng.integers(-3, 1, size=(T, nb + 1)).astype(np.float64))
    return np.ascontiguousarray(np.log(rng.uniform(1e-6, 1.0, size=(T, nb + 1))))


@pytest.mark.parametrize('name', ['glide16000', 'speech16', 'random', 'ties', 'ties_r44', 'one_frame', 'two_frames'])
def test_decode_equals_the_model(name, gpu_ctx):
    from kwiiyatta_amd.backend import pyin
    nb, R, floor = 420, 22, 71.0
    if name in ('glide16000', 'speech16'):
        x, p = case(name)
        L = pc.log_matrix(reference(name)[0], p)
    elif name == 'ties_r44':
        L, R = random_rows(24, 60, 5, True), 44          # a window wider than the bin range on both sides
        nb = 60
    else:
        T = {'one_frame': 1, 'two_frames': 2}.get(name, 40)
        L = random_rows(T, nb, 3, name != 'random')
    trans = pyin.transition_table(R)
    freq = pyin.bin_frequencies(nb, floor)
    assert np.array_equal(trans, pc.transition_table(R)) and np.array_equal(freq, pc.bin_frequencies(nb, floor))
    want, states, _ = pc.decode(L, trans, freq)
    got = pyin.decode(L, trans, freq, ctx=gpu_ctx)
    assert np.array_equal(got, want), f'{int((got != want).sum())} of {len(want)} frames differ'
    if name in ('ties', 'ties_r44'):
        assert len(set(states.tolist())) > 1


def path_is_stable(name):
    """the model's path under +- the observation bound on every probability"""
    x, p = case(name)
    frames, P, d, bound, keep = reference(name)
    trans, freq = pc.transition_table(p.R), pc.bin_frequencies(p.nb, p.f0_floor)
    want = pc.decode(np.log(np.maximum(P, pc.TINY)), trans, freq)[1]
    rng = np.random.default_rng(11)
    for _ in range(2):
        Q = np.maximum(P + bound * rng.choice([-1.0, 1.0], size=P.shape), pc.TINY)
        if not np.array_equal(pc.decode(np.log(Q), trans, freq)[1], want):
            return False
    return True


@pytest.mark.parametrize('name', ['glide16000', 'glide48000', 'speech16', 'speech96'])
def test_track_end_to_end(name, gpu_ctx):
    from kwiiyatta_amd.backend import pyin
    x, p = case(name)
    assert path_is_stable(name)
    want = pc.decode(pc.log_matrix(reference(name)[0], p), pc.transition_table(p.R),
                     pc.bin_frequencies(p.nb, p.f0_floor))[0]
    f0, t = pyin.pyin(np.ascontiguousarray(x), p.fs, ctx=gpu_ctx)          # (speech96: N = 4096 end to end)
    assert np.array_equal(t, np.arange(len(want)) * p.frame_period / 1000.0)
    differ = int((np.abs(f0 - want) > 1e-12 * np.maximum(want, 1.0)).sum())
    print(f'{name}: {differ} of {len(want)} frames differ from the model')
    assert differ <= 0.02 * len(want)
    if name.startswith('glide'):
        assert (f0[(t >= 0.12) & (t <= 0.48)] > 0).all()
        assert (f0[(t < 0.08) | (t >= 0.52)] == 0).all()
        v = (f0 > 0) & (t >= 0.1) & (t <= 0.5)
        assert pc.cents(f0[v], pc.glide_f0_at(t[v])).max() < 25.0


def batch_tracks(ctx, waves, fs, **kw):
    import torch
    from kwiiyatta_amd.backend import pyin
    dev = [torch.from_numpy(np.ascontiguousarray(w)).cuda() for w in waves]
    T = [pyin.frames(fs, len(w)) for w in waves]
    t = [torch.full((n,), -1.0, dtype=torch.float64, device='cuda') for n in T]
    f = [torch.full((n,), -1.0, dtype=torch.float64, device='cuda') for n in T]
    status = torch.full((len(waves),), 7, dtype=torch.int32, device='cuda')
    pyin.pyin_batch_dev(ctx, dev, fs, t, f, status, **kw)
    ctx.sync()
    return [a.cpu().numpy() for a in f], [a.cpu().numpy() for a in t], status.cpu().numpy()


def test_batch_equals_single_calls_bit_for_bit(gpu_ctx):
    from kwiiyatta_amd.backend import pyin
    g = case('glide16000')[0]
    s = case('speech16')[0]
    waves = [g, s[:3000], np.zeros(500), s, g[2000:6000]] + [s[i * 200:i * 200 + 1500 + 37 * i] for i in range(30)]
    f, t, status = batch_tracks(gpu_ctx, waves, 16000)          # 35 utterances: two passes of launches
    assert (status == 0).all()
    for w, fb, tb in zip(waves, f, t):
        f1, t1 = pyin.pyin(np.ascontiguousarray(w), 16000, ctx=gpu_ctx)
        assert np.array_equal(f1, fb) and np.array_equal(t1, tb)
    f2, t2, _ = batch_tracks(gpu_ctx, waves, 16000)
    assert all(np.array_equal(a, b) for a, b in zip(f, f2))


def test_non_finite_sample_sets_the_status_word(gpu_ctx):
    from kwiiyatta_amd.backend import pyin
    g = case('glide16000')[0]
    bad = g.copy()
    bad[4000] = np.nan
    inf = g[:5000].copy()
    inf[-1] = np.inf                     # the last sample: no frame of a narrow window need cover it
    f, t, status = batch_tracks(gpu_ctx, [g, bad, g[1000:7000], inf], 16000)
    assert status.tolist() == [0, 1, 0, 1]
    assert (f[1] == 0).all() and (f[3] == 0).all()
    assert np.array_equal(f[0], pyin.pyin(g, 16000, ctx=gpu_ctx)[0])
    assert np.array_equal(f[2], pyin.pyin(np.ascontiguousarray(g[1000:7000]), 16000, ctx=gpu_ctx)[0])
    with pytest.raises(ValueError, match='not finite'):
        pyin.check_status(status)
    with pytest.raises(ValueError, match='not finite'):
        pyin.pyin(bad, 16000, ctx=gpu_ctx)
    with pytest.raises(ValueError, match='not finite'):
        pyin.observe(bad, 16000, ctx=gpu_ctx)
    f, t, status = batch_tracks(gpu_ctx, [inf], 16000, f0_floor=400.0, f0_ceil=800.0)
    assert status.tolist() == [1] and (f[0] == 0).all()


def test_unsupported_sizes_are_refused(gpu_ctx):
    from kwiiyatta_amd.backend import pyin
    x = np.zeros(4000)
    assert pyin.fft_size(96000) == 4096 and pyin.fft_size(192000) == 8192
    with pytest.raises(ValueError, match='4096'):
        pyin.pyin(x, 192000, ctx=gpu_ctx)
    with pytest.raises(ValueError, match='4096'):
        pyin.pyin(x, 16000, f0_floor=7.0, ctx=gpu_ctx)
    assert 2 * pyin.bins(40.0, 1000.0) > 1024
    with pytest.raises(ValueError, match='1024 states'):
        pyin.pyin(x, 16000, f0_floor=40.0, f0_ceil=1000.0, ctx=gpu_ctx)
    with pytest.raises(ValueError, match='1024 states'):
        pyin.decode(np.zeros((3, 514)), pyin.transition_table(2), np.ones(513), ctx=gpu_ctx)
    assert pyin.scratch_bytes(2001, 420) >= 2001 * (421 * 8 + 840 * 2)
    assert pyin.scratch_bytes(2001, 420, 256) == pyin.scratch_bytes(2001, 420, 32)


# ---- plumbing: the analyzer, the batch head and the options ------------------------------------------------------------
def test_analyzer_follows_the_estimator(gpu_ctx):
    import kwiiyatta_amd as k
    from kwiiyatta_amd.backend import world
    x, fs = pc.speech()
    wav = k.Wavdata(fs, x)
    a = k.Analyzer(wav, f0_estimator='pyin')
    coarse, t = world.pyin(x, fs)
    assert np.array_equal(a.extract_f0(), world.stonemask(x, coarse, t, fs))
    assert np.array_equal(k.Analyzer(wav).extract_f0(estimator='pyin'), a.f0)
    coarse, t = world.dio(x, fs)
    dio = world.stonemask(x, coarse, t, fs)
    assert np.array_equal(k.Analyzer(wav).extract_f0(), dio)          # the default is today's path, bit for bit
    assert np.array_equal(k.Analyzer(wav, f0_estimator='dio').f0, dio)
    assert not np.array_equal(a.f0, dio)
    held = k.Analyzer(wav)
    assert np.array_equal(held.f0, dio)
    with pytest.raises(ValueError, match="holds dio's track already"):      # the track is made once
        held.extract_f0(estimator='pyin')
    assert np.array_equal(held.extract_f0(estimator='dio'), dio)
    with pytest.raises(ValueError, match='harvest'):
        k.Analyzer(wav, f0_estimator='harvest')
    assert a.spectrum_envelope.shape[0] == len(a.f0) == 121          # nothing downstream changes shape


def test_batch_head_equals_the_analyzer(gpu_ctx):
    """what the device drivers run in front of a wave (pipeline.coarse_f0_batch_dev + StoneMask) gives the per-file
    tracks"""
    import torch
    import kwiiyatta_amd as k
    from kwiiyatta_amd import pipeline
    from kwiiyatta_amd.backend import world
    x, fs = pc.speech()
    waves = [x, np.ascontiguousarray(x[:5000]), pc.glide(fs)[0]]
    for estimator in pipeline.F0_ESTIMATORS:
        dev = [torch.from_numpy(w).cuda() for w in waves]
        T = [world.dio_frames(fs, len(w)) for w in waves]
        t, coarse, f0 = ([torch.empty(n, dtype=torch.float64, device='cuda') for n in T] for _ in range(3))
        status = torch.zeros(len(waves), dtype=torch.int32, device='cuda')
        jobs, sm = pipeline.f0_jobs(dev, t, coarse, f0, status)
        pipeline.coarse_f0_batch_dev(gpu_ctx, estimator, jobs, len(waves), fs, 5.0)
        world.stonemask_batch_dev(gpu_ctx, dev, t, coarse, fs, f0)
        gpu_ctx.sync()
        pipeline.check_f0_status(estimator, status.cpu().numpy())
        for w, track in zip(waves, f0):
            assert np.array_equal(track.cpu().numpy(), k.Analyzer(k.Wavdata(fs, w), f0_estimator=estimator).f0)
    with pytest.raises(ValueError, match='not finite'):
        pipeline.check_f0_status('pyin', [0, 1])
    with pytest.raises(RuntimeError, match='zero-crossing'):
        pipeline.check_f0_status('dio', [0, 1])


def test_convert_batch_takes_the_estimator(gpu_ctx):
    from kwiiyatta_amd import corpus
    with pytest.raises(ValueError, match='harvest'):
        corpus.convert_batch([], 16000, None, f0_estimator='harvest')
    with pytest.raises(ValueError, match='lockstep'):
        corpus.convert_batch([], 16000, None, f0_estimator='pyin', driver='streams')
