"""The pitch-shift kernels (kwy_pitch.hip) through the C ABI and the shim, against the numpy statement of
tests/pitch_cases.py.

Positions are checked CONDITIONALLY -- one flipped near-tie would change the whole chain behind it: for every step the
yardstick's distances are computed from the kernel's own p_{k-1}, and the kernel's p_k must be a minimiser within the
rounding of a sum of L non-negative terms on both sides (pitch_cases.distance_slack).  The waveform is compared with
the yardstick's stretch + resample fed with the kernel's positions, sample by sample against pitch_cases.waveform_bound.
"""
import numpy as np
import pytest

import pitch_cases as pc
from conftest import CLB_WAV, SLT_WAV, clb_variant

pytestmark = pytest.mark.gpu


def _synthetic():
    from kwiiyatta_amd.synthetic import make_utterance
    return 48000, make_utterance(seed=11, fs=48000, seconds=1.5)[0]


CASES = [('clb16', CLB_WAV, 0.5), ('clb16', CLB_WAV, 0.8909), ('clb16', CLB_WAV, 1.4983), ('clb16', CLB_WAV, 2.0),
         ('clb22', clb_variant('22'), 1.4983), ('clb44', clb_variant('44'), 0.8909), ('clb44', clb_variant('44'), 2.0),
         ('clb48', clb_variant('48'), 0.5), ('clb48', clb_variant('48'), 2.0), ('clb96', clb_variant('96'), 1.4983),
         ('synthetic', None, 0.8909), ('synthetic', None, 2.0)]


def _input(wav):
    return _synthetic() if wav is None else pc.load(wav)


@pytest.mark.parametrize('name,wav,rate', CASES, ids=[f'{c[0]}-{c[2]}' for c in CASES])
def test_positions_and_waveform_against_the_yardstick(name, wav, rate, gpu_ctx):
    from kwiiyatta_amd.backend import pitch
    fs, x = _input(wav)
    y, p = pitch.shift_pitch(x, fs, rate, positions=True, ctx=gpu_ctx)
    H, L, S, M, K = pc.constants(len(x), fs, rate)
    assert p.dtype == np.int32 and p.shape == (K,) and y.shape == x.shape
    assert pitch.frames(len(x), fs, rate) == K and pitch.stretched_length(len(x), rate) == M
    assert p[0] == 0
    slack = pc.distance_slack(fs)
    differ = 0
    for k in range(1, K):
        q, d, a = pc.step_distances(x, fs, k, int(p[k - 1]), M=M)
        assert q[0] <= p[k] <= q[-1], f'step {k}: position {p[k]} outside [{q[0]}, {q[-1]}]'
        d_kernel, d_min = d[p[k] - q[0]], d.min()
        assert d_kernel <= d_min * (1 + slack), \
            f'step {k}: d({p[k]}) = {d_kernel!r} is not minimal within rounding (min {d_min!r})'
        differ += int(p[k]) != pc.choose(q, d, a)
    print(f'{name} rate {rate}: {differ} of {K - 1} steps differ from the yardstick\'s conditional choice')
    assert differ <= 0.01 * (K - 1)
    ref = pc.resample(pc.stretch(x, fs, p, M), len(x))
    bound = pc.waveform_bound(x, fs, p, len(x), M)
    err = np.abs(y - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f'{name} rate {rate}: worst |error| / bound = {worst:.4f}, max |error| = {err.max():.3e}')
    assert (err <= bound).all()


@pytest.mark.parametrize('wav', [CLB_WAV, clb_variant('48'), clb_variant('44')], ids=['16k', '48k', '44k'])
def test_rate_one_is_the_identity_bit_for_bit(wav, gpu_ctx):
    from kwiiyatta_amd.backend import pitch
    fs, x = pc.load(wav)
    y, p = pitch.shift_pitch(x, fs, 1.0, positions=True, ctx=gpu_ctx)
    assert np.array_equal(y, x)
    assert np.array_equal(p, np.arange(len(p)) * int(fs * 0.010))


def test_silence_and_short_inputs(gpu_ctx):
    from kwiiyatta_amd.backend import pitch
    for rate in (0.5, 1.0, 2.0):
        assert not pitch.shift_pitch(np.zeros(5000), 16000, rate, ctx=gpu_ctx).any()
        y, p = pitch.shift_pitch(np.zeros(0), 16000, rate, positions=True, ctx=gpu_ctx)
        assert y.shape == (0,) and p.shape == (0,)
        for n in (1, 50, 159, 161, 333):
            x = np.random.RandomState(n).uniform(-0.5, 0.5, n)
            y, p = pitch.shift_pitch(x, 16000, rate, positions=True, ctx=gpu_ctx)
            ref, p_ref = pc.shift_pitch(x, 16000, rate, with_positions=True)
            assert np.array_equal(p, p_ref)
            M = pc.constants(n, 16000, rate)[3]
            assert (np.abs(y - ref) <= pc.waveform_bound(x, 16000, p, n, M)).all()


def test_batch_equals_single_bit_for_bit(gpu_ctx):
    import torch
    from kwiiyatta_amd.backend import pitch
    fs, x = pc.load(CLB_WAV)
    lengths = [len(x), 0, 50, 12345, 160, 30001, 7, 4800]
    dev = torch.device('cuda', 0)
    for rate in (0.5, 1.4983, 2.0):
        singles = [pitch.shift_pitch(np.ascontiguousarray(x[:n]), fs, rate, positions=True, ctx=gpu_ctx) for n in lengths]
        xs = [torch.from_numpy(np.ascontiguousarray(x[:n])).to(dev) for n in lengths]
        ys = [torch.full_like(v, float('nan')) for v in xs]
        ps = [torch.full((pitch.frames(n, fs, rate),), -7, dtype=torch.int32, device=dev) if i % 2 == 0 else None
              for i, n in enumerate(lengths)]
        torch.cuda.synchronize()
        pitch.shift_pitch_batch_dev(gpu_ctx, xs, ys, fs, rate, positions=ps)
        gpu_ctx.sync()
        for (y1, p1), y, p in zip(singles, ys, ps):
            assert np.array_equal(y.cpu().numpy(), y1)
            if p is not None:
                assert np.array_equal(p.cpu().numpy(), p1)


def test_a_batch_beyond_one_table_group(gpu_ctx):
    """more jobs than one table kernel takes: every job still gets its own result"""
    import torch
    from kwiiyatta_amd.backend import pitch
    fs, x = pc.load(CLB_WAV)
    dev = torch.device('cuda', 0)
    lengths = [2000 + 37 * i for i in range(70)]
    xs = [torch.from_numpy(np.ascontiguousarray(x[20000:20000 + n])).to(dev) for n in lengths]
    ys = [torch.empty_like(v) for v in xs]
    torch.cuda.synchronize()
    pitch.shift_pitch_batch_dev(gpu_ctx, xs, ys, fs, 1.25)
    gpu_ctx.sync()
    for i in (0, 63, 64, 69):
        single = pitch.shift_pitch(np.ascontiguousarray(x[20000:20000 + lengths[i]]), fs, 1.25, ctx=gpu_ctx)
        assert np.array_equal(ys[i].cpu().numpy(), single)


def test_two_runs_are_bit_reproducible(gpu_ctx):
    from kwiiyatta_amd.backend import pitch
    fs, x = pc.load(clb_variant('48'))
    a = pitch.shift_pitch(x, fs, 1.4983, positions=True, ctx=gpu_ctx)
    b = pitch.shift_pitch(x, fs, 1.4983, positions=True, ctx=gpu_ctx)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('wav', [CLB_WAV, SLT_WAV], ids=['clb', 'slt'])
def test_f0_follows_the_rate_through_the_device(wav, gpu_ctx):
    from kwiiyatta_amd.backend import pitch, world

    def f0_of(v):
        f0, t = world.dio(v, fs, ctx=gpu_ctx)
        return world.stonemask(v, f0, t, fs, ctx=gpu_ctx)
    fs, x = pc.load(wav)
    f0_in = f0_of(x)
    for rate in pc.RATES:
        median, share = pc.f0_ratio(f0_in, f0_of(pitch.shift_pitch(x, fs, rate, ctx=gpu_ctx)))
        print(f'rate {rate}: median f0 ratio / rate = {median / rate:.4f} over {100 * share:.0f} % of the frames')
        assert share > 0.2
        assert abs(median / rate - 1) <= 0.02


def test_value_errors(gpu_ctx):
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import pitch
    x = np.zeros(1000)
    for rate in (0.49, 2.01, float('nan'), float('inf'), -1.0, 0.0):
        with pytest.raises(ValueError, match='rate'):
            pitch.shift_pitch(x, 16000, rate, ctx=gpu_ctx)
    with pytest.raises(ValueError, match="expected 'double'"):
        pitch.shift_pitch(x.astype(np.float32), 16000, 1.5, ctx=gpu_ctx)
    with pytest.raises(ValueError, match='not C-contiguous'):
        pitch.shift_pitch(np.zeros(2000)[::2], 16000, 1.5, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        pitch.shift_pitch(np.zeros((10, 10)), 16000, 1.5, ctx=gpu_ctx)
    # the C entry itself refuses what the shim would not pass on
    y = np.empty_like(x)
    for fs, rate in ((16000, 2.5), (16000, float('nan')), (50, 1.5), (200000, 1.5)):
        rc = _lib.lib.kwy_pitch_shift(gpu_ctx.handle, _lib.ptr(x), len(x), fs, rate, _lib.ptr(y), None)
        assert rc == _lib.KWY_EINVAL
    assert _lib.lib.kwy_pitch_frames(1000, 16000, 3.0) == -1 and _lib.lib.kwy_pitch_stretched_length(-1, 1.0) == -1
    assert _lib.lib.kwy_pitch_frames(1000, 16000, 2.0) == 13 and _lib.lib.kwy_pitch_stretched_length(1000, 0.5) == 500
