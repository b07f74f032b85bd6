"""DIO and StoneMask on their options, rates and input edges, against the CPU oracle through tests/f0_cases.py.

* every rate class: f0 on the floor, on every band boundary and around the ceiling, exact zeros, a noise burst, and
  signals of a few periods (edge_case, long and short);
* every option of world.dio / dio_batch_dev at non-default values, on a recording and on edge_case;
* lengths around the overlap-save block; the documented refusals; a ragged batch of 33 with guard words;
* the zero-crossing buffers' capacity: an input over the cap sets its status word and leaves its neighbours alone;
* StoneMask on a sweep through its f0 limits, FFT-size steps, the 20 % fall-back, the early stop and both ends of
  the signal.

The frames DIO is held to are those of f0_cases.stable_frames (made from the oracle alone; at most 2 % masked,
asserted in tests/test_f0_cases.py)."""
import numpy as np
import pytest
from scipy.io import wavfile

import f0_cases as fc
from conftest import CLB_WAV, SLT_WAV, clb_variant
from d4c_cases import RATES

pytestmark = pytest.mark.gpu

GUARD = -12345.678


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


def recording(fs, tag='clb'):
    path = {('clb', 16000): CLB_WAV, ('slt', 16000): SLT_WAV, ('clb', 48000): clb_variant('48')}[(tag, fs)]
    rate, d = wavfile.read(path)
    assert rate == fs
    return np.ascontiguousarray(d.astype(np.float64) / 2 ** 15)


def check_dio(ko, x, fs, label, **options):
    """host entry against the oracle on the stable frames; returns the oracle's (f0, t)"""
    from kwiiyatta_amd.backend import world
    ref = ko.dio(x, fs, **options)
    got = world.dio(x, fs, **options)
    fc.assert_f0_close(got, ref, fc.stable_frames(ko, x, fs, **options), label,
                       options.get('f0_floor', fc.F0_FLOOR), options.get('f0_ceil', fc.F0_CEIL))
    return ref


def batch_dio(ctx, waves, fs, **options):
    """dio_batch_dev with one guard word before and after every output buffer and around the status words.
    Returns (t, f0, status) per utterance; asserts the guards."""
    import torch
    from kwiiyatta_amd.backend import world
    T = [world.dio_frames(fs, len(x), options.get('frame_period', 5.0)) for x in waves]
    start = np.concatenate([[0], np.cumsum([n + 2 for n in T])])
    dx = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in waves]
    tbuf = torch.full((int(start[-1]),), GUARD, dtype=torch.float64, device='cuda')
    fbuf = torch.full((int(start[-1]),), GUARD, dtype=torch.float64, device='cuda')
    sbuf = torch.full((len(waves) + 2,), 7, dtype=torch.int32, device='cuda')
    t = [tbuf[int(a) + 1:int(a) + 1 + n] for a, n in zip(start, T)]
    f0 = [fbuf[int(a) + 1:int(a) + 1 + n] for a, n in zip(start, T)]
    torch.cuda.synchronize()          # (torch filled these on ITS stream; the library runs on the context's)
    world.dio_batch_dev(ctx, dx, fs, t, f0, sbuf[1:len(waves) + 1], **options)
    ctx.sync()
    th, fh, sh = tbuf.cpu().numpy(), fbuf.cpu().numpy(), sbuf.cpu().numpy()
    for a, n in zip(start, T):
        for buf in (th, fh):
            assert buf[int(a)] == GUARD and buf[int(a) + n + 1] == GUARD, 'a word next to an output buffer was written'
    assert sh[0] == 7 and sh[-1] == 7
    return ([th[int(a) + 1:int(a) + 1 + n] for a, n in zip(start, T)],
            [fh[int(a) + 1:int(a) + 1 + n] for a, n in zip(start, T)], sh[1:-1])


# ------------------------------------------------------------------------------------------------------------ DIO
@pytest.mark.parametrize('fs', RATES)
def test_dio_edges(ko, fs):
    """edge_case, long and short, at default options on every rate class"""
    x, _ = fc.edge_case(fs, 1)
    f0, _ = check_dio(ko, x, fs, f'edge {fs}')
    assert f0.max() > 785.0
    for seed in range(len(fc.SHORT_PERIODS)):
        xs, claims = fc.edge_case(fs, seed, short=True)
        check_dio(ko, xs, fs, f'edge {fs} short {claims["periods"]}')


@pytest.mark.parametrize('options', fc.OPTION_SETS, ids=fc.option_id)
@pytest.mark.parametrize('fs', [16000, 48000])
def test_dio_options(ko, fs, options):
    """every option at non-default values, on a recording and on the form of edge_case paired with the set; then
    StoneMask of the oracle's track"""
    from kwiiyatta_amd.backend import world
    inputs = ((f'arctic_a0001 {fc.recording_for(fs, options)}', recording(fs, fc.recording_for(fs, options))),
              ('edge_case', fc.edge_case(fs, 1, in_range=fc.wants_in_range(options))[0]))
    for name, x in inputs:
        label = f'{name} {fs} {fc.option_id(options)}'
        f0, t = check_dio(ko, x, fs, label, **options)
        fc.assert_refined_close(world.stonemask(x, f0, t, fs), ko.stonemask(x, f0, t, fs), label, f0_in=f0)


@pytest.mark.parametrize('fs', [16000, 96000])
def test_dio_lengths(ko, fs):
    """lengths around one and two overlap-save blocks, 1 and 2 samples and one low-cut half length; and a second
    of signal at k V - 1, k V, k V + 1, so that edges fall on both sides of many block seams"""
    from kwiiyatta_amd.backend import world
    V = fc.band_plan(fs)['V']
    lengths = fc.length_cases(fs) + fc.length_cases(fs, ks=(fs // V + 1,))[3:]
    for n in lengths:
        x = fc.length_signal(fs, n)
        ref = check_dio(ko, x, fs, f'length {fs} {n}')
        assert len(ref[0]) == world.dio_frames(fs, n) == int(1000.0 * n / fs / 5.0) + 1
    assert ref[0].any()


def test_dio_refusals(ko):
    """the documented refusals raise ValueError and leave the context usable"""
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import world
    ctx = _lib.Context(0)
    x16, x96, x8 = fc.edge_case(16000, 2)[0], fc.edge_case(96000, 2)[0], fc.edge_case(8000, 2)[0]

    after = x16[:8000]
    after_ref, after_mask = ko.dio(after, 16000), fc.stable_frames(ko, after, 16000)
    assert after_ref[0].any()

    def refused(x, fs, **options):
        with pytest.raises(ValueError):
            world.dio(x, fs, ctx=ctx, **options)
        # a default call right after agrees with the oracle
        fc.assert_f0_close(world.dio(after, 16000, ctx=ctx), after_ref, after_mask,
                           f'after refusal {fs} {fc.option_id(options)}')

    assert fc.band_plan(16000, channels_in_octave=4.6)['nbands'] == 17
    refused(x16, 16000, channels_in_octave=4.6)                       # 17 bands
    assert min(fc.band_plan(8000, f0_ceil=12000.0)['hal']) < 1
    refused(x8, 8000, f0_ceil=12000.0)                                # a band above the sampling rate: hal < 1
    assert fc.band_plan(96000, f0_floor=40.0)['filter_span'] > fc.FILTER_SPAN_MAX
    refused(x96, 96000, f0_floor=40.0)                                # filters too long for the block
    refused(x16, 16000, speed=2)
    with pytest.raises(ValueError):
        ko.dio(x16, 16000, speed=2)                                   # (the oracle refuses it too)
    refused(x16, 16000, f0_floor=0.0)
    refused(x16, 16000, f0_floor=-71.0)
    refused(x16, 16000, f0_floor=800.0)                               # ceil <= floor
    refused(x16, 16000, f0_ceil=71.0)
    refused(x16, 16000, f0_ceil=60.0)
    refused(x16, 16000, channels_in_octave=0.0)
    refused(x16, 16000, channels_in_octave=-2.0)
    refused(x16, 16000, frame_period=0.0)                             # (the wrapper's own check: no frame count)
    refused(x16, 16000, frame_period=-5.0)
    import torch
    dx = torch.from_numpy(after).cuda()
    out = [torch.zeros(world.dio_frames(16000, len(after)), dtype=torch.float64, device='cuda') for _ in range(2)]
    torch.cuda.synchronize()
    for bad in (dict(frame_period=0.0), dict(frame_period=-5.0), dict(f0_floor=0.0), dict(speed=2)):
        with pytest.raises(ValueError):                               # ... and the library's, through the device entry
            world.dio_batch_dev(ctx, [dx], 16000, out[:1], out[1:], **bad)
    ctx.sync()
    # ... next to the smallest floor the block admits at 96 kHz, which must run and agree
    lo = fc.smallest_floor(96000)
    assert fc.band_plan(96000, f0_floor=lo)['filter_span'] == fc.FILTER_SPAN_MAX
    ref = ko.dio(x96, 96000, f0_floor=lo)
    fc.assert_f0_close(world.dio(x96, 96000, f0_floor=lo, ctx=ctx), ref,
                       fc.stable_frames(ko, x96, 96000, f0_floor=lo), f'96 kHz floor {lo}', f0_floor=lo)
    assert ref[0].any()


BATCH_OPTIONS = dict(f0_floor=60.0, f0_ceil=1000.0, channels_in_octave=3.0, allowed_range=0.05, frame_period=2.5)


@pytest.mark.parametrize('fs', [16000, 48000])
def test_dio_batch_mixed(fs):
    """33 utterances from 1 sample to 2 s in one call (two passes) with non-default options: every member bit-equal
    to its own single call, no status word set, no word next to an output buffer written"""
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import world
    waves = fc.batch_mixed_cases(fs)
    assert len(waves) == 33 and min(len(x) for x in waves) == 1 and max(len(x) for x in waves) == 2 * fs
    ctx = _lib.Context(0)
    t, f0, status = batch_dio(ctx, waves, fs, **BATCH_OPTIONS)
    assert not status.any()
    voiced = 0
    for i, x in enumerate(waves):
        f0_h, t_h = world.dio(x, fs, **BATCH_OPTIONS)
        assert np.array_equal(t[i], t_h) and np.array_equal(f0[i], f0_h), (i, len(x))
        voiced += int((f0_h > 0).sum())
    assert voiced > 1000


def test_dio_capacity(ko):
    """An utterance with more zero crossings than the buffers hold (f0_cases.capacity_cases, 1.8 x the cap on the
    CPU) sets its status word through the device entry and raises through the host entry; its neighbours in the
    batch are untouched, no word next to a buffer is written, and the context goes on working.  The one 0.4 x
    under the cap runs as usual."""
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import world
    fs, options = fc.CAPACITY_FS, fc.CAPACITY_OPTIONS
    over, under = fc.capacity_cases()
    ctx = _lib.Context(0)
    ref = ko.dio(under, fs, **options)
    fc.assert_f0_close(world.dio(under, fs, ctx=ctx, **options), ref, fc.stable_frames(ko, under, fs, **options),
                       'under the cap', f0_ceil=options['f0_ceil'])
    edge = fc.edge_case(fs, 5)[0]
    waves = [edge[:len(over)], under, over, edge[len(over):2 * len(over)], under[:1000]]
    t, f0, status = batch_dio(ctx, waves, fs, **options)
    assert status.tolist() == [0, 0, 1, 0, 0]
    assert np.isfinite(f0[2]).all()
    for i in (0, 1, 3, 4):
        f0_h, t_h = world.dio(waves[i], fs, ctx=ctx, **options)
        assert np.array_equal(t[i], t_h) and np.array_equal(f0[i], f0_h), i
    assert sum(int(f0[i].any()) for i in (0, 3)) == 2
    with pytest.raises(RuntimeError, match='overflow'):
        world.dio(over, fs, ctx=ctx, **options)
    x = fc.edge_case(16000, 5)[0]
    fc.assert_f0_close(world.dio(x, 16000, ctx=ctx), ko.dio(x, 16000), fc.stable_frames(ko, x, 16000),
                       'after the overflow')


# ------------------------------------------------------------------------------------------------------ StoneMask
def stonemask_dev(ctx, items, fs, batch):
    """the device entries on items (x, f0, t): one kwy_stonemask_dev call per item, or one stonemask_batch_dev call
    over all"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, c_vp
    from kwiiyatta_amd.backend import world
    dev = [[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in item] for item in items]
    out = [torch.full((len(item[1]) + 2,), GUARD, dtype=torch.float64, device='cuda') for item in items]
    torch.cuda.synchronize()
    if batch:
        world.stonemask_batch_dev(ctx, [d[0] for d in dev], [d[2] for d in dev], [d[1] for d in dev], fs,
                                  [o[1:-1] for o in out])
    else:
        for (dx, df, dt), o in zip(dev, out):
            _lib.check(ctx, lib.kwy_stonemask_dev(ctx.handle, c_vp(dx.data_ptr()), dx.numel(), fs, c_vp(dt.data_ptr()),
                                                  c_vp(df.data_ptr()), df.numel(), c_vp(o[1:-1].data_ptr())))
    ctx.sync()
    res = [o.cpu().numpy() for o in out]
    assert all(r[0] == GUARD and r[-1] == GUARD for r in res)
    return [r[1:-1] for r in res]


@pytest.mark.parametrize('fs', fc.STONEMASK_RATES)
def test_stonemask_edges(ko, fs):
    """the sweep from 38 Hz to fs / 11.5 with its limit frames, the off-by-25 % / 2.2 x track (the 20 % fall-back),
    the track at 1 / 3.5 and 1 / 4.5 of the sweep (the early stop at twice the input), a signal shorter than every
    window, and the silent signal: host entry, device entry, and all five as one batch"""
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import world
    x, t, f0, f0_off, f0_low = fc.stonemask_case(fs)
    xs, ts, f0s = fc.stonemask_short_case(fs)
    items = [(x, f0, t), (x, f0_off, t), (x, f0_low, t), (xs, f0s, ts), (np.zeros(len(x)), f0, t)]
    names = ['sweep', 'off', 'low', 'short', 'silent']
    refs = [ko.stonemask(*item, fs) for item in items]
    ctx = _lib.Context(0)
    host = [world.stonemask(*item, fs, ctx=ctx) for item in items]
    single = stonemask_dev(ctx, items, fs, batch=False)
    batch = stonemask_dev(ctx, items, fs, batch=True)
    for name, item, ref, h, s, b in zip(names, items, refs, host, single, batch):
        fc.assert_refined_close(h, ref, f'{name} {fs}', f0_in=item[1])
        assert np.array_equal(s, h) and np.array_equal(b, h), name
    assert np.array_equal(refs[4], np.where((f0 > 40.0) & (f0 <= fs / 12.0), f0, 0.0))     # silence keeps the input
