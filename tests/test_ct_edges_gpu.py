"""CheapTrick and its fused mel-cepstrum form on the GPU, through the C ABI, on the inputs of tests/ct_cases.py: every
rate class and fft size, f0 on / below / just above the effective floor, windows of a handful of samples, frames
beyond the signal, positions off the frame grid, sub-window and one-sample signals, a closing stretch that shows
whether every frame found its place in the noise stream; the batched entries against the single calls; the options
and the refusals of the host and device entries.  Compared with the oracle by ct_cases.assert_sp_close /
assert_mc_close, whose bounds tests/test_ct_cases.py guards on the CPU."""
import numpy as np
import pytest

from ct_cases import (FFT_SIZES, RATES, assert_mc_close, assert_sp_close, batch_cases, default_fft_size, edge_case,
                      fft_sizes, floor_of, gpu_inputs)

pytestmark = pytest.mark.gpu

ORDERS = (1, 15, 16, 24, 31, 32, 47, 48, 63)


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def kw():
    from kwiiyatta_amd.backend import world
    return world


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('fs', RATES)
def test_cheaptrick_edges(ko, kw, fs):
    """ct_cases.gpu_inputs(fs): main, off-grid, sub-window and one-sample case at the default fft size and every
    supported override, q1 in {-0.15, -0.09, 0, 0.3}."""
    worst = [0.0, 0.0]
    for label, x, f0, t, opt in gpu_inputs(fs):
        e = assert_sp_close(kw.cheaptrick(x, f0, t, fs, **opt), ko.cheaptrick(x, f0, t, fs, **opt), label)
        worst = [max(a, b) for a, b in zip(worst, e)]
    print(f'\nCheapTrick edges {fs}: worst frame rel {worst[0]:.3e}  worst log {worst[1]:.3e}')


def test_f0_floor_option_and_refusals(ko, kw):
    """f0_floor picks the fft size (no fft_size given); what the entries refuse, with the text on record."""
    fs = 16000
    for floor, fft in ((71.0, 1024), (40.0, 2048), (120.0, 512)):
        assert kw.get_cheaptrick_fft_size(fs, floor) == fft == ko.get_cheaptrick_fft_size(fs, floor)
        x, f0, t, _ = edge_case(fs, 2, fft)
        got = kw.cheaptrick(x, f0, t, fs, f0_floor=floor)
        assert got.shape == (len(f0), fft // 2 + 1)
        assert_sp_close(got, ko.cheaptrick(x, f0, t, fs, f0_floor=floor), f'f0_floor {floor} at {fs}')
        assert np.array_equal(got, kw.cheaptrick(x, f0, t, fs, fft_size=fft))
    x, f0, t, _ = edge_case(fs, 2)
    for bad in (0.375 * fs, 0.4 * fs, float('nan'), float('inf')):
        g = f0.copy()
        g[7] = bad
        with pytest.raises(ValueError) as e:
            kw.cheaptrick(x, g, t, fs)
        assert str(e.value) == 'cheaptrick: f0 must be below 3*fs/8'
    g = f0.copy()
    g[7] = np.nextafter(0.375 * fs, 0)          # the largest f0 the host entry takes
    assert_sp_close(kw.cheaptrick(x, g, t, fs), ko.cheaptrick(x, g, t, fs), 'f0 one rounding below 3 fs / 8')
    for fft in (256, 8192, 1000, 1536):
        with pytest.raises(ValueError) as e:
            kw.cheaptrick(x, f0, t, fs, fft_size=fft)
        assert str(e.value) == 'cheaptrick: fft_size must be a power of two in [512, 4096]'
    # f0_floor = 30 at 48 kHz asks for 8192 points: not built
    x48, f048, t48, _ = edge_case(48000, 2)
    assert kw.get_cheaptrick_fft_size(48000, 30.0) == 8192
    with pytest.raises(ValueError) as e:
        kw.cheaptrick(x48, f048, t48, 48000, f0_floor=30.0)
    assert str(e.value) == 'cheaptrick: fft_size must be a power of two in [512, 4096]'
    # 512 points at 96 kHz: the 577-sample window of the 500 Hz default does not fit (WORLD overruns its buffer)
    assert 512 not in fft_sizes(96000) and fft_sizes(48000) == FFT_SIZES
    x96, f096, t96, _ = edge_case(96000, 2)
    with pytest.raises(ValueError) as e:
        kw.cheaptrick(x96, f096, t96, 96000, fft_size=512)
    assert str(e.value) == ('cheaptrick: fft_size too short for the sampling rate (the window of the 500 Hz default '
                            'does not fit)')
    with pytest.raises(ValueError):
        ko.cheaptrick(x96, f096, t96, 96000, fft_size=512)
    with pytest.raises(ValueError) as e:
        kw.cheaptrick(x, f0, t, fs, f0_floor=0.0)
    assert str(e.value) == 'cheaptrick: f0_floor must be positive'


def _batch(ctx, utts, fs, fft, out_div, q1=-0.15):
    """kwy_cheaptrick_batch_dev on host utterances -> list of envelopes"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    K = fft // 2 + 1
    dev = [tuple(_dev(a) for a in u) for u in utts]
    sp = [torch.full((len(u[1]), K), float('nan'), dtype=torch.float64, device='cuda') for u in utts]
    torch.cuda.synchronize()
    arr = _lib.utterance_array([(d[0], d[2], d[1], o) for d, o in zip(dev, sp)])
    _lib.check(ctx, lib.kwy_cheaptrick_batch_dev(ctx.handle, arr, len(utts), fs, q1, 71.0, fft, float(out_div)))
    ctx.sync()
    return [s.cpu().numpy() for s in sp]


@pytest.mark.parametrize('fs', [8000, 44100])
def test_cheaptrick_batch_edges(ko, kw, fs):
    """kwy_cheaptrick_batch_dev on batch_cases(fs) (20 utterances, two launches): bit-equal to the single calls, with
    out_div 1 and fs; and the single calls agree with the oracle."""
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    utts = batch_cases(fs)
    fft = default_fft_size(fs)
    for out_div in (1.0, float(fs)):
        got = _batch(ctx, utts, fs, fft, out_div)
        for n, ((x, f0, t), g) in enumerate(zip(utts, got)):
            single = kw.cheaptrick(x, f0, t, fs, out_div=out_div)
            assert np.array_equal(g, single), (n, out_div)
            ref = ko.cheaptrick(x, f0, t, fs)
            assert_sp_close(g, ref / out_div if out_div != 1.0 else ref, f'batch {fs} utterance {n} out_div {out_div}')


def _mcep(ctx, utts, fs, fft, out_div, order, alpha, guard=3):
    """kwy_cheaptrick_mcep_batch_dev into one NaN-filled buffer per utterance with `guard` rows on either side"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    dev = [tuple(_dev(a) for a in u) for u in utts]
    bufs = [torch.full((len(u[1]) + 2 * guard, order + 1), float('nan'), dtype=torch.float64, device='cuda')
            for u in utts]
    outs = [b[guard:guard + len(u[1])] for b, u in zip(bufs, utts)]
    torch.cuda.synchronize()
    arr = _lib.utterance_array([(d[0], d[2], d[1], o) for d, o in zip(dev, outs)])
    _lib.check(ctx, lib.kwy_cheaptrick_mcep_batch_dev(ctx.handle, arr, len(utts), fs, -0.15, 71.0, fft, float(out_div),
                                                      order, float(alpha)))
    ctx.sync()
    res = []
    for b, u in zip(bufs, utts):
        h = b.cpu().numpy()
        assert np.isnan(h[:guard]).all() and np.isnan(h[guard + len(u[1]):]).all()     # the neighbours' rows
        res.append(h[guard:guard + len(u[1])])
    return res


# (rate, fft size): every fft size class, 512 points at the rate where it is the default and as an override
MCEP_CLASSES = [(8000, 512), (16000, 512), (16000, 1024), (48000, 2048), (96000, 4096)]


@pytest.mark.parametrize('fs,fft', MCEP_CLASSES)
def test_cheaptrick_mcep_edges(ko, fs, fft):
    """kwy_cheaptrick_mcep_batch_dev on batch_cases(fs, fft) against ko.sp2mc(ko.cheaptrick(...) / out_div): orders that
    need 1, 2, 3 and 4 coefficient blocks and sit on their edges, alpha = mcepalpha(fs), 0, -0.3 and 0.7 (at 512
    points 0.7 with order >= 32 reads the mirrored half of the cepstrum), out_div 1 and fs, every utterance, and
    nothing written outside an utterance's own T x (order + 1)."""
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import sptk
    ctx = _lib.Context(0)
    utts = batch_cases(fs, fft)
    sp = [ko.cheaptrick(x, f0, t, fs, fft_size=fft) for x, f0, t in utts]
    logsp = {1.0: sp, float(fs): [np.ascontiguousarray(s / fs) for s in sp]}
    worst = [0.0, 0.0]
    combos = [(order, alpha, out_div) for order in ORDERS for alpha in (sptk.mcepalpha(fs), 0.0, -0.3, 0.7)
              for out_div in (1.0, float(fs))]
    for order, alpha, out_div in combos:
        got = _mcep(ctx, utts, fs, fft, out_div, order, alpha)
        for n, g in enumerate(got):
            e = assert_mc_close(g, ko.sp2mc(logsp[out_div][n], order, alpha),
                                f'{fs} fft {fft} order {order} alpha {alpha} out_div {out_div} utterance {n}')
            worst = [max(a, b) for a, b in zip(worst, e)]
    print(f'\nmcep edges {fs} fft {fft}: worst rel {worst[0]:.3e}  worst c0 {worst[1]:.3e}')


def test_cheaptrick_mcep_refusals():
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    fs = 16000
    utts = batch_cases(fs)[:3]
    for order, alpha, out_div in ((0, 0.42, 1.0), (64, 0.42, 1.0), (24, 1.0, 1.0), (24, -1.0, 1.0), (24, float('nan'), 1.0),
                                  (24, 0.42, 0.0), (24, 0.42, -1.0), (24, 0.42, float('nan'))):
        with pytest.raises(ValueError) as e:
            _mcep(ctx, utts, fs, 1024, out_div, order, alpha)
        assert str(e.value) == 'cheaptrick_mcep_batch: bad argument (order 1..63)'
    with pytest.raises(ValueError) as e:
        _mcep(ctx, utts, fs, 8192, 1.0, 24, 0.42)
    assert str(e.value) == 'cheaptrick: fft_size must be a power of two in [512, 4096]'


@pytest.mark.parametrize('fs', [16000, 96000])
def test_cheaptrick_jump_ahead_edges(ko, kw, fs):
    """The main edge case on contexts whose randn table is cut to nothing and to the middle of the utterance: the
    draws beyond it come from the jump-ahead inside the kernel, every bit as from the table."""
    from kwiiyatta_amd import _lib
    x, f0, t, _ = edge_case(fs, 1)
    fft = default_fft_size(fs)
    fl = floor_of(fs, fft)
    cf0 = np.where(f0 <= fl, 500.0, f0)
    draws = np.cumsum([2 * int(1.5 * fs / f + 0.5) + 1 + fft // 2 + 1 for f in cf0])
    full = _lib.Context(0)
    want = kw.cheaptrick(x, f0, t, fs, ctx=full)
    assert_sp_close(want, ko.cheaptrick(x, f0, t, fs), f'edge {fs} main, full table')
    for limit in (0, int(draws[len(f0) // 2]) - 7):
        cut = _lib.Context(0)
        assert cut.set_randn_limit(limit) == limit
        assert np.array_equal(kw.cheaptrick(x, f0, t, fs, ctx=cut), want), limit
