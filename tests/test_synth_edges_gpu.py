"""WORLD synthesis on the GPU, through the C ABI, on the inputs of tests/synth_cases.py: every rate class, fft size
and frame period, f0 on either side of the integer-division voicing floor, a period equal to the hop, f0 one rounding
below fs / 12, the periodic gate on the interpolated aperiodicity, both aperiodicity clamps, negative / tiny / huge
envelope rows, two-frame and one-frame inputs; more pulses than response slots at every fft size; sp_mul; the noise
generator beyond the randn table at 512 and 8192 points; the host, device, plan + render and batched entries against
each other; the refusals.  Compared with the oracle by synth_cases.assert_wave_close, whose bounds
tests/test_synth_cases.py guards on the CPU."""
import numpy as np
import pytest

from synth_cases import (DENSE, RATES, assert_wave_close, batch_cases, conditioned_samples, default_fft_size, dense_case,
                         edge_case, gpu_inputs, y_length_of)

pytestmark = pytest.mark.gpu


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


def _p(a):
    from kwiiyatta_amd import _lib
    return _lib.c_vp(a.data_ptr())


@pytest.mark.parametrize('fs', RATES)
def test_synthesis_edges(ko, kw, fs):
    """synth_cases.gpu_inputs(fs): the main case and the 3-, 2- and 1-frame forms at the default fft size with frame
    periods 5, 2.5 and 10 ms; at 16 and 48 kHz also at every fft size from 512 to 8192."""
    worst = [0.0, 0.0]
    for label, f0, sp, ap, N, fp, cond in gpu_inputs(fs):
        got, ref = kw.synthesize(f0, sp, ap, fs, fp), ko.synthesize(f0, sp, ap, fs, fp)
        e = assert_wave_close(got, ref, N, label, conditioned=cond)
        worst = [max(a, b) for a, b in zip(worst, e)]
        if len(f0) == 1:
            assert (got == 0).all() and len(got) == y_length_of(1, fs, fp) > 0
    print(f'\nsynthesis edges {fs}: worst local rel {worst[0]:.3e}  worst abs rel {worst[1]:.3e}')


@pytest.mark.parametrize('fs,fft', DENSE)
def test_synthesis_beyond_the_slots(ko, kw, fs, fft):
    """dense_case: f0 one rounding below fs / 12 until the pulses outnumber the response slots -- those beyond them
    take the serial kernel (one instantiation per fft size) straight onto the waveform; same bits on a second run."""
    f0, sp, ap, _ = dense_case(fs, fft)
    got = kw.synthesize(f0, sp, ap, fs, 5.0)
    e = assert_wave_close(got, ko.synthesize(f0, sp, ap, fs, 5.0), fft, f'dense {fs} fft {fft} ({len(f0)} frames)')
    assert np.array_equal(got, kw.synthesize(f0, sp, ap, fs, 5.0))
    print(f'\nsynthesis beyond the slots {fs} fft {fft}: local rel {e[0]:.3e}  abs rel {e[1]:.3e}')


def test_sp_mul(ko, kw):
    """sp_mul scales the envelope inside the kernel: |s m| of the same product numpy forms, so the ordinary bounds
    hold against the oracle on sp * m."""
    worst = [0.0, 0.0]
    for fs in (16000, 44100):
        N = default_fft_size(fs)
        f0, sp, ap, c = edge_case(fs, 3)
        for m in (1.0 / fs, 3.0):
            ref = ko.synthesize(f0, np.ascontiguousarray(sp * m), ap, fs, 5.0)
            e = assert_wave_close(kw.synthesize(f0, sp, ap, fs, 5.0, sp_mul=m), ref, N, f'edge {fs} sp_mul {m}',
                                  conditioned=conditioned_samples(c, fs, N))
            worst = [max(a, b) for a, b in zip(worst, e)]
    print(f'\nsynthesis sp_mul: worst local rel {worst[0]:.3e}  worst abs rel {worst[1]:.3e}')


@pytest.mark.parametrize('fft', [512, 8192])
def test_jump_ahead_edges(ko, kw, fft):
    """The main edge case at 16 kHz on contexts whose randn table is cut to nothing and to the middle of the
    utterance: the noise beyond it comes from the generator inside the kernel -- at 512 points by the branch that
    combines the jump polynomials directly, at 8192 by the one that builds a table first -- every bit as from the
    table."""
    from kwiiyatta_amd import _lib
    fs = 16000
    f0, sp, ap, c = edge_case(fs, 1, fft)
    full = _lib.Context(0)
    want = kw.synthesize(f0, sp, ap, fs, 5.0, ctx=full)
    e = assert_wave_close(want, ko.synthesize(f0, sp, ap, fs, 5.0), fft, f'edge {fs} fft {fft}, full table',
                          conditioned=conditioned_samples(c, fs, fft))
    print(f'\nsynthesis jump-ahead {fft}: local rel {e[0]:.3e}  abs rel {e[1]:.3e}')
    for limit in (0, len(want) // 2 - 7):
        cut = _lib.Context(0)
        assert cut.set_randn_limit(limit) == limit
        assert np.array_equal(kw.synthesize(f0, sp, ap, fs, 5.0, ctx=cut), want), limit


def _device_entries(ctx, f0, sp, ap, fs, fft, fp=5.0):
    """kwy_synthesize_dev, and kwy_synth_plan_dev + kwy_synth_render_dev, on one utterance"""
    import torch
    from kwiiyatta_amd import _lib
    lib = _lib.lib
    T = len(f0)
    ylen = lib.kwy_synth_length(T, fp, fs)
    df0, dsp, dap = _dev(f0), _dev(sp), _dev(ap)
    whole = torch.full((ylen,), float('nan'), dtype=torch.float64, device='cuda')
    split = torch.full((ylen,), float('nan'), dtype=torch.float64, device='cuda')
    plan = torch.zeros(lib.kwy_synth_plan_bytes(ylen), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    _lib.check(ctx, lib.kwy_synthesize_dev(ctx.handle, _p(df0), T, _p(dsp), _p(dap), fft, fp, fs, 1.0, ylen, _p(whole)))
    _lib.check(ctx, lib.kwy_synth_plan_dev(ctx.handle, _p(df0), T, fft, fp, fs, ylen, _p(plan)))
    _lib.check(ctx, lib.kwy_synth_render_dev(ctx.handle, _p(plan), T, _p(dsp), _p(dap), fft, fp, fs, 1.0, ylen, _p(split)))
    ctx.sync()
    return whole.cpu().numpy(), split.cpu().numpy()


def _batched_entries(ctx, jobs, fs, fft, fp=5.0, guard=5):
    """kwy_synth_plan_batch_dev + kwy_synth_render_batch_dev into one NaN-filled buffer per job with `guard` samples on
    either side, which must stay NaN"""
    import torch
    from kwiiyatta_amd import _lib
    lib = _lib.lib
    dev = [tuple(_dev(a) for a in j[:3]) for j in jobs]
    ylens = [lib.kwy_synth_length(len(j[0]), fp, fs) for j in jobs]
    plans = [torch.zeros(lib.kwy_synth_plan_bytes(n), dtype=torch.uint8, device='cuda') for n in ylens]
    bufs = [torch.full((n + 2 * guard,), float('nan'), dtype=torch.float64, device='cuda') for n in ylens]
    outs = [b[guard:guard + n] for b, n in zip(bufs, ylens)]
    torch.cuda.synchronize()
    parr = _lib.job_array(_lib.SynthPlanJob, [(d[0], len(j[0]), n, pl) for d, j, n, pl in zip(dev, jobs, ylens, plans)])
    _lib.check(ctx, lib.kwy_synth_plan_batch_dev(ctx.handle, parr, len(jobs), fft, fp, fs))
    rarr = _lib.synth_job_array([(pl, d[1], d[2], o) for pl, d, o in zip(plans, dev, outs)])
    _lib.check(ctx, lib.kwy_synth_render_batch_dev(ctx.handle, rarr, len(jobs), fft, fp, fs, 1.0))
    ctx.sync()
    res = []
    for b, n in zip(bufs, ylens):
        h = b.cpu().numpy()
        assert np.isnan(h[:guard]).all() and np.isnan(h[guard + n:]).all()      # the neighbours' samples
        res.append(h[guard:guard + n])
    return res


@pytest.mark.parametrize('fs', [16000, 96000])
def test_entries_agree(ko, kw, fs):
    """The host entry, kwy_synthesize_dev, plan + render and the batched plan + render (batch_cases: 19 jobs, two
    passes of placement launches, five of rendering) give the same bits; the host entry's agree with the oracle."""
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    fft = default_fft_size(fs)
    f0, sp, ap, c = edge_case(fs, 1)
    host = kw.synthesize(f0, sp, ap, fs, 5.0)
    assert_wave_close(host, ko.synthesize(f0, sp, ap, fs, 5.0), fft, f'edge {fs} main, host entry',
                      conditioned=conditioned_samples(c, fs, fft))
    whole, split = _device_entries(ctx, f0, sp, ap, fs, fft)
    assert np.array_equal(whole, host) and np.array_equal(split, host)
    jobs = batch_cases(fs)
    got = _batched_entries(ctx, jobs, fs, fft)
    worst = [0.0, 0.0]
    for n, ((jf0, jsp, jap, cond), g) in enumerate(zip(jobs, got)):
        assert np.array_equal(g, kw.synthesize(jf0, jsp, jap, fs, 5.0)), n
        e = assert_wave_close(g, ko.synthesize(jf0, jsp, jap, fs, 5.0), fft, f'batch {fs} job {n} ({len(jf0)} frames)',
                              conditioned=cond)
        worst = [max(a, b) for a, b in zip(worst, e)]
        if len(jf0) == 1 or (jf0 == 0).all():
            assert len(g) > 0 and ((g == 0).all() if len(jf0) == 1 else np.abs(g).max() > 0)
    print(f'\nsynthesis batch {fs}: worst local rel {worst[0]:.3e}  worst abs rel {worst[1]:.3e}')


def test_refusals(kw):
    """what the entries refuse, with the text on record"""
    fs = 16000
    f0, sp, ap, _ = edge_case(fs, 2)
    T = len(f0)
    for fft in (256, 16384, 1000):
        bad = np.ones((T, fft // 2 + 1))
        with pytest.raises(ValueError) as e:
            kw.synthesize(f0, bad, bad, fs, 5.0)
        assert str(e.value) == 'synthesize: fft_size must be a power of two in [512, 8192]'
    for bad in (fs / 12.0, 0.1 * fs, -1.0, -1e-300, float('nan'), float('inf'), float('-inf')):
        g = f0.copy()
        g[7] = bad
        with pytest.raises(ValueError) as e:
            kw.synthesize(g, sp, ap, fs, 5.0)
        assert str(e.value) == 'synthesize: f0 must lie in [0, fs/12)'
    for a, b, c in ((f0[::2], sp[:len(f0[::2])], ap[:len(f0[::2])]), (f0, sp[:, ::2], ap[:, ::2]), (f0, sp, ap.T.copy().T),
                    (f0, np.asfortranarray(sp), ap)):
        with pytest.raises(ValueError) as e:
            kw.synthesize(a, b, c, fs, 5.0)
        assert str(e.value) == 'ndarray is not C-contiguous'
    with pytest.raises(ValueError) as e:
        kw.synthesize(f0, sp[:-1], ap[:-1], fs, 5.0)
    assert str(e.value) == 'f0, spectrogram and aperiodicity shapes do not match'
    with pytest.raises(ValueError) as e:
        kw.synthesize(f0, sp, ap, fs, 0.0)
    assert str(e.value) == 'synthesize: bad argument'
