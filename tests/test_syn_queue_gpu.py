"""The pulse queue of k_syn_pulse<LOG2N, false> (kwy_synth.hip): the workgroups of a rendering pass draw one ticket per
pulse from a head word in the context's arena, and a ticket names (utterance, pulse) through the running sum of the
utterances' pulse counts.  Who renders a pulse must not show in the waveform, so everything here is bit equality
between kwy_synth_render_batch_dev and the one-utterance entry kwy_synthesize_dev on the same inputs, through the C ABI,
on tiny utterances at 16 kHz (1024 points) and 48 kHz (2048 points):

  * 35 jobs (2 KWY_BATCH_MAX + 3: more than two passes whatever the pass size) of 2-60 frames: all-unvoiced tracks,
    80 Hz tracks, a track dense enough to overflow its response slots (the serial kernel runs beside the queue), jobs
    that take the memset path (one frame; one output sample), voiced tracks with unvoiced ends;
  * one 200-frame voiced utterance among fifteen 2-frame ones: nearly every ticket belongs to one utterance, several
    utterances own one pulse or none, and an utterance's last pulse has no response;
  * the head word is zero at every launch: the same call three times on one context, then captured on the context's
    stream and replayed three times, into NaN-filled outputs -- six equal results;
  * and, so that the equalities are not between two wrong waveforms, one mixed job per rate against oracle.synthesize
    at the RMS bound of tests/test_world_gpu.py::test_synthesis_parity (1e-9)."""
import numpy as np
import pytest

from synth_cases import KWY_BATCH_MAX, _features, slots

pytestmark = pytest.mark.gpu

RATES = ((16000, 1024), (48000, 2048))
FP = 5.0


def _p(a):
    from kwiiyatta_amd import _lib
    return _lib.c_vp(a.data_ptr())


def _job(f0, fs, fft, seed, ylen=None):
    """(f0, sp, ap, y_length); y_length None: the library's own for the frame count"""
    from kwiiyatta_amd import _lib
    f0 = np.ascontiguousarray(f0, dtype=np.float64)
    sp, ap = _features(len(f0), fft // 2 + 1, np.random.default_rng([seed, len(f0), fft]))
    return f0, sp, ap, int(_lib.lib.kwy_synth_length(len(f0), FP, fs)) if ylen is None else ylen


def _ends(T, hz, lead, tail):
    f0 = np.full(T, float(hz))
    f0[:lead] = 0.0
    f0[T - tail:] = 0.0
    return f0


def mix_jobs(fs, fft):
    """the 35 jobs of the first test; job 3 is the dense one, jobs 4 and 11 take the memset path"""
    jobs = []
    for k in range(2 * KWY_BATCH_MAX + 3):
        T = 2 + (13 * k + 5) % 59
        kind = k % 7
        if k == 3:
            f0 = np.full(40, 0.98 * fs / 12.0)                    # 6.5 (16 kHz) / 19.6 (48 kHz) pulses a frame
        elif k == 4:
            f0 = np.full(1, 200.0)                                # f0_length < 2
        elif kind == 0:
            f0 = np.zeros(T)
        elif kind == 1:
            f0 = np.full(T, 80.0)
        elif kind == 2:
            f0 = _ends(T, 140.0 + 3 * k, T // 4, T // 3)
        elif kind == 3:
            f0 = 200.0 + 90.0 * np.sin(np.arange(T) * 0.3 + k)
        elif kind == 4:
            f0 = np.full(T, 220.0)
        elif kind == 5:
            f0 = np.full(2, 300.0)
        else:
            f0 = _ends(T, 110.0, 0, T // 2)
        jobs.append(_job(f0, fs, fft, 1000 + k, ylen=1 if k == 11 else None))     # (job 11: y_length < 2)
    return jobs


def skew_jobs(fs, fft):
    """two frames are 10 ms: unvoiced (500 Hz) a handful of pulses, 150 Hz one, 90 Hz none"""
    jobs = [_job(np.full(2, (0.0, 90.0, 150.0)[k % 3]), fs, fft, 2000 + k) for k in range(15)]
    jobs.insert(6, _job(np.full(200, 200.0), fs, fft, 2100))
    return jobs


class Batch:
    """the jobs on the device, placed (kwy_synth_plan_batch_dev); render() enqueues kwy_synth_render_batch_dev"""
    GUARD = 5

    def __init__(self, ctx, jobs, fs, fft):
        import torch
        from kwiiyatta_amd import _lib
        self.ctx, self.jobs, self.fs, self.fft = ctx, jobs, fs, fft
        self.dev = [tuple(torch.from_numpy(a).cuda() for a in j[:3]) for j in jobs]
        self.ylens = [j[3] for j in jobs]
        lib = _lib.lib
        self.plans = [torch.zeros(max(1, lib.kwy_synth_plan_bytes(n)), dtype=torch.uint8, device='cuda') for n in self.ylens]
        self.bufs = [torch.empty(n + 2 * self.GUARD, dtype=torch.float64, device='cuda') for n in self.ylens]
        outs = [b[self.GUARD:self.GUARD + n] for b, n in zip(self.bufs, self.ylens)]
        torch.cuda.synchronize()
        parr = _lib.job_array(_lib.SynthPlanJob, [(d[0], len(j[0]), n, pl)
                                                  for d, j, n, pl in zip(self.dev, jobs, self.ylens, self.plans)])
        _lib.check(ctx, lib.kwy_synth_plan_batch_dev(ctx.handle, parr, len(jobs), fft, FP, fs))
        ctx.sync()
        self.rarr = _lib.synth_job_array([(pl, d[1], d[2], o) for pl, d, o in zip(self.plans, self.dev, outs)])

    def poison(self):
        for b in self.bufs:
            b.fill_(float('nan'))

    def render(self):
        from kwiiyatta_amd import _lib
        _lib.check(self.ctx, _lib.lib.kwy_synth_render_batch_dev(self.ctx.handle, self.rarr, len(self.jobs), self.fft, FP,
                                                                 self.fs, 1.0))

    def read(self):
        """the waveforms; the guard samples around each must still be NaN"""
        res = []
        for b, n in zip(self.bufs, self.ylens):
            h = b.cpu().numpy()
            assert np.isnan(h[:self.GUARD]).all() and np.isnan(h[self.GUARD + n:]).all()
            res.append(h[self.GUARD:self.GUARD + n])
        return res


def _single(ctx, job, fs, fft):
    """kwy_synthesize_dev on one job"""
    import torch
    from kwiiyatta_amd import _lib
    f0, sp, ap, ylen = job
    d = [torch.from_numpy(a).cuda() for a in (f0, sp, ap)]
    y = torch.full((ylen,), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    _lib.check(ctx, _lib.lib.kwy_synthesize_dev(ctx.handle, _p(d[0]), len(f0), _p(d[1]), _p(d[2]), fft, FP, fs, 1.0, ylen,
                                                _p(y)))
    ctx.sync()
    return y.cpu().numpy()


_CACHE = {}


def _mix(fs, fft):
    """(jobs, the single calls' waveforms, the batched call's waveforms): computed once per rate, read-only"""
    if fs not in _CACHE:
        from kwiiyatta_amd import _lib
        jobs = mix_jobs(fs, fft)
        want = [_single(_lib.Context(0), j, fs, fft) for j in jobs]
        b = Batch(_lib.Context(0), jobs, fs, fft)
        b.poison()
        b.render()
        b.ctx.sync()
        got = b.read()
        for a in want + got:
            a.setflags(write=False)
        _CACHE[fs] = (jobs, want, got)
    return _CACHE[fs]


def _pulses(job, fs, fft):
    from oracle import oracle
    f0, _, _, ylen = job
    return len(oracle.synth_timebase(f0, fs, FP, ylen, fft)[0]) if ylen >= 2 and len(f0) >= 2 else 0


@pytest.mark.parametrize('fs,fft', RATES)
def test_batch_equals_the_single_calls(fs, fft):
    jobs, want, got = _mix(fs, fft)
    assert len(jobs) == 2 * KWY_BATCH_MAX + 3
    assert all(2 <= len(j[0]) <= 60 for n, j in enumerate(jobs) if n != 4)
    assert _pulses(jobs[3], fs, fft) > slots(jobs[3][3], fs)                    # the serial kernel has work
    for n, (w, g) in enumerate(zip(want, got)):
        assert np.isfinite(g).all(), n
        assert np.array_equal(g, w), n
        if n in (4, 11):
            assert (g == 0).all() and len(g) > 0, n                             # the memset path
        else:
            assert np.abs(g).max() > 0, n


@pytest.mark.parametrize('fs,fft', RATES)
def test_skewed_tickets(fs, fft):
    from kwiiyatta_amd import _lib
    jobs = skew_jobs(fs, fft)
    counts = [_pulses(j, fs, fft) for j in jobs]
    assert counts[6] > 0.8 * sum(counts) and counts.count(0) >= 2 and counts.count(1) >= 2, counts
    b = Batch(_lib.Context(0), jobs, fs, fft)
    b.poison()
    b.render()
    b.ctx.sync()
    single = _lib.Context(0)
    for n, (j, g) in enumerate(zip(jobs, b.read())):
        assert np.array_equal(g, _single(single, j, fs, fft)), n
    print(f'\nsyn queue skewed {fs}: pulses per utterance {counts}')


@pytest.mark.parametrize('fs,fft', RATES)
def test_head_word_is_reset(fs, fft):
    import torch
    from kwiiyatta_amd import _lib
    jobs, want, _ = _mix(fs, fft)
    stream = torch.cuda.Stream()
    b = Batch(_lib.Context(0, stream=stream.cuda_stream), jobs, fs, fft)
    results = []
    for _ in range(3):
        with torch.cuda.stream(stream):
            b.poison()
        b.render()
        b.ctx.sync()
        results.append(b.read())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        b.render()
    b.ctx.sync()
    for _ in range(3):
        with torch.cuda.stream(stream):
            b.poison()
            graph.replay()
        stream.synchronize()
        results.append(b.read())
    for r, res in enumerate(results):
        for n, (w, g) in enumerate(zip(want, res)):
            assert np.array_equal(g, w), (r, n)


@pytest.mark.parametrize('fs,fft', RATES)
def test_against_the_oracle(fs, fft):
    from oracle import oracle
    jobs, _, got = _mix(fs, fft)
    n = 16                                  # 38 frames: unvoiced lead, voiced middle, unvoiced tail
    f0, sp, ap, ylen = jobs[n]
    assert f0[0] == 0 and f0[-1] == 0 and f0.max() > 100
    ref = oracle.synthesize(f0, sp, ap, fs, FP)
    assert len(ref) == ylen
    rms = np.sqrt(np.mean((got[n] - ref) ** 2))
    print(f'\nsyn queue oracle {fs}: rms {rms:.3e} (signal rms {np.sqrt(np.mean(ref ** 2)):.3e})')
    assert rms <= 1e-9, rms
