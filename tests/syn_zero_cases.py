"""Inputs for the synthesis kernel's transforms that know their zeros (tests/test_syn_zero_gpu.py, recorded by
tools/record_syn_zero_bits.py into tests/golden/syn_zero_bits_parent.npz).

The noise of a pulse of at most 256 samples fills no more than the H/8 packed points a sparse first pass of the
2048-point transform takes: the cases put pulse intervals of 255, 256 and 257 samples side by side (an f0 glide
through fs / 256), voiced pulses well below 256 samples (400 Hz) with and without a periodic response, and unvoiced
stretches (a pulse every fs / 500 samples) at both ends.  22.05 kHz is given 1025 bins, so that it runs 2048 points
like 48 kHz; 16 kHz (1024 points) is the length whose code did not change.
"""
import numpy as np

SEED = 47
FRAMES = 60
RATES = (48000, 22050, 16000)          # (rate, fft size) below
FFT_SIZE = {48000: 2048, 22050: 2048, 16000: 1024}
GLIDE = (6, 30)                        # frames of the glide through fs / 256
HIGH = (30, 46)                        # frames at 400 Hz
APERIODIC = (14, 15, 36, 37, 38)       # voiced frames with ap[:, 0] > 0.9995: no periodic response
BATCH_CUT = 41                         # the second utterance of the batched run: the first frames of the case


def case(fs):
    """(f0, sp, ap) of 60 frames at 5 ms: unvoiced, a glide of the period from 253.4 to 258.6 samples, 400 Hz, unvoiced"""
    rng = np.random.default_rng([int(fs), SEED])
    T, K = FRAMES, FFT_SIZE[fs] // 2 + 1
    f0 = np.zeros(T)
    f0[GLIDE[0]:GLIDE[1]] = fs / np.linspace(253.4, 258.6, GLIDE[1] - GLIDE[0])
    f0[HIGH[0]:HIGH[1]] = 400.0
    fr = np.linspace(0.0, 1.0, K)
    env = np.exp(-6.0 * fr)[None, :] * (1.0 + 0.5 * np.cos(2 * np.pi * (3.0 * fr[None, :] + np.arange(T)[:, None] / 20.0)))
    sp = np.ascontiguousarray(1e-3 * env * np.exp(0.1 * rng.standard_normal((T, K))) + 1e-9)
    ap = np.clip(0.05 + 0.9 * fr[None, :] + 0.03 * rng.standard_normal((T, K)), 0.001, 0.999)
    ap[f0 == 0.0] = 1.0 - 1e-12
    ap[list(APERIODIC), 0] = 0.9999
    return f0, sp, np.ascontiguousarray(ap)


def batch(fs):
    """the two utterances of the batched run: the case and its first BATCH_CUT frames (which end inside the 400 Hz
    stretch); a pulse's response does not depend on the frames behind the next one, so the cut's waveform is the
    case's up to the last pulses"""
    f0, sp, ap = case(fs)
    n = BATCH_CUT
    return [(f0, sp, ap), (np.ascontiguousarray(f0[:n]), np.ascontiguousarray(sp[:n]), np.ascontiguousarray(ap[:n]))]


def y_length(T, fs, frame_period=5.0):
    return int(T * frame_period * fs / 1000)


def key(fs, k=0):
    return f'y_{fs}_{k}'


def render_single(fs, ctx=None):
    """the waveforms of batch(fs), one kwy_synthesize call each"""
    from kwiiyatta_amd.backend import world
    return [world.synthesize(f0, sp, ap, fs, 5.0, ctx=ctx) for f0, sp, ap in batch(fs)]


def render_batch(ctx, fs):
    """the waveforms of batch(fs) from one kwy_synth_plan_batch_dev + kwy_synth_render_batch_dev of two utterances"""
    import torch
    from kwiiyatta_amd import _lib
    lib = _lib.lib
    fft, fp = FFT_SIZE[fs], 5.0
    jobs = batch(fs)
    dev = [tuple(torch.from_numpy(a).cuda() for a in j) for j in jobs]
    ylens = [lib.kwy_synth_length(len(j[0]), fp, fs) for j in jobs]
    plans = [torch.zeros(lib.kwy_synth_plan_bytes(n), dtype=torch.uint8, device='cuda') for n in ylens]
    outs = [torch.full((n,), float('nan'), dtype=torch.float64, device='cuda') for n in ylens]
    torch.cuda.synchronize()
    parr = _lib.job_array(_lib.SynthPlanJob, [(d[0], len(j[0]), n, pl) for d, j, n, pl in zip(dev, jobs, ylens, plans)])
    _lib.check(ctx, lib.kwy_synth_plan_batch_dev(ctx.handle, parr, len(jobs), fft, fp, fs))
    rarr = _lib.synth_job_array([(pl, d[1], d[2], o) for pl, d, o in zip(plans, dev, outs)])
    _lib.check(ctx, lib.kwy_synth_render_batch_dev(ctx.handle, rarr, len(jobs), fft, fp, fs, 1.0))
    ctx.sync()
    return [o.cpu().numpy() for o in outs]
