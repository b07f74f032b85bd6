"""Inputs that sit on either side of the "half frame" switch of k_d4c_body -- a frame whose analysis window ends at
sample N/2 takes a first FFT pass that knows the zero half -- and the calls that run them.

A plain module, shared by tools/record_half_frame_bits.py (which records the outputs of the build BEFORE the change on
an MI355X) and tests/test_d4c_half_gpu.py (which holds every later build to those bits).  Signals:
d4c_cases.edge_case; tracks: constant f0 (or the MIXED pattern) on a few frame positions of it -- the first frame
(window clamped at sample 0), one in the middle, the last one (beyond the end of the signal).

wl = 2 round(2 fs / f0) + 1 samples of N = 4096 (32, 48 kHz), 2048 (16 kHz), 8192 (96 kHz); half when wl <= N/2 + 1,
i.e. f0 >= 8 fs / N.  Exactly there wl = N/2 + 1 and sample N/2 -- the packed point H/2, which only the half pass's
thread 0 reads -- is live.  threshold = 0 so that every voiced frame is analysed.
"""
import functools

import numpy as np

from d4c_cases import edge_case

SEED = 11
THRESHOLD = 0.0

# rate -> (D4C transform length, constant tracks).  8 fs / N = 93.75 Hz at 48 and 96 kHz, 62.5 Hz at 32 and 16 kHz (all
# above D4C's f0 floor of 47 Hz, so none is clamped by it): just below (dense), exactly on it, and far from it.
D4C_N = {48000: 4096, 32000: 4096, 16000: 2048, 96000: 8192}
D4C_F0 = {48000: (93.0, 93.75, 94.5, 106.0, 140.0, 185.0, 400.0, 790.0),
          32000: (62.0, 62.5, 140.0), 16000: (62.0, 62.5, 140.0), 96000: (93.0, 93.75, 140.0)}
D4C_FILE = {48000: 'd4c_half_bits_48k_parent.npz', 32000: 'd4c_half_bits_rates_parent.npz',
            16000: 'd4c_half_bits_rates_parent.npz', 96000: 'd4c_half_bits_rates_parent.npz'}
MIXED = (93.0, 140.0, 93.75, 185.0)        # dense, half, half with point H/2 live, half: one track, one utterance


def d4c_window(fs, f0):
    """(window length, whether k_d4c_body takes the half path) of a frame at f0"""
    wl = 2 * int(np.floor(2.0 * fs / max(f0, 47.0) + 0.5)) + 1
    return wl, wl <= D4C_N[fs] // 2 + 1


@functools.lru_cache(maxsize=None)
def _edge(fs):
    x, _, t, _ = edge_case(fs, SEED)
    return x, t


def signal(fs):
    """(x, t3): the edge-case signal and three frame positions: first, middle, last (beyond the end of x)"""
    x, t = _edge(fs)
    T = len(t)
    return x, np.ascontiguousarray(t[[0, T // 2, T - 1]])


def d4c_case(fs, f0):
    """constant track f0 (a number) or the MIXED pattern ('mixed') on the signal of rate fs -> (x, f0, t)"""
    x, t3 = signal(fs)
    if f0 == 'mixed':
        t = _edge(fs)[1]
        T = len(t)
        return x, np.array(MIXED), np.ascontiguousarray(t[[0, T // 3, T // 2, T - 1]])
    return x, np.full(len(t3), float(f0)), t3


def d4c_one_frame(fs):
    x, _ = signal(fs)
    return np.ascontiguousarray(x[:int(0.03 * fs)]), np.array([120.0]), np.array([0.01])


def d4c_key(fs, f0):
    return f'ap_{fs}_{f0}'


def d4c_names(fs):
    return list(D4C_F0[fs]) + (['mixed', 'one_frame'] if fs == 48000 else [])


def d4c_cases(fs):
    """name -> (x, f0, t) of every recorded D4C case of the rate"""
    return {name: d4c_one_frame(fs) if name == 'one_frame' else d4c_case(fs, name) for name in d4c_names(fs)}


def d4c_single(fs, case, ctx=None):
    from kwiiyatta_amd.backend import world
    x, f0, t = case
    return world.d4c(x, f0, t, fs, threshold=THRESHOLD, ctx=ctx)


def d4c_batch(ctx, fs, cases):
    """kwy_d4c_batch_dev on the (x, f0, t) of `cases` in one call -> list of aperiodicities"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    fft = lib.kwy_cheaptrick_fft_size(fs, 71.0)
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in u) for u in cases]
    ap = [torch.full((len(u[1]), fft // 2 + 1), float('nan'), dtype=torch.float64, device='cuda') for u in cases]
    torch.cuda.synchronize()
    arr = _lib.utterance_array([(d[0], d[2], d[1], o) for d, o in zip(dev, ap)])
    _lib.check(ctx, lib.kwy_d4c_batch_dev(ctx.handle, arr, len(cases), fs, THRESHOLD, fft))
    ctx.sync()
    return [a.cpu().numpy() for a in ap]
