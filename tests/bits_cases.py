"""Inputs of the bit-for-bit comparisons against an earlier build of the library (tests/test_twiddle_powers_gpu.py):
the D4C cases and the synthesis utterances whose outputs, recorded on an MI355X, are kept under tests/golden/.

A plain module: the recorder (tests/golden/make_bits_parent.py) and the tests build their inputs here, so both see the
same arrays.  The fixtures store the commit they were recorded from and the seed.
"""
import numpy as np

from d4c_cases import FRAME_PERIOD, edge_case

SEED = 31
D4C_RATES = (16000, 32000, 48000, 96000)
D4C_F0 = (47.0, 55.0, 140.0, 400.0, 790.0)
# f0 above the C entry's fs / 5 check has to go through the device entry; these two are high enough that the first
# smoothing of the static group delay reads its input up to the last bin (kwy_d4c.hip: d4c_linear_smoothing's kmax)
D4C_HIGH = ((48000, 2400.0), (32000, 3000.0))
D4C_BIN_STEP = 8               # the fixture keeps every 8th bin and the last one of every frame
SYNTH_RATES = (16000, 48000)


def d4c_case(fs, f0_value):
    """The short edge case of d4c_cases (25 ms of a 47 Hz voice, every window clamped at both ends) under an f0 track
    at f0_value: (x, f0, t)."""
    x, f0, t, _ = edge_case(fs, SEED, short=True)
    return x, np.full(len(f0), float(f0_value)), t


def d4c_sample(ap):
    """the bins of an aperiodicity array the fixture keeps"""
    return np.ascontiguousarray(np.concatenate([ap[:, ::D4C_BIN_STEP], ap[:, -1:]], axis=1))


def d4c_key(fs, f0_value, dev=False):
    return f"{'dev' if dev else 'ap'}_{fs}_{int(f0_value)}"


def synth_case(fs):
    """0.3 s: unvoiced frames, a voiced stretch at a gliding f0 with three frames whose aperiodicity at bin 0 is above
    0.9995 (no periodic response for the pulses there), unvoiced frames again: (f0, sp, ap)."""
    from kwiiyatta_amd.backend import world
    rng = np.random.default_rng([int(fs), SEED])
    T = 60
    K = world.get_cheaptrick_fft_size(fs) // 2 + 1
    f0 = np.zeros(T)
    f0[6:38] = np.linspace(180.0, 120.0, 32)
    fr = np.linspace(0.0, 1.0, K)
    env = np.exp(-6.0 * fr)[None, :] * (1.0 + 0.5 * np.cos(2 * np.pi * (3.0 * fr[None, :] + np.arange(T)[:, None] / 20.0)))
    sp = np.ascontiguousarray(1e-3 * env * np.exp(0.1 * rng.standard_normal((T, K))) + 1e-9)
    ap = np.clip(0.05 + 0.9 * fr[None, :] + 0.03 * rng.standard_normal((T, K)), 0.001, 0.999)
    ap[f0 == 0.0] = 1.0 - 1e-12
    ap[20:23, 0] = 0.9999
    return f0, sp, np.ascontiguousarray(ap)
