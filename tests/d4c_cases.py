"""D4C aperiodicity: the one comparison every GPU test uses against the oracle, and synthetic inputs that reach
the corners of D4C (f0 at and below its floors, windows that cross an end of the signal, voiced frames that
LoveTrain refuses, every band count).

A plain module, imported by tests/test_world_gpu.py and friends and checked without a GPU by
tests/test_d4c_cases.py: the bounds below must reject small one-line bugs in the oracle itself.
"""
import numpy as np

# Bounds on gated rows, 10x the worst error the HIP kernels showed against the oracle on an MI355X, rounded up to
# 1, 2 or 5 x 10^k.  Worst seen: 7.5e-9 / 3.2e-7 dB (16 kHz recording at threshold 0, frame 203 / 204).  That is the
# conditioning of D4C itself, not a kernel's: LinearSmoothing differences two running sums, so a bin far below the
# running total carries an error of about eps * total / local in any summation order.  The oracle with its running
# sums kept in long double moves by the same amounts (1.8e-9 on that recording).
AP_ABS = 1e-7
AP_DB = 5e-6
# Recordings resampled up from 16 kHz have nothing above 8 kHz but the 16-bit floor, and the bands at 9, 12 and
# 15 kHz are made of it: there the long-double oracle moves by 1.1e-7 (22.05 kHz) ... 3.4e-5 (96 kHz), the kernels
# by 1.4e-7 ... 3.8e-5 (48 kHz, frame 146, bin 512 = 12 kHz).  Their abs bound stays the former 1e-4.
AP_ABS_UPSAMPLED = 1e-4
AP_DB_UPSAMPLED = 5e-3

UNGATED = 1.0 - 1e-12          # what D4C writes on every bin of a frame it does not analyse
FRAME_PERIOD = 0.005

# every rate class the D4C kernels distinguish (FFT size, band count, dense / sparse band kernel, 512 threads)
RATES = (8000, 12000, 16000, 22050, 24000, 32000, 36000, 44100, 48000, 96000)


def ap_errors(got, ref):
    """Worst |got - ref| and |20 log10(got / ref)| over the rows ref analysed, with where they occur."""
    on = ~(ref == UNGATED).all(axis=1)
    if not on.any():
        return 0.0, 0.0, None, None
    rows = np.flatnonzero(on)
    d = np.abs(got[on] - ref[on])
    db = np.abs(20.0 * np.log10(got[on] / ref[on]))
    ia, idb = np.unravel_index(np.argmax(d), d.shape), np.unravel_index(np.argmax(db), db.shape)
    return float(d[ia]), float(db[idb]), (int(rows[ia[0]]), int(ia[1])), (int(rows[idb[0]]), int(idb[1]))


def assert_ap_close(got, ref, label, upsampled=False):
    """got (HIP) against ref (oracle): same shape, finite, in (0, 1]; the same frames gated, the ungated ones
    bit-equal; on the gated ones |d| <= AP_ABS and |d| in dB <= AP_DB (the _UPSAMPLED pair for a recording
    resampled up from 16 kHz).  Prints the worst errors under `label`."""
    ap_abs, ap_db = (AP_ABS_UPSAMPLED, AP_DB_UPSAMPLED) if upsampled else (AP_ABS, AP_DB)
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    assert np.isfinite(got).all(), label
    assert ((got > 0) & (got <= 1)).all(), label
    off_ref, off_got = (ref == UNGATED).all(axis=1), (got == UNGATED).all(axis=1)
    flips = np.flatnonzero(off_ref != off_got)
    assert flips.size == 0, f'{label}: gate decision differs on frames {flips[:16].tolist()}'
    e_abs, e_db, at_abs, at_db = ap_errors(got, ref)
    print(f'\nD4C {label}: gated {int((~off_ref).sum())}/{len(ref)}  max abs {e_abs:.3e} at {at_abs}  '
          f'max dB {e_db:.3e} at {at_db}')
    assert e_abs <= ap_abs, f'{label}: max |d| {e_abs:.3e} at (frame, bin) {at_abs} > {ap_abs}'
    assert e_db <= ap_db, f'{label}: max |d| {e_db:.3e} dB at (frame, bin) {at_db} > {ap_db} dB'


# ------------------------------------------------------------------------------------------- synthetic edge cases
PLATEAUS = (30.0, 39.9, 40.0, 40.1, 46.9, 47.0, 47.1, 60.0, 120.0, 300.0, 600.0)
UNGATED_F0 = 400.0             # f0 over the high-passed noise stretches: short LoveTrain windows
HIGHPASS = 4300.0


def _harmonics(f0_s, fs, rng):
    """Harmonic signal along the per-sample f0 (phase = integrated f0), harmonic k at 1/k (-6 dB/octave),
    at most 128 harmonics, none above 0.45 fs."""
    phase = 2.0 * np.pi * np.cumsum(f0_s) / fs + rng.uniform(0, 2 * np.pi)
    y = np.zeros_like(f0_s)
    for k in range(1, 129):
        live = k * f0_s < 0.45 * fs
        if not live.any():
            break
        y += np.where(live, np.sin(k * phase) / k, 0.0)
    return y


def edge_case(fs, seed, short=False):
    """Deterministic D4C input at rate fs: (x, f0, t, claims).

    The main case (<= 0.7 s) runs f0 plateaus of >= 3 frames at 30, 39.9, 40, 40.1, 46.9, 47, 47.1, 60, 120, 300,
    600 and min(1000, 0.19 fs) Hz, broken up by unvoiced frames and by voiced stretches that carry only noise
    high-passed above 4.3 kHz (LoveTrain refuses those), so gated, voiced-ungated and unvoiced frames alternate.
    The first frame sits at t = 0, frame T - 3 on the last sample of x, and the last two frames beyond it; the
    closing plateau (from the unvoiced frames before it) is 120 dB down.

    short=True: 25 ms of signal at f0 = 47 Hz, every window clamped at both ends of x.

    claims: the properties the oracle's output on this input shows (checked by tests/test_d4c_cases.py).
    """
    rng = np.random.default_rng([int(fs), int(seed), int(short)])
    if short:
        T = 6
        f0 = np.full(T, 47.0)
        kinds = ['h'] * T
    else:
        top = min(1000.0, 0.19 * fs)
        seq = [('h', 120.0, 3), ('u', 0, 2)]
        for n, f in enumerate(PLATEAUS[:-1] + (top,)):
            seq.append(('h', f, 4 if f < 47.5 else 3))
            seq.append(('n', UNGATED_F0, 4) if n % 3 == 0 else ('u', 0, 2) if n % 3 == 1 else ('h', 600.0, 0))
        seq += [('n', UNGATED_F0, 4), ('h', 600.0, 3), ('u', 0, 2), ('h', 120.0, 5)]
        kinds, f0 = [], []
        for kind, f, n in seq:
            kinds += [kind] * n
            f0 += [f] * n
        f0 = np.array(f0)
        T = len(f0)
    t = np.arange(T) * FRAME_PERIOD
    n_x = int(t[T - 3] * fs + 0.001 + 0.5) + 1 if not short else int(0.025 * fs) + 1
    # per-sample f0 and kind: those of the nearest frame
    frame = np.minimum(np.rint(np.arange(n_x) / (fs * FRAME_PERIOD)).astype(int), T - 1)
    kind_s = np.array(kinds)[frame]
    f0_s = np.where(kind_s == 'h', f0[frame], 0.0)
    x = _harmonics(f0_s, fs, rng)
    x *= 0.3 / max(np.sqrt(np.mean(x[kind_s == 'h'] ** 2)), 1e-12)
    x += 0.3 * 10 ** (-30 / 20) * rng.standard_normal(n_x)              # noise 30 dB down
    if HIGHPASS < 0.45 * fs:
        import scipy.signal as ss
        hp = ss.sosfilt(ss.butter(8, HIGHPASS, 'highpass', fs=fs, output='sos'), rng.standard_normal(n_x))
        ungated = fs >= 12000
    else:
        hp = rng.standard_normal(n_x)   # nothing above 4 kHz to keep: LoveTrain's 7.9 kHz lies above Nyquist
        ungated = False
    x += np.where(kind_s == 'n', 0.3 * 10 ** (-10 / 20) * hp / hp.std(), 0.0)
    if not short:
        # the closing plateau 120 dB down: there D4C's 1e-12 guard noise is part of the signal, so every gated frame
        # of it shows whether both noise-offset scans found the right place in the stream
        x[frame >= T - 5 - 2] *= 1e-6
    x = np.ascontiguousarray(x)
    claims = {'below_40': not short, 'between_40_47': not short, 'voiced_ungated': ungated and not short,
              'gated_first': True, 'gated_last': True, 'beyond_end': not short, 'sub_window': short}
    return x, np.ascontiguousarray(f0), t, claims


def batch_cases(fs):
    """19 utterances of mixed length for the batched D4C call: cuts of edge_case inputs, a one-frame utterance,
    an unvoiced one and the sub-window case."""
    out = []
    for k in range(16):
        x, f0, t, _ = edge_case(fs, 100 + k)
        T = len(f0) - 4 * k - k % 2
        n = min(len(x), int(t[T - 1] * fs + 0.5) + 1 - (k % 3) * int(0.002 * fs))
        out.append((np.ascontiguousarray(x[:n]), np.ascontiguousarray(f0[:T]), t[:T].copy()))
    x, f0, t, _ = edge_case(fs, 200)
    out.append((np.ascontiguousarray(x[:int(0.03 * fs)]), np.array([120.0]), np.array([0.01])))
    out.append((x, np.zeros_like(f0), t))
    out.append(edge_case(fs, 201, short=True)[:3])
    return out
