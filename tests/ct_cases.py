"""CheapTrick spectral envelope and its fused mel-cepstrum form: the comparisons every GPU test uses against the
oracle, and synthetic inputs that reach the corners of CheapTrick (f0 on, below and just above the effective floor
of the fft size in force, windows of a handful of samples, a closing stretch that only the noise stream fills,
frames at t = 0, on the last sample and beyond it, positions off the frame grid, a signal shorter than any window).

A plain module, imported by tests/test_ct_edges_gpu.py, tests/test_world_gpu.py and friends and checked without a
GPU by tests/test_ct_cases.py: the bounds below must reject small one-line bugs in the oracle itself.
"""
import numpy as np

from d4c_cases import FRAME_PERIOD, _harmonics

# Bounds: 10x the worst error the HIP kernels showed against the oracle on an MI355X over every input the GPU tests
# compare under them, rounded up to 1, 2 or 5 x 10^k.  Worst seen on the synthetic inputs (edge_case, batch_cases,
# make_utterance, the noise / silence / 90-sample inputs of test_edge_inputs):
#   frame rel 3.1e-12  edge 96000 single (one sample), default fft, frame 0, bin 1056
#   log       4.8e-7   edge 8000 short, fft 4096, frame 1 (f0 = nextafter(floor): a 4093-sample window over 20
#                      samples), bin 1329; the main cases stay below 1.8e-8 (96 kHz, fft 2048, frame 0 at t = 0)
# Both log figures sit on frames whose window is mostly the clamped end sample: the bins above the window's main lobe
# lie 90 dB and more below the frame's total, and LinearSmoothing differences two running sums, so such a bin carries
# an error of about eps * total / local in ANY summation order.  It is the oracle's own: with its running sum kept in
# long double the oracle moves by as much (tests/test_ct_cases.py::test_oracles_own_running_sum_error).
SP_FRAME_REL = 5e-11
SP_LOG = 5e-6
# Recordings have bins with nothing in them, and there the oracle's double running sum is the limit: on the 16 kHz
# recording (Nyquist bin) the long-double oracle moves by 1.1e-4 in log and 2.2e-10 of a frame's maximum, the kernels
# differ by 1.8e-4 (frame period 3, frame 684, bin 512) and 6.4e-10 (frame 178, bin 12); at 12 kHz both by 2.9e-6.
SP_FRAME_REL_RECORDED = 1e-8
SP_LOG_RECORDED = 2e-3
# Recordings resampled up from 16 kHz carry nothing but the 16-bit floor above 8 kHz: 3.5e-9 (96 kHz, frame 55, bin 41)
# and 6.7e-3 in log (96 kHz, frame 209, bin 2047); the long-double oracle: 1.9e-9 and 7.9e-4 at 48 kHz.
SP_FRAME_REL_UPSAMPLED = 5e-8
SP_LOG_UPSAMPLED = 1e-1
# The fused mel-cepstrum on batch_cases at every fft size class, order and alpha, and on make_utterance at 48 kHz:
#   rel 1.2e-10, c0 3.6e-10: 96 kHz, fft 4096, order 47, alpha -0.3, out_div 1, utterance 18 (the short form), frame 1;
#   without the short form 7.1e-11 / 1.5e-10 (48 kHz, utterance 4, frames at t = 0); make_utterance 1.3e-12 / 4.7e-12.
# The coefficients are sums over the log spectrum, so they inherit the running-sum error of the bins above.
MC_ABS = 2e-9
MC_C0 = 5e-9

DEFAULT_F0 = 500.0             # what CheapTrick analyses a frame with whose f0 is at or below the effective floor
FFT_SIZES = (512, 1024, 2048, 4096)
Q1S = (-0.15, -0.09, 0.0, 0.3)

# one rate per CheapTrick rate class (default fft size 512: 8 kHz; 1024: 16 and 22.05 kHz; 2048: 44.1 and 48 kHz;
# 4096: 96 kHz); 22.05 and 44.1 kHz put every other frame of the 5 ms grid on a half sample
RATES = (8000, 16000, 22050, 44100, 48000, 96000)


def default_fft_size(fs, f0_floor=71.0):
    return int(2 ** (1 + int(np.log(3.0 * fs / f0_floor + 1) / np.log(2.0))))


def floor_of(fs, fft_size):
    """the effective f0 floor of an fft size: at or below it a frame is analysed with DEFAULT_F0"""
    return 3.0 * fs / (fft_size - 3.0)


def half_window(fs, f0):
    """half the window length of a frame analysed with f0 (WORLD's matlab_round)"""
    return int(1.5 * fs / f0 + 0.5)


def fft_sizes(fs):
    """the fft sizes CheapTrick supports at rate fs: the window of the DEFAULT_F0 frames has to fit (at 96 kHz it is
    577 samples, so 512 points are refused)"""
    return tuple(N for N in FFT_SIZES if 2 * half_window(fs, DEFAULT_F0) + 1 <= N)


def sp_errors(got, ref):
    """Worst per-frame max_k |d| / max_k ref with its (frame, bin), and worst |log got - log ref| over every bin
    with its (frame, bin)."""
    d = np.abs(got - ref)
    fr = d.max(axis=1) / ref.max(axis=1)
    f = int(np.argmax(fr))
    lg = np.abs(np.log(got) - np.log(ref))
    il = np.unravel_index(np.argmax(lg), lg.shape)
    return float(fr[f]), (f, int(np.argmax(d[f]))), float(lg[il]), (int(il[0]), int(il[1]))


def assert_sp_close(got, ref, label, recording=None):
    """got (HIP) against ref (oracle): same shape, finite, positive; per frame max |d| <= SP_FRAME_REL of the frame's
    own maximum, and |log got - log ref| <= SP_LOG on every bin of every frame, no bin left out.  recording='native':
    the _RECORDED pair, for a recording at its own rate or resampled down; recording='upsampled': the _UPSAMPLED pair,
    for a recording resampled up from 16 kHz.  Prints the worst errors under `label` and returns them."""
    b_rel, b_log = {None: (SP_FRAME_REL, SP_LOG), 'native': (SP_FRAME_REL_RECORDED, SP_LOG_RECORDED),
                    'upsampled': (SP_FRAME_REL_UPSAMPLED, SP_LOG_UPSAMPLED)}[recording]
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    assert np.isfinite(got).all(), label
    assert (got > 0).all(), label
    e_rel, at_rel, e_log, at_log = sp_errors(got, ref)
    print(f'\nCheapTrick {label}: {len(ref)} x {ref.shape[1]}  frame rel {e_rel:.3e} at {at_rel}  '
          f'log {e_log:.3e} at {at_log}')
    assert e_rel <= b_rel, f'{label}: max |d| / frame max {e_rel:.3e} at (frame, bin) {at_rel} > {b_rel}'
    assert e_log <= b_log, f'{label}: max |d log| {e_log:.3e} at (frame, bin) {at_log} > {b_log}'
    return e_rel, e_log


def assert_mc_close(got, ref, label):
    """The fused mel-cepstrum (HIP) against sp2mc(cheaptrick(x) / out_div) of the oracle for one utterance: same
    shape, finite, max |d| <= MC_ABS of the utterance's max |ref|, and on c0 alone (where the log(out_div) / 2 fold
    lands) max |d| <= MC_C0.  Prints the worst errors under `label` and returns them."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    assert np.isfinite(got).all(), label
    d = np.abs(got - ref)
    ia = np.unravel_index(np.argmax(d), d.shape)
    e_abs = float(d[ia]) / float(np.abs(ref).max())
    i0 = int(np.argmax(d[:, 0]))
    e_c0 = float(d[i0, 0])
    print(f'\nmcep {label}: {len(ref)} x {ref.shape[1]}  rel {e_abs:.3e} at {(int(ia[0]), int(ia[1]))}  '
          f'c0 {e_c0:.3e} at frame {i0}')
    assert e_abs <= MC_ABS, f'{label}: max |d| / max |ref| {e_abs:.3e} at (frame, coefficient) {(int(ia[0]), int(ia[1]))} > {MC_ABS}'
    assert e_c0 <= MC_C0, f'{label}: max |d c0| {e_c0:.3e} at frame {i0} > {MC_C0}'
    return e_abs, e_c0


# ------------------------------------------------------------------------------------------- synthetic edge cases
def edge_case(fs, seed, fft_size=None, short=False, offgrid=False):
    """Deterministic CheapTrick input at rate fs for the fft size in force: (x, f0, t, claims).

    The main case (<= 0.7 s) runs f0 plateaus of 3 frames, with fl = floor_of(fs, fft size): fl (1 - 1e-12), fl,
    nextafter(fl), 1.001 fl, a value between the default floor and fl when fft_size is below the default, 120, 499,
    500 (the substituted default itself), 800, 0.2 fs, 0.3 fs, 0.3749 fs, 0 and -1, with unvoiced frames between
    voiced ones, so window lengths -- and the draw counts -- change from frame to frame.  Harmonics plus noise 30 dB
    down.  The closing stretch of 12 frames alternates 150 Hz, 0 and 0.2 fs; its first three frames are scaled by
    1e-6, the next three by 1e-9 and the rest is exact zeros: what comes out there is the noise stream, at the place
    every earlier frame left it.  Frame 0 sits at t = 0, frame T - 3 on the last sample, the last two beyond it
    with windows that see nothing but the clamped last sample (0).

    offgrid=True: the same signal with t moved off the 5 ms grid by fractions of a sample; one group of frames has
    t fs + 0.001 within 1e-3 of a half-integer, among them consecutive doubles around the tie.

    short=True: 2.5 ms of signal, less than the shortest window (3 ms each side at the 500 Hz default), six frames
    inside it: every window is clamped at both ends.  short='single': one sample, one frame.

    claims: frame indices of the properties the oracle's output on this input shows (tests/test_ct_cases.py).
    """
    N = fft_size or default_fft_size(fs)
    fl = floor_of(fs, N)
    rng = np.random.default_rng([int(fs), int(seed), int(N), {False: 0, True: 1, 'single': 2}[short]])
    if short == 'single':
        x = np.array([0.25])
        return x, np.array([120.0]), np.array([0.0]), {'single': True}
    if short:
        f0 = np.array([fl * (1 - 1e-12), np.nextafter(fl, np.inf), 120.0, 0.0, 400.0, -1.0])
        n_x = int(0.0025 * fs)
        t = np.linspace(0.0, (n_x - 1) / fs, len(f0))
        x = 0.3 * np.sin(2 * np.pi * 400.0 * np.arange(n_x) / fs + rng.uniform(0, 2 * np.pi))
        x += 0.3 * 10 ** (-30 / 20) * rng.standard_normal(n_x)
        return np.ascontiguousarray(x), f0, t, {'sub_window': True}

    nf = np.nextafter(fl, np.inf)
    seq = [120.0] * 3 + [0.0] + [fl * (1 - 1e-12)] * 3 + [fl] * 3 + [nf] * 3 + [1.001 * fl] * 3 + [0.0]
    at_floor, above_floor = 3 + 1 + 3 + 1, 3 + 1 + 6 + 1          # the middle frame of either plateau
    raised = N < default_fft_size(fs)
    if raised:
        seq += [np.sqrt(floor_of(fs, default_fft_size(fs)) * fl)] * 3
    seq += [499.0] * 3 + [500.0] * 3 + [0.0] + [800.0] * 3 + [0.2 * fs] * 3 + [-1.0] * 2
    seq += [0.3 * fs] * 3 + [0.0] + [0.3749 * fs] * 3 + [0.0] * 2
    tiny = len(seq) - 4
    closing = len(seq)
    seq += [150.0, 0.0, 0.2 * fs] * 4
    f0 = np.array(seq)
    T = len(f0)
    grid = np.arange(T) * FRAME_PERIOD
    n_x = int(grid[T - 3] * fs + 0.001 + 0.5) + 1
    frame = np.minimum(np.rint(np.arange(n_x) / (fs * FRAME_PERIOD)).astype(int), T - 1)
    f0_s = np.where(f0[frame] > 0, f0[frame], 0.0)
    x = _harmonics(f0_s, fs, rng)
    x *= 0.3 / np.sqrt(np.mean(x[f0_s > 0] ** 2))
    x += 0.3 * 10 ** (-30 / 20) * rng.standard_normal(n_x)              # noise 30 dB down
    x[frame >= closing] *= 1e-6
    x[frame >= closing + 3] *= 1e-3
    x[frame >= closing + 6] = 0.0
    t = grid.copy()
    claims = {'at_floor': at_floor, 'above_floor': above_floor, 'tiny_window': tiny, 'raised_floor': raised,
              'closing': closing, 'beyond_end': (T - 2, T - 1), 'half_sample': ()}
    if offgrid:
        # fractions of a sample, the first and the last three frames left where they are
        frac = rng.uniform(-0.45, 0.45, T)
        frac[0] = 0.0
        frac[T - 3:] = 0.0
        t = (np.rint(grid * fs) + frac) / fs
        # t fs + 0.001 within 1e-3 of a half-integer: .4985 ... .4995, then consecutive doubles around the tie
        half = list(range(4, 4 + 9)) + [closing + 1, closing + 4, closing + 7]
        for n, k in enumerate(half):
            m = np.rint(grid[k] * fs)
            if n < 5:
                t[k] = (m + 0.499 + (n - 2) * 4e-4) / fs
            else:
                tie = (m + 0.499) / fs
                for _ in range(abs(n - 8)):
                    tie = np.nextafter(tie, np.inf if n > 8 else -np.inf)
                t[k] = tie
        claims['half_sample'] = tuple(half)
    return np.ascontiguousarray(x), np.ascontiguousarray(f0), t, claims


def batch_cases(fs, fft_size=None):
    """20 utterances of mixed length for the batched calls, more than one launch takes (KWY_BATCH_MAX = 16): cuts of
    edge_case inputs (every third off the grid); at 3, 4 and 5 three utterances of 5, 2 and 4 frames, so that one
    16-row tile of k_cep2mc covers three utterances; a one-frame utterance, an all-unvoiced one, the sub-window form
    and the one-sample form."""
    out = []
    for k in range(16):
        x, f0, t, _ = edge_case(fs, 100 + k, fft_size, offgrid=k % 3 == 2)
        T = (5, 2, 4)[k - 3] if 3 <= k <= 5 else len(f0) - 3 * k - k % 2
        n = min(len(x), int(t[T - 1] * fs + 0.5) + 1 - (k % 3) * int(0.002 * fs))
        out.append((np.ascontiguousarray(x[:n]), np.ascontiguousarray(f0[:T]), t[:T].copy()))
    x, f0, t, _ = edge_case(fs, 200, fft_size)
    out.append((np.ascontiguousarray(x[:int(0.03 * fs)]), np.array([120.0]), np.array([0.01])))
    out.append((x, np.zeros_like(f0), t))
    out.append(edge_case(fs, 201, fft_size, short=True)[:3])
    out.append(edge_case(fs, 201, fft_size, short='single')[:3])
    return out


def gpu_inputs(fs):
    """Every single-utterance input tests/test_ct_edges_gpu.py::test_cheaptrick_edges runs at rate fs, as
    (label, x, f0, t, options): the default fft size and every supported override; the main case with every q1,
    the off-grid case with two, the sub-window and the one-sample case."""
    for N in (None,) + fft_sizes(fs):
        opt = {} if N is None else {'fft_size': N}
        runs = [('main', dict(), q1) for q1 in Q1S] + [('offgrid', dict(offgrid=True), q1) for q1 in (-0.15, 0.3)]
        runs += [('short', dict(short=True), -0.15), ('single', dict(short='single'), -0.15)]
        made = {}
        for name, kw, q1 in runs:
            if name not in made:
                made[name] = edge_case(fs, 1, N, **kw)[:3]
            x, f0, t = made[name]
            yield f'edge {fs} {name} fft {N or "default"} q1 {q1}', x, f0, t, dict(opt, q1=q1)
