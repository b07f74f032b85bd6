"""DIO / StoneMask: the comparisons every GPU test of the f0 front end uses against the oracle, the mask of frames
whose discrete decisions two correct implementations may take differently, and synthetic inputs that reach the
corners of both (f0 on the floor, on every band boundary and around the ceiling, lengths around the overlap-save
block, bands with too few zero crossings, the zero-crossing buffers' capacity, StoneMask's f0 limits, FFT-size
steps, fallbacks and windows across the ends of the signal).

A plain module, imported by tests/test_f0_edges_gpu.py and friends and checked without a GPU by
tests/test_f0_cases.py: the bounds below must reject small one-line bugs in the oracle itself, and the mask is made
from the oracle alone.
"""
import numpy as np

from d4c_cases import RATES  # noqa: F401  (the rate classes the suite runs)

# Bounds, 10x the worst error the HIP kernels showed against the oracle on an MI355X over every case of
# tests/test_f0_edges_gpu.py, test_backends_gpu.py -k dio and test_f0_finish_gpu.py -k f0, rounded up to 1, 2 or
# 5 x 10^k.
# DIO, worst seen on stable frames: 1.214e-10 Hz (48 kHz recording at frame_period 1, frame 2327, f0 158.7 Hz); next
# 1.099e-10 Hz (96 kHz recording, frame 691) and 9.9e-11 Hz (edge_case in_range at 16 kHz, allowed_range 0.5, frame
# 305); edge_case at default options stays below 5e-11 Hz on every rate.  That is the conditioning of the
# zero-crossing intervals, not a kernel's: the oracle's own track moves by 9.2e-11 Hz on that frame 2327 when the
# input is perturbed by 1e-13 of its peak (4 draws).  No voicing decision differed on a stable frame.
F0_ABS = 2e-9                  # Hz (the suite held 1e-8 before)
# StoneMask, worst seen per frame: 2.083e-12 relative (48 kHz recording on the oracle's track for allowed_range 0.5,
# frame 453, f0 136.6 Hz); the recordings give 2e-13 ... 2e-12, every synthetic case (edge_case, the sweeps of
# stonemask_case) at most 1.4e-12, mostly 5e-14.  Again the frame's conditioning (the instantaneous frequency divides
# by the power of a harmonic bin that real speech may leave nearly empty): under the same perturbation of 1e-13 the
# oracle moves by 2.1e-12 on that frame and by up to 7.4e-12 on that recording (8 draws).
F0_REL = 5e-11                 # per frame (the suite held 1e-10 of the track's maximum before)

F0_FLOOR, F0_CEIL = 71.0, 800.0
DEFAULTS = dict(f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, channels_in_octave=2.0, frame_period=5.0, allowed_range=0.1)

# the mask's constants (fixed: they do not follow F0_ABS)
MASK_DRAWS = 8
MASK_EPS = 1e-13               # about a thousand times the rounding of a double FFT filter
MASK_HZ = 1e-9
MASK_CAP = 0.02                # at most this share of a (case, option set)'s frames may be unstable

# every option set the GPU suite runs (test_dio_options), each with the form of edge_case it is paired with
OPTION_SETS = (
    dict(f0_floor=40.0),
    dict(f0_floor=50.0, f0_ceil=400.0),
    dict(f0_floor=120.0, f0_ceil=300.0),
    dict(f0_ceil=1200.0),
    dict(channels_in_octave=1.0),
    dict(channels_in_octave=2.5),
    dict(channels_in_octave=3.0),
    dict(channels_in_octave=4.0),
    dict(allowed_range=0.02),
    dict(allowed_range=0.3),
    dict(allowed_range=0.5),
    dict(frame_period=1.0),
    dict(frame_period=2.5),
    dict(frame_period=10.0),
    dict(f0_floor=60.0, f0_ceil=1000.0, channels_in_octave=3.0, allowed_range=0.05, frame_period=2.5),
    dict(f0_floor=75.0, f0_ceil=750.0, channels_in_octave=1.5, allowed_range=0.2, frame_period=4.0),
)


def option_id(o):
    return ','.join(f'{k}={v:g}' for k, v in o.items()) or 'defaults'


def wants_in_range(options):
    """With a wide allowed_range or a 1 ms frame period the frames over a fundamental above f0_ceil pick spurious
    candidates that a perturbation of 1e-13 moves; those option sets get the in_range form."""
    return options.get('allowed_range', 0.1) > 0.1 or options.get('frame_period', 5.0) < 2.5


def recording_for(fs, options):
    """Which arctic_a0001 recording test_dio_options pairs with an option set: the clb speaker's, except at 16 kHz
    with allowed_range = 0.5, where 15 of its 738 frames (2.03 %: trailing low-level frames that the oracle itself
    moves by 1e-9 ... 1.7e-9 Hz under the mask's perturbation) break the cap; the slt speaker's has 11 of 672."""
    return 'slt' if fs == 16000 and options.get('allowed_range', 0.1) >= 0.5 else 'clb'


# ----------------------------------------------------------------------------------------------- the kernel's plan
FILTER_SPAN_MAX = 8192 - 1024  # the kernel refuses 2 (round(fs / 50) + 2 max hal) above this
MAX_BANDS = 16


def band_plan(fs, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, channels_in_octave=2.0, **_):
    """Band boundaries, half filter lengths and the overlap-save block, restated from the comments of
    kwiiyatta_amd/csrc/kwy_dio.hip: boundary_i = floor 2^((i + 1) / channels), hal_i = round(fs / boundary_i / 2),
    half = round(fs / 50) + 2 max hal, a block of 8192 samples OWNS V = 8192 - 2 half - 1 outputs."""
    nbands = 1 + int(np.log(f0_ceil / f0_floor) / np.log(2.0) * channels_in_octave)
    boundary = [f0_floor * 2.0 ** ((i + 1) / channels_in_octave) for i in range(nbands)]
    hal = [int(fs / b / 2.0 + 0.5) for b in boundary]
    lh = int(fs / 50.0 + 0.5)
    half = lh + 2 * max(hal)
    return dict(nbands=nbands, boundary=boundary, hal=hal, lh=lh, half=half, V=8192 - 2 * half - 1,
                filter_span=2 * half)


def smallest_floor(fs, step=0.01):
    """the smallest f0_floor (on a grid of `step` Hz above 40 Hz) whose filters fit the overlap-save block at fs"""
    k = 0
    while band_plan(fs, f0_floor=40.0 + k * step)['filter_span'] > FILTER_SPAN_MAX:
        k += 1
    return 40.0 + k * step


def length_cases(fs, ks=(1, 2), **options):
    """Signal lengths around the overlap-save block: k V - 1, k V, k V + 1 for k in ks, plus 1, 2 and round(fs / 50)
    samples."""
    V = band_plan(fs, **options)['V']
    return [1, 2, int(fs / 50.0 + 0.5)] + [k * V + d for k in ks for d in (-1, 0, 1)]


def length_signal(fs, n, seed=0):
    """A 150 Hz tone with three harmonics plus a 1e-3 noise floor, n samples: edges of every band on both sides
    of every block seam."""
    rng = np.random.default_rng([int(fs), int(n), int(seed)])
    ph = 2.0 * np.pi * 150.0 * np.arange(n) / fs + 0.3
    x = 0.3 * (np.sin(ph) + np.sin(2 * ph) / 2 + np.sin(3 * ph) / 3) + 1e-3 * rng.standard_normal(n)
    return np.ascontiguousarray(x)


def band_signals(x, fs, **options):
    """DIO's filtered signals in numpy: the mean over n + 1 samples removed, the low-cut of 2 round(fs / 50) + 1 taps,
    one Nuttall low-pass per band.  Returns a list over bands of arrays of n + 1 samples."""
    from scipy.signal import fftconvolve
    plan = band_plan(fs, **{k: v for k, v in options.items() if k in ('f0_floor', 'f0_ceil', 'channels_in_octave')})
    x = np.asarray(x, dtype=np.float64)
    ny = len(x) + 1
    y = np.zeros(ny)
    y[:len(x)] = x
    y -= y.sum() / ny
    lh = plan['lh']
    g = 0.5 - 0.5 * np.cos(np.arange(1, 2 * lh + 2) * 2.0 * np.pi / (2 * lh + 2))
    g = -g / g.sum()
    g[lh] += 1.0
    ylc = fftconvolve(y, g)[lh:lh + ny]
    out = []
    for hal in plan['hal']:
        i = np.arange(4 * hal) / (4 * hal - 1.0)
        w = (0.355768 - 0.487396 * np.cos(2 * np.pi * i) + 0.144232 * np.cos(4 * np.pi * i)
             - 0.012604 * np.cos(6 * np.pi * i))
        out.append(fftconvolve(ylc, w)[2 * hal:2 * hal + ny])
    return out


def engine_edge_counts(x, fs, **options):
    """Negative-going zero crossings of the four engine signals (f, -f, the forward difference of -f and its
    negative) of every band: an int array [bands, 4]."""
    counts = []
    for f in band_signals(x, fs, **options):
        d = f[1:] - f[:-1]
        counts.append([int(np.sum((0.0 < s[:-1]) & (s[1:] <= 0.0))) for s in (f, -f, d, -d)])
    return np.array(counts)


def edge_cap(n):
    """edges one engine may leave per utterance of n samples (a block takes all it finds; beyond this the kernel sets
    the utterance's status word and the host entry raises)"""
    return (n + 1) // 8 + 64


CAPACITY_FS = 8000
CAPACITY_OPTIONS = dict(f0_ceil=4000.0)


def capacity_cases():
    """(over, under): 0.5 s at 8 kHz with f0_ceil = 4000 Hz (the top band's low-pass is four taps).  `over` is white
    noise, whose negative-going crossings run at about fs / 4 per second, twice the cap of fs / 8; `under` is the
    same noise smoothed over 16 samples."""
    rng = np.random.default_rng(8000)
    n = CAPACITY_FS // 2
    over = 0.1 * rng.standard_normal(n)
    under = np.convolve(0.1 * rng.standard_normal(n + 15), np.hanning(18)[1:-1] / 8.0, 'valid')
    return np.ascontiguousarray(over), np.ascontiguousarray(under)


# ------------------------------------------------------------------------------------------- synthetic edge cases
BOUNDARIES = tuple(F0_FLOOR * 2.0 ** ((i + 1) / 2.0) for i in range(7))       # 100.4 ... 803.3 Hz
BELOW_FLOOR, ABOVE_CEIL = 60.0, (803.0, 1000.0)
FULL_PLATEAUS = (BELOW_FLOOR, F0_FLOOR) + BOUNDARIES[:6] + (790.0,) + ABOVE_CEIL + (BOUNDARIES[4], BOUNDARIES[1])
IN_RANGE_PLATEAUS = (80.0,) + BOUNDARIES[:6] + (700.0, BOUNDARIES[3], BOUNDARIES[1])
SHORT_PERIODS = (2, 3, 4, 6, 9, 20)        # lengths of the short form in periods of f0_floor, chosen by seed % 6
SHORT_F0 = 1.5 * F0_FLOOR
IN_RANGE_ZEROS = 0.035


def _harmonic(f0_s, fs):
    """five harmonics 1/h along the per-sample f0 (phase = integrated f0), none above 0.45 fs"""
    ph = 2.0 * np.pi * np.cumsum(f0_s) / fs
    x = np.zeros(len(f0_s))
    for h in range(1, 6):
        x += np.where((f0_s > 0) & (h * f0_s < 0.45 * fs), np.sin(h * ph) / h, 0.0)
    return 0.25 * x


def edge_case(fs, seed, short=False, in_range=False):
    """Deterministic DIO input at rate fs: (x, claims).

    The full form (1.7 s) holds the fundamental of five harmonics 1/h on plateaus at 60 Hz (below f0_floor), 71 Hz
    (on it), on the default band boundaries 71 * 2^((i + 1) / 2) up to 568 Hz, at 790 Hz, 803 Hz and 1000 Hz (just
    below and above f0_ceil), then at 401.6 and 142 Hz again, with log-glides of 35 ms between them; after the fifth
    plateau a stretch of exact zeros (1/21 of the length), after the eighth 50 ms of noise at 0.1; a noise floor of
    1e-3 everywhere but in the zeros.  in_range=True: the same with plateaus from 80 to 700 Hz only, each 1.6 times
    as long (1.9 s in all) and 35 ms of zeros: shorter than the reach of the low-cut filter alone (2 round(fs / 50)
    samples, 40 ms), so that in every band every sample of the stretch is made of signal, none of rounding alone.
    (With a wide allowed_range the contour repair accepts any band's in-range candidate next to a voiced stretch,
    and a band whose filters see nothing but zeros offers candidates made of rounding noise, which no two
    implementations share and the mask's white perturbation does not imitate.  Seen on an MI355X with 60 ms of
    zeros at 48 kHz and allowed_range 0.5: frame 200, 12 ms into the zeros and stable by the mask, came out at
    110.0 Hz from the kernels and 0 from the oracle, and the masked frames next to it differed by 0.02 to 1.3 Hz;
    with a noise floor of 1e-9 in place of the zeros the two tracks agreed again.  So a wide allowed_range or a 1 ms
    period across a LONG stretch of digital silence is compared nowhere: ADVICE.md.)

    short=True: SHORT_PERIODS[seed % 6] periods of f0_floor of a 106.5 Hz tone plus the noise floor: so few zero
    crossings that bands have 0 to 5 edges per engine (the shortest) or just enough for a voiced stretch (the
    longest).

    claims: 'plateaus': (f, t0, t1) per plateau in seconds; 'voiced': the plateaus' fundamentals on which the oracle
    finds that fundamental; 'unvoiced': those on which it returns no frame at the fundamental (what it does return
    there at default options: nothing, no harmonic and no subharmonic); 'on_floor': the plateau that sits on
    f0_floor, where the noise floor decides every frame's `c < f0_floor`; 'boundaries': the band boundaries the
    track passes on both sides; 'few_edges' (short form): some band has fewer than 3 interval points.
    """
    rng = np.random.default_rng([int(fs), int(seed), int(short), int(in_range)])
    if short:
        periods = SHORT_PERIODS[seed % len(SHORT_PERIODS)]
        n = int(periods * fs / F0_FLOOR + 0.5)
        x = _harmonic(np.full(n, SHORT_F0), fs) + 1e-3 * rng.standard_normal(n)
        return np.ascontiguousarray(x), {'periods': periods, 'few_edges': periods <= 2, 'voiced_stretch': periods >= 9}
    plateaus = IN_RANGE_PLATEAUS if in_range else FULL_PLATEAUS
    seg, n_p = [], 0
    for k, f in enumerate(plateaus):
        if k:
            seg.append(('g', plateaus[k - 1], f, 0.035))
        seg.append(('p', f, f, (0.13 if f < 110 else 0.09 if f < 300 else 0.07) * (1.6 if in_range else 1.0)))
        n_p += 1
        if n_p == 5:
            seg.append(('z', 0.0, 0.0, IN_RANGE_ZEROS if in_range else None))
        if n_p == 8:
            seg.append(('b', 0.0, 0.0, 0.05))
    total = sum(d for _, _, _, d in seg if d) * 21.0 / 20.0       # (full form: the zeros are 1/21 of it)
    f0_s, kind, spans, pos = [], [], [], 0
    for k, a, b, d in seg:
        n = int(round((d if d else total / 21.0) * fs))
        f0_s.append(a * (b / a) ** (np.arange(n) / n) if k in 'pg' else np.zeros(n))
        kind.append(np.full(n, k))
        if k == 'p':
            spans.append((a, pos / fs, (pos + n) / fs))
        pos += n
    f0_s, kind = np.concatenate(f0_s), np.concatenate(kind)
    x = _harmonic(f0_s, fs)
    x += 1e-3 * rng.standard_normal(len(x))
    x += np.where(kind == 'b', 0.1 * rng.standard_normal(len(x)), 0.0)
    x[kind == 'z'] = 0.0
    inside = [f for f in plateaus if F0_FLOOR < f <= F0_CEIL]
    claims = {'plateaus': spans, 'voiced': inside,
              'unvoiced': [f for f in plateaus if f < F0_FLOOR or f > F0_CEIL],
              'on_floor': F0_FLOOR if F0_FLOOR in plateaus else None,
              'boundaries': list(BOUNDARIES[:6]), 'zeros': True, 'burst': True}
    return np.ascontiguousarray(x), claims


def plateau_frames(claims, t, margin=0.015):
    """per plateau (f, frame indices at least `margin` seconds inside it)"""
    return [(f, np.flatnonzero((t >= a + margin) & (t <= b - margin))) for f, a, b in claims['plateaus']]


def batch_mixed_cases(fs):
    """33 utterances (two passes of the 32-wide pass) from 1 sample to 2 s: edge cases of both forms and cuts of
    them, short forms, length cases, silence and noise."""
    out = []
    full, _ = edge_case(fs, 3)
    inr, _ = edge_case(fs, 4, in_range=True)
    out += [full, inr, np.concatenate([inr, full])[:2 * fs]]
    out += [edge_case(fs, s, short=True)[0] for s in range(6)]
    out += [length_signal(fs, n) for n in length_cases(fs)]
    rng = np.random.default_rng(fs + 33)
    out += [np.zeros(int(0.2 * fs)), 0.05 * rng.standard_normal(int(0.3 * fs))]
    k = 0
    while len(out) < 33:
        src = (full, inr)[k % 2]
        a = (k * 977) % (len(src) // 3)
        out.append(np.ascontiguousarray(src[a:a + len(src) // 2 + 131 * k]))
        k += 1
    return out


# ------------------------------------------------------------------------------------------------------ StoneMask
STONEMASK_RATES = (8000, 16000, 48000, 96000)
OFF_FACTORS = (1.25, 0.75, 2.2, 1.0 / 2.2, 1.0 / 1.195, 1.35)
LOW_FACTORS = (1.0 / 3.5, 1.0 / 4.5)


def stonemask_case(fs):
    """(x, t, f0, f0_off, f0_low): five harmonics along a log sweep of f0 from 38 Hz to fs / 11.5 over 200 frames of
    5 ms (through every FFT-size step of 2^(2 + floor(log2(2 half + 1)))), and three input tracks.

    f0: the sweep itself, every 17th frame unvoiced; frame 0 (t = 0) at 41 Hz; the frames nearest to 40 Hz and
    fs / 12 at exactly those values and the next frame at the next double above them; three more frames of fs / 12.5
    on the last sample of x and 1 and 40 ms beyond it.
    f0_off: the sweep times OFF_FACTORS in turn, so that the correction exceeds 20 % (the refined value falls back
    to the input), a correction of 19.5 % is just accepted, and at 1.25 (a correction of 20 % of the input) the sweep
    within the window decides frame by frame.  (None of these reaches the early stop: from an input of the sweep /
    2.2 the first, two-harmonic estimate lands near 1.1 times the input.)
    f0_low: the sweep times LOW_FACTORS in turn (1 / 3.5, 1 / 4.5).  Both bins of the first estimate then lie below
    the signal's fundamental and lean towards it, so that on a part of the frames the estimate exceeds twice the
    input and the refinement stops early (tests/test_f0_cases.py counts them with an instrumented oracle)."""
    T = 200
    n = int(T * 0.005 * fs)
    top = fs / 11.5
    f0_s = 38.0 * (top / 38.0) ** (np.arange(n) / n)
    rng = np.random.default_rng([int(fs), 77])
    x = np.ascontiguousarray(_harmonic(f0_s, fs) + 1e-3 * rng.standard_normal(n))
    t = np.concatenate([np.arange(T) * 0.005, [(n - 1) / fs, n / fs, (n - 1) / fs + 0.04]])
    sweep = 38.0 * (top / 38.0) ** (np.arange(T) / T)
    f0 = np.concatenate([sweep, np.full(3, fs / 12.5)])
    f0_off = f0 * np.resize(OFF_FACTORS, len(f0))
    f0_low = f0 * np.resize(LOW_FACTORS, len(f0))
    f0[::17] = 0.0
    f0[0] = 41.0
    for v in (40.0, fs / 12.0):
        k = int(np.argmin(np.abs(sweep - v)))
        k = min(max(k, 1), T - 2)
        if k % 17 == 0 or (k + 1) % 17 == 0:
            k += 2
        f0[k], f0[k + 1] = v, np.nextafter(v, np.inf)
    return (x, np.ascontiguousarray(t), np.ascontiguousarray(f0), np.ascontiguousarray(f0_off),
            np.ascontiguousarray(f0_low))


def stonemask_short_case(fs):
    """(x, t, f0): 100 samples, every window of the four frames (41 ... 200 Hz) longer than the signal"""
    rng = np.random.default_rng([int(fs), 78])
    x = np.sin(2.0 * np.pi * 200.0 * np.arange(100) / fs) + 1e-3 * rng.standard_normal(100)
    return np.ascontiguousarray(x), np.array([0.0, 50.0 / fs, 99.0 / fs, 0.01]), np.array([41.0, 100.0, 200.0, 200.0])


# --------------------------------------------------------------------------------------------------------- the mask
def stable_frames(ko, x, fs, **options):
    """Boolean mask of the frames on which two correct implementations of DIO must agree.

    DIO takes discrete decisions (edge / no edge, candidate in range, best band, contour repair), so a frame whose
    decision hangs on the last bits of the filtered signal cannot be required to agree.  The mask comes from the
    oracle `ko` alone: its track on x and on x + MASK_EPS max|x| N(0, 1) for MASK_DRAWS seeded draws; a frame is
    stable if its voicing never flips and its f0 never moves by more than MASK_HZ."""
    from concurrent.futures import ThreadPoolExecutor
    x = np.ascontiguousarray(x, dtype=np.float64)
    ref, _ = ko.dio(x, fs, **options)
    scale = MASK_EPS * float(np.abs(x).max()) if len(x) else 0.0

    def draw(k):
        rng = np.random.default_rng([20240, k])
        f0, _ = ko.dio(x + scale * rng.standard_normal(len(x)), fs, **options)
        return ((f0 > 0) == (ref > 0)) & (np.abs(f0 - ref) <= MASK_HZ)

    # (the draws side by side: the oracle is called through ctypes, without the interpreter lock, and the call
    # above has made its FFT tables for these sizes)
    with ThreadPoolExecutor(MASK_DRAWS) as pool:
        return np.logical_and.reduce(list(pool.map(draw, range(MASK_DRAWS))))


def all_frames(ref):
    return np.ones(len(ref), dtype=bool)


# -------------------------------------------------------------------------------------------------- the comparisons
def assert_f0_close(got, ref, stable, label, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, f0_abs=None):
    """got = (f0, t) of the HIP kernels against ref = (f0, t) of the oracle: same length, the temporal positions
    bit-equal, every value finite and either 0 or within [f0_floor, f0_ceil]; on the frames of `stable` the same
    voicing and |got - ref| <= F0_ABS (f0_abs: a test's own tighter bound).  Prints the worst error and its frame
    under `label`; returns it."""
    bound = F0_ABS if f0_abs is None else min(f0_abs, F0_ABS)
    (g, gt), (r, rt) = got, ref
    g, gt, r, rt, stable = np.asarray(g), np.asarray(gt), np.asarray(r), np.asarray(rt), np.asarray(stable, dtype=bool)
    assert g.shape == r.shape == gt.shape == rt.shape == stable.shape, (label, g.shape, r.shape, stable.shape)
    assert np.array_equal(gt, rt), f'{label}: temporal positions differ'
    assert np.isfinite(g).all(), label
    bad = np.flatnonzero((g != 0) & ((g < f0_floor) | (g > f0_ceil)))
    assert bad.size == 0, f'{label}: f0 outside [{f0_floor}, {f0_ceil}] on frames {bad[:16].tolist()}: {g[bad[:4]]}'
    flips = np.flatnonzero(stable & ((g > 0) != (r > 0)))
    d = np.where(stable, np.abs(g - r), 0.0)
    at = int(np.argmax(d)) if d.size else -1
    worst = float(d[at]) if d.size else 0.0
    print(f'\nDIO {label}: voiced {int((r > 0).sum())}/{len(r)}  masked {int((~stable).sum())}  '
          f'max |d| {worst:.3e} Hz at frame {at} (ref {r[at] if d.size else 0.0:.6f})')
    assert flips.size == 0, f'{label}: voicing differs on stable frames {flips[:16].tolist()}'
    assert worst <= bound, f'{label}: |d| {worst:.3e} Hz at frame {at} > {bound}'
    return worst


def assert_refined_close(got, ref, label, f0_in=None, f0_rel=None):
    """StoneMask, got (HIP) against ref (oracle): same zeros; the frames on which the oracle fell back to the input
    (ref == f0_in) bit-equal to it; elsewhere |got / ref - 1| <= F0_REL per frame (f0_rel: a test's own tighter
    bound).  Prints the worst error and its frame under `label`; returns it."""
    bound = F0_REL if f0_rel is None else min(f0_rel, F0_REL)
    g, r = np.asarray(got), np.asarray(ref)
    assert g.shape == r.shape, (label, g.shape, r.shape)
    assert np.isfinite(g).all(), label
    zeros = np.flatnonzero((g == 0) != (r == 0))
    assert zeros.size == 0, f'{label}: zeros differ on frames {zeros[:16].tolist()}'
    kept = np.zeros(len(r), dtype=bool)
    if f0_in is not None:
        kept = (r == np.asarray(f0_in)) & (r != 0)
        off = np.flatnonzero(kept & (g != r))
        assert off.size == 0, f'{label}: frames {off[:16].tolist()} do not keep the input f0 as the oracle does'
    on = (r != 0) & ~kept
    rel = np.zeros(len(r))
    rel[on] = np.abs(g[on] / r[on] - 1.0)
    at = int(np.argmax(rel)) if rel.size else -1
    worst = float(rel[at]) if rel.size else 0.0
    print(f'\nStoneMask {label}: refined {int(on.sum())}/{len(r)}  kept {int(kept.sum())}  '
          f'max rel {worst:.3e} at frame {at} (ref {r[at] if rel.size else 0.0:.6f})')
    assert worst <= bound, f'{label}: relative error {worst:.3e} at frame {at} > {bound}'
    return worst
