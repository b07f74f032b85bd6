"""WORLD synthesis: the comparison every GPU test uses against the oracle, and synthetic inputs that reach the corners
of the pulse placement and of the rendering kernel (f0 on either side of the integer-division floor, a period equal
to the hop, single voiced / unvoiced frames, f0 one rounding below fs / 12, the periodic gate on the interpolated
aperiodicity, both clamps of the aperiodicity, negative / tiny / huge envelope rows, responses clipped at either end
of the waveform, more pulses than response slots).

A plain module, imported by tests/test_synth_edges_gpu.py and tests/test_world_gpu.py and checked without a GPU by
tests/test_synth_cases.py: the bounds below must reject small one-line bugs in the oracle itself.
"""
import numpy as np

from ct_cases import RATES, default_fft_size  # noqa: F401  (RATES: one rate per rate class, re-exported)

# Bounds: 10x the worst error the HIP kernels showed against the oracle on an MI355X over every input the GPU tests
# compare under them, rounded up to 1, 2 or 5 x 10^k.  Worst seen on the synthetic inputs:
#   local 2.6e-15  phase chain, 16 kHz, 30 s at 1250 Hz, block 206, sample 105570 (dense 96000 fft 4096, also job 18
#                  of batch_cases(96000): 2.5e-15, block 1, sample 2617; edge_case at every rate, fft size and frame
#                  period: 1.6e-15, edge 48000 main fft 512 period 5.0, block 24, sample 6340; voicing patterns 2.2e-15)
#   abs   2.4e-15  dense 96000 fft 4096, sample 2617
# The kernels place every pulse where the oracle does, to the bit, and differ by the rounding of the transforms alone.
# The oracle rebuilt in another summation order (-O3 -march=native -ffp-contract=fast, on a CPU with fused multiply-add:
# a figure of the machine that measured it; tests/test_synth_cases.py::test_oracles_own_reordering_noise re-measures
# it) stays within 1.5e-14 / 7.5e-15 of itself on these blocks wherever its time base is the oracle's own.
SYN_LOCAL_REL = 5e-14
SYN_ABS_REL = 5e-14
# Recordings are longer and louder in places: local 1.0e-14 (48 kHz recording, block 68, sample 70576), abs 6.8e-15
# (96 kHz recording, 120 frames stretched to 8192 points, sample 25054); the rebuilt oracle 2.1e-14 / 9.1e-15 (16 kHz).
SYN_LOCAL_REL_RECORDED = 2e-13
SYN_ABS_REL_RECORDED = 1e-13
# The blocks that edge_case names as badly conditioned in ANY arithmetic (claims['conditioned'], conditioned_samples):
# those within reach of a response whose pulse reads the pair of aperiodicity rows on the ceiling.  Between the two the
# periodic part is envelope x (1 - r^2) with 1 - r^2 = 2e-12 and r = (1 - w) c + w c one rounding off c or not: 1e-4
# of it.  The kernels show local 1.5e-15 (edge 16000, sp_mul 1 / fs, block 10, sample 5519) and abs 8.0e-16 (edge
# 16000 main fft 1024 period 2.5, sample 3362) there, but no kernel can be HELD closer to the oracle than the oracle
# is to itself: rebuilt as above it moves by local 3.9e-12 (edge 48000 main fft 2048 period 10.0, block 32, sample
# 33761) and abs 1.3e-13 (edge 16000 main fft 4096 period 5.0, sample 5624).  This pair is 10x the oracle's own
# figures, for these blocks alone: 2 to 5 of an edge case, none of any other input.
SYN_LOCAL_REL_CONDITIONED = 5e-11
SYN_ABS_REL_CONDITIONED = 2e-12

FFT_SIZES = (512, 1024, 2048, 4096, 8192)
FRAME_PERIODS = (5.0, 2.5, 10.0)
KWY_BATCH_MAX = 16                    # utterances per pass of launches (include/kwy.h)
GATE = 0.999                          # a pulse has a periodic part while its interpolated ap[0]^2 is at most this
SYN_SAFE = 1e-12                      # kMySafeGuardMinimum


def slots(y_length, fs):
    """SYN_SLOTS of kwy_synth.hip: the pulses rendered in parallel; those beyond take the DIRECT kernel"""
    return y_length * 640 // fs + 64


def y_length_of(T, fs, frame_period=5.0):
    return int(T * frame_period * fs / 1000)


def lowest_f0(fs, fft_size):
    """below this a frame is unvoiced: fs / fft_size + 1 with the INTEGER division of upstream WORLD"""
    return float(fs // fft_size + 1)


def wave_errors(got, ref, fft_size, conditioned=(), inside=False):
    """Both waveforms in blocks of fft_size / 2 samples; a block's scale is max |ref| over it and its two neighbours.
    Over the blocks that touch none of the sample ranges `conditioned` (inside=True: over those that do) returns
    (local, (block, sample), absolute, sample, stray): the worst block's max |got - ref| / scale and where it fell,
    max |got - ref| / max |ref| of the whole waveform (the plain difference if ref is all zero) and where, and the
    first sample at which got is not exactly 0 inside a block of scale 0 (None if there is none)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    n, B = len(ref), fft_size // 2
    if n == 0:
        return 0.0, (0, 0), 0.0, 0, None
    nb = -(-n // B)
    pad = nb * B - n
    use = np.zeros(nb, dtype=bool)
    for a, b in conditioned:
        use[max(0, int(a) // B):max(0, -(-int(b) // B))] = True
    if not inside:
        use = ~use
    d = np.abs(np.r_[got - ref, np.zeros(pad)]).reshape(nb, B) * use[:, None]
    a = np.abs(np.r_[ref, np.zeros(pad)]).reshape(nb, B).max(axis=1)
    scale = np.maximum(a, np.maximum(np.r_[0.0, a[:-1]], np.r_[a[1:], 0.0]))
    err = d.max(axis=1)
    quiet = scale == 0
    stray = None
    if (err[quiet] != 0).any():
        b = int(np.flatnonzero(quiet & (err != 0))[0])
        stray = b * B + int(np.argmax(d[b] != 0))
    rel = np.where(quiet, 0.0, err / np.where(quiet, 1.0, scale))
    b = int(np.argmax(rel))
    top = float(np.abs(ref).max())
    i = int(np.argmax(d))
    return float(rel[b]), (b, b * B + int(np.argmax(d[b]))), float(d.flat[i]) / (top if top > 0 else 1.0), i, stray


def conditioned_samples(claims, fs, fft_size, frame_period=5.0):
    """The sample ranges within reach of a response whose pulse reads a row of the frame ranges claims['conditioned']
    (rows a .. b - 1 are read by the pulses in ((a - 1) hop, b hop), a response spans fft_size / 2 to either side)."""
    hop = fs * frame_period / 1000.0
    return [(max(0, int((a - 1) * hop) - fft_size // 2), int(b * hop) + fft_size // 2 + 1)
            for a, b in claims.get('conditioned', ())]


def assert_wave_close(got, ref, fft_size, label, recording=False, conditioned=()):
    """got (HIP) against ref (oracle): same shape, finite; in every block of fft_size / 2 samples max |d| <=
    SYN_LOCAL_REL of the block's scale (max |ref| over the block and its two neighbours), no block left out; where
    that scale is 0, got is exactly 0; and max |d| <= SYN_ABS_REL max |ref|.  recording=True: the _RECORDED pair.
    The blocks that touch a sample range of `conditioned` (conditioned_samples of an edge_case) are held to the
    _CONDITIONED pair instead.  Prints the worst errors under `label` and returns those of the ordinary blocks."""
    b_loc, b_abs = (SYN_LOCAL_REL_RECORDED, SYN_ABS_REL_RECORDED) if recording else (SYN_LOCAL_REL, SYN_ABS_REL)
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.ndim == 1, (label, got.shape, ref.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all(), label
    e_loc, at_loc, e_abs, at_abs, stray = wave_errors(got, ref, fft_size, conditioned)
    c_loc, c_at_loc, c_abs, c_at_abs, c_stray = wave_errors(got, ref, fft_size, conditioned, inside=True)
    print(f'\nsynthesis {label}: {len(ref)} samples, fft {fft_size}  local rel {e_loc:.3e} at (block, sample) {at_loc}  '
          f'abs rel {e_abs:.3e} at sample {at_abs}' +
          (f'  conditioned blocks: local rel {c_loc:.3e} at {c_at_loc}  abs rel {c_abs:.3e} at {c_at_abs}'
           if len(conditioned) else ''))
    stray = c_stray if stray is None else stray
    assert stray is None, f'{label}: got {got[stray]!r} at sample {stray}, where the oracle is exactly 0 for blocks around'
    assert e_loc <= b_loc, f'{label}: max |d| / local scale {e_loc:.3e} at (block, sample) {at_loc} > {b_loc}'
    assert e_abs <= b_abs, f'{label}: max |d| / max |ref| {e_abs:.3e} at sample {at_abs} > {b_abs}'
    assert c_loc <= SYN_LOCAL_REL_CONDITIONED, (f'{label}: conditioned blocks: max |d| / local scale {c_loc:.3e} at '
                                                f'(block, sample) {c_at_loc} > {SYN_LOCAL_REL_CONDITIONED}')
    assert c_abs <= SYN_ABS_REL_CONDITIONED, (f'{label}: conditioned blocks: max |d| / max |ref| {c_abs:.3e} at sample '
                                              f'{c_at_abs} > {SYN_ABS_REL_CONDITIONED}')
    return e_loc, e_abs


# ------------------------------------------------------------------------------------------- synthetic edge cases
def _features(T, K, rng):
    """a smooth decaying envelope times a per-frame gain; an aperiodicity that rises with frequency"""
    k = np.arange(K)
    sp = np.exp(-k[None, :] / (K / 6.0)) * (1.0 + 0.3 * rng.random((T, 1))) * 1e-3 + 1e-9
    ap = np.clip(0.1 + 0.8 * k[None, :] / K + 0.05 * rng.standard_normal((T, K)), 0.001, 0.999)
    return np.ascontiguousarray(sp), np.ascontiguousarray(ap)


def _lead_in(fs, frame_period):
    """f0 of frame 0 in front of a plateau at F = 1000 / frame_period from frame 1 on, such that the phase sum reaches
    k cycles one sample after frame time k: sum_{i <= n} f0(i) = F (n - 1) from the plateau on.  The ramp over the
    first hop then has to fall 2 F short of the plateau's own sum."""
    F = 1000.0 / frame_period
    hop = fs * frame_period / 1000.0
    i = np.arange(int(np.ceil(hop)))
    return F * (1.0 - 2.0 / float((1.0 - i / hop).sum()))


def edge_case(fs, seed, fft_size=None, frame_period=5.0, short=None):
    """Deterministic synthesis input at rate fs: (f0, sp, ap, claims); 92 frames, sp / ap of fft_size / 2 + 1 bins
    (the rate's CheapTrick default if fft_size is None).  With L = fs // fft + 1 (the voicing floor, by integer
    division), R = fs / fft + 1, F = 1000 / frame_period, B = max(150, 2 L) and top = nextafter(fs / 12, 0), in turn:

      frame 0 and a plateau at F: the period equals the hop, and frame 0 is set so that the phase sum reaches whole
        cycles one sample after a frame time -- the pulse falls ON the frame time (fl == ce) or one sample later, as
        the last bit of the running sum decides; the first responses are clipped at n < 0;
      plateaus (L + R) / 2 (voiced only under the integer division), nextafter(L, 0) (unvoiced) and L (voiced), each
        between voiced frames at B, so no pulse interval grows beyond the fft size;
      a single voiced frame between unvoiced ones, a single unvoiced frame between voiced ones;
      a ramp that ends at top, the largest f0 the host entry takes;
      a stretch at about 520 Hz (several pulses per frame) where ap[:, 0] alternates between 0.9999 (its square above
        the gate) and 0.999 (below it): pulses between such frames see the interpolated value on either side of it;
      an ap row of exact 0.0; a row of 1.0 but for bin 0, followed by a row of exact 1.0: the pulses between the two
        have a periodic part of envelope x (1 - r^2) + the safeguard with 1 - r^2 = 2e-12, the ceiling's own;
      an sp row with its sign flipped, a row at 1e-13 (below the safeguard), a row at 1e+3 times its neighbours;
      voicing through the last frame: the last responses are clipped at y_length.

    short = 3, 2, 1: the first frames of (0.8 top, 0.9 top, 0) -- 2 is the shortest input that synthesises, 1 gives zeros.

    claims: frame indices (or ranges) of the above, for tests/test_synth_cases.py to check on the oracle's time base;
    claims['conditioned']: the frame ranges whose rows are badly conditioned (conditioned_samples).
    """
    N = fft_size or default_fft_size(fs)
    K = N // 2 + 1
    rng = np.random.default_rng([int(fs), int(seed), int(N), int(round(frame_period * 10)), int(short or 0)])
    F = 1000.0 / frame_period
    lead = _lead_in(fs, frame_period)
    top = np.nextafter(fs / 12.0, 0.0)
    if short:
        T = int(short)
        f0 = np.array([0.8 * top, 0.9 * top, 0.0])[:T]             # (high: several pulses within two short frames)
        sp, ap = _features(T, K, rng)
        return np.ascontiguousarray(f0), sp, ap, {'short': T}
    L = lowest_f0(fs, N)
    R = fs / N + 1.0
    B = max(150.0, 2.0 * L)
    gate_f0 = min(520.0, 0.8 * top)
    seq, c = [], {}

    def put(name, values):
        c[name] = (len(seq), len(seq) + len(values))
        seq.extend(values)

    put('lead_in', [lead])
    put('hop_period', [F] * 17)           # (at 22.05 kHz and 2.5 ms only every 8th frame time is a whole sample)
    put('b0', [B] * 2)
    put('between', [0.5 * (L + R)] * 3)
    put('b1', [B] * 2)
    put('below_floor', [np.nextafter(L, 0.0)] * 3)
    put('b2', [B] * 2)
    put('at_floor', [L] * 3)
    put('b3', [B])
    put('u0', [0.0] * 2)
    put('single_voiced', [min(max(B, 3.0 * F), 0.9 * top)])      # (high: a pulse falls within its one frame)
    put('u1', [0.0] * 2)
    put('b4', [B] * 3)
    put('single_unvoiced', [0.0])
    put('b5', [B] * 3)
    put('ramp', list(np.geomspace(1.5 * B, top, 6)[:-1]) + [top])
    put('u2', [0.0] * 2)
    put('gate', [gate_f0] * 10)
    V = min(max(B, 2.4 * F), 0.75 * top)                  # a pulse and more per frame: every row below is read
    put('clamps', [V * (1.0 + 0.2 * np.sin(k / 3.0)) for k in range(12)])
    put('rows', [V * (1.0 + 0.2 * np.cos(k / 3.0)) for k in range(12)])
    put('closing', [min(max(B, 2.4 * F), 0.9 * top)] * 4)          # two pulses and more beyond the last frame time
    f0 = np.array(seq)
    T = len(f0)
    sp, ap = _features(T, K, rng)
    g0 = c['gate'][0]
    ap[g0:g0 + 10, 0] = np.where(np.arange(10) % 2 == 0, 0.9999, 0.999)
    c['gate_above'] = tuple(range(g0, g0 + 10, 2))
    c['gate_below'] = tuple(range(g0 + 1, g0 + 10, 2))
    k0 = c['clamps'][0]
    ap[k0 + 2] = 0.0
    ap[k0 + 6, 1:] = 1.0
    ap[k0 + 7] = 1.0
    c['ap_zero'], c['ap_one_but_bin0'], c['ap_one'] = k0 + 2, k0 + 6, k0 + 7
    r0 = c['rows'][0]
    sp[r0 + 2] = -sp[r0 + 2]
    sp[r0 + 5] = 1e-13
    sp[r0 + 8] = 1e3 * sp[r0 + 8]
    c['sp_negative'], c['sp_tiny'], c['sp_huge'] = r0 + 2, r0 + 5, r0 + 8
    c['top'] = c['ramp'][1] - 1
    c['beyond_slots'] = False                      # every pulse has a response slot (dense_case: not so)
    c['conditioned'] = ((k0 + 6, k0 + 8),)             # (see SYN_LOCAL_REL_CONDITIONED)
    return np.ascontiguousarray(f0), sp, ap, c


def dense_case(fs, fft_size, factor=2.0):
    """A constant f0 one rounding below fs / 12, the limit of the host entry, for long enough that the pulses
    outnumber the response slots (f0 T' > 640 T' + 64 with T' in seconds; here by `factor` x 64): (f0, sp, ap, claims).
    About 0.2 s from 16 kHz on, 5 s at 8 kHz, where fs / 12 is 667 Hz."""
    f = np.nextafter(fs / 12.0, 0.0)
    T = max(20, int(np.ceil(factor * 64.0 / (f - 640.0) / 0.005)) + 1)
    rng = np.random.default_rng([int(fs), int(fft_size), 7])
    sp, ap = _features(T, fft_size // 2 + 1, rng)
    return np.full(T, f), sp, ap, {'beyond_slots': True}


# (rate, fft size) of tests/test_synth_edges_gpu.py::test_synthesis_beyond_the_slots: every fft size once
DENSE = ((8000, 512), (22050, 1024), (44100, 2048), (96000, 4096), (48000, 8192))


def count_pulses(ko, f0, fs, fft_size, frame_period=5.0):
    return len(ko.synth_timebase(f0, fs, frame_period, y_length_of(len(f0), fs, frame_period), fft_size)[0])


def batch_cases(fs):
    """19 jobs of mixed lengths at the rate's default fft size, more than one pass of launches takes (KWY_BATCH_MAX =
    16): cuts of edge_case inputs, a one-frame job (all zeros), an all-unvoiced job, a two-frame job and a
    dense_case: (f0, sp, ap, conditioned sample ranges) each."""
    out = []
    for k in range(15):
        f0, sp, ap, c = edge_case(fs, 100 + k)
        T = len(f0) - 5 * k - k % 2
        out.append((np.ascontiguousarray(f0[:T]), np.ascontiguousarray(sp[:T]), np.ascontiguousarray(ap[:T]),
                    conditioned_samples(c, fs, default_fft_size(fs))))
    out.insert(3, edge_case(fs, 120, short=1)[:3] + ([],))
    f0, sp, ap, _ = edge_case(fs, 121)
    out.insert(7, (np.zeros(37), np.ascontiguousarray(sp[:37]), np.ascontiguousarray(ap[:37]), []))
    out.append(edge_case(fs, 122, short=2)[:3] + ([],))
    out.append(dense_case(fs, default_fft_size(fs))[:3] + ([],))
    return out


def gpu_inputs(fs):
    """Every single-utterance input tests/test_synth_edges_gpu.py::test_synthesis_edges runs at rate fs, as
    (label, f0, sp, ap, fft_size, frame_period, conditioned sample ranges): the main case and its short forms at the
    default fft size and frame periods 5, 2.5 and 10 ms; at 16 and 48 kHz also every fft size at 5 ms."""
    N0 = default_fft_size(fs)
    runs = [(N0, fp) for fp in FRAME_PERIODS]
    if fs in (16000, 48000):
        runs += [(N, 5.0) for N in FFT_SIZES if N != N0]
    for N, fp in runs:
        for short in (None, 3, 2, 1):
            f0, sp, ap, c = edge_case(fs, 1, N, fp, short)
            yield (f'edge {fs} {"main" if short is None else f"T={short}"} fft {N} period {fp}', f0, sp, ap, N, fp,
                   conditioned_samples(c, fs, N, fp))
