"""CPU checks of tests/synth_cases.py, the yardstick of every synthesis parity test on the GPU.

Coverage: at every rate, the oracle's own time base and output on edge_case() show each property the case claims, so
an edit of the generator cannot silently stop reaching the corners of the pulse placement and of the rendering.

Sensitivity: one-line bugs in a scratch copy of the oracle move the waveform by as little as 1e-9 of its local scale;
assert_wave_close must reject each of them on at least one of the inputs the GPU suite uses, by either criterion
alone.  A later loosening of SYN_LOCAL_REL or SYN_ABS_REL then fails here, without a GPU.  The check that
test_world_gpu.py used alone before (rms <= 1e-9, max <= 1e-8) runs on the same mutants: the output records on how
many inputs it lets each pass.

The oracle's own noise: the same oracle built with another summation order (-O3, fused multiply-add) stays inside the
bounds on every edge case, so they ask nothing of a kernel that the reference itself does not deliver.
"""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (conftest puts the repository root on sys.path)
import synth_cases as sc
from synth_cases import (DENSE, FFT_SIZES, GATE, RATES, SYN_SAFE, assert_wave_close, batch_cases, count_pulses,
                         default_fft_size, dense_case, edge_case, gpu_inputs, lowest_f0, slots, wave_errors, y_length_of)
from test_d4c_cases import load_mutant


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


def safe_ap(x):
    return np.maximum(0.001, np.minimum(0.999999999999, x))


def pulses(ko, f0, fs, N, fp):
    """the oracle's time base: pulse index, voicing of the pulse, floor / ceil frame and the interpolation weight"""
    T = len(f0)
    idx, shift, vuv = ko.synth_timebase(f0, fs, fp, y_length_of(T, fs, fp), N)
    ct = idx / float(fs) / (fp / 1000.0)
    fl = np.minimum(T - 1, np.floor(ct).astype(int))
    ce = np.minimum(T - 1, np.ceil(ct).astype(int))
    return idx, vuv[idx] > 0.5, fl, ce, ct - fl, vuv


def main_runs():
    """(rate, fft size, frame period) of every main edge case the GPU suite runs"""
    return [(fs, r[4], r[5]) for fs in RATES for r in gpu_inputs(fs) if ' main ' in r[0]]


@pytest.mark.parametrize('fs,N,fp', main_runs())
def test_edge_case_reaches_the_corners(ko, fs, N, fp):
    assert default_fft_size(fs) == ko.get_cheaptrick_fft_size(fs)
    f0, sp, ap, c = edge_case(fs, 1, N, fp)
    again = edge_case(fs, 1, N, fp)
    assert all(np.array_equal(a, b) for a, b in zip((f0, sp, ap), again[:3])) and again[3] == c
    T, K = len(f0), N // 2 + 1
    assert T <= 100 and sp.shape == ap.shape == (T, K)
    assert ((f0 >= 0) & (f0 < fs / 12.0)).all()
    hop = fs * fp / 1000.0
    ylen = y_length_of(T, fs, fp)
    idx, voiced, fl, ce, w, vuv = pulses(ko, f0, fs, N, fp)
    ref = ko.synthesize(f0, sp, ap, fs, fp)
    assert len(ref) == ylen and np.isfinite(ref).all()
    at = lambda k: vuv[int(round(k * hop))] > 0.5                          # noqa: E731  voicing at frame time k
    mid = lambda name: (c[name][0] + c[name][1]) // 2                       # noqa: E731

    # the floor: L by integer division, R by real division, a plateau strictly between them that is voiced, one
    # rounding below L unvoiced, L itself voiced
    L, R = lowest_f0(fs, N), fs / N + 1.0
    assert L == float(int(fs) // N + 1) and L < R
    a, b = c['between']
    assert b - a >= 3 and (f0[a:b] > L).all() and (f0[a:b] < R).all() and at(mid('between'))
    a, b = c['below_floor']
    assert b - a >= 3 and (f0[a:b] == np.nextafter(L, 0.0)).all() and not at(mid('below_floor'))
    a, b = c['at_floor']
    assert b - a >= 3 and (f0[a:b] == L).all() and at(mid('at_floor'))
    for name in ('between', 'below_floor', 'at_floor'):               # voiced frames on either side
        assert at(c[name][0] - 1) and at(c[name][1])

    # the period equals the hop: the pulses of the plateau fall on a frame time or one sample after it, at least one
    # of them ON it (fl == ce inside the utterance) and the lead-in frame makes it so
    a, b = c['hop_period']
    assert (f0[a:b] == 1000.0 / fp).all() and c['lead_in'] == (0, 1) and 0 < f0[0] < f0[1]
    inside = (idx > hop) & (idx <= (b - 1) * hop + 1)
    off = idx[inside] - np.floor(np.rint(idx[inside] / hop) * hop)
    assert inside.sum() >= 6 and set(off.astype(int).tolist()) <= {0, 1}, off
    on = inside & (fl == ce)
    assert on.sum() >= 1
    assert (fl[fl < T - 1] == ce[fl < T - 1]).sum() >= on.sum()

    # single frames
    k = c['single_voiced'][0]
    assert at(k) and not at(k - 1) and not at(k + 1) and (voiced & (np.rint(idx / hop) == k)).any()
    k = c['single_unvoiced'][0]
    assert not at(k) and at(k - 1) and at(k + 1) and (~voiced & (np.rint(idx / hop) == k)).any()

    # the ramp ends one rounding below fs / 12
    assert f0[c['top']] == np.nextafter(fs / 12.0, 0.0) == f0.max() and (np.diff(f0[slice(*c['ramp'])]) > 0).all()

    # the gate: frames above and below it, and between neighbouring ones voiced pulses on either side of it
    above, below = np.array(c['gate_above']), np.array(c['gate_below'])
    assert (ap[above, 0] ** 2 > GATE).all() and (ap[below, 0] ** 2 <= GATE).all()
    assert (np.abs(above[:, None] - below[None, :]) == 1).sum() >= 8
    a, b = c['gate']
    between = voiced & (fl >= a) & (ce < b) & (fl != ce)
    rv0 = (1.0 - w) * safe_ap(ap[fl, 0]) + w * safe_ap(ap[ce, 0])
    assert (between & (rv0 ** 2 > GATE)).sum() >= 3 and (between & (rv0 ** 2 <= GATE)).sum() >= 3
    assert (voiced & (rv0 ** 2 > GATE)).sum() >= 4 and (voiced & (rv0 ** 2 <= GATE)).sum() >= 40

    # both clamps of the aperiodicity, on rows that voiced pulses read
    def read(k):
        return (voiced & ((fl == k) | (ce == k))).any()
    assert (ap[c['ap_zero']] == 0.0).all() and read(c['ap_zero'])
    k = c['ap_one_but_bin0']
    assert (ap[k, 1:] == 1.0).all() and ap[k, 0] ** 2 < GATE and (ap[k + 1] == 1.0).all() and c['ap_one'] == k + 1
    assert (voiced & (fl == k) & (ce == k + 1) & (rv0 ** 2 <= GATE)).any()     # periodic part with 1 - r^2 = 2e-12
    assert ((ap >= 0) & (ap <= 1)).all()

    # the envelope rows
    k = c['sp_negative']
    assert (sp[k] < 0).all() and read(k)
    k = c['sp_tiny']
    assert (sp[k] == 1e-13).all() and 1e-13 < SYN_SAFE and read(k)
    k = c['sp_huge']
    assert (sp[k] > 700 * sp[k - 1]).all() and (sp[k] > 700 * sp[k + 1]).all() and read(k)
    assert (np.delete(sp, [c['sp_negative']], axis=0) > 0).all()

    # voiced from frame 0 with the first response clipped at n < 0; voiced through the end, clipped at y_length
    assert at(0) and voiced[0] and idx[0] - N // 2 + 1 < 0 and ref[0] != 0.0
    assert vuv[-1] > 0.5 and voiced[-2] and idx[-2] - N // 2 + 1 + N > ylen and ref[-1] != 0.0
    # (a rendered pulse beyond the last frame time, fl == ce == T - 1 by the clamp, wherever fs / 12 allows two per hop)
    assert fl[-2] >= T - 2 and ((fl[-2] == T - 1 and ce[-2] == T - 1) or 2000.0 / fp > 0.9 * fs / 12.0)

    # all pulses have a slot; no interval is longer than the transform (the oracle's noise buffer)
    assert c['beyond_slots'] == (len(idx) > slots(ylen, fs)) and not c['beyond_slots']
    assert np.diff(idx).max() <= N and 1000.0 / fp >= L
    # the conditioned blocks: around the ceiling pair, a small part of the case unless the transform spans it
    cond = sc.conditioned_samples(c, fs, N, fp)
    k = c['ap_one_but_bin0']
    assert c['conditioned'] == ((k, k + 2),) and cond == [(max(0, int((k - 1) * hop) - N // 2), int((k + 2) * hop) + N // 2 + 1)]
    assert cond[0][1] - cond[0][0] <= N + 3 * hop + 2

    # the short forms
    for n in (3, 2, 1):
        s0, ssp, sap, sc_ = edge_case(fs, 1, N, fp, short=n)
        assert len(s0) == n and ssp.shape == sap.shape == (n, K) and sc_ == {'short': n}
        y = ko.synthesize(s0, ssp, sap, fs, fp)
        assert len(y) == y_length_of(n, fs, fp) and ((y == 0).all() if n == 1 else np.abs(y).max() > 1e-4)


def test_sizes_and_periods():
    assert FFT_SIZES == (512, 1024, 2048, 4096, 8192) and sc.FRAME_PERIODS == (5.0, 2.5, 10.0)
    for fs in RATES:
        labels = [r[0] for r in gpu_inputs(fs)]
        assert len(labels) == len(set(labels)) == 4 * (3 + (4 if fs in (16000, 48000) else 0))
    assert sorted(N for _, N in DENSE) == list(FFT_SIZES) and set(fs for fs, _ in DENSE) <= set(RATES)


@pytest.mark.parametrize('fs,fft', DENSE)
def test_dense_case_goes_beyond_the_slots(ko, fs, fft):
    f0, sp, ap, c = dense_case(fs, fft)
    T = len(f0)
    assert (f0 == np.nextafter(fs / 12.0, 0.0)).all() and sp.shape == ap.shape == (T, fft // 2 + 1)
    assert T <= 100 or fs == 8000
    n = count_pulses(ko, f0, fs, fft)
    assert c['beyond_slots'] and n > slots(y_length_of(T, fs), fs) + 32, (n, slots(y_length_of(T, fs), fs))
    assert n <= y_length_of(T, fs) // 8 + 16                       # the plan's pulse capacity


@pytest.mark.parametrize('fs', RATES)
def test_batch_cases(ko, fs):
    jobs = batch_cases(fs)
    N = default_fft_size(fs)
    assert len(jobs) >= sc.KWY_BATCH_MAX + 2 == 18
    T = [len(j[0]) for j in jobs]
    assert all(j[1].shape == j[2].shape == (len(j[0]), N // 2 + 1) for j in jobs)
    assert len(set(T)) >= 12 and 1 in T and 2 in T
    assert any((j[0] == 0).all() and len(j[0]) > 2 for j in jobs)
    assert sum(n >= 2 for n in T) > sc.KWY_BATCH_MAX                # two passes of placement launches
    f0 = jobs[-1][0]
    assert count_pulses(ko, f0, fs, N) > slots(y_length_of(len(f0), fs), fs)


def test_wave_errors():
    """a single-sample error inside a quiet block is reported at that block, at its own scale; a nonzero sample where
    the oracle is exactly zero around fails; neighbours lend their scale"""
    N = 512
    ref = np.zeros(8 * 256)
    ref[:256] = 1.0                         # block 0 loud
    ref[3 * 256:4 * 256] = 1e-6             # block 3 quiet, blocks 2 and 4 silent but beside it, 5.. silent
    got = ref.copy()
    got[3 * 256 + 17] += 1e-12
    e_loc, at_loc, e_abs, at_abs, stray = wave_errors(got, ref, N)
    assert at_loc == (3, 3 * 256 + 17) and at_abs == 3 * 256 + 17 and stray is None
    assert abs(e_loc - 1e-6) < 1e-9 and abs(e_abs - 1e-12) < 1e-15
    with pytest.raises(AssertionError, match='local scale'):
        assert_wave_close(got, ref, N, 'quiet block')
    assert_wave_close(ref, ref, N, 'equal')
    got = ref.copy()
    got[2 * 256 + 5] = 1e-15                # block 2: silent itself, scaled by its neighbour
    assert wave_errors(got, ref, N)[1] == (2, 2 * 256 + 5) and wave_errors(got, ref, N)[4] is None
    got = ref.copy()
    got[6 * 256 + 3] = 1e-300               # block 6: silent, and so are 5 and 7
    assert wave_errors(got, ref, N)[4] == 6 * 256 + 3
    with pytest.raises(AssertionError, match='exactly 0'):
        assert_wave_close(got, ref, N, 'stray sample')
    got = np.zeros(700)
    got[699] = 1e-300                       # an all-zero reference (one frame), last partial block
    assert wave_errors(got, np.zeros(700), N)[4] == 699
    with pytest.raises(AssertionError):
        assert_wave_close(np.zeros(699), np.zeros(700), N, 'length')
    with pytest.raises(AssertionError):
        assert_wave_close(np.r_[ref[:-1], np.nan], ref, N, 'nan')
    # the absolute criterion alone: a loud block beside the error hides it locally at a size that max |ref| shows
    assert sc.SYN_ABS_REL <= sc.SYN_LOCAL_REL and sc.SYN_ABS_REL_RECORDED <= sc.SYN_LOCAL_REL_RECORDED
    # conditioned sample ranges: the blocks they touch answer to the _CONDITIONED pair, the others to the ordinary one
    got = ref.copy()
    got[3 * 256 + 17] += 1e-6 * 1e-12
    got[40] += 1e-12
    cond = [(3 * 256 + 200, 3 * 256 + 201)]
    assert wave_errors(got, ref, N, cond)[1] == (0, 40) and wave_errors(got, ref, N, cond, inside=True)[1] == (3, 3 * 256 + 17)
    assert sc.SYN_LOCAL_REL < 1e-12 < sc.SYN_LOCAL_REL_CONDITIONED
    with pytest.raises(AssertionError, match='local scale'):
        assert_wave_close(got, ref, N, 'the ordinary block fails', conditioned=cond)
    got[40] = ref[40]
    assert_wave_close(got, ref, N, 'the conditioned block passes', conditioned=cond)
    with pytest.raises(AssertionError, match='local scale'):
        assert_wave_close(got, ref, N, 'not when it is an ordinary one')


# one-line edits of oracle/ko_world.c: (name, text, replacement)
MUTANTS = [
    ('fractional pulse shift biased by 1e-7 sample',
     'pulse_time_shift[number_of_pulses] = xx / fs;', 'pulse_time_shift[number_of_pulses] = (xx + 1e-7) / fs;'),
    ('fractional pulse shift biased by 1e-11 sample',
     'pulse_time_shift[number_of_pulses] = xx / fs;', 'pulse_time_shift[number_of_pulses] = (xx + 1e-11) / fs;'),
    ('GetSafeAperiodicity ceiling 1 - 1e-12 -> 1 - 1e-11',
     'return dmax(0.001, dmin(0.999999999999, x));', 'return dmax(0.001, dmin(0.99999999999, x));'),
    ('GetSafeAperiodicity floor 0.001 -> 0.0011',
     'return dmax(0.001, dmin(0.999999999999, x));', 'return dmax(0.0011, dmin(0.999999999999, x));'),
    ('lowest_f0 by real division',
     'double lowest_f0 = fs / fft_size + 1.0; /* integer division, as upstream */',
     'double lowest_f0 = (double)fs / fft_size + 1.0;'),
    ('periodic gate removed',
     'if (current_vuv <= 0.5 || aperiodic_ratio[0] > 0.999) {', 'if (current_vuv <= 0.5) {'),
    ('periodic kMySafeGuardMinimum dropped',
     'log(spectral_envelope[i] * (1.0 - aperiodic_ratio[i]) +\n                              kMySafeGuardMinimum) / 2.0;',
     'log(spectral_envelope[i] * (1.0 - aperiodic_ratio[i]) +\n                              0.0) / 2.0;'),
    ('dc sum starts one sample late',
     'for (int i = half; i < fft_size; ++i) dc_component += periodic_response[i];',
     'for (int i = half + 1; i < fft_size; ++i) dc_component += periodic_response[i];'),
    ('noise mean divided by noise_size + 1',
     '      average /= noise_size;\n      for (int i = 0; i < noise_size; ++i) wave[i] -= average;',
     '      average /= noise_size + 1;\n      for (int i = 0; i < noise_size; ++i) wave[i] -= average;'),
    ('last response sample not added',
     'int upper_limit = (int)((y_length - offset) < fft_size ? (y_length - offset) : fft_size);',
     'int upper_limit = (int)((y_length - offset) < fft_size - 1 ? (y_length - offset) : fft_size - 1);'),
    ('Nyquist bin left out of the fractional shift',
     '      for (int i = 0; i <= half; ++i) {\n        double re = mps[2 * i], im = mps[2 * i + 1];',
     '      for (int i = 0; i < half; ++i) {\n        double re = mps[2 * i], im = mps[2 * i + 1];'),
    ('Nyquist bin left out of the aperiodic product',
     '      for (int i = 0; i <= half; ++i) {\n        ispec[2 * i] = mps[2 * i] * nspec[2 * i]',
     '      for (int i = 0; i < half; ++i) {\n        ispec[2 * i] = mps[2 * i] * nspec[2 * i]'),
]


def former_passes(got, ref):
    """what tests/test_world_gpu.py asked of a synthesised waveform before: rms <= 1e-9 and max <= 1e-8"""
    d = got - ref
    with np.errstate(over='ignore'):
        return bool(np.sqrt(np.mean(d ** 2)) <= 1e-9 and np.abs(d).max() <= 1e-8)


@pytest.fixture(scope='module')
def inputs(ko):
    """The GPU suite's synthetic single-utterance inputs, cheapest first (rates in rising order, within a rate the
    short transforms first), each with its conditioned sample ranges and the oracle's waveform."""
    out = []
    for fs in sorted(RATES):
        rows = sorted((r for r in gpu_inputs(fs) if ' main ' in r[0]), key=lambda r: (r[5] != 5.0, r[4]))
        out += [(label, f0, sp, ap, fs, N, fp, cond, ko.synthesize(f0, sp, ap, fs, fp))
                for label, f0, sp, ap, N, fp, cond in rows]
    return out


def criteria(got, ref, N, cond):
    """the two criteria of assert_wave_close apart: (local, where) and (absolute, where) over the ordinary blocks, each
    None unless beyond SYN_LOCAL_REL / SYN_ABS_REL; failing that, over the conditioned blocks beyond their own pair"""
    e_loc, at_loc, e_abs, at_abs, _ = wave_errors(got, ref, N, cond)
    c_loc, c_at_loc, c_abs, c_at_abs, _ = wave_errors(got, ref, N, cond, inside=True)
    loc = (e_loc, at_loc) if e_loc > sc.SYN_LOCAL_REL else (c_loc, c_at_loc) if c_loc > sc.SYN_LOCAL_REL_CONDITIONED else None
    ab = (e_abs, at_abs) if e_abs > sc.SYN_ABS_REL else (c_abs, c_at_abs) if c_abs > sc.SYN_ABS_REL_CONDITIONED else None
    return loc, ab


# the mutants that the ordinary blocks have to reject under SYN_LOCAL_REL alone and under SYN_ABS_REL alone, whatever
# the conditioned blocks say.  Of the others only the ceiling mutant has to rely on the conditioned pair: it lives on
# the rows those blocks surround, where it shows 2e-7 against 5e-11; the remaining nine fail on ordinary blocks too,
# by many orders of magnitude.
TIGHT_PAIR_REJECTS = {'fractional pulse shift biased by 1e-7 sample', 'fractional pulse shift biased by 1e-11 sample'}


@pytest.mark.parametrize('name,text,replacement', MUTANTS, ids=[m[0] for m in MUTANTS])
def test_bounds_reject_one_line_bugs(ko, inputs, tmp_path, capsys, name, text, replacement):
    """Each mutant must fail assert_wave_close on an input of the GPU suite, checked as the GPU suite checks it (the
    conditioned blocks of edge_case under their own pair) -- by the local criterion alone, and by the absolute one
    alone.  This is the test that fails when a bound is loosened until a listed mutant passes: the smallest of them, a
    pulse shift biased by 1e-11 sample, moves the waveform by 1e-11 of its scale, 200 x SYN_LOCAL_REL."""
    mutant = load_mutant(tmp_path, name, text, replacement)
    rejected, by_loc, by_abs, former, tight = None, None, None, [], [False, False]
    for label, f0, sp, ap, fs, N, fp, cond, ref in inputs:
        got = mutant.synthesize(f0, sp, ap, fs, fp)
        former.append(former_passes(got, ref))
        loc, ab = criteria(got, ref, N, cond)
        e = wave_errors(got, ref, N, cond)
        tight = [tight[0] or e[0] > sc.SYN_LOCAL_REL, tight[1] or e[2] > sc.SYN_ABS_REL]
        if loc and not by_loc:
            by_loc = f'{loc[0]:.3e} at (block, sample) {loc[1]} on {label}'
        if ab and not by_abs:
            by_abs = f'{ab[0]:.3e} at sample {ab[1]} on {label}'
        if not rejected:
            try:
                assert_wave_close(got, ref, N, f'{name} / {label}', conditioned=cond)
            except AssertionError as e:
                rejected = f'rejected: {name} on {label}: {str(e).splitlines()[0]}'
        if rejected and by_loc and by_abs and all(tight) and len(former) >= 6:
            break
    capsys.readouterr()                                     # (drop the per-input lines of the inputs that passed)
    with capsys.disabled():
        print(f'\n{rejected or "NOT rejected: " + name}\n    local criterion alone: {by_loc}; absolute criterion alone: '
              f'{by_abs}\n    the former check (rms 1e-9, max 1e-8) passes it on {sum(former)} of {len(former)} inputs tried')
    assert rejected, f'no input tells "{name}" from the oracle within the bounds of synth_cases'
    assert by_loc, f'no input tells "{name}" from the oracle by the local criterion'
    assert by_abs, f'no input tells "{name}" from the oracle by the absolute criterion'
    assert all(tight) or name not in TIGHT_PAIR_REJECTS, f'SYN_LOCAL_REL, SYN_ABS_REL alone reject "{name}": {tight}'


FMA_BUILD = ('built with -O3 -march=native -ffp-contract=fast', 'Makefile',
             'CFLAGS ?= -O2 -fPIC -std=gnu99 -Wall -Wno-unused-function -ffp-contract=off',
             'CFLAGS ?= -O3 -fPIC -std=gnu99 -march=native -ffp-contract=fast')


def test_oracles_own_reordering_noise(ko, inputs, tmp_path):
    """Where the bounds of synth_cases.py may not go.  The same oracle in another summation order (-O3, and fused
    multiply-add where the CPU has it: the figures depend on the machine) is no less right.  Against the oracle it
      * keeps every pulse on its sample, and on most inputs every fractional shift to the bit.  Then it stays inside
        SYN_LOCAL_REL / SYN_ABS_REL on the ordinary blocks and inside the _CONDITIONED pair on the blocks edge_case
        names (around the pair of aperiodicity rows on the ceiling), on the dense cases throughout, and
        inside the _RECORDED pair on a recording: each pair asks nothing that the reference alone does not deliver;
      * on some inputs moves fractional shifts in their last bits (interp1's a + w (b - a) fuses, one bit of the phase
        sum is eps x cycles x fs / (2 pi f0) of a sample, and every later pulse inherits it).  That is another time
        base, which the kernels reproduce to the bit and no GPU test varies: the shifts stay within 1e-9 sample and
        the waveform inside the _CONDITIONED pair everywhere."""
    from scipy.io import wavfile
    from conftest import CLB_WAV
    name, file, text, replacement = FMA_BUILD
    fma = load_mutant(tmp_path, name, text, replacement, file)
    worst, where, moved = [0.0, 0.0, 0.0, 0.0], ['', '', '', ''], []
    rows = list(inputs)
    for fs, N in DENSE:
        f0, sp, ap, _ = dense_case(fs, N)
        rows.append((f'dense {fs} fft {N}', f0, sp, ap, fs, N, 5.0, [], ko.synthesize(f0, sp, ap, fs, 5.0)))
    for label, f0, sp, ap, fs, N, fp, cond, ref in rows:
        ylen = y_length_of(len(f0), fs, fp)
        i0, s0, v0 = ko.synth_timebase(f0, fs, fp, ylen, N)
        i1, s1, v1 = fma.synth_timebase(f0, fs, fp, ylen, N)
        assert np.array_equal(i0, i1) and np.array_equal(v0, v1), label
        got = fma.synthesize(f0, sp, ap, fs, fp)
        if np.array_equal(s0, s1):
            assert_wave_close(got, ref, N, f'fma / {label}', conditioned=cond)
            e = wave_errors(got, ref, N, cond), wave_errors(got, ref, N, cond, inside=True)
        else:
            moved.append(label)
            assert np.abs(s1 - s0).max() * fs <= 1e-9, label
            assert_wave_close(got, ref, N, f'fma / {label}, shifts moved', conditioned=[(0, len(ref))])
            e = (0.0, None, 0.0), wave_errors(got, ref, N)
        for n, v in enumerate((e[0][0], e[0][2], e[1][0], e[1][2])):
            if v > worst[n]:
                worst[n], where[n] = v, label
    print(f'\nthe oracle rebuilt with fused multiply-add, ordinary blocks: worst local rel {worst[0]:.3e} on {where[0]}  '
          f'worst abs rel {worst[1]:.3e} on {where[1]}\n    conditioned blocks and moved shifts: worst local rel '
          f'{worst[2]:.3e} on {where[2]}  worst abs rel {worst[3]:.3e} on {where[3]}\n    shifts moved on {moved}')
    assert len(moved) <= 2, f'the rebuilt oracle moved fractional shifts on {moved}: these fell back to the conditioned pair'
    fs, d = wavfile.read(CLB_WAV)
    x = np.ascontiguousarray(d.astype(np.float64) / 2 ** 15)
    f0, t = ko.dio(x, fs)
    f0 = ko.stonemask(x, f0, t, fs)
    sp, ap = ko.cheaptrick(x, f0, t, fs), ko.d4c(x, f0, t, fs)
    e = assert_wave_close(fma.synthesize(f0, sp, ap, fs, 5.0), ko.synthesize(f0, sp, ap, fs, 5.0), (sp.shape[1] - 1) * 2,
                          'fma / 16 kHz recording', recording=True)
    print(f'the oracle rebuilt with fused multiply-add, 16 kHz recording: local rel {e[0]:.3e}  abs rel {e[1]:.3e}')
