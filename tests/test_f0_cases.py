"""CPU checks of tests/f0_cases.py, the yardstick of every DIO / StoneMask parity test on the GPU.

Coverage: at every rate the oracle's own output on edge_case() shows each property the case claims, so an edit of
the generator cannot silently stop reaching DIO's corners; the same for the StoneMask sweep and the capacity inputs.

The mask: for every (case, option set) the GPU suite uses, at most MASK_CAP of the frames are unstable.  It is made
from the oracle alone, here as on the GPU.

Option sensitivity: every option set of the GPU suite changes the oracle's track on at least one of the suite's
inputs, so a kernel that ignored the option could not pass.

Sensitivity of the bounds: one-line bugs in a scratch copy of the oracle; assert_f0_close / assert_refined_close
must reject each of them on at least one of the inputs the GPU suite uses.  A later loosening of F0_ABS / F0_REL by
a factor 100 lets the two scaled-output mutants through and fails here, without a GPU.
"""
import numpy as np
import pytest
from scipy.io import wavfile

import f0_cases as fc
from conftest import CLB_WAV, SLT_WAV, clb_variant
from d4c_cases import RATES
from test_d4c_cases import load_mutant


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


def recording(fs, tag='clb'):
    path = {('clb', 16000): CLB_WAV, ('slt', 16000): SLT_WAV, ('clb', 48000): clb_variant('48')}[(tag, fs)]
    rate, d = wavfile.read(path)
    assert rate == fs
    return np.ascontiguousarray(d.astype(np.float64) / 2 ** 15)


def share(mask):
    return float((~mask).mean())


# ------------------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize('fs', RATES)
def test_edge_case_reaches_the_corners(ko, fs):
    x, claims = fc.edge_case(fs, 1)
    x2, _ = fc.edge_case(fs, 1)
    assert np.array_equal(x, x2) and len(x) <= 2.1 * fs
    assert not np.array_equal(x, fc.edge_case(fs, 2)[0][:len(x)])
    assert [f for f, _, _ in claims['plateaus']] == list(fc.FULL_PLATEAUS)
    # the stretch of exact zeros (1/21 of the length) and the burst
    z = np.flatnonzero(x == 0.0)
    assert claims['zeros'] and len(z) >= len(x) // 22 and z[-1] - z[0] == len(z) - 1
    assert claims['burst'] and np.abs(x).max() > 0.25 * (1 + 1 / 2 + 1 / 3 + 1 / 4 + 1 / 5) * 0.5

    f0, t = ko.dio(x, fs)
    assert 0.55 <= (f0 > 0).mean() <= 0.9
    assert f0.max() > 785.0 and f0.max() <= fc.F0_CEIL          # reaches the band below the ceiling, never above
    frames = dict(fc.plateau_frames(claims, t)[:len(fc.FULL_PLATEAUS) - 2])
    tail = fc.plateau_frames(claims, t)[-2:]
    assert [f for f, _ in tail] == [fc.BOUNDARIES[4], fc.BOUNDARIES[1]]     # ... and back down: 401.6 and 142 Hz
    assert len(fc.FULL_PLATEAUS) == 13 and fc.FULL_PLATEAUS[0] == 60.0 and fc.FULL_PLATEAUS[8:11] == (790.0, 803.0, 1000.0)
    for f in claims['voiced']:
        at = frames[f] if f in frames else None
        assert at is not None and len(at) >= 5, f
        near = np.abs(f0[at] / f - 1.0) < 5e-3
        assert near.sum() >= 3, (f, f0[at])
    for f, at in tail:                                          # ... and back down
        assert (np.abs(f0[at] / f - 1.0) < 5e-3).sum() >= 3, (f, f0[at])
    # below the floor and above the ceiling: what the oracle does at default options is nothing at all -- no frame
    # at the fundamental, and no harmonic or subharmonic picked either
    assert min(claims['unvoiced']) < fc.F0_FLOOR and sorted(claims['unvoiced'])[-2] > fc.F0_CEIL
    assert claims['on_floor'] == fc.F0_FLOOR and set(fc.BOUNDARIES[:6]) <= set(claims['voiced'])
    assert any(fc.F0_CEIL * 0.98 < f <= fc.F0_CEIL for f in claims['voiced'])
    for f in claims['unvoiced']:
        assert f < fc.F0_FLOOR or f > fc.F0_CEIL
        assert not f0[frames[f]].any(), (f, f0[frames[f]])
    # on the floor the noise floor decides `c < f0_floor` frame by frame: whatever is voiced is the fundamental, and
    # the stretch is never voiced throughout
    at = frames[claims['on_floor']]
    on = f0[at][f0[at] > 0]
    assert (f0[at] == 0).any() and (on >= fc.F0_FLOOR).all() and (on < fc.F0_FLOOR * 1.005).all(), f0[at]
    # voiced frames on both sides of every default band boundary below the ceiling
    v = f0[f0 > 0]
    for b in claims['boundaries']:
        assert ((v >= 0.93 * b) & (v < b)).any() and ((v > b) & (v <= 1.07 * b)).any(), b
    assert share(fc.stable_frames(ko, x, fs)) <= fc.MASK_CAP

    xi, ci = fc.edge_case(fs, 1, in_range=True)
    assert len(xi) <= 2.1 * fs and [f for f, _, _ in ci['plateaus']] == list(fc.IN_RANGE_PLATEAUS)
    assert not ci['unvoiced'] and np.count_nonzero(xi == 0.0) >= int(fc.IN_RANGE_ZEROS * fs) - 1
    assert fc.IN_RANGE_ZEROS * fs < 2 * fc.band_plan(fs)['lh']
    fi, ti = ko.dio(xi, fs)
    for f, at in fc.plateau_frames(ci, ti):
        assert (np.abs(fi[at] / f - 1.0) < 5e-3).sum() >= 3, (f, fi[at])
    assert share(fc.stable_frames(ko, xi, fs)) <= fc.MASK_CAP


@pytest.mark.parametrize('fs', RATES)
def test_short_form_has_too_few_edges(ko, fs):
    seen = set()
    for seed in range(len(fc.SHORT_PERIODS)):
        x, claims = fc.edge_case(fs, seed, short=True)
        assert np.array_equal(x, fc.edge_case(fs, seed, short=True)[0])
        assert abs(len(x) - claims['periods'] * fs / fc.F0_FLOOR) <= 1
        seen.add(claims['periods'])
        counts = fc.engine_edge_counts(x, fs)
        assert counts.shape == (7, 4)
        # an engine with c edges has c - 1 interval points; DIO wants 3 of every engine of a band
        assert claims['few_edges'] == bool((counts - 1 < 3).any()), counts.tolist()
        f0, _ = ko.dio(x, fs)
        assert claims['voiced_stretch'] == bool(f0.any())
        if claims['few_edges']:
            assert counts.max() <= 6 and counts.min() >= 0
        assert share(fc.stable_frames(ko, x, fs)) <= fc.MASK_CAP
    assert seen == set(fc.SHORT_PERIODS)


def test_plan_restates_the_kernel():
    """the numbers written in kwy_dio.hip and its refusals, from the restated formulas"""
    p16, p48, p96 = fc.band_plan(16000), fc.band_plan(48000), fc.band_plan(96000)
    assert (p16['nbands'], p48['nbands'], p96['nbands']) == (7, 7, 7)
    assert 2 * p48['lh'] + 1 == 1921 and 4 * max(p48['hal']) == 956         # the taps the kernel's header names
    assert p16['V'] == 7231 and p96['V'] == 2439
    assert p96['filter_span'] == 5752 <= fc.FILTER_SPAN_MAX
    assert fc.band_plan(96000, f0_floor=40.0)['filter_span'] > fc.FILTER_SPAN_MAX
    lo = fc.smallest_floor(96000)
    assert fc.band_plan(96000, f0_floor=lo)['filter_span'] <= fc.FILTER_SPAN_MAX
    assert fc.band_plan(96000, f0_floor=lo - 0.01)['filter_span'] > fc.FILTER_SPAN_MAX
    assert fc.band_plan(16000, channels_in_octave=4.6)['nbands'] == fc.MAX_BANDS + 1
    high = fc.band_plan(8000, f0_ceil=12000.0)
    assert high['nbands'] <= fc.MAX_BANDS and min(high['hal']) < 1
    for fs in (16000, 96000):
        V = fc.band_plan(fs)['V']
        assert fc.length_cases(fs) == [1, 2, fs // 50, V - 1, V, V + 1, 2 * V - 1, 2 * V, 2 * V + 1]
    for fs in (16000, 48000):
        for o in fc.OPTION_SETS:
            p = fc.band_plan(fs, **o)
            assert p['nbands'] <= fc.MAX_BANDS and min(p['hal']) >= 1 and p['filter_span'] <= fc.FILTER_SPAN_MAX


def test_capacity_inputs_sit_on_both_sides_of_the_cap():
    over, under = fc.capacity_cases()
    cap = fc.edge_cap(len(over))
    assert len(over) == len(under) and cap == (len(over) + 1) // 8 + 64
    c_over = fc.engine_edge_counts(over, fc.CAPACITY_FS, **fc.CAPACITY_OPTIONS)
    c_under = fc.engine_edge_counts(under, fc.CAPACITY_FS, **fc.CAPACITY_OPTIONS)
    print('\ncapacity: over', c_over.max() / cap, 'under', c_under.max() / cap)
    assert c_over.max() >= 1.5 * cap
    assert c_under.max() <= 0.7 * cap
    # one block holds the whole utterance; a block takes every edge it can find ((V + 1) / 2), so the cap per
    # utterance is the one that decides
    plan = fc.band_plan(fc.CAPACITY_FS, **fc.CAPACITY_OPTIONS)
    assert len(over) + 1 <= plan['V'] and plan['nbands'] <= fc.MAX_BANDS and min(plan['hal']) >= 1


@pytest.mark.parametrize('fs', fc.STONEMASK_RATES)
def test_stonemask_case_reaches_the_corners(ko, fs):
    x, t, f0, f0_off, f0_low = fc.stonemask_case(fs)
    assert len(t) == len(f0) == len(f0_off) == len(f0_low) == 203
    ref = ko.stonemask(x, f0, t, fs)
    assert not ref[f0 == 0].any() and (f0[:200:17] == 0).sum() >= 11
    k40, k12 = int(np.flatnonzero(f0 == 40.0)[0]), int(np.flatnonzero(f0 == fs / 12.0)[0])
    assert f0[k40 + 1] == np.nextafter(40.0, 50.0) and f0[k12 + 1] == np.nextafter(fs / 12.0, fs)
    assert ref[k40] == 0 and ref[k40 + 1] > 40 and ref[k12] > 0 and ref[k12 + 1] == 0
    assert t[0] == 0 and ref[0] > 0 and ref[0] != f0[0]
    last = (len(x) - 1) / fs
    assert t[-3] == last and (t[-2:] > last).all() and (ref[-3:] > 0).all() and (ref[-3:-1] != f0[-3:-1]).all()
    assert ref[-1] == f0[-1]            # a window wholly beyond the end sees one repeated sample: the input is kept
    half = (1.5 * fs / f0[f0 > 40.0] + 1.0).astype(int)
    sizes = set((2 + np.floor(np.log2(2.0 * half + 1.0))).astype(int).tolist())
    assert len(sizes) >= 5 and min(sizes) == 7, sizes                    # every FFT-size step down to 128
    # the second track: corrections above 20 % fall back to the input, 19.5 % is accepted (the early stop is the
    # third track's: test_stonemask_early_stop_is_reached)
    off = ko.stonemask(x, f0_off, t, fs)
    live = (f0_off > 40.0) & (f0_off <= fs / 12.0) & (np.arange(203) > 20) & (np.arange(203) < 195)
    factor = np.resize(fc.OFF_FACTORS, 203)
    for fac in (1.25, 0.75, 2.2, 1.35):     # (StoneMask does not find the sweep from that far: some frames it moves)
        m = live & (factor == fac)
        assert m.sum() >= 10 and (off[m] == f0_off[m]).sum() >= 4, fac
    m = live & (factor == 0.75)
    assert (off[m] == f0_off[m]).mean() >= 0.7
    m = live & (factor == 1.25)             # a correction of 20 % of the input: frames on both sides of the rule
    assert (off[m] == f0_off[m]).any() and (off[m] != f0_off[m]).any()
    m = live & (factor == fc.OFF_FACTORS[4])
    moved = np.abs(off[m] / f0_off[m] - 1.0)
    assert m.sum() >= 10 and ((moved > 0.19) & (moved <= 0.2)).sum() >= 5, moved
    xs, ts, fs0 = fc.stonemask_short_case(fs)
    assert len(xs) < 2 * int(1.5 * fs / fs0.max() + 1.0) + 1 and (ko.stonemask(xs, fs0, ts, fs) > 0).all()


EARLY_STOP = '  if (tentative_f0 <= 0.0 || tentative_f0 > initial_f0 * 2)'


def test_stonemask_early_stop_is_reached(ko, tmp_path):
    """The `est > 2 initial` stop of StoneMask, counted with an oracle whose branch returns -1: at every rate at
    least 8 frames of the f0_low track of stonemask_case take it (none of the sweep's own track or of f0_off does),
    and on each of them the oracle returns the input.

    The stop cannot be told from the 20 % rule by the output: it leaves 0, which that rule replaces by the input;
    without it the second estimate starts from more than twice the input, at harmonics of a value that the signal
    does not have below its own fundamental, and ends more than 20 % from the input, which the same rule replaces.
    An oracle without the stop is therefore equal to the oracle on these frames, which is asserted too: what the
    kernel is held to on them is the input, bit for bit (assert_refined_close with f0_in)."""
    counted = load_mutant(tmp_path / 'counted', 'early stop returns -1', EARLY_STOP,
                          '  if (tentative_f0 > initial_f0 * 2) return -1.0;\n  if (tentative_f0 <= 0.0)')
    no_stop = load_mutant(tmp_path / 'no_stop', 'no early stop', EARLY_STOP, '  if (tentative_f0 <= 0.0)')
    for fs in fc.STONEMASK_RATES:
        x, t, f0, f0_off, f0_low = fc.stonemask_case(fs)
        for track in (f0, f0_off):
            assert not (counted.stonemask(x, track, t, fs) == -1.0).any()
        stopped = counted.stonemask(x, f0_low, t, fs) == -1.0
        ref = ko.stonemask(x, f0_low, t, fs)
        print(f'\n{fs}: {int(stopped.sum())} frames of f0_low stop early, {int((f0_low > 40.0).sum())} above 40 Hz')
        assert stopped.sum() >= 8
        assert np.array_equal(ref[stopped], f0_low[stopped])
        assert ((ref != f0_low) & (ref != 0)).sum() >= 20               # ... next to frames that are refined
        assert np.array_equal(no_stop.stonemask(x, f0_low, t, fs)[stopped], ref[stopped])


# -------------------------------------------------------------------------------------- the mask, option sensitivity
@pytest.mark.parametrize('fs', [16000, 48000])
def test_option_sets_stay_under_the_cap_and_bite(ko, fs):
    edge = {False: fc.edge_case(fs, 1)[0], True: fc.edge_case(fs, 1, in_range=True)[0]}
    rec = {}
    for o in fc.OPTION_SETS:
        tag = fc.recording_for(fs, o)
        if tag not in rec:
            rec[tag] = recording(fs, tag)
        bites = []
        for name, x in (('recording', rec[tag]), ('edge_case', edge[fc.wants_in_range(o)])):
            mask = fc.stable_frames(ko, x, fs, **o)
            print(f'\n{fs} {fc.option_id(o)} {name}: {int((~mask).sum())}/{len(mask)} unstable')
            assert share(mask) <= fc.MASK_CAP, (fc.option_id(o), name, int((~mask).sum()), len(mask))
            period = {k: v for k, v in o.items() if k == 'frame_period'}
            f0, _ = ko.dio(x, fs, **o)
            base, _ = ko.dio(x, fs, **period)
            bites.append(not np.array_equal(f0, base))
            if 'frame_period' in o:             # another frame grid: the frame count itself differs
                bites.append(len(f0) != len(ko.dio(x, fs)[0]))
        assert any(bites), fc.option_id(o)
        if o == dict(f0_ceil=1200.0):
            assert bites[1]                     # the recordings never reach 800 Hz; edge_case does


def test_length_cases_stay_under_the_cap(ko):
    for fs in (16000, 96000):
        V = fc.band_plan(fs)['V']
        for n in fc.length_cases(fs) + fc.length_cases(fs, ks=(fs // V + 1,))[3:]:
            x = fc.length_signal(fs, n)
            assert len(x) == n
            mask = fc.stable_frames(ko, x, fs)
            assert share(mask) <= fc.MASK_CAP, (fs, n)
        assert ko.dio(fc.length_signal(fs, (fs // V + 1) * V), fs)[0].any()


# ------------------------------------------------------------------------------------------------------- mutants
# one-line edits of oracle/ko_world.c: (name, text, replacement)
DIO_MUTANTS = [
    ('candidate range test without boundary / 2',
     'if (c > boundary_f0 || c < boundary_f0 / 2.0 || c > f0_ceil || c < f0_floor) {',
     'if (c > boundary_f0 || c > f0_ceil || c < f0_floor) {'),
    ('f0_ceil ignored',
     'if (c > boundary_f0 || c < boundary_f0 / 2.0 || c > f0_ceil || c < f0_floor) {',
     'if (c > boundary_f0 || c < boundary_f0 / 2.0 || c < f0_floor) {'),
    ('prediction 2 c - p instead of (3 c - p) / 2',
     'double reference_f0 = (current_f0 * 3.0 - past_f0) / 2.0;',
     'double reference_f0 = current_f0 * 2.0 - past_f0;'),
    ('allowed_range replaced by its default',
     '               f0_length, f0_floor, allowed_range, f0);',
     '               f0_length, f0_floor, 0.1, f0);'),
    ('contour repair step 2 one frame narrower',
     'int center = (voice_range_minimum - 1) / 2;',
     'int center = (voice_range_minimum - 1) / 2 - 1;'),
    ('contour repair step 3 stops one frame early',
     'int limit = i == negative_count - 1 ? f0_length - 1 : negative_index[i + 1];',
     'int limit = i == negative_count - 1 ? f0_length - 2 : negative_index[i + 1];'),
    ('contour repair step 4 stops one frame early',
     '    int limit = i == 0 ? 1 : positive_index[i - 1];',
     '    int limit = i == 0 ? 2 : positive_index[i - 1];'),
    ('contour repair step 1 compares with the frame before the last',
     '    f0_tmp1[i] = fabs((f0_base[i] - f0_base[i - 1]) / (kMySafeGuardMinimum + f0_base[i])) <',
     '    f0_tmp1[i] = fabs((f0_base[i] - f0_base[i - 2]) / (kMySafeGuardMinimum + f0_base[i])) <'),
    ('interpolation clamped instead of extrapolated at the ends',
     '    double s = (xi[i] - x[k[i] - 1]) / h[k[i] - 1];',
     '    double s = (xi[i] - x[k[i] - 1]) / h[k[i] - 1]; s = s < 0.0 ? 0.0 : s > 1.0 ? 1.0 : s;'),
    ('mean over n instead of n + 1',
     '    mean_y /= y_length;',
     '    mean_y /= x_length;'),
    ('intervals scaled by 1 + 2e-11',
     '    intervals[i] = fs / (fine_edges[i + 1] - fine_edges[i]);',
     '    intervals[i] = fs * (1.0 + 2e-11) / (fine_edges[i + 1] - fine_edges[i]);'),
]
# Not among them, because no input can tell them from the oracle:
#  * `<= 0` as `< 0` in the zero-crossing test needs a filtered sample that is exactly 0 after a positive one; the
#    filters are FFT products (here) and overlap-save blocks (the kernel), whose outputs are never exact zeros except
#    for digital silence, where both forms find no edge.
#  * the score's variance over 4 instead of 3 scales every band's score alike, so the best band stays the same.
#  * `num - 2 <= 0` as `num - 1 <= 0` (two interval points enough): a band whose engines found only three edges
#    covers less than three periods of a frequency in its range, and a signal long enough to leave a voiced frame
#    after the contour repair (three voiced-range minima, 105 ms at the default floor) gives such a band at least
#    seven.  The short forms of edge_case run through that guard; what they show of it is that nothing faults and
#    every frame stays 0.

SM_MUTANTS = [
    ('fall-back at 19 % instead of 20 %',
     'if (fabs(mean_f0 - initial_f0) > initial_f0 * 0.2) mean_f0 = initial_f0;',
     'if (fabs(mean_f0 - initial_f0) > initial_f0 * 0.19) mean_f0 = initial_f0;'),
    ('five harmonics instead of six',
     'int number_of_harmonics = imin((int)(fs / 2.0 / initial_f0), 6);',
     'int number_of_harmonics = imin((int)(fs / 2.0 / initial_f0), 5);'),
    ('<= 40 as < 40',
     'if (initial_f0 <= kFloorF0StoneMask || initial_f0 > fs / 12.0) return 0.0;',
     'if (initial_f0 < kFloorF0StoneMask || initial_f0 > fs / 12.0) return 0.0;'),
    ('> fs / 12 as >= fs / 12',
     'if (initial_f0 <= kFloorF0StoneMask || initial_f0 > fs / 12.0) return 0.0;',
     'if (initial_f0 <= kFloorF0StoneMask || initial_f0 >= fs / 12.0) return 0.0;'),
    ('window samples outside the signal read as 0',
     '    wave[i] = x[idx] * main_window[i];',
     '    wave[i] = (idx == basic_index + i - 1 ? x[idx] : 0.0) * main_window[i];'),
    ('refined f0 scaled by 1 + 2e-10',
     '  return numerator / (denominator + kMySafeGuardMinimum);',
     '  return numerator * (1.0 + 2e-10) / (denominator + kMySafeGuardMinimum);'),
]


@pytest.fixture(scope='module')
def dio_inputs(ko):
    """The GPU suite's DIO inputs with the options they run under, cheapest first; each entry makes
    (x, fs, options, oracle track, mask) once."""
    cache = {}

    def entry(label, fs, options, make):
        def get():
            if label not in cache:
                x = make()
                cache[label] = (x, fs, options, ko.dio(x, fs, **options), fc.stable_frames(ko, x, fs, **options))
            return cache[label]
        return label, get

    out = [entry('edge 16k', 16000, {}, lambda: fc.edge_case(16000, 1)[0]),
           entry('edge 16k short 9', 16000, {}, lambda: fc.edge_case(16000, 4, short=True)[0]),
           entry('edge 16k short 20', 16000, {}, lambda: fc.edge_case(16000, 5, short=True)[0]),
           entry('length 16k V', 16000, {}, lambda: fc.length_signal(16000, fc.band_plan(16000)['V'])),
           entry('edge 8k', 8000, {}, lambda: fc.edge_case(8000, 1)[0])]
    for o in (dict(allowed_range=0.3), dict(allowed_range=0.02), dict(f0_ceil=1200.0), dict(f0_floor=40.0),
              dict(frame_period=1.0)):
        out.append(entry(f'edge 16k {fc.option_id(o)}', 16000, o,
                         lambda o=o: fc.edge_case(16000, 1, in_range=fc.wants_in_range(o))[0]))
    out.append(entry('clb 16k', 16000, {}, lambda: recording(16000)))
    return out


@pytest.mark.parametrize('name,text,replacement', DIO_MUTANTS, ids=[m[0] for m in DIO_MUTANTS])
def test_f0_bound_rejects_one_line_bugs(ko, dio_inputs, tmp_path, name, text, replacement):
    mutant = load_mutant(tmp_path, name, text, replacement)
    for label, get in dio_inputs:
        x, fs, options, ref, mask = get()
        try:
            fc.assert_f0_close(mutant.dio(x, fs, **options), ref, mask, f'{name} / {label}',
                               options.get('f0_floor', fc.F0_FLOOR), options.get('f0_ceil', fc.F0_CEIL))
        except AssertionError as e:
            print(f'\nrejected: {name} on {label}: {str(e).splitlines()[0]}')
            return
    pytest.fail(f'no input tells "{name}" from the oracle within F0_ABS')


@pytest.mark.parametrize('name,text,replacement', SM_MUTANTS, ids=[m[0] for m in SM_MUTANTS])
def test_refined_bound_rejects_one_line_bugs(ko, tmp_path, name, text, replacement):
    mutant = load_mutant(tmp_path, name, text, replacement)
    for fs in (16000, 8000, 48000, 96000):
        x, t, f0, f0_off, f0_low = fc.stonemask_case(fs)
        xs, ts, f0s = fc.stonemask_short_case(fs)
        for label, (xx, tt, ff) in (('sweep', (x, t, f0)), ('off', (x, t, f0_off)), ('low', (x, t, f0_low)),
                                    ('short', (xs, ts, f0s))):
            try:
                fc.assert_refined_close(mutant.stonemask(xx, ff, tt, fs), ko.stonemask(xx, ff, tt, fs),
                                        f'{name} / {label} {fs}', f0_in=ff)
            except AssertionError as e:
                print(f'\nrejected: {name} on {label} {fs}: {str(e).splitlines()[0]}')
                return
    pytest.fail(f'no input tells "{name}" from the oracle within F0_REL')
