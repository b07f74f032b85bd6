"""CPU checks of tests/ct_cases.py, the yardstick of every CheapTrick parity test on the GPU.

Coverage: at every rate, the oracle's own output on edge_case() shows each property the case claims, so an edit of
the generator cannot silently stop reaching CheapTrick's corners.

Sensitivity: one-line bugs in a scratch copy of the oracle move CheapTrick's output by as little as 1e-8 in log;
assert_sp_close / assert_mc_close must reject each of them on at least one of the inputs the GPU suite uses.  A later
loosening of SP_* / MC_* then fails here, without a GPU.  The check that test_world_gpu.py used before
(former_check_spectrum) runs on the same mutants: the output records which of them it lets pass.
"""
import numpy as np
import pytest

from conftest import CLB_WAV  # noqa: F401  (conftest puts the repository root on sys.path)
import d4c_cases
from ct_cases import (DEFAULT_F0, FFT_SIZES, RATES, SP_FRAME_REL, SP_LOG, assert_mc_close, assert_sp_close, batch_cases,
                      default_fft_size, edge_case, fft_sizes, floor_of, gpu_inputs, half_window, sp_errors)
from test_d4c_cases import load_mutant


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


def former_check_spectrum(got, ref):
    """The former check of tests/test_world_gpu.py (check_spectrum), kept to show what it did not see."""
    assert got.shape == ref.shape
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() / np.abs(ref).max() <= 1e-8
    assert np.abs(got - ref).sum() / np.abs(ref).sum() <= 1e-9
    live = ref >= ref.max(axis=1, keepdims=True) * 1e-10
    lsd = np.abs(np.log(got[live]) - np.log(ref[live]))
    assert lsd.max() <= 1e-3, lsd.max()


def former_passes(got, ref):
    try:
        with np.errstate(all='ignore'):
            former_check_spectrum(got, ref)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize('fs', RATES)
def test_edge_case_reaches_the_corners(ko, fs):
    assert default_fft_size(fs) == ko.get_cheaptrick_fft_size(fs)
    assert fft_sizes(fs) == (FFT_SIZES[1:] if fs == 96000 else FFT_SIZES)
    for N in (None,) + fft_sizes(fs):
        fft = N or default_fft_size(fs)
        fl = floor_of(fs, fft)
        assert fl == ko.get_cheaptrick_f0_floor(fs, fft)
        kw = {} if N is None else {'fft_size': N}
        x, f0, t, c = edge_case(fs, 1, N)
        x2, f02, t2, _ = edge_case(fs, 1, N)
        assert np.array_equal(x, x2) and np.array_equal(f0, f02) and np.array_equal(t, t2)
        T = len(f0)
        assert len(x) <= 0.7 * fs and len(t) == T
        assert (f0 < 0.375 * fs).all()
        # every plateau the case promises, each of at least 3 frames
        want = [fl * (1 - 1e-12), fl, np.nextafter(fl, np.inf), 1.001 * fl, 120.0, 499.0, 500.0, 800.0, 0.2 * fs,
                0.3 * fs, 0.3749 * fs]
        for f in want:
            assert (f0 == f).sum() >= 3, f
        assert (f0 == 0).any() and (f0 == -1).any()
        assert c['raised_floor'] == (fft < default_fft_size(fs))
        if c['raised_floor']:
            assert ((f0 > floor_of(fs, default_fft_size(fs))) & (f0 < fl) & (f0 != 120) & (f0 != 499) & (f0 != 500)
                    & (f0 != 800)).sum() >= 3
        # window lengths change from frame to frame
        cf0 = np.where(f0 <= fl, DEFAULT_F0, f0)
        hw = np.array([half_window(fs, f) for f in cf0])
        assert len(set(hw.tolist())) >= 6 and (np.diff(hw) != 0).sum() >= 12
        assert 2 * hw.max() + 1 <= fft
        ref = ko.cheaptrick(x, f0, t, fs, **kw)
        assert np.isfinite(ref).all() and (ref > 0).all()
        # a frame at the floor is the 500 Hz frame, bit for bit; one rounding above it is not
        k = c['at_floor']
        assert f0[k] == fl
        g = f0.copy()
        g[k] = DEFAULT_F0
        assert np.array_equal(ko.cheaptrick(x, g, t, fs, **kw), ref)
        k = c['above_floor']
        assert f0[k] == np.nextafter(fl, np.inf)
        g = f0.copy()
        g[k] = DEFAULT_F0
        assert not np.array_equal(ko.cheaptrick(x, g, t, fs, **kw)[k], ref[k])
        assert 2 * hw[k] + 1 in (fft - 3, fft - 2)
        assert hw[c['tiny_window']] <= 4 and f0[c['tiny_window']] == 0.3749 * fs
        # positions: frame 0 at 0, frame T - 3 on the last sample, two frames beyond it that see only zeros
        assert t[0] == 0 and int(t[T - 3] * fs + 0.001 + 0.5) == len(x) - 1
        assert c['beyond_end'] == (T - 2, T - 1)
        for b in c['beyond_end']:
            assert int(t[b] * fs + 0.001 + 0.5) - hw[b] > len(x) - 1
        ref2 = ko.cheaptrick(np.ascontiguousarray(2.0 * x), f0, t, fs, **kw)
        assert np.array_equal(ref2[T - 2:], ref[T - 2:]) and not np.array_equal(ref2[0], ref[0])
        # the closing stretch: >= 6 frames, f0 alternating, 1e-6, 1e-9 and exact zeros
        cl = c['closing']
        assert T - cl >= 6 and (np.diff(f0[cl:]) != 0).all()
        frame_of = np.minimum(np.rint(np.arange(len(x)) / (fs * d4c_cases.FRAME_PERIOD)).astype(int), T - 1)
        loud = np.abs(x[frame_of < cl]).max()
        assert 1e-8 * loud < np.abs(x[(frame_of >= cl) & (frame_of < cl + 3)]).max() < 1e-5 * loud
        assert 1e-11 * loud < np.abs(x[(frame_of >= cl + 3) & (frame_of < cl + 6)]).max() < 1e-8 * loud
        assert (x[frame_of >= cl + 6] == 0).all() and (frame_of >= cl + 6).sum() > 0.015 * fs
        # the below-floor, high-f0 and tiny-window frames all lie before it
        assert max(c['at_floor'], c['tiny_window']) < cl

        # off the grid: the same signal, positions moved by fractions of a sample, a group around the half sample
        xo, f0o, to, co = edge_case(fs, 1, N, offgrid=True)
        assert np.array_equal(xo, x) and np.array_equal(f0o, f0)
        moved = to * fs - np.rint(t * fs)
        assert (np.abs(moved) < 0.5).all() and (np.abs(moved) > 1e-3).sum() >= T - 8
        hs = np.array(co['half_sample'])
        r = to[hs] * fs + 0.001
        assert len(hs) >= 8 and (np.abs(r - np.floor(r) - 0.5) <= 1e-3).all()
        # the rounding of the group is decided both ways
        o = (r + 0.5).astype(int) - np.rint(t[hs] * fs).astype(int)
        assert set(o.tolist()) == {0, 1}
        refo = ko.cheaptrick(xo, f0o, to, fs, **kw)
        assert np.isfinite(refo).all() and (refo > 0).all()

        # shorter than the shortest window: every window clamped at both ends
        xs, f0s, ts, cs = edge_case(fs, 1, N, short=True)
        assert cs['sub_window']
        hs_ = np.array([half_window(fs, f) for f in np.where(f0s <= fl, DEFAULT_F0, f0s)])
        origin = (ts * fs + 0.001 + 0.5).astype(int)
        assert len(xs) < 2 * hs_.min() + 1
        assert (origin - hs_ < 0).all() and (origin + hs_ > len(xs) - 1).all()
        refs = ko.cheaptrick(xs, f0s, ts, fs, **kw)
        assert np.isfinite(refs).all() and (refs > 0).all()
        x1, f01, t1, _ = edge_case(fs, 1, N, short='single')
        assert len(x1) == 1 and len(f01) == 1 and len(t1) == 1
        ref1 = ko.cheaptrick(x1, f01, t1, fs, **kw)
        assert np.isfinite(ref1).all() and (ref1 > 0).all()


@pytest.mark.parametrize('fs', RATES)
def test_batch_cases(fs):
    utts = batch_cases(fs)
    assert len(utts) >= 19
    T = [len(u[1]) for u in utts]
    assert all(len(u[1]) == len(u[2]) and len(u[0]) >= 1 for u in utts)
    assert 1 in T and any((u[1] == 0).all() and len(u[1]) > 1 for u in utts)
    assert any(len(u[0]) == 1 for u in utts) and any(1 < len(u[0]) <= 0.0025 * fs for u in utts)
    # three consecutive utterances of at most 5 frames each inside one launch of 16: rows [a, a + sum) lie in one
    # or two 16-row tiles, and one of them holds rows of all three (and of a neighbour, if they do not fill it)
    assert all(n <= 5 for n in T[3:6])
    first = sum(T[:3])
    tiles = [set((first + sum(T[3:3 + k]) + r) // 16 for r in range(T[3 + k])) for k in range(3)]
    assert tiles[0] & tiles[1] & tiles[2]
    assert len(set(T)) >= 12


# one-line edits of the oracle: (name, file, text, replacement)
W = 'ko_world.c'
SP_MUTANTS = [
    ('floor compared with <', W,
     '    double current_f0 = f0[i] <= floor_eff ? kDefaultF0 : f0[i];\n    cheaptrick_frame',
     '    double current_f0 = f0[i] < floor_eff ? kDefaultF0 : f0[i];\n    cheaptrick_frame'),
    ('extra draw after a below-floor frame', W,
     '    double current_f0 = f0[i] <= floor_eff ? kDefaultF0 : f0[i];\n    cheaptrick_frame',
     '    double current_f0 = f0[i] <= floor_eff ? kDefaultF0 : f0[i];\n    if (f0[i] <= floor_eff) rng_randn(&rng);\n'
     '    cheaptrick_frame'),
    ('window noise scaled 2x', W,
     '    waveform[i] = x[safe] * window[i] + rng_randn(rng) * 0.000000000000001;',
     '    waveform[i] = x[safe] * window[i] + rng_randn(rng) * 0.000000000000002;'),
    ('samples outside the signal read as 0', W,
     '    waveform[i] = x[safe] * window[i] + rng_randn(rng) * 0.000000000000001;',
     '    waveform[i] = (safe == origin + i - half_window_length ? x[safe] : 0.0) * window[i] + '
     'rng_randn(rng) * 0.000000000000001;'),
    ('DC correction upper limit 1 + ...', W,
     '  int upper_limit = 2 + (int)(f0 * fft_size / fs);', '  int upper_limit = 1 + (int)(f0 * fft_size / fs);'),
    ('smoothing width off by 1e-7 relative', W,
     'LinearSmoothing(power_spectrum, current_f0 * 2.0 / 3.0, fs,',
     'LinearSmoothing(power_spectrum, current_f0 * 2.0 / 3.0 * (1.0 + 1e-7), fs,'),
    ('q1 + 1e-7', W,
     '2.0 * q1 * cos(2.0 * kPi * quefrency * current_f0);',
     '2.0 * (q1 + 1e-7) * cos(2.0 * kPi * quefrency * current_f0);'),
    ('window centre moved by 1e-6 sample', W,
     '    double position = (i - half_window_length) / 1.5 / fs;\n'
     '    window[i] = 0.5 * cos(kPi * position * current_f0) + 0.5;\n    average',
     '    double position = (i - half_window_length + 1e-6) / 1.5 / fs;\n'
     '    window[i] = 0.5 * cos(kPi * position * current_f0) + 0.5;\n    average'),
    ('sinc lifter argument off by 1e-9 relative', W,
     'smoothing_lifter = sin(kPi * current_f0 * quefrency) / (kPi * current_f0 * quefrency);',
     'smoothing_lifter = sin(kPi * current_f0 * quefrency * (1.0 + 1e-9)) / (kPi * current_f0 * quefrency);'),
    ('origin rounded without + 0.001', W,
     '  int origin = matlab_round(current_position * fs + 0.001);\n  double average = 0.0;',
     '  int origin = matlab_round(current_position * fs);\n  double average = 0.0;'),
    ('upper mirrored end of the smoothing one bin low', W,
     '    mirroring_spectrum[i] = input[half - (i - (half + boundary))];',
     '    mirroring_spectrum[i] = input[half - 1 - (i - (half + boundary))];'),
]
# the two the former check is known to let pass, and on which inputs: on the D4C edge inputs (no f0 on the floor) /
# on every input but the one-sample ones (a constant: after the DC removal the noise is all there is)
FORMER_BLIND = {'floor compared with <': ('the D4C edge', lambda label: label.startswith('d4c-edge')),
                'window noise scaled 2x': ('all but the one-sample', lambda label: ' single ' not in label)}

S = 'ko_sptk.c'
MC_MUTANTS = [
    ('alpha off by 1e-9', S,
     'ko_freqt(c, n - 1, mc + t * (order + 1), order, alpha);',
     'ko_freqt(c, n - 1, mc + t * (order + 1), order, alpha + 1e-9);'),
    ('c0 not halved', S, '    c[0] /= 2.0;\n    ko_freqt(c, n - 1', '    ko_freqt(c, n - 1'),
]


@pytest.fixture(scope='module')
def sp_inputs(ko):
    """The GPU suite's synthetic CheapTrick inputs, cheapest first (rates in rising order, within a rate the short
    transforms first), each with the oracle's result: everything test_cheaptrick_edges runs, then the D4C edge cases
    that test_d4c_edges and the former check ran (16 and 48 kHz)."""
    out = []
    for fs in sorted(RATES):
        rows = sorted(gpu_inputs(fs), key=lambda r: r[4].get('fft_size', default_fft_size(fs)))
        out += [(label, x, f0, t, fs, opt) for label, x, f0, t, opt in rows]
    for fs in (16000, 48000):
        for short in (False, True):
            x, f0, t, _ = d4c_cases.edge_case(fs, 1, short)
            out.append((f'd4c-edge {fs} {"short" if short else "main"}', x, f0, t, fs, {}))
    return [row + (ko.cheaptrick(row[1], row[2], row[3], row[4], **row[5]),) for row in out]


# the mutants that the log criterion has to reject on its own, whatever the per-frame criterion says (the others move
# the logarithm by less than SP_LOG: 3e-7 ... 2e-6, measured here)
LOG_REJECTS = {'floor compared with <', 'extra draw after a below-floor frame', 'window noise scaled 2x',
               'samples outside the signal read as 0', 'DC correction upper limit 1 + ...',
               'origin rounded without + 0.001', 'upper mirrored end of the smoothing one bin low'}


@pytest.mark.parametrize('name,file,text,replacement', SP_MUTANTS, ids=[m[0] for m in SP_MUTANTS])
def test_sp_bounds_reject_one_line_bugs(ko, sp_inputs, tmp_path, capsys, name, file, text, replacement):
    """Each mutant of CheapTrick must fail assert_sp_close on an input of the GPU suite -- by the per-frame criterion
    alone, and those of LOG_REJECTS by the log criterion alone as well.  This is the test that fails when SP_FRAME_REL
    or SP_LOG is loosened until a listed mutant passes.  The former check runs beside it: on every input for the two
    mutants it is known to miss, up to the rejecting input for the others."""
    mutant = load_mutant(tmp_path, name, text, replacement, file)
    rejected, by_rel, by_log, former = None, None, None, []
    need_log = name in LOG_REJECTS
    for label, x, f0, t, fs, opt, ref in sp_inputs:
        done = rejected and by_rel and (by_log or not need_log)
        if done and (name not in FORMER_BLIND or not FORMER_BLIND[name][1](label)):
            continue
        got = mutant.cheaptrick(x, f0, t, fs, **opt)
        former.append((label, former_passes(got, ref)))
        if done:
            continue
        e_rel, _, e_log, _ = sp_errors(got, ref)
        if e_rel > SP_FRAME_REL and not by_rel:
            by_rel = f'{e_rel:.3e} on {label}'
        if e_log > SP_LOG and not by_log:
            by_log = f'{e_log:.3e} on {label}'
        if not rejected:
            try:
                assert_sp_close(got, ref, f'{name} / {label}')
            except AssertionError as e:
                rejected = f'rejected: {name} on {label}: {str(e).splitlines()[0]}'
    capsys.readouterr()                                     # (drop the per-input lines of the inputs that passed)
    with capsys.disabled():
        print(f'\n{rejected or "NOT rejected: " + name}\n    per-frame criterion alone: {by_rel}; log criterion alone: '
              f'{by_log}\n    the former check passes it on {sum(ok for _, ok in former)} of {len(former)} inputs tried')
    assert rejected, f'no input tells "{name}" from the oracle within SP_FRAME_REL / SP_LOG'
    assert by_rel, f'no input tells "{name}" from the oracle within SP_FRAME_REL'
    assert by_log or not need_log, f'no input tells "{name}" from the oracle within SP_LOG'
    if name in FORMER_BLIND:
        missed = [ok for label, ok in former if FORMER_BLIND[name][1](label)]
        with capsys.disabled():
            print(f'    the former check passes it on {sum(missed)} of {len(missed)}: {FORMER_BLIND[name][0]} inputs')
        assert missed and all(missed), f'the former check was recorded as blind to "{name}"'


WIDE_SUM = ('LinearSmoothing keeps its running sum in long double', W,
            '''  mirroring_segment[0] = mirroring_spectrum[0] * fs / fft_size;
  for (int i = 1; i < mlen; ++i)
    mirroring_segment[i] = mirroring_spectrum[i] * fs / fft_size + mirroring_segment[i - 1];''',
            '''  long double acc = mirroring_spectrum[0] * fs / fft_size;
  mirroring_segment[0] = (double)acc;
  for (int i = 1; i < mlen; ++i) {
    acc += (long double)(mirroring_spectrum[i] * fs / fft_size);
    mirroring_segment[i] = (double)acc;
  }''')


def test_oracles_own_running_sum_error(ko, tmp_path):
    """Where the bounds of ct_cases.py come from.  LinearSmoothing differences two running sums; the oracle keeps them
    in double.  The same oracle with the sum in long double is no less right, and differs from it
      * on the synthetic input with the worst conditioning (8 kHz, 4096 points, sub-window form: a 4093-sample window
        over 20 samples) by more than the 1e-7 in log one might hope for, and by less than SP_LOG;
      * on the 16 kHz recording by more than SP_FRAME_REL and SP_LOG, which is why recordings have pairs of their own,
        and by less than SP_FRAME_REL_RECORDED / SP_LOG_RECORDED.
    So no kernel can be held closer to this oracle than these figures, whatever its summation order."""
    from scipy.io import wavfile
    import ct_cases as cc
    wide = load_mutant(tmp_path, *WIDE_SUM[:1], *WIDE_SUM[2:], WIDE_SUM[1])
    x, f0, t, _ = edge_case(8000, 1, 4096, short=True)
    e_rel, _, e_log, at = sp_errors(wide.cheaptrick(x, f0, t, 8000, fft_size=4096), ko.cheaptrick(x, f0, t, 8000, fft_size=4096))
    print(f'\nlong-double running sum, edge 8000 short fft 4096: frame rel {e_rel:.3e}  log {e_log:.3e} at {at}')
    assert 1e-7 < e_log <= cc.SP_LOG and e_rel <= cc.SP_FRAME_REL
    fs, d = wavfile.read(CLB_WAV)
    x = np.ascontiguousarray(d.astype(np.float64) / 2 ** 15)
    f0, t = ko.dio(x, fs)
    f0 = ko.stonemask(x, f0, t, fs)
    e_rel, at_rel, e_log, at = sp_errors(wide.cheaptrick(x, f0, t, fs), ko.cheaptrick(x, f0, t, fs))
    print(f'long-double running sum, 16 kHz recording: frame rel {e_rel:.3e} at {at_rel}  log {e_log:.3e} at {at}')
    assert cc.SP_LOG < e_log <= cc.SP_LOG_RECORDED
    assert cc.SP_FRAME_REL < e_rel <= cc.SP_FRAME_REL_RECORDED


@pytest.mark.parametrize('name,file,text,replacement', MC_MUTANTS, ids=[m[0] for m in MC_MUTANTS])
def test_mc_bounds_reject_one_line_bugs(ko, tmp_path, capsys, name, file, text, replacement):
    """Each mutant of sp2mc must fail assert_mc_close on an utterance of the GPU suite's batches (16 kHz, 1024 points,
    order 63, alpha 0.7, out_div 1, then 8 kHz with out_div = fs): the test that fails when MC_ABS / MC_C0 are
    loosened too far.  (alpha + 1e-9 moves the coefficients by up to 4.6e-9 of their scale, 2.3 x MC_ABS.)"""
    mutant = load_mutant(tmp_path, name, text, replacement, file)
    rejected = None
    for fs, fft, order, alpha, out_div in ((16000, 1024, 63, 0.7, 1.0), (8000, 512, 24, 0.7, 8000.0)):
        for n, (x, f0, t) in enumerate(batch_cases(fs, fft)):
            sp = np.ascontiguousarray(ko.cheaptrick(x, f0, t, fs, fft_size=fft) / out_div)
            try:
                assert_mc_close(mutant.sp2mc(sp, order, alpha), ko.sp2mc(sp, order, alpha), f'{name} / utterance {n}')
            except AssertionError as e:
                rejected = (f'rejected: {name} on batch_cases({fs}, {fft})[{n}] order {order} alpha {alpha}: '
                            f'{str(e).splitlines()[0]}')
                break
        if rejected:
            break
    capsys.readouterr()
    with capsys.disabled():
        print(f'\n{rejected or "NOT rejected: " + name}')
    assert rejected, f'no utterance tells "{name}" from the oracle within MC_ABS / MC_C0'
