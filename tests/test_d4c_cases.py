"""CPU checks of tests/d4c_cases.py, the yardstick of every D4C parity test on the GPU.

Coverage: at every rate, the oracle's own output on edge_case() shows each property the case claims, so an edit of
the generator cannot silently stop reaching D4C's corners.

Sensitivity: one-line bugs in a scratch copy of the oracle move D4C's output by as little as a few 1e-9; the
bounds of assert_ap_close must reject each of them on at least one of the inputs the GPU suite uses.  A later
loosening of AP_ABS / AP_DB then fails here, without a GPU.
"""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.io import wavfile

from conftest import CLB_WAV, ROOT, clb_variant
from d4c_cases import PLATEAUS, RATES, UNGATED, assert_ap_close, edge_case


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


def gated_rows(ap):
    return ~(ap == UNGATED).all(axis=1)


@pytest.mark.parametrize('fs', RATES)
def test_edge_case_reaches_the_corners(ko, fs):
    x, f0, t, claims = edge_case(fs, 1)
    assert len(x) <= 0.7 * fs and len(f0) == len(t)
    assert (f0 >= 0).all() and (f0 < fs / 5).all()
    x2, f02, t2, _ = edge_case(fs, 1)
    assert np.array_equal(x, x2) and np.array_equal(f0, f02) and np.array_equal(t, t2)
    g = gated_rows(ko.d4c(x, f0, t, fs))
    voiced = f0 > 0
    assert (g <= voiced).all()
    assert claims['below_40'] == (g & (f0 < 40)).any()
    assert claims['between_40_47'] == (g & (f0 > 40) & (f0 < 47)).any()
    plateaus = {f: int((g & (f0 == f)).sum()) for f in PLATEAUS + (min(1000.0, 0.19 * fs),)}
    assert min(plateaus.values()) >= 1, plateaus           # every plateau has a gated frame
    # a run of >= 3 voiced frames that LoveTrain refuses, with gated frames on both sides
    runs, n = [], 0
    for k in range(len(f0)):
        if voiced[k] and not g[k]:
            n += 1
            continue
        if n and g[k] and k - n - 1 >= 0 and g[k - n - 1]:
            runs.append(n)
        n = 0
    assert claims['voiced_ungated'] == any(r >= 3 for r in runs), runs
    if not claims['voiced_ungated']:
        assert (g == voiced).all()          # 8 kHz: every voiced frame passes the gate
    last = int(t[-3] * fs + 0.001 + 0.5)
    assert last == len(x) - 1
    assert claims['gated_first'] and t[0] == 0 and g[0]
    assert claims['gated_last'] and g[-3]
    assert claims['beyond_end'] and (t[-2:] * fs > len(x) - 1).all() and g[-2:].all()

    xs, f0s, ts, cs = edge_case(fs, 1, short=True)
    assert cs['sub_window'] and abs(len(xs) / fs - 0.025) < 1e-3
    half = int(4.0 * fs / 47.0 / 2.0 + 0.5)              # the centroid window: 4 periods at D4C's 47 Hz floor
    origin = (ts * fs + 0.001 + 0.5).astype(int)
    assert (origin - half < 0).all() and (origin + half > len(xs) - 1).all()
    assert gated_rows(ko.d4c(xs, f0s, ts, fs)).all()


# one-line edits of oracle/ko_world.c: (name, text, replacement)
MUTANTS = [
    ('extra noise draw per voiced-but-ungated frame',
     '    if (f0[i] == 0 || aperiodicity0[i] <= threshold) continue;',
     '    if (f0[i] == 0 || aperiodicity0[i] <= threshold) { if (f0[i] != 0) rng_randn(&rng); continue; }'),
    ('f0 revision biased by 0.02 Hz',
     'coarse_aperiodicity[i] + (current_f0 - 100) / 50.0',
     'coarse_aperiodicity[i] + (current_f0 + 0.02 - 100) / 50.0'),
    ('group-delay smoothing width off by 1e-4 relative',
     'LinearSmoothing(static_group_delay, current_f0 / 2.0, fs,',
     'LinearSmoothing(static_group_delay, current_f0 / 2.0 * (1.0 + 1e-4), fs,'),
    ('D4C f0 floor 47 Hz -> 40 Hz',
     'd4c_general_body(x, x_length, fs, dmax(kFloorF0D4C, f0[i]),',
     'd4c_general_body(x, x_length, fs, dmax(40.0, f0[i]),'),
    ('window samples outside the signal read as 0',
     '    waveform[i] = x[safe] * window[i] + rng_randn(rng) * kMySafeGuardMinimum;',
     '    waveform[i] = (safe == origin + i - half_window_length ? x[safe] : 0.0) * window[i] + '
     'rng_randn(rng) * kMySafeGuardMinimum;'),
    ('band selection sums m + 1 smallest',
     'power_spectrum[half - boundary - 1] / power_spectrum[half]',
     'power_spectrum[half - boundary] / power_spectrum[half]'),
    ('band centre one bin low',
     'int center = (int)(kFrequencyInterval * (i + 1) * fft_size / fs);',
     'int center = (int)(kFrequencyInterval * (i + 1) * fft_size / fs) - 1;'),
    ('centroid window moved one sample',
     'current_position - 0.25 / current_f0, rng, waveform, spec, centroid1);',
     'current_position - 0.25 / current_f0 + 1.0 / fs, rng, waveform, spec, centroid1);'),
]


def load_mutant(tmp_path, name, text, replacement, file='ko_world.c'):
    """A copy of oracle/ with one edit of ko_world.c (or of another `file` of it), built by its own Makefile and
    loaded as a module of its own."""
    src = os.path.join(ROOT, 'oracle')
    dst = tmp_path / 'oracle'
    shutil.copytree(src, dst, ignore=shutil.ignore_patterns('*.so', '__pycache__', '_ref'))
    c = (dst / file).read_text()
    assert c.count(text) == 1, name
    (dst / file).write_text(c.replace(text, replacement))
    subprocess.run(['make', '-C', str(dst), '-s'], check=True, capture_output=True)
    spec = importlib.util.spec_from_file_location(f'mutant_oracle_{abs(hash(name))}', dst / 'oracle.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def recording(ko, path):
    fs, d = wavfile.read(path)
    x = np.ascontiguousarray(d.astype(np.float64) / 2 ** 15)
    f0, t = ko.dio(x, fs)
    return x, ko.stonemask(x, f0, t, fs), t, fs


@pytest.fixture(scope='module')
def inputs(ko):
    """The GPU suite's D4C inputs, cheapest first: edge cases at every rate (16 and 48 kHz leading), then the
    16 and 48 kHz recordings (their DIO + StoneMask tracks only made when a mutant gets that far)."""
    out = []
    for fs in (16000, 48000) + tuple(r for r in RATES if r not in (16000, 48000)):
        for short in (False, True):
            out.append((f'edge {fs} {"short" if short else "main"}', False,
                        lambda fs=fs, s=short: edge_case(fs, 1, s)[:3] + (fs,)))
    cache = {}
    for path, tag, up in ((CLB_WAV, 'clb 16k', False), (clb_variant('48'), 'clb 48k', True)):
        def rec(path=path):
            if path not in cache:
                cache[path] = recording(ko, path)
            return cache[path]
        out.append((tag, up, rec))
    return out


@pytest.mark.parametrize('name,text,replacement', MUTANTS, ids=[m[0] for m in MUTANTS])
def test_bounds_reject_one_line_bugs(ko, inputs, tmp_path, name, text, replacement):
    mutant = load_mutant(tmp_path, name, text, replacement)
    for label, upsampled, make in inputs:
        x, f0, t, fs = make()
        try:
            assert_ap_close(mutant.d4c(x, f0, t, fs), ko.d4c(x, f0, t, fs), f'{name} / {label}', upsampled)
        except AssertionError as e:
            print(f'\nrejected: {name} on {label}: {str(e).splitlines()[0]}')
            return
    pytest.fail(f'no input tells "{name}" from the oracle within AP_ABS / AP_DB')
