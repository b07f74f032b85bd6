"""k_d4c_body on half frames: where a frame's window ends at sample N/2 (f0 >= 8 fs / N: 93.75 Hz at 48 kHz) the fills
store no zeros and the first radix-8 pass of its five transforms reads points 0 .. H/2 only.  Adding exact zeros changes
no value, so the aperiodicity is, bit for bit, what the build before the change computed on an MI355X
(tests/golden/d4c_half_bits_*_parent.npz, recorded by tools/record_half_frame_bits.py; inputs:
tests/half_frame_cases.py): constant tracks just below the switch (dense), exactly on it (the window's last sample is
the packed point H/2, which only thread 0 of the half pass reads -- and which holds stale data unless the fill stores
it), just above and far above it, at every transform length (16, 32, 48 and 96 kHz); first and last frame of the signal,
where the sample indices are clamped; a one-frame utterance; a track that mixes both kinds of frame; and all of a
rate's cases in one batched call.
"""
import os

import numpy as np
import pytest

import half_frame_cases as hc
from d4c_cases import UNGATED

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = [(fs, name) for fs in hc.D4C_F0 for name in hc.d4c_names(fs)]


@pytest.fixture(scope='module')
def golden():
    g = {}
    for name in sorted(set(hc.D4C_FILE.values())):
        f = np.load(os.path.join(GOLDEN, name))
        assert int(f['seed']) == hc.SEED and len(str(f['commit'])) == 40
        g[name] = f
    return g


def test_cases_lie_on_both_sides_of_the_switch():
    for fs, f0s in hc.D4C_F0.items():
        n = hc.D4C_N[fs]
        assert 8.0 * fs / n == f0s[1] and f0s[0] < f0s[1] > 47.0
        assert hc.d4c_window(fs, f0s[0])[1] is False and hc.d4c_window(fs, f0s[0])[0] <= n
        assert hc.d4c_window(fs, f0s[1]) == (n // 2 + 1, True)
        assert all(hc.d4c_window(fs, f)[1] for f in f0s[2:])
    assert [hc.d4c_window(48000, f)[1] for f in hc.MIXED] == [False, True, True, True]
    x, t3 = hc.signal(48000)
    assert t3[0] == 0.0 and t3[-1] * 48000 > len(x)          # windows clamped at the first and beyond the last sample


@pytest.mark.parametrize('fs,name', CASES)
def test_bits_of_the_parent_build(golden, fs, name):
    g = golden[hc.D4C_FILE[fs]]
    want = g[hc.d4c_key(fs, name)]
    case = hc.d4c_cases(fs)[name]
    assert want.shape[0] == len(case[1]) and not (want == UNGATED).all(axis=1).any()
    got = hc.d4c_single(fs, case)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"frames {bad.tolist()} differ from the build at {g['commit']}"
    assert np.array_equal(got, want)


@pytest.mark.parametrize('fs', list(hc.D4C_F0))
def test_one_batched_call_of_both_kinds(golden, fs):
    """every case of the rate as one utterance of one kwy_d4c_batch_dev call: dense and half utterances, at 48 kHz the
    mixed track and the one-frame utterance, side by side in one grid"""
    from kwiiyatta_amd import _lib
    g = golden[hc.D4C_FILE[fs]]
    cases = hc.d4c_cases(fs)
    for name, got in zip(cases, hc.d4c_batch(_lib.Context(0), fs, list(cases.values()))):
        assert np.array_equal(got, g[hc.d4c_key(fs, name)]), (fs, name)
