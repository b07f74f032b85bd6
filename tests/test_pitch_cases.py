"""The claims of the pitch shifter's numpy statement (tests/pitch_cases.py) itself: no GPU.  The kernels are held
against this statement in tests/test_pitch_gpu.py."""
import numpy as np
import pytest

import pitch_cases as pc
from conftest import CLB_WAV, SLT_WAV, clb_variant


@pytest.mark.parametrize('wav', [CLB_WAV, clb_variant('48')], ids=['16k', '48k'])
def test_rate_one_is_the_identity_bit_for_bit(wav):
    fs, x = pc.load(wav)
    y, p = pc.shift_pitch(x, fs, 1.0, with_positions=True)
    assert np.array_equal(y, x)
    assert np.array_equal(p, np.arange(len(p)) * int(fs * 0.010))


@pytest.mark.parametrize('rate', pc.RATES + (1.0,))
@pytest.mark.parametrize('n', [0, 1, 50, 159, 160, 161, 1000, 4801])
def test_length_is_kept_for_any_length(n, rate):
    fs = 16000
    x = np.random.RandomState(n).uniform(-0.5, 0.5, n)
    y, p = pc.shift_pitch(x, fs, rate, with_positions=True)
    H, _, _, M, K = pc.constants(n, fs, rate)
    assert y.shape == (n,) and np.isfinite(y).all()
    assert len(p) == K == (-(-M // H) if M else 0)
    if 0 < n < H and rate <= 1.0:
        assert K == 1


def test_silence_stays_silence():
    for rate in pc.RATES:
        y, p = pc.shift_pitch(np.zeros(5000), 16000, rate, with_positions=True)
        assert not y.any()
        # every distance is an exact zero: the tie rule picks the ideal position
        assert [int(v) for v in p[1:]] == [pc.ideal_position(k, 5000, 16000, rate) for k in range(1, len(p))]


@pytest.mark.parametrize('rate', pc.RATES)
def test_positions_stay_in_their_windows(rate):
    fs, x = pc.load(CLB_WAV)
    n, S = len(x), int(fs * 0.010)
    p = pc.positions(x, fs, rate)
    assert p[0] == 0
    for k in range(1, len(p)):
        a = pc.ideal_position(k, n, fs, rate)
        assert max(a - S, 0) <= p[k] <= min(a + S, n - 1)


def _oracle_f0(x, fs):
    from oracle import oracle as ko
    f0, t = ko.dio(x, fs)
    return ko.stonemask(x, f0, t, fs)


@pytest.mark.parametrize('wav', [CLB_WAV, SLT_WAV], ids=['clb', 'slt'])
def test_f0_follows_the_rate(wav):
    fs, x = pc.load(wav)
    f0_in = _oracle_f0(x, fs)
    for rate in pc.RATES:
        median, share = pc.f0_ratio(f0_in, _oracle_f0(pc.shift_pitch(x, fs, rate), fs))
        print(f'rate {rate}: median f0 ratio / rate = {median / rate:.4f} over {100 * share:.0f} % of the frames')
        assert share > 0.2
        assert abs(median / rate - 1) <= 0.02


@pytest.mark.parametrize('wav,rates', [(CLB_WAV, pc.RATES), (SLT_WAV, pc.RATES), (clb_variant('48'), (1.0, 1.4983))],
                         ids=['clb', 'slt', 'clb48'])
def test_positions_do_not_depend_on_the_summation_order(wav, rates):
    """what makes the comparison of the kernel's positions meaningful: the best and the second-best distance lie far
    enough apart for any order of the sum (exact ties inside digital silence are settled by the tie rule)"""
    fs, x = pc.load(wav)
    for rate in rates:
        forward, backward = pc.positions(x, fs, rate), pc.positions(x, fs, rate, reverse=True)
        assert np.array_equal(forward, backward), f'rate {rate}: {(forward != backward).sum()} steps differ'


def test_bounds_are_what_they_say():
    assert pc.distance_slack(16000) == 2 * (320 + 2) * 2.0 ** -53
    fs, x = pc.load(CLB_WAV)
    x = x[:8000]
    _, _, _, M, _ = pc.constants(len(x), fs, 2.0)
    p = pc.positions(x, fs, 2.0)
    b = pc.waveform_bound(x, fs, p, len(x), M)
    y = pc.resample(pc.stretch(x, fs, p, M), len(x))
    assert b.shape == y.shape and (b >= 0).all()
    assert b.max() < 1e-10 * np.abs(y).max()            # a rounding bound: far below the signal
