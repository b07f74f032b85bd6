"""The numpy model of the pYIN estimator (tests/pyin_cases.py) held to what the specification promises; no GPU."""
import numpy as np
import pytest

import pyin_cases as pc

LD = pc.LD


@pytest.fixture(scope='module', params=[16000, 48000])
def glide_model(request):
    fs = request.param
    x, _ = pc.glide(fs)
    p = pc.Params(fs)
    track, L, frames = pc.model(x, p)
    return fs, p, track, frames


def test_glide_has_121_frames(glide_model):
    fs, p, track, frames = glide_model
    assert len(track) == 121


def test_glide_voiced_inside_the_tone(glide_model):
    fs, p, track, frames = glide_model
    t = np.arange(len(track)) * p.frame_period / 1000.0
    inside = (t >= 0.12) & (t <= 0.48)
    assert (track[inside] > 0).all()


def test_glide_unvoiced_outside_the_tone(glide_model):
    fs, p, track, frames = glide_model
    t = np.arange(len(track)) * p.frame_period / 1000.0
    outside = (t < 0.08) | (t >= 0.52)
    assert (track[outside] == 0).all()


def test_glide_pitch_within_25_cents(glide_model):
    fs, p, track, frames = glide_model
    t = np.arange(len(track)) * p.frame_period / 1000.0
    v = (track > 0) & (t >= 0.1) & (t <= 0.5)           # (a frame half a window outside the tone may be voiced too)
    err = pc.cents(track[v], pc.glide_f0_at(t[v]))
    print(f'fs={fs}: voiced frames {v.sum()}, worst error {err.max():.2f} cents')
    assert err.max() < 25.0


@pytest.mark.parametrize('name', ['zeros', 'constant'])
def test_flat_signals_are_unvoiced(name):
    x, p = pc.edge_cases()[name]
    track, L, frames = pc.model(x, p)
    assert (track == 0).all()
    assert all(not f.taus for f in frames)


def test_prior_is_a_distribution_function():
    v = np.linspace(0.0, 1.0, 2001)
    F = np.array([pc.prior_cdf(np.float64(a)) for a in v])
    assert F[0] == 0.0 and F[-1] == 1.0
    assert (np.diff(F) >= 0).all()
    assert pc.prior_cdf(np.float64(-0.5)) == 0.0 and pc.prior_cdf(np.float64(1.5)) == 1.0


def test_frame_masses_are_probabilities(glide_model):
    fs, p, track, frames = glide_model
    for f in frames:
        total = float(f.p.sum())
        assert 0.0 <= total <= 1.0 + 1e-12
        assert (f.p >= 0).all()


def test_defaults_derive_the_documented_sizes():
    p = pc.Params(16000)
    assert (p.tau_min, p.tau_max, p.W, p.nb, p.R, p.N) == (20, 226, 227, 420, 22, 1024)
    assert pc.Params(48000).N == 2048 and pc.Params(44100).N == 2048 and pc.Params(96000).N == 4096
    assert pc.Params(16000, frame_period=1.0).R == 5 and pc.Params(16000, frame_period=10.0).R == 44
    assert pc.Params(16000, 50.0, 400.0).nb == 360


def test_float64_and_longdouble_models_agree_on_speech():
    x, fs = pc.speech()
    p = pc.Params(fs)
    a = pc.observe(x, p)
    b = pc.observe(x, p, dtype=LD)
    assert len(a) == 121
    assert all(pc.same_decisions(fa, fb) for fa, fb in zip(a, b))
    # ... and the whole candidate lists: the same lags, the same lags lowering the running minimum, the same bins
    assert all(fa.taus == fb.taus and fa.setters == fb.setters and fa.bins == fb.bins for fa, fb in zip(a, b))
    dev = np.abs(pc.probabilities(a, p) - pc.probabilities(b, p)).max()
    print(f'float64 against long double on S: {dev:.3e}')
    assert dev < 64 * 2.0 ** -52 * p.tau_max


def test_fft_form_of_the_difference_function():
    x, fs = pc.speech()
    p = pc.Params(fs)
    worst = 0.0
    for i in range(0, 121, 8):
        fr = pc.frame_of(x, i, p)
        d, s = pc.difference_direct(fr, p.W, LD)
        df, _ = pc.difference_fft(fr, p.W, p.N)
        if s[0] > 0:
            worst = max(worst, float(np.abs(df - d).max() / s[0]))
    print(f'FFT form against direct sums, relative to the frame energy: {worst:.3e}')
    assert worst < 1e-13


def test_decode_prefers_same_voicing_then_lowest_bin():
    nb, R = 6, 1
    trans = pc.transition_table(R)
    freq = pc.bin_frequencies(nb)
    L = np.zeros((3, nb + 1))                 # every state equal: the lowest state wins at the end and stays
    track, states, _ = pc.decode(L, trans, freq)
    assert states.tolist() == [0, 0, 0] and (track == freq[0]).all()
    # bins 1 and 3 lead by exactly the step's handicap log 2 over staying: bin 2 has three equal predecessors of its
    # own voicing (1, 2 and 3 reach it with log 2 + log(1/4) = log(2/4)) and takes the lowest
    L = np.full((2, nb + 1), -50.0)
    L[0, [1, 3]] = trans[1] - trans[0]
    L[0, 2] = 0.0
    L[1, 2] = 0.0
    assert L[0, 1] + trans[0] == L[0, 2] + trans[1]
    track, states, _ = pc.decode(L, trans, freq)
    assert states.tolist() == [1, 2]
    # ... and an unvoiced predecessor that ties with a voiced one loses to it.  A hand-made table of integers makes
    # every sum exact: staying costs 0, a step 2, a change of voicing 3 more
    table = -np.array([2.0, 0.0, 2.0, 5.0, 3.0, 5.0])
    L = np.full((2, nb + 1), -50.0)
    L[0, 2] = -3.0               # voiced bin 2 reaches voiced bin 2 with -3 + 0
    L[0, nb] = 0.0               # every unvoiced bin starts at 0: unvoiced bin 2 reaches voiced bin 2 with 0 - 3
    L[1, 2] = 0.0
    track, states, _ = pc.decode(L, table, freq)
    assert states.tolist() == [2, 2]
    L[0, 2] = -3.5               # ... and wins as soon as it leads
    assert pc.decode(L, table, freq)[1].tolist() == [nb + 2, 2]
