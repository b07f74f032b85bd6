"""The inputs of the band codec's edge tests (tests/codec_cases.py) held to their conditions with the CPU oracle alone,
without a GPU: the band counts of the oracle, of the library's host function and of the vocoder class agree on every
rate; the aperiodicity rows code to finite dB values and decode as voiced or unvoiced as their names say; the threshold
rows fall on the side of -0.5 dB that their flags state -- so what test_codec_edges_gpu.py expects is established here."""
import numpy as np
import pytest

import codec_cases as cc


def test_band_counts_agree():
    from oracle import oracle as ko
    from kwiiyatta_amd._lib import lib
    from kwiiyatta_amd.vocoder.world import WorldSynthesizer
    assert tuple(ko.lib().ko_d4c_num_bands(fs) for fs in cc.RATES) == cc.BANDS
    assert tuple(lib.kwy_aperiodicity_bands(fs) for fs in cc.RATES) == cc.BANDS
    assert tuple(WorldSynthesizer._get_aperiodicity_num(fs) for fs in cc.RATES) == cc.BANDS
    assert {cc.bands(fs) for fs, _ in cc.PAIRS} == {1, 2, 3, 4, 5}
    for fs in cc.RATES:                                      # the interpolation nodes 0, 3k, .., 3k nb, fs/2 increase
        assert cc.bands(fs) * cc.INTERVAL < fs / 2


@pytest.mark.parametrize('fs,fft_size', cc.PAIRS)
def test_rows_code_and_decode_as_their_names_say(fs, fft_size):
    from oracle import oracle as ko
    nb, K = cc.bands(fs), fft_size // 2 + 1
    assert 0 <= cc.step_bin(fs, fft_size) < K - 1
    for name, ap in cc.inputs(fs, fft_size).items():
        assert ap.shape[1] == K and ap.min() >= cc.SAFE and ap.max() <= 1.0, name
        coded = ko.code_aperiodicity(ap, fs)
        assert coded.shape == (len(ap), nb) and np.isfinite(coded).all(), name
        assert coded.min() >= -240.0 - 1e-9 and coded.max() <= 0.0, name
        unvoiced = coded.mean(axis=1) > -0.5
        for cols in (nb, 1):
            back = ko.decode_aperiodicity(np.ascontiguousarray(coded[:, :cols]), fs, fft_size)
            assert back.shape == ap.shape and np.isfinite(back).all() and back.min() > 0 and back.max() <= 1.0, name
            if cols == nb:
                assert np.array_equal((back == cc.UNVOICED).all(axis=1), unvoiced), name
        if name == 'fixed rows':
            assert unvoiced.tolist() == [True, False, False]
            assert np.abs(coded[1] + 240.0).max() <= 1e-9
            frac = cc.INTERVAL * nb / (fs / fft_size) - cc.step_bin(fs, fft_size)
            assert abs(coded[2, nb - 1] - (-120.0 + 114.0 * frac)) <= 0.1     # the step is what the last band sees
        else:
            assert not unvoiced.any() and len(ap) in cc.FRAMES


def test_threshold_rows_fall_where_their_flags_say():
    from oracle import oracle as ko
    for fs, coded, flags in cc.threshold_cases():
        assert coded.shape[1] == cc.bands(fs)
        ap = ko.decode_aperiodicity(coded, fs, 1024)
        assert (ap == cc.UNVOICED).all(axis=1).tolist() == flags
        assert ((ap == cc.UNVOICED).any(axis=1) == (ap == cc.UNVOICED).all(axis=1)).all()
