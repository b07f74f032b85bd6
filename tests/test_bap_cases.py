"""CPU checks of the band-aperiodicity conversion's test inputs and of its restatement (tests/bap_cases.py), and of the
host-side surface that needs no device: signatures, parser options, the model file of a converter without the band
mixture, and the refusal of a sampling rate without a band before anything is read."""
import inspect
import sys

import numpy as np
import pytest

import bap_cases as bc
import codec_cases as cc


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize('T', bc.FRAMES)
def test_patterns_have_the_property_they_are_named_for(T):
    P = bc.PASS_FRAMES
    pats = bc.patterns(T)
    assert pats['all voiced'].all() and not pats['none voiced'].any()
    last = pats['one voiced frame, last']
    assert last.sum() == 1 and last[-1]
    if T >= 2:
        lead, trail, alt = pats['leading run'], pats['trailing run'], pats['alternating']
        n = int(np.argmax(lead))
        assert n >= 1 and not lead[:n].any() and lead[n:].all()
        m = int(np.argmax(~trail))
        assert 1 <= m < T and trail[:m].all() and not trail[m:].any()
        assert (alt[1:] != alt[:-1]).all()
    else:
        assert set(pats) == {'all voiced', 'none voiced', 'one voiced frame, last'}
    if T >= 2 * P + 1:
        v = pats['unvoiced run over a pass']
        assert not v[P:2 * P].any() and v[:P - 1].all() and v[2 * P:].all()       # pass 1 has no voiced frame at all
    else:
        assert 'unvoiced run over a pass' not in pats
    assert all(len(v) == T and v.dtype == bool for v in pats.values())


def test_frames_and_rates_cover_what_the_contract_names():
    P = bc.PASS_FRAMES
    assert bc.FRAMES == (1, 2, P, P + 1, 2 * P + 1)
    assert all(cc.bands(fs) >= 1 for fs, _ in bc.PAIRS)
    assert (48000, 742) in bc.PAIRS and (48000, 6) in bc.PAIRS and (16000, 1024) in bc.PAIRS
    assert cc.bands(16000) == 1 and sorted({cc.bands(fs) for fs, _ in bc.PAIRS}) == [1, 2, 3, 4, 5]


def _case_inputs():
    for fs, fft_size in bc.PAIRS:
        yield from ((fs, fft_size, ap) for ap in cc.inputs(fs, fft_size).values())
        for T in (1, 2, 5):
            yield from ((fs, fft_size, bc.ap_for(v, fs, fft_size)) for v in bc.patterns(T).values())


def test_flags_are_the_complement_of_what_the_decoder_flattens(ko):
    for fs, fft_size, ap in _case_inputs():
        coded = ko.code_aperiodicity(ap, fs)
        flat = (ko.decode_aperiodicity(coded, fs, fft_size) == cc.UNVOICED).all(axis=1)
        assert np.array_equal(bc.flags(coded) == 0.0, flat), (fs, fft_size)
    for fs, coded, unvoiced in cc.threshold_cases():
        flat = (ko.decode_aperiodicity(coded, fs, 1024) == cc.UNVOICED).all(axis=1)
        assert flat.tolist() == unvoiced
        assert (bc.flags(coded) == 0.0).tolist() == unvoiced, fs


def test_pattern_inputs_code_to_their_voicing(ko):
    for fs, fft_size in ((16000, 1024), (48000, 742), (48000, 6)):
        for name, v in bc.patterns(5).items():
            coded = ko.code_aperiodicity(bc.ap_for(v, fs, fft_size), fs)
            assert np.array_equal(bc.flags(coded) == 1.0, v), (fs, name)
            assert coded[v].max(initial=-99.0) <= -10.0 + 1e-9        # far below the threshold, as ap_for says


def test_threshold_rows_step_through_the_threshold(ko):
    rows = bc.threshold_ap()
    coded = ko.code_aperiodicity(rows, 16000)
    assert coded.shape == (len(rows), 1)
    assert (coded > -0.5).any() and (coded <= -0.5).any()
    assert np.abs(coded + 0.5).max() < 1e-12


def test_fill_holds_the_nearest_voiced_row_and_is_idempotent():
    rng = np.random.default_rng(3)
    for name, v in bc.patterns(9).items():
        coded = -rng.uniform(5.0, 50.0, (9, 3))
        coded[~v] = 20 * np.log10(cc.UNVOICED)
        S = bc.fill(coded)
        assert np.array_equal(S[:, 0] == 1.0, v), name
        assert np.array_equal(S[v, 1:], coded[v]), name
        if not v.any():
            assert np.array_equal(S[:, 1:], coded)
            continue
        first = int(np.argmax(v))
        for t in np.flatnonzero(~v):
            src = first if t < first else max(i for i in np.flatnonzero(v) if i < t)
            assert np.array_equal(S[t, 1:], coded[src]), (name, t)
        assert np.array_equal(bc.fill(S[:, 1:])[:, 1:], S[:, 1:]), name        # a filled track has nothing left to fill


def test_joint_rows_and_band_error_restated(ko):
    X, Y = bc.random_track(40, 2, 0), bc.random_track(50, 2, 1)
    ix, iy = bc.random_lists(60, 40, 50, 0)
    delta = lambda g: ko.delta_features(g, ko.DELTA_WINDOWS)  # noqa: E731
    rows = bc.joint_rows(X, Y, ix, iy, delta)
    keep = bc.kept_cells(X, Y, ix, iy)
    assert 0 < keep.sum() < len(keep) and rows.shape == (keep.sum(), 12)
    assert np.array_equal(rows[:, :2], X[ix[keep], 1:]) and np.array_equal(rows[:, 6:8], Y[iy[keep], 1:])
    m, cells = bc.band_error(X, Y, ix, iy)
    assert m[0] == keep.sum() and np.array_equal(~np.isnan(cells), keep)
    assert np.isclose(m[1], np.nanmean(cells)) and m[2] >= 0
    assert np.array_equal(bc.clamp(np.array([3.0, -80.0, -60.0, -1e-12, -7.0])), [-1e-12, -60.0, -60.0, -1e-12, -7.0])


def test_defaults_appear_in_the_signatures():
    import kwiiyatta_amd as k
    from kwiiyatta_amd import convert_voice, corpus, evaluate_voice
    from kwiiyatta_amd._convert_options import ConvertOptions
    from kwiiyatta_amd.converter import PaddedDataset
    for fn in (corpus.ConvertWave.__init__, corpus.convert_batch, corpus.evaluate_batch, corpus._lockstep_batch):
        assert inspect.signature(fn).parameters['ap_gmm'].default is None, fn
    assert 'ap_gmm' not in ConvertOptions.DEFAULTS                      # a parameter of its own beside gmm
    assert inspect.signature(corpus.build_training_matrix).parameters['bands'].default is False
    assert inspect.signature(corpus.realign_training_matrix).parameters['bands'].default is False
    assert inspect.signature(corpus._Alignment.rows_into).parameters['band_sink'].default is None
    assert inspect.signature(corpus.EvalWave.measure).parameters['ap_gmm'].default is None
    assert corpus._AlignInputs._fields[-1] == 'track' and corpus._AlignInputs._field_defaults == {'track': None}
    p = inspect.signature(k.MelCepstrumConverter().train).parameters
    assert p['ap_model'].default is False and p['ap_components'].default == 16
    assert convert_voice.COMMAND_OPTIONS['convert_ap'] is False
    assert inspect.signature(convert_voice.convert).parameters['convert_ap'].default is False
    assert inspect.signature(evaluate_voice.evaluate_pair).parameters['convert_ap'].default is False
    assert inspect.signature(PaddedDataset.__init__).parameters['bands'].default is False
    assert 'band_track' in k.__all__
    assert k.MelCepstrumConverter().ap_converter is None


def test_parser_takes_the_options(monkeypatch):
    import kwiiyatta_amd as k
    monkeypatch.setattr(sys, 'argv', ['prog'])
    conf = k.Config()
    conf.add_aperiodicity_arguments()
    conf.parse_args([])
    assert conf.convert_aperiodicity is False and conf.ap_components == 16
    conf = k.Config()
    conf.add_aperiodicity_arguments()
    conf.parse_args(['--convert-aperiodicity', '--ap-components', '4'])
    assert conf.convert_aperiodicity is True and conf.ap_components == 4
    conf = k.Config()
    conf.add_aperiodicity_arguments()
    with pytest.raises(SystemExit):
        conf.parse_args(['--ap-components', '0'])
    from kwiiyatta_amd import evaluate_voice
    conf = evaluate_voice.make_config()
    conf.parse_args(['--convert-aperiodicity'])
    assert conf.convert_aperiodicity is True


def _plain_model(path, fs=16000):
    """a converter model file as `save` writes it for a stack trained without the band mixture"""
    import kwiiyatta_amd as k
    conv = k.MelCepstrumConverter(components=1)
    rng = np.random.default_rng(0)
    conv.order, conv.fs = 2, fs
    conv.base.frame_period = 5
    conv.gmm.weights_, conv.gmm.means_ = np.ones(1), rng.standard_normal((1, 12))
    conv.gmm.covariances_ = np.eye(12)[None]
    conv.save(path)
    return conv


def test_model_without_the_mixture_has_none_of_the_keys(tmp_path):
    import kwiiyatta_amd as k
    path = tmp_path / 'plain.npz'
    _plain_model(path)
    with np.load(path) as z:
        assert not [name for name in z.files if name.startswith('ap_')]
        assert str(z['format']) == k.MelCepstrumConverter().MODEL_FORMAT == 'kwiiyatta_amd.converter/1'
    loaded = k.MelCepstrumConverter().load(path)
    assert loaded.ap_converter is None and loaded.ap_rows == 0


def test_model_with_the_mixture_round_trips_on_the_host(tmp_path):
    import kwiiyatta_amd as k
    path = tmp_path / 'banded.npz'
    conv = _plain_model(tmp_path / 'plain.npz')
    band = bc.BandGMM(1, M=2, seed=5)
    stack = conv._band_stack(2)
    stack.gmm.weights_, stack.gmm.means_, stack.gmm.covariances_ = band.weights_, band.means_, band.covariances_
    stack.frame_period = 5
    conv.ap_converter = stack
    conv.save(path)
    with np.load(path) as z:
        assert {'ap_weights', 'ap_means', 'ap_covariances', 'ap_covariance'} <= set(z.files)
    loaded = k.MelCepstrumConverter().load(path)
    got = loaded.ap_converter.gmm
    assert np.array_equal(got.weights_, band.weights_) and np.array_equal(got.means_, band.means_)
    assert np.array_equal(got.covariances_, band.covariances_) and got.n_components == 2
    assert loaded.ap_converter.frame_period == 5 and got.covariance_structure == 'full'


def test_rate_without_a_band_raises_before_a_file_is_read(tmp_path):
    import kwiiyatta_amd as k
    from kwiiyatta_amd import convert_voice
    from kwiiyatta_amd.backend import bap
    assert bap.bands(8000) == 0 and bap.bands(12000) == 1
    with pytest.raises(ValueError, match='12 kHz'):
        bap.check_rate(8000)
    with pytest.raises(ValueError, match='12 kHz'):
        k.band_track(np.full((3, 513), 0.5), 8000)
    with pytest.raises(ValueError, match='12 kHz'):
        bap.apply(np.zeros((3, 2)), np.zeros((3, 2)), np.full((3, 513), 0.5), 8000)

    class Unreadable:
        """a dataset that fails the test when anything is read from it"""
        def keys(self):
            raise AssertionError('the dataset was read')
        __getitem__ = __iter__ = keys
    with pytest.raises(ValueError, match='12 kHz'):
        k.MelCepstrumConverter(mcep_fs=8000).train(Unreadable(), ['a'], ap_model=True)
    conv = _plain_model(tmp_path / 'm8.npz', fs=8000)
    with pytest.raises(ValueError, match='12 kHz'):
        convert_voice.convert(None, conv, tmp_path / 'missing.wav', diffvc=False, convert_ap=True)
    conv16 = _plain_model(tmp_path / 'm16.npz', fs=16000)
    with pytest.raises(ValueError, match='no band-aperiodicity mixture'):
        convert_voice.convert(None, conv16, tmp_path / 'missing.wav', diffvc=False, convert_ap=True)


def test_loaded_model_without_the_mixture_is_a_parser_error(tmp_path, monkeypatch, capsys):
    import kwiiyatta_amd as k
    path = tmp_path / 'plain.npz'
    _plain_model(path)
    monkeypatch.setattr(sys, 'argv', ['prog'])
    conf = k.Config()
    conf.add_aperiodicity_arguments()
    conf.add_converter_arguments()
    conf.parse_args(['--convert-aperiodicity', '--converter-model', str(path), '--converter-components', '1'])
    with pytest.raises(SystemExit):
        conf.train_converter(use_delta=True, ap_model=True)
    assert 'no band-aperiodicity mixture' in capsys.readouterr().err
