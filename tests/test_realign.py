"""`--align-iterations`: iterative re-alignment of the training set -- what needs no device: the option and its conflict
with a loaded model, the model file's new fields, the shape check of `dtw_feature(x_mapped=...)` and the refusals of the
device driver.  The arithmetic is tested on the GPU (test_realign_gpu.py)."""
import argparse
import sys

import numpy as np
import pytest

from conftest import CLB_DIR, CLB_WAV, SLT_DIR


def _run_cli(main, argv):
    old = sys.argv
    sys.argv = ['prog'] + argv
    try:
        main()
    finally:
        sys.argv = old


def _parser_error(main, argv, capsys):
    with pytest.raises(SystemExit) as e:
        _run_cli(main, argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def _config(argv):
    import kwiiyatta_amd as k
    conf = k.Config(argparse.ArgumentParser())
    conf.add_converter_arguments()
    conf.parser.parse_args(argv, namespace=conf)
    return conf


def _stack(iterations=None, history=()):
    from test_f0_convert import _trained_stack
    conv = _trained_stack()
    if iterations is not None:
        conv.align_iterations = iterations
        conv.align_history = [dict(rows=r, mcd=m, em_iterations=e) for r, m, e in history]
    return conv


HISTORY = ((1200, 7.25, 11), (1180, 5.5, 9), (1175, 5.375, 12))


# ---- the option ------------------------------------------------------------------------------------------------------
def test_option_is_an_integer_within_its_range():
    assert _config([]).align_iterations is None           # not given: 0 for training, no demand on a loaded model
    for text, n in (('0', 0), ('1', 1), ('3', 3), ('10', 10)):
        conf = _config(['--align-iterations', text])
        assert conf.align_iterations == n and isinstance(conf.align_iterations, int)


@pytest.mark.parametrize('text', ['-1', '11', '1.5', 'two', '', 'nan'])
def test_anything_else_is_a_parser_error(text, capsys):
    import kwiiyatta_amd.convert_voice as cv
    import kwiiyatta_amd.evaluate_voice as ev
    assert '--align-iterations' in _parser_error(cv.main, ['--align-iterations', text, CLB_WAV], capsys)
    assert '--align-iterations' in _parser_error(ev.main, ['--align-iterations', text], capsys)


def test_both_commands_document_the_option(capsys):
    import kwiiyatta_amd.convert_voice as cv
    import kwiiyatta_amd.evaluate_voice as ev
    for main in (cv.main, ev.main):
        with pytest.raises(SystemExit) as e:
            _run_cli(main, ['--help'])
        assert e.value.code == 0
        assert '--align-iterations N' in capsys.readouterr().out


def test_the_option_reaches_train(monkeypatch):
    """Config._train passes the count on -- and passes nothing for 0 or when the option is absent, so a converter
    class that predates the argument keeps working"""
    import kwiiyatta_amd as k
    seen = []

    class Fake:
        source_f0_rate = 1.0

        def train(self, dataset, keys, **kwargs):
            seen.append(kwargs)
    for argv, want in (([], {}), (['--align-iterations', '0'], {}), (['--align-iterations', '4'], dict(align_iterations=4))):
        conf = _config(['--source', CLB_DIR, '--target', SLT_DIR, '--max-files', '1'] + argv)
        monkeypatch.setattr(k.Config, 'load_dataset', lambda self, rate=None: {'a': None})
        conf._train(Fake())
        assert seen.pop() == want


# ---- the model file --------------------------------------------------------------------------------------------------
def test_model_round_trip_keeps_count_and_record(tmp_path):
    import kwiiyatta_amd as k
    path = tmp_path / 'model.npz'
    fresh = _stack()
    assert fresh.align_iterations == 0 and fresh.align_history == []
    _stack(2, HISTORY).save(path)
    loaded = k.MelCepstrumConverter(components=2).load(path)
    assert loaded.align_iterations == 2 and isinstance(loaded.align_iterations, int)
    assert [r['mcd'] for r in loaded.align_history] == [7.25, 5.5, 5.375]
    assert [r['rows'] for r in loaded.align_history] == [1200, 1180, 1175]
    with np.load(path) as z:
        assert str(z['format']) == loaded.MODEL_FORMAT          # the format string is unchanged
        assert int(z['align_iterations']) == 2 and z['align_iterations'].dtype.kind == 'i'
        assert z['align_mcd'].shape == (3,) and z['align_mcd'].dtype == np.float64


def test_a_converter_aligned_once_writes_zero_and_an_empty_record(tmp_path):
    import kwiiyatta_amd as k
    path = tmp_path / 'model.npz'
    _stack().save(path)
    with np.load(path) as z:
        assert int(z['align_iterations']) == 0 and z['align_mcd'].shape == (0,)
    loaded = k.MelCepstrumConverter(components=2).load(path)
    assert loaded.align_iterations == 0 and loaded.align_history == []


def test_old_model_loads_as_aligned_once(tmp_path):
    import kwiiyatta_amd as k
    from test_f0_convert import _old_model
    path = tmp_path / 'old.npz'
    _old_model(path)
    loaded = k.MelCepstrumConverter(components=2).load(path)
    assert loaded.align_iterations == 0 and loaded.align_history == []


def test_a_count_that_conflicts_with_the_model_is_a_parser_error(tmp_path, capsys):
    import kwiiyatta_amd.convert_voice as cv
    import kwiiyatta_amd.evaluate_voice as ev
    path = tmp_path / 'model.npz'
    _stack(2, HISTORY).save(path)
    err = _parser_error(cv.main, ['--align-iterations', '3', '--converter-model', str(path), '--result-dir',
                                  str(tmp_path / 'out'), CLB_WAV], capsys)
    assert 'trained with --align-iterations 2' in err and 'retrain' in err and 'not 3' in err
    assert not (tmp_path / 'out').exists()
    err = _parser_error(ev.main, ['--source', CLB_DIR, '--target', SLT_DIR, '--align-iterations', '0',
                                  '--converter-model', str(path)], capsys)
    assert 'trained with --align-iterations 2' in err and 'retrain' in err
    # an old model counts as aligned once
    from test_f0_convert import _old_model
    old = tmp_path / 'old.npz'
    _old_model(old)
    err = _parser_error(cv.main, ['--align-iterations', '1', '--converter-model', str(old), '--result-dir',
                                  str(tmp_path / 'out'), CLB_WAV], capsys)
    assert 'trained with --align-iterations 0' in err


def test_a_loaded_model_decides_when_the_option_is_absent_or_agrees(tmp_path):
    path = tmp_path / 'model.npz'
    _stack(2, HISTORY).save(path)
    for extra in ([], ['--align-iterations', '2']):
        conf = _config(['--converter-model', str(path), '--converter-components', '2'] + extra)
        assert conf.train_converter(use_delta=True).align_iterations == 2


def test_report_lines_of_the_training_record():
    import kwiiyatta_amd.evaluate_voice as ev
    assert ev.training_record_lines(_stack()) == []
    lines = ev.training_record_lines(_stack(2, HISTORY))
    assert lines == ['training alignment 0: rows 1200 monitor MCD 7.250 dB',
                     'training alignment 1: rows 1180 monitor MCD 5.500 dB',
                     'training alignment 2: rows 1175 monitor MCD 5.375 dB']


# ---- the pieces --------------------------------------------------------------------------------------------------------
class _Side:
    """what make_feature asks of a feature set"""

    def __init__(self, frames, order=24, fs=16000, seed=0):
        rng = np.random.RandomState(seed)
        self.fs, self.frame_len = fs, frames
        self.data = rng.standard_normal((frames, order + 1))
        self.is_voiced = rng.rand(frames) > 0.5

    def resample_mel_cepstrum(self, fs):
        assert fs == self.fs
        return self


@pytest.mark.parametrize('shape', [(39, 24), (40, 25), (40, 23), (40,), (24, 40), (40, 24, 1)])
def test_x_mapped_of_another_shape_is_refused_before_anything_runs(shape):
    from kwiiyatta_amd.vocoder.align import align_even, dtw_feature, even_indices
    x, y = _Side(40), _Side(50, seed=1)
    for call in (lambda **kw: dtw_feature(x, y, **kw), lambda **kw: even_indices(x, y, 5, **kw),
                 lambda **kw: align_even(x, y, padded=True, pad_len=5, **kw)):
        with pytest.raises(ValueError, match=r'x_mapped.*\(40, 24\)'):
            call(x_mapped=np.zeros(shape))


def test_negative_or_fractional_counts_are_refused_by_train():
    import kwiiyatta_amd as k
    conv = k.MelCepstrumConverter(components=2)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match='align_iterations'):
            conv.train({}, [], align_iterations=bad)


def test_train_with_iterations_needs_an_aligned_dataset():
    import kwiiyatta_amd as k
    from kwiiyatta_amd.converter import AlignedDataset, TrimmedDataset
    conv = k.MelCepstrumConverter(components=2)
    with pytest.raises(ValueError, match='aligned dataset'):
        conv.train(TrimmedDataset({}), [], align_iterations=1)
    with pytest.raises(ValueError, match='pads'):
        conv.train(AlignedDataset(TrimmedDataset({}), pad_silence=False), [], align_iterations=1)


def test_stream_driver_is_refused():
    from kwiiyatta_amd import corpus as cp
    with pytest.raises(ValueError, match="align_iterations.*lockstep.*'streams'"):
        cp.train_converter_realigned([], 16000, components=2, align_iterations=1, driver='streams')
    with pytest.raises(ValueError, match="keep=True.*lockstep"):
        cp.build_training_matrix([], 16000, driver='streams', keep=True)
    with pytest.raises(ValueError, match='negative'):
        cp.train_converter_realigned([], 16000, components=2, align_iterations=-1)


# ---- the per-item path, host logic (numerics by the CPU oracle here, by the kernels under -m gpu) -----------------------------
def _numpy_mcd(a, b, idx_a=None, idx_b=None, **_):
    d = a[idx_a][:, 1:] - b[idx_b][:, 1:]
    v = 10.0 / np.log(10.0) * np.sqrt(2.0 * (d * d).sum(axis=1))
    return np.array([len(v), v.mean(), ((v - v.mean()) ** 2).sum()]), 0


def test_train_with_iterations_on_the_per_item_path(kwiiyatta, request, monkeypatch):
    """two short pairs, N = 2: fit 0 is the training of N = 0 (same matrix, same draws), every later matrix is the
    composition convert -> dtw_feature(x_mapped=) -> even_indices -> deltas of the ORIGINAL coefficients on the pads
    drawn once, and the record holds a row per fit"""
    from kwiiyatta_amd.backend import distortion
    from kwiiyatta_amd.backend.mlpg import DELTA_WINDOWS, delta_features
    from kwiiyatta_amd.converter import GMMFeatureConverter, PaddedDataset, TrimmedDataset, align_dataset
    from kwiiyatta_amd.converter.dataset import remove_zeros_frames
    from kwiiyatta_amd.synthetic import make_utterance
    from kwiiyatta_amd.vocoder.align import even_indices
    if request.node.callspec.params['kwiiyatta'] == 'oracle':
        monkeypatch.setattr(distortion, 'mcd', _numpy_mcd)
    kw = kwiiyatta
    fs = 16000
    pairs = {}
    for k in range(2):
        sides = [make_utterance(seed=s, fs=fs, seconds=0.5 + 0.1 * k, time_warp=w, formant_scale=f)[0]
                 for s, w, f in ((300 + k, 1.0, 1.0), (400 + k, 1.1, 1.12))]
        pairs[f'{k}'] = tuple(kw.Analyzer(kw.Wavdata(fs, x)) for x in sides)
    keys = sorted(pairs)

    class Recording(GMMFeatureConverter):
        def _train(self, dataarray, **options):
            self.matrices = getattr(self, 'matrices', []) + [np.array(dataarray)]
            self.models = getattr(self, 'models', [])
            super()._train(dataarray, **options)
            self.models.append((self.gmm.weights_.copy(), self.gmm.means_.copy(), self.gmm.covariances_.copy()))

    def stack():
        return kw.MelCepstrumConverter(use_delta=True, Converter=Recording, components=1, random_state=0, verbose=0)
    np.random.seed(3)
    plain = stack()
    plain.train(align_dataset(pairs), keys)
    state_zero = np.random.get_state()
    np.random.seed(3)
    conv = stack()
    conv.train(align_dataset(pairs), keys, align_iterations=2)
    state = np.random.get_state()
    assert state[0] == state_zero[0] and np.array_equal(state[1], state_zero[1]) and state[2:] == state_zero[2:]
    assert (conv.order, conv.fs, conv.frame_period) == (plain.order, plain.fs, plain.frame_period)
    assert len(conv.matrices) == 3 and np.array_equal(conv.matrices[0], plain.matrices[0])
    assert conv.align_iterations == 2 and [r['rows'] for r in conv.align_history] == [len(m) for m in conv.matrices]
    assert all(np.isfinite(r['mcd']) and r['mcd'] > 0 and r['em_iterations'] >= 1 for r in conv.align_history)
    # the composition, on the same pads: the same seed draws them again in the same order
    np.random.seed(3)
    padded = PaddedDataset(TrimmedDataset(pairs))
    for key in keys:
        a, b = padded[key]
        assert a.frame_len == padded.sides[key][0].frame_len and not hasattr(padded.sides[key][0], 'spectrum_envelope')
    with pytest.raises(ValueError, match='once'):
        padded[keys[0]]
    for it in (1, 2):
        gmm = conv.gmm
        gmm.weights_, gmm.means_, gmm.covariances_ = conv.models[it - 1]
        blocks = []
        for key in keys:
            x, y = padded.sides[key]
            mapped = conv.convert(kw.MelCepstrum(x.fs, x.frame_period, x.data), diff=False).data
            assert np.array_equal(mapped[:, 0], x.data[:, 0])
            xs, ys = even_indices(x, y, 100, x_mapped=mapped[:, 1:])
            blocks.append(remove_zeros_frames(np.hstack([delta_features(np.ascontiguousarray(s.data[i][:, 1:]), DELTA_WINDOWS)
                                                         for s, i in ((x, xs), (y, ys))])))
        assert np.array_equal(np.concatenate(blocks), conv.matrices[it]), it
    gmm.weights_, gmm.means_, gmm.covariances_ = conv.models[2]


def test_aligned_dataset_sits_on_the_padded_stage(kwiiyatta):
    """AlignedDataset(PaddedDataset(...), padded=True) gives what align_dataset gives, draw for draw"""
    from kwiiyatta_amd.converter import AlignedDataset, PaddedDataset, TrimmedDataset, align_dataset
    from kwiiyatta_amd.synthetic import make_utterance
    kw = kwiiyatta
    sides = [make_utterance(seed=s, fs=16000, seconds=0.5, time_warp=w, formant_scale=f)[0]
             for s, w, f in ((300, 1.0, 1.0), (400, 1.1, 1.12))]
    pairs = {'a': tuple(kw.Analyzer(kw.Wavdata(16000, x)) for x in sides)}
    np.random.seed(8)
    want = align_dataset(pairs)['a']
    state = np.random.get_state()
    np.random.seed(8)
    got = AlignedDataset(PaddedDataset(TrimmedDataset(pairs)), padded=True)['a']
    assert np.array_equal(np.random.get_state()[1], state[1])
    for a, b in zip(got, want):
        assert a.frame_len == b.frame_len > 50
        for slot in ('f0', 'spectrum_envelope', 'aperiodicity'):
            assert np.array_equal(getattr(a, slot), getattr(b, slot)), slot
        assert np.array_equal(a.mel_cepstrum.data, b.mel_cepstrum.data)
