"""`--source-f0-rate`: the pitch shifter in front of training, conversion and evaluation -- host logic on both backends.
For the oracle backend the shifter is the numpy statement of tests/pitch_cases.py and the log-f0 moments are numpy's
(the oracle has neither); the hip leg runs the kernels."""
import argparse
import pathlib
import shutil
import sys

import numpy as np
import pytest

import pitch_cases as pc
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


def _moments(tracks, ctx=None):
    out = np.zeros((len(tracks), 3))
    for row, f0 in zip(out, tracks):
        v = np.log(f0[f0 > 0])
        if len(v):
            row[:] = len(v), v.mean(), ((v - v.mean()) ** 2).sum()
    return out


def _merge(m, ctx=None):
    from test_f0_convert import chan_merge
    return np.array(chan_merge([tuple(r) for r in m]))


@pytest.fixture
def kw(kwiiyatta, request, monkeypatch):
    """the `kwiiyatta` fixture; its oracle leg also gets the numpy pitch shifter and numpy log-f0 moments"""
    if request.node.callspec.params['kwiiyatta'] == 'oracle':
        from kwiiyatta_amd.backend import f0 as f0map
        from kwiiyatta_amd.backend import pitch
        monkeypatch.setattr(pitch, 'shift_pitch', lambda x, fs, rate, positions=False, ctx=None:
                            pc.shift_pitch(x, fs, pitch.check_rate(rate), with_positions=positions))
        monkeypatch.setattr(f0map, 'logf0_moments', _moments)
        monkeypatch.setattr(f0map, 'merge_moments', _merge)
    return kwiiyatta


def _config(argv):
    import kwiiyatta_amd as k
    conf = k.Config(argparse.ArgumentParser())
    conf.add_converter_arguments()
    conf.parser.parse_args(argv, namespace=conf)
    return conf


def test_size_helpers_need_no_device_and_agree_with_the_yardstick():
    from kwiiyatta_amd.backend import pitch
    for fs in (8000, 16000, 22050, 44100, 48000, 96000):
        for n in (0, 1, 79, 441, 4800, 58960, 480000):
            for rate in (0.5, 0.8909, 1.0, 1.4983, 2.0):
                _, _, _, M, K = pc.constants(n, fs, rate)
                assert pitch.stretched_length(n, rate) == M and pitch.frames(n, fs, rate) == K
    for rate in (0.49, 2.5, float('nan')):
        with pytest.raises(ValueError, match='rate'):
            pitch.frames(1000, 16000, rate)
    with pytest.raises(ValueError):
        pitch.frames(1000, 50, 1.0)


# ---- the option ------------------------------------------------------------------------------------------------------
def test_option_parses_numbers_and_auto():
    assert _config([]).source_f0_rate is None and _config([]).resolve_source_f0_rate() == 1.0
    for text, rate in (('1', 1.0), ('0.5', 0.5), ('2.0', 2.0), ('1.4983', 1.4983)):
        conf = _config(['--source-f0-rate', text])
        assert conf.source_f0_rate == rate and conf.resolve_source_f0_rate() == rate
    assert _config(['--source-f0-rate', 'auto']).source_f0_rate == 'auto'


@pytest.mark.parametrize('text', ['0.49', '2.01', 'nan', 'inf', '-1', 'up'])
def test_rate_out_of_range_is_a_parser_error(text, capsys):
    import kwiiyatta_amd.convert_voice as cv
    import kwiiyatta_amd.evaluate_voice as ev
    assert '--source-f0-rate' in _parser_error(cv.main, ['--source-f0-rate', text, CLB_WAV], capsys)
    assert '--source-f0-rate' in _parser_error(ev.main, ['--source-f0-rate', text], capsys)


def test_auto_is_the_ratio_of_the_mean_log_f0(kw):
    """exp(mean voiced log-f0 of the target - of the source) over the training files' unshifted f0 tracks"""
    conf = _config(['--source', CLB_DIR, '--target', SLT_DIR, '--skip-files', '1', '--max-files', '2',
                    '--source-f0-rate', 'auto'])
    rate = conf.resolve_source_f0_rate()
    means = []
    for side in (CLB_DIR, SLT_DIR):
        logs = []
        for n in (2, 3):                      # the training keys: sorted, one skipped, two taken
            f0 = kw.analyze_wav(pathlib.Path(side) / f'arctic_a{n:04}.wav').f0
            logs.append(np.log(f0[f0 > 0]))
        means.append(np.concatenate(logs).mean())
    assert rate == pytest.approx(np.exp(means[1] - means[0]), rel=1e-12)
    assert 0.5 <= rate <= 2.0 and conf.resolve_source_f0_rate() == rate


def test_auto_outside_the_range_is_a_parser_error_naming_the_value(kw, monkeypatch, capsys):
    from kwiiyatta_amd.backend import f0 as f0map
    sides = iter((np.log(100.0), np.log(250.0)))
    monkeypatch.setattr(f0map, 'merge_moments', lambda m, ctx=None: np.array([10.0, next(sides), 1.0]))
    conf = _config(['--source', CLB_DIR, '--target', SLT_DIR, '--max-files', '1', '--source-f0-rate', 'auto'])
    with pytest.raises(SystemExit):
        conf.resolve_source_f0_rate()
    err = capsys.readouterr().err
    assert '--source-f0-rate auto' in err and '2.5000' in err


# ---- the model file --------------------------------------------------------------------------------------------------
def _stack(rate=None):
    from test_f0_convert import _trained_stack
    conv = _trained_stack()
    if rate is not None:
        conv.source_f0_rate = rate
    return conv


def test_model_round_trip_keeps_the_rate(tmp_path):
    import kwiiyatta_amd as k
    path = tmp_path / 'model.npz'
    assert _stack().source_f0_rate == 1.0
    _stack(1.4983).save(path)
    loaded = k.MelCepstrumConverter(components=2).load(path)
    assert loaded.source_f0_rate == 1.4983 and isinstance(loaded.source_f0_rate, float)
    with np.load(path) as z:
        assert str(z['format']) == loaded.MODEL_FORMAT          # the format string is unchanged


def test_old_model_loads_with_rate_one(tmp_path):
    import kwiiyatta_amd as k
    from test_f0_convert import _old_model
    path = tmp_path / 'old.npz'
    _old_model(path)
    assert k.MelCepstrumConverter(components=2).load(path).source_f0_rate == 1.0


def test_a_numeric_rate_that_conflicts_with_the_model_is_a_parser_error(tmp_path, capsys):
    import kwiiyatta_amd.convert_voice as cv
    import kwiiyatta_amd.evaluate_voice as ev
    path = tmp_path / 'model.npz'
    _stack(1.25).save(path)
    err = _parser_error(cv.main, ['--source-f0-rate', '1.5', '--converter-model', str(path), '--result-dir',
                                  str(tmp_path / 'out'), CLB_WAV], capsys)
    assert 'trained with --source-f0-rate 1.25' in err and 'retrain' in err and '1.5' in err
    assert not (tmp_path / 'out').exists()
    err = _parser_error(ev.main, ['--source', CLB_DIR, '--target', SLT_DIR, '--source-f0-rate', '1',
                                  '--converter-model', str(path)], capsys)
    assert 'trained with --source-f0-rate 1.25' in err and 'retrain' in err


def test_a_loaded_model_decides_the_rate(tmp_path):
    path = tmp_path / 'model.npz'
    _stack(1.25).save(path)
    for extra in ([], ['--source-f0-rate', 'auto'], ['--source-f0-rate', '1.25']):
        conf = _config(['--converter-model', str(path), '--converter-components', '2'] + extra)
        assert conf.train_converter(use_delta=True).source_f0_rate == 1.25        # (`auto` measures nothing here)


# ---- through the commands ----------------------------------------------------------------------------------------------
def _copy_training_files(tmp_path, count):
    src = tmp_path / 'src'
    src.mkdir()
    for n in range(1, count + 1):
        shutil.copy(pathlib.Path(CLB_DIR) / f'arctic_a{n:04}.wav', src)
    return src


def test_rate_one_never_calls_the_shifter(kw, monkeypatch, tmp_path):
    import kwiiyatta_amd.convert_voice as cv
    from kwiiyatta_amd.backend import pitch

    def refuse(*args, **kwargs):
        raise AssertionError('the pitch shifter was called at rate 1')
    monkeypatch.setattr(pitch, 'shift_pitch', refuse)
    monkeypatch.setattr(pitch, 'shift_pitch_batch_dev', refuse)
    src = _copy_training_files(tmp_path, 2)
    model = tmp_path / 'model.npz'
    inputs = [str(pathlib.Path(CLB_DIR) / 'arctic_a0009.wav')]
    np.random.seed(0)
    _run_cli(cv.main, ['--source', str(src), '--target', SLT_DIR, '--result-dir', str(tmp_path / 'a'), '--converter-seed',
                       '0', '--converter-components', '1', '--converter-model', str(model)] + inputs)
    with np.load(model) as z:
        assert float(z['source_f0_rate']) == 1.0
    _run_cli(cv.main, ['--result-dir', str(tmp_path / 'b'), '--converter-model', str(model), '--source-f0-rate', '1']
             + inputs)
    for kind in ('synth', 'diff'):
        assert (tmp_path / 'a' / f'arctic_a0009.{kind}.wav').read_bytes() == \
            (tmp_path / 'b' / f'arctic_a0009.{kind}.wav').read_bytes()


RATE = 1.25
# |median f0 ratio / RATE - 1| of the outputs.  The shifter alone is held to 2 % (test_pitch_cases.py); the MLSA filter
# and the 16-bit output sit between here, hence 3 %.
F0_MARGIN = 0.03


def test_both_outputs_follow_the_rate(kw, request, monkeypatch, tmp_path, capsys):
    """a one-component converter trained on shifted sources: the .diff.wav and the .synth.wav of convert_voice have
    RATE times the input's f0; training, conversion and the model file agree on the rate; on the GPU `--batch` writes
    the same files and evaluate_voice --batch the same figures"""
    import kwiiyatta_amd.convert_voice as cv
    from kwiiyatta_amd.backend import pitch
    from scipy.io import wavfile as sio
    calls = []
    real = pitch.shift_pitch

    def counted(x, fs, rate, *args, **kwargs):
        calls.append(rate)
        return real(x, fs, rate, *args, **kwargs)
    monkeypatch.setattr(pitch, 'shift_pitch', counted)
    src = _copy_training_files(tmp_path, 2)
    model = tmp_path / 'model.npz'
    names = ['arctic_a0008', 'arctic_a0009']
    inputs = [str(pathlib.Path(CLB_DIR) / f'{name}.wav') for name in names]
    np.random.seed(0)
    _run_cli(cv.main, ['--source', str(src), '--target', SLT_DIR, '--result-dir', str(tmp_path / 'a'), '--converter-seed',
                       '0', '--converter-components', '1', '--source-f0-rate', str(RATE), '--converter-model', str(model)]
             + inputs)
    with np.load(model) as z:
        assert float(z['source_f0_rate']) == RATE
    # the training files (a dataset analyses on every access) and every input once per output: all at the one rate
    assert len(calls) >= 2 + 2 * len(inputs) and set(calls) == {RATE}
    trained = len(calls)
    for name, wav in zip(names, inputs):
        f0_in = kw.analyze_wav(wav).f0
        for kind in ('diff', 'synth'):
            median, share = pc.f0_ratio(f0_in, kw.analyze_wav(tmp_path / 'a' / f'{name}.{kind}.wav').f0)
            print(f'{name}.{kind}: median f0 ratio / rate = {median / RATE:.4f} over {100 * share:.0f} % of the frames')
            assert share > 0.2 and abs(median / RATE - 1) <= F0_MARGIN, (name, kind)
    # the model decides in a later run: the same files bit for bit without the option
    _run_cli(cv.main, ['--result-dir', str(tmp_path / 'b'), '--converter-model', str(model)] + inputs)
    assert calls[trained:] == [RATE] * (2 * len(inputs))
    for name in names:
        for kind in ('diff', 'synth'):
            assert (tmp_path / 'a' / f'{name}.{kind}.wav').read_bytes() == \
                (tmp_path / 'b' / f'{name}.{kind}.wav').read_bytes(), (name, kind)
    if request.node.callspec.params['kwiiyatta'] != 'hip':
        return
    del calls[:]
    _run_cli(cv.main, ['--result-dir', str(tmp_path / 'c'), '--converter-model', str(model), '--batch'] + inputs)
    assert calls == []                  # the batch is shifted by the device call, no file goes through the host call
    for name in names:
        for kind in ('diff', 'synth'):
            _, a = sio.read(tmp_path / 'a' / f'{name}.{kind}.wav')
            _, c = sio.read(tmp_path / 'c' / f'{name}.{kind}.wav')
            assert a.shape == c.shape and c.dtype == np.int16
            assert np.abs(a.astype(np.int64) - c.astype(np.int64)).max() <= 1, (name, kind)      # 16-bit samples
    # evaluate_voice: its source side is shifted too, and --batch measures what the pair-by-pair path measures (the two
    # run the same kernels on bit-equal shifted waveforms and f0 tracks; they differ in how the mel-cepstra reach the
    # measure, 1e-12 relative by include/kwy.h -- 1e-9 dB leaves that room)
    import json
    import kwiiyatta_amd.evaluate_voice as ev
    common = ['--source', CLB_DIR, '--target', SLT_DIR, '--converter-model', str(model), '--eval-skip-files', '7',
              '--eval-max-files', '2']
    capsys.readouterr()
    np.random.seed(5)
    _run_cli(ev.main, common + ['--json', str(tmp_path / 'plain.json')])
    assert len(calls) >= 2 and set(calls) == {RATE}         # the source side of both pairs, through the host call
    del calls[:]
    np.random.seed(5)
    _run_cli(ev.main, common + ['--batch', '--json', str(tmp_path / 'batch.json')])
    assert calls == []                                      # ... and through the device call
    plain, batch = (json.loads((tmp_path / f'{n}.json').read_text()) for n in ('plain', 'batch'))
    for a, b in zip(batch['files'] + [batch['total']], plain['files'] + [plain['total']]):
        assert (a['frames'], a['aligned'], a['counts']) == (b['frames'], b['aligned'], b['counts'])
        assert abs(a['f0_rmse_cents'] - b['f0_rmse_cents']) <= 1e-9
        assert abs(a['mcd'] - b['mcd']) <= 1e-9 and abs(a['mcd_source'] - b['mcd_source']) <= 1e-9
    print(f"evaluate_voice: MCD {plain['total']['mcd']:.3f} dB, shifted source {plain['total']['mcd_source']:.3f} dB")
