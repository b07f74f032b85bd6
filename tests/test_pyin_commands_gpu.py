"""convert_voice and evaluate_voice with --f0-estimator pyin, per file and --batch: the f0 tracks the commands really
work on are pYIN's (not DIO's), and the same on both paths."""
import pathlib
import sys

import numpy as np
import pytest

from conftest import CLB_DIR, SLT_DIR

pytestmark = pytest.mark.gpu

FILE = 'arctic_a0003.wav'
TRAIN = ['--source', CLB_DIR, '--target', SLT_DIR, '--max-files', '1', '--converter-components', '2', '--converter-seed',
         '0', '--source-f0-rate', '1.1']


def run(monkeypatch, main, argv):
    monkeypatch.setattr(sys, 'argv', ['prog'] + [str(a) for a in argv])
    np.random.seed(0)
    main()


@pytest.fixture
def tracks(monkeypatch):
    """every f0 track the analyzers extract (per-file paths) and the device drivers extract (batch paths), by length"""
    from kwiiyatta_amd import corpus, evaluate_voice
    from kwiiyatta_amd.vocoder.world import WorldAnalyzer
    seen = dict(analyzer=[], wave=[], shifted=[])
    extract, run_wave, shifted = WorldAnalyzer.extract_f0, corpus.ConvertWave.run, evaluate_voice._shifted_triples

    def spy_extract(self, *a, **kw):
        fresh = self._f0 is None
        f0 = extract(self, *a, **kw)
        if fresh:
            seen['analyzer'].append((self._f0_from, np.array(self.data), np.array(f0)))
        return f0

    def spy_run(self):
        run_wave(self)
        if self.wav_in:
            corpus.torch.cuda.synchronize()
            seen['wave'] += [(self.f0_estimator, x.cpu().numpy(), f.cpu().numpy()) for x, f in zip(self.x, self.f0)]

    def spy_shifted(*a, **kw):
        out = shifted(*a, **kw)
        seen['shifted'] += [(kw.get('f0_estimator', 'dio'), x.cpu().numpy(), f.cpu().numpy()) for x, f, _ in out]
        return out

    monkeypatch.setattr(WorldAnalyzer, 'extract_f0', spy_extract)
    monkeypatch.setattr(corpus.ConvertWave, 'run', spy_run)
    monkeypatch.setattr(evaluate_voice, '_shifted_triples', spy_shifted)
    return seen


def references(x, fs):
    """(pYIN's, DIO's) refined track of a waveform, from the backend entries themselves"""
    from kwiiyatta_amd.backend import world
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = []
    for coarse_track in (world.pyin, world.dio):
        coarse, t = coarse_track(x, fs)
        out.append(world.stonemask(x, coarse, t, fs))
    return out


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    """a converter trained by evaluate_voice itself with --f0-estimator pyin (one file, shifted source)"""
    from kwiiyatta_amd import evaluate_voice
    path = tmp_path_factory.mktemp('pyin') / 'model.npz'
    with pytest.MonkeyPatch.context() as m:
        run(m, evaluate_voice.main, TRAIN + ['--converter-model', path, '--f0-estimator', 'pyin', '--eval-skip-files', '2',
                                              '--eval-max-files', '1'])
    with np.load(path) as z:
        assert str(z['f0_estimator']) == 'pyin' and float(z['source_f0_rate']) == 1.1
    return path


def test_convert_voice_per_file_and_batch_work_on_the_same_pyin_track(model, tracks, monkeypatch, tmp_path):
    from kwiiyatta_amd import convert_voice
    wav = pathlib.Path(CLB_DIR) / FILE
    common = ['--converter-model', model, '--f0-estimator', 'pyin', '--no-diffvc', wav]
    run(monkeypatch, convert_voice.main, ['--result-dir', tmp_path / 'file'] + common)
    per_file = [rec for rec in tracks['analyzer']]
    assert len(per_file) == 1 and not tracks['wave']
    run(monkeypatch, convert_voice.main, ['--result-dir', tmp_path / 'batch', '--batch'] + common)
    assert len(tracks['wave']) == 1
    (est_a, x_a, f0_a), (est_b, x_b, f0_b) = per_file[0], tracks['wave'][0]
    assert est_a == est_b == 'pyin'
    assert np.array_equal(x_a, x_b)                    # the shifted waveform, from the host and from the device shifter
    assert np.array_equal(f0_a, f0_b)
    pyin_track, dio_track = references(x_b, 16000)
    assert np.array_equal(f0_b, pyin_track) and not np.array_equal(f0_b, dio_track)
    assert (tmp_path / 'file' / FILE).with_suffix('.synth.wav').is_file()
    assert (tmp_path / 'batch' / FILE).with_suffix('.synth.wav').is_file()


def test_evaluate_voice_per_file_and_batch_work_on_the_same_pyin_tracks(model, tracks, monkeypatch, tmp_path):
    import json
    from kwiiyatta_amd import evaluate_voice
    common = ['--source', CLB_DIR, '--target', SLT_DIR, '--converter-model', model, '--f0-estimator', 'pyin',
              '--eval-skip-files', '2', '--eval-max-files', '1']
    run(monkeypatch, evaluate_voice.main, common + ['--json', tmp_path / 'file.json'])
    per_file = list(tracks['analyzer'])
    assert len(per_file) == 2 and all(est == 'pyin' for est, _, _ in per_file) and not tracks['shifted']
    del tracks['analyzer'][:]
    run(monkeypatch, evaluate_voice.main, common + ['--batch', '--json', tmp_path / 'batch.json'])
    assert len(tracks['shifted']) == 1 and tracks['shifted'][0][0] == 'pyin'
    # source: the shifted waveform analysed on the device; target: an analyzer, as per file
    _, x_s, f0_s = tracks['shifted'][0]
    source = next(rec for rec in per_file if len(rec[2]) == len(f0_s) and np.array_equal(rec[1], x_s))
    target = next(rec for rec in per_file if rec is not source)
    assert np.array_equal(source[2], f0_s)
    assert any(np.array_equal(target[2], f0) and est == 'pyin' for est, _, f0 in tracks['analyzer'])
    for _, x, f0 in (source, target):
        pyin_track, dio_track = references(x, 16000)
        assert np.array_equal(f0, pyin_track) and not np.array_equal(f0, dio_track)
    a, b = (json.loads((tmp_path / n).read_text())['total'] for n in ('file.json', 'batch.json'))
    assert a['counts'] == b['counts'] and a['frames'] == b['frames']


def test_the_other_estimator_is_refused_for_the_trained_model(model, monkeypatch, capsys):
    from kwiiyatta_amd import evaluate_voice
    with pytest.raises(SystemExit):
        run(monkeypatch, evaluate_voice.main, ['--source', CLB_DIR, '--target', SLT_DIR, '--converter-model', model])
    assert 'trained with --f0-estimator pyin, not dio' in capsys.readouterr().err
