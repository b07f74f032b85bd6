"""--f0-estimator on the command line and in the converter model file; no GPU."""
import numpy as np
import pytest


def config(monkeypatch, *args):
    import sys
    import kwiiyatta_amd as k
    monkeypatch.setattr(sys, 'argv', ['prog', *args])
    conf = k.Config()
    conf.add_converter_arguments()
    conf.parse_args()
    return conf


def test_option_defaults_to_dio_and_reaches_the_analyzers(monkeypatch):
    from kwiiyatta_amd.config import VOCODER_OPTIONS
    assert dict(VOCODER_OPTIONS)['--f0-estimator']['default'] == 'dio'
    seen = []
    make = lambda *a, **kw: seen.append(kw)        # noqa: E731
    conf = config(monkeypatch)
    assert conf.f0_estimator == 'dio'
    conf.create_analyzer('x.wav', Analyzer=make)
    conf = config(monkeypatch, '--f0-estimator', 'pyin')
    conf.create_analyzer('x.wav', Analyzer=make)
    assert seen == [dict(frame_period=5, mcep_order=24), dict(frame_period=5, mcep_order=24, f0_estimator='pyin')]
    with pytest.raises(SystemExit):
        config(monkeypatch, '--f0-estimator', 'harvest')


class _Loaded:
    kind, source_f0_rate, align_iterations, nonparallel, covariance = 'gmm', 1.0, 0, None, 'full'
    f0_stats = gv_stats = gv_var = ms_stats = ap_converter = None

    def __init__(self, trained_with):
        self.trained_with = trained_with

    def load(self, path):
        self.f0_estimator = self.trained_with


@pytest.mark.parametrize('trained, asked, fine', [('dio', 'dio', True), ('pyin', 'pyin', True), ('dio', 'pyin', False),
                                                  ('pyin', 'dio', False)])
def test_a_loaded_model_keeps_its_estimator(monkeypatch, tmp_path, capsys, trained, asked, fine):
    model = tmp_path / 'model.npz'
    np.savez(model, format='x')
    conf = config(monkeypatch, '--converter-model', str(model), '--f0-estimator', asked)
    monkeypatch.setattr(conf, 'create_converter', lambda **kw: _Loaded(trained))
    if fine:
        assert conf.train_converter().f0_estimator == asked
    else:
        with pytest.raises(SystemExit):
            conf.train_converter()
        assert f'trained with --f0-estimator {trained}, not {asked}' in capsys.readouterr().err


@pytest.mark.parametrize('estimator', ['dio', 'pyin'])
def test_model_file_carries_the_key(tmp_path, estimator):
    """written by training with pyin; a file without it was trained with dio (such files stay what they were)"""
    import kwiiyatta_amd as k
    c = k.MelCepstrumConverter(components=2)
    c.gmm.weights_ = np.array([0.5, 0.5])
    c.gmm.means_ = np.zeros((2, 150))
    c.gmm.covariances_ = np.stack([np.eye(150)] * 2)
    c.order, c.fs, c.f0_estimator = 24, 16000, estimator
    path = tmp_path / 'model.npz'
    c.save(path)
    with np.load(path) as z:
        assert ('f0_estimator' in z.files) == (estimator == 'pyin')
    assert k.MelCepstrumConverter(components=2).load(path).f0_estimator == estimator
