"""Host side of the exemplar converter (--converter exemplar): option parsing, the table of options that do not go
with it, the model file's keys and the message for a model of the other kind.  No GPU: nothing here prepares a
spectrum or converts."""
import re
import sys

import numpy as np
import pytest

import nmf_cases as nc


def parsed(monkeypatch, argv, make=None):
    import kwiiyatta_amd as k
    monkeypatch.setattr(sys, 'argv', ['prog'] + [str(a) for a in argv])
    if make is None:
        conf = k.Config()
        conf.add_converter_arguments()
    else:
        conf = make()
    conf.parse_args()
    return conf


def test_options_and_defaults(monkeypatch):
    from kwiiyatta_amd.converter import exemplar
    conf = parsed(monkeypatch, [])
    assert conf.converter == 'gmm' and conf.converter_components == 64
    assert (conf.exemplars, conf.exemplar_iterations, conf.exemplar_sparsity, conf.exemplar_fft) == (None,) * 4
    assert conf.create_converter(use_delta=True).kind == 'gmm'
    conf = parsed(monkeypatch, ['--converter', 'exemplar'])
    stage = conf.create_converter(use_delta=True).base
    assert isinstance(stage, exemplar.ExemplarFeatureConverter)
    assert dict(exemplars=stage.exemplars, iterations=stage.iterations, sparsity=stage.sparsity,
                fft=stage.fft) == exemplar.DEFAULTS
    conf = parsed(monkeypatch, ['--converter', 'exemplar', '--exemplars', '256', '--exemplar-iterations', '25',
                                '--exemplar-sparsity', '0.2', '--exemplar-fft', '1024', '--mcep-fs', '16000'])
    conv = conf.create_converter(use_delta=True)
    stage = conv.base
    assert (stage.exemplars, stage.iterations, stage.sparsity, stage.fft, conv.mcep_fs) == (256, 25, 0.2, 1024, 16000)
    assert conv.kind == 'exemplar' and conv.gmm is None


def test_package_factory():
    import kwiiyatta_amd as k
    conv = k.MelCepstrumConverter(converter='exemplar', exemplars=8, exemplar_iterations=3, exemplar_sparsity=0.0,
                                  exemplar_fft=256, components=4, random_state=0)
    assert (conv.base.exemplars, conv.base.iterations, conv.base.fft) == (8, 3, 256)
    with pytest.raises(TypeError, match='covariance'):
        k.MelCepstrumConverter(converter='exemplar', covariance='block_diag')
    with pytest.raises(TypeError, match="converter='exemplar'"):
        k.MelCepstrumConverter(exemplars=8)
    with pytest.raises(ValueError, match='one of'):
        k.MelCepstrumConverter(converter='nmf')
    for bad in (dict(exemplars=0), dict(exemplars=8193), dict(exemplar_iterations=1001), dict(exemplar_iterations=-1),
                dict(exemplar_sparsity=-0.1), dict(exemplar_sparsity=float('nan')), dict(exemplar_fft=500)):
        with pytest.raises(ValueError):
            k.MelCepstrumConverter(converter='exemplar', **bad)


@pytest.mark.parametrize('argv, text', [
    (['--mlpg-em', '1'], '--mlpg-em does not go with --converter exemplar'),
    (['--mlpg-gv', '2'], '--mlpg-gv does not go with --converter exemplar'),
    (['--converter-covariance', 'full'], '--converter-covariance does not go with --converter exemplar'),
    (['--converter-components', '64'], '--converter-components does not go with --converter exemplar'),
    (['--convert-aperiodicity'], '--convert-aperiodicity does not go with --converter exemplar'),
    (['--nonparallel', '1'], '--nonparallel does not go with --converter exemplar'),
    (['--batch'], '--batch does not go with --converter exemplar'),
])
def test_what_does_not_go_with_it(monkeypatch, capsys, argv, text):
    """parser errors, raised by parse_args itself: no file is read (the directories do not exist)"""
    from kwiiyatta_amd import evaluate_voice
    base = ['--source', '/nonexistent/src', '--target', '/nonexistent/tgt', '--converter', 'exemplar']
    with pytest.raises(SystemExit):
        parsed(monkeypatch, base + argv, evaluate_voice.make_config)
    assert text in capsys.readouterr().err
    parsed(monkeypatch, base[:4] + argv, evaluate_voice.make_config)          # fine with the mixture


@pytest.mark.parametrize('argv, text', [
    (['--exemplars', '256'], '--exemplars needs --converter exemplar'),
    (['--exemplar-iterations', '5'], '--exemplar-iterations needs --converter exemplar'),
    (['--exemplar-sparsity', '0.1'], '--exemplar-sparsity needs --converter exemplar'),
    (['--exemplar-fft', '512'], '--exemplar-fft needs --converter exemplar'),
    (['--converter', 'exemplar', '--exemplars', '0'], r'outside \[1, 8192\]'),
    (['--converter', 'exemplar', '--exemplars', '8193'], r'outside \[1, 8192\]'),
    (['--converter', 'exemplar', '--exemplar-iterations', '1001'], r'outside \[0, 1000\]'),
    (['--converter', 'exemplar', '--exemplar-sparsity', '-1'], 'not a finite sparsity'),
    (['--converter', 'exemplar', '--exemplar-sparsity', 'nan'], 'not a finite sparsity'),
    (['--converter', 'exemplar', '--exemplar-fft', '500'], 'invalid choice'),
    (['--converter', 'nmf'], 'invalid choice'),
])
def test_option_errors(monkeypatch, capsys, argv, text):
    with pytest.raises(SystemExit):
        parsed(monkeypatch, argv)
    assert re.search(text, capsys.readouterr().err)


def toy_converter(kind):
    """a stack with made-up state, enough to be written to a model file (nothing is converted)"""
    import kwiiyatta_amd as k
    rng = np.random.default_rng(0)
    if kind == 'exemplar':
        conv = k.MelCepstrumConverter(converter='exemplar', exemplars=8, exemplar_iterations=3, exemplar_sparsity=0.25,
                                      exemplar_fft=256)
        conv._train(rng.normal(size=(21, 8)))
    else:
        conv = k.MelCepstrumConverter(use_delta=True, components=2, random_state=0)
        conv.gmm.weights_, conv.gmm.means_ = np.array([0.5, 0.5]), rng.normal(size=(2, 24))
        conv.gmm.covariances_ = np.stack([np.eye(24)] * 2)
        conv.base.frame_period = 5
    conv.order, conv.fs = 4, 16000
    return conv


def test_dictionary_rows_and_model_keys(tmp_path):
    import kwiiyatta_amd as k
    from kwiiyatta_amd.converter.exemplar import select_rows
    for rows, atoms in ((5, 8), (8, 8), (10, 4), (1809, 512)):
        assert select_rows(rows, atoms).tolist() == nc.select_rows(rows, atoms).tolist()
    conv = toy_converter('exemplar')
    joint = np.random.default_rng(0).normal(size=(21, 8))
    keep = [i * 21 // 8 for i in range(8)]
    assert np.array_equal(conv.base.source, joint[keep, :4]) and np.array_equal(conv.base.target, joint[keep, 4:])
    assert conv.base.rows == 21
    model = tmp_path / 'exemplar.npz'
    conv.save(model)
    with np.load(model) as z:
        assert str(z['converter']) == 'exemplar'
        assert {'exemplar_source', 'exemplar_target', 'exemplar_fft', 'exemplar_iterations',
                'exemplar_sparsity'} <= set(z.files)
        assert not {'weights', 'means', 'covariances'} & set(z.files)
        assert (int(z['exemplar_fft']), int(z['exemplar_iterations']), float(z['exemplar_sparsity'])) == (256, 3, 0.25)
    back = k.MelCepstrumConverter(converter='exemplar').load(model)
    assert np.array_equal(back.base.source, conv.base.source) and np.array_equal(back.base.target, conv.base.target)
    assert (back.base.fft, back.base.iterations, back.base.sparsity, back.base.rows) == (256, 3, 0.25, 21)
    assert (back.order, back.fs, back.base.fs) == (4, 16000, 16000)
    gmm_model = tmp_path / 'gmm.npz'
    toy_converter('gmm').save(gmm_model)
    with np.load(gmm_model) as z:                  # a mixture's file is what it was: no `converter` key
        assert 'converter' not in z.files and {'weights', 'means', 'covariances'} <= set(z.files)


def test_model_of_the_other_kind(monkeypatch, capsys, tmp_path):
    import kwiiyatta_amd as k
    models = {}
    for kind in ('exemplar', 'gmm'):
        models[kind] = tmp_path / f'{kind}.npz'
        toy_converter(kind).save(models[kind])
    with pytest.raises(ValueError, match='a model of the exemplar converter, not of the gmm converter'):
        k.MelCepstrumConverter(use_delta=True).load(models['exemplar'])
    with pytest.raises(ValueError, match='a model of the gmm converter, not of the exemplar converter'):
        k.MelCepstrumConverter(converter='exemplar').load(models['gmm'])
    conf = parsed(monkeypatch, ['--converter-model', models['exemplar']])
    with pytest.raises(SystemExit):
        conf.train_converter(use_delta=True)
    assert 'was trained with --converter exemplar, not gmm; retrain it with --converter gmm' in capsys.readouterr().err
    conf = parsed(monkeypatch, ['--converter-model', models['gmm'], '--converter', 'exemplar'])
    with pytest.raises(SystemExit):
        conf.train_converter(use_delta=True)
    assert 'was trained with --converter gmm, not exemplar' in capsys.readouterr().err
    conf = parsed(monkeypatch, ['--converter-model', models['exemplar'], '--converter', 'exemplar', '--exemplars', '4'])
    loaded = conf.train_converter(use_delta=True)           # the model decides
    assert loaded.kind == 'exemplar' and len(loaded.base.source) == 8 and loaded.base.iterations == 3
    conf = parsed(monkeypatch, ['--converter-model', models['gmm']])
    assert conf.train_converter(use_delta=True).kind == 'gmm'


def test_training_record_line():
    from kwiiyatta_amd import evaluate_voice as ev
    conv = toy_converter('exemplar')
    assert ev.training_record_lines(conv) == ['exemplar dictionary: 8 exemplars of 21 training rows, 129 bins, '
                                              '3 iterations, sparsity 0.25']
    assert ev.training_record_lines(toy_converter('gmm')) == []


def test_mixture_options_are_refused_by_the_stage():
    conv = toy_converter('exemplar')
    conv.base.bind_rate(16000)
    conv.base._spectra = (np.ones((8, 129)), np.ones((8, 129)))          # (never used: the call raises first)
    with pytest.raises(ValueError, match='no mixture: em'):
        conv.base.convert(np.zeros((3, 4)), em=2)
    with pytest.raises(TypeError):
        conv.base._train(np.zeros((4, 8)), max_iter=3)
