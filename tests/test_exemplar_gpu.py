"""The exemplar converter end to end on the 16 kHz fixtures: trained on a0001 - a0003 with small settings (256
exemplars, 25 iterations), a0008 converted both ways, the model file, the evaluation, and the options of convert_voice
that work on the converted mel-cepstrum.

"Converted distortion < unconverted" is asserted: at this small setting the measured margin
(profiles/exemplar_quality.json, `small/256/0.05/25 on a0001-a0003`) is 0.87 dB over both held-out sentences (6.728
against 7.601 dB) and 1.93 dB on a0008 alone, the sentence evaluated here (6.097 against 8.031 dB), above the 0.5 dB
the assertion was made to depend on."""
import pathlib
import sys

import numpy as np
import pytest

from conftest import CLB_DIR, SLT_DIR

pytestmark = pytest.mark.gpu

HELD_OUT = 'arctic_a0008.wav'
SETTINGS = dict(exemplars=256, exemplar_iterations=25, exemplar_sparsity=0.05, exemplar_fft=512)


@pytest.fixture(scope='module', autouse=True)
def keep_global_random_state():
    """training and evaluation draw their silence pads from numpy's global generator, and tests elsewhere in the suite
    read that generator without seeding it: leave it as this module found it"""
    state = np.random.get_state()
    yield
    np.random.set_state(state)


@pytest.fixture(scope='module')
def dataset():
    import kwiiyatta_amd as k
    return k.align(k.WavFileDataset(pathlib.Path(CLB_DIR)), k.WavFileDataset(pathlib.Path(SLT_DIR)))


@pytest.fixture(scope='module')
def trained(dataset, tmp_path_factory):
    import kwiiyatta_amd as k
    keys = sorted(dataset.keys())[:3]
    conv = k.MelCepstrumConverter(converter='exemplar', **SETTINGS)
    np.random.seed(0)
    conv.train(dataset, keys, gv_stats=True)
    model = tmp_path_factory.mktemp('exemplar') / 'model.npz'
    conv.save(model)
    return conv, model


@pytest.fixture(scope='module')
def source():
    import kwiiyatta_amd as k
    return k.analyze_wav(pathlib.Path(CLB_DIR) / HELD_OUT)


def config(monkeypatch, argv=()):
    import kwiiyatta_amd as k
    monkeypatch.setattr(sys, 'argv', ['prog'] + [str(a) for a in argv])
    conf = k.Config()
    conf.add_converter_arguments()
    conf.parse_args()
    return conf


def test_dictionary(trained):
    conv, _ = trained
    stage = conv.base
    assert conv.kind == 'exemplar' and (conv.order, conv.fs, stage.fs) == (24, 16000, 16000)
    assert stage.source.shape == stage.target.shape == (256, 24) and stage.rows > 256
    S, Tg = stage.dictionaries()
    assert S.shape == Tg.shape == (256, 257) and (S > 0).all() and (Tg > 0).all()
    assert np.abs(S.sum(axis=1) - 1).max() < 1e-14 and np.abs(Tg.sum(axis=1) - 1).max() < 1e-14
    # the preparation: the amplitude envelope exp(sum_m c_m cos(m w~)) with c0 = 0; back through sp2mc it is c1..cN
    from kwiiyatta_amd.backend import sptk
    # (the round trip truncates the warped cepstrum at the transform's half length, so it is not exact; coefficients
    # are of size 0.1 .. 1 and a hundredth of that is far below what the conversion changes)
    back = sptk.sp2mc(S * S, order=24, alpha=sptk.mcepalpha(16000))[:, 1:]
    print('round trip of the preparation: largest coefficient error', np.abs(back - stage.source).max())
    assert np.abs(back - stage.source).max() < 1e-2


def test_convert_both_ways(trained, source):
    conv, _ = trained
    mc = source.mel_cepstrum
    plain, diff = conv.convert(mc, diff=False), conv.convert(mc, diff=True)
    for out in (plain, diff):
        assert out.data.shape == mc.data.shape and np.isfinite(out.data).all()
        assert np.array_equal(out.data[:, 0], mc.data[:, 0])          # c0 is the source's
    assert np.allclose(diff.data[:, 1:], plain.data[:, 1:] - mc.data[:, 1:], rtol=0, atol=1e-12)
    assert np.abs(plain.data[:, 1:] - mc.data[:, 1:]).max() > 1e-3    # it does convert
    again = conv.convert(mc, diff=False)
    assert np.array_equal(again.data, plain.data)
    # an exemplar of the dictionary is explained by itself: its activations concentrate on atoms like it
    stage = conv.base
    _, H = stage.convert(stage.source[:4], return_h=True)
    assert H.shape == (4, 256) and (H >= 0).all()


def test_model_round_trip(trained, source):
    import kwiiyatta_amd as k
    conv, model = trained
    with np.load(model) as z:
        assert str(z['converter']) == 'exemplar'
        assert z['exemplar_source'].shape == z['exemplar_target'].shape == (256, 24)
        assert (int(z['exemplar_fft']), int(z['exemplar_iterations']), float(z['exemplar_sparsity'])) == (512, 25, 0.05)
        assert 'gv_stats' in z.files and 'weights' not in z.files
    back = k.MelCepstrumConverter(converter='exemplar').load(model)
    mc = source.mel_cepstrum
    for diff in (False, True):
        assert np.array_equal(back.convert(mc, diff=diff).data, conv.convert(mc, diff=diff).data)
    assert np.array_equal(back.convert(mc, gv=1.0).data, conv.convert(mc, gv=1.0).data)


def test_gmm_model_is_what_it_was(dataset, source, monkeypatch, tmp_path):
    """the default path is untouched: a mixture trained, saved (no `converter` key), loaded through the package and
    through Config converts bit for bit as the object that was trained"""
    import kwiiyatta_amd as k
    conv = k.MelCepstrumConverter(use_delta=True, components=2, random_state=0)
    np.random.seed(0)
    conv.train(dataset, sorted(dataset.keys())[:2])
    model = tmp_path / 'gmm.npz'
    conv.save(model)
    with np.load(model) as z:
        assert 'converter' not in z.files and not [n for n in z.files if n.startswith('exemplar')]
    mc = source.mel_cepstrum
    want = [conv.convert(mc, diff=diff).data for diff in (False, True)]
    loaded = [k.MelCepstrumConverter(use_delta=True).load(model),
              config(monkeypatch, ['--converter-model', model]).train_converter(use_delta=True)]
    for back in loaded:
        assert back.kind == 'gmm'
        for diff, data in zip((False, True), want):
            assert np.array_equal(back.convert(mc, diff=diff).data, data)


def test_evaluate_pair(trained, dataset):
    import kwiiyatta_amd as k
    from kwiiyatta_amd.converter.mcep import _trimmed_stage
    conv, _ = trained
    np.random.seed(0)
    r = k.evaluate_pair(conv, *_trimmed_stage(dataset)[HELD_OUT])
    print(f'exemplar 256 x 25 on three sentences, {HELD_OUT}: {r.mcd:.3f} dB converted, {r.mcd_source:.3f} dB unconverted, '
          f'{r.frames} frames')
    assert r.frames > 100 and np.isfinite(r.mcd) and np.isfinite(r.mcd_source)
    assert r.mcd < r.mcd_source


@pytest.mark.parametrize('diffvc, options', [(False, dict(gv=1.0)), (True, dict(gv=1.0)),
                                             (False, dict(postfilter=0.2, keep_power=True)),
                                             (True, dict(postfilter=0.2, keep_power=True)),
                                             (True, dict(diff_filter='fft'))])
def test_convert_voice_options(trained, source, monkeypatch, diffvc, options):
    from kwiiyatta_amd import convert_voice
    conv, _ = trained
    conf = config(monkeypatch)
    wav = convert_voice.convert(conf, conv, pathlib.Path(CLB_DIR) / HELD_OUT, diffvc=diffvc, **options)
    assert wav.fs == 16000 and np.isfinite(wav.data).all() and np.abs(wav.data).max() > 0
    assert abs(len(wav.data) - len(source.wavdata.data)) <= 16000 * 0.005 * 2


def test_realignment_runs_without_a_mixture(dataset):
    """--align-iterations needs `convert` between its passes only"""
    import kwiiyatta_amd as k
    conv = k.MelCepstrumConverter(converter='exemplar', **SETTINGS)
    np.random.seed(0)
    conv.train(dataset, sorted(dataset.keys())[:2], align_iterations=1)
    assert len(conv.align_history) == 2 and conv.base.source.shape == (256, 24)
    assert all(np.isfinite(r['mcd']) and r['rows'] > 256 for r in conv.align_history)


@pytest.mark.parametrize('argv, text', [
    (['--mlpg-em', '1'], '--mlpg-em does not go with'), (['--mlpg-gv', '1'], '--mlpg-gv does not go with'),
    (['--converter-covariance', 'block_diag'], '--converter-covariance does not go with'),
    (['--converter-components', '4'], '--converter-components does not go with'),
    (['--convert-aperiodicity'], '--convert-aperiodicity does not go with'),
    (['--batch'], '--batch does not go with')])
def test_parser_errors(monkeypatch, capsys, argv, text):
    from kwiiyatta_amd import evaluate_voice
    monkeypatch.setattr(sys, 'argv', ['prog', '--source', CLB_DIR, '--target', SLT_DIR, '--converter', 'exemplar'] + argv)
    with pytest.raises(SystemExit):
        evaluate_voice.make_config().parse_args()
    assert text in capsys.readouterr().err


def test_model_of_the_other_kind_is_a_parser_error(trained, monkeypatch, capsys):
    _, model = trained
    conf = config(monkeypatch, ['--converter-model', model])
    with pytest.raises(SystemExit):
        conf.train_converter(use_delta=True)
    assert 'was trained with --converter exemplar, not gmm' in capsys.readouterr().err
    conf = config(monkeypatch, ['--converter-model', model, '--converter', 'exemplar'])
    assert conf.train_converter(use_delta=True).kind == 'exemplar'
