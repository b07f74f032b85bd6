"""Host logic of non-parallel training (MelCepstrumFeatureConverter.train_nonparallel, --nonparallel) without a device:
the search and the monitor are served by numpy here (tests/nn_cases.py), the rest by the `kwiiyatta` fixture.  Which
files each side trains on, the order of the joint rows, the history, the model keys and the option checks."""
import os
import pathlib
import sys

import numpy as np
import pytest

import inca_cases
import nn_cases
from conftest import CLB_DIR, SLT_DIR

N = inca_cases.ORDER


@pytest.fixture
def numpy_search(kwiiyatta, monkeypatch):
    """backend.nn.nearest and backend.distortion.mcd in numpy: the training then needs no device under the oracle"""
    from kwiiyatta_amd.backend import distortion, nn

    def nearest(queries, candidates, splits=0, center=True, strict=True, ctx=None):
        idx, dist2 = nn_cases.nearest(queries, candidates)
        return idx, dist2.astype(np.float64)

    def mcd(a, b, idx_a=None, idx_b=None, first_col=1, **kwargs):
        rows = inca_cases.DB * np.sqrt(2.0 * ((a[idx_a, first_col:] - b[idx_b, first_col:]) ** 2).sum(axis=1))
        return np.array([len(rows), rows.mean(), ((rows - rows.mean()) ** 2).sum()]), 0
    monkeypatch.setattr(nn, 'nearest', nearest)
    monkeypatch.setattr(distortion, 'mcd', mcd)
    return kwiiyatta


recording_converter, small_set, expected_fit0 = (inca_cases.recording_converter, inca_cases.small_set,
                                                    inca_cases.expected_fit0)


def test_joint_rows_history_and_model_keys(numpy_search, tmp_path):
    kw = numpy_search
    src, tgt = small_set(quiet=True)
    source_keys, target_keys = ['s2', 's0', 's1'], ['t1', 't2']          # the callers' order is the rows' order
    conv = recording_converter(kw, components=1, random_state=0)
    conv.train_nonparallel(src, tgt, source_keys, target_keys, iterations=2)
    want, S, T, p, q = expected_fit0(src, tgt, source_keys, target_keys)
    assert len(S) == 180 - 3 and len(T) == 100 - 1 and S.shape[1] == 2 * N + 1
    assert set(S[:, 0]) == {0.0, 9.0}                                     # the voicing term of make_feature
    matrices = inca_cases.recorded_matrices(conv)
    assert len(matrices) == 3 and np.array_equal(matrices[0], want)
    for m in matrices[1:]:                                                # x is always the original source rows
        assert m.shape == want.shape
        assert np.array_equal(m[:len(S), :3 * N], want[:len(S), :3 * N])
        assert np.array_equal(m[len(S):, 3 * N:], want[len(S):, 3 * N:])
    history = conv.nonparallel_history
    assert conv.nonparallel == 2 and [r['rows'] for r in history] == [len(S) + len(T)] * 3
    monitor0 = inca_cases.mcd_db(np.vstack((S, S[q]))[:, 1:N + 1], np.vstack((T[p], T))[:, 1:N + 1])
    assert history[0]['mcd'] == pytest.approx(monitor0, rel=1e-12)
    assert all(np.isfinite(r['mcd']) and r['em_iterations'] >= 1 for r in history)
    assert history[-1]['mcd'] < history[0]['mcd']
    assert (conv.order, conv.fs, conv.align_iterations, conv.align_history) == (N, 16000, 0, [])

    path = tmp_path / 'model.npz'
    conv.save(path)
    with np.load(path) as z:
        assert int(z['nonparallel']) == 2 and z['nonparallel_history'].shape == (3, 3)
    back = kw.MelCepstrumConverter(use_delta=True).load(path)
    assert back.nonparallel == 2 and back.nonparallel_history == history
    assert np.array_equal(back.gmm.means_, conv.gmm.means_)

    conv.nonparallel, conv.nonparallel_history = None, []                 # a model trained on parallel data
    conv.save(path)
    with np.load(path) as z:
        assert 'nonparallel' not in z.files and 'nonparallel_history' not in z.files
    back = kw.MelCepstrumConverter(use_delta=True).load(path)
    assert back.nonparallel is None and back.nonparallel_history == []


def test_value_errors(numpy_search):
    kw = numpy_search
    src, tgt = small_set()
    keys = (sorted(src), sorted(tgt))

    def train(source=src, target=tgt, source_keys=keys[0], target_keys=keys[1], **kwargs):
        conv = kw.MelCepstrumConverter(use_delta=True, components=1, random_state=0)
        conv.train_nonparallel(source, target, source_keys, target_keys, **dict(dict(iterations=0), **kwargs))
        return conv
    with pytest.raises(ValueError, match='ap_model'):
        train(ap_model=True)
    for bad in (-1, 65, 1.5, True):
        with pytest.raises(ValueError, match=r'within \[0, 64\]'):
            train(iterations=bad)
    with pytest.raises(ValueError, match='no source files'):
        train(source_keys=[])
    with pytest.raises(ValueError, match='no target files'):
        train(target_keys=[])
    source, target = inca_cases.synthetic(3)
    with pytest.raises(ValueError, match='order 5'):
        train(target=dict(tgt, t1=inca_cases.Utterance(target[1][:, :5])))
    with pytest.raises(ValueError, match='does not resample'):
        train(target=dict(tgt, t1=inca_cases.Utterance(target[1], fs=22050)))
    with pytest.raises(ValueError, match='frame_period'):
        train(source=dict(src, s2=inca_cases.Utterance(source[2], frame_period=10)))
    with pytest.raises(ValueError, match='delta stage'):
        kw.MelCepstrumConverter(use_delta=False, components=1).train_nonparallel(src, tgt, *keys, iterations=0)
    conv = train()
    assert conv.nonparallel == 0 and len(conv.nonparallel_history) == 1
    assert train(iterations=None).nonparallel == type(conv).NONPARALLEL_DEFAULT


# ---- the options ----------------------------------------------------------------------------------------------------
@pytest.fixture
def disjoint_dirs(tmp_path):
    """source: clb a0001 - a0004, target: slt a0003 - a0007, as directories of links"""
    dirs = []
    for name, origin, numbers in (('src', CLB_DIR, range(1, 5)), ('tgt', SLT_DIR, range(3, 8))):
        d = tmp_path / name
        d.mkdir()
        for n in numbers:
            os.symlink(os.path.join(origin, f'arctic_a{n:04}.wav'), d / f'arctic_a{n:04}.wav')
        dirs.append(d)
    return dirs


def parsed(kw, monkeypatch, argv, make=None):
    monkeypatch.setattr(sys, 'argv', ['prog'] + [str(a) for a in argv])
    if make is None:
        conf = kw.Config()
        conf.add_converter_arguments()
    else:
        conf = make()
    conf.parse_args()
    return conf


class Recorder:
    """stands in for the converter stack: remembers what Config hands to the training"""
    nonparallel = None

    def train_nonparallel(self, *args, **kwargs):
        self.args, self.kwargs = args, kwargs

    def train(self, *args, **kwargs):
        raise AssertionError('the parallel training was called')


def test_each_side_picks_its_own_files(numpy_search, monkeypatch, disjoint_dirs):
    kw = numpy_search
    src, tgt = disjoint_dirs
    conf = parsed(kw, monkeypatch, ['--source', src, '--target', tgt, '--nonparallel', '3', '--skip-files', '1',
                                    '--max-files', '3'])
    rec = conf._train(Recorder(), f0_stats=True, gv_stats=True)
    source, target, source_keys, target_keys = rec.args
    names = lambda keys: [pathlib.Path(k).name for k in keys]      # noqa: E731
    assert names(source_keys) == [f'arctic_a{n:04}.wav' for n in (2, 3, 4)]      # sorted(keys)[skip:][:max] per side
    assert names(target_keys) == [f'arctic_a{n:04}.wav' for n in (4, 5, 6)]
    assert rec.kwargs == dict(iterations=3, f0_stats=True, gv_stats=True)
    assert source.data_dir == src and target.data_dir == tgt and rec.source_f0_rate == 1.0
    conf = parsed(kw, monkeypatch, ['--source', src, '--target', tgt, '--nonparallel'])
    assert conf.nonparallel == kw.converter.MelCepstrumFeatureConverter.NONPARALLEL_DEFAULT
    rec = conf._train(Recorder())
    assert len(rec.args[2]) == 4 and len(rec.args[3]) == 5 and rec.kwargs == dict(iterations=conf.nonparallel)
    conf = parsed(kw, monkeypatch, ['--source', src, '--target', tgt])
    assert conf.nonparallel is None


def test_parser_errors(numpy_search, monkeypatch, capsys, disjoint_dirs, tmp_path):
    kw = numpy_search
    from kwiiyatta_amd import evaluate_voice
    src, tgt = disjoint_dirs
    base = ['--source', src, '--target', tgt]
    for argv, make, text in (
            (['--nonparallel', '65'], None, r'outside \[0, 64\]'),
            (['--nonparallel', '-1'], None, r'outside \[0, 64\]'),
            (['--nonparallel', 'x'], None, 'invalid iteration count'),
            (['--nonparallel', '1', '--align-iterations', '1'], None, 'does not go with --align-iterations'),
            (['--nonparallel', '1', '--align-iterations', '0'], None, 'does not go with --align-iterations'),
            (['--nonparallel', '1', '--convert-aperiodicity'], evaluate_voice.make_config,
             'does not go with --convert-aperiodicity')):
        with pytest.raises(SystemExit):
            parsed(kw, monkeypatch, base + argv, make)
        assert __import__('re').search(text, capsys.readouterr().err), argv

    # a model file trained with another value
    s, t = small_set()
    conv = kw.MelCepstrumConverter(use_delta=True, components=1, random_state=0)
    conv.train_nonparallel(s, t, sorted(s), sorted(t), iterations=1)
    model = tmp_path / 'model.npz'
    conv.save(model)
    conf = parsed(kw, monkeypatch, base + ['--converter-model', model, '--nonparallel', '2'])
    with pytest.raises(SystemExit):
        conf.train_converter(use_delta=True)
    assert 'was trained with --nonparallel 1, not with --nonparallel 2' in capsys.readouterr().err
    for argv in (['--nonparallel', '1'], []):                 # the same value, or none asked: the model decides
        conf = parsed(kw, monkeypatch, base + ['--converter-model', model] + argv)
        assert conf.train_converter(use_delta=True).nonparallel == 1
    conv.nonparallel, conv.nonparallel_history = None, []
    conv.save(model)
    conf = parsed(kw, monkeypatch, base + ['--converter-model', model, '--nonparallel', '2'])
    with pytest.raises(SystemExit):
        conf.train_converter(use_delta=True)
    assert 'was trained on parallel data, not with --nonparallel 2' in capsys.readouterr().err


def test_record_lines_and_overlap(numpy_search):
    from kwiiyatta_amd import evaluate_voice as ev

    class Trained:
        nonparallel = 1
        nonparallel_history = [dict(rows=10, mcd=7.25, em_iterations=3), dict(rows=10, mcd=6.5, em_iterations=4)]
        align_iterations, align_history = 0, []
    assert ev.training_record_lines(Trained()) == ['non-parallel fit 0: rows 10 monitor MCD 7.250 dB',
                                                   'non-parallel fit 1: rows 10 monitor MCD 6.500 dB']
    Trained.nonparallel = None
    assert ev.training_record_lines(Trained()) == []
