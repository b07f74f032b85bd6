"""Non-parallel training on the device (MelCepstrumFeatureConverter.train_nonparallel, --nonparallel): identical sides,
the joint rows against the numpy gather, the monitor on the synthetic set of tests/inca_cases.py, the model file, and
the two commands on directories that share no file name."""
import os
import sys

import numpy as np
import pytest

import inca_cases
from conftest import CLB_DIR, SLT_DIR

pytestmark = pytest.mark.gpu

N = inca_cases.ORDER


def matrices_of(conv):
    return inca_cases.recorded_matrices(conv)


def test_identical_sides_pair_with_themselves():
    """the target's features are the source's: p and q are the identity, every joint row has x == y and the monitor is
    exactly 0"""
    import kwiiyatta_amd as kw
    source, _ = inca_cases.synthetic(5)
    source = [m[:120] for m in source[:2]]
    src, tgt = inca_cases.datasets(source, [m.copy() for m in source])
    conv = inca_cases.recording_converter(kw, components=1, random_state=0, verbose=0)
    conv.train_nonparallel(src, tgt, ['s0', 's1'], ['t0', 't1'], iterations=0)
    (joint,) = matrices_of(conv)
    assert joint.shape == (480, 6 * N)
    assert np.array_equal(joint[:, :3 * N], joint[:, 3 * N:])
    assert np.array_equal(joint[:240], joint[240:])                   # p = q = identity
    assert conv.nonparallel_history == [dict(rows=480, mcd=0.0, em_iterations=conv.gmm.n_iter_)]


def test_joint_rows_equal_the_numpy_gather():
    """fit 0 on well separated rows, with frames that are not speech and unvoiced stretches: the matrix is the numpy
    gather along the reference's indices, bit for bit; the monitor is the reference's"""
    import kwiiyatta_amd as kw
    src, tgt = inca_cases.small_set(quiet=True)
    source_keys, target_keys = ['s2', 's0', 's1'], ['t1', 't2']
    conv = inca_cases.recording_converter(kw, components=1, random_state=0, verbose=0)
    conv.train_nonparallel(src, tgt, source_keys, target_keys, iterations=0)
    want, S, T, p, q = inca_cases.expected_fit0(src, tgt, source_keys, target_keys)
    (joint,) = matrices_of(conv)
    assert np.array_equal(joint, want)
    monitor = inca_cases.mcd_db(np.vstack((S, S[q]))[:, 1:N + 1], np.vstack((T[p], T))[:, 1:N + 1])
    assert conv.nonparallel_history[0]['mcd'] == pytest.approx(monitor, rel=1e-12)
    assert conv.nonparallel_history[0]['rows'] == len(S) + len(T) == 276


def test_the_monitor_falls_on_the_synthetic_set(tmp_path):
    """the synthetic set laid out as mel-cepstra of order 8, N = 3, one component: the last monitor is strictly below
    the first, the rows of every fit are the speech frames of both sides; the model file keeps the record"""
    import kwiiyatta_amd as kw
    source, target = inca_cases.synthetic(0)
    src, tgt = inca_cases.datasets(source, target)
    conv = inca_cases.recording_converter(kw, components=1, random_state=0, verbose=0)
    conv.train_nonparallel(src, tgt, sorted(src), sorted(tgt), iterations=3, f0_stats=True, gv_stats=True)
    history = conv.nonparallel_history
    print('monitor: ' + ' -> '.join(f'{r["mcd"]:.4f}' for r in history) + ' dB')
    assert len(history) == 4 and conv.nonparallel == 3
    assert [r['rows'] for r in history] == [3 * 300 + 3 * 280] * 4
    assert history[-1]['mcd'] < history[0]['mcd']
    assert all(np.isfinite(r['mcd']) for r in history)
    xs = np.concatenate(source)
    for m in matrices_of(conv):                              # always the original source rows
        assert np.array_equal(m[:900, :N], xs)
    assert conv.f0_stats is not None and conv.gv_stats.shape == (N + 1,) and conv.gv_var.shape == (N + 1,)
    # the first fit saw what the numpy INCA's first fit saw (static columns; same search, same order)
    want = inca_cases.expected_fit0(src, tgt, sorted(src), sorted(tgt))[0]
    assert np.array_equal(matrices_of(conv)[0], want)

    path = tmp_path / 'model.npz'
    conv.save(path)
    back = kw.MelCepstrumConverter(use_delta=True).load(path)
    assert back.nonparallel == 3 and back.nonparallel_history == history
    out = back.convert(src['s0'].mel_cepstrum, diff=False)
    assert np.array_equal(out.data, conv.convert(src['s0'].mel_cepstrum, diff=False).data)
    conv.nonparallel, conv.nonparallel_history = None, []    # a file from before the feature has neither key
    conv.save(path)
    assert kw.MelCepstrumConverter(use_delta=True).load(path).nonparallel is None


def test_value_errors():
    import kwiiyatta_amd as kw
    src, tgt = inca_cases.small_set()
    conv = kw.MelCepstrumConverter(use_delta=True, components=1, random_state=0, verbose=0)
    with pytest.raises(ValueError, match='ap_model'):
        conv.train_nonparallel(src, tgt, sorted(src), sorted(tgt), iterations=0, ap_model=True)
    with pytest.raises(ValueError, match=r'within \[0, 64\]'):
        conv.train_nonparallel(src, tgt, sorted(src), sorted(tgt), iterations=65)
    with pytest.raises(ValueError, match='no target files'):
        conv.train_nonparallel(src, tgt, sorted(src), [], iterations=0)
    with pytest.raises(ValueError, match='transform length'):
        conv.train_nonparallel(src, tgt, sorted(src), sorted(tgt), iterations=0, ms_stats=True, ms_length=1000)
    bad = dict(tgt, t0=inca_cases.Utterance(np.full((50, N), np.nan)))
    with pytest.raises(ValueError, match='no finite score'):
        conv.train_nonparallel(src, bad, sorted(src), ['t0'], iterations=0)


# ---- through the commands ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def disjoint(tmp_path_factory):
    """source: clb a0001 - a0003, target: slt a0004 - a0006: directories of links that share no file name"""
    root = tmp_path_factory.mktemp('disjoint')
    dirs = []
    for name, origin, numbers in (('clb', CLB_DIR, (1, 2, 3)), ('slt', SLT_DIR, (4, 5, 6))):
        d = root / name
        d.mkdir()
        for n in numbers:
            os.symlink(os.path.join(origin, f'arctic_a{n:04}.wav'), d / f'arctic_a{n:04}.wav')
        dirs.append(d)
    return root, dirs[0], dirs[1]


def run_main(main, argv, capsys):
    old = sys.argv
    sys.argv = ['prog'] + [str(a) for a in argv]
    try:
        np.random.seed(0)
        main()
    finally:
        sys.argv = old
    return capsys.readouterr()


def test_convert_voice_trains_on_disjoint_files(disjoint, capsys):
    import kwiiyatta_amd.convert_voice as cv
    root, src, tgt = disjoint
    model = root / 'model.npz'
    wav = src / 'arctic_a0001.wav'
    common = [wav, '--source', src, '--target', tgt, '--nonparallel', '1', '--converter-components', '2',
              '--converter-seed', '0', '--converter-model', model]
    run_main(cv.main, common + ['--result-dir', root / 'single'], capsys)
    with np.load(model) as z:
        assert int(z['nonparallel']) == 1 and z['nonparallel_history'].shape == (2, 3)
        assert (z['nonparallel_history'][:, 0] > 600).all() and np.isfinite(z['nonparallel_history']).all()
        assert int(z['align_iterations']) == 0
    run_main(cv.main, common + ['--result-dir', root / 'batch', '--batch'], capsys)      # (loads the model)
    import kwiiyatta_amd as kw
    for where in ('single', 'batch'):
        for suffix in ('diff', 'synth'):
            out = kw.load_wav(root / where / f'arctic_a0001.{suffix}.wav')
            assert out.fs == 16000 and len(out.data) > 16000 and np.isfinite(out.data).all() and np.abs(out.data).max() > 0


def test_evaluate_voice_prints_a_line_per_fit(disjoint, capsys):
    """the evaluated files are still the common ones: a0003 of clb's and slt's full directories, while the training
    took a0001, a0002 of clb and a0001, a0002 of slt -- each directory's own first two"""
    import kwiiyatta_amd.evaluate_voice as ev
    out = run_main(ev.main, ['--source', CLB_DIR, '--target', SLT_DIR, '--max-files', '2', '--eval-skip-files', '2',
                             '--eval-max-files', '1', '--converter-components', '2', '--converter-seed', '0',
                             '--nonparallel', '1'], capsys)
    lines = [line for line in out.out.splitlines() if line.startswith('non-parallel fit')]
    assert len(lines) == 2 and lines[0].startswith('non-parallel fit 0: rows ') and 'monitor MCD' in lines[1]
    assert 'warning' not in out.err
    assert 'total (1 of 1 files)' in out.out
    out = run_main(ev.main, ['--source', CLB_DIR, '--target', SLT_DIR, '--max-files', '3', '--eval-skip-files', '2',
                             '--eval-max-files', '1', '--converter-components', '1', '--converter-seed', '0',
                             '--nonparallel', '0'], capsys)
    assert 'were also trained on' in out.err and 'arctic_a0003.wav' in out.err
