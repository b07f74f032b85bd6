"""What tests/eval_cases.py (the numpy statement of the objective evaluation measures) claims, checked without a
GPU, and the host-side bookkeeping of the `evaluate_voice` command: its options, file slices, overlap warning and
JSON layout."""
import json
import math
import sys

import numpy as np
import pytest

import eval_cases as ec


# ---- the yardstick's own claims ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cols', ec.COLS)
def test_distortion_of_a_matrix_with_itself_is_zero(cols):
    rng = np.random.RandomState(cols)
    a, _ = ec.matrices(rng, 300, 1, cols)
    rows, status = ec.mcd_rows(a, a.copy())
    assert status == 0 and not rows.any() and ec.moments(rows).tolist() == [300.0, 0.0, 0.0]
    ia, _ = ec.index_lists(rng, 200, 300, 300)
    rows, _ = ec.mcd_rows(a, a.copy(), ia, ia)
    assert not rows.any() and len(rows) == 200


@pytest.mark.parametrize('k, delta', [(1, 1.0), (24, 0.125), (24, -0.5), (7, 2.0 ** -10), (63, 3.0)])
def test_constant_offset_on_k_coefficients(k, delta):
    """(10 / ln 10) sqrt(2 k) |delta|: on integers the sum of squares is exact, so only the square root and the
    product round -- once in the yardstick and once in the closed form, plus the rounding of sqrt(2 k) there"""
    a = np.random.RandomState(k).randint(-8, 8, size=(50, 64)).astype(np.float64)
    b = a.copy()
    b[:, 1:1 + k] += delta
    rows, _ = ec.mcd_rows(a, b)
    want = ec.DB * math.sqrt(2 * k) * abs(delta)
    assert np.all(np.abs(rows - want) <= 4 * ec.U * want)
    # first_col: c0 is left out by default, counted with first_col=0
    b = a.copy()
    b[:, 0] += delta
    assert not ec.mcd_rows(a, b)[0].any()
    assert np.all(np.abs(ec.mcd_rows(a, b, first_col=0)[0] - ec.DB * math.sqrt(2) * abs(delta)) <= 4 * ec.U * want)


def test_index_lists_offsets_and_masks():
    rng = np.random.RandomState(1)
    a, b = ec.matrices(rng, 40, 30, 25)
    ia, ib = ec.index_lists(rng, 100, 40, 30, 100, 7)
    assert ia.dtype == np.int32 and np.any(np.diff(ia) < 0) and np.any(np.diff(ia) == 0)       # not monotone, repeats
    rows, status = ec.mcd_rows(a, b, ia, ib, 100, 7)
    direct = ec.mcd_rows(np.ascontiguousarray(a[ia - 100]), np.ascontiguousarray(b[ib - 7]))[0]
    assert status == 0 and rows.tobytes() == direct.tobytes()
    for kind, count in (('set', 100), ('clear', 0)):
        masked, _ = ec.mcd_rows(a, b, ia, ib, 100, 7, mask=ec.mask_vector(rng, 37, kind))
        assert (~np.isnan(masked)).sum() == count
    mask = ec.mask_vector(rng, 37, 'mixed')
    masked, _ = ec.mcd_rows(a, b, ia, ib, 100, 7, mask=mask)
    assert np.array_equal(~np.isnan(masked), mask[ib] > 0)                 # the UNSHIFTED b-side index
    assert masked[mask[ib] > 0].tobytes() == rows[mask[ib] > 0].tobytes()
    # not finite: left out and counted; beyond either matrix: passed over; no rows: zeros
    bad = a.copy()
    bad[ia[3] - 100, 5] = np.nan
    rows, status = ec.mcd_rows(bad, b, ia, ib, 100, 7)
    assert status == (ia == ia[3]).sum() and np.isnan(rows[ia == ia[3]]).all()
    far = ia.copy()
    far[:4] = 140, 99, 1000, -5
    rows, status = ec.mcd_rows(a, b, far, ib, 100, 7)
    assert status == 0 and np.isnan(rows[:4]).all() and not np.isnan(rows[4:]).any()
    assert ec.moments(ec.mcd_rows(a[:0], b[:0])[0]).tolist() == [0.0, 0.0, 0.0]


def test_merging_equals_the_moments_of_the_concatenation():
    rng = np.random.RandomState(2)
    for sizes in ((5, 300, 64), (0, 1, 0, 2049, 7, 0), (1, 1, 1, 1), (4097,), (0, 0)):
        parts = [rng.standard_normal(n) * 3 + 7 for n in sizes]
        merged = ec.merge([ec.moments(p) for p in parts])
        whole = ec.moments(np.concatenate(parts))
        mean_b, m2_b = ec.merge_bound(parts)
        assert merged[0] == whole[0] == sum(sizes)
        assert abs(merged[1] - whole[1]) <= mean_b and abs(merged[2] - whole[2]) <= m2_b, sizes
        if sum(sizes):
            assert m2_b <= 1e-9 * max(whole[2], 1.0)                  # (the bound says something)
    # grouping does not matter to the fold: a merged head stands for its rows
    triples = [ec.moments(rng.standard_normal(n)) for n in (3, 0, 50, 8, 1)]
    assert ec.merge([ec.merge(triples[:3])] + triples[3:]).tobytes() == ec.merge(triples).tobytes()


def test_f0_figures_on_hand_made_tracks():
    fa = np.array([0.0, 100.0, 200.0, 0.0, 400.0, 150.0])
    fb = np.array([0.0, 200.0, 100.0, 120.0, 0.0, 150.0])
    counts, m, status, vals = ec.f0_error(fa, fb)
    assert counts.tolist() == [3, 1, 1, 1] and status == 0 and vals.tolist() == [-1200.0, 1200.0, 0.0]
    assert m.tolist() == [3.0, 0.0, 2 * 1200.0 ** 2] and ec.rmse(m) == math.sqrt(2 * 1200.0 ** 2 / 3)
    # a semitone up on every voiced frame: 100 cents, no spread
    counts, m, _, _ = ec.f0_error(fa * 2 ** (1 / 12), fa)
    assert counts.tolist() == [4, 0, 0, 2] and abs(m[1] - 100) <= 1e-10 and abs(ec.rmse(m) - 100) <= 1e-10
    # through an alignment, and with frames that cannot be judged
    ia, ib = np.array([105, 104, 103, 101, 100, 106], dtype=np.int32), np.array([8, 11, 10, 7, 7, 8], dtype=np.int32)
    counts, m, status, vals = ec.f0_error(fa, fb, ia, ib, 100, 7)         # (the last row lies beyond track a)
    assert counts.tolist() == [1, 2, 1, 1] and status == 0 and vals.tolist() == [1200.0 * np.log2(150.0 / 200.0)]
    odd = fa.copy()
    odd[1], odd[2] = np.nan, -5.0
    counts, m, status, _ = ec.f0_error(odd, fb)
    assert status == 2 and counts.tolist() == [1, 1, 1, 1]
    assert np.isnan(ec.rmse(ec.f0_error(np.zeros(4), np.zeros(4))[1]))


# ---- the command's bookkeeping ---------------------------------------------------------------------------------------------
def _parse(argv, monkeypatch):
    from kwiiyatta_amd import evaluate_voice as ev
    monkeypatch.setattr(sys, 'argv', ['evaluate_voice'] + argv)
    conf = ev.make_config()
    conf.parse_args()
    return conf


def test_option_defaults(monkeypatch):
    conf = _parse(['--source', 'a', '--target', 'b'], monkeypatch)
    assert conf.eval_skip_files == 0 and conf.eval_max_files is None           # the evaluated slice: every common file
    assert conf.gv == 0.0 and conf.convert_f0 is False and conf.transpose_key == 0.0 and conf.frames == 'speech'
    assert conf.batch is False and conf.json is None
    # Config's vocoder and converter options, unchanged
    assert (conf.frame_period, conf.mcep_order, conf.converter_components) == (5, 24, 64)
    assert conf.skip_files is None and conf.max_files is None and conf.converter_model is None and conf.mcep_fs is None
    conf = _parse(['--source', 'a', '--target', 'b', '--eval-skip-files', '3', '--eval-max-files', '2', '--gv', '--frames',
                   'all', '--convert-f0', '--transpose-key', '-2.5', '--batch', '--json', 'out.json', '--max-files', '3',
                   '--converter-model', 'm.npz'], monkeypatch)
    assert (conf.eval_skip_files, conf.eval_max_files, conf.gv, conf.frames) == (3, 2, 1.0, 'all')
    assert conf.convert_f0 and conf.transpose_key == -2.5 and conf.batch and conf.json == 'out.json'
    assert conf.max_files == 3 and conf.converter_model == 'm.npz'
    assert _parse(['--gv', '0.25'], monkeypatch).gv == 0.25


@pytest.mark.parametrize('argv', [['--eval-skip-files', '-1'], ['--eval-max-files', '0'], ['--eval-max-files', 'x'],
                                  ['--gv', '1.5'], ['--gv', '-0.1'], ['--transpose-key', '100'], ['--frames', 'voiced']])
def test_option_ranges(argv, monkeypatch, capsys):
    with pytest.raises(SystemExit):
        _parse(argv, monkeypatch)
    assert 'error' in capsys.readouterr().err


def test_file_slices_and_the_overlap_warning():
    from kwiiyatta_amd import evaluate_voice as ev
    keys = [f'arctic_a{n:04}.wav' for n in (3, 1, 2, 5, 4)]
    assert ev.file_slice(keys, 0, None) == sorted(keys) == ev.file_slice(keys, None, None)
    assert ev.file_slice(keys, 3, None) == sorted(keys)[3:] and ev.file_slice(keys, 1, 2) == sorted(keys)[1:3]
    assert ev.file_slice(keys, 5, None) == []
    trained, held_out = ev.file_slice(keys, None, 3), ev.file_slice(keys, 3, None)
    assert ev.overlap_warning(trained, held_out) is None
    line = ev.overlap_warning(trained, ev.file_slice(keys, 2, 2))
    assert line.startswith('warning: 1 evaluated file(s)') and line.endswith('arctic_a0003.wav') and '\n' not in line
    line = ev.overlap_warning(trained, keys)
    assert '3 evaluated file(s)' in line and line.endswith('arctic_a0001.wav, arctic_a0002.wav, arctic_a0003.wav')


def test_result_figures_and_json_layout():
    from kwiiyatta_amd import evaluate_voice as ev
    one = ev.Result((200.0, 6.5, 80.0), (200.0, 8.25, 120.0), (3.0, 0.0, 2 * 1200.0 ** 2), (3, 1, 1, 1), 260, outside=4)
    assert (one.frames, one.mcd, one.mcd_source, one.aligned, one.outside) == (200, 6.5, 8.25, 260, 4)
    assert one.f0_rmse_cents == math.sqrt(2 * 1200.0 ** 2 / 3) and one.vuv_error == 2 / 6 and one.counts == (3, 1, 1, 1)
    none = ev.Result((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0, 0, 0, 0), 0)
    assert none.frames == 0 and all(math.isnan(v) for v in (none.mcd, none.mcd_source, none.f0_rmse_cents, none.vuv_error))
    assert 'MCD nan dB' in none.line('x.wav') and none.line('x.wav').startswith('x.wav: frames 0 ')
    assert one.line('a.wav') == ('a.wav: frames 200 MCD 6.500 dB (source 8.250 dB) f0 RMSE 979.8 cents '
                                 'V/UV error 33.33 %')
    options = dict(gv=0.5, convert_f0=False, transpose_key=0.0, frames='speech')
    doc = ev.report(['a.wav', 'b.wav'], [one, none], one, options)
    doc = json.loads(json.dumps(doc, allow_nan=False))                      # plain JSON: nan travels as null
    assert sorted(doc) == ['files', 'options', 'total'] and doc['options'] == options
    record = doc['files'][0]
    assert sorted(record) == ['aligned', 'counts', 'f0_frames', 'f0_rmse_cents', 'frames', 'mcd', 'mcd_source', 'name',
                              'outside', 'vuv_error']
    assert record['name'] == 'a.wav' and record['counts'] == dict(vv=3, vu=1, uv=1, uu=1) and record['f0_frames'] == 3
    assert (record['frames'], record['mcd'], record['mcd_source']) == (200, 6.5, 8.25)
    assert doc['files'][1]['mcd'] is None and doc['files'][1]['vuv_error'] is None and doc['files'][1]['frames'] == 0
    assert doc['total']['files'] == 1 and doc['total']['mcd'] == 6.5 and 'name' not in doc['total']
    for frames in ('voiced', None):
        with pytest.raises(ValueError, match='frames must be'):
            ev.evaluate_pair(None, None, None, frames=frames)
    with pytest.raises(ValueError, match=r'outside \[0, 1\]'):
        ev.evaluate_pair(None, None, None, gv=1.5)
