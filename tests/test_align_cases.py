"""The numpy statements of the alignment and training-set glue (tests/align_cases.py) against the package's host code
and the CPU oracle, without a GPU: vocoder.align's project_path_iter, dtw_feature(strict=...) and even_indices,
oracle.delta_features, np.trim_zeros and a literal hstack with the zero frames removed.  The long-gap, one-cell and
eps-boundary cases are among them, so what the GPU tests expect of the kernels is established here."""
import importlib
import types

import numpy as np
import pytest

import align_cases as ac


# ---- projection -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def project_cases():
    return ac.project_cases()


def test_project_equals_the_generator_on_every_case(project_cases):
    from kwiiyatta_amd.vocoder.align import project_path_iter
    for name, (path, trim_len) in project_cases.items():
        want = list(project_path_iter(path.tolist(), trim=trim_len > 0, trim_len=trim_len))   # (none of them raises)
        got = ac.project(path, trim_len)
        assert got.dtype == np.int32 and got.tolist() == want, name


def test_project_cases_are_what_their_names_say(project_cases):
    long, trim = project_cases['long']
    assert len(long) == 9001 and trim == 7 and len(ac.project(long, trim)) == ac.LONG_INDICES == long[-1, 1] + 1 - 14
    jumps = {}
    for name, (path, trim_len) in project_cases.items():
        dy = np.diff(np.r_[-1, path[:, 1]])
        jumps[name] = int(dy.max())
        if name.startswith(('gap_', 'two_long')) and not name.endswith('short'):
            assert len(ac.project(path, trim_len)) == ac.LONG_INDICES, name         # a gap is filled: nothing is lost
    assert jumps['gap_1500'] == 1501 and jumps['gap_tile_plus_1'] == ac.AL_TILE + 1
    assert jumps['gap_tile_plus_2'] == ac.AL_TILE + 2 and jumps['gap_tile'] == ac.AL_TILE
    assert jumps['gap_900_behind_600'] == 900 and jumps['gap_3000_two_flushes'] == 3001
    path, trim = project_cases['gap_900_behind_600']
    k = int(np.argmax(np.diff(path[:, 1]) > 1)) + 1                                   # the cell behind the jump
    assert k < ac.AL_TILE and path[k - 1, 1] - trim + 1 == 600                        # 600 indices out, in the first tile
    for name in ('gap_to_end', 'gap_to_end_short'):                                   # the jump lands behind the trimmed end
        path, trim = project_cases[name]
        k = int(np.argmax(np.diff(path[:, 1]) > 1)) + 1
        assert path[k, 1] == path[-1, 1] > path[-1, 1] - trim
    assert jumps['gap_to_end'] > ac.AL_TILE
    for name in ('backsteps_3000', 'late_start_3000', 'irregular_3000_trim0'):
        path, _ = project_cases[name]
        assert len(path) > 2 * ac.AL_TILE
    assert (np.diff(project_cases['backsteps_3000'][0][:, 1]) < 0).sum() >= 4
    assert project_cases['late_start_3000'][0][0].tolist() == [3, 40] and project_cases['irregular_3000_trim0'][1] == 0
    for name in ('last_y_below_trim', 'last_y_below_trim_gaps'):
        path, trim = project_cases[name]
        assert path[-1, 1] < trim and len(ac.project(path, trim)) == 0
    assert ac.project(*project_cases['one_cell_trim0']).tolist() == [0]
    assert ac.project(*project_cases['one_cell_trim3']).tolist() == []
    assert ac.project(*project_cases['one_cell_far_trim3']).tolist() == [-1, 1, 3, 5]
    assert len(ac.project(*project_cases['one_cell_far_trim0'])) == 10


def test_project_batch_mixes_regular_and_irregular_paths():
    from kwiiyatta_amd.vocoder.align import project_path_iter
    paths = ac.project_batch()
    assert len(paths) == ac.PROJECT_BATCH > ac.AL_BATCH
    irregular = [bool(((d := np.diff(np.r_[-1, p[:, 1]])) < 0).any() or (d > 1).any()) for p in paths]
    assert 10 < sum(irregular) < len(paths) - 10
    for p in paths:
        assert ac.project(p, 7).tolist() == list(project_path_iter(p.tolist(), trim=True, trim_len=7))


# ---- DTW features -----------------------------------------------------------------------------------------------------
def test_align_features_equal_make_feature():
    align = importlib.import_module('kwiiyatta_amd.vocoder.align')      # (the package exports a function of that name)
    for T in ac.FEATURE_T:
        for ncoef in ac.FEATURE_NCOEF:
            for mode in ac.FEATURE_MODES:
                mc, f0 = ac.feature_case(T, ncoef, mode)
                assert np.isfinite(mc).all()
                f = types.SimpleNamespace(f0=f0, resample_mel_cepstrum=lambda fs, mc=mc: types.SimpleNamespace(data=mc))
                want = align.make_feature(f, 16000, vuv='f0', vuv_weight=ac.VUV_WEIGHT, power_weight=ac.POWER_WEIGHT,
                                          power_threshold=ac.POWER_THRESHOLD)
                got = ac.align_features(mc, f0)
                assert ac.same(got, want), (T, ncoef, mode)
                if mode == 'edge' and T >= 7:
                    assert got[T // 3 + 1, 0] == ac.POWER_WEIGHT and got[T // 3 + 2, 0] == 0     # >= keeps the edge frame
                if mode == 'tied':
                    assert (got[[0, T // 2, T - 1], 0] == ac.POWER_WEIGHT).all()
    mc, f0 = ac.feature_case(9, 2, 'first')
    assert f0[:5].tolist() == list(ac.F0_SPECIALS) and ac.align_features(mc, f0)[:5, 1].tolist() == [0, 0, 9, 0, 9]


# ---- gather -----------------------------------------------------------------------------------------------------------
def test_gather_is_fancy_indexing_with_the_ends_clamped():
    src = np.arange(35.0).reshape(7, 5)
    idx = np.array([3, 3, 0, 6, 2, 3], dtype=np.int32)
    assert ac.same(ac.gather(src, idx), src[idx])
    assert ac.same(ac.gather(src, [-1, -2 ** 31, 7, 2 ** 31 - 1, 6]), src[[0, 0, 6, 6, 6]])   # no wrap, no failure
    assert ac.gather(src, np.zeros(0, dtype=np.int32)).shape == (0, 5)


# ---- trim length ------------------------------------------------------------------------------------------------------
def test_trim_length_equals_trim_zeros():
    from kwiiyatta_amd.converter.dataset import trim_zeros_frames
    lengths = {}
    for T in ac.TRIM_T:
        for K in ac.TRIM_K:
            for kind in ac.TRIM_KINDS:
                sp, eps = ac.trim_case(T, K, kind)
                mass = np.abs(sp).sum(axis=1)
                mass[mass < eps] = 0
                n = ac.trim_length(sp, eps)
                assert n == len(np.trim_zeros(mass)) == len(trim_zeros_frames(sp, eps)), (T, K, kind)
                lengths[T, K, kind] = n
    assert lengths[700, 513, 'zeros'] == 0 and lengths[700, 513, 'first'] == 1 == lengths[1, 1, 'last']
    assert lengths[700, 64, 'runs'] == 700 - 140 - 175 and lengths[257, 65, 'nan'] == 257 // 2 - 257 // 3 + 1
    # [below, at, ..., above, below]: the rows an ulp under eps are counted off, the row at eps and the one above stay
    assert lengths[700, 513, 'eps'] == 698 == lengths[700, 513, 'eps_two'] and lengths[5, 1, 'eps'] == 3
    assert lengths[1, 1, 'eps'] == 0 and lengths[3, 63, 'eps_two'] == 1


def test_rows_around_eps_are_exact_in_any_order():
    rng = np.random.default_rng(0)
    for eps in (ac.EPS, ac.EPS_TWO):
        for K in (1, 2, 63, 64, 65, 513):
            rows, zero = ac.eps_rows(K, eps)
            for _ in range(5):
                order = rng.permutation(K)
                sums = [float(np.sum(np.abs(r[order]))) for r in rows] + [float(sum(abs(v) for v in r[order][::-1])) for r in rows]
                assert sums == [eps, np.nextafter(eps, 0), np.nextafter(eps, 1)] * 2
            assert ac.same(ac.frame_is_zero(rows, eps), zero)


# ---- voicing and pad --------------------------------------------------------------------------------------------------
def test_is_voiced_at_its_two_edges():
    for fs, K in ac.VOICED_SHAPES:
        f0, ap = ac.voiced_case(fs, K, T=40)
        got = ac.is_voiced(f0, ap[:, 0], fs, K)
        # (f0 at / below / above the lowest voiced f0) x (ap0 at / below / above 0.999)
        assert got[:9].tolist() == [1, 1, 0, 0, 0, 0, 1, 1, 0]
        assert 0 < got[9:].sum() < len(got) - 9
    assert ac.lowest_f0(16000, 513) == 63.5 and ac.lowest_f0(8000, 3) == 8001.0


def test_pad_against_a_literal_pad_silence():
    for fs, K in ((16000, 65), (8000, 3)):
        for n in ac.PAD_N:
            for pad_len in ac.PAD_LEN:
                f0, ap = ac.voiced_case(fs, K, T=max(n, 1))
                ap_pad = np.full((n + 2 * pad_len, K), -7.0)
                ap_pad[pad_len:pad_len + n] = ap[:n]
                f0_pad, ap_out, voiced = ac.pad(f0, n, ap_pad, pad_len, fs, True)
                assert ac.same(f0_pad, np.r_[np.zeros(pad_len), f0[:n], np.zeros(pad_len)])
                assert (ap_out[:pad_len] == -7.0).all() and ac.same(ap_out[pad_len:pad_len + n], ap[:n])
                assert (ap_out[pad_len + n:] == 1 - 1e-12).all()
                full = np.vstack((np.full((pad_len, K), 1 - 1e-12), ap[:n], np.full((pad_len, K), 1 - 1e-12)))
                assert ac.same(voiced, ac.is_voiced(f0_pad, full[:, 0], fs, K))
                assert not voiced[:pad_len].any() and not voiced[pad_len + n:].any()
                assert ac.pad(f0, n, ap_pad, pad_len, fs, False)[2] is None


# ---- strict filter and cut --------------------------------------------------------------------------------------------
def _host_even(monkeypatch, path, fx, fy, strict, use_power, use_vuv, pad_len):
    """even_indices / dtw_feature of the package on a given path and given feature rows"""
    align = importlib.import_module('kwiiyatta_amd.vocoder.align')      # (the package exports a function of that name)
    a = types.SimpleNamespace(fs=16000, frame_len=len(fx), rows=fx)
    b = types.SimpleNamespace(fs=16000, frame_len=len(fy), rows=fy)
    monkeypatch.setattr(align, 'make_feature', lambda f, fs, **kw: f.rows)
    monkeypatch.setattr(align.fastdtw, 'fastdtw', lambda x, y, dist, radius: (0.0, [tuple(c) for c in path.tolist()]))
    kw = dict(strict=bool(strict), power='binalize' if use_power else None, vuv='voiced' if use_vuv else None)
    _, filtered = align.dtw_feature(a, b, **kw)
    xs, ys = align.even_indices(a, b, pad_len if pad_len > 0 else None, **kw)
    return filtered, xs, ys


def _check_even(monkeypatch, path, fx, fy, flags, pad_len, where):
    filtered, xs, ys = _host_even(monkeypatch, path, fx, fy, *flags, pad_len)
    assert ac.strict_filter(path, fx, fy, *flags).tolist() == filtered.tolist(), where
    gx, gy = ac.even(path, fx, fy, *flags, len(fx), len(fy), pad_len)
    assert gx.dtype == gy.dtype == np.int32 and gx.tolist() == xs.tolist() and gy.tolist() == ys.tolist(), where
    return gx, gy


def test_even_equals_the_host_code(monkeypatch):
    kept = []
    for cells in ac.EVEN_CELLS:
        path, fx, fy = ac.even_case(cells)
        assert len(path) == cells <= len(fx) + len(fy) + 4
        for flags in ac.FLAGS:
            for pad_len in (0, 5):
                gx, _ = _check_even(monkeypatch, path, fx, fy, flags, pad_len, (cells, flags, pad_len))
                kept.append(((cells, flags, pad_len), len(gx)))
    kept = dict(kept)
    assert kept[1300, (0, 1, 1), 0] == 1300 > kept[1300, (1, 1, 0), 0] > kept[1300, (1, 1, 1), 0] > 100
    assert kept[1300, (1, 0, 0), 0] == 1300 and 0 < kept[1300, (1, 1, 1), 5] < kept[1300, (1, 1, 1), 0]
    # the one-cell path: twice under strict, once without
    assert kept[1, (1, 1, 1), 0] == 2 and kept[1, (0, 1, 1), 0] == 1 and kept[1, (1, 0, 0), 0] == 2


def test_even_pins_the_voicing_test_on_column_zero_of_y(monkeypatch):
    path, fx, fy = ac.even_case(1300)
    assert 0.3 < np.mean((fy[:, 0] > 0) != (fy[:, 1] > 0)) < 0.7          # the columns disagree on many frames
    got = ac.strict_filter(path, fx, fy, 1, 0, 1)
    inner = path[1:-1]
    fixed = inner[(fx[inner[:, 0], 1] > 0) == (fy[inner[:, 1], 1] > 0)]   # what reading y's voicing column would keep
    as_is = inner[(fx[inner[:, 0], 1] > 0) == (fy[inner[:, 1], 0] > 0)]
    assert got[1:-1].tolist() == as_is.tolist() != fixed.tolist()
    _check_even(monkeypatch, path, fx, fy, (1, 0, 1), 0, 'vuv only')


def test_even_drops_the_cells_on_round_and_wavefront_boundaries(monkeypatch):
    path, fx, fy, drop = ac.even_boundary_case()
    for b in (63, 64, 255, 256, 257, 512, 1024):
        assert b in drop
    gx, gy = _check_even(monkeypatch, path, fx, fy, (1, 1, 0), 0, 'boundary')
    assert gx.tolist() == [v for v in range(1300) if v not in drop] == gy.tolist()
    gx, _ = _check_even(monkeypatch, path, fx, fy, (1, 1, 1), 5, 'boundary, cut')
    assert gx.tolist() == [v for v in range(5, 1295) if v not in drop]
    assert len(_check_even(monkeypatch, path, fx, fy, (0, 1, 1), 0, 'boundary, not strict')[0]) == 1300


def test_even_cuts_that_come_out_empty(monkeypatch):
    cases = ac.even_cut_cases()
    assert len(cases) == 5
    for name, path, fx, fy, pad_len in cases:
        for flags in ac.FLAGS:
            assert len(_check_even(monkeypatch, path, fx, fy, flags, pad_len, name)[0]) == 0, (name, flags)
        # ... and not because the path is empty: without the cut the cells are there
        assert len(_check_even(monkeypatch, path, fx, fy, (0, 1, 1), 0, name)[0]) == len(path)


# ---- delta features and joint rows ------------------------------------------------------------------------------------
def _delta_input(rng, n, d):
    x = rng.standard_normal((n, d))
    if n >= 3:
        x[1, 0], x[n - 1, d - 1], x[0, d // 2] = -0.0, np.inf, -np.inf
        x[2] = 0.0
    return x


def test_delta_equals_the_oracle_and_correlate():
    from oracle import oracle as ko
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 300):
        for d in (1, 24, 64, 65):
            x = _delta_input(rng, n, d)
            got = ac.delta(x)
            with np.errstate(invalid='ignore'):
                assert ac.same(got, ko.delta_features(x, ko.DELTA_WINDOWS)), (n, d)
                if n >= 3:
                    for c in {0, d // 2, d - 1}:
                        for k, (_, _, w) in enumerate(ko.DELTA_WINDOWS[1:], 1):
                            assert ac.same(got[:, k * d + c], np.correlate(x[:, c], w, 'same')), (n, d, c, k)
    assert ac.delta(np.zeros((0, 5))).shape == (0, 15)
    x = np.array([[1.0], [np.inf], [2.0]])
    assert np.isnan(ac.delta(x)[1, 1]) and ac.delta(x)[0, 1] == np.inf                 # 0.0 * inf of the row itself


def test_joint_equals_hstack_and_zero_frame_removal():
    from kwiiyatta_amd.converter.dataset import remove_zeros_frames
    counts = {}
    for n in ac.JOINT_N:
        for w in ac.JOINT_W:
            for kind in ac.JOINT_KINDS:
                xd, yd, eps = ac.joint_case(n, w, kind)
                got = ac.joint(xd, yd, eps)
                rows = np.hstack((xd, yd))
                mass = np.sum(np.abs(rows), axis=1)
                mass[mass < eps] = 0.0
                finite = ~np.isnan(mass)                                    # (a NaN row: below)
                assert ac.same(got[~np.isnan(got).any(axis=1)], rows[finite][mass[finite] > 0.0]), (n, w, kind)
                if finite.all():
                    assert ac.same(got, remove_zeros_frames(rows, eps))
                counts[n, w, kind] = len(got)
    assert counts[600, 144, 'all_dropped'] == 0 and counts[600, 1, 'none_dropped'] == 600
    assert counts[600, 72, 'marks'] == 600 - (10 + 1 + 12 + 6 - 2)          # 0, 64, .., 576; 599; 250..261 (256 twice); 509..514 (512 twice)
    assert counts[257, 65, 'marks'] == 257 - (5 + 1 + 7 - 2)                # 0, 64, 128, 192, 256; 256 again; 250..256
    # a NaN row has no norm below eps: the statement (and the kernel) keeps it, where the host's `mass > 0` drops it
    xd, yd, eps = ac.joint_case(65, 64, 'nan_eps')
    got = ac.joint(xd, yd, eps)
    assert np.isnan(got).any(axis=1).sum() == 1 and len(remove_zeros_frames(np.hstack((xd, yd)), eps)) == len(got) - 1
    # rows 0..2 are at eps, an ulp below, an ulp above: the middle one goes
    for kind in ('nan_eps', 'nan_eps_two'):
        xd, yd, eps = ac.joint_case(3, 72, kind)
        assert ac.same(ac.joint(xd, yd, eps), np.hstack((xd, yd))[[0, 2]])


def test_train_rows_are_the_composition(monkeypatch):
    from oracle import oracle as ko
    from kwiiyatta_amd.converter.dataset import remove_zeros_frames
    sizes = []
    for k, steps in enumerate(ac.TRAIN_STEPS):
        path, fx, fy, mc_x, mc_y = ac.train_pair(steps, 3, k)
        for flags, pad_len in (((1, 1, 1), 5), ((0, 1, 1), 0)):
            _, xs, ys = _host_even(monkeypatch, path, fx, fy, *flags, pad_len)
            want = np.hstack((ko.delta_features(mc_x[xs][:, 1:], ko.DELTA_WINDOWS),
                              ko.delta_features(mc_y[ys][:, 1:], ko.DELTA_WINDOWS))) if len(xs) else np.zeros((0, 18))
            want = remove_zeros_frames(want, ac.EPS)
            got = ac.train_rows(path, fx, fy, mc_x, mc_y, *flags, pad_len)
            assert ac.same(got, want), (steps, flags, pad_len)
            sizes.append((len(xs), len(got)))
    assert len(ac.TRAIN_STEPS) == 17 > ac.TR_PAIRS
    assert any(0 < rows < cells for cells, rows in sizes)                   # zero rows were removed somewhere
    assert len({rows for _, rows in sizes}) > 10                            # ragged
