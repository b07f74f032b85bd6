"""Objective evaluation on the MI355X: the distortion, f0 error and merge kernels of kwy_eval.hip through the C ABI
against their numpy statement (tests/eval_cases.py), their determinism and input edges."""
import numpy as np
import pytest

import eval_cases as ec

pytestmark = pytest.mark.gpu


def _device():
    """device, stream, context: the tests upload from pageable memory (complete on return), launch on the stream,
    synchronise it and read back"""
    import torch
    from kwiiyatta_amd import _lib
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    return dev, stream, _lib.Context(0, stream=stream.cuda_stream)


def _mcd_cases(seed, cols, lengths=ec.LENGTHS):
    """per length: identity indexing (equal row counts), then gathered indexing with offsets and each kind of mask"""
    rng = np.random.RandomState(seed)
    for n in lengths:
        a, b = ec.matrices(rng, n, n, cols)
        yield dict(a=a, b=b)
        rows_a, rows_b = max(1, n // 2 + 3), max(1, n // 3 + 5)
        a, b = ec.matrices(rng, rows_a, rows_b, cols)
        off_a, off_b = 100, 7
        ia, ib = ec.index_lists(rng, n, rows_a, rows_b, off_a, off_b)
        for kind in ('set', 'clear', 'mixed'):
            yield dict(a=a, b=b, idx_a=ia, idx_b=ib, off_a=off_a, off_b=off_b, mask=ec.mask_vector(rng, rows_b + off_b, kind))
        yield dict(a=a, b=b, idx_a=ia, idx_b=ib, off_a=off_a, off_b=off_b)


def _want(case, first_col=1):
    return ec.mcd_rows(case['a'], case['b'], case.get('idx_a'), case.get('idx_b'), case.get('off_a', 0),
                       case.get('off_b', 0), case.get('mask'), first_col)


def _check_mcd(case, cols, first_col, moments, status, rows):
    want, want_status = _want(case, first_col)
    k = cols - first_col
    assert status == want_status
    assert rows.shape == want.shape
    assert np.array_equal(np.isnan(rows), np.isnan(want))
    used = ~np.isnan(want)
    err, bound = np.abs(rows[used] - want[used]), ec.row_bound(want[used], k)
    assert np.all(err <= bound), (len(want), cols, first_col)
    wm = ec.moments(want)
    assert moments[0] == wm[0]
    mean_b, m2_b = ec.moments_bounds(want[used], bound.max() if used.any() else 0.0)
    assert abs(moments[1] - wm[1]) <= mean_b, (len(want), cols, moments[1], wm[1], mean_b)
    assert abs(moments[2] - wm[2]) <= m2_b, (len(want), cols, moments[2], wm[2], m2_b)
    worst = (err / np.maximum(bound, 1e-300)).max() if used.any() else 0.0
    return worst, abs(moments[1] - wm[1]) / mean_b if mean_b else 0.0, abs(moments[2] - wm[2]) / m2_b if m2_b else 0.0


@pytest.mark.parametrize('cols', ec.COLS)
def test_mcd_against_numpy(cols):
    from kwiiyatta_amd.backend import distortion as dist
    worst = np.zeros(3)
    for first_col in sorted({0, min(1, cols)}):
        for case in _mcd_cases(cols, cols):
            moments, status, rows = dist.mcd(first_col=first_col, per_row=True, **case)
            worst = np.maximum(worst, _check_mcd(case, cols, first_col, moments, status, rows))
    print(f'mcd cols={cols}: worst error / bound: rows {worst[0]:.4f}, mean {worst[1]:.4f}, M2 {worst[2]:.4f}')


def test_mcd_exact_claims_on_the_device():
    from kwiiyatta_amd.backend import distortion as dist
    rng = np.random.RandomState(3)
    a, _ = ec.matrices(rng, 777, 1, 25)
    m, status, rows = dist.mcd(a, a.copy(), per_row=True)
    assert status == 0 and not rows.any() and m.tolist() == [777.0, 0.0, 0.0]
    ia, _ = ec.index_lists(rng, 500, 777, 777)
    m, status = dist.mcd(a, a.copy(), idx_a=ia, idx_b=ia)
    assert status == 0 and m.tolist() == [500.0, 0.0, 0.0]
    # a constant offset on k coefficients: (10 / ln 10) sqrt(2 k) |delta|
    for k, delta in ((24, 0.125), (7, -0.3)):
        b = a.copy()
        b[:, 1:1 + k] += delta
        m, _, rows = dist.mcd(a, b, per_row=True)
        d = (a - b)[:, 1:1 + k]                      # (what the shift became in floating point)
        want = ec.DB * np.sqrt(2.0 * (d * d).sum(axis=1))
        assert np.all(np.abs(rows - want) <= ec.row_bound(want, 24))
        # (the shifted coefficients are rounded at their own scale, below 16: a few 1e-15 of the figure)
        assert abs(m[1] - ec.DB * np.sqrt(2 * k) * abs(delta)) <= 1e-12
    # c0 is left out by default and taken with first_col=0
    b = a.copy()
    b[:, 0] += 1.0
    assert dist.mcd(a, b)[0].tolist() == [777.0, 0.0, 0.0]
    assert abs(dist.mcd(a, b, first_col=0)[0][1] - ec.DB * np.sqrt(2.0)) <= 1e-12


def test_mcd_batch_device_forms_and_reproducibility():
    import torch
    from kwiiyatta_amd.backend import distortion as dist
    cases = list(_mcd_cases(11, 25, lengths=(0, 1, 9, 65, 257, 1000, 4097))) + list(_mcd_cases(12, 25, lengths=(5, 511)))
    assert len(cases) > 32                                    # more than two launch groups
    keys = ('idx_a', 'idx_b', 'off_a', 'off_b', 'mask')

    def call(sub):
        kw = {k: [c.get(k, 0 if k.startswith('off') else None) for c in sub] for k in keys}
        return dist.mcd([c['a'] for c in sub], [c['b'] for c in sub], per_row=True, **kw)
    m, status, rows = call(cases)
    m2, status2, rows2 = call(cases)
    assert m.tobytes() == m2.tobytes() and status.tobytes() == status2.tobytes()
    assert all(r.tobytes() == s.tobytes() for r, s in zip(rows, rows2))
    for i, c in enumerate(cases):                             # a batch equals its utterances one by one
        m1, s1, r1 = dist.mcd(per_row=True, **c)
        assert m1.tobytes() == m[i].tobytes() and s1 == status[i] and r1.tobytes() == rows[i].tobytes(), i
    # the device form: index lists and masks in HBM, the row count as a device word behind lists with room to spare
    dev, stream, ctx = _device()
    up = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    jobs, outs, held = [], [], []
    for c in cases:
        n = len(ec.mcd_rows(c['a'], c['b'], c.get('idx_a'), c.get('idx_b'), c.get('off_a', 0), c.get('off_b', 0))[0])
        a, b, mask = up(c['a']), up(c['b']), up(c.get('mask'))
        ia, ib, n_dev, cap = None, None, None, n
        if c.get('idx_a') is not None:
            cap = n + 13
            pad = np.full(13, 2 ** 30, dtype=np.int32)          # beyond the count: never read
            ia, ib = up(np.concatenate((c['idx_a'], pad))), up(np.concatenate((c['idx_b'], pad)))
            n_dev = torch.tensor([n], dtype=torch.int64, device=dev)
        out = torch.full((cap,), 7.0, dtype=torch.float64, device=dev)
        jobs.append(dist.mcd_job(a, b, ia, ib, c.get('off_a', 0), c.get('off_b', 0), rows=cap, n_dev=n_dev, mask=mask,
                                 per_row=out))
        outs.append((out, n))
        held.append((a, b, mask, ia, ib, n_dev))
    d_m = torch.empty((len(cases), 3), dtype=torch.float64, device=dev)
    d_s = torch.full((len(cases),), -1, dtype=torch.int32, device=dev)
    for lo in range(0, len(cases), 5):
        dist.mcd_batch_dev(ctx, jobs[lo:lo + 5], 25, d_m[lo:lo + 5], d_s[lo:lo + 5])
    stream.synchronize()
    assert d_m.cpu().numpy().tobytes() == m.tobytes()
    assert d_s.cpu().numpy().tobytes() == status.tobytes()
    for (out, n), r in zip(outs, rows):
        got = out.cpu().numpy()
        assert got[:n].tobytes() == r.tobytes() and np.all(got[n:] == 7.0)
    # a matrix that is a strided view of a wider block (the padded mel-cepstra of a wave are such rows)
    wide = torch.from_numpy(np.random.RandomState(5).standard_normal((300, 40))).to(dev)
    a_view, b_rows = wide[:, 3:28], wide[10:310:1, 3:28]
    a_host = np.ascontiguousarray(a_view.cpu().numpy())
    b_host = np.ascontiguousarray(b_rows.cpu().numpy())
    n = len(b_host)
    d_one = torch.empty((1, 3), dtype=torch.float64, device=dev)
    dist.mcd_batch_dev(ctx, [dist.mcd_job(a_view[:n], b_rows)], 25, d_one)
    stream.synchronize()
    assert d_one.cpu().numpy()[0].tobytes() == dist.mcd(a_host[:n], b_host)[0].tobytes()


def test_mcd_status_and_argument_errors():
    from kwiiyatta_amd.backend import distortion as dist
    rng = np.random.RandomState(21)
    a, b = ec.matrices(rng, 300, 300, 25)
    bad = a.copy()
    bad[17, 3], bad[40, 24], bad[41, 0] = np.nan, np.inf, np.nan          # (c0 is not measured: row 41 counts)
    other = b.copy()
    other[99, 1] = -np.inf
    m, status, rows = dist.mcd(bad, other, per_row=True, strict=False)
    want, want_status = ec.mcd_rows(bad, other)
    assert status == want_status == 3 and m[0] == 297
    assert np.array_equal(np.isnan(rows), np.isnan(want)) and np.isnan(rows[[17, 40, 99]]).all()
    assert dist.mcd(bad, other, first_col=0, strict=False)[1] == 4
    with pytest.raises(ValueError, match=r'3 row\(s\) of utterance\(s\) \[1\]'):
        dist.mcd([a, bad], [b, other])
    # a masked-out row is not examined; a row whose index lies outside its matrix is passed over
    mask = np.full(300, 9.4)
    mask[[17, 40, 99]] = 0.0
    assert dist.mcd(bad, other, mask=mask)[1] == 0
    ia = np.arange(300, dtype=np.int32)
    ia[5], ia[6] = 300, -1
    m, status, rows = dist.mcd(a, b, idx_a=ia, idx_b=np.arange(300, dtype=np.int32), per_row=True, strict=False)
    assert status == 0 and m[0] == 298 and np.isnan(rows[[5, 6]]).all()
    # no rows, and no rows that count: zeros
    assert dist.mcd(a[:0], b[:0])[0].tolist() == [0.0, 0.0, 0.0]
    assert dist.mcd(a, b, mask=np.zeros(300))[0].tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match='C-contiguous'):
        dist.mcd(a[:, ::2], b[:, ::2])
    with pytest.raises(ValueError, match='dtype mismatch'):
        dist.mcd(a.astype(np.float32), b)
    with pytest.raises(ValueError, match='columns'):
        dist.mcd(np.zeros((10, 65)), np.zeros((10, 65)))
    with pytest.raises(ValueError, match='same number of rows'):
        dist.mcd(a, b[:200])
    with pytest.raises(ValueError, match='int32'):
        dist.mcd(a, b, idx_a=np.arange(300), idx_b=np.arange(300))
    with pytest.raises(ValueError, match='first_col'):
        dist.mcd(a, b, first_col=26)


# ---- f0 and voicing ----------------------------------------------------------------------------------------------------
def _f0_cases(seed, lengths=ec.LENGTHS):
    rng = np.random.RandomState(seed)
    for n in lengths:
        fa, fb = ec.f0_tracks(rng, n, n)
        yield dict(f0_a=fa, f0_b=fb)
        rows_a, rows_b = max(1, n // 2 + 3), max(1, n // 3 + 5)
        fa, fb = ec.f0_tracks(rng, rows_a, rows_b)
        ia, ib = ec.index_lists(rng, n, rows_a, rows_b, 100, 7)
        yield dict(f0_a=fa, f0_b=fb, idx_a=ia, idx_b=ib, off_a=100, off_b=7)


def _f0_want(c):
    return ec.f0_error(c['f0_a'], c['f0_b'], c.get('idx_a'), c.get('idx_b'), c.get('off_a', 0), c.get('off_b', 0))


def test_f0_error_against_numpy_batched_and_reproducible():
    import torch
    from kwiiyatta_amd.backend import distortion as dist
    cases = list(_f0_cases(31))
    keys = ('idx_a', 'idx_b', 'off_a', 'off_b')
    kw = {k: [c.get(k, 0 if k.startswith('off') else None) for c in cases] for k in keys}
    counts, m, status = dist.f0_error([c['f0_a'] for c in cases], [c['f0_b'] for c in cases], **kw)
    again = dist.f0_error([c['f0_a'] for c in cases], [c['f0_b'] for c in cases], **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((counts, m, status), again))
    worst = np.zeros(2)
    for i, c in enumerate(cases):
        w_counts, w_m, w_status, vals = _f0_want(c)
        assert counts[i].tolist() == w_counts.tolist() and status[i] == w_status == 0, i
        assert m[i, 0] == w_m[0] == w_counts[0]
        mean_b, m2_b = ec.moments_bounds(vals, ec.cents_bound(vals))
        assert abs(m[i, 1] - w_m[1]) <= mean_b and abs(m[i, 2] - w_m[2]) <= m2_b, i
        if len(vals):
            worst = np.maximum(worst, (abs(m[i, 1] - w_m[1]) / mean_b, abs(m[i, 2] - w_m[2]) / m2_b))
            assert abs(dist.rmse(m[i]) - ec.rmse(w_m)) <= 1e-9
        one = dist.f0_error(**c)
        assert one[0].tobytes() == counts[i].tobytes() and one[1].tobytes() == m[i].tobytes() and one[2] == status[i], i
    print(f'f0 error: worst error / bound: mean {worst[0]:.4f}, M2 {worst[1]:.4f}')
    # the device form, the row count as a device word
    dev, stream, ctx = _device()
    up = lambda v: None if v is None else torch.from_numpy(v).to(dev)  # noqa: E731
    jobs, held = [], []
    for c in cases:
        n = len(c['idx_a']) if 'idx_a' in c else len(c['f0_a'])
        fa, fb, ia, ib, n_dev, cap = up(c['f0_a']), up(c['f0_b']), None, None, None, n
        if 'idx_a' in c:
            cap = n + 5
            pad = np.full(5, -2 ** 30, dtype=np.int32)
            ia, ib = up(np.concatenate((c['idx_a'], pad))), up(np.concatenate((c['idx_b'], pad)))
            n_dev = torch.tensor([n], dtype=torch.int64, device=dev)
        jobs.append(dist.f0_error_job(fa, fb, ia, ib, c.get('off_a', 0), c.get('off_b', 0), rows=cap, n_dev=n_dev))
        held.append((fa, fb, ia, ib, n_dev))
    d_c = torch.full((len(cases), 4), -1, dtype=torch.int64, device=dev)
    d_m = torch.empty((len(cases), 3), dtype=torch.float64, device=dev)
    d_s = torch.full((len(cases),), -1, dtype=torch.int32, device=dev)
    for lo in range(0, len(cases), 7):
        dist.f0_error_batch_dev(ctx, jobs[lo:lo + 7], d_c[lo:lo + 7], d_m[lo:lo + 7], d_s[lo:lo + 7])
    stream.synchronize()
    assert d_c.cpu().numpy().tobytes() == counts.tobytes()
    assert d_m.cpu().numpy().tobytes() == m.tobytes()
    assert d_s.cpu().numpy().tobytes() == status.tobytes()


def test_f0_error_hand_made_tracks_and_status():
    from kwiiyatta_amd.backend import distortion as dist
    fa = np.array([0.0, 100.0, 200.0, 0.0, 400.0, 150.0])
    fb = np.array([0.0, 200.0, 100.0, 120.0, 0.0, 150.0])
    counts, m, status = dist.f0_error(fa, fb)
    assert counts.tolist() == [3, 1, 1, 1] and status == 0
    assert m.tolist() == [3.0, 0.0, 2 * 1200.0 ** 2]              # -1200, +1200 and 0 cents
    assert dist.rmse(m) == np.sqrt(2 * 1200.0 ** 2 / 3) and dist.vuv_error(counts) == 2 / 6
    same = dist.f0_error(fa, fa.copy())
    assert same[0].tolist() == [4, 0, 0, 2] and same[1].tolist() == [4.0, 0.0, 0.0]
    assert np.isnan(dist.rmse(dist.f0_error(np.zeros(9), np.zeros(9))[1]))
    odd = fa.copy()
    odd[1], odd[2] = np.nan, -5.0
    counts, m, status = dist.f0_error(odd, fb, strict=False)
    assert status == 2 and counts.tolist() == [1, 1, 1, 1] and m.tolist() == [1.0, 0.0, 0.0]
    assert counts.tolist() == ec.f0_error(odd, fb)[0].tolist()
    with pytest.raises(ValueError, match=r'2 row\(s\) of utterance\(s\) \[0\]'):
        dist.f0_error(odd, fb)
    with pytest.raises(ValueError, match='dtype mismatch'):
        dist.f0_error(fa.astype(np.float32), fb)


EV_GROUP = 16                # utterances per launch (kwy_eval.hip)


def test_one_job_more_than_a_launch_holds():
    """kwy_mcd_batch_dev and kwy_f0_error_batch_dev on EV_GROUP + 1 tiny jobs of unequal size in ONE call each, the
    job that falls into the second launch without rows: every job equals the same job through the single call,
    bit for bit, and the words of the last job are written"""
    import torch
    from kwiiyatta_amd.backend import distortion as dist
    rng = np.random.RandomState(41)
    rows = [1 + i % 5 for i in range(EV_GROUP)] + [0]
    dev, stream, ctx = _device()
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    pairs = [ec.matrices(rng, n, n, 25) for n in rows]
    tracks = [ec.f0_tracks(rng, n, n) for n in rows]
    held = [[up(v) for v in p] for p in pairs + tracks]
    outs = [torch.full((n,), 7.0, dtype=torch.float64, device=dev) for n in rows]
    count = len(rows)
    d_m = torch.full((count, 3), -1.0, dtype=torch.float64, device=dev)
    d_s = torch.full((count,), -1, dtype=torch.int32, device=dev)
    dist.mcd_batch_dev(ctx, [dist.mcd_job(a, b, per_row=o) for (a, b), o in zip(held[:count], outs)], 25, d_m, d_s)
    f_c = torch.full((count, 4), -1, dtype=torch.int64, device=dev)
    f_m = torch.full((count, 3), -1.0, dtype=torch.float64, device=dev)
    f_s = torch.full((count,), -1, dtype=torch.int32, device=dev)
    dist.f0_error_batch_dev(ctx, [dist.f0_error_job(fa, fb) for fa, fb in held[count:]], f_c, f_m, f_s)
    stream.synchronize()
    for i, ((a, b), (fa, fb)) in enumerate(zip(pairs, tracks)):
        m1, s1, r1 = dist.mcd(a, b, per_row=True)
        assert d_m[i].cpu().numpy().tobytes() == m1.tobytes() and int(d_s[i]) == s1, i
        assert outs[i].cpu().numpy().tobytes() == r1.tobytes(), i
        c1, fm1, fs1 = dist.f0_error(fa, fb)
        assert f_c[i].cpu().numpy().tobytes() == c1.tobytes() and f_m[i].cpu().numpy().tobytes() == fm1.tobytes(), i
        assert int(f_s[i]) == fs1, i
    assert d_m[-1].tolist() == [0.0, 0.0, 0.0] and f_c[-1].tolist() == [0, 0, 0, 0]


# ---- merging -----------------------------------------------------------------------------------------------------------
def test_merge_equals_the_fold_and_the_concatenation():
    import torch
    from kwiiyatta_amd.backend import distortion as dist
    rng = np.random.RandomState(41)
    parts = [rng.standard_normal(n) * 2 + 6 for n in (0, 5, 1, 0, 300, 64, 2049, 0)]
    triples = np.array([ec.moments(p) for p in parts])
    got = dist.merge_moments(triples)
    assert got.tobytes() == ec.merge(triples).tobytes()                  # the same fold of the same triples
    whole = ec.moments(np.concatenate(parts))
    mean_b, m2_b = ec.merge_bound(parts)
    assert got[0] == whole[0] and abs(got[1] - whole[1]) <= mean_b and abs(got[2] - whole[2]) <= m2_b
    assert dist.merge_moments(np.zeros((4, 3))).tolist() == [0.0, 0.0, 0.0]
    # several columns of triples at once, bit-equal to the columns one by one and however the rows were grouped
    wide = np.ascontiguousarray(np.stack([triples, triples[::-1], np.roll(triples, 3, axis=0)], axis=1))
    m = dist.merge_moments(wide)
    assert m.shape == (3, 3)
    for c in range(3):
        assert m[c].tobytes() == ec.merge(wide[:, c]).tobytes(), c
    head = dist.merge_moments(np.ascontiguousarray(wide[:5]))
    assert dist.merge_moments(np.ascontiguousarray(np.concatenate((head[None], wide[5:])))).tobytes() == m.tobytes()
    dev, stream, ctx = _device()
    d_out = torch.empty((3, 3), dtype=torch.float64, device=dev)
    dist.merge_moments_dev(ctx, torch.from_numpy(wide).to(dev), d_out)
    stream.synchronize()
    assert d_out.cpu().numpy().tobytes() == m.tobytes()
    with pytest.raises(ValueError, match='non-empty'):
        dist.merge_moments(np.zeros((0, 3)))


# ---- package path, driver, command line --------------------------------------------------------------------------------
TRAINED, HELD_OUT = 4, 3            # files of the sorted keys the converter is trained on / evaluated on

# |driver - package| of a held-out pair's mean distortions, measured on the MI355X against the package path and taken
# times ten (both sides run the same kernels on the same alignment; they differ in how the mel-cepstra reach them --
# sp2mc over the padded block of a wave against the analyser's own -- and in the batching of the MLPG partitions).
# Measured: 0 on every figure of every pair and option set (test_driver_equals_the_package_path's docstring), so ten
# times that asks for equal bits.
DRIVER_MCD_BOUND = 10 * 0.0
DRIVER_SOURCE_BOUND = 10 * 0.0


def _run_cli(main, argv):
    import sys
    old = sys.argv
    sys.argv = ['prog'] + argv
    try:
        main()
    finally:
        sys.argv = old


def _dataset():
    import pathlib
    import kwiiyatta_amd as k
    from conftest import CLB_DIR, SLT_DIR
    return k.align(k.WavFileDataset(pathlib.Path(CLB_DIR)), k.WavFileDataset(pathlib.Path(SLT_DIR)))


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """a small converter (2 components, seed 0, with f0 and global-variance statistics) trained through the package
    API on the first 4 CLB -> SLT files, its model file, the dataset and the held-out keys"""
    import kwiiyatta_amd as k
    dataset = _dataset()
    keys = sorted(dataset.keys())
    conv = k.MelCepstrumConverter(use_delta=True, components=2, random_state=0)
    np.random.seed(0)
    conv.train(dataset, keys[:TRAINED], f0_stats=True, gv_stats=True)
    model = tmp_path_factory.mktemp('eval') / 'model.npz'
    conv.save(model)
    return conv, model, dataset, keys[TRAINED:TRAINED + HELD_OUT]


def _pairs(keys):
    import pathlib
    import kwiiyatta_amd as k
    from conftest import CLB_DIR, SLT_DIR
    from kwiiyatta_amd.evaluate_voice import _triple
    return [tuple(_triple(k.analyze_wav(pathlib.Path(d) / key)) for d in (CLB_DIR, SLT_DIR)) for key in keys]


def _same_figures(r, s):
    return (r.mcd_moments, r.source_moments, r.f0_moments, r.counts, r.aligned, r.outside) == \
        (s.mcd_moments, s.source_moments, s.f0_moments, s.counts, s.aligned, s.outside)


@pytest.mark.parametrize('opts', [dict(), dict(frames='all'), dict(gv=1.0, convert_f0=True, transpose_key=1.0)],
                         ids=['plain', 'all', 'gv-f0'])
def test_driver_equals_the_package_path(trained, opts):
    """corpus.evaluate_batch against evaluate over evaluate_pair on the held-out pairs, under one seed: the alignments
    are equal as integer lists, hence the frame counts, the voicing counts and the f0 triples (the same tracks through
    the same kernel) are equal; the distortions agree within ten times the difference measured on the MI355X.
    Measured (arctic_a0005 .. a0007, 2 components, seed 0; MCD converted / unconverted source in dB, frames of aligned):
    speech frames 5.0400 / 7.7514 (137 of 235), 5.2502 / 8.1328 (328 of 508), 5.9557 / 7.7624 (322 of 444); all frames
    5.0733 / 7.2147, 5.6310 / 8.1098 (472 of 508: 36 aligned cells lie in a trailing pad), 5.7557 / 7.4383; with --gv 1
    5.7479, 6.0328, 6.7405.  |driver - package| = 0 for every triple, count and index list: the two paths hand the
    kernels the same bits."""
    from kwiiyatta_amd import corpus, evaluate_voice as ev
    conv, _, dataset, held = trained
    np.random.seed(1)
    results, total = ev.evaluate(conv, dataset, held, per_frame=True, **opts)
    kw = dict(frames=opts.get('frames', 'speech'), transpose_key=opts.get('transpose_key', 0.0),
              f0_stats=conv.f0_stats if opts.get('convert_f0') else None)
    if opts.get('gv'):
        kw.update(gv_stats=conv.gv_stats, gv_strength=opts['gv'])
    np.random.seed(1)
    records, pooled = corpus.evaluate_batch(_pairs(held), conv.fs, conv.gmm, order=conv.order, per_frame=True,
                                            wave_pairs=2, converter_fs=conv.fs, **kw)
    assert len(records) == len(results) == HELD_OUT
    worst = np.zeros(2)
    for key, r, d in zip(list(held) + ['total'], results + [total], records + [pooled]):
        if 'idx_x' in d:
            assert d['idx_x'].dtype.kind == 'i' and d['idx_x'].tolist() == r.idx_x.tolist(), key
            assert d['idx_y'].tolist() == r.idx_y.tolist(), key
            assert np.array_equal(np.isnan(d['mcd_frames']), np.isnan(r.mcd_frames)), key
        assert d['aligned'] == r.aligned and d['outside'] == r.outside and tuple(d['counts']) == r.counts, key
        assert d['mcd_moments'][0] == r.frames and d['source_moments'][0] == r.frames, key
        assert tuple(d['f0_moments']) == r.f0_moments or opts.get('convert_f0'), key
        diff = abs(d['mcd_moments'][1] - r.mcd), abs(d['source_moments'][1] - r.mcd_source)
        print(f'{key}: frames {r.frames} of {r.aligned} aligned ({r.outside} outside) MCD {r.mcd:.4f} dB, source '
              f'{r.mcd_source:.4f} dB, f0 RMSE {r.f0_rmse_cents:.2f} cents, V/UV {100 * r.vuv_error:.2f} %; driver - package: '
              f'MCD {diff[0]:.3e} source {diff[1]:.3e} f0 mean {abs(d["f0_moments"][1] - r.f0_moments[1]):.3e}')
        worst = np.maximum(worst, diff)
    print(f'worst driver - package difference: MCD {worst[0]:.3e} dB, source {worst[1]:.3e} dB')
    assert worst[0] <= DRIVER_MCD_BOUND and worst[1] <= DRIVER_SOURCE_BOUND
    if opts.get('convert_f0'):
        # (the mapped f0 comes from the same map kernel in both paths)
        for r, d in zip(results, records):
            assert tuple(d['f0_moments']) == r.f0_moments


class _Identity:
    """a converter that hands the mel-cepstrum back: what evaluate_pair asks of a converter, and nothing else"""
    f0_stats = None

    def convert(self, mel_cepstrum, **kwargs):
        import copy
        return copy.copy(mel_cepstrum)


def test_a_pair_against_itself(trained):
    import pathlib
    import kwiiyatta_amd as k
    from conftest import CLB_DIR
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd.converter.dataset import trim_zeros_frames
    conv, _, _, held = trained
    f = k.feature(k.analyze_wav(pathlib.Path(CLB_DIR) / held[0]))
    f = f[:len(trim_zeros_frames(f.spectrum_envelope))]
    np.random.seed(2)
    r = k.evaluate_pair(_Identity(), f, f, per_frame=True)
    assert r.idx_x.tolist() == r.idx_y.tolist() and r.aligned > 0 and r.frames > 0
    assert r.mcd_moments == (float(r.frames), 0.0, 0.0) == r.source_moments
    assert r.f0_rmse_cents == 0.0 and r.vuv_error == 0.0 and r.vu == r.uv == 0 and r.vv > 0
    r = k.evaluate_pair(conv, f, f)                       # a trained converter moves the voice away from its source
    assert r.source_moments == (float(r.frames), 0.0, 0.0) and r.mcd > 0.0
    pair = _pairs(held[:1])[0]
    np.random.seed(2)
    records, total = corpus.evaluate_batch([(pair[0], pair[0])], conv.fs, conv.gmm, order=conv.order)
    assert records[0]['source_moments'] == (float(r.frames), 0.0, 0.0) == total['source_moments']
    assert records[0]['f0_moments'][1:] == (0.0, 0.0) and records[0]['counts'][1:3] == (0, 0)


def test_model_gv_and_frame_selection(trained):
    import copy
    import kwiiyatta_amd as k
    from kwiiyatta_amd import evaluate_voice as ev
    conv, model, dataset, held = trained
    pair = ev._trimmed(dataset)[held[0]]

    def run(converter=conv, **kw):
        np.random.seed(3)
        return k.evaluate_pair(converter, *pair, **kw)
    base = run()
    assert _same_figures(run(), base)                                     # one seed, one result
    assert _same_figures(run(gv=0.0), base)                               # --gv 0 is no --gv
    # the unconverted source's distortion does not depend on the model
    other = k.MelCepstrumConverter(use_delta=True, components=2).load(model)
    other.gmm.means_ = other.gmm.means_ + 0.05
    moved = run(other)
    assert moved.source_moments == base.source_moments and moved.mcd_moments != base.mcd_moments
    assert moved.counts == base.counts and moved.f0_moments == base.f0_moments
    # the postfilter moves the converted voice only
    full = run(gv=1.0)
    assert full.source_moments == base.source_moments and full.mcd_moments != base.mcd_moments
    assert full.frames == base.frames
    print(f'{held[0]}: MCD {base.mcd:.4f} dB, with --gv {full.mcd:.4f} dB, unconverted source {base.mcd_source:.4f} dB')
    # frames='all': every aligned frame.  The cut of align_even ends where BOTH sides are in their trailing pads, so an
    # alignment may keep cells with ONE side in its pad (36 of arctic_a0006's 508); such a cell has no converted frame
    # and is passed over and reported: frames + outside is the length of the alignment, for every pair
    for key in held:
        np.random.seed(3)
        every = k.evaluate_pair(conv, *ev._trimmed(dataset)[key], frames='all', per_frame=True)
        rows = [len(f.f0) for f in ev._trimmed(dataset)[key]]
        beyond = int(((every.idx_x < 0) | (every.idx_x >= rows[0]) | (every.idx_y < 0) | (every.idx_y >= rows[1])).sum())
        print(f'{key}: {every.aligned} aligned frames, {beyond} of them beyond either utterance, {every.frames} measured')
        assert every.aligned == len(every.idx_x) == len(every.idx_y) and every.outside == beyond
        assert every.frames + beyond == every.aligned and np.isnan(every.mcd_frames).sum() == beyond
        if key == held[0]:
            assert every.aligned == base.aligned and every.frames > base.frames
    # the f0 map changes the f0 figures only
    keyed = run(transpose_key=12.0)
    assert keyed.mcd_moments == base.mcd_moments and keyed.counts == base.counts
    assert abs(keyed.f0_moments[1] - (base.f0_moments[1] + 1200.0)) <= 1e-9
    mapped = run(convert_f0=True)
    assert mapped.counts == base.counts and mapped.f0_moments != base.f0_moments
    print(f'{held[0]}: f0 RMSE {base.f0_rmse_cents:.1f} cents, with --convert-f0 {mapped.f0_rmse_cents:.1f} cents')
    bare = copy.copy(conv)
    bare.f0_stats = None
    with pytest.raises(ValueError, match='no statistics'):
        k.evaluate_pair(bare, *pair, convert_f0=True)


def test_a_pair_across_sampling_rates(trained):
    import pathlib
    import kwiiyatta_amd as k
    from conftest import SLT_DIR, clb_variant
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd.converter.dataset import trim_zeros_frames
    from kwiiyatta_amd.evaluate_voice import _triple
    conv, _, _, _ = trained
    analysed = [k.analyze_wav(pathlib.Path(p)) for p in (clb_variant('22'), pathlib.Path(SLT_DIR) / 'arctic_a0001.wav')]
    assert analysed[0].fs == 22050 and conv.fs == analysed[1].fs == 16000
    with pytest.raises(ValueError, match='22050 Hz, the converter at 16000 Hz'):
        corpus.evaluate_batch([tuple(_triple(a) for a in analysed)], analysed[0].fs, conv.gmm, converter_fs=conv.fs)
    pair = []
    for a in analysed:
        f = k.feature(a)
        pair.append(f[:len(trim_zeros_frames(f.spectrum_envelope))])
    np.random.seed(4)
    r = k.evaluate_pair(conv, *pair)
    print('22.05 kHz source: ' + r.line('arctic_a0001.wav'))
    assert r.frames > 100 and 0 < r.mcd < 30 and 0 < r.mcd_source < 30 and r.vv > 0


def test_evaluate_voice_command(trained, tmp_path, capsys, monkeypatch):
    import json
    import kwiiyatta_amd as k
    from conftest import CLB_DIR, SLT_DIR
    from kwiiyatta_amd import evaluate_voice as ev
    conv, model, dataset, held = trained
    # from a saved model: nothing is trained, the held-out slice is evaluated, the file holds the figures printed
    monkeypatch.setattr(k.Config, '_train', lambda *a, **kw: pytest.fail('a saved model must not be retrained'))
    common = ['--source', CLB_DIR, '--target', SLT_DIR, '--converter-components', '2', '--converter-model', str(model),
              '--eval-skip-files', str(TRAINED), '--eval-max-files', str(HELD_OUT)]
    np.random.seed(5)
    _run_cli(ev.main, common + ['--json', str(tmp_path / 'out' / 'plain.json')])
    out, err = capsys.readouterr()
    assert 'warning' not in err
    lines = out.strip().splitlines()
    doc = json.loads((tmp_path / 'out' / 'plain.json').read_text())
    assert len(lines) == HELD_OUT + 1 and [f['name'] for f in doc['files']] == [str(key) for key in held]
    assert doc['options'] == dict(gv=0.0, convert_f0=False, transpose_key=0.0, frames='speech')
    np.random.seed(5)
    results, total = k.evaluate(conv, dataset, held)
    for line, record, r, name in zip(lines, doc['files'] + [doc['total']], results + [total],
                                     [str(key) for key in held] + [f'total ({HELD_OUT} of {HELD_OUT} files)']):
        assert line == r.line(name)
        assert {k_: v for k_, v in record.items() if k_ not in ('name', 'files')} == r.as_dict()
    assert doc['total']['files'] == HELD_OUT and doc['total']['frames'] == sum(f['frames'] for f in doc['files'])
    # --gv 0 is no --gv; --gv, --convert-f0 and --frames reach the figures; --batch goes through the driver
    np.random.seed(5)
    _run_cli(ev.main, common + ['--gv', '0'])
    assert capsys.readouterr().out.strip().splitlines() == lines
    np.random.seed(5)
    _run_cli(ev.main, common + ['--gv', '--convert-f0', '--frames', 'all', '--json', str(tmp_path / 'full.json')])
    full = json.loads((tmp_path / 'full.json').read_text())
    shown = lines + capsys.readouterr().out.strip().splitlines()
    assert full['options'] == dict(gv=1.0, convert_f0=True, transpose_key=0.0, frames='all')
    assert full['total']['frames'] > doc['total']['frames'] and full['total']['mcd'] != doc['total']['mcd']
    assert full['total']['f0_rmse_cents'] != doc['total']['f0_rmse_cents']
    np.random.seed(5)
    _run_cli(ev.main, common + ['--batch', '--json', str(tmp_path / 'batch.json')])
    capsys.readouterr()
    batch = json.loads((tmp_path / 'batch.json').read_text())
    for a, b in zip(batch['files'] + [batch['total']], doc['files'] + [doc['total']]):
        assert (a['frames'], a['aligned'], a['counts'], a['f0_rmse_cents']) == \
            (b['frames'], b['aligned'], b['counts'], b['f0_rmse_cents'])
        assert abs(a['mcd'] - b['mcd']) <= DRIVER_MCD_BOUND and abs(a['mcd_source'] - b['mcd_source']) <= DRIVER_SOURCE_BOUND
    # no file with a selected frame: a parser error
    none = ev.Result((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0, 0, 0, 0), 0)
    monkeypatch.setattr(ev, 'evaluate', lambda *a, **kw: ([none], none))
    with pytest.raises(SystemExit):
        _run_cli(ev.main, common)
    out, err = capsys.readouterr()
    assert 'MCD nan dB' in out and 'has a selected frame' in err
    with pytest.raises(SystemExit):
        _run_cli(ev.main, common[:-4] + ['--eval-skip-files', '9'])
    assert 'no files to evaluate' in capsys.readouterr().err
    print('\n'.join(shown))


def test_evaluate_voice_trains_and_warns_of_an_overlap(tmp_path, capsys):
    from conftest import CLB_DIR, SLT_DIR
    from kwiiyatta_amd import evaluate_voice as ev
    np.random.seed(6)
    _run_cli(ev.main, ['--source', CLB_DIR, '--target', SLT_DIR, '--converter-components', '2', '--converter-seed', '0',
                       '--max-files', '2', '--eval-skip-files', '1', '--eval-max-files', '2'])
    out, err = capsys.readouterr()
    assert err.count('warning: 1 evaluated file(s) were also trained on') == 1 and 'arctic_a0002.wav' in err
    lines = [line for line in out.strip().splitlines() if not line.startswith('Initialization')]       # (the fit's own)
    assert 'arctic_a0003.wav' not in err and len(lines) == 3 and lines[1].startswith('arctic_a0003.wav: frames ')
    print(out)
