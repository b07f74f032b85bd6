"""The GV ascent on the device (k_gv_ascent behind kwy_gv_ascent_batch_dev / kwy_gv_ascent) against the numpy
restatement of tests/gvgen_cases.py, on every case of its table: the kernel is handed exactly the records, offset and
y_ML the restatement gets.

Bound: 1e-9 of the largest reference value for every y_N, 1e-9 of the sum of the magnitudes of Q_k's three terms for
every Q_k (Q itself can pass through zero), and Q_k never decreasing as returned.  tests/test_gvgen_cases.py shows on
the CPU that a relative perturbation of 1e-13 of the records and of y_ML moves no y_k of the table by more than 3e-10 of
its peak, so f64 rounding (1e-16) has three orders of magnitude of room.
"""
import ctypes

import numpy as np
import pytest

import gvgen_cases as gc

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope='module')
def ctx():
    from kwiiyatta_amd import _lib
    return _lib.Context(0)


def _close(got, ref, what):
    err, peak = np.abs(got - ref).max(), np.abs(ref).max()
    print(f'{what}: max |got - numpy| = {err:.3e}, largest reference value {peak:.3e}')
    assert np.isfinite(got).all() and err <= TOL * peak, what


def _close_objective(got, ref, mags, what):
    assert len(got) == len(ref)
    for k, (a, b, m) in enumerate(zip(got, ref, mags)):
        print(f'{what}: Q_{k} = {a!r}, numpy {b!r}, term magnitudes {m:.3e}')
        assert abs(a - b) <= TOL * m, (what, k)
    assert all(got[k + 1] >= got[k] for k in range(len(got) - 1)), (what, list(got))


@pytest.mark.parametrize('case', gc.CASES, ids=gc.case_id)
def test_device_ascent_equals_the_restatement(ctx, case):
    d, T, off, up, Ns = case
    rec, y, s, mean, var = gc.inputs(d, T, off, up)
    ys, Qs, mags, status = gc.case_reference(case)
    for N in Ns:
        (got,), (obj,), (st,) = gc.ascent_dev(ctx, [(rec, s, y)], mean, var, N)
        what = f'{gc.case_id(case)}, iterations = {N}'
        assert st == status == 0
        _close(got, ys[N], what)
        _close_objective(obj, Qs[:N + 1], mags[:N + 1], what)
        if N == max(Ns):
            (bare,), _, _ = gc.ascent_dev(ctx, [(rec, s, y)], mean, var, N, objective=False)
            assert np.array_equal(bare, got), 'the trajectory does not depend on the objective being asked for'
    if T == 1:
        assert np.array_equal(got, y), 'a single frame has no variance: unchanged'


def test_host_entry(ctx):
    d, T, off, up, N = 2, 257, True, True, 8
    rec, y, s, mean, var = gc.inputs(d, T, off, up)
    ys, Qs, mags, _ = gc.ascent(rec, y, s, mean, var, N)
    got, obj, st = gc.ascent_host(ctx, rec, s, y, mean, var, N)
    assert st == 0
    _close(got, ys[N], 'kwy_gv_ascent')
    _close_objective(obj, Qs, mags, 'kwy_gv_ascent')
    (dev,), (dobj,), _ = gc.ascent_dev(ctx, [(rec, s, y)], mean, var, N)
    assert np.array_equal(dev, got) and np.array_equal(dobj, obj), 'host and device entries run the same kernel'


def test_weight_scales_the_gv_term(ctx):
    d, T, off, up, N = 2, 257, False, True, 2
    rec, y, s, mean, var = gc.inputs(d, T, off, up)
    for weight in (0.25, 4.0):
        ys, Qs, mags, _ = gc.ascent(rec, y, s, mean, var, N, weight=weight)
        (got,), (obj,), _ = gc.ascent_dev(ctx, [(rec, s, y)], mean, var, N, weight=weight)
        _close(got, ys[N], f'weight {weight}')
        _close_objective(obj, Qs, mags, f'weight {weight}')


def test_unusable_columns_are_kept_and_counted(ctx):
    d, T, N = 24, 33, 2
    rec, y, s, mean, var = gc.inputs(d, T, True, True)
    mean, var = mean.copy(), var.copy()
    var[3] = 0.0
    mean[7] = np.nan
    ys, Qs, mags, status = gc.ascent(rec, y, s, mean, var, N)
    assert status == 2
    (got,), (obj,), (st,) = gc.ascent_dev(ctx, [(rec, s, y)], mean, var, N)
    assert st == 2
    assert np.array_equal(got[:, 3], y[:, 3]) and np.array_equal(got[:, 7], y[:, 7])
    _close(got, ys[N], 'two unusable columns')
    _close_objective(obj, Qs, mags, 'two unusable columns')


def test_constant_track_is_returned_unchanged(ctx):
    d, T, N = 2, 33, 2
    rec, y, s, mean, var = gc.inputs(d, T, False, True)
    y = y.copy()
    y[:, 1] = 0.75
    ys, Qs, mags, status = gc.ascent(rec, y, None, mean, var, N)
    (got,), (obj,), (st,) = gc.ascent_dev(ctx, [(rec, None, y)], mean, var, N)
    assert st == status == 0
    assert np.array_equal(got[:, 1], y[:, 1])
    _close(got, ys[N], 'constant column')
    _close_objective(obj, Qs, mags, 'constant column')


@pytest.mark.parametrize('count', (3, 17))
def test_batch_equals_single_bit_for_bit(ctx, count):
    d, Ts, off, up, N = gc.BATCH
    Ts = [Ts[j % len(Ts)] for j in range(count)]
    assert count <= len(gc.BATCH[1]) or count > gc.KWY_BATCH_MAX
    mean = var = None
    jobs = []
    for T in Ts:
        rec, y, s, m, v = gc.inputs(d, T, off, up)
        mean, var = (m, v) if mean is None else (mean, var)        # one statistic for the call: the first job's
        jobs.append((rec, s, y))
    outs, objs, sts = gc.ascent_dev(ctx, jobs, mean, var, N)
    for j in list(range(len(gc.BATCH[1]))) + ([count - 1] if count > gc.KWY_BATCH_MAX else []):
        (y1,), (q1,), (s1,) = gc.ascent_dev(ctx, [jobs[j]], mean, var, N)
        assert np.isfinite(y1).all()
        assert np.array_equal(outs[j], y1), f'job {j} of {count}'
        assert np.array_equal(objs[j], q1), f'objective of job {j} of {count}'
        assert sts[j] == s1 == 0
    if count == 3:
        for j, (rec, s, y) in enumerate(jobs):
            ys, Qs, mags, _ = gc.ascent(rec, y, s, mean, var, N)
            _close(outs[j], ys[N], f'batch job {j}')
            _close_objective(objs[j], Qs, mags, f'batch job {j}')


def test_two_runs_give_the_same_bits(ctx):
    d, T, off, up = 24, 257, False, False
    rec, y, s, mean, var = gc.inputs(d, T, off, up)
    a = gc.ascent_dev(ctx, [(rec, s, y)], mean, var, 8)
    b = gc.ascent_dev(ctx, [(rec, s, y)], mean, var, 8)
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[1][0], b[1][0])


def test_empty_batch_is_ok(ctx):
    from kwiiyatta_amd import _lib
    jobs = _lib.job_array(_lib.GvAscentJob, [(None, None, None, 0, None)])
    assert _lib.lib.kwy_gv_ascent_batch_dev(ctx.handle, ctypes.cast(jobs, ctypes.c_void_p), 0, 2, None, None, 1.0, 2,
                                            None) == _lib.KWY_OK


@pytest.mark.parametrize('what, kwargs', (
    ('iterations below 0', dict(N=-1)),
    ('iterations above the maximum', dict(N=gc.KWY_MLPG_GV_MAX + 1)),
    ('weight 0', dict(weight=0.0)),
    ('weight negative', dict(weight=-1.0)),
    ('weight not finite', dict(weight=float('inf'))),
    ('weight NaN', dict(weight=float('nan'))),
))
def test_refusals_write_nothing(ctx, what, kwargs):
    from kwiiyatta_amd import _lib
    rec, y, s, mean, var = gc.inputs(2, 33, True, True)
    args = dict(N=2, weight=1.0)
    args.update(kwargs)
    rc, (got,), (obj,), (st,) = gc.ascent_dev(ctx, [(rec, s, y)], mean, var, args['N'], weight=args['weight'],
                                              check=False)
    assert rc == _lib.KWY_EINVAL, what
    assert np.array_equal(got, y) and np.isnan(obj).all() and st == -1, what


def test_statistics_from_moments(ctx):
    from kwiiyatta_amd.backend import gv
    rng = np.random.default_rng(5)
    mats = [rng.standard_normal((T, 5)) * (1.0 + j) for j, T in enumerate((40, 0, 33, 7))]
    moments = gv.column_moments([m for m in mats], ctx=ctx)
    mean, var = gv.gv_statistics(moments, ctx=ctx)
    assert np.array_equal(mean, gv.gv_from_moments(moments, ctx=ctx)), 'the mean is the postfilter statistic, bit for bit'
    per = np.stack([m.var(axis=0) for m in mats if len(m)])
    assert np.allclose(mean, per.mean(axis=0), rtol=1e-13, atol=0)
    assert np.allclose(var, per.var(axis=0), rtol=1e-12, atol=0)
    one_mean, one_var = gv.gv_statistics(moments[:2], ctx=ctx)
    assert np.array_equal(one_var, np.zeros(5)), 'fewer than two utterances with frames: variance 0'
    assert np.allclose(one_mean, mats[0].var(axis=0), rtol=1e-13, atol=0)
