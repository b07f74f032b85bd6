"""EM trajectory conversion over soft mixture posteriors on the device (k_em_estep and the entries around it) against
the numpy restatement of tests/em_cases.py, on every case of its table.

Bound: 1e-9 of the largest reference value for every y_k and 1e-9 |L_k| for every L_k -- what
tests/test_convert_kernels_gpu.py holds kwy_convert_mcep_dev to.  tests/test_em_cases.py shows on the CPU that a
relative perturbation of 1e-13 of the log-densities and conditional means moves no y_k of the table by more than 3e-10
of its peak, so f64 rounding (1e-16) has three orders of magnitude of room.
"""
import numpy as np
import pytest

import convert_cases as cc
import em_cases as ec

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope='module')
def ctx():
    from kwiiyatta_amd import _lib
    return _lib.Context(0)


def _prepared(ctx, d, w, mu, cov, diff=0):
    rc, model = cc.prepare(ctx, d, w, mu, cov, diff)
    assert rc == 0
    return model


def _close(got, ref, what):
    err, peak = np.abs(got - ref).max(), np.abs(ref).max()
    print(f'{what}: max |got - numpy| = {err:.3e}, largest reference value {peak:.3e}')
    assert np.isfinite(got).all() and err <= TOL * peak, what


def _close_lik(got, ref, what):
    for k, (a, b) in enumerate(zip(got, ref)):
        print(f'{what}: L_{k} = {a!r}, numpy {b!r}, relative difference {abs(a - b) / abs(b):.3e}')
        assert abs(a - b) <= TOL * abs(b), (what, k)


def _non_decreasing(lik, what):
    for k in range(len(lik) - 1):
        assert lik[k + 1] >= lik[k] - TOL * abs(lik[k]), (what, k, lik)


@pytest.mark.parametrize('case', ec.CASES, ids=ec.case_id)
def test_device_entry_equals_the_restatement(ctx, case):
    d, M, s, tag, T, N = case
    w, mu, cov, mc = ec.inputs(d, M, s, tag, T)
    model = _prepared(ctx, d, w, mu, cov)
    outs, Ls = ec.case_reference(case)
    for k in range(N + 1):
        got, lik = ec.convert_em(ctx, model, M, mc, k)
        what = f'{ec.case_id(case)}, em_iterations = {k}'
        assert np.array_equal(got[:, 0], mc[:, 0]), 'column 0 is copied'
        _close(got[:, 1:], outs[k][:, 1:], what)
        assert len(lik) == k + 1
        _close_lik(lik, Ls[:k + 1], what)
        _non_decreasing(lik, what)
        if k == N:
            bare, none = ec.convert_em(ctx, model, M, mc, k, loglik=False)
            assert none is None and np.array_equal(bare, got), 'the trajectory does not depend on loglik being asked for'


@pytest.mark.parametrize('count', (3, 17))
def test_batch_equals_single_bit_for_bit(ctx, count):
    d, M, s, tag, Ts, N = ec.BATCH
    w, mu, cov = cc.mixture(3 * d, M, tag, spread=s)
    model = _prepared(ctx, d, w, mu, cov)
    Ts = [Ts[j % len(Ts)] for j in range(count)]
    assert count <= len(ec.BATCH[4]) or count > ec.KWY_BATCH_MAX
    mcs = [cc.mcep(T, d, M, tag) for T in Ts]
    outs, liks = ec.convert_em_batch(ctx, model, M, mcs, N)
    bare, _ = ec.convert_em_batch(ctx, model, M, mcs, N, loglik=False)
    single = {}
    for j, mc in enumerate(mcs):
        if j < len(ec.BATCH[4]) or j >= ec.KWY_BATCH_MAX:      # the distinct lengths of each pass of launches
            single[j] = ec.convert_em(ctx, model, M, mc, N)
    for j, (y, lik) in single.items():
        assert np.isfinite(y).all()
        assert np.array_equal(outs[j], y), f'job {j} of {count}'
        assert liks[j] == lik, f'log-likelihoods of job {j} of {count}'
        assert np.array_equal(bare[j], y), f'job {j} of {count} without loglik'
    if count == 3:
        for mc, y, lik in zip(mcs, outs, liks):
            refs, Ls = ec.ref_mcep_em(mc, w, mu, cov, N)
            _close(y, refs[N], f'batch job of {len(mc)} frames')
            _close_lik(lik, Ls, f'batch job of {len(mc)} frames')


def test_empty_batch_is_ok(ctx):
    import ctypes
    from kwiiyatta_amd import _lib
    jobs = _lib.job_array(_lib.ConvertEmJob, [(None, 0, None, None)])
    assert _lib.lib.kwy_convert_mcep_em_batch_dev(ctx.handle, ctypes.cast(jobs, ctypes.c_void_p), 0, 24, 3, None,
                                                  2) == _lib.KWY_OK


def test_differential_model(ctx):
    d, M, s, tag, T, N = 24, 3, 0.2, 8, 33, 2
    w, mu, cov, mc = ec.inputs(d, M, s, tag, T)
    model = _prepared(ctx, d, w, mu, cov, diff=1)
    mu2, cov2 = ec.diff_mixture(mu, cov)
    refs, Ls = ec.ref_mcep_em(mc, w, mu2, cov2, N)
    got, lik = ec.convert_em(ctx, model, M, mc, N)
    _close(got, refs[N], 'diff = 1')
    _close_lik(lik, Ls, 'diff = 1')
    plain, _ = ec.convert_em(ctx, _prepared(ctx, d, w, mu, cov), M, mc, N)
    assert np.abs(plain - got).max() > 1e-2 * np.abs(plain).max()


@pytest.mark.parametrize('d,M,s,tag,T,N,diff', ((2, 3, 1.0, 7, 17, 4, 0), (24, 3, 0.2, 8, 33, 2, 0), (24, 3, 0.2, 8, 33, 2, 1)))
def test_host_entry_equals_device_entry_bit_for_bit(ctx, d, M, s, tag, T, N, diff):
    w, mu, cov, mc = ec.inputs(d, M, s, tag, T)
    dev, lik = ec.convert_em(ctx, _prepared(ctx, d, w, mu, cov, diff), M, mc, N)
    y, hlik = ec.mlpg_em_host(ctx, mc[:, 1:], w, mu, cov, N, diff)
    assert np.isfinite(y).all() and np.array_equal(y, dev[:, 1:])
    assert hlik == lik


def test_refusals_write_nothing(ctx):
    from kwiiyatta_amd import _lib
    d, M, s, tag, T = 2, 3, 1.0, 7, 17
    w, mu, cov, mc = ec.inputs(d, M, s, tag, T)
    model = _prepared(ctx, d, w, mu, cov)
    for N in (-1, ec.KWY_MLPG_EM_MAX + 1):
        rc, out, lik = ec.convert_em(ctx, model, M, mc, N, check=False)
        assert rc == _lib.KWY_EINVAL and np.isnan(out).all() and np.isnan(lik).all(), N
    import torch
    din, = cc._dev(mc)
    out = torch.full((T, d + 1), np.nan, dtype=torch.float64, device='cuda')
    lik = torch.full((3,), np.nan, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    call = _lib.lib.kwy_convert_mcep_em_dev
    h, m = ctx.handle, model.data_ptr()
    assert call(h, din.data_ptr(), 0, d, M, m, 2, out.data_ptr(), lik.data_ptr()) == _lib.KWY_EINVAL
    assert call(h, None, T, d, M, m, 2, out.data_ptr(), lik.data_ptr()) == _lib.KWY_EINVAL
    assert call(h, din.data_ptr(), T, d, M, None, 2, out.data_ptr(), lik.data_ptr()) == _lib.KWY_EINVAL
    assert call(h, din.data_ptr(), T, d, M, m, 2, None, lik.data_ptr()) == _lib.KWY_EINVAL
    ctx.sync()
    assert torch.isnan(out).all() and torch.isnan(lik).all()
    x = np.ascontiguousarray(mc[:, 1:])
    y, hl = np.full(x.shape, np.nan), np.full(3, np.nan)
    for N in (-1, ec.KWY_MLPG_EM_MAX + 1):
        rc = _lib.lib.kwy_gmm_mlpg_em(h, _lib.ptr(x), T, d, M, _lib.ptr(w), _lib.ptr(mu), _lib.ptr(cov), 0, N, _lib.ptr(y),
                                      _lib.ptr(hl))
        assert rc == _lib.KWY_EINVAL and np.isnan(y).all() and np.isnan(hl).all()
    # the call still works afterwards
    got, _ = ec.convert_em(ctx, model, M, mc, 2)
    assert np.isfinite(got).all()


def test_python_front_end(ctx):
    """backend.mlpg.MLPG(em=N) runs kwy_gmm_mlpg_em and keeps its log-likelihoods"""
    from types import SimpleNamespace
    from kwiiyatta_amd.backend.mlpg import DELTA_WINDOWS, MLPG
    d, M, s, tag, T, N = 24, 3, 0.2, 8, 33, 2
    w, mu, cov, mc = ec.inputs(d, M, s, tag, T)
    gmm = SimpleNamespace(weights_=w, means_=mu, covariances_=cov, covariance_type='full')
    refs, Ls = ec.ref_mcep_em(mc, w, mu, cov, N)
    stage = MLPG(gmm, windows=DELTA_WINDOWS, em=N, ctx=ctx)
    y = stage.transform(cc.delta_features(mc[:, 1:]))
    _close(y, refs[N][:, 1:], 'MLPG(em=2)')
    _close_lik(stage.loglik_, Ls, 'MLPG(em=2)')
    hard = MLPG(gmm, windows=DELTA_WINDOWS, ctx=ctx)
    z = hard.transform(mc[:, 1:])
    assert hard.loglik_ is None and hard.em is None and np.isfinite(z).all()
    y0 = MLPG(gmm, windows=DELTA_WINDOWS, em=0, ctx=ctx).transform(mc[:, 1:])
    assert np.abs(z - y0).max() > 1e-2 * np.abs(y0).max(), 'the arg-max conversion is another trajectory'


def test_through_the_package(tmp_path):
    """a converter of 2 components trained on two CLB -> SLT files: convert(mc, em=N) against the restatement on the
    mixture it fitted, on 257 frames of speech.  N is the largest of 2, 1, 0 at which the conditioning gate of
    tests/test_em_cases.py holds for this mixture and track (computed here, on the CPU, from the restatement alone)."""
    import pathlib
    import shutil
    import kwiiyatta_amd as k
    from conftest import CLB_DIR, SLT_DIR
    src = tmp_path / 'src'
    src.mkdir()
    for n in (1, 2):
        shutil.copy(pathlib.Path(CLB_DIR) / f'arctic_a{n:04}.wav', src)
    dataset = k.align(k.WavFileDataset(src), k.WavFileDataset(pathlib.Path(SLT_DIR)))
    conv = k.MelCepstrumConverter(use_delta=True, components=2, random_state=0)
    np.random.seed(0)
    conv.train(dataset, sorted(dataset.keys())[:2])
    full = k.analyze_wav(pathlib.Path(CLB_DIR) / 'arctic_a0001.wav').mel_cepstrum
    mc = np.ascontiguousarray(full.data[100:357], dtype=np.float64)
    gmm = conv.gmm
    w, mu, cov = (np.asarray(a, dtype=np.float64) for a in (gmm.weights_, gmm.means_, gmm.covariances_))
    logp, E, v = ec.terms(mc, w, mu, cov)
    ys, Ls = ec.em_from_terms(logp, E, v, 2)
    moved = np.zeros(3)
    for seed in range(3):
        rng = np.random.default_rng([seed, 4])
        ps, _ = ec.em_from_terms(logp * (1 + 1e-13 * rng.standard_normal(logp.shape)),
                                 E * (1 + 1e-13 * rng.standard_normal(E.shape)), v, 2)
        moved = np.maximum(moved, [np.abs(a - b).max() / np.abs(b).max() for a, b in zip(ps, ys)])
    print(f'conditioning of y_0, y_1, y_2 on the trained mixture: {moved}')
    assert moved[0] <= 3e-10
    N = max(n for n in range(3) if moved[:n + 1].max() <= 3e-10)
    got = conv.convert(k.MelCepstrum(full.fs, full.frame_period, mc), em=N).data
    assert np.array_equal(got[:, 0], mc[:, 0])
    _close(got[:, 1:], ys[N], f'converter.convert(em={N})')
    hard = conv.convert(k.MelCepstrum(full.fs, full.frame_period, mc)).data
    assert np.isfinite(hard).all()
