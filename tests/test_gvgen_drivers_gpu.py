"""The conversion with the GV ascent behind it (kwy_gmm_mlpg_gv, kwy_convert_mcep_gv_dev, kwy_convert_mcep_gv_batch_dev)
against the numpy restatement chained behind the numpy conversions of tests/em_cases.py / convert_cases.py, its bit
equalities, and the option through the Python stack: MLPG, the converter, the corpus drivers and the two commands.

Bound of the chained comparison: 1e-9 of the largest reference value for y_N and 1e-9 of Q_k's term magnitudes, the
bound of tests/test_gvgen_gpu.py; tests/test_gvgen_cases.py shows every chained case to pass the conditioning gate.
"""
import pathlib
import shutil
import sys

import numpy as np
import pytest

import convert_cases as cc
import em_cases as ec
import gvgen_cases as gc
from conftest import CLB_DIR, SLT_DIR

pytestmark = pytest.mark.gpu

TOL = 1e-9
FS = 16000
GV = 4
TRAINED, HELD_OUT = 4, 2


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


def _close_objective(got, ref, mags, what):
    assert len(got) == len(ref)
    for k, (a, b, m) in enumerate(zip(got, ref, mags)):
        print(f'{what}: Q_{k} = {a!r}, numpy {b!r}, term magnitudes {m:.3e}')
        assert abs(a - b) <= TOL * m, (what, k)
    assert all(got[k + 1] >= got[k] for k in range(len(got) - 1)), (what, list(got))


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ---- against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', gc.CHAINED, ids=gc.chained_id)
def test_entries_equal_the_chained_restatement(ctx, case):
    d, M, spread, tag, T, diff, em = case
    w, mu, cov, mc, s, mean, var, rec, y, (ys, Qs, mags, status) = gc.chained_reference(case)
    N = gc.CHAINED_N
    model = _prepared(ctx, d, w, mu, cov, diff)
    out, lik, obj, st = gc.convert_gv(ctx, model, M, mc, em, diff, mean, var, N)
    what = gc.chained_id(case)
    assert st == status == 0 and np.array_equal(out[:, 0], mc[:, 0]), 'column 0 is copied'
    _close(out[:, 1:], ys[N], what + ', kwy_convert_mcep_gv_dev')
    _close_objective(obj, Qs, mags, what)
    if em >= 0:
        _, em_lik = ec.convert_em(ctx, model, M, mc, em)
        assert lik.tolist() == em_lik, 'the log-likelihoods are those of the EM entry'
    hy, hlik, hobj, hst = gc.mlpg_gv_host(ctx, mc[:, 1:], w, mu, cov, diff, em, diff, mean, var, N)
    assert hst == 0
    _close(hy, ys[N], what + ', kwy_gmm_mlpg_gv')
    _close_objective(hobj, Qs, mags, what + ', kwy_gmm_mlpg_gv')


# ---- bit equality and stability --------------------------------------------------------------------------------------------
def _existing(ctx, model, M, mc, em):
    return cc.convert_mcep(ctx, model, M, mc) if em < 0 else ec.convert_em(ctx, model, M, mc, em, loglik=False)[0]


@pytest.mark.parametrize('diff, em', ((0, -1), (1, -1), (0, 2), (1, 2)))
def test_no_iterations_on_the_tracks_own_variance_is_the_existing_entry(ctx, diff, em):
    d, M, spread, tag, T = gc.CHAINED_SIZES[1]
    w, mu, cov, mc = ec.inputs(d, M, spread, tag, T)
    model = _prepared(ctx, d, w, mu, cov, diff)
    base = _existing(ctx, model, M, mc, em)
    mean = (base[:, 1:] + mc[:, 1:] if diff else base[:, 1:]).var(axis=0)
    out, lik, obj, st = gc.convert_gv(ctx, model, M, mc, em, diff, mean, (0.3 * mean) ** 2, 0)
    assert st == 0 and np.array_equal(out[:, 0], base[:, 0])
    err = np.abs(out - base).max() / np.abs(base).max()
    print(f'diff {diff}, em {em}: gv_iterations = 0 at mu = v moves the trajectory by {err:.3e} of its peak')
    assert err <= 1e-12


@pytest.mark.parametrize('count', (3, 17))
def test_batch_equals_single_bit_for_bit_and_runs_repeat(ctx, count):
    d, M, spread, tag, Ts, _ = ec.BATCH
    w, mu, cov = cc.mixture(3 * d, M, tag, spread=spread)
    model = _prepared(ctx, d, w, mu, cov, 1)
    Ts = [Ts[j % len(Ts)] for j in range(count)]
    mcs = [cc.mcep(T, d, M, tag) for T in Ts]
    mean = 2.0 * mcs[1][:, 1:].var(axis=0)
    var = (0.3 * mean) ** 2
    res = gc.convert_gv(ctx, model, M, mcs, 2, 1, mean, var, GV)
    again = gc.convert_gv(ctx, model, M, mcs, 2, 1, mean, var, GV)
    for j in list(range(len(ec.BATCH[4]))) + ([count - 1] if count > gc.KWY_BATCH_MAX else []):
        one = gc.convert_gv(ctx, model, M, mcs[j], 2, 1, mean, var, GV)
        assert np.isfinite(one[0]).all() and one[3] == 0
        for a, b, c in zip(res[j][:3], one[:3], again[j][:3]):
            assert np.array_equal(a, b) and np.array_equal(a, c), f'job {j} of {count}'
        assert all(one[2][k + 1] >= one[2][k] for k in range(GV))
        assert not np.array_equal(one[0], _existing(ctx, model, M, mcs[j], 2)), 'the ascent moves the trajectory'


@pytest.mark.parametrize('what, kwargs', (
    ('gv_iterations below 0', dict(N=-1)),
    ('gv_iterations above the maximum', dict(N=gc.KWY_MLPG_GV_MAX + 1)),
    ('em_iterations below -1', dict(em=-2)),
    ('em_iterations above the maximum', dict(em=ec.KWY_MLPG_EM_MAX + 1)),
    ('weight 0', dict(weight=0.0)),
    ('weight NaN', dict(weight=float('nan'))),
))
def test_refusals_write_nothing(ctx, what, kwargs):
    from kwiiyatta_amd import _lib
    d, M, spread, tag, T = gc.CHAINED_SIZES[0]
    w, mu, cov, mc = ec.inputs(d, M, spread, tag, T)
    model = _prepared(ctx, d, w, mu, cov)
    args = dict(em=0, N=2, weight=1.0)
    args.update(kwargs)
    rc, out, lik, obj, st = gc.convert_gv(ctx, model, M, mc, args['em'], 0, np.ones(d), np.ones(d), args['N'],
                                          weight=args['weight'], check=False)
    assert rc == _lib.KWY_EINVAL, what
    assert np.isnan(out).all() and np.isnan(lik).all() and np.isnan(obj).all() and st == -1, what


def test_empty_batch_is_ok(ctx):
    import ctypes
    from kwiiyatta_amd import _lib
    jobs = _lib.job_array(_lib.ConvertGvJob, [(None, 0, None, None, None)])
    assert _lib.lib.kwy_convert_mcep_gv_batch_dev(ctx.handle, ctypes.cast(jobs, ctypes.c_void_p), 0, 24, 3, None, 2, 0,
                                                  None, None, 1.0, 2, None) == _lib.KWY_OK


# ---- MLPG and the converter ---------------------------------------------------------------------------------------------
class _Gmm:
    covariance_type = 'full'

    def __init__(self, w, mu, cov):
        self.weights_, self.means_, self.covariances_ = w, mu, cov


@pytest.mark.parametrize('diff, em', ((False, None), (True, 2)))
def test_mlpg_sets_objective_and_loglik(ctx, diff, em):
    from kwiiyatta_amd.backend import mlpg
    d, M, spread, tag, T = gc.CHAINED_SIZES[0]
    w, mu, cov, mc = ec.inputs(d, M, spread, tag, T)
    x = np.ascontiguousarray(mc[:, 1:])
    mean = 2.0 * x.var(axis=0)
    var = (0.3 * mean) ** 2
    m = mlpg.MLPG(_Gmm(w, mu, cov), diff=diff, em=em, gv=(mean, var), gv_iterations=GV, gv_weight=2.0, ctx=ctx)
    y = m.transform(x)
    want = gc.mlpg_gv_host(ctx, x, w, mu, cov, int(diff), -1 if em is None else em, int(diff), mean, var, GV, weight=2.0)
    assert np.array_equal(y, want[0]) and m.objective_ == want[2].tolist() and len(m.objective_) == GV + 1
    assert all(m.objective_[k + 1] >= m.objective_[k] for k in range(GV))
    assert m.loglik_ is None if em is None else m.loglik_ == want[1].tolist()
    bad = mlpg.MLPG(_Gmm(w, mu, cov), gv=(mean, var * np.array([1.0, np.inf])), gv_iterations=1, ctx=ctx)
    with pytest.raises(ValueError, match=r'1 coefficient\(s\) were left'):
        bad.transform(x)


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """a small converter (2 components, seed 0, with the global-variance statistics) trained through the package API on
    the first 4 CLB -> SLT files, its model file, the dataset and the held-out keys"""
    import kwiiyatta_amd as k
    dataset = k.align(k.WavFileDataset(pathlib.Path(CLB_DIR)), k.WavFileDataset(pathlib.Path(SLT_DIR)))
    keys = sorted(dataset.keys())
    conv = k.MelCepstrumConverter(use_delta=True, components=2, random_state=0)
    np.random.seed(0)
    conv.train(dataset, keys[:TRAINED], gv_stats=True)
    root = tmp_path_factory.mktemp('gvgen')
    conv.save(root / 'model.npz')
    return conv, root, dataset, keys[TRAINED:TRAINED + HELD_OUT]


def test_training_keeps_the_variance_of_the_global_variance(trained):
    import kwiiyatta_amd as k
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd.converter.mcep import _target_mel_cepstra
    from kwiiyatta_amd.evaluate_voice import _triple
    conv, root, dataset, _ = trained
    keys = sorted(dataset.keys())[:TRAINED]
    per = np.stack([m.var(axis=0) for m in _target_mel_cepstra(dataset, keys, conv.order, conv.fs)])
    assert conv.gv_var.shape == (conv.order + 1,) and (conv.gv_var[1:] > 0).all()
    assert np.allclose(conv.gv_stats, per.mean(axis=0), rtol=1e-9) and np.allclose(conv.gv_var, per.var(axis=0), rtol=1e-8)
    back = k.MelCepstrumConverter(use_delta=True, components=2).load(root / 'model.npz')
    assert np.array_equal(back.gv_var, conv.gv_var)
    pairs = [tuple(_triple(k.analyze_wav(pathlib.Path(d) / key)) for d in (CLB_DIR, SLT_DIR)) for key in keys[:2]]
    np.random.seed(0)
    X, frames, gv, gv_var = corpus.build_training_matrix(pairs, FS, gv_moments=True, gv_variance=True)
    np.random.seed(0)
    X0, frames0, gv0 = corpus.build_training_matrix(pairs, FS, gv_moments=True)
    assert _bytes(X) == _bytes(X0) and gv.tobytes() == gv0.tobytes() and gv_var.shape == gv.shape
    assert np.allclose(gv_var, per[:2].var(axis=0), rtol=1e-7)
    with pytest.raises(ValueError, match='gv_moments'):
        corpus.build_training_matrix(pairs, FS, gv_variance=True)


@pytest.mark.parametrize('diff, em', ((False, None), (True, None), (True, 1)))
def test_converter_agrees_with_the_abi_call(ctx, trained, diff, em):
    import kwiiyatta_amd as k
    conv, _, dataset, held = trained
    source = k.analyze_wav(pathlib.Path(CLB_DIR) / held[0]).mel_cepstrum
    options = dict(diff=diff, **({} if em is None else dict(em=em)))
    got = conv.convert(source, mlpg_gv=GV, gv_weight=0.5, **options)
    mc = np.ascontiguousarray(source.data, dtype=np.float64)
    assert np.array_equal(got.data[:, 0], mc[:, 0])
    mean, var = conv.gv_ascent_statistics()
    gmm = conv.gmm
    model = _prepared(ctx, conv.order, gmm.weights_, gmm.means_, gmm.covariances_, int(diff))
    want, _, obj, st = gc.convert_gv(ctx, model, len(gmm.weights_), mc, -1 if em is None else em, int(diff), mean, var,
                                     GV, weight=0.5)
    assert st == 0 and all(obj[k + 1] >= obj[k] for k in range(GV))
    assert conv.gmm is gmm and conv.mlpg_.objective_ == obj.tolist()
    err = np.abs(got.data - want).max() / np.abs(want).max()
    print(f'diff {diff}, em {em}: converter - ABI = {err:.3e} of the peak; Q {obj[0]!r} -> {obj[-1]!r}')
    assert err <= 1e-12
    plain = conv.convert(source, **options)
    assert not np.array_equal(plain.data, got.data) and np.array_equal(plain.data, conv.convert(source, **options).data)
    z, z0 = ((c.data + mc if diff else c.data)[:, 1:].var(axis=0) for c in (got, plain))
    assert np.abs(z - mean).sum() < np.abs(z0 - mean).sum(), 'the variance moved towards the target statistic'


# ---- the corpus drivers ---------------------------------------------------------------------------------------------------
def _waves(keys):
    import kwiiyatta_amd as k
    return [np.ascontiguousarray(k.analyze_wav(pathlib.Path(CLB_DIR) / key).wavdata.data, dtype=np.float64) for key in keys]


def test_convert_wave_and_batch_run_the_gv_entries(ctx, trained):
    import torch
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd import pipeline as pl
    conv, _, _, held = trained
    waves = _waves(held)
    stats = dict(gv_stats=conv.gv_stats, gv_var=conv.gv_var)
    mean, var = conv.gv_ascent_statistics()

    def wave(**options):
        dg = pl.DeviceGMM(conv.gmm.weights_, conv.gmm.means_, conv.gmm.covariances_, torch.device('cuda', 0))
        ls = corpus._Lockstep(0)
        wv = corpus.ConvertWave(ls, FS, waves, gmm=dg, order=conv.order, diff=True, **options)
        wv.run()
        ls.sync()
        return wv, dg
    wv, dg = wave(mlpg_gv=GV, mlpg_em=1, **stats)
    plain, _ = wave(mlpg_em=1)
    assert wv.gvgen['iterations'] == GV and plain.gvgen is None and plain.gvgen_status is None
    assert wv.gvgen_status.cpu().tolist() == [0] * (2 * len(waves))
    assert _bytes(wv.mc) == _bytes(plain.mc), 'the analysis does not see the option'
    first = 0
    for i, T in enumerate(wv.T):
        rows = slice(first, first + T)
        first += T
        for model, got, offset in ((wv.model, wv.mc_conv[rows], 0), (wv.model_diff, wv.mc_diff[rows], 1)):
            out = gc.convert_gv(ctx, model, dg.M, wv.mc[rows].cpu().numpy(), 1, offset, mean, var, GV)[0]
            assert np.isfinite(out).all() and got.cpu().numpy().tobytes() == out.tobytes(), (i, offset)
    assert _bytes(wv.mc_conv) != _bytes(plain.mc_conv) and _bytes(wv.mc_diff) != _bytes(plain.mc_diff)
    opts = dict(order=conv.order, diff=True)
    batch = corpus.convert_batch(waves, FS, conv.gmm, mlpg_gv=GV, mlpg_em=1, **stats, **opts)
    before = corpus.convert_batch(waves, FS, conv.gmm, mlpg_em=1, **opts)
    unset = corpus.convert_batch(waves, FS, conv.gmm, mlpg_em=1, mlpg_gv=None, gv_var=conv.gv_var, **opts)
    for i in range(len(waves)):
        assert _bytes(batch[0][i]) == _bytes(wv.wave[i]) and _bytes(batch[2][i]) == _bytes(wv.wave_diff[i]), i
        assert _bytes(before[0][i]) == _bytes(unset[0][i]) == _bytes(plain.wave[i]), i
        assert _bytes(before[2][i]) == _bytes(unset[2][i]) == _bytes(plain.wave_diff[i]), i
        assert _bytes(batch[0][i]) != _bytes(before[0][i]) and bool(torch.isfinite(batch[0][i]).all()), i
    for bad in (True, 1.5, -1, 257):
        with pytest.raises(ValueError, match='iterations'):
            corpus.convert_batch(waves, FS, conv.gmm, mlpg_gv=bad, **stats, **opts)
    with pytest.raises(ValueError, match='needs gv_stats and gv_var'):
        corpus.convert_batch(waves, FS, conv.gmm, mlpg_gv=GV, gv_stats=conv.gv_stats, **opts)
    with pytest.raises(ValueError, match='two or more'):
        corpus.convert_batch(waves, FS, conv.gmm, mlpg_gv=GV, gv_stats=conv.gv_stats, gv_var=0.0 * conv.gv_var, **opts)
    with pytest.raises(ValueError, match='same variance twice'):
        corpus.convert_batch(waves, FS, conv.gmm, mlpg_gv=GV, gv_strength=1.0, **stats, **opts)
    with pytest.raises(ValueError, match='lockstep'):
        corpus.convert_batch(waves, FS, conv.gmm, driver='streams', mlpg_gv=GV, **stats)


def test_evaluate_batch_equals_the_package_path(trained):
    """corpus.evaluate_batch(mlpg_gv=...) against evaluate over evaluate_pair on the held-out pairs under one seed, to
    the bound tests/test_eval_gpu.py holds the two paths to without the option: equal figures"""
    import kwiiyatta_amd as k
    from kwiiyatta_amd import corpus, evaluate_voice as ev
    from kwiiyatta_amd.evaluate_voice import _triple
    conv, _, dataset, held = trained
    pairs = [tuple(_triple(k.analyze_wav(pathlib.Path(d) / key)) for d in (CLB_DIR, SLT_DIR)) for key in held]
    np.random.seed(1)
    results, total = ev.evaluate(conv, dataset, held, mlpg_gv=GV)
    np.random.seed(1)
    records, pooled = corpus.evaluate_batch(pairs, conv.fs, conv.gmm, order=conv.order, converter_fs=conv.fs, mlpg_gv=GV,
                                            gv_stats=conv.gv_stats, gv_var=conv.gv_var)
    np.random.seed(1)
    before, _ = corpus.evaluate_batch(pairs, conv.fs, conv.gmm, order=conv.order, converter_fs=conv.fs)
    np.random.seed(1)
    unset, _ = corpus.evaluate_batch(pairs, conv.fs, conv.gmm, order=conv.order, converter_fs=conv.fs, mlpg_gv=None)
    for key, r, d, b, u in zip(held, results, records, before, unset):
        print(f'{key}: MCD with mlpg_gv = {GV}: driver {d["mcd_moments"][1]!r} dB, package {r.mcd!r} dB; without '
              f'{b["mcd_moments"][1]!r} dB')
        assert d['aligned'] == r.aligned and d['mcd_moments'][0] == r.frames
        assert d['mcd_moments'][1] == r.mcd, key
        assert b == u and d['mcd_moments'][1] != b['mcd_moments'][1], key
    assert pooled['mcd_moments'][1] == total.mcd
    with pytest.raises(ValueError, match='same variance twice'):
        corpus.evaluate_batch(pairs, conv.fs, conv.gmm, order=conv.order, mlpg_gv=GV, gv_stats=conv.gv_stats,
                              gv_var=conv.gv_var, gv_strength=1.0)


# ---- the commands ---------------------------------------------------------------------------------------------------------
def _run_cli(main, argv):
    old = sys.argv
    sys.argv = ['prog'] + argv
    try:
        main()
    finally:
        sys.argv = old


def test_convert_voice_mlpg_gv(trained, monkeypatch):
    import kwiiyatta_amd as k
    import kwiiyatta_amd.convert_voice as cv
    from scipy.io import wavfile as sio
    conv, root, _, held = trained
    monkeypatch.setattr(k.Config, '_train', lambda *a, **kw: pytest.fail('a saved model must not be retrained'))
    src = root / 'src'
    src.mkdir()
    shutil.copy(pathlib.Path(CLB_DIR) / held[0], src)
    inputs = [str(src / pathlib.Path(held[0]).name)]
    model = ['--converter-components', '2', '--converter-model', str(root / 'model.npz')]
    for name, extra in (('plain', []), ('gvgen', ['--mlpg-gv', str(GV)]), ('batch', ['--mlpg-gv', str(GV), '--batch']),
                        ('em', ['--mlpg-gv', str(GV), '--mlpg-em', '1'])):
        _run_cli(cv.main, ['--result-dir', str(root / name)] + extra + model + inputs)
    stem = pathlib.Path(held[0]).stem
    for kind in ('synth', 'diff'):
        _, p = sio.read(root / 'plain' / f'{stem}.{kind}.wav')
        _, a = sio.read(root / 'gvgen' / f'{stem}.{kind}.wav')
        _, b = sio.read(root / 'batch' / f'{stem}.{kind}.wav')
        _, e = sio.read(root / 'em' / f'{stem}.{kind}.wav')
        assert a.shape == p.shape and not np.array_equal(a, p), kind
        assert not np.array_equal(a, e), kind
        # (the per-file and the batch path agree to one step of the 16-bit samples, as tests/test_gv_gpu.py holds them)
        assert a.shape == b.shape and np.abs(a.astype(np.int64) - b.astype(np.int64)).max() <= 1, kind
    old = root / 'old.npz'
    with np.load(root / 'model.npz') as z:
        np.savez(open(old, 'wb'), **{name: z[name] for name in z.files if name != 'gv_var'})
    with pytest.raises(SystemExit):
        _run_cli(cv.main, ['--mlpg-gv', str(GV), '--converter-components', '2', '--converter-model', str(old)] + inputs)


def test_evaluate_voice_mlpg_gv(trained, tmp_path, capsys, monkeypatch):
    import json
    import kwiiyatta_amd as k
    from kwiiyatta_amd import evaluate_voice as ev
    conv, root, dataset, held = trained
    monkeypatch.setattr(k.Config, '_train', lambda *a, **kw: pytest.fail('a saved model must not be retrained'))
    common = ['--source', CLB_DIR, '--target', SLT_DIR, '--converter-components', '2', '--converter-model',
              str(root / 'model.npz'), '--eval-skip-files', str(TRAINED), '--eval-max-files', str(HELD_OUT)]
    docs = {}
    for name, extra in (('plain', []), ('gvgen', ['--mlpg-gv', str(GV)]), ('batch', ['--mlpg-gv', str(GV), '--batch'])):
        np.random.seed(5)
        _run_cli(ev.main, common + extra + ['--json', str(tmp_path / f'{name}.json')])
        docs[name] = json.loads((tmp_path / f'{name}.json').read_text())
    capsys.readouterr()
    assert 'mlpg_gv' not in docs['plain']['options'] and docs['gvgen']['options']['mlpg_gv'] == GV
    np.random.seed(5)
    results, total = k.evaluate(conv, dataset, held, mlpg_gv=GV)
    assert docs['gvgen']['total']['mcd'] == total.mcd != docs['plain']['total']['mcd']
    for a, b in zip(docs['batch']['files'] + [docs['batch']['total']], docs['gvgen']['files'] + [docs['gvgen']['total']]):
        assert (a['frames'], a['aligned'], a['counts'], a['mcd']) == (b['frames'], b['aligned'], b['counts'], b['mcd'])
