"""The HBM-resident drivers with the EM trajectory conversion switched on (corpus.ConvertWave / convert_batch /
evaluate_batch, `mlpg_em=N`): they call kwy_convert_mcep_em_batch_dev where they called kwy_convert_mcep_batch_dev, for
the plain and the differential conversion, and stay bit for bit what they were without the option."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 16000
EM = 2


@pytest.fixture(scope='module')
def utterances():
    from kwiiyatta_amd.synthetic import make_utterance
    return [make_utterance(seed=41, fs=FS, seconds=0.3), make_utterance(seed=42, fs=FS, seconds=0.4, f0_base=190.0)]


@pytest.fixture(scope='module')
def mixture():
    from kwiiyatta_amd import pipeline as pl
    return pl.synthetic_gmm(order=24, components=4, seed=0, n_frames=3000)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _wave(utterances, mixture, **options):
    import torch
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd import pipeline as pl
    dg = pl.DeviceGMM(mixture.weights_, mixture.means_, mixture.covariances_, torch.device('cuda', 0))
    ls = corpus._Lockstep(0)
    wv = corpus.ConvertWave(ls, FS, utterances, gmm=dg, diff=True, **options)
    wv.run()
    ls.sync()
    return wv, dg


def test_convert_wave_and_batch_run_the_em_entries(utterances, mixture):
    import torch
    from kwiiyatta_amd import _lib, corpus
    wv, dg = _wave(utterances, mixture, mlpg_em=EM)
    plain, _ = _wave(utterances, mixture)
    assert wv.mlpg_em == EM and plain.mlpg_em is None
    assert _bytes(wv.mc) == _bytes(plain.mc), 'the analysis does not see the option'
    ctx = _lib.Context(0)
    first = 0
    for i, T in enumerate(wv.T):
        rows = slice(first, first + T)
        first += T
        for model, got in ((wv.model, wv.mc_conv[rows]), (wv.model_diff, wv.mc_diff[rows])):
            mc = wv.mc[rows].contiguous()
            out = torch.full_like(mc, float('nan'))
            torch.cuda.synchronize()
            _lib.check(ctx, _lib.lib.kwy_convert_mcep_em_dev(ctx.handle, mc.data_ptr(), T, 24, dg.M, model.data_ptr(), EM,
                                                             out.data_ptr(), None))
            ctx.sync()
            assert bool(torch.isfinite(out).all()) and _bytes(got) == _bytes(out), i
    assert _bytes(wv.mc_conv) != _bytes(plain.mc_conv) and _bytes(wv.mc_diff) != _bytes(plain.mc_diff)
    batch = corpus.convert_batch(utterances, FS, mixture, diff=True, mlpg_em=EM)
    before = corpus.convert_batch(utterances, FS, mixture, diff=True)
    unset = corpus.convert_batch(utterances, FS, mixture, diff=True, mlpg_em=None)
    for i in range(len(utterances)):
        assert _bytes(batch[0][i]) == _bytes(wv.wave[i]) and _bytes(batch[2][i]) == _bytes(wv.wave_diff[i]), i
        assert _bytes(before[0][i]) == _bytes(unset[0][i]) == _bytes(plain.wave[i]), i
        assert _bytes(before[2][i]) == _bytes(unset[2][i]) == _bytes(plain.wave_diff[i]), i
        assert _bytes(batch[0][i]) != _bytes(before[0][i]) and bool(torch.isfinite(batch[0][i]).all()), i
    for bad in (True, 1.5, -1, 17):
        with pytest.raises(ValueError, match='mlpg_em'):
            corpus.convert_batch(utterances, FS, mixture, mlpg_em=bad)
    with pytest.raises(ValueError, match='lockstep'):
        corpus.convert_batch(utterances, FS, mixture, driver='streams', mlpg_em=1)


def test_evaluate_batch_measures_the_em_conversion(utterances):
    """on a mixture whose neighbours overlap (convert_cases.mixture at spread 0.2): the fitted synthetic mixture above
    has one-hot posteriors on these utterances, where the EM conversion equals the arg-max one to rounding), and with
    mlpg_em = 0, the single solve under the source-only posteriors: at D = 72 the re-estimated posteriors of later
    iterations sharpen to one-hot, and here they settle on the arg-max sequence (31.0636119406247 dB either way)"""
    from types import SimpleNamespace
    import convert_cases as cc
    from kwiiyatta_amd import corpus
    w, mu, cov = cc.mixture(72, 4, 8, spread=0.2)
    mixture = SimpleNamespace(weights_=w, means_=mu, covariances_=cov)
    pairs = [(utterances[0], utterances[1]), (utterances[1], utterances[0])]
    figures = {}
    for name, options in (('before', {}), ('unset', dict(mlpg_em=None)), ('em', dict(mlpg_em=0))):
        np.random.seed(3)
        records, total = corpus.evaluate_batch(pairs, FS, mixture, order=24, frames='all', **options)
        figures[name] = [r['mcd_moments'] for r in records] + [total['mcd_moments']]
        assert all(np.isfinite(m).all() and m[0] > 0 for m in figures[name]), name
    assert figures['before'] == figures['unset']
    for a, b in zip(figures['em'], figures['before']):
        print(f'mcd moments with mlpg_em = 0: {a}; without: {b}')
        assert a[0] == b[0], 'the alignment does not see the conversion'
        assert abs(a[1] - b[1]) > 1e-6 * b[1], 'another conversion, another distortion'
