"""The device-resident driver of non-parallel training (corpus.train_converter_nonparallel) against the Python API path
(MelCepstrumFeatureConverter.train_nonparallel), and backend.nn.nearest's centring beside rows that are not finite."""
import numpy as np
import pytest

import inca_cases
import nn_cases

pytestmark = pytest.mark.gpu

FS = 16000


@pytest.fixture(scope='module')
def sides():
    """three source and two target utterances of another voice and other lengths, (x, f0, t) each: f0 from the package's
    own DIO + StoneMask, as the Analyzer of the API path finds it"""
    from kwiiyatta_amd.backend import world
    from kwiiyatta_amd.synthetic import make_utterance
    out = []
    for seeds, warp, form in (((100, 101, 102), 1.0, 1.0), ((203, 204), 1.1, 1.12)):
        side = []
        for k, seed in enumerate(seeds):
            x, _, _ = make_utterance(seed=seed, fs=FS, seconds=1.0 + 0.1 * k, time_warp=warp, formant_scale=form)
            f0, t = world.dio(x, FS, frame_period=5)
            side.append((x, world.stonemask(x, f0, t, FS), t))
        out.append(side)
    return out


def test_api_path_equals_the_driver(sides):
    """N = 2: the joint matrix of every fit bit for bit, rows, monitor and EM iterations of every record, the mixture
    within the bounds of test_realign_gpu.py::test_api_path_equals_the_driver; the f0 moments and the global variance
    beside the API path's statistics"""
    import kwiiyatta_amd as kw
    from kwiiyatta_amd import corpus as cp
    from kwiiyatta_amd.backend import f0 as f0map
    src, tgt = ({f'{name}{k}': kw.Analyzer(kw.Wavdata(FS, u[0])) for k, u in enumerate(side)}
                for name, side in zip('st', sides))
    conv = inca_cases.recording_converter(kw, components=2, random_state=0, verbose=0)
    conv.train_nonparallel(src, tgt, sorted(src), sorted(tgt), iterations=2, f0_stats=True, gv_stats=True)
    g, history, moments, gv = cp.train_converter_nonparallel(sides[0], sides[1], FS, components=2, seed=0, iterations=2,
                                                             keep_matrices=True, f0_moments=True, gv_moments=True)
    matrices = inca_cases.recorded_matrices(conv)
    assert len(matrices) == len(history) == len(conv.nonparallel_history) == 3
    for it, (got, rec, api) in enumerate(zip(matrices, history, conv.nonparallel_history)):
        want = rec['X'].cpu().numpy()
        print(f'fit {it}: rows api {api["rows"]} driver {rec["rows"]} monitor api {api["mcd"]!r} driver {rec["mcd"]!r} '
              f'EM api {api["em_iterations"]} driver {rec["em_iterations"]}')
        assert got.shape == want.shape and np.array_equal(got, want), it
        assert api['rows'] == rec['rows'] == len(want) > 100
        assert api['mcd'] == pytest.approx(rec['mcd'], rel=1e-12) and np.isfinite(api['mcd'])
        assert api['em_iterations'] == rec['em_iterations']
    assert np.allclose(conv.gmm.weights_, g.weights_, rtol=1e-6, atol=1e-10)
    assert np.allclose(conv.gmm.means_, g.means_, rtol=1e-6, atol=1e-8)
    assert np.allclose(conv.gmm.covariances_, g.covariances_, rtol=1e-5, atol=1e-9)
    assert np.allclose(f0map.stats_from_moments(*moments), conv.f0_stats, rtol=1e-12, atol=0)
    assert np.allclose(gv, conv.gv_stats, rtol=1e-12, atol=0)


def test_driver_argument_checks(sides):
    from kwiiyatta_amd import corpus as cp
    with pytest.raises(ValueError, match=r'within \[0, 64\]'):
        cp.train_converter_nonparallel(sides[0], sides[1], FS, iterations=65)
    with pytest.raises(ValueError, match='no target files'):
        cp.train_converter_nonparallel(sides[0], [], FS, iterations=0)


def test_centring_leaves_rows_that_are_not_finite_aside(gpu_ctx):
    """nearest(center=True): a candidate row with a NaN or an infinity is never chosen and does not spoil the mean the
    other rows are centred by; dist2 is the distance of the rows as given, summed in the kernel's order"""
    from kwiiyatta_amd.backend import nn
    Q, C = nn_cases.normal_rows(91, 40, 7, offset=50.0), nn_cases.normal_rows(92, 70, 7, offset=50.0)
    want = nn_cases.nearest(Q, C)[0]
    for j, v in zip(sorted(set(want.tolist()))[:3], (np.nan, np.inf, -np.inf)):
        C[j, j % 7] = v
    want, want_d = nn_cases.nearest(Q, C)
    for center in (True, False):
        idx, dist2 = nn.nearest(Q, C, center=center, ctx=gpu_ctx)
        assert np.array_equal(idx, want) and np.isfinite(C[idx]).all()
        direct = np.zeros(len(Q))
        for k in range(7):
            direct += (Q[:, k] - C[idx, k]) * (Q[:, k] - C[idx, k])
        assert np.array_equal(dist2, direct)
        assert np.allclose(dist2, want_d.astype(np.float64), rtol=8 * 2.0 ** -52, atol=0)
    with pytest.raises(ValueError, match='no finite score'):
        nn.nearest(Q, np.full((3, 7), np.nan), ctx=gpu_ctx)
