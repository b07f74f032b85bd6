"""k_align_features (kwy_align.hip) around its work unit: a workgroup finds the utterance's power threshold (the
maximum of c0 over ALL frames, minus the offset) and writes the feature rows of 64 consecutive frames, element by
element.  kwy_align_features_dev and kwy_align_features_batch_dev against the numpy statement of tests/align_cases.py,
exactly (index, copy and fixed-expression work: no tolerance): T below, at and beyond 8 frames (the former unit) and
64 frames (this one), the maximum in the first frame, in the last one -- the last workgroup's, which every other
workgroup has to see -- and shared by all frames, and a ragged batch in which every utterance has a maximum of its
own, so that a threshold taken from a neighbour shows in the power column."""
import numpy as np
import pytest

import align_cases as ac

pytestmark = pytest.mark.gpu

FRAMES = 64                                     # AL_FEAT_FRAMES of kwy_align.hip
T_CASES = (1, 7, 8, 9, FRAMES - 1, FRAMES, FRAMES + 1, 2 * FRAMES + 3)
NCOEF = (1, 25, 33)                             # rows of 2, 26 and 34 values
MODES = ('first', 'last', 'all')
F_SENT, GUARD = -7.25, 16


def _case(T, ncoef, mode, seed=0):
    mc, f0 = ac.feature_case(T, ncoef, 'first' if mode == 'all' else mode, seed=seed)
    if mode == 'all':
        mc[:, 0] = 6.0
    return mc, f0


class Glue:
    def __init__(self):
        import torch
        from kwiiyatta_amd import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.lib
        self.ctx = _lib.Context(0)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def fill(self, shape):
        return self.up(np.full(shape, F_SENT))

    def ok(self, name, *args):
        rc = getattr(self.lib, name)(self.ctx.handle, *[a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args])
        assert rc == self._lib.KWY_OK, (name, rc, self.ctx.error())

    def down(self, *tensors):
        self.ctx.sync()
        return [t.cpu().numpy() for t in tensors]


@pytest.fixture(scope='module')
def g():
    return Glue()


def _single(g, mc, f0):
    T, ncoef = mc.shape
    out = g.fill((T + GUARD, ncoef + 1))
    g.ok('kwy_align_features_dev', g.up(mc), T, ncoef, g.up(f0), ac.POWER_WEIGHT, ac.POWER_THRESHOLD, ac.VUV_WEIGHT, out)
    out, = g.down(out)
    assert (out[T:] == F_SENT).all(), (T, ncoef)            # nothing behind the last frame
    return out[:T]


@pytest.mark.parametrize('mode', MODES)
def test_single_entry_against_the_statement(g, mode):
    for T in T_CASES:
        for ncoef in NCOEF:
            mc, f0 = _case(T, ncoef, mode)
            want = ac.align_features(mc, f0)
            if mode == 'all':
                assert (want[:, 0] == ac.POWER_WEIGHT).all()
            assert ac.same(_single(g, mc, f0), want), (T, ncoef, mode)


def test_ragged_batch_every_threshold_its_own(g):
    """utterance k's c0 is shifted by 2 k (exact: c0 is a multiple of 1/8), the offset is 1.5: with a neighbour's
    threshold the power column would be all set or all clear."""
    Ts = list(T_CASES) + [3 * FRAMES, 100]
    for ncoef in (25, 2):
        cases = []
        for k, T in enumerate(Ts):
            mc, f0 = _case(T, ncoef, MODES[k % 3], seed=k)
            mc[:, 0] += 2.0 * k
            cases.append((mc, f0))
        mcs, f0s = [g.up(mc) for mc, _ in cases], [g.up(f0) for _, f0 in cases]
        outs = [g.fill((T + GUARD, ncoef + 1)) for T in Ts]
        jobs = g._lib.job_array(g._lib.AlignJob, [(mcs[k], f0s[k], Ts[k], outs[k]) for k in range(len(Ts))])
        g.ok('kwy_align_features_batch_dev', jobs, len(Ts), ncoef, ac.POWER_WEIGHT, ac.POWER_THRESHOLD, ac.VUV_WEIGHT)
        for k, out in enumerate(g.down(*outs)):
            assert (out[Ts[k]:] == F_SENT).all(), k
            want = ac.align_features(*cases[k])
            assert 0 < (want[:, 0] > 0).sum() and (Ts[k] < 9 or MODES[k % 3] == 'all' or (want[:, 0] == 0).any()), k
            assert np.array_equal(out[:Ts[k]], want), k
            assert np.array_equal(out[:Ts[k]], _single(g, *cases[k])), k
