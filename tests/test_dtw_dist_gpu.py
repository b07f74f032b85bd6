"""k_dtw_dist (kwy_dtw.hip) at the edges of its work unit: a workgroup takes a run of 64 consecutive steps of one
strip of 64 rows, 32 dimensions at a time.  A level reaches the kernel only with more than 64 rows (a single-strip
level computes its distances inside k_dtw_small), so every case has Tx > 64.  The distances feed the recurrence and
the back-trace, so a wrong, missing or misplaced cell shows in the path or in the distance: both must EQUAL the
oracle's (fastdtw 0.3.2 with dist=2), as in tests/test_backends_gpu.py::test_fastdtw_bit_exact, which keeps covering
the workload's 2201 x 2401 x 26."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [
    (65, 70, 1, 1),                             # a second strip of one row
    (128, 129, 31, 2), (129, 128, 32, 2),       # the dimension tile one short and exactly full; a strip boundary at the end
    (130, 150, 33, 3),                          # one dimension into the second tile
    (191, 260, 26, 32),                         # the workload's dim and radius, a full-width window, partial last runs
    (150, 300, 26, 1), (300, 150, 26, 1),       # steep paths, narrow windows, strips with very different step counts
]
BATCH = [(191, 260), (40, 90), (130, 77)]       # (40, 90): a single strip at every level -- it sits k_dtw_dist out


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


def _series(rng, T, dim, warp):
    t = np.linspace(0, 1, T) ** warp
    base = np.stack([np.sin(2 * np.pi * (k + 1) * t * 3 + k) for k in range(dim)], 1)
    return base + 0.05 * rng.standard_normal((T, dim))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('Tx,Ty,dim,radius', CASES)
def test_fastdtw_equals_the_oracle(ko, Tx, Ty, dim, radius):
    from kwiiyatta_amd.backend import dtw
    rng = np.random.default_rng(Tx * 7919 + Ty)
    x, y = _series(rng, Tx, dim, 1.0), _series(rng, Ty, dim, 1.3)
    d_ref, p_ref = ko.fastdtw(x, y, radius=radius, dist=2)
    d_got, p_got = dtw.fastdtw(x, y, radius=radius, dist=2)
    assert p_got == p_ref
    assert d_got == d_ref


def test_batch_of_three_equals_single_calls_and_oracle(ko):
    """kwy_fastdtw_batch_dev on three pairs of different lengths, one of them without a multi-strip level: every
    pair equals its own kwy_fastdtw_dev call and the oracle."""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, c_vp
    dim, radius = 26, 32
    rng = np.random.default_rng(77)
    xs = [_series(rng, a, dim, 1.0) for a, _ in BATCH]
    ys = [_series(rng, b, dim, 1.3) for _, b in BATCH]
    ctx = _lib.Context(0)
    dxs, dys = [_dev(x) for x in xs], [_dev(y) for y in ys]
    paths = [torch.zeros((a + b + 2, 2), dtype=torch.int32, device='cuda') for a, b in BATCH]
    lens = torch.zeros(len(BATCH), dtype=torch.int64, device='cuda')
    dists = torch.zeros(len(BATCH), dtype=torch.float64, device='cuda')
    jobs = _lib.job_array(_lib.DtwJob, [(dxs[i], BATCH[i][0], dys[i], BATCH[i][1], dists[i:i + 1], paths[i],
                                         lens[i:i + 1]) for i in range(len(BATCH))])
    _lib.check(ctx, lib.kwy_fastdtw_batch_dev(ctx.handle, jobs, len(BATCH), dim, radius))
    ctx.sync()
    for i, (a, b) in enumerate(BATCH):
        path1 = torch.zeros((a + b + 2, 2), dtype=torch.int32, device='cuda')
        n1 = torch.zeros(1, dtype=torch.int64, device='cuda')
        d1 = torch.zeros(1, dtype=torch.float64, device='cuda')
        _lib.check(ctx, lib.kwy_fastdtw_dev(ctx.handle, c_vp(dxs[i].data_ptr()), a, c_vp(dys[i].data_ptr()), b, dim,
                                            radius, c_vp(d1.data_ptr()), c_vp(path1.data_ptr()), c_vp(n1.data_ptr())))
        ctx.sync()
        pb = paths[i].cpu().numpy()[:int(lens[i].item())]
        assert np.array_equal(pb, path1.cpu().numpy()[:int(n1.item())]), BATCH[i]
        assert float(dists[i].item()) == float(d1.item()), BATCH[i]
        d_ref, p_ref = ko.fastdtw(xs[i], ys[i], radius=radius, dist=2)
        assert [tuple(r) for r in pb.tolist()] == p_ref and float(dists[i].item()) == d_ref, BATCH[i]
