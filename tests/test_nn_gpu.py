"""kwy_nn_search / kwy_nn_search_dev (include/kwy.h, "non-parallel training") through the C ABI against the longdouble
reference of tests/nn_cases.py: exact arithmetic on integer rows over the tile, wavefront and column-block edges,
ties, padding, independence of the slicing, the error bound on random doubles, rows that are not finite, the two
entry forms and the argument checks."""
import functools

import numpy as np
import pytest

import nn_cases

NQ = (1, 31, 32, 33, 257)
NC = (1, 15, 16, 17, 63, 64, 65, 129, 257)
DS = (1, 3, 4, 5, 16, 17, 49, 160)
U = 2.0 ** -53


def search(ctx, Q, C, splits=0, status=True, fill=None):
    """the host entry on numpy arrays -> (rc, idx, dist2, status word or None)"""
    from kwiiyatta_amd import _lib
    Q, C = np.ascontiguousarray(Q, dtype=np.float64), np.ascontiguousarray(C, dtype=np.float64)
    idx = np.full(len(Q), -7 if fill is None else fill, dtype=np.int32)
    dist2 = np.full(len(Q), -7.0)
    st = np.full(1, -7, dtype=np.int32) if status else None
    rc = _lib.lib.kwy_nn_search(ctx.handle, _lib.ptr(Q), len(Q), _lib.ptr(C), len(C), Q.shape[1], splits, _lib.ptr(idx),
                                _lib.ptr(dist2), _lib.ptr(st) if status else None)
    return rc, idx, dist2, None if st is None else int(st[0])


@functools.lru_cache(maxsize=None)
def integer_case(D):
    """257 integer queries and candidates of D columns with their exact score and distance matrices"""
    Q, C = nn_cases.integer_rows(100 + D, max(NQ), D), nn_cases.integer_rows(200 + D, max(NC), D)
    return Q, C, nn_cases.scores(Q, C), nn_cases.distances(Q, C)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- 1. exact arithmetic ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('D', DS)
def test_integer_rows_are_exact(gpu_ctx, D):
    Q, C, s, d = integer_case(D)
    full = D in (5, 49)                     # the whole product of the row counts at two widths, a cross elsewhere
    for nq in NQ if full else (1, 33, 257):
        for nc in NC if full else (1, 17, 64, 65, 257):
            rc, idx, dist2, st = search(gpu_ctx, Q[:nq], C[:nc])
            want = np.argmin(s[:nq, :nc], axis=1)
            assert rc == 0 and st == 0
            assert np.array_equal(idx, want), (nq, nc, D)
            assert np.array_equal(dist2, d[np.arange(nq), want].astype(np.float64)), (nq, nc, D)


# ---- 2. ties ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('splits', [0, 1, 3])
def test_the_lower_index_wins_a_tie(gpu_ctx, splits):
    nc = 200
    C = nn_cases.integer_rows(31, nc, 5)
    assert nn_cases.slice_length(nc, 3) == 128          # (127, 128): the last row of a forced slice and the next one
    for lo, hi in ((63, 64), (0, nc - 1), (127, 128)):
        Cd = C.copy()
        Cd[hi] = Cd[lo]
        assert len(np.unique(Cd, axis=0)) == nc - 1     # no other duplicate
        Q = np.vstack([Cd[lo], Cd[hi], Cd[5]])
        rc, idx, dist2, st = search(gpu_ctx, Q, Cd, splits)
        assert rc == 0 and st == 0
        assert idx.tolist() == [lo, lo, 5] and dist2.tolist() == [0.0, 0.0, 0.0]


# ---- 3. padding never wins ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('nc', [1, 17, 65])
@pytest.mark.parametrize('D', [1, 5, 49])
def test_padding_never_wins(gpu_ctx, nc, D):
    """q = 0 scores 0 against a zero row: every real candidate is non-zero, so a padded row or column that took part
    would win"""
    rs = np.random.RandomState(nc * 100 + D)
    C = rs.randint(2, 9, size=(nc, D)) * rs.choice([-1.0, 1.0], size=(nc, D))
    Q = np.zeros((3, D))
    for last in (False, True):
        if last:
            C[nc - 1] = 0.0
            C[nc - 1, D - 1] = 1.0                       # the least norm, at the last index
        want, want_d = nn_cases.nearest(Q, C)
        rc, idx, dist2, st = search(gpu_ctx, Q, C)
        assert rc == 0 and st == 0
        assert np.array_equal(idx, want) and np.array_equal(dist2, want_d.astype(np.float64))
        assert np.array_equal(idx, np.full(3, np.argmin((C * C).sum(axis=1))))
        if last:
            assert idx[0] == nc - 1 and dist2[0] == 1.0


# ---- 4. the slicing does not show ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('nc', [200, 65])
def test_results_do_not_depend_on_splits(gpu_ctx, nc):
    Q, C = nn_cases.normal_rows(41, 70, 49), nn_cases.normal_rows(42, nc, 49)
    _, idx1, d1, _ = search(gpu_ctx, Q, C, 1)
    assert np.array_equal(idx1, nn_cases.nearest(Q, C)[0])
    for splits in (2, 3, 7, 0):                          # 7 slices of 64 rows: empty ones behind the candidates
        rc, idx, d, st = search(gpu_ctx, Q, C, splits)
        assert rc == 0 and st == 0
        assert np.array_equal(idx, idx1) and np.array_equal(bits(d), bits(d1)), splits


# ---- 5. random doubles ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('D', [5, 49])
@pytest.mark.parametrize('offset, center', [(0.0, True), (0.0, False), (1e3, False)])
def test_random_rows_within_the_bound(gpu_ctx, D, offset, center):
    """d2(q, c_idx) - min_j d2(q, c_j) <= 4 (D + 1) u (|q|^2 + max_j |c_j|^2), u = 2^-53, for EVERY query: the score
    carries at most D u |c|^2 from the norm, D u (|q|^2 + |c|^2) from the product and one rounding of the difference,
    and two scores are compared.  dist2 is a direct sum: (D + 1) 2^-52 relative."""
    from kwiiyatta_amd.backend import nn
    Q, C = nn_cases.normal_rows(51, 257, D, offset), nn_cases.normal_rows(52, 300, D, offset)
    idx, dist2 = nn.nearest(Q, C, center=center, ctx=gpu_ctx)
    d = nn_cases.distances(Q, C)
    got = d[np.arange(len(Q)), idx]
    q2 = (np.asarray(Q, dtype=nn_cases.LD) ** 2).sum(axis=1)
    c2 = (np.asarray(C, dtype=nn_cases.LD) ** 2).sum(axis=1).max()
    bound = 4 * (D + 1) * U * (q2 + c2)
    excess = got - d.min(axis=1)
    print(f'D={D} offset={offset} center={center}: worst excess / bound = {float((excess / bound).max()):.3e}, '
          f'queries off the reference index = {int((idx != d.argmin(axis=1)).sum())}')
    assert (excess <= bound).all()
    rel = np.abs(dist2 - got) / got
    print(f'  worst dist2 error / ((D + 1) 2^-52) = {float(rel.max() / ((D + 1) * 2 * U)):.3e}')
    assert (rel <= (D + 1) * 2 * U).all()


# ---- 6. rows that are not finite ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rows_that_are_not_finite(gpu_ctx):
    Q, C = nn_cases.integer_rows(61, 40, 5), nn_cases.integer_rows(62, 70, 5)
    want, want_d = nn_cases.nearest(Q, C)
    Qn = Q.copy()
    Qn[17, 3] = np.nan
    rc, idx, dist2, st = search(gpu_ctx, Qn, C)
    assert rc == 0 and st == 1
    assert idx[17] == -1 and np.isnan(dist2[17])
    keep = np.arange(40) != 17                           # its neighbours are untouched
    assert np.array_equal(idx[keep], want[keep]) and np.array_equal(dist2[keep], want_d[keep].astype(np.float64))
    rc, idx, dist2, st = search(gpu_ctx, Qn, C, status=False)      # status may be NULL
    assert rc == 0 and idx[17] == -1

    Cn = C.copy()
    for j in set(want.tolist()[:6]):                     # the rows that used to win: NaN, +inf, -inf in turn
        Cn[j, j % 5] = (np.nan, np.inf, -np.inf)[j % 3]
    want, want_d = nn_cases.nearest(Q, Cn)
    rc, idx, dist2, st = search(gpu_ctx, Q, Cn, 3)
    assert rc == 0 and st == 0
    assert np.isfinite(Cn[idx]).all()
    assert np.array_equal(idx, want) and np.array_equal(dist2, want_d.astype(np.float64))

    rc, idx, dist2, st = search(gpu_ctx, Q[:3], np.full((2, 5), np.nan))   # no finite candidate at all
    assert rc == 0 and st == 3 and idx.tolist() == [-1] * 3 and np.isnan(dist2).all()


# ---- 7. entry forms and errors -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_form_equals_the_host_form(gpu_ctx):
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import nn
    Q, C = nn_cases.normal_rows(71, 300, 49), nn_cases.normal_rows(72, 500, 49)
    Q[5, 0] = np.nan
    _, idx, dist2, st = search(gpu_ctx, Q, C)
    dev = torch.device('cuda', gpu_ctx.device)
    dq, dc = torch.from_numpy(Q).to(dev), torch.from_numpy(C).to(dev)
    di = torch.full((300,), -7, dtype=torch.int32, device=dev)
    dd = torch.full((300,), -7.0, dtype=torch.float64, device=dev)
    ds = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for splits in (0, 5):
        nn.nearest_dev(gpu_ctx, dq, dc, di, dd, ds, splits=splits)
        gpu_ctx.sync()
        assert np.array_equal(di.cpu().numpy(), idx)
        assert np.array_equal(bits(dd.cpu().numpy()), bits(dist2))
        assert int(ds.item()) == st == 1
    with pytest.raises(ValueError, match='no finite score'):
        nn.check_status(ds)
    assert _lib.lib.kwy_nn_scratch_bytes(300, 0) >= _lib.lib.kwy_nn_scratch_bytes(300, 5) > 0


@pytest.mark.gpu
def test_bad_arguments_write_nothing(gpu_ctx):
    from kwiiyatta_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    Q, C = nn_cases.integer_rows(81, 4, 3), nn_cases.integer_rows(82, 6, 3)
    idx, dist2, st = np.full(4, -7, dtype=np.int32), np.full(4, -7.0), np.full(1, -7, dtype=np.int32)

    def call(q=Q, nq=4, c=C, nc=6, D=3, splits=0, i=idx, d=dist2):
        return lib.kwy_nn_search(gpu_ctx.handle, None if q is None else ptr(q), nq, None if c is None else ptr(c), nc, D,
                                 splits, None if i is None else ptr(i), None if d is None else ptr(d), ptr(st))

    wide = np.zeros((4, 161))
    bad = [dict(D=0), dict(q=wide, c=wide, nc=4, D=161), dict(nq=-1), dict(nc=0), dict(nc=-3), dict(splits=-1),
           dict(splits=65), dict(q=None), dict(c=None), dict(i=None), dict(d=None)]     # 65: KWY_NN_MAX_SPLITS + 1
    for kw in bad:
        assert call(**kw) == _lib.KWY_EINVAL, kw
        assert gpu_ctx.error().startswith('nn_search')
        assert (idx == -7).all() and (dist2 == -7.0).all() and st[0] == -7, kw
    assert call(nq=0) == 0 and call(nq=0, q=None, c=None, nc=0, i=None, d=None) == 0     # no queries: fine, nothing written
    assert (idx == -7).all() and (dist2 == -7.0).all() and st[0] == -7
    assert call() == 0 and st[0] == 0 and np.array_equal(idx, nn_cases.nearest(Q, C)[0])


def test_scratch_bytes_needs_no_device():
    from kwiiyatta_amd import _lib
    lib = _lib.lib
    assert lib.kwy_nn_scratch_bytes(0, 1) == 0 and lib.kwy_nn_scratch_bytes(-5, 1) == 0
    one = lib.kwy_nn_scratch_bytes(1000, 1)
    assert one >= 1000 * 12 and lib.kwy_nn_scratch_bytes(1000, 7) >= 7 * 1000 * 12
    assert lib.kwy_nn_scratch_bytes(1000, 0) == lib.kwy_nn_scratch_bytes(1000, 64) >= lib.kwy_nn_scratch_bytes(1000, 7)
    for nc in (1, 64, 65, 200, 10 ** 6):
        for splits in (1, 2, 3, 7, 64):
            assert lib.kwy_nn_slice(nc, splits) == nn_cases.slice_length(nc, splits)
    assert lib.kwy_nn_slice(0, 1) == 0 and lib.kwy_nn_slice(10, 0) == 0 and lib.kwy_nn_slice(10, 65) == 0
