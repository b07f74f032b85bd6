"""The numpy model of the exemplar converter's arithmetic (tests/nmf_cases.py) on its own: the properties the
contract in include/kwy.h states, and the host arithmetic of the converter's preparation.  No GPU."""
import numpy as np
import pytest

import nmf_cases as nc


@pytest.mark.parametrize('sparsity', [0.0, 0.1])
def test_objective_never_increases(sparsity):
    S, _, X = nc.make_case(65, 48, 20)
    H = nc.nmf_updates(S, X, 0, sparsity)
    last = nc.nmf_objective(S, X, H, sparsity)
    for n in range(60):
        H = nc.nmf_updates(S, X, 1, sparsity, h0=H)
        obj = nc.nmf_objective(S, X, H, sparsity)
        # the multiplicative update is a majorise-minimise step: monotone but for the rounding of a sum of size 1
        assert (obj <= last + 1e-14).all(), (n, (obj - last).max())
        last = obj


@pytest.mark.parametrize('dtype', [np.float64, np.longdouble])
def test_prefix_property(dtype):
    """the result after n updates does not depend on how many were asked for, and chains through h0 bit for bit"""
    S, _, X = nc.make_case(65, 48, 20)
    H7 = nc.nmf_updates(S, X, 7, 0.1, dtype=dtype)
    H = nc.nmf_updates(S, X, 4, 0.1, dtype=dtype)
    assert np.array_equal(nc.nmf_updates(S, X, 3, 0.1, h0=H, dtype=dtype), H7)
    assert H7.dtype == dtype


def fixed_point_case(B, A, T, seed=3):
    """W: at most three active atoms per frame, convex weights; X = W S has unit sums because the atoms have"""
    rng = np.random.default_rng(seed)
    S = nc.smooth_spectra(rng, A, B)
    W = np.zeros((T, A))
    for t in range(T):
        atoms = rng.choice(A, size=min(3, A), replace=False)
        w = rng.uniform(0.1, 1.0, size=len(atoms))
        W[t, atoms] = w / w.sum()
    return S, W, W @ S


def test_fixed_point():
    """lambda = 0, X = W S, h0 = W: G is 1 in exact arithmetic, so H stays W to within 8 N ulp"""
    N = 50
    S, W, X = fixed_point_case(65, 48, 20)
    H = nc.nmf_updates(S, X, N, 0.0, h0=W)
    assert (np.abs(H - W) <= 8 * N * np.spacing(W)).all()
    assert (H[W == 0] == 0).all()


def test_row_selection():
    assert nc.select_rows(5, 8).tolist() == [0, 1, 2, 3, 4]
    assert nc.select_rows(8, 8).tolist() == list(range(8))
    assert nc.select_rows(10, 4).tolist() == [0, 2, 5, 7]
    assert nc.select_rows(1809, 512).tolist() == [i * 1809 // 512 for i in range(512)]
    rows = nc.select_rows(1809, 512)
    assert len(set(rows.tolist())) == 512 and rows[0] == 0 and rows[-1] < 1809 and (np.diff(rows) > 0).all()


def test_unit_sum_preparation():
    rng = np.random.default_rng(0)
    rows = rng.uniform(1e-6, 3.0, size=(9, 129))
    u = nc.unit_sum(rows)
    assert np.allclose(u.sum(axis=1), 1.0, rtol=0, atol=4e-16 * 129)
    assert np.allclose(u * rows.sum(axis=1, keepdims=True), rows, rtol=1e-15, atol=0)
    S, Tg, X = nc.make_case(65, 48, 20)
    for m in (S, Tg, X):
        assert (m > 0).all() and np.isfinite(m).all()
        assert np.abs(m.sum(axis=1) - 1.0).max() < 1e-14


def test_every_other_frame_is_an_exact_mixture():
    S, _, X = nc.make_case(65, 48, 20)
    for t in range(0, 20, 2):
        w, res = np.linalg.lstsq(S.T, X[t], rcond=None)[:2]
        assert np.abs(w @ S - X[t]).max() < 1e-12
