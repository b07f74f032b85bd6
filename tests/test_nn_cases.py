"""The numpy reference of the nearest-neighbour search (tests/nn_cases.py) against scipy's k-d tree, and its
conventions: ties to the lowest index, rows that are not finite.  No device."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import nn_cases


@pytest.mark.parametrize('nq, nc, D', [(1, 1, 1), (40, 70, 3), (257, 300, 8), (64, 129, 49)])
def test_reference_agrees_with_the_kd_tree(nq, nc, D):
    Q, C = nn_cases.normal_rows(11, nq, D), nn_cases.normal_rows(12, nc, D)
    idx, dist2 = nn_cases.nearest(Q, C)
    d_tree, i_tree = cKDTree(C).query(Q)
    assert np.array_equal(idx, i_tree)                    # random rows: the nearest is unique
    np.testing.assert_allclose(np.sqrt(dist2.astype(np.float64)), d_tree, rtol=1e-13, atol=0)


def test_direct_distances_match_the_scores():
    Q, C = nn_cases.integer_rows(3, 20, 5), nn_cases.integer_rows(4, 33, 5)
    d = nn_cases.distances(Q, C)
    s = nn_cases.scores(Q, C) + (Q * Q).sum(axis=1)[:, None]
    assert np.array_equal(d, s)                           # integers: both exact
    idx, dist2 = nn_cases.nearest(Q, C)
    assert np.array_equal(dist2, d.min(axis=1))
    assert np.array_equal(idx, d.argmin(axis=1))


def test_ties_go_to_the_lowest_index():
    C = nn_cases.integer_rows(5, 10, 4)
    C[7] = C[2]
    idx, dist2 = nn_cases.nearest(C[[7, 2]], C)
    assert idx.tolist() == [2, 2] and dist2.tolist() == [0, 0]


def test_rows_that_are_not_finite():
    Q, C = nn_cases.integer_rows(6, 4, 3), nn_cases.integer_rows(7, 6, 3)
    Q[1, 2] = np.nan
    C[0, 0] = np.nan
    C[3, 1] = np.inf
    idx, dist2 = nn_cases.nearest(Q, C)
    assert idx[1] == -1 and np.isnan(dist2[1])
    keep = [1, 2, 4, 5]
    ref, ref_d = nn_cases.nearest(Q[[0, 2, 3]], C[keep])
    assert idx[[0, 2, 3]].tolist() == [keep[j] for j in ref]
    assert np.array_equal(dist2[[0, 2, 3]], ref_d)


def test_slice_length():
    assert [nn_cases.slice_length(200, s) for s in (1, 2, 3, 7)] == [256, 128, 128, 64]
    assert [nn_cases.slice_length(65, s) for s in (1, 2, 3, 7)] == [128, 64, 64, 64]
