"""k_stretch_log at the edges of its tiling: a workgroup stages R = min(8, 8192 / span) rows of `span` inputs in LDS,
and span grows with the ratio of the bin counts -- pairs that leave 7, 3 and 1 rows per workgroup with a row count off
the tile, a pair whose span no longer fits (refused), and bin counts of a few bins, where the whole row is edge
replication.

Checker: ko.stretch_log (the reference's call chain on scipy.signal.resample_poly), on the rows of
test_backends_gpu.test_stretch_log_matches_resample_poly and within its bound, |got / want - 1| <= 1e-12."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUND = 1e-12
ST_COLS, ST_MAX_ROWS, ST_LDS_DOUBLES = 256, 8, 8192          # kwy_stretch.hip


def tiling(bins, new_bins):
    """-> (span, rows per workgroup) of stretch_make_plan"""
    g = math.gcd(bins, new_bins)
    up, down = new_bins // g, bins // g
    numtaps = 20 * max(up, down) + 1
    span = ((ST_COLS - 1) * down + numtaps) // up + 3
    return span, min(ST_MAX_ROWS, ST_LDS_DOUBLES // span)


def _rows(T, bins, new_bins):
    rng = np.random.default_rng([T, bins, new_bins])
    return np.exp(np.cumsum(rng.standard_normal((T, bins)), axis=1) * 0.35 + rng.uniform(-8, 2, (T, 1)))


def _check(T, bins, new_bins):
    from oracle import oracle as ko
    from kwiiyatta_amd.backend import resample
    rows = _rows(T, bins, new_bins)
    got, want = resample.stretch_log(rows, new_bins), ko.stretch_log(rows, new_bins)
    assert got.shape == want.shape == (T, new_bins)
    err = np.abs(got / want - 1).max()
    print(f'stretch {bins} -> {new_bins}, T={T}: max |got / want - 1| = {err:.3e}')
    assert err <= BOUND, err


@pytest.mark.parametrize('bins,new_bins,per_group,T', [(2049, 513, 7, 8), (4097, 513, 3, 4), (8193, 513, 1, 2),
                                                      (2049, 513, 7, 1), (4097, 513, 3, 1), (8193, 513, 1, 1)])
def test_fewer_than_eight_rows_per_workgroup(bins, new_bins, per_group, T):
    assert tiling(bins, new_bins)[1] == per_group and (T == 1 or T == per_group + 1)
    _check(T, bins, new_bins)


@pytest.mark.parametrize('bins,new_bins', [(2, 3), (3, 2), (1, 2), (5, 1)])
def test_small_bin_counts(bins, new_bins):
    _check(3, bins, new_bins)


def test_span_beyond_lds_is_refused_and_the_context_goes_on():
    from oracle import oracle as ko
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, ptr
    from kwiiyatta_amd.backend import resample
    bins, new_bins, T = 8193, 257, 2
    assert tiling(bins, new_bins)[0] > ST_LDS_DOUBLES > tiling(8193, 513)[0]
    ctx = _lib.Context(0)
    rows = _rows(T, bins, new_bins)
    out = np.full((T, new_bins), np.nan)
    rc = lib.kwy_stretch_log(ctx.handle, ptr(rows), T, bins, new_bins, ptr(out))
    assert rc == _lib.KWY_EINVAL and 'ratio of bin counts too large' in ctx.error()
    assert np.isnan(out).all()
    rows = _rows(3, 65, 129)
    got = resample.stretch_log(rows, 129, ctx=ctx)
    assert np.abs(got / ko.stretch_log(rows, 129) - 1).max() <= BOUND
