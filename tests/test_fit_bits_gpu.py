"""The matrix-core kernels of the mixture fit and of k-means (kwy_gmmfit.hip, kwy_kmeans.hip) held to the bits of the
commit recorded in tests/golden/fit_bits_parent.npz (tools/record_fit_bits.py; inputs and calls: fit_cases.py, section
5): the E-step's responsibilities and log-likelihood parts, the sums and covariance statistics, the k-means labels and
changed counts -- at one, two, nine and ten column blocks, around the 16 / 32 / 256-row tiles and the 64-centre groups.
Bytes are compared: there is no tolerance.  test_fit_kernels_gpu.py holds the same kernels to longdouble references."""
import os

import numpy as np
import pytest

import fit_cases as fc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fit_bits_parent.npz')


@pytest.fixture(scope='module')
def ctx():
    from kwiiyatta_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _same(got, want, golden, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), f"{what}: differs from the build at {golden['commit']}"


def test_the_fixture_holds_every_case_and_nothing_else(golden):
    want = {'commit', 'km_labels_tie', 'km_changed_tie'}
    want |= {f'estep_{k}_{n}' for n in fc.BITS_ESTEP for k in ('resp', 'parts')}
    want |= {f'{k}_{n}' for n in fc.BITS_STATS for k in ('sums', 'cov_tril', 'cov_stats_sha256')}
    want |= {f'{k}_sha256_{n}' for n in fc.BITS_STATS_DIGEST for k in ('sums', 'cov', 'cov_stats')}
    want |= {f'km_{k}_{n}' for n in fc.BITS_KM for k in ('labels', 'changed')}
    assert set(golden.files) == want


@pytest.mark.parametrize('name', fc.BITS_ESTEP)
def test_estep_bits(name, ctx, golden):
    resp, parts, status = fc.bits_estep(ctx, name)
    assert status[0] == 0
    _same(resp, golden[f'estep_resp_{name}'], golden, f'{name} responsibilities')
    _same(parts, golden[f'estep_parts_{name}'], golden, f'{name} log-likelihood parts')


@pytest.mark.parametrize('name', fc.BITS_STATS + fc.BITS_STATS_DIGEST)
def test_sums_and_covariance_bits(name, ctx, golden):
    sums, cov, cov_stats = fc.bits_stats(ctx, name)
    if name in fc.BITS_STATS:
        _same(sums, golden[f'sums_{name}'], golden, f'{name} sums')
        _same(cov, fc.tril_unpack(golden[f'cov_tril_{name}'], cov.shape[1]), golden, f'{name} sxx')
    else:
        assert fc.digest(sums) == golden[f'sums_sha256_{name}'], f'{name} sums'
        assert fc.digest(cov) == golden[f'cov_sha256_{name}'], f'{name} sxx'
    assert fc.digest(cov_stats) == golden[f'cov_stats_sha256_{name}'], f'{name} sxx, sums given'


@pytest.mark.parametrize('name', fc.BITS_KM + ('tie',))
def test_kmeans_assignment_bits(name, ctx, golden):
    labels, changed = fc.bits_tie(ctx) if name == 'tie' else fc.bits_km(ctx, name)
    _same(labels, golden[f'km_labels_{name}'], golden, f'{name} labels')
    _same(changed, golden[f'km_changed_{name}'], golden, f'{name} changed counts')
