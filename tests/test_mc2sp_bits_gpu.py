"""k_mc2sp_mfma gives a wavefront four neighbouring 16 x 16 products at a time and sends the results to memory a
row per store through LDS.  Every value is still the same exp of the same accumulator, summed over the same k-steps in
the same order (the library is built with -ffp-contract=off), so kwy_mc2sp_dev must equal, as bytes, what the build
before the change wrote: tests/golden/mc2sp_bits_parent.npz, recorded on an MI355X by tools/record_mc2sp_bits.py from
the inputs of tests/mc2sp_cases.py -- T in {1, 15, 16, 17, 33, 70} x fft sizes 512, 1024, 2048 x orders 24, 48, 63, each
into a buffer with NaN guard rows.  The fixture holds the SHA-256 of every case's bytes and three cases in full (those
say WHERE a build differs); the check against numpy's rfft keeps the equalities from being between two wrong spectra.
"""
import os

import numpy as np
import pytest

import mc2sp_cases as mc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mc2sp_bits_parent.npz')


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    assert int(g['seed']) == mc.SEED and len(str(g['commit'])) == 40
    assert g['names'].tolist() == [mc.key(*c) for c in mc.cases()] and len(g['names']) == 54
    return g, dict(zip(g['names'].tolist(), g['sha256'].tolist()))


@pytest.fixture(scope='module')
def ctx():
    from kwiiyatta_amd import _lib
    return _lib.Context(0)


@pytest.mark.parametrize('fft', mc.FFT_SIZES)
@pytest.mark.parametrize('order', mc.ORDERS)
def test_bits_of_the_parent_build(golden, ctx, fft, order):
    g, sha = golden
    for T in mc.FRAMES:
        got = mc.run(ctx, T, fft, order)
        assert got.shape == (T, fft // 2 + 1) and np.isfinite(got).all()
        name = mc.key(T, fft, order)
        if (T, fft, order) in mc.KEPT:
            bad = np.argwhere(got != g[name])
            assert bad.size == 0, (f'{name}: {len(bad)} values differ from the build at {g["commit"]}, '
                                   f'first (frame, bin) {bad[0]}')
        assert mc.digest(got) == sha[name], f'{name}: differs from the build at {g["commit"]}'


def test_kept_cases_are_spectra(golden):
    """the recorded arrays against the definition: exp(real(rfft(mirror(freqt(mc, -alpha) with c0 doubled))))"""
    from oracle import oracle
    g, _ = golden
    assert {c[1] for c in mc.KEPT} == set(mc.FFT_SIZES) and {c[2] for c in mc.KEPT} == set(mc.ORDERS)
    for T, fft, order in mc.KEPT:
        want = oracle.mc2sp(mc.mcep(T, fft, order), mc.ALPHA[fft], fft)
        got = g[mc.key(T, fft, order)]
        assert got.shape == want.shape
        assert np.abs(np.log(got) - np.log(want)).max() < 1e-9
