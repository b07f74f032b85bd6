"""CPU checks of tests/mcep_cases.py, the yardstick of tests/test_mcep_edges_gpu.py.

Seams: the case table has a case on each side of every seam of kwy_mcep.hip it claims to cross (frames per workgroup,
bins per product and per wavefront step, coefficients per k-step, the grid's gy switches, the cut of the freqt matrix,
the LDS limit of k_sp2mc), worked out from constants copied from the source.

References: the float64 oracle the GPU tests compare with lies within ORACLE_MC_REL of max |ref| (sp2mc) and
ORACLE_SP_LOG in log (mc2sp) of the long-double reference on every case; a relative 1e-16 on the inputs moves the
reference by less than a tenth of the bound in force.

Sensitivity: six wrong kernels, restated as options of the long-double reference, each fail assert_mc_close /
assert_sp_close on a case of the table -- the sp2mc ones in the FFT form's cases and in the dense form's.  A later
loosening of MC_REL / SP_LOG, or the loss of the cases that tell them apart, fails here without a GPU.
"""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (conftest puts the repository root on sys.path)
import mcep_cases as mcc
from mcep_cases import (DISTINCT, FFT_KS, GY_SWITCHES, LD, LDS_MAX, MC2SP_CASES, MC2SP_GRID_CASES, MC2SP_MUTANTS, MC_FR,
                        MCD_FR, RANGE_CASE, RANGE_TARGETS, SP2MC_DENSE_CASES, SP2MC_FALLBACK_CASES, SP2MC_FFT_CASES,
                        SP2MC_MUTANTS, Case, assert_mc_close, assert_sp_close, case_id, mc2sp_gy, ncut_of, sp2mc_form,
                        sp2mc_lds)

SP2MC_ALL = SP2MC_FFT_CASES + SP2MC_FALLBACK_CASES + SP2MC_DENSE_CASES
MC2SP_ALL = MC2SP_CASES + MC2SP_GRID_CASES         # (RANGE_CASE is compared with the long-double reference itself)


def test_bounds_are_within_the_projects_caps():
    assert 0 < mcc.MC_REL <= mcc.MC_CAP == 1e-12
    assert 0 < mcc.SP_LOG <= mcc.SP_CAP == 1e-11
    assert mcc.SP_LOG_SCALE == 15.0
    # 8 x the measured worst of each kernel (the comment table of mcep_cases.py), two orders below the caps
    assert mcc.MC_REL == 8 * 1.376e-15 and mcc.SP_LOG == 8 * 1.483e-14


def test_lds_table():
    """the four rows of the LDS table: the largest setting k_sp2mc has room for, and three it has not"""
    rows = [(4096, 63, 0.90, 2682, 130896, True), (4096, 63, 0.95, 4096, 176144, False),
            (8192, 63, 0.90, 2682, 167760, False), (8192, 24, 0.97, 5793, 267312, False)]
    for N, order, alpha, ncut, lds, fits in rows:
        assert ncut_of(N, order, alpha) == ncut
        assert sp2mc_lds(N, ncut) == lds
        assert (lds <= LDS_MAX) == fits
        assert sp2mc_form(N // 2 + 1, order, alpha) == ('fft' if fits else 'dense')
    # "the largest that does": one more order or the next alpha of the table does not fit at N = 4096, order 63
    assert sp2mc_lds(4096, ncut_of(4096, 63, 0.91)) > sp2mc_lds(4096, 2682)
    # the dense form has room for every length the entry takes
    assert mcc.sp2mc_dense_lds(mcc.K_MAX) == 139296 <= LDS_MAX


def test_sp2mc_cases_cross_every_seam():
    fft, dense, fb = set(SP2MC_FFT_CASES), set(SP2MC_DENSE_CASES), set(SP2MC_FALLBACK_CASES)
    assert len(fft) == len(SP2MC_FFT_CASES) and len(dense) == len(SP2MC_DENSE_CASES)
    assert all(sp2mc_form(c.K, c.order, c.alpha) == 'fft' for c in fft)
    assert all(sp2mc_form(c.K, c.order, c.alpha) == 'dense' for c in dense | fb)
    assert all(2 * (c.K - 1) in (4096, 8192) for c in fb)           # power-of-two lengths that leave the FFT form
    assert {c for c in fb} == {Case(2049, 63, 0.95, 5), Case(4097, 63, 0.9, 5), Case(4097, 24, 0.97, 5)}
    # every instance of k_sp2mc, each with a last workgroup of one frame
    assert tuple(sorted({c.K for c in fft})) == FFT_KS == tuple((1 << l) // 2 + 1 for l in mcc.FFT_LOG2)
    for K in FFT_KS:
        assert Case(K, 24, 0.41, 5) in fft and 5 % MC_FR == 1
    assert Case(4097, 63, 0.77, 5) in fft and ncut_of(8192, 63, 0.77) == 1084
    # frames: below, on and above one and two workgroups
    Ts = {c.T for c in fft if (c.K, c.order, c.alpha) == (257, 24, 0.41)}
    assert Ts == {1, 3, 4, 5, 8, 9}
    assert {MC_FR - 1, MC_FR, MC_FR + 1, 2 * MC_FR, 2 * MC_FR + 1} <= Ts
    # orders: the smallest, around one k of the four strided sums, the largest two
    assert {c.order for c in fft if (c.K, c.alpha, c.T) == (257, 0.41, 5)} >= {1, 2, 3, 4, 24, 62, 63}
    assert mcc.MC_MAX_ORDER == 63
    # alpha at order 63: the matrix keeps all N columns and the mirrored half is read; alpha = 0 keeps order + 1
    alphas = {c.alpha for c in fft if (c.K, c.order, c.T) == (257, 63, 5)}
    assert alphas >= {0.0, -0.41, 0.41, 0.77, 0.9, 0.95, -0.9}
    for a in (0.77, 0.9, 0.95, -0.9):
        assert ncut_of(512, 63, a) == 512
    assert ncut_of(512, 24, 0.41) < 256                              # the typical setting never reads the mirrored half
    assert ncut_of(512, 63, 0.0) == 64
    assert Case(257, 1, 0.0, 5) in fft and ncut_of(512, 1, 0.0) == 2 < mcc.MC_PARTS   # strides 2 and 3 have no term
    # the LDS edge
    edge = Case(2049, 63, 0.9, 5)
    assert edge in fft and sp2mc_lds(4096, ncut_of(4096, 63, 0.9)) <= LDS_MAX
    assert all(sp2mc_lds(2 * (c.K - 1), ncut_of(2 * (c.K - 1), c.order, c.alpha)) > LDS_MAX for c in fb)
    # the dense form: lengths, the largest order a length admits, frames around one workgroup
    assert {c.K for c in dense} == {2, 3, 4, 17, 100, 372, 4096}
    for K in (2, 3, 4, 17):
        assert any(c.K == K and c.order == K - 1 for c in dense)     # order = N / 2
    assert Case(4096, 24, 0.41, 5) in dense and 4096 < mcc.K_MAX
    Ts = {c.T for c in dense if (c.K, c.order, c.alpha) == (100, 24, 0.41)}
    assert Ts == {1, 3, 4, 5} and {MCD_FR - 1, MCD_FR, MCD_FR + 1} <= Ts
    assert {c.alpha for c in dense if (c.K, c.order) == (100, 40)} == {0.0, -0.41, 0.8}
    assert ncut_of(198, 40, 0.8) == 198


def test_mc2sp_cases_cross_every_seam():
    cases = set(MC2SP_CASES)
    assert len(cases) == len(MC2SP_CASES)
    Ks = {c.K for c in cases if c.T == 17 and c.alpha == 0.41 and c.order == min(24, c.K - 1)}
    assert Ks == set(mcc.MC2SP_KS) == {2, 3, 16, 17, 63, 64, 65, 501, 2049, 4097}
    tile, group = mcc.MC2_TILE_BINS, mcc.MC2_TILE_BINS * mcc.MC2_TILES
    assert (tile, group) == (16, 64)
    assert {tile, tile + 1, group - 1, group, group + 1} <= Ks and min(Ks) < tile
    assert any(K % tile not in (0, 1) and K > group for K in Ks)     # 501: a last product of 5 bins
    ngroup = lambda K: -(-(-(-K // tile)) // mcc.MC2_TILES)          # noqa: E731
    assert ngroup(65) == 2 and ngroup(1025) == 17 and ngroup(4097) == 65
    # orders: order + 1 coefficients in k-steps of 4: exactly one, one over, two, one over, seven of 16, all 16
    n = {c.order + 1 for c in cases if (c.K, c.T, c.alpha) == (65, 17, 0.41)}
    assert n == {2, 3, 4, 5, 8, 9, 25, 64}
    assert {mcc.MC2_KSTEP, mcc.MC2_KSTEP + 1, 2 * mcc.MC2_KSTEP, 2 * mcc.MC2_KSTEP + 1, mcc.MC_MAX_ORDER + 1} <= n
    # frames around one and two tiles of 16
    Ts = {c.T for c in cases if (c.K, c.order, c.alpha) == (65, 3, 0.41)}
    F = mcc.MC2_FRAMES
    assert Ts == {1, 15, 16, 17, 33} and {F - 1, F, F + 1, 2 * F + 1} <= Ts
    assert {c.alpha for c in cases if (c.K, c.order, c.T) == (17, 8, 17)} == {0.0, 0.41, -0.41, 0.9, -0.9}
    # the grid: both sides of both switches, and the long trip count at gy = 1
    assert GY_SWITCHES == (4081, 8177)
    for s, (before, after) in zip(GY_SWITCHES, ((4, 2), (2, 1))):
        assert mc2sp_gy(s - 1) == before and mc2sp_gy(s) == after
        assert Case(65, 24, 0.41, s - 1) in MC2SP_GRID_CASES and Case(65, 24, 0.41, s) in MC2SP_GRID_CASES
    assert Case(1025, 24, 0.41, 8177) in MC2SP_GRID_CASES
    assert ngroup(65) < mcc.KWY_WAVES                                # two wavefronts idle
    trips = [len(range(w, ngroup(1025), mc2sp_gy(8177) * mcc.KWY_WAVES)) for w in range(mcc.KWY_WAVES)]
    assert trips == [5, 4, 4, 4]
    assert DISTINCT == 37 and DISTINCT % F                          # a repeat never starts a tile where its first did
    assert all(s % F == 1 for s in GY_SWITCHES)                      # one frame in the last tile just past a switch


def test_range_rows_are_unambiguous():
    """each row of RANGE_CASE lies in one class, well away from the thresholds of a double (709.78, -708.40, -745.13)"""
    ref = mcc.mc2sp_long(RANGE_CASE)
    log = np.log(ref)
    want = {690.0: (660.0, 705.0), 720.0: (712.0, 760.0), -700.0: (-706.0, -680.0), -800.0: (-840.0, -750.0)}
    over, under = mcc.range_class(ref)
    for row, target in enumerate(RANGE_TARGETS):
        lo, hi = want[target]
        assert lo < log[row].min() and log[row].max() < hi, (target, float(log[row].min()), float(log[row].max()))
        assert over[row].all() == (target == 720.0) and over[row].any() == (target == 720.0)
        assert under[row].all() == (target == -800.0) and under[row].any() == (target == -800.0)
    # the oracle agrees on the classes
    got = mcc.mc2sp_oracle(RANGE_CASE)
    assert np.isposinf(got[1]).all() and (got[3] == 0).all()
    assert np.isfinite(got[0]).all() and (got[2] > 1e-307).all() and (got[2] < 1e-290).all()


# ---- the oracle has to earn its place ------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SP2MC_ALL, ids=case_id)
def test_oracle_sp2mc_is_the_long_double_reference(case):
    """... and the reference is well conditioned: a relative 1e-16 on every input bin moves it by less than a tenth of
    MC_REL"""
    ref = mcc.sp2mc_long(case)
    assert ref.dtype == LD and ref.shape == (case.T, case.order + 1) and np.isfinite(ref).all()
    e = assert_mc_close(mcc.sp2mc_oracle(case), ref, f'oracle sp2mc {case_id(case)}', mcc.ORACLE_MC_REL)
    assert e <= mcc.ORACLE_MC_REL
    sp = mcc.spectra(*case)
    rng = np.random.default_rng(mcc._seed(*case[:3], 99))
    moved = mcc.sp2mc_ref(sp.astype(LD) * (1 + LD(1e-16) * rng.choice([-1.0, 1.0], sp.shape)), case.order, case.alpha)
    m = mcc.mc_error(moved, ref)
    print(f'a relative 1e-16 on the spectrum moves the reference by {m:.3e} of max |ref|')
    assert 0 < m <= mcc.MC_REL / 10


@pytest.mark.parametrize('case', MC2SP_ALL, ids=case_id)
def test_oracle_mc2sp_is_the_long_double_reference(case):
    ref = mcc.mc2sp_long(case)
    rows = min(case.T, DISTINCT)
    assert ref.dtype == LD and ref.shape == (rows, case.K)
    e = assert_sp_close(mcc.mc2sp_oracle(case), ref, f'oracle mc2sp {case_id(case)}', mcc.ORACLE_SP_LOG)
    assert e <= mcc.ORACLE_SP_LOG
    mc = mcc.mc2sp_input(case)
    rng = np.random.default_rng(mcc._seed(*case[:3], 98))
    moved = mcc.mc2sp_ref(mc.astype(LD) * (1 + LD(1e-16) * rng.choice([-1.0, 1.0], mc.shape)), case.alpha,
                          2 * (case.K - 1))
    live = ~np.logical_or(*mcc.range_class(ref))
    m = float(np.abs(np.log(moved[live]) - np.log(ref[live])).max()) if live.any() else 0.0
    scale = max(1.0, float(np.abs(np.log(ref[live])).max()) / mcc.SP_LOG_SCALE) if live.any() else 1.0
    print(f'a relative 1e-16 on the coefficients moves the reference by {m:.3e} in log (scale {scale:.3g})')
    assert m <= mcc.SP_LOG * scale / 10


# ---- the assertions have to reject wrong kernels -------------------------------------------------------------------
def _cheap_first(cases):
    return sorted(cases, key=lambda c: c.K * (c.order + 1) * min(c.T, DISTINCT))


@pytest.mark.parametrize('form', ['fft', 'dense'])
@pytest.mark.parametrize('mutant', SP2MC_MUTANTS)
def test_mc_bound_rejects_wrong_kernels(mutant, form):
    """A kernel that warps only c[0 .. N/2], that weights the Nyquist bin 2, or that leaves c[0] whole, fails
    assert_mc_close against the oracle on a case of the FFT form's table and on one of the dense form's."""
    rejected = []
    for case in _cheap_first(SP2MC_FFT_CASES if form == 'fft' else SP2MC_DENSE_CASES):
        if case.K > 1025:
            continue
        got = np.asarray(mcc.sp2mc_long(case, mutant), np.float64)
        try:
            assert_mc_close(got, mcc.sp2mc_oracle(case), f'{mutant} / {case_id(case)}')
        except AssertionError:
            rejected.append(case)
    print(f'"{mutant}" ({form}) rejected on {[case_id(c) for c in rejected]}')
    assert rejected, f'no {form} case tells "{mutant}" from the oracle within MC_REL'
    if mutant == 'half only':
        # seen only where the matrix reads the mirrored half, and there by far: 1e-2 ... 1e-1 of the result
        assert all(ncut_of(2 * (c.K - 1), c.order, c.alpha) > c.K for c in rejected)
        worst = max(mcc.mc_error(mcc.sp2mc_long(c, mutant), mcc.sp2mc_long(c)) for c in rejected)
        assert worst > 1e-2


@pytest.mark.parametrize('mutant', MC2SP_MUTANTS)
def test_sp_bound_rejects_wrong_kernels(mutant):
    """A kernel that weights c[H] 2, whose last bin repeats bin K - 2, or that computes the last frame of a partial
    16-frame tile from zeros, fails assert_sp_close against the oracle on a case of the table."""
    rejected = []
    for case in _cheap_first(MC2SP_CASES):
        if case.K > 501:
            continue
        with np.errstate(all='ignore'):
            got = np.asarray(mcc.mc2sp_long(case, mutant), np.float64)
        try:
            assert_sp_close(got, mcc.mc2sp_oracle(case), f'{mutant} / {case_id(case)}')
        except AssertionError:
            rejected.append(case)
    print(f'"{mutant}" rejected on {[case_id(c) for c in rejected]}')
    assert rejected, f'no case tells "{mutant}" from the oracle within SP_LOG'
    if mutant == 'partial tile from zeros':
        assert all(c.T % 16 for c in rejected) and Case(65, 3, 0.41, 16) not in rejected
    if mutant == 'c[H] twice':
        assert any(c.K == 17 and c.order == 8 for c in rejected)     # where c[H] is not negligible


def test_the_unmutated_reference_passes():
    """the helpers accept the long-double reference rounded to double, on the cases the mutants are tried on"""
    for case in (Case(257, 63, 0.9, 5), Case(100, 40, 0.8, 5)):
        assert_mc_close(np.asarray(mcc.sp2mc_long(case), np.float64), mcc.sp2mc_oracle(case), case_id(case))
    for case in (Case(17, 8, 0.9, 17), Case(65, 3, 0.41, 17), RANGE_CASE):
        with np.errstate(over='ignore'):                             # (the +720 row overflows a double, as it should)
            got = np.asarray(mcc.mc2sp_long(case), np.float64)
        assert_sp_close(got, mcc.mc2sp_oracle(case), case_id(case))
