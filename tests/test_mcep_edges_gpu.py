"""kwy_sp2mc_dev and kwy_mc2sp_dev at their edges (kwiiyatta_amd/csrc/kwy_mcep.hip): every instance of k_sp2mc<LOG2N>,
k_sp2mc_dense and k_mc2sp_mfma across the orders, warps, lengths and frame counts of tests/mcep_cases.py, against the
float64 oracle that tests/test_mcep_cases.py holds to a long-double reference.

Every output lies between NaN guard rows, which must stay NaN.  Beyond parity: a row's result has the same bits
wherever it stands in a call and whatever its neighbours hold; the cached tables of one context give what a fresh
context gives; a refused call writes nothing.
"""
import numpy as np
import pytest

import mcep_cases as mcc
from mcep_cases import (DISTINCT, MC2SP_CASES, MC2SP_GRID_CASES, RANGE_CASE, SP2MC_DENSE_CASES, SP2MC_FALLBACK_CASES,
                        SP2MC_FFT_CASES, assert_mc_close, assert_sp_close, case_id, run_mc2sp, run_sp2mc, same_bits)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from kwiiyatta_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


# ------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('case', SP2MC_FFT_CASES, ids=case_id)
def test_sp2mc_fft_form(ctx, case):
    assert mcc.sp2mc_form(case.K, case.order, case.alpha) == 'fft'
    got = run_sp2mc(ctx, mcc.spectra(*case), case.order, case.alpha)
    assert_mc_close(got, mcc.sp2mc_oracle(case), f'k_sp2mc {case_id(case)}')


@pytest.mark.parametrize('case', SP2MC_DENSE_CASES, ids=case_id)
def test_sp2mc_dense_form(ctx, case):
    assert mcc.sp2mc_form(case.K, case.order, case.alpha) == 'dense'
    got = run_sp2mc(ctx, mcc.spectra(*case), case.order, case.alpha)
    assert_mc_close(got, mcc.sp2mc_oracle(case), f'k_sp2mc_dense {case_id(case)}')


@pytest.mark.parametrize('case', SP2MC_FALLBACK_CASES, ids=case_id)
def test_sp2mc_takes_the_warps_the_lds_has_no_room_for(ctx, case):
    """Power-of-two lengths whose cepstra (ncut of them per frame) do not fit beside the transform in LDS: the entry
    admitted them in its argument check and then refused them; now the dense form converts them, to the same bound.
    (The one-off host build of the largest, the 64 x 4097 matrix over 2682 cepstral indices, takes about a second.)"""
    from kwiiyatta_amd import _lib
    N = 2 * (case.K - 1)
    assert mcc.sp2mc_lds(N, mcc.ncut_of(N, case.order, case.alpha)) > mcc.LDS_MAX
    rc, got = run_sp2mc(ctx, mcc.spectra(*case), case.order, case.alpha, check=False)
    assert rc == _lib.KWY_OK, ctx.error()
    assert_mc_close(got, mcc.sp2mc_oracle(case), f'k_sp2mc_dense (fallback) {case_id(case)}')


@pytest.mark.parametrize('case', MC2SP_CASES, ids=case_id)
def test_mc2sp(ctx, case):
    got = run_mc2sp(ctx, mcc.mc2sp_input(case), case.alpha, 2 * (case.K - 1))
    assert_sp_close(got, mcc.mc2sp_oracle(case), f'k_mc2sp_mfma {case_id(case)}')


@pytest.mark.parametrize('case', MC2SP_GRID_CASES, ids=case_id)
def test_mc2sp_across_the_grid_switches(ctx, case):
    """T on both sides of the launch's gy switches (4 -> 2 at T = 4081, 2 -> 1 at 8177): DISTINCT rows tiled down the
    matrix; the first occurrences against the oracle, every repeat against its first occurrence bit for bit"""
    rows = mcc.mc2sp_input(case)
    assert len(rows) == DISTINCT
    got = run_mc2sp(ctx, mcc.tiled(rows, case.T), case.alpha, 2 * (case.K - 1))
    assert got.shape == (case.T, case.K)
    assert_sp_close(got[:DISTINCT], mcc.mc2sp_oracle(case), f'k_mc2sp_mfma {case_id(case)}')
    differ = np.flatnonzero((mcc.bits(got) != mcc.bits(mcc.tiled(got[:DISTINCT], case.T))).any(axis=1))
    assert differ.size == 0, f'{differ.size} repeated rows differ from their first occurrence, the first at {differ[0]}'


def test_mc2sp_range(ctx):
    """c0 puts the log-spectrum near +690 (finite), +720 (+inf exactly), -700 (normal, 1e-304) and -800 (exactly 0);
    against the long-double reference itself (four rows of 65 bins), whose exponent range holds all four"""
    got = run_mc2sp(ctx, mcc.mc2sp_input(RANGE_CASE), RANGE_CASE.alpha, 2 * (RANGE_CASE.K - 1))
    assert np.isposinf(got[1]).all() and (got[3] == 0).all()
    assert np.isfinite(got[0]).all() and (got[0] > 1e280).all()
    assert (got[2] >= np.finfo(np.float64).tiny).all() and (got[2] < 1e-290).all()
    assert_sp_close(got, mcc.mc2sp_long(RANGE_CASE), 'k_mc2sp_mfma range')


# --------------------------------------------------------------------------------------------- position independence
SP2MC_POSITIONS = (0, 1, 2, 3, 4)
MC2SP_POSITIONS = (0, 1, 2, 3, 4, 15, 16, 17)


@pytest.mark.parametrize('K,order,alpha', [(257, 24, 0.41), (257, 63, 0.9), (100, 40, 0.8), (17, 16, 0.41)])
def test_sp2mc_row_does_not_depend_on_its_position(ctx, K, order, alpha):
    """one spectrum at frames 0 ... 4 of calls of different lengths (first and last frame of a workgroup, alone in the
    last one): the same bits every time"""
    rows = mcc.spectra(K, order, alpha, 8, extra=1)
    probe, outs = rows[7], []
    for pos in SP2MC_POSITIONS:
        for T in (pos + 1, pos + 3):
            sp = np.ascontiguousarray(rows[:T])
            sp[pos] = probe
            outs.append(run_sp2mc(ctx, sp, order, alpha)[pos])
    assert np.isfinite(outs[0]).all()
    assert all(same_bits(o, outs[0]) for o in outs), 'a row of sp2mc depends on where it stands in the call'


@pytest.mark.parametrize('K,order,alpha', [(65, 3, 0.41), (65, 24, 0.41), (501, 63, 0.41), (17, 8, -0.9)])
def test_mc2sp_row_does_not_depend_on_its_position(ctx, ko, K, order, alpha):
    rows = mcc.mcep(ko, K, order, alpha, 21, extra=1)
    probe, outs = rows[20], []
    for pos in MC2SP_POSITIONS:
        for T in (pos + 1, pos + 3):
            mc = np.ascontiguousarray(rows[:T])
            mc[pos] = probe
            outs.append(run_mc2sp(ctx, mc, alpha, 2 * (K - 1))[pos])
    assert np.isfinite(outs[0]).all() and (outs[0] > 0).all()
    assert all(same_bits(o, outs[0]) for o in outs), 'a row of mc2sp depends on where it stands in the call'


# ------------------------------------------------------------------------------------------------------------ poison
@pytest.mark.parametrize('K,order,alpha', [(257, 24, 0.41), (100, 24, 0.41)], ids=['fft', 'dense'])
@pytest.mark.parametrize('poison', [0.0, float('nan'), float('inf')])
def test_sp2mc_poisoned_row_stays_alone(ctx, K, order, alpha, poison):
    """one bin of one spectrum is 0, NaN or inf: its coefficients are all non-finite, as the reference's are, and every
    other row -- the rows of its own workgroup too -- keeps the bits it has without the poison"""
    T, row = 9, 5
    sp = mcc.spectra(K, order, alpha, T, extra=2)
    clean = run_sp2mc(ctx, sp, order, alpha)
    bad = sp.copy()
    bad[row, K // 3] = poison
    assert not np.isfinite(mcc.sp2mc_ref(bad[row:row + 1], order, alpha)).any()
    got = run_sp2mc(ctx, bad, order, alpha)
    assert not np.isfinite(got[row]).any(), 'a poisoned spectrum gave finite coefficients'
    others = np.arange(T) != row
    assert np.isfinite(got[others]).all() and same_bits(got[others], clean[others])


@pytest.mark.parametrize('poison,at', [(float('nan'), 0), (float('nan'), 5), (float('inf'), 0)])
def test_mc2sp_poisoned_row_stays_alone(ctx, ko, poison, at):
    """one coefficient of one frame is NaN (c0, or one inside a k-step), or c0 is +inf: every bin of the frame is
    non-finite, as the reference's is, and the other 15 frames of its tile and those of the next keep their bits.
    (Not claimed: an inf in a coefficient above c0.  SPTK's recursion turns it into NaN in every bin; the dense sum
    gives each bin its own limit, exp(+-inf) = inf or 0 by the sign of the matrix entry.)"""
    K, order, alpha, T, row = 65, 24, 0.41, 19, 6
    mc = mcc.mcep(ko, K, order, alpha, T, extra=2)
    clean = run_mc2sp(ctx, mc, alpha, 2 * (K - 1))
    bad = mc.copy()
    bad[row, at] = poison
    assert not np.isfinite(np.asarray(mcc.mc2sp_ref(bad[row:row + 1], alpha, 2 * (K - 1)), np.float64)).any()
    got = run_mc2sp(ctx, bad, alpha, 2 * (K - 1))
    assert not np.isfinite(got[row]).any(), 'a poisoned frame gave finite bins'
    others = np.arange(T) != row
    assert np.isfinite(got[others]).all() and same_bits(got[others], clean[others])


# ------------------------------------------------------------------------------------------------------------ tables
TABLE_SETTINGS = ((24, 0.41), (25, 0.41), (24, float(np.nextafter(0.41, 1.0))), (24, -0.41))
TABLE_SEQUENCE = (0, 1, 2, 3, 2, 0, 3, 1)


@pytest.mark.parametrize('K', [257, 100], ids=['fft', 'dense'])
def test_cached_tables_are_keyed_by_order_and_alpha(K):
    """On one context, calls whose matrices differ in the order, in the last bit of alpha and in its sign, interleaved
    at one length: each equals the same call on a fresh context bit for bit (kwy_cached_table's keys, the ncut entry
    beside k_sp2mc's matrix, the process-wide host copies of the dense matrices)."""
    from kwiiyatta_amd import _lib
    from oracle import oracle as ko
    sp = mcc.spectra(K, 24, 0.41, 6, extra=3)
    mcs = [ko.sp2mc(sp, order, alpha) for order, alpha in TABLE_SETTINGS]
    shared = _lib.Context(0)
    seen_mc, seen_sp = {}, {}
    for k in TABLE_SEQUENCE:
        order, alpha = TABLE_SETTINGS[k]
        got_mc, got_sp = run_sp2mc(shared, sp, order, alpha), run_mc2sp(shared, mcs[k], alpha, 2 * (K - 1))
        assert k not in seen_mc or (same_bits(got_mc, seen_mc[k]) and same_bits(got_sp, seen_sp[k]))
        seen_mc[k], seen_sp[k] = got_mc, got_sp
    shared.close()
    for k, (order, alpha) in enumerate(TABLE_SETTINGS):
        fresh = _lib.Context(0)
        assert same_bits(run_sp2mc(fresh, sp, order, alpha), seen_mc[k]), f'sp2mc order {order} alpha {alpha!r}'
        assert same_bits(run_mc2sp(fresh, mcs[k], alpha, 2 * (K - 1)), seen_sp[k]), \
            f'mc2sp order {order} alpha {alpha!r}'
        fresh.close()
    # the settings are told apart: the last bit of alpha moves the result, the order adds a column
    assert not same_bits(seen_mc[0], seen_mc[2]) and not same_bits(seen_mc[0], seen_mc[3])
    assert seen_mc[1].shape[1] == seen_mc[0].shape[1] + 1


# ---------------------------------------------------------------------------------------------------------- refusals
# (K, order, alpha, T); tests/test_host_entries_gpu.py holds alpha = 1
REFUSALS = {
    'order above N / 2': (3, 3, 0.41, 2),
    'order 64': (257, 64, 0.41, 2),
    'order 0': (257, 0, 0.41, 2),
    'alpha -1': (257, 24, -1.0, 2),
    'alpha NaN': (257, 24, float('nan'), 2),
    'K 1': (1, 1, 0.41, 2),
    'K 4098': (4098, 24, 0.41, 2),
    'T 0': (257, 24, 0.41, 0),
}
SENTINEL = -1234.5


@pytest.mark.parametrize('dev', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('direction', ['sp2mc', 'mc2sp'])
@pytest.mark.parametrize('name', list(REFUSALS))
def test_refusals_write_nothing(ctx, name, direction, dev):
    import torch
    from kwiiyatta_amd import _lib
    K, order, alpha, T = REFUSALS[name]
    rows = max(T, 2)
    a = np.full((rows, max(K, 2)), 1e-3)                              # a spectrum
    b = np.full((rows, order + 1), 0.1)                               # coefficients
    src, dst = (a, b) if direction == 'sp2mc' else (b, a)
    out = np.full(dst.size + 128, SENTINEL)
    if dev:
        src_d, out_d = torch.from_numpy(src).cuda(), torch.from_numpy(out).cuda()
        p_in, p_out = src_d.data_ptr(), out_d.data_ptr() + 8 * 64
    else:
        p_in, p_out = src.ctypes.data, out.ctypes.data + 8 * 64
    fn = getattr(_lib.lib, f'kwy_{direction}' + ('_dev' if dev else ''))
    if direction == 'sp2mc':
        rc = fn(ctx.handle, p_in, T, K, order, alpha, p_out)
    else:
        rc = fn(ctx.handle, p_in, T, order, alpha, 2 * (K - 1), p_out)
    assert rc == _lib.KWY_EINVAL and ctx.error()
    ctx.sync()
    after = out_d.cpu().numpy() if dev else out
    assert (after == SENTINEL).all(), f'{name}: a refused call wrote to its output'
