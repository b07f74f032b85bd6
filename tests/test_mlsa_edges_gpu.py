"""k_mlsa_filter at the seams of its maps (tests/mlsa_cases.py; the inputs are checked on the CPU in
test_mlsa_cases.py): hop sizes around the 64-sample staging stride and at MLSA_MAX_HOP, orders on both sides of every
eight-link block, every position of the signal's end against the frame grid, constant coefficients and all-pass
constants of either sign, the batched entry on ragged jobs, and the argument refusals of the host and device entries.

Checker: the CPU oracle (ko.mc2b, ko.mlsa_synthesis).  Bound: max |got - ref| <= 1e-11 max |ref|, the bound this
kernel has in test_mlsa_codec.py -- the kernel keeps SPTK's order of operations, only exp() differs from libm's in the
last bit.  Behind the last filtered frame the output is exactly zero.  Every case prints its measured ratio."""
import numpy as np
import pytest

import mlsa_cases as mc

pytestmark = pytest.mark.gpu


def _hip(case, x, b):
    from kwiiyatta_amd.backend import sptk
    return sptk.Synthesizer(sptk.MLSADF(order=case.order, alpha=case.alpha, pd=case.pd), hopsize=case.hop).synthesis(x, b)


def _check(case):
    x, _, b, ref = mc.reference(case)
    got = _hip(case, x, b)
    ratio = mc.deviation(got, ref)
    print(f'mlsa {case.name}: max |got - ref| / max |ref| = {ratio:.3e}')
    assert got.shape == ref.shape
    assert np.all(got[mc.nproc(case) * case.hop:] == 0.0), case.name
    assert ratio <= mc.BOUND, (case.name, ratio)


@pytest.mark.parametrize('case', mc.HOP_CASES, ids=lambda c: c.name)
def test_hop_seams(case):
    _check(case)


@pytest.mark.parametrize('case', mc.ORDER_CASES, ids=lambda c: c.name)
def test_order_seams(case):
    _check(case)


@pytest.mark.parametrize('case', mc.GRID_CASES, ids=lambda c: c.name)
def test_signal_end_against_the_frame_grid(case):
    _check(case)


@pytest.mark.parametrize('case', mc.COEF_CASES, ids=lambda c: c.name)
def test_constant_coefficients_and_allpass_constants(case):
    _check(case)


def test_mc2b_keeps_c0():
    """the coefficients the filter cases run on: kwy_mc2b against the oracle's, c0 included"""
    from oracle import oracle as ko
    from kwiiyatta_amd.backend import sptk
    for case in mc.COEF_CASES + mc.ORDER_CASES[::2]:
        _, mcep = mc.inputs(case)
        assert np.abs(sptk.mc2b(mcep, case.alpha) - ko.mc2b(mcep, case.alpha)).max() <= 1e-15, case.name


@pytest.mark.parametrize('ignore_c0', [0, 1])
def test_batch_entry_on_ragged_jobs(ignore_c0):
    """one kwy_mlsa_filter_batch_dev call, one job without a filtered frame: every job equals kwy_mc2b_dev +
    kwy_mlsa_synthesis_dev bit for bit and the oracle (column 0 zeroed for ignore_c0) within the bound"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, c_vp
    ctx = _lib.Context(0)
    first = mc.BATCH_JOBS[0]
    refs = [mc.reference(c, bool(ignore_c0)) for c in mc.BATCH_JOBS]
    dev = [(torch.from_numpy(x).cuda(), torch.from_numpy(mcep).cuda(),
            torch.full((c.n,), float('nan'), dtype=torch.float64, device='cuda'))
           for c, (x, mcep, _, _) in zip(mc.BATCH_JOBS, refs)]
    torch.cuda.synchronize()
    arr = _lib.job_array(_lib.MlsaJob, [(x, c.n, m, c.T, y) for c, (x, m, y) in zip(mc.BATCH_JOBS, dev)])
    _lib.check(ctx, lib.kwy_mlsa_filter_batch_dev(ctx.handle, arr, len(dev), first.order, first.alpha, first.pd,
                                                  first.hop, ignore_c0))
    ctx.sync()
    for c, (x, m, y), (_, _, _, ref) in zip(mc.BATCH_JOBS, dev, refs):
        m2 = m.clone()
        if ignore_c0:
            m2[:, 0] = 0.0
        b, y1 = torch.empty_like(m2), torch.full_like(y, float('nan'))
        torch.cuda.synchronize()
        _lib.check(ctx, lib.kwy_mc2b_dev(ctx.handle, c_vp(m2.data_ptr()), c.T, c.order, c.alpha, c_vp(b.data_ptr())))
        _lib.check(ctx, lib.kwy_mlsa_synthesis_dev(ctx.handle, c_vp(x.data_ptr()), c.n, c_vp(b.data_ptr()), c.T, c.order,
                                                   c.alpha, c.pd, c.hop, c_vp(y1.data_ptr())))
        ctx.sync()
        assert torch.equal(y, y1), c.name
        got = y.cpu().numpy()
        ratio = mc.deviation(got, ref)
        print(f'mlsa batch ignore_c0={ignore_c0} {c.name}: max |got - ref| / max |ref| = {ratio:.3e}')
        assert np.all(got[mc.nproc(c) * c.hop:] == 0.0), c.name
        assert ratio <= mc.BOUND, (c.name, ratio)


MLSA_JOBS_MAX = 64           # signals per launch (kwy_mlsa.hip)


def test_batch_entry_on_one_job_more_than_a_launch_holds():
    """one kwy_mlsa_filter_batch_dev call on MLSA_JOBS_MAX + 1 signals of a few dozen samples and unequal length (the
    entry takes no empty signal): every job equals kwy_mc2b_dev + kwy_mlsa_synthesis_dev bit for bit"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, c_vp
    ctx = _lib.Context(0)
    order, alpha, pd, hop = 5, 0.41, 5, 8
    rng = np.random.default_rng(7)
    shapes = [(20 + 7 * i % 41, 1 + i % 5) for i in range(MLSA_JOBS_MAX + 1)]        # (samples, frames)
    dev = [(torch.from_numpy(rng.standard_normal(n) * 0.1).cuda(),
            torch.from_numpy(rng.standard_normal((T, order + 1)) * 0.05).cuda(),
            torch.full((n,), float('nan'), dtype=torch.float64, device='cuda')) for n, T in shapes]
    torch.cuda.synchronize()
    arr = _lib.job_array(_lib.MlsaJob, [(x, n, m, T, y) for (n, T), (x, m, y) in zip(shapes, dev)])
    _lib.check(ctx, lib.kwy_mlsa_filter_batch_dev(ctx.handle, arr, len(dev), order, alpha, pd, hop, 0))
    ctx.sync()
    for i, ((n, T), (x, m, y)) in enumerate(zip(shapes, dev)):
        b, y1 = torch.empty_like(m), torch.full_like(y, float('nan'))
        torch.cuda.synchronize()
        _lib.check(ctx, lib.kwy_mc2b_dev(ctx.handle, c_vp(m.data_ptr()), T, order, alpha, c_vp(b.data_ptr())))
        _lib.check(ctx, lib.kwy_mlsa_synthesis_dev(ctx.handle, c_vp(x.data_ptr()), n, c_vp(b.data_ptr()), T, order, alpha,
                                                   pd, hop, c_vp(y1.data_ptr())))
        ctx.sync()
        assert not bool(torch.isnan(y).any()) and torch.equal(y, y1), i


@pytest.mark.parametrize('name,change', mc.REFUSALS, ids=[name for name, _ in mc.REFUSALS])
def test_refusals_leave_the_output_untouched(name, change):
    """KWY_EINVAL from the host entry and from the device entry, nothing written"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, c_vp, ptr
    ctx = _lib.Context(0)
    a = dict(mc.GOOD, **change)
    rng = np.random.default_rng(1)
    # buffers as large as the largest claim made about them, so that an entry that went ahead would stay in bounds
    x = rng.standard_normal(mc.GOOD['n']) * 0.1
    b = rng.standard_normal((mc.GOOD['T'], mc.MLSA_MAX_ORDER + 2)) * 0.01
    y = np.full(mc.GOOD['n'], np.nan)
    rc = lib.kwy_mlsa_synthesis(ctx.handle, ptr(x), a['n'], ptr(b), a['T'], a['order'], a['alpha'], a['pd'], a['hop'], ptr(y))
    assert rc == _lib.KWY_EINVAL and 'mlsa_synthesis' in ctx.error(), name
    assert np.isnan(y).all(), name
    dx, db = torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda()
    dy = torch.full((mc.GOOD['n'],), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    rc = lib.kwy_mlsa_synthesis_dev(ctx.handle, c_vp(dx.data_ptr()), a['n'], c_vp(db.data_ptr()), a['T'], a['order'],
                                    a['alpha'], a['pd'], a['hop'], c_vp(dy.data_ptr()))
    ctx.sync()
    assert rc == _lib.KWY_EINVAL, name
    assert bool(torch.isnan(dy).all()), name
    # the context still works: the good call right behind the refusal
    g = mc.GOOD
    good = np.empty(g['n'])
    bg = np.ascontiguousarray(b[:, :g['order'] + 1])
    _lib.check(ctx, lib.kwy_mlsa_synthesis(ctx.handle, ptr(x), g['n'], ptr(bg), g['T'], g['order'], g['alpha'], g['pd'],
                                           g['hop'], ptr(good)))
    from oracle import oracle as ko
    assert mc.deviation(good, ko.mlsa_synthesis(x, bg, g['alpha'], g['hop'], g['pd'])) <= mc.BOUND, name
