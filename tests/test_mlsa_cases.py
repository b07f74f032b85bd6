"""The inputs of the MLSA edge tests (tests/mlsa_cases.py) held to their conditions with the CPU oracle alone, without a
GPU: the case lists are what the kernel's seams ask for, every oracle output is finite, nonzero in the filtered frames
and exactly zero behind them -- so what test_mlsa_edges_gpu.py expects of the kernel is established here."""
import numpy as np
import pytest

import mlsa_cases as mc


def test_case_lists_sit_on_the_kernel_seams():
    assert [c.hop for c in mc.HOP_CASES[::2]] == [1, 2, 63, 64, 65, 127, 128, 129, mc.MLSA_MAX_HOP]
    assert all(c.n == c.T * c.hop + 1 and mc.nproc(c) == c.T for c in mc.HOP_CASES + mc.ORDER_CASES)
    blocks = [(c.order - 1 + 7) // 8 for c in mc.ORDER_CASES[::2]]
    assert blocks == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8]         # last order of a block, first of the next
    assert mc.ORDER_CASES[0].order == 2 and mc.ORDER_CASES[-1].order == mc.MLSA_MAX_ORDER
    assert {c.pd for c in mc.HOP_CASES} == {c.pd for c in mc.ORDER_CASES} == {4, 5}
    assert tuple(mc.nproc(c) for c in mc.GRID_CASES[:-1]) == mc.GRID_NPROC
    assert mc.nproc(mc.GRID_CASES[-1]) == 1 and mc.GRID_CASES[-1].T == 1      # T, not n, ends the filtering
    assert sorted(mc.nproc(c) for c in mc.BATCH_JOBS) == [0, 1, 1, 2, 3]
    assert len({c.n for c in mc.BATCH_JOBS}) == 5 and len(mc.BATCH_JOBS) <= mc.MLSA_JOBS_MAX
    assert len({c.name for c in mc.ALL_CASES}) == len(mc.ALL_CASES)


def test_inputs_keep_c0_and_constant_cases_have_no_slope():
    for case in mc.ALL_CASES:
        x, mcep = mc.inputs(case)
        assert x.shape == (case.n,) and mcep.shape == (case.T, case.order + 1)
        assert np.all(mcep[:, 0] != 0.0)
        if case.constant:
            assert np.all(mcep == mcep[0])
    c0 = np.concatenate([mc.inputs(c)[1][:, 0] for c in mc.HOP_CASES])
    assert 0.5 < c0.std() < 1.5 and np.ptp(c0) > 3.0                          # b[0] moves by units between frames


@pytest.mark.parametrize('case', mc.ALL_CASES + mc.BATCH_JOBS, ids=lambda c: c.name)
def test_oracle_output_is_finite_nonzero_in_front_and_zero_behind(case):
    for ignore_c0 in ((False, True) if case in mc.BATCH_JOBS else (False,)):
        x, mcep, b, y = mc.reference(case, ignore_c0)
        if ignore_c0:
            from oracle import oracle as ko
            assert np.array_equal(b[:, 1:], ko.mc2b(mcep, case.alpha)[:, 1:]) and not np.array_equal(b, ko.mc2b(mcep, case.alpha))
        done = mc.nproc(case) * case.hop
        assert np.isfinite(y).all()
        assert np.all(y[done:] == 0.0) and len(y[done:]) >= 1
        if done:
            assert np.all(y[:done] != 0.0)
            assert 1e-3 < np.abs(y).max() < 1e3
