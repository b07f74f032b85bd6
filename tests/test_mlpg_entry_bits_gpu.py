"""Every exported entry of the trajectory conversion (kwy_mlpg.hip) against the bits of the build before its host side
was folded into one core, one batch driver and one staging path (tests/golden/mlpg_entry_bits_parent.npz, recorded on
an MI355X by tools/record_mlpg_entry_bits.py; inputs and calls: tests/mlpg_entry_cases.py).  The host code decides
which kernels run, in which order, on which grids and buffers, so every output of every entry has to come out bit for
bit: the converted rows, the log-likelihoods, the ascent's objective and its status, on em in {none, 0, 2} x gv in
{none, 0, 4 iterations}, through the single-utterance device entries, the batch entries (17 utterances: two passes), the
host-pointer entries and the frame-wise conversion.  A refused call gives the recorded return code and message and
leaves its output buffers as they were.
"""
import os

import numpy as np
import pytest

import mlpg_entry_cases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mlpg_entry_bits_parent.npz')


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    assert int(g['seed']) == mc.SEED and len(str(g['commit'])) == 40
    return g


@pytest.fixture(scope='module')
def recorded(golden):
    return mc.unpack(golden)


@pytest.fixture(scope='module')
def ctx():
    from kwiiyatta_amd import _lib
    return _lib.Context(0)


def test_fixture_holds_every_case(golden, recorded):
    assert os.path.getsize(GOLDEN) < 350 * 1024
    assert {key for key, _, _ in mc.CASES} == set(recorded)
    assert str(golden['refusal_digest']) == mc.refusal_digest()
    n = len(mc.REFUSALS)
    assert golden['refusal_rc'].shape == golden['refusal_message'].shape == golden['refusal_clean'].shape == (n,)
    assert (golden['refusal_rc'] != 0).all()
    # the grid of options on every shape, through every kind of entry
    assert mc.EMS == (-1, 0, 2) and mc.GVS == (-1, 0, 4) and mc.TS == (1, 17, 65)
    assert [s[:2] for s in mc.SHAPES] == [(2, 3), (24, 3)] and [h[:2] + h[4:] for h in mc.HOST] == [(2, 3, 17), (24, 3, 33)]
    for em in mc.EMS:
        for gv in mc.GVS:
            opt = mc._opt(em, gv)
            assert 'out' in recorded[f'batch_{opt}']
            for d, *_ in mc.SHAPES:
                for T in mc.TS:
                    assert recorded[f'dev_d{d}_T{T}_{opt}']['mc_out'].size == T * (d + 1)
                    assert recorded[f'mlpg_dev_d{d}_T{T}']['y'].size == recorded[f'mlpg_model_dev_d{d}_T{T}']['y'].size == T * d
            for d, _, _, _, T in mc.HOST:
                for diff in (0, 1):
                    outs = recorded[f'host_d{d}_diff{diff}_{opt}']
                    assert outs['y'].size == T * d
                    assert ('loglik' in outs) == (em >= 0 or gv >= 0) and ('objective' in outs) == ('status' in outs) == (gv >= 0)
    # 17 utterances of 1 .. 17 frames, d = 2: rows of d + 1 (of d + 2 where the DTW feature rows are written)
    assert len(mc.BATCH_TS) == mc.KWY_BATCH_MAX + 1
    assert recorded['batch_emnone_gvnone']['out'].size == sum(mc.BATCH_TS) * 3
    assert recorded['batch_realign']['out'].size == sum(mc.BATCH_TS) * 4
    assert recorded['frames_host_diff0']['y'].size == 17 * mc.FRAMES_D


@pytest.mark.gpu
@pytest.mark.parametrize('group', mc.GROUPS)
def test_entries_give_the_bits_of_the_parent_build(golden, recorded, ctx, group):
    for key, g, call in mc.CASES:
        if g != group:
            continue
        got, want = mc.run_case(ctx, call), recorded[key]
        assert got.keys() == want.keys(), key
        for name, a in got.items():
            assert a.size == want[name].size and np.array_equal(a.ravel(), want[name], equal_nan=True), \
                f"{key}, {name}: differs from the build at {golden['commit']}"


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ('dev', 'batch', 'host', 'mlpg', 'frames'))
def test_refusals_give_the_code_and_message_of_the_parent_build(golden, ctx, kind):
    messages = [m.decode() for m in golden['refusal_messages']]
    seen = 0
    for i, (key, call) in enumerate(mc.REFUSALS):
        if not key.startswith(f'refuse_{kind}_'):
            continue
        seen += 1
        rc, err, clean = mc.run_refusal(ctx, call)
        assert rc != 0 and rc == int(golden['refusal_rc'][i]), key
        assert err == messages[golden['refusal_message'][i]], key
        assert clean == bool(golden['refusal_clean'][i]), key
    assert seen > 0
