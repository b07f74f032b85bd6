"""D4C with the closing FFT pass drained into registers (4096-point frames: 32 and 48 kHz) beside the sizes that keep
the stored pass (96 kHz: 8192 points, no radix-4 tail; 16 kHz: 2048 points): parity with the oracle on the short edge
case, batched calls bit-equal to single ones, a one-frame utterance, and the bits of the build before the change
(tests/golden/d4c_regs_48k.npz)."""
import os

import numpy as np
import pytest

from d4c_cases import FRAME_PERIOD, UNGATED, assert_ap_close, edge_case

pytestmark = pytest.mark.gpu

RATES = (32000, 48000, 96000, 16000)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'd4c_regs_48k.npz')


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def kw():
    from kwiiyatta_amd.backend import world
    return world


@pytest.mark.parametrize('fs', RATES)
def test_short_edge_case_parity(ko, kw, fs):
    x, f0, t, _ = edge_case(fs, 3, short=True)
    ref = ko.d4c(x, f0, t, fs)
    assert not (ref == UNGATED).all(), 'the case must reach the gated path'
    assert_ap_close(kw.d4c(x, f0, t, fs), ref, f'regs edge {fs} short')


def _ragged(fs):
    """the short edge case, a signal shorter than one analysis window, an all-unvoiced track"""
    edge = edge_case(fs, 4, short=True)[:3]
    rng = np.random.default_rng([fs, 5])
    n = int(0.005 * fs)                                   # 5 ms against windows of 30 .. 40 ms at 100 Hz
    sub = (np.ascontiguousarray(np.sin(2 * np.pi * 100.0 * np.arange(n) / fs) + 0.01 * rng.standard_normal(n)),
           np.full(3, 100.0), np.arange(3) * FRAME_PERIOD)
    xu = 0.1 * rng.standard_normal(int(0.04 * fs))
    unvoiced = (np.ascontiguousarray(xu), np.zeros(8), np.arange(8) * FRAME_PERIOD)
    return [edge, sub, unvoiced]


@pytest.mark.parametrize('fs', RATES)
def test_batched_call_equals_single_calls(kw, fs):
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    ctx = _lib.Context(0)
    utts = _ragged(fs)
    fft = lib.kwy_cheaptrick_fft_size(fs, 71.0)
    K = fft // 2 + 1
    dev = [tuple(torch.from_numpy(a).cuda() for a in u) for u in utts]
    ap = [torch.empty((len(u[1]), K), dtype=torch.float64, device='cuda') for u in utts]
    torch.cuda.synchronize()
    arr = _lib.utterance_array([(d[0], d[2], d[1], o) for d, o in zip(dev, ap)])
    _lib.check(ctx, lib.kwy_d4c_batch_dev(ctx.handle, arr, len(utts), fs, 0.85, fft))
    ctx.sync()
    for i, ((x, f0, t), a_) in enumerate(zip(utts, ap)):
        assert np.array_equal(a_.cpu().numpy(), kw.d4c(x, f0, t, fs)), (fs, i)
    assert (ap[2].cpu().numpy() == UNGATED).all()


@pytest.mark.parametrize('fs', RATES)
def test_one_frame_utterance(ko, kw, fs):
    x, _, _, _ = edge_case(fs, 6, short=True)
    f0, t = np.array([120.0]), np.array([0.01])
    ref = ko.d4c(x, f0, t, fs)
    assert_ap_close(kw.d4c(x, f0, t, fs), ref, f'regs one frame {fs}')


def test_bits_of_the_stored_pass_build(kw):
    """The change moves data, not arithmetic: the aperiodicity of the short 48 kHz edge case is, bit for bit, what the
    library computed on an MI355X before it (commit and seed are recorded in the file)."""
    g = np.load(GOLDEN)
    fs, seed = int(g['fs']), int(g['seed'])
    x, f0, t, _ = edge_case(fs, seed, short=bool(g['short']))
    got = kw.d4c(x, f0, t, fs)
    assert got.shape == g['ap'].shape
    assert not (g['ap'] == UNGATED).all()
    assert np.array_equal(got, g['ap']), f"differs from the build at {g['commit']}"
