"""The stride-64 radix-8 pass of the LDS transforms takes the powers of its wave-uniform factor from a per-context
table by scalar loads instead of forming them in every lane.  That may not change a bit:

  * the pass with per-lane powers and with table powers, side by side in libkwy_selftest.so, on every bin; the table
    against a one-thread recomputation, and its conjugate against the powers of the conjugate factor;
  * D4C and the synthesis against outputs recorded on an MI355X from the build before the change
    (tests/golden/d4c_bits_parent.npz, synth_bits_parent.npz; inputs: tests/bits_cases.py).  The D4C cases run every
    transform length (16 .. 96 kHz) over f0 tracks from the floor to 790 Hz, and two tracks so high that the first
    smoothing of the static group delay reads its input up to the last bin; the synthesis cases have voiced pulses
    with and without a periodic response and unvoiced ones.
"""
import ctypes
import os

import numpy as np
import pytest

import bits_cases as bc
from d4c_cases import UNGATED

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# (log2 of the transform length, threads): the thread counts the kernels run these lengths with
SHAPES = ((10, 128), (10, 256), (11, 256), (12, 512))
PREFIXES = (1, 2, 3, 63, 64, 65, 511, 512, 513)
IMPULSES = (0, 1, 63, 64, 65, 511, 512, -1)


def _rows(h):
    """complex rows of h points as (rows, h, 2) doubles: random, a wide dynamic range, non-zero on a prefix whose
    length sits on the seams of the thread / butterfly maps, unit impulses"""
    rng = np.random.default_rng(13)
    rows = [rng.standard_normal((h, 2)) for _ in range(3)]
    rows.append(rng.standard_normal((h, 2)) * np.exp(rng.normal(0, 6, (h, 1))))
    for wl in PREFIXES:
        r = np.zeros((h, 2))
        r[:wl] = rng.standard_normal((wl, 2))
        rows.append(r)
    for i in IMPULSES:
        r = np.zeros((h, 2))
        r[i, 0] = 1.0
        rows.append(r)
    return np.ascontiguousarray(np.stack(rows))


def _entry():
    from conftest import ROOT
    from kwiiyatta_amd import _lib  # noqa: F401  (loads the HIP runtime the way the package does)
    st = ctypes.CDLL(os.path.join(ROOT, 'kwiiyatta_amd', 'libkwy_selftest.so'))
    st.kwy_debug_fft_powers_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int] + [ctypes.c_void_p] * 5
    return st.kwy_debug_fft_powers_dev


@pytest.mark.parametrize('inverse', (False, True))
@pytest.mark.parametrize('log2h,nt', SHAPES)
def test_table_powers_equal_lane_powers(log2h, nt, inverse):
    import torch
    h = 1 << log2h
    x = _rows(h)
    dev = torch.device('cuda', 0)
    dx = torch.from_numpy(x).to(dev)
    lane, table = (torch.full(x.shape, np.nan, dtype=torch.float64, device=dev) for _ in range(2))
    tab, ref, refc = (torch.full((h // 512, 8, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    assert _entry()(torch.cuda.current_stream().cuda_stream, dx.data_ptr(), len(x), log2h, nt, int(inverse),
                    lane.data_ptr(), table.data_ptr(), tab.data_ptr(), ref.data_ptr(), refc.data_ptr()) == 0
    torch.cuda.synchronize()
    lane, table = lane.cpu().numpy(), table.cpu().numpy()
    for i in range(len(x)):
        bad = np.flatnonzero((lane[i] != table[i]).any(axis=1))
        assert bad.size == 0, f'row {i}: bins {bad[:8].tolist()} differ, e.g. {lane[i, bad[0]]} / {table[i, bad[0]]}'
    assert np.array_equal(lane, table)
    # the table is what one thread computes from w, and its conjugate what one thread computes from conj(w)
    tab, ref, refc = tab.cpu().numpy(), ref.cpu().numpy(), refc.cpu().numpy()
    assert np.array_equal(tab, ref)
    assert np.array_equal(tab * np.array([1.0, -1.0]), refc)
    w = np.exp(-2j * np.pi * 64 * np.arange(h // 512)[:, None] * np.arange(8)[None, :] / h)
    # (w^1 is within an ulp of exp(), a power up to w^7 multiplies that by 7, and each of its <= 3 complex products adds
    # at most sqrt(5) units of 2^-53: below 2e-15 in all; the bound is four times that)
    assert np.abs(tab[..., 0] + 1j * tab[..., 1] - w).max() <= 8e-15
    # and both paths are the transform (double precision, log2h butterfly levels)
    z = x[..., 0] + 1j * x[..., 1]
    want = np.fft.ifft(z, axis=1) * h if inverse else np.fft.fft(z, axis=1)
    got = table[..., 0] + 1j * table[..., 1]
    assert (np.abs(got - want) <= 1e-12 * np.abs(want).max(axis=1, keepdims=True)).all()


def test_other_shapes_are_refused():
    import torch
    buf = torch.zeros(1 << 14, dtype=torch.float64, device='cuda')
    p = buf.data_ptr()
    for log2h, nt in ((9, 256), (10, 64), (11, 128), (12, 256), (13, 512)):
        assert _entry()(None, p, 1, log2h, nt, 0, p, p, p, p, p) == -1


@pytest.fixture(scope='module')
def kw():
    from kwiiyatta_amd.backend import world
    return world


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def d4c_golden():
    return np.load(os.path.join(GOLDEN, 'd4c_bits_parent.npz'))


def _check_d4c(got, x, f0, t, fs, ko, want, commit):
    assert not (ko.d4c(x, f0, t, fs) == UNGATED).all(), 'the case must reach the gated path'
    assert not (want == UNGATED).all()
    got = bc.d4c_sample(got)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f'differs from the build at {commit}'


@pytest.mark.parametrize('f0_value', bc.D4C_F0)
@pytest.mark.parametrize('fs', bc.D4C_RATES)
def test_d4c_bits_of_the_parent_build(kw, ko, d4c_golden, fs, f0_value):
    assert int(d4c_golden['seed']) == bc.SEED and int(d4c_golden['bin_step']) == bc.D4C_BIN_STEP
    x, f0, t = bc.d4c_case(fs, f0_value)
    _check_d4c(kw.d4c(x, f0, t, fs), x, f0, t, fs, ko, d4c_golden[bc.d4c_key(fs, f0_value)], d4c_golden['commit'])


@pytest.mark.parametrize('fs,f0_value', bc.D4C_HIGH)
def test_d4c_bits_where_every_bin_is_read(ko, d4c_golden, fs, f0_value):
    """f0 so high that the first smoothing of the static group delay reads the quotient up to the last bin: through
    the device entry, which does not hold f0 below fs / 5"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    x, f0, t = bc.d4c_case(fs, f0_value)
    n4 = 4096                                             # D4C's own transform length at 32 and 48 kHz
    c = int(f0_value * n4 / fs)
    dv_last = int(3000.0 * min(5, int((fs / 2 - 3000.0) / 3000.0)) * n4 / fs) + int(3000.0 * n4 / fs)
    assert dv_last + 2 * (c + 1) + 4 + int(f0_value / 2 * n4 / fs) + 1 + 3 >= n4 // 2, 'the read bound must reach H'
    ctx = _lib.Context(0)
    fft = lib.kwy_cheaptrick_fft_size(fs, 71.0)
    dx, df0, dt = (torch.from_numpy(a).cuda() for a in (x, f0, t))
    out = torch.empty((len(f0), fft // 2 + 1), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    _lib.check(ctx, lib.kwy_d4c_dev(ctx.handle, dx.data_ptr(), len(x), fs, dt.data_ptr(), df0.data_ptr(), len(f0),
                                    0.85, fft, out.data_ptr()))
    ctx.sync()
    _check_d4c(out.cpu().numpy(), x, f0, t, fs, ko, d4c_golden[bc.d4c_key(fs, f0_value, dev=True)],
               d4c_golden['commit'])


@pytest.mark.parametrize('fs', bc.SYNTH_RATES)
def test_synthesis_bits_of_the_parent_build(kw, fs):
    g = np.load(os.path.join(GOLDEN, 'synth_bits_parent.npz'))
    assert int(g['seed']) == bc.SEED
    f0, sp, ap = bc.synth_case(fs)
    assert (f0 > 0).any() and (f0 == 0).any()
    aperiodic_voiced = (f0 > 0) & (ap[:, 0] > 0.9995)
    assert aperiodic_voiced.any() and ((f0 > 0) & ~aperiodic_voiced).any()
    y = kw.synthesize(f0, sp, ap, fs, 5.0)
    want = g[f'y_{fs}']
    assert y.shape == want.shape == (int(0.3 * fs),)
    assert np.abs(want).max() > 0
    assert np.array_equal(y, want), f"differs from the build at {g['commit']}"
