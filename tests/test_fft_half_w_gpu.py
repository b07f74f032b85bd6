"""kwy_fft_inplace_sel_w with half = true (kwy_fft.hpp), the LDS transform whose first radix-8 pass knows that the
packed points above H/2 are zero
(the windows of k_d4c_body at f0 >= 8 fs / N), against kwy_fft_inplace_w on the zero-padded row, side by side in
libkwy_selftest.so: every bin equal (adding exact zeros changes no value; np.array_equal takes -0 for +0), in the
three shapes of the body (1024 and 2048 points on 256 threads, 4096 on 512), forward and inverse, with the closing pass
and stopped in front of it.  The half path's buffer holds NaNs -- in the last rows random numbers -- above point H/2,
where the callers' buffer holds the smoothing scratch or the previous transform: nothing there may be read, and point
H/2 itself must be.
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (10, 11, 12)


def _rows(H, rng):
    """(rows, H, 2) inputs, zero above their support, the stale upper halves of the half path, and a name per row"""
    rows, stale, names = [], [], []

    def add(name, n, full, old=None):
        r = np.zeros((H, 2))
        r[:n] = full[:n]
        rows.append(r)
        stale.append(np.full((H, 2), np.nan) if old is None else old)
        names.append(name)

    wide = rng.standard_normal((H, 2)) * np.exp(rng.normal(0, 6, (H, 1)))
    supports = (('support H/2 + 1', H // 2 + 1), ('support H/2', H // 2), ('support H/8', H // 8), ('one point', 1))
    for name, n in supports:
        add(name, n, rng.standard_normal((H, 2)))
        add(name + ', wide range', n, wide)
    r = np.zeros((H, 2))
    r[H // 2] = rng.standard_normal(2)
    add('point H/2 alone', H // 2 + 1, r)
    add('all zero', 0, r)
    for n in (H // 2 + 1, H // 2 - 3):
        add(f'stale upper half, support {n}', n, rng.standard_normal((H, 2)), rng.standard_normal((H, 2)) * 1e3)
    return np.ascontiguousarray(np.stack(rows)), np.ascontiguousarray(np.stack(stale)), names


@pytest.fixture(scope='module')
def runs():
    import torch
    from conftest import ROOT
    from kwiiyatta_amd import _lib  # noqa: F401  (loads the HIP runtime the way the package does)
    st = ctypes.CDLL(os.path.join(ROOT, 'kwiiyatta_amd', 'libkwy_selftest.so'))
    st.kwy_debug_fft_half_w_dev.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(41)
    out = {}
    for log2h in SIZES:
        x, stale, names = _rows(1 << log2h, rng)
        dx, ds = torch.from_numpy(x).to(dev), torch.from_numpy(stale).to(dev)
        for inverse in (0, 1):
            for tail in (1, 0):
                dense, half = (torch.full(x.shape, np.nan, dtype=torch.float64, device=dev) for _ in range(2))
                torch.cuda.synchronize()
                stream = torch.cuda.current_stream().cuda_stream
                assert st.kwy_debug_fft_half_w_dev(stream, dx.data_ptr(), ds.data_ptr(), len(x), log2h, inverse, tail,
                                                   dense.data_ptr(), half.data_ptr()) == 0
                torch.cuda.synchronize()
                out[log2h, inverse, tail] = (x, names, dense.cpu().numpy(), half.cpu().numpy())
    return out


@pytest.mark.parametrize('inverse', (0, 1))
@pytest.mark.parametrize('log2h', SIZES)
def test_half_transform_equals_the_dense_one(runs, log2h, inverse):
    for tail in (1, 0):
        x, names, dense, half = runs[log2h, inverse, tail]
        assert np.isfinite(dense).all() and np.abs(dense).max() > 0
        for i, name in enumerate(names):
            assert np.isfinite(half[i]).all(), f'{name}: the half transform read above point H/2'
            bad = np.flatnonzero((half[i] != dense[i]).any(axis=1))
            assert bad.size == 0, f'{name}, tail {tail}: bins {bad[:8].tolist()} differ'
        assert np.array_equal(half, dense)


@pytest.mark.parametrize('inverse', (0, 1))
@pytest.mark.parametrize('log2h', SIZES)
def test_dense_transform_is_the_transform(runs, log2h, inverse):
    """what the comparison above rests on: the dense path is the (unnormalised) DFT of the rows
    (double precision, at most twelve butterfly levels: the bound of tests/test_twiddle_powers_gpu.py)"""
    x, _, dense, _ = runs[log2h, inverse, 1]
    z = x[..., 0] + 1j * x[..., 1]
    want = np.fft.ifft(z, axis=1) * z.shape[1] if inverse else np.fft.fft(z, axis=1)
    got = dense[..., 0] + 1j * dense[..., 1]
    assert (np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want).max(axis=1, keepdims=True), 1e-300)).all()
