"""The closing radix-4 pass of the 2048-point LDS transform drained into registers (kwy_fft_tail4_drain, behind the
4096-sample real transforms of the D4C kernels) against the stored pass it replaces: the same rows through both
paths of libkwy_selftest.so must give the same bits in every bin 0 .. N/2.  Rows: random, non-zero on a prefix whose
length sits on the seams of the thread / butterfly maps, and unit impulses."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# sizes with a drained closing pass (kwy_d4c.hip: d4c_drain); the others keep the stored pass and have no second path
LOG2N = (12,)
PREFIXES = (1, 2, 3, 15, 16, 17, 511, 512, 513, -1, 0)       # -1, 0: N - 1 and N
IMPULSES = (0, 1, 255, 256, 257, 2047, 2048, -1)            # -1: N - 1


def _rows(n):
    rng = np.random.default_rng(12)
    rows = [rng.standard_normal(n) for _ in range(3)]
    rows.append(rng.standard_normal(n) * np.exp(rng.normal(0, 6, n)))          # a wide dynamic range
    for wl in PREFIXES:
        r = np.zeros(n)
        r[:(wl + n if wl <= 0 else wl)] = rng.standard_normal(wl + n if wl <= 0 else wl)
        rows.append(r)
    for i in IMPULSES:
        r = np.zeros(n)
        r[i] = 1.0
        rows.append(r)
    return np.ascontiguousarray(np.stack(rows))


def _entry():
    from conftest import ROOT
    from kwiiyatta_amd import _lib  # noqa: F401  (loads the HIP runtime the way the package does)
    st = ctypes.CDLL(os.path.join(ROOT, 'kwiiyatta_amd', 'libkwy_selftest.so'))
    st.kwy_debug_rfft_paths_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p]
    return st.kwy_debug_rfft_paths_dev


@pytest.mark.parametrize('log2n', LOG2N)
def test_drained_pass_equals_stored_pass(log2n):
    import torch
    n = 1 << log2n
    x = _rows(n)
    dev = torch.device('cuda', 0)
    dx = torch.from_numpy(x).to(dev)
    old = torch.full((len(x), n // 2 + 1, 2), np.nan, dtype=torch.float64, device=dev)
    new = torch.full((len(x), n // 2 + 1, 2), np.nan, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    assert _entry()(torch.cuda.current_stream().cuda_stream, dx.data_ptr(), len(x), log2n, old.data_ptr(),
                    new.data_ptr()) == 0
    torch.cuda.synchronize()
    old, new = old.cpu().numpy(), new.cpu().numpy()
    for i in range(len(x)):
        bad = np.flatnonzero((old[i] != new[i]).any(axis=1))
        assert bad.size == 0, f'row {i}: bins {bad[:8].tolist()} differ, e.g. {old[i, bad[0]]} / {new[i, bad[0]]}'
    assert np.array_equal(old, new)
    # and both are the transform: twice the bins of the real FFT (double precision, 12 butterfly levels)
    ref = 2.0 * np.fft.rfft(x, axis=1)
    got = old[..., 0] + 1j * old[..., 1]
    scale = np.abs(ref).max(axis=1, keepdims=True)
    assert (np.abs(got - ref) <= 1e-12 * scale).all()


def test_sizes_without_a_drained_pass_are_refused():
    import torch
    buf = torch.zeros(1 << 14, dtype=torch.float64, device='cuda')
    for log2n in (10, 11, 13):
        assert _entry()(None, buf.data_ptr(), 1, log2n, buf.data_ptr(), buf.data_ptr()) == -1
