"""The block-wide exclusive scan of one int per thread (kwy_block_exscan, kwy_device.hpp) that the training rows, the
band rows and the synthesis pulse lists share, against numpy.cumsum: exact, on the wavefront seams."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NT = 256


def _cases():
    rng = np.random.default_rng(8)                                # (a seed whose last case sums past 2^23; asserted below)
    out = [np.zeros(NT), np.ones(NT)]
    for t in (0, 63, 64, 127, 128, 255):                          # a single one on either side of every seam
        v = np.zeros(NT); v[t] = 1; out.append(v)
    v = np.zeros(NT); v[63::64] = 1; out.append(v)                # the last lane of every wavefront
    v = np.zeros(NT); v[0::64] = 1; out.append(v)                 # the first lane of every wavefront
    out.append(rng.integers(0, 4, NT))
    out.append(rng.integers(0, 65536, NT))                        # the total passes 2^23: no float path holds it
    return np.stack(out).astype(np.int32)


def test_block_exscan_matches_cumsum():
    import torch
    import ctypes
    import os
    from conftest import ROOT
    from kwiiyatta_amd import _lib                   # loads the HIP runtime the way the package does
    st = ctypes.CDLL(os.path.join(ROOT, 'kwiiyatta_amd', 'libkwy_selftest.so'))
    st.kwy_debug_block_exscan_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p]
    V = _cases()
    assert V[-1].sum() > 2 ** 23
    dev = torch.device('cuda', 0)
    dv = torch.from_numpy(V).to(dev)
    off = torch.full(V.shape, -1, dtype=torch.int32, device=dev)
    tot = torch.full((len(V),), -1, dtype=torch.int32, device=dev)
    assert st.kwy_debug_block_exscan_dev(torch.cuda.current_stream().cuda_stream, dv.data_ptr(), len(V),
                                         off.data_ptr(), tot.data_ptr()) == 0
    torch.cuda.synchronize()
    inc = np.cumsum(V, axis=1, dtype=np.int64)
    assert np.array_equal(off.cpu().numpy(), inc - V)
    assert np.array_equal(tot.cpu().numpy(), inc[:, -1])
