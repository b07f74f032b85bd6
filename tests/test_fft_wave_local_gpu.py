"""The wave-local form of the 2048-point LDS transform (kwy_fftwl_* in kwy_fft.hpp: in-place decimation in frequency
behind the first pass, two workgroup barriers per transform) against the Stockham chain it replaces in k_d4c_body<12>
and k_d4c_bands<12>, side by side in libkwy_selftest.so on the same rows: the drained pairs lo[0..3], hi[0..3], mid of
every thread are the same numbers (np.array_equal, which takes -0 for +0; both paths take the same first pass for a kind
of input, so the half form's zeros of either sign are the same ones).  Four kinds of input: dense, half with a live point
H/2, half with point H/2 stored as zero, sparse (257 points from registers).  Every problem starts from a buffer full of
stale numbers -- NaNs, in the last problems of a kind large random values -- where the kernels' buffer holds the previous
transform, the smoothing scratch or the select's words.
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, NT = 2048, 256
KINDS = {'dense': 0, 'half': 1, 'half, point H/2 zero': 2, 'sparse': 3}
SUPPORT = {0: H, 1: H // 2 + 1, 2: H // 2, 3: H // 8 + 1}      # points the transform takes from the row


def _impulse_positions():
    """32 positions j + 256 m of the first-pass index: every j mod 8, every (j >> 3) mod 4, every j >> 5, every m"""
    pos = []
    for i in range(32):
        j = (i % 8) + 8 * ((i // 8) % 4) + 32 * ((3 * i + i // 8) % 8)
        pos.append(j + 256 * ((i + i // 8) % 8))
    assert {p % 8 for p in pos} == set(range(8)) and {(p >> 3) % 4 for p in pos} == set(range(4))
    assert {(p % 256) >> 5 for p in pos} == set(range(8)) and {p >> 8 for p in pos} == set(range(8))
    return pos


def _rows(kind, rng):
    n = SUPPORT[kind]
    rows, stale, names = [], [], []

    def add(name, r, old=None):
        r = np.array(r, dtype=np.float64)
        r[n:] = 0.0                                    # what the kind of input takes as zero IS zero in the row
        rows.append(r)
        stale.append(np.full((H + 1, 2), np.nan) if old is None else old)
        names.append(name)

    for i in range(3):
        add(f'random {i}', rng.standard_normal((H, 2)))
    add('random, wide range', rng.standard_normal((H, 2)) * np.exp(rng.normal(0, 6, (H, 1))))
    add('constant', np.full((H, 2), (0.75, -1.25)))
    # (the narrower inputs: the positions inside the support, and every fourth of the others at its first-pass index j)
    pos = _impulse_positions()
    pos = [p for p in pos if p < n] + [p % 256 for p in pos[::4] if p >= n] + [H // 2, H // 8, n - 1]
    for p in sorted(set(pos)):
        if p < n:
            r = np.zeros((H, 2))
            r[p] = (1.0, 0.5)
            add(f'impulse at {p}', r)
    for i in range(2):
        add(f'random {i}, stale numbers', rng.standard_normal((H, 2)), rng.standard_normal((H + 1, 2)) * 1e3)
    return np.ascontiguousarray(np.stack(rows)), np.ascontiguousarray(np.stack(stale)), names


@pytest.fixture(scope='module')
def runs():
    import torch
    from conftest import ROOT
    from kwiiyatta_amd import _lib  # noqa: F401  (loads the HIP runtime the way the package does)
    st = ctypes.CDLL(os.path.join(ROOT, 'kwiiyatta_amd', 'libkwy_selftest.so'))
    st.kwy_debug_fft_wave_local_dev.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(2048)
    out = {}
    for kind in KINDS.values():
        x, stale, names = _rows(kind, rng)
        dx, ds = torch.from_numpy(x).to(dev), torch.from_numpy(stale).to(dev)
        old, new = (torch.full((len(x), NT, 9, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(2))
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        assert st.kwy_debug_fft_wave_local_dev(stream, dx.data_ptr(), ds.data_ptr(), len(x), kind, old.data_ptr(),
                                               new.data_ptr()) == 0
        torch.cuda.synchronize()
        out[kind] = (x, names, old.cpu().numpy(), new.cpu().numpy())
    return out


def test_the_inputs_cover_what_they_should(runs):
    total = 0
    for kind in KINDS.values():
        x, names, _, _ = runs[kind]
        total += len(names)
        assert any(name.startswith('impulse') for name in names) and 'constant' in names
        if kind == 1:
            assert (x[0][H // 2] != 0).all()                       # a live point H/2
        if kind == 3:
            assert (x[0][:H // 8 + 1] != 0).all() and not x[0][H // 8 + 1:].any()      # 257 points, x[256] among them
    assert total <= 120                                         # a few dozen problems


@pytest.mark.parametrize('name', list(KINDS))
def test_wave_local_pairs_equal_the_chain(runs, name):
    x, names, old, new = runs[KINDS[name]]
    assert np.isfinite(old).all() and np.abs(old).max() > 0
    for i, row in enumerate(names):
        assert np.isfinite(new[i]).all(), f'{name}, {row}: the transform read a stale point'
        bad = np.argwhere((new[i] != old[i]).any(axis=-1))
        assert bad.size == 0, f'{name}, {row}: (thread, slot) {bad[:8].tolist()} differ'
    assert np.array_equal(new, old)


def _bins(pairs):
    """(problems, NT, 9) complex drained pairs -> (problems, H) bins, by the slots of kwy_fft_tail4_drain"""
    t = np.arange(NT)
    k = np.stack([t, 512 + t, np.where(t > 0, 512 - t, 256), np.where(t > 0, 1024 - t, 768)], axis=1)     # kwy_drain_bin
    X = np.full((pairs.shape[0], H), np.nan, dtype=np.complex128)
    X[:, k] = pairs[:, :, 0:4]
    X[:, (H - k) % H] = pairs[:, :, 4:8]
    X[:, 1024 + t] = pairs[:, :, 8]
    return X


@pytest.mark.parametrize('name', list(KINDS))
def test_the_chain_is_the_transform(runs, name):
    """what the comparison above rests on: the pairs are the (unnormalised) DFT of the rows (double precision, eleven
    butterfly levels: the bound of tests/test_fft_half_w_gpu.py), thread 0's slot 0 holds X[0] twice"""
    x, _, old, new = runs[KINDS[name]]
    z = x[..., 0] + 1j * x[..., 1]
    want = np.fft.fft(z, axis=1)
    for got in (old, new):
        c = got[..., 0] + 1j * got[..., 1]
        assert np.array_equal(c[:, 0, 0], c[:, 0, 4])
        X = _bins(c)
        assert (np.abs(X - want) <= 1e-12 * np.maximum(np.abs(want).max(axis=1, keepdims=True), 1e-300)).all()
