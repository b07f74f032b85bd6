"""The block-wide "sum of the m smallest of n" (kwy_device.hpp) against the reference copy of its earlier form that the
self-test library keeps (ONE histogram counted with same-address atomics, kwy_block_sum2 behind it): the two sums must
agree BIT FOR BIT -- the threshold is one of the keys and the sums keep their order -- and both lie within the
sort-based bound of test_select_gpu.py (1e-13 of the total).

The inputs are built bin by bin.  The from-the-top path puts a key into the bin (hmax - high word) >> 18, hmax the
largest high word of the block: quarter binades below the maximum, 256 of them, the last one taking everything lower.
Every constructed case asserts on the host, with that formula, that it has the bin population it is meant to have:
  - runs of >= 64 consecutive elements in one bin (a whole wavefront counts into one bin),
  - a chosen bin of exactly LIST keys (the largest the ranking takes) and of LIST + 1 (hand-over to the radix path),
  - the wanted rank first / last in its bin, ties that straddle the cut inside the chosen bin,
  - the threshold in the last (overflow) bin, all keys equal, all keys zero,
for n = 65, 66, 257, 2049 and (512 threads) 4097 with m = n - 65 where that is positive, and m = 1.
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BINS = 256
LIST = BINS // 2 - 4                # KWY_SELECT_LIST
SHIFT = 18
HMAX = 0x3FF00000                   # high word of the constructed maximum, 1.0
CHOSEN = 20                         # the bin the constructed cases put the wanted rank in


def _bins(x):
    hi = (np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) >> np.uint64(32)).astype(np.int64)
    return np.minimum((hi.max() - hi) >> SHIFT, BINS - 1)


def _keys(bins, rng, distinct=False):
    """doubles whose high word lies `bins` quarter binades below HMAX, random below that"""
    bins = np.asarray(bins, dtype=np.int64)
    off = rng.choice(1 << SHIFT, len(bins), replace=False) if distinct else rng.integers(0, 1 << SHIFT, len(bins))
    hi = (HMAX - (bins << SHIFT) - off).astype(np.uint64)
    lo = rng.integers(0, 1 << 32, len(bins), dtype=np.uint64)
    return ((hi << np.uint64(32)) | lo).view(np.float64)


def _built(n, kk, above, pop, rng, run=False, ties=None, overflow=False):
    """n keys: `above` of them in the bins in front of CHOSEN (the maximum 1.0 among them), `pop` in CHOSEN, the rest
    behind it (overflow: `pop` is ignored, everything else lies below the last bin's edge).  Checks the population and
    that the kk-th largest key lies in the intended bin.  run: the chosen bin's keys and 64 keys of one lower bin are
    consecutive elements from index 64 on, so whole wavefronts count into one bin."""
    top = np.r_[1.0, _keys(rng.integers(0, CHOSEN, above - 1), rng)]
    top[1:] = np.minimum(top[1:], 1.0)
    if overflow:
        rest = rng.random(n - above) * 1e-200 + 1e-250
        x = np.r_[top, rest]
        x = x[rng.permutation(n)]
        b = _bins(x)
        assert (b < BINS - 1).sum() == above and (b == BINS - 1).sum() == n - above and kk > above
        return x
    mid = _keys(np.full(pop, CHOSEN), rng, distinct=True)
    if ties is not None:
        mid = np.sort(mid)[::-1].copy()
        mid[ties[0]:ties[1]] = mid[ties[0]]
    nlow = n - above - pop
    if run:
        nrun = 64
        low = np.r_[_keys(np.full(nrun, CHOSEN + 8), rng), _keys(rng.integers(CHOSEN + 1, BINS - 1, nlow - nrun), rng)]
        x = np.r_[top[:1], top[1:], low[nrun:]]
        x = x[rng.permutation(len(x))]
        x = np.r_[x[:64], mid, low[:nrun], x[64:]]
        b = _bins(x)
        assert (b[64:64 + pop] == CHOSEN).all() and pop >= 64
        assert (b[64 + pop:64 + pop + nrun] == CHOSEN + 8).all() and nrun >= 64
    else:
        low = _keys(rng.integers(CHOSEN + 1, BINS - 1, nlow), rng)
        x = np.r_[top, mid, low]
        x = x[rng.permutation(n)]
        b = _bins(x)
    assert len(x) == n and x.max() == 1.0
    assert (b < CHOSEN).sum() == above and (b == CHOSEN).sum() == pop
    srt = np.sort(x)[::-1]
    assert above < kk <= above + pop and _bins(np.r_[1.0, srt[kk - 1]])[1] == CHOSEN
    inbin = np.sort(x[b == CHOSEN])[::-1]
    assert inbin[kk - above - 1] == srt[kk - 1]
    if ties is not None:                # equal keys on both sides of the cut
        assert ties[0] < kk - above - 1 < ties[1] - 1 and (inbin[ties[0]:ties[1]] == srt[kk - 1]).all()
    return x


def _cases(n, m, rng):
    kk = n - m + 1                      # the wanted key's rank from the top
    k = np.arange(n)
    out = []
    for width, floor in ((20.0, 1e-9), (3.0, 1e-14)):      # a lobe over a floor: smooth, neighbours share a bin
        out.append(np.exp(-0.5 * ((k - n // 3) / width) ** 2) * 1.7 + floor * rng.random(n))
    out.append(rng.random(n))                               # flat: crowded bins
    out.append(np.full(n, 3.25))                            # all equal
    out.append(np.zeros(n))                                 # all zero
    t = rng.random(n) * 1e-3; t[rng.choice(n, min(90, n - 1), replace=False)] = 7.0; out.append(t)
    if kk == 66 and n >= 257:
        out.append(_built(n, kk, 30, 64, rng, run=True))               # whole wavefronts in one bin, twice
        out.append(_built(n, kk, 10, LIST, rng))                        # the largest list
        out.append(_built(n, kk, 10, LIST + 1, rng))                    # one too many: radix path
        out.append(_built(n, kk, 65, 40, rng))                          # first key of its bin
        out.append(_built(n, kk, 26, 40, rng))                          # last key of its bin
        out.append(_built(n, kk, 51, 50, rng, ties=(10, 30)))           # ties across the cut inside the bin
        out.append(_built(n, kk, 30, 0, rng, overflow=True))            # threshold in the overflow bin
    elif kk == n and n >= 257:
        out.append(_built(n, kk, 30, 0, rng, overflow=True))            # the smallest of the overflow bin
        out.append(_built(n, kk, n - LIST, LIST, rng))                  # last key of the last occupied bin
    return np.stack([np.ascontiguousarray(a, dtype=np.float64) for a in out])


_NM = [(65, 1), (66, 1), (257, 192), (257, 1), (2049, 1984), (2049, 1)]


@pytest.mark.parametrize('threads,n,m', [(256, n, m) for n, m in _NM] +
                         [(512, n, m) for n, m in _NM + [(4097, 4032), (4097, 1)]])
def test_select_equals_reference_copy(threads, n, m):
    import torch
    from conftest import ROOT
    from kwiiyatta_amd import _lib                   # noqa: F401  (loads the HIP runtime the way the package does)
    st = ctypes.CDLL(os.path.join(ROOT, 'kwiiyatta_amd', 'libkwy_selftest.so'))
    fn = st.kwy_debug_select_paths_dev if threads == 256 else st.kwy_debug_select_paths512_dev
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                   ctypes.c_void_p]
    X = _cases(n, m, np.random.default_rng(1000 * n + m))
    dev = torch.device('cuda', 0)
    dx = torch.from_numpy(X).to(dev)
    ref = torch.full((len(X), 2), -1.0, dtype=torch.float64, device=dev)
    new = torch.full((len(X), 2), -2.0, dtype=torch.float64, device=dev)
    assert fn(torch.cuda.current_stream().cuda_stream, dx.data_ptr(), len(X), n, m, ref.data_ptr(),
              new.data_ptr()) == 0
    torch.cuda.synchronize()
    ref, new = ref.cpu().numpy(), new.cpu().numpy()
    for i, x in enumerate(X):
        srt = np.sort(x)
        want_small, want_all = srt[:m].sum(), srt.sum()
        tol = 1e-13 * max(want_all, 1e-300)
        print(f'case {i}: new {new[i]} ref {ref[i]} sort {want_small!r} {want_all!r}')
        for got in (ref[i], new[i]):
            assert abs(got[1] - want_all) <= tol, (i, got[1], want_all)
            assert abs(got[0] - want_small) <= tol, (i, got[0], want_small)
    assert np.array_equal(new[:, 0], ref[:, 0])
    assert np.array_equal(new[:, 1], ref[:, 1])
