"""The 2048-point synthesis kernel leaves out work on known zeros and on values nobody reads: the causal cepstrum goes
into a first radix-8 pass that knows its upper half is zero, and the real split in front of the cepstrum fold forms only
the real parts it folds.  Adding exact zeros changes no value, so none of it may move a bit:

  * every first pass -- the dense one, the half-zero one and the sparse one that takes x[0 .. H/8] from registers (a
    short pulse's noise through it was measured slower and is not in the kernel) -- and both forms of
    the split + fold side by side in libkwy_selftest.so, on the same rows;
  * the synthesis against waveforms recorded on an MI355X from the build before the change
    (tests/golden/syn_zero_bits_parent.npz, recorded by tools/record_syn_zero_bits.py; inputs: tests/syn_zero_cases.py):
    pulse intervals of 255, 256 and 257 samples (noise of exactly H/8 packed points and one sample to either side),
    voiced pulses at 400 Hz with and without a periodic response, unvoiced stretches at both ends, at 48 and 22.05 kHz
    (2048 points) and at 16 kHz (1024 points, the untouched code); through the single call, through the batched entry
    with two utterances, and with the noise drawn by the generator inside the kernel instead of from the table (its
    word sequence now sits in the idle FFT buffer).
"""
import ctypes
import os

import numpy as np
import pytest

import syn_zero_cases as zc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'syn_zero_bits_parent.npz')
H = 1024
PREFIXES = (1, 47, 48, 49, 127, 128, 129)


def _rows():
    """complex rows of 1024 points as (rows, 1024, 2) doubles and, per row, the number of leading points that may be
    non-zero: random data and a wide dynamic range (whole, and cut to the 513 points the half pass and the 129 points
    the sparse pass take), non-zero prefixes on the seams of the sparse pass, point 512 alone, all zero"""
    rng = np.random.default_rng(29)
    rows, support = [], []
    for full in (rng.standard_normal((H, 2)), rng.standard_normal((H, 2)) * np.exp(rng.normal(0, 6, (H, 1)))):
        for n in (H, H // 2 + 1, H // 8 + 1):
            r = np.zeros((H, 2))
            r[:n] = full[:n]
            rows.append(r)
            support.append(n)
    for n in PREFIXES:
        r = np.zeros((H, 2))
        r[:n] = rng.standard_normal((n, 2))
        rows.append(r)
        support.append(n)
    r = np.zeros((H, 2))
    r[H // 2] = rng.standard_normal(2)
    rows.append(r)
    support.append(H // 2 + 1)
    rows.append(np.zeros((H, 2)))
    support.append(0)
    return np.ascontiguousarray(np.stack(rows)), np.array(support)


@pytest.fixture(scope='module')
def passes():
    import torch
    from conftest import ROOT
    from kwiiyatta_amd import _lib  # noqa: F401  (loads the HIP runtime the way the package does)
    st = ctypes.CDLL(os.path.join(ROOT, 'kwiiyatta_amd', 'libkwy_selftest.so'))
    st.kwy_debug_syn_first_passes_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5
    x, support = _rows()
    dev = torch.device('cuda', 0)
    dx = torch.from_numpy(x).to(dev)
    dense, sparse, half = (torch.full(x.shape, np.nan, dtype=torch.float64, device=dev) for _ in range(3))
    fold_ref, fold_new = (torch.full((len(x), H + 1), np.nan, dtype=torch.float64, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    assert st.kwy_debug_syn_first_passes_dev(torch.cuda.current_stream().cuda_stream, dx.data_ptr(), len(x),
                                             dense.data_ptr(), sparse.data_ptr(), half.data_ptr(), fold_ref.data_ptr(),
                                             fold_new.data_ptr()) == 0
    torch.cuda.synchronize()
    return x, support, [a.cpu().numpy() for a in (dense, sparse, half, fold_ref, fold_new)]


def test_first_passes_equal_the_dense_pass(passes):
    x, support, (dense, sparse, half, _, _) = passes
    assert (support <= H // 8 + 1).sum() >= len(PREFIXES) + 3 and (support == H).sum() == 2
    z = x[..., 0] + 1j * x[..., 1]
    want = np.fft.fft(z, axis=1)
    got = dense[..., 0] + 1j * dense[..., 1]
    # (double precision, ten butterfly levels: as tests/test_twiddle_powers_gpu.py)
    assert (np.abs(got - want) <= 1e-12 * np.abs(want).max(axis=1, keepdims=True)).all()
    for name, out, limit in (('sparse', sparse, H // 8 + 1), ('half', half, H // 2 + 1)):
        rows = np.flatnonzero(support <= limit)
        assert np.isfinite(out[rows]).all(), name
        for i in rows:
            bad = np.flatnonzero((out[i] != dense[i]).any(axis=1))
            assert bad.size == 0, f'{name}, row {i} ({support[i]} points): bins {bad[:8].tolist()} differ'
        assert np.array_equal(out[rows], dense[rows]), name
        got = out[rows, :, 0] + 1j * out[rows, :, 1]
        assert (np.abs(got - want[rows]) <= 1e-12 * np.abs(want[rows]).max(axis=1, keepdims=True)).all(), name


def test_fused_fold_equals_split_then_fold(passes):
    x, _, (_, _, _, fold_ref, fold_new) = passes
    assert np.isfinite(fold_ref).all()
    assert np.array_equal(fold_ref, fold_new)
    # the rows as 2048 packed reals: the fold keeps the real parts of bins 0 .. 1024, twice those in between
    want = np.fft.rfft(x.reshape(len(x), 2 * H), axis=1).real
    want[:, 1:H] *= 2.0
    assert (np.abs(fold_new - want) <= 1e-12 * np.maximum(np.abs(want).max(axis=1, keepdims=True), 1e-300)).all()


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    assert int(g['seed']) == zc.SEED and len(str(g['commit'])) == 40
    return g


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize('fs', zc.RATES)
def test_cases_reach_the_seams(ko, fs):
    f0, sp, ap = zc.case(fs)
    assert len(f0) == zc.FRAMES == 60 and sp.shape[1] == zc.FFT_SIZE[fs] // 2 + 1
    assert zc.FFT_SIZE[48000] == zc.FFT_SIZE[22050] == 2048 and zc.FFT_SIZE[16000] == 1024
    assert (f0[:zc.GLIDE[0]] == 0).all() and (f0[zc.HIGH[1]:] == 0).all() and zc.HIGH[1] < zc.FRAMES
    a = list(zc.APERIODIC)
    assert (f0[a] > 0).all() and (ap[a, 0] > 0.9995).all() and (f0[a] == 400.0).any() and (f0[a] != 400.0).any()
    idx, _, vuv = ko.synth_timebase(f0, fs, 5.0, zc.y_length(len(f0), fs), zc.FFT_SIZE[fs])
    d, voiced = np.diff(idx), vuv[idx[:-1]] > 0.5
    assert {255, 256, 257} <= set(d[voiced].tolist())
    assert (d[voiced] == fs // 400).any() or (d[voiced] == fs // 400 + 1).any()      # the 400 Hz stretch
    assert (d[~voiced] <= 256).all() and (~voiced).sum() > 20


@pytest.mark.parametrize('fs', zc.RATES)
def test_synthesis_bits_of_the_parent_build(golden, fs):
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    want = [golden[zc.key(fs, k)] for k in range(2)]
    for k, y in enumerate(want):
        assert y.shape == (zc.y_length(len(zc.batch(fs)[k][0]), fs),) and np.abs(y).max() > 0
    for name, got in (('single call', zc.render_single(fs, ctx)), ('batch of two', zc.render_batch(ctx, fs))):
        for k in range(2):
            assert np.array_equal(got[k], want[k]), f"{name}, utterance {k}: differs from the build at {golden['commit']}"


def test_bits_with_the_noise_from_the_generator(golden):
    """48 kHz on contexts whose randn table is cut to nothing and to the middle of the utterance: the pulses beyond it
    draw their noise inside the kernel (the generator's word sequence sits in the idle FFT buffer)"""
    from kwiiyatta_amd import _lib
    fs = 48000
    want = golden[zc.key(fs, 0)]
    for limit in (0, len(want) // 2 - 7):
        cut = _lib.Context(0)
        assert cut.set_randn_limit(limit) == limit
        assert np.array_equal(zc.render_single(fs, cut)[0], want), limit
