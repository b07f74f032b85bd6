"""The frame-parallel FFT differential filter: a numpy restatement of its contract (include/kwy.h, "frame-parallel FFT
form of the differential filter") and the cases the CPU and GPU tests share.  No test in here: test_fftfilt_cases.py
validates the restatement against the MLSA oracle, test_fftfilt_gpu.py holds the kernel to the restatement."""
import numpy as np


def fft_size(fs, hop):
    """kwy_mcep_filter_fft_size restated: max(1024, power of two >= hop + ceil(0.025 fs)), 0 beyond 8192"""
    need = hop + -(-fs // 40)
    n = 1024
    while n < need:
        n *= 2
    return n if n <= 8192 else 0


def response(mc, alpha, N, ignore_c0):
    """H[i][k] = exp(sum_{m >= m0} mc[i][m] exp(-j m w~_k)), k = 0 .. N/2"""
    m0 = 1 if ignore_c0 else 0
    w = 2 * np.pi * np.arange(N // 2 + 1) / N
    wt = w + 2 * np.arctan2(alpha * np.sin(w), 1 - alpha * np.cos(w))
    m = np.arange(m0, mc.shape[1])
    return np.exp(mc[:, m0:] @ np.exp(-1j * np.outer(m, wt)))


def fft_filter(x, mc, alpha, hop, N, ignore_c0=True):
    x = np.asarray(x, dtype=np.float64)
    mc = np.asarray(mc, dtype=np.float64)
    n, T = len(x), len(mc)
    y = np.zeros(n)
    nproc = min(T, (n - 1) // hop) if n > 0 else 0
    if nproc <= 0:
        return y
    H = response(mc[:nproc], alpha, N, ignore_c0)
    padded = np.concatenate([np.zeros(N), x])            # samples before index 0 count as zero
    u = np.arange(hop) / hop
    for i in range(nproc):
        X = np.fft.rfft(padded[(i + 1) * hop:(i + 1) * hop + N])      # x[(i+1) hop - N : (i+1) hop]
        a = np.fft.irfft(X * H[max(i - 1, 0)], N)[N - hop:]
        b = np.fft.irfft(X * H[i], N)[N - hop:]
        y[i * hop:(i + 1) * hop] = (1 - u) * a + u * b
    return y


def mcep(rng, order, scale=0.3):
    """tests/test_mlsa_codec.py's random mel-cepstrum (c0 = 0)"""
    mc = np.zeros(order + 1)
    mc[1:] = rng.standard_normal(order) * scale / np.arange(1, order + 1)
    return mc


def frames(rng, T, order, scale=0.4, c0=0.0):
    """T independently drawn frames; c0 != 0: a non-zero, slowly moving c0 column"""
    mc = np.stack([mcep(rng, order, scale) for _ in range(T)])
    if c0:
        mc[:, 0] = c0 * (1 + 0.5 * np.sin(np.arange(T)))
    return mc


# (fs, order, fft_size, hop): every transform length the kernel has, the smallest and the largest order around them
RATES = ((16000, 24, 1024, 80), (22050, 33, 1024, 110), (48000, 48, 2048, 240), (96000, 60, 4096, 480),
         (16000, 2, 8192, 80))
FRAMES = 40

# (name, n as a function of hop, T) at 16 kHz / order 24 / 1024: the edges of the processed-frames rule
EDGES = (('last frame unprocessed', lambda hop: 12 * hop - 37, 12),
         ('one sample', lambda hop: 1, 3),
         ('n == hop', lambda hop: hop, 3),
         ('n == hop + 1', lambda hop: hop + 1, 3),
         ('T == 1', lambda hop: 5 * hop, 1),
         ('T longer than the signal', lambda hop: 6 * hop + 11, 30),
         ('T shorter than the signal', lambda hop: 20 * hop + 3, 7))


def signal(rng, n):
    return rng.standard_normal(n) * 0.1
