"""The waveform pitch shifter stated in numpy -- the yardstick of tests/test_pitch_cases.py (its own claims), of
tests/test_pitch_gpu.py (the kernels of kwy_pitch.hip against it) and the stand-in of the oracle backend in
tests/test_pitch_convert.py -- and the generators of their inputs.

x: N float64 samples, xb: x extended with zeros on both sides, rate within [0.5, 2.0]; int64 index arithmetic.

    constants   H = int(fs * 0.010), L = 2 H, S = H;  M = floor(N rate + 0.5);  K = ceil(M / H) frames (0 for M = 0)
    positions   p_0 = 0;  a_k = (k H N + M // 2) // M;  candidates q in [lo, hi], lo = min(max(a_k - S, 0), N - 1),
                hi = min(a_k + S, N - 1);  t[i] = xb[p_{k-1} + H + i], i < L;  d(q) = sum_i (xb[q + i] - t[i])^2;
                p_k = the q of the smallest d, ties to the smallest |q - a_k|, then to the smaller q
    stretch     s[n] = xb[i] for k = 0, else a + w_i (b - a), a = xb[p_{k-1} + H + i], b = xb[p_k + i],
                w_i = 0.5 - 0.5 cos(2 pi i / L)                                  (k = n // H, i = n % H, n < M)
    resample    M == N: y = s.  Else c = min(1, N / M), W = 32 / c, base = (n M) // N, frac = ((n M) % N) / N,
                y[n] = sum_j s[base + j] g(frac - j) over 0 <= base + j < M and |frac - j| < W,
                g(t) = c sinc(c t) bh(t / W),  bh(u) = 0.35875 + 0.48829 cos(pi u) + 0.14128 cos(2 pi u)
                + 0.01168 cos(3 pi u)

`positions`, `stretch`, `resample`, `shift_pitch`; `step_distances` gives the candidates of one step and their d."""
import numpy as np

U = 2.0 ** -53            # unit roundoff of float64
ZEROS = 32
RATES = (0.5, 0.8909, 1.4983, 2.0)


def constants(n, fs, rate):
    """(H, L, S, M, K)"""
    H = int(fs * 0.010)
    M = int(np.floor(n * rate + 0.5))
    return H, 2 * H, H, M, (M + H - 1) // H if M > 0 else 0


def _xb(x, start, count):
    """xb[start : start + count] of the zero-extended signal"""
    out = np.zeros(count)
    lo, hi = max(start, 0), min(start + count, len(x))
    if hi > lo:
        out[lo - start:hi - start] = x[lo:hi]
    return out


def ideal_position(k, n, fs, rate):
    H, _, _, M, _ = constants(n, fs, rate)
    return (k * H * n + M // 2) // M


def step_distances(x, fs, k, p_prev, rate=None, reverse=False, M=None):
    """(q, d, a_k): the candidates of step k >= 1 given p_{k-1}, and their distances.  rate (or M) fixes a_k.
    The squares are added pairwise from the first on (numpy's sum); reverse=True adds them one by one from the last
    to the first (a strict fold)"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    H = int(fs * 0.010)
    L, S = 2 * H, H
    if M is None:
        M = int(np.floor(n * rate + 0.5))
    a = (k * H * n + M // 2) // M
    lo, hi = min(max(a - S, 0), n - 1), min(a + S, n - 1)
    q = np.arange(lo, hi + 1, dtype=np.int64)
    t = _xb(x, p_prev + H, L)
    w = _xb(x, lo, hi - lo + L)
    frames = np.lib.stride_tricks.sliding_window_view(w, L)[:len(q)]
    e = (frames - t) ** 2
    d = e[:, ::-1].cumsum(axis=1)[:, -1] if reverse else e.sum(axis=1)
    return q, d, a


def choose(q, d, a):
    """the tie rule: smallest d, then smallest |q - a|, then the smaller q"""
    best = np.flatnonzero(d == d.min())
    cand = q[best]
    off = np.abs(cand - a)
    return int(cand[off == off.min()].min())


def positions(x, fs, rate, reverse=False):
    """the K positions p_k (int64)"""
    x = np.asarray(x, dtype=np.float64)
    _, _, _, M, K = constants(len(x), fs, rate)
    p = np.zeros(K, dtype=np.int64)
    for k in range(1, K):
        q, d, a = step_distances(x, fs, k, int(p[k - 1]), M=M, reverse=reverse)
        p[k] = choose(q, d, a)
    return p


def _stretch_parts(x, fs, p, M):
    """(a, b, w) per stretched sample: s = a + w (b - a); frame 0 has a = b = xb[i]"""
    x = np.asarray(x, dtype=np.float64)
    H = int(fs * 0.010)
    L = 2 * H
    n = np.arange(M, dtype=np.int64)
    k, i = n // H, n % H
    p = np.asarray(p, dtype=np.int64)
    xz = np.concatenate((x, np.zeros(3 * H + 1)))        # indices beyond the end read zero; none is negative
    first = k == 0
    km = np.where(first, 0, k - 1)
    ia = np.where(first, i, p[km] + H + i) if M else n
    ib = np.where(first, i, p[np.where(first, 0, k)] + i) if M else n
    ia, ib = np.minimum(ia, len(xz) - 1), np.minimum(ib, len(xz) - 1)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * i / L)
    return xz[ia], xz[ib], w


def stretch(x, fs, p, M):
    """the M stretched samples for the positions p"""
    a, b, w = _stretch_parts(x, fs, p, M)
    return a + w * (b - a)


CHUNK = 4096


def _taps(n_out, M, lo=0, hi=None):
    """(index (n, J), valid (n, J), sinc, bh, c) of the resampling sum for the outputs lo <= n < hi"""
    c = min(1.0, n_out / M)
    W = ZEROS / c
    reach = int(np.ceil(W))
    n = np.arange(lo, n_out if hi is None else min(hi, n_out), dtype=np.int64)
    base, frac = (n * M) // n_out, ((n * M) % n_out) / n_out
    j = np.arange(-reach, reach + 1, dtype=np.int64)
    t = frac[:, None] - j[None, :]
    idx = base[:, None] + j[None, :]
    valid = (idx >= 0) & (idx < M) & (np.abs(t) < W)
    u = c * t
    pu = np.pi * u
    with np.errstate(invalid='ignore', divide='ignore'):
        sinc = np.where(u == 0, 1.0, np.sin(pu) / pu)
    v = t / W
    bh = 0.35875 + 0.48829 * np.cos(np.pi * v) + 0.14128 * np.cos(2 * np.pi * v) + 0.01168 * np.cos(3 * np.pi * v)
    return np.clip(idx, 0, max(M - 1, 0)), valid, sinc, bh, c


def resample(s, n_out):
    """s (M samples) -> n_out samples"""
    s = np.asarray(s, dtype=np.float64)
    M = len(s)
    if M == n_out:
        return s.copy()
    y = np.zeros(n_out)
    if M == 0:
        return y
    for lo in range(0, n_out, CHUNK):
        idx, valid, sinc, bh, c = _taps(n_out, M, lo, lo + CHUNK)
        g = np.where(valid, c * sinc * bh, 0.0)
        y[lo:lo + CHUNK] = (s[idx] * g).sum(axis=1)
    return y


def shift_pitch(x, fs, rate, with_positions=False):
    """y (N samples, the pitch of x times rate) -- and the positions"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if not 0.5 <= rate <= 2.0:
        raise ValueError(f'pitch shift: rate {rate!r} is outside [0.5, 2.0]')
    _, _, _, M, _ = constants(len(x), fs, rate)
    p = positions(x, fs, rate)
    y = resample(stretch(x, fs, p, M), len(x))
    return (y, p) if with_positions else y


# ---- bounds (reasoned from the number format and the operation count, not measured) --------------------------------
def distance_slack(fs):
    """a sum of L non-negative terms, each a rounded square of a rounded difference, carries a relative error of at
    most (L + 2) U whatever its order; two such sums (kernel, yardstick) that compare equal in exact arithmetic may
    therefore differ by the factor 1 + 2 (L + 2) U"""
    return 2 * (2 * int(fs * 0.010) + 2) * U


def waveform_bound(x, fs, p, n_out, M):
    """per output sample, the bound of |kernel - resample(stretch(x, p))|, both in float64 with their own sin / cos:
        U * sum_j A_j ((taps + 16) |g_j| + 8 c bh_j + 20 c |sinc_j|),        A_j = |a_j| + |b_j| >= |s_j|, |b_j - a_j|
    - (taps + 16) |g_j|: a sum of `taps` rounded products in any order (taps U), the products of g = c sinc bh (3 U), the
      roundings of s = a + w (b - a) (3 U) and of the weight w on both sides (cos of a rounded argument: <= 8 U of
      |b - a|), rounded up;
    - 8 c bh_j: sin(pi u) of the rounded argument pi u is off by |pi u| 2 U + 2 U in absolute terms, on both sides;
      divided by pi |u| that is an ABSOLUTE 4 U .. 8 U of sinc, which matters where sinc is near a zero;
    - 20 c |sinc_j|: the cosines of bh (arguments up to 3 pi, rounded: <= 6 U of the weighted sum), the kernel's
      double- and triple-angle forms (<= 2 U) and four additions, on both sides: an ABSOLUTE 20 U of bh, which matters
      at the ends of the window, where bh falls to 6e-5.
    M == n_out copies s: only the (taps + 16) term with one tap."""
    a, b, _ = _stretch_parts(x, fs, p, M)
    A = np.abs(a) + np.abs(b)
    if M == n_out:
        return 17 * U * A
    bound = np.zeros(n_out)
    for lo in range(0, n_out, CHUNK):
        idx, valid, sinc, bh, c = _taps(n_out, M, lo, lo + CHUNK)
        taps = valid.sum(axis=1)
        per_tap = (taps[:, None] + 16) * np.abs(c * sinc * bh) + 8 * c * np.abs(bh) + 20 * c * np.abs(sinc)
        bound[lo:lo + CHUNK] = U * (A[idx] * np.where(valid, per_tap, 0.0)).sum(axis=1)
    return bound


# ---- measures and generators ------------------------------------------------------------------------------------------
def f0_ratio(f0_in, f0_out):
    """(median of f0_out / f0_in over the frames both tracks voice, share of those frames)"""
    n = min(len(f0_in), len(f0_out))
    a, b = np.asarray(f0_in[:n]), np.asarray(f0_out[:n])
    both = (a > 0) & (b > 0)
    if not both.any():
        return float('nan'), 0.0
    return float(np.median(b[both] / a[both])), float(both.mean())


def load(path):
    """(fs, float64 samples) of a 16-bit wav fixture"""
    from scipy.io import wavfile
    fs, pcm = wavfile.read(path)
    return int(fs), np.ascontiguousarray(pcm.astype(np.float64) / 32768.0)
