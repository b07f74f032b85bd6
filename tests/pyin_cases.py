"""numpy model of the pYIN estimator (include/kwy.h, "probabilistic YIN", steps 1 - 7) and the inputs its tests share.

The model forms the difference function by direct sums.  `dtype=LD` runs steps 1 - 6 in np.longdouble, `form='fft'`
forms step 2 the way the kernel does (e(0) + e(tau) - 2 r(tau) with numpy's FFT): the two deviations of the float64
model that set the tests' bound.  Every frame also reports how close its own decisions (local-minimum tests,
running-minimum tests, bin boundaries, the 2^-40 floor) came to their edges."""
import math
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from conftest import CLB_WAV, clb_variant

LD = np.longdouble
BPO = 120
TINY = 1e-300
P_A, SWITCH, MAX_RATE = 0.01, 0.01, 35.92


class Params:
    def __init__(self, fs, f0_floor=71.0, f0_ceil=800.0, frame_period=5.0):
        self.fs, self.f0_floor, self.f0_ceil, self.frame_period = fs, float(f0_floor), float(f0_ceil), float(frame_period)
        self.tau_min = int(math.floor(fs / self.f0_ceil))
        self.tau_max = int(math.ceil(fs / self.f0_floor))
        self.W = self.tau_max + 1
        self.nb = int(math.ceil(BPO * np.log2(self.f0_ceil / self.f0_floor)))
        self.R = int(math.ceil(MAX_RATE * BPO * self.frame_period / 1000.0))
        self.N = 1024
        while self.N < 2 * self.W:
            self.N *= 2

    def kwargs(self):
        return dict(f0_floor=self.f0_floor, f0_ceil=self.f0_ceil, frame_period=self.frame_period)


def n_frames(n, fs, frame_period):
    return int(1000.0 * n / fs / frame_period) + 1


def frame_of(x, i, p):
    """x[c - W .. c + W) with zeros outside the signal, c = floor(t_i fs + 0.5)"""
    c = int(math.floor(i * p.frame_period / 1000.0 * p.fs + 0.5))
    out = np.zeros(2 * p.W)
    lo, hi = c - p.W, c + p.W
    a, b = max(lo, 0), min(hi, len(x))
    if b > a:
        out[a - lo:b - lo] = x[a:b]
    return out


def difference_direct(fr, W, dtype=np.float64):
    """(d, s): d(tau) = sum_{j < W} (x_j - x_{j + tau})^2 and s(tau) = e(0) + e(tau), tau <= W"""
    f = np.asarray(fr, dtype=dtype)
    win = sliding_window_view(f, W)[:W + 1]                 # win[tau, j] = x[j + tau]
    diff = win - f[None, :W]
    d = (diff * diff).sum(axis=1)
    e = (win * win).sum(axis=1)
    return d, e[0] + e


def difference_fft(fr, W, N):
    """the kernel's form in float64: e(0) + e(tau) - 2 r(tau), the 2^-40 floor applied"""
    a = np.zeros(N)
    a[:W] = fr[:W]
    b = np.zeros(N)
    b[:2 * W] = fr
    r = np.fft.irfft(np.conj(np.fft.rfft(a)) * np.fft.rfft(b), N)[:W + 1]
    sq = fr * fr
    e = np.concatenate([[sq[:W].sum()], sq[:W].sum() + np.cumsum(sq[W:2 * W] - sq[:W])])
    s = e[0] + e
    d = s - 2.0 * r
    d[(d < 2.0 ** -40 * s) | (d < 0)] = 0.0
    return d, s


def prior_cdf(v):
    """F(v) = 1 - (1 - v)^18 (1 + 18 v), the powers by squaring as the kernel forms them"""
    v = min(max(v, type(v)(0)), type(v)(1))
    u = 1 - v
    u2 = u * u
    u4 = u2 * u2
    u8 = u4 * u4
    u16 = u8 * u8
    return 1 - (u16 * u2) * (1 + 18 * v)


# 1 - F(V0) = 2.4e-14: a candidate whose trough lies above V0 moves less probability than the least deviation the tests
# allow for (2^-52 tau_max = 5.0e-14 at 16 kHz), unless it is the only kind the frame has (then p_a F(m) goes to it)
V0 = 0.85


class Frame:
    """steps 2 - 6 of one frame: p (nb masses), the candidates, and the margin of the frame's closest decision:
    a local-minimum test (two values of d' next to each other), a running-minimum test (v against m), a bin boundary
    (in units of d'), the floor of d.  Not edges: two floored zeros, two troughs above V0 beside one below it, and
    d' = 1 = 1 in a frame whose first half is silent (its sums are exact)."""


def observe_frame(fr, p, dtype=np.float64, form='direct', p_a=P_A):
    one = dtype(1)
    if form == 'fft':
        d, s = difference_fft(fr, p.W, p.N)
    else:
        d, s = difference_direct(fr, p.W, dtype)
    draw = d
    if form != 'fft':
        d = np.where(d < dtype(2.0 ** -40) * s, dtype(0), d)
    cum = np.cumsum(d[1:])
    dp = np.ones(p.W + 1, dtype=dtype)
    taus = np.arange(1, p.W + 1)
    nz = cum != 0
    dp[1:][nz] = (d[1:] * taus.astype(dtype))[nz] / cum[nz]
    lo = max(p.tau_min, 1)
    out = Frame()
    cands = []
    m = one
    masses, setters, tests = [], [], []
    last = None
    for tau in range(lo, p.tau_max + 1):
        a, b, c = dp[tau - 1], dp[tau], dp[tau + 1]
        if not (b < a and b <= c):
            continue
        den = a - 2 * b + c
        off, v = dtype(0), b
        if den > 0:
            off = dtype(0.5) * (a - c) / den
            v = b - dtype(0.25) * (a - c) * off
        if v < 0:
            v = dtype(0)
        tests.append((float(v), float(m)))
        mass = dtype(0)
        if v < m:
            mass = prior_cdf(m) - prior_cdf(v)
            m = v
            last = len(cands)
            setters.append(last)
        cands.append((tau, off, v, float(den)))
        masses.append(mass)
    if last is not None:
        masses[last] = masses[last] + dtype(p_a) * prior_cdf(cands[last][2])
    pb = np.zeros(p.nb, dtype=dtype)
    bins, edges = [], []
    for (tau, off, v, den), mass in zip(cands, masses):
        f = dtype(p.fs) / (tau + off)
        y = BPO * np.log2(f / dtype(p.f0_floor))
        b = int(np.floor(y))
        bins.append(b)
        if mass > 0:
            # the change of the three points that moves the trough across the nearest bin boundary, roughly
            dy = min(float(y - np.floor(y)), float(np.floor(y) + 1 - y))
            edges.append(dy * (tau * math.log(2.0) / BPO) * max(den, 0.0))
        if 0 <= b < p.nb:
            pb[b] = pb[b] + mass
    out.p = pb
    out.unvoiced = (one - pb.sum()) / p.nb
    out.taus = [cd[0] for cd in cands]
    out.setters = setters
    out.bins = bins
    low = [i for i in setters if cands[i][2] < V0]
    out.relevant = [(cands[i][0], bins[i]) for i in (low or setters)]
    # ---- how close the frame's decisions came to their edges
    margin = min(edges) if edges else np.inf
    if ((draw > dtype(2.0 ** -42) * s) & (draw < dtype(2.0 ** -38) * s)).any():
        margin = 0.0                                        # the floor
    k = np.arange(max(lo - 1, 1), p.tau_max + 1)           # local-minimum tests
    if len(k):
        gap = np.abs(dp[k + 1] - dp[k]).astype(np.float64)
        live = ~((d[k] == 0) & (d[k + 1] == 0))
        if low:
            live &= ~((dp[k] >= V0) & (dp[k + 1] >= V0))
        if s[0] == 0:
            live &= ~((dp[k] == 1) & (dp[k + 1] == 1))
        if live.any():
            margin = min(margin, float(gap[live].min()))
    for v, mb in tests:                                     # running-minimum tests
        if (v == 0 and mb == 0) or (low and v >= V0):
            continue
        margin = min(margin, abs(v - mb))
    out.margin = margin
    return out


def observe(x, p, dtype=np.float64, form='direct', p_a=P_A, stride=1):
    """[Frame] of every frame of x; stride > 1: of every stride-th frame, None for the others"""
    x = np.asarray(x, dtype=np.float64)
    return [observe_frame(frame_of(x, i, p), p, dtype, form, p_a) if i % stride == 0 else None
            for i in range(n_frames(len(x), p.fs, p.frame_period))]


def probabilities(frames, p):
    """(T, nb + 1) float64: what exp(L) approximates, without the 1e-300 floor"""
    return np.array([np.concatenate([np.asarray(f.p, dtype=np.float64), [float(f.unvoiced)]]) for f in frames])


def log_matrix(frames, p):
    """L (T, nb + 1) of the float64 model"""
    return np.ascontiguousarray(np.log(np.maximum(probabilities(frames, p), TINY)))


def same_decisions(fa, fb):
    """the candidates that carry probability (those that lowered the running minimum; where one of them lies below V0,
    only those below it) are the same lags in the same bins"""
    return fa.relevant == fb.relevant


def transition_table(R, switch=SWITCH):
    k = np.abs(np.arange(-R, R + 1))
    w = (R + 1 - k) / float((R + 1) * (R + 1))
    return np.concatenate([np.log(w * (1.0 - switch)), np.log(w * switch)])


def bin_frequencies(nb, f0_floor=71.0):
    return np.array([f0_floor * math.pow(2.0, (b + 0.5) / BPO) for b in range(nb)])


def decode(L, trans, freq):
    """step 7: (track, states, delta of the last frame); the first of equal maxima wins throughout"""
    L = np.asarray(L, dtype=np.float64)
    T, nb = L.shape[0], L.shape[1] - 1
    R = len(trans) // 4
    n = 2 * R + 1
    tr_same, tr_other = trans[:n], trans[n:]
    obs = np.concatenate([L[:, :nb], np.repeat(L[:, nb:], nb, axis=1)], axis=1)
    delta = obs[0].copy()
    pad = np.full(R, -np.inf)
    back = np.zeros((T, 2 * nb), dtype=np.int64)
    for t in range(1, T):
        wv = sliding_window_view(np.concatenate([pad, delta[:nb], pad]), n)      # [b, j] = delta_voiced[b - R + j]
        wu = sliding_window_view(np.concatenate([pad, delta[nb:], pad]), n)
        allv = np.concatenate([np.concatenate([wv + tr_same, wu + tr_other], axis=1),
                               np.concatenate([wu + tr_same, wv + tr_other], axis=1)], axis=0)
        code = np.argmax(allv, axis=1)
        back[t] = code
        delta = allv[np.arange(2 * nb), code] + obs[t]
    s = int(np.argmax(delta))
    states = np.empty(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        if t == 0:
            break
        code = back[t, s]
        voiced = s < nb
        b = (s if voiced else s - nb) - R + code % n
        prev_voiced = voiced != (code >= n)
        s = b if prev_voiced else b + nb
    track = np.where(states < nb, freq[np.minimum(states, nb - 1)], 0.0)
    return track, states, delta


def model(x, p, p_a=P_A, switch=SWITCH):
    """the coarse track of the float64 model, its L and the frames"""
    frames = observe(x, p, p_a=p_a)
    L = log_matrix(frames, p)
    track, states, _ = decode(L, transition_table(p.R, switch), bin_frequencies(p.nb, p.f0_floor))
    return track, L, frames


# ---- inputs ------------------------------------------------------------------------------------------------------
def glide(fs):
    """input G: 0.4 s of sum_{h <= 10} sin(h phi) / h with f0 rising exponentially from 120 to 240 Hz between 0.1 s of
    zeros, plus 1e-3 white noise"""
    n_tone, n_pad = int(0.4 * fs), int(0.1 * fs)
    t = np.arange(n_tone) / fs
    f0 = 120.0 * 2.0 ** (t / 0.4)
    phi = 2 * np.pi * np.cumsum(f0) / fs
    tone = sum(np.sin(h * phi) / h for h in range(1, 11))
    x = np.concatenate([np.zeros(n_pad), tone, np.zeros(n_pad)])
    return x + 1e-3 * np.random.default_rng(0).standard_normal(len(x)), f0


def glide_f0_at(times):
    """the generating f0 at `times` (seconds from the start of G)"""
    return 120.0 * 2.0 ** ((np.asarray(times) - 0.1) / 0.4)


def speech(suffix=None):
    """input S: samples 0.3 s .. 0.9 s of arctic_a0001 (suffix '96': the 96 kHz copy) -> (x, fs)"""
    from scipy.io import wavfile
    fs, data = wavfile.read(CLB_WAV if suffix is None else clb_variant(suffix))
    x = data.astype(np.float64) / (32768.0 if data.dtype == np.int16 else 1.0)
    return np.ascontiguousarray(x[int(0.3 * fs):int(0.9 * fs)]), fs


def sine(freq, fs, seconds=0.3):
    return np.sin(2 * np.pi * freq * np.arange(int(seconds * fs)) / fs)


def edge_cases():
    """name -> (x, Params)"""
    fs = 16000
    d = Params(fs)
    g, _ = glide(fs)
    short = g[int(0.2 * fs):int(0.2 * fs) + 150]                     # shorter than W = 227
    click = np.zeros(800)
    click[300] = 0.7
    return {
        'zeros': (np.zeros(1600), d),
        'constant': (np.full(1600, 0.5), d),
        'one_sample': (np.array([0.25]), d),
        'click': (click, d),
        'short': (np.ascontiguousarray(short), d),
        'sine_floor': (sine(71.0, fs), d),
        'sine_ceil': (sine(800.0, fs), d),
        'period_1ms': (np.ascontiguousarray(g[int(0.25 * fs):int(0.35 * fs)]), Params(fs, frame_period=1.0)),
        'period_10ms': (np.ascontiguousarray(g[:int(0.6 * fs)]), Params(fs, frame_period=10.0)),
        'range_50_400': (np.ascontiguousarray(g[:int(0.4 * fs)]), Params(fs, f0_floor=50.0, f0_ceil=400.0)),
    }


def cents(f, ref):
    return 1200.0 * np.abs(np.log2(np.asarray(f) / np.asarray(ref)))
