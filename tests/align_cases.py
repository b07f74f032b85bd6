"""The alignment and training-set glue (kwy_align.hip, kwy_train.hip) stated in plain numpy and Python, and the case
lists that the CPU checks of these statements (test_align_cases.py) and the GPU tests of the kernels
(test_align_glue_gpu.py) share.  Written from the definitions in include/kwy.h and the reference call sites they cite;
nothing here imports the product.

Every operation is index, copy or fixed-expression work, so every statement is exact: the tests compare with `same`
(equal values, NaN in the same places), never with a tolerance.  Two operations compare a row's L1 norm with `eps`,
and the kernels sum a row in another order than numpy does: `eps_rows` builds rows whose sum is exact in any order
and sits at `eps`, one ulp below and one ulp above it; every other row of a case is either exactly zero or far from
`eps`."""
import itertools

import numpy as np

AL_TILE, AL_BATCH = 1024, 64                 # kwy_align.hip: cells / indices per tile, jobs per launch
TR_NT, TR_BATCH, TR_PAIRS = 256, 32, 16      # kwy_train.hip: rows per scan round, jobs and pairs per launch
EPS = 1e-7                                   # nnmnkwii's zero-frame threshold, what the corpus drivers pass
EPS_TWO = 2.0 ** -23 + 2.0 ** -25            # a threshold that two entries of a row add up to, exactly
PAD_ONE = 1 - 1e-12                          # the aperiodicity of the silence pads
POWER_WEIGHT, POWER_THRESHOLD, VUV_WEIGHT = 9.4, 1.5, 9.0


def same(a, b):
    """equal shape, dtype and values, NaN allowed where both have one"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'))


# ---- the statements ---------------------------------------------------------------------------------------------------
def align_features(mc, f0, power_weight=POWER_WEIGHT, power_threshold=POWER_THRESHOLD, vuv_weight=VUV_WEIGHT):
    """rows [power term, voicing term, c1 .. cN]: the power term is power_weight where c0 >= max(c0) -
    power_threshold, the voicing term vuv_weight where f0 > 0, both 0 elsewhere (c0 finite)"""
    out = np.zeros((len(mc), mc.shape[1] + 1))
    out[:, 0] = np.where(mc[:, 0] >= mc[:, 0].max() - power_threshold, power_weight, 0.0)
    out[:, 1] = np.where(f0 > 0, vuv_weight, 0.0)
    out[:, 2:] = mc[:, 1:]
    return out


def project(path, trim_len):
    """one x per target frame y of [trim_len, last y - trim_len]: the x of the first cell that reaches y; where the
    path jumps over target frames, x ramps from the last cell's to this cell's with floor division; a jump that
    passes the end stops at the end.  Cells whose y was reached before are passed over"""
    out = []
    end = int(path[-1][1]) + 1 - trim_len                  # first target frame that is not produced
    at_x, at_y = -1, trim_len - 1
    for x, y in ((int(c[0]), int(c[1])) for c in path):
        if y <= at_y:
            continue
        if y == at_y + 1:
            if y >= end:
                break
            out.append(x)
        else:
            y = min(y, end - 1)
            n = y - at_y
            out.extend(at_x + (x - at_x) * i // (n - 1) for i in range(n))
        at_x, at_y = x, y
    return np.array(out, dtype=np.int32)


def gather(src, idx):
    """dst[i] = src[idx[i]], an index outside [0, rows) taken as the nearest valid one"""
    return src[np.clip(np.asarray(idx, dtype=np.int64), 0, len(src) - 1)]


def frame_is_zero(rows, eps):
    """a row counts as zero when its L1 norm is below eps (a NaN row does not)"""
    return np.abs(rows).sum(axis=1) < eps


def trim_length(sp, eps=EPS):
    """frames left when the zero rows at both ends are counted off (zero rows inside stay)"""
    kept = np.flatnonzero(~frame_is_zero(sp, eps))
    return int(kept[-1] - kept[0] + 1) if len(kept) else 0


def lowest_f0(fs, K):
    return fs / ((K - 1) / 2.0) + 1.0


def is_voiced(f0, ap0, fs, K):
    """1.0 where f0 >= fs / ((K - 1) / 2) + 1 and the first aperiodicity bin is <= 0.999, else 0.0"""
    return ((f0 >= lowest_f0(fs, K)) & (ap0 <= 0.999)).astype(np.float64)


def pad(f0, n, ap_pad, pad_len, fs, with_voiced):
    """-> (f0_pad, ap_pad, voiced or None) for the first n frames of f0 between pad_len silent frames on both ends:
    ap_pad's rows behind the analysed ones become PAD_ONE, the others stay; a silent frame is unvoiced"""
    Tp = n + 2 * pad_len
    f0_pad = np.zeros(Tp)
    f0_pad[pad_len:pad_len + n] = f0[:n]
    ap_out = ap_pad.copy()
    ap_out[pad_len + n:Tp] = PAD_ONE
    voiced = None
    if with_voiced:
        a0 = np.full(Tp, PAD_ONE)
        a0[pad_len:pad_len + n] = ap_pad[pad_len:pad_len + n, 0]
        voiced = is_voiced(f0_pad, a0, fs, ap_pad.shape[1])
    return f0_pad, ap_out, voiced


def strict_filter(path, fx, fy, strict, use_power, use_vuv):
    """the path after dtw_feature's filter.  Without `strict`: the path.  With it: the first cell, the inner cells
    that pass, the last cell -- a one-cell path is then its cell twice.  An inner cell (x, y) passes when the power
    classes fx[x, 0] > 0 and fy[y, 0] > 0 agree (use_power) and the x voicing fx[x, 1] > 0 agrees with
    fy[y, 0] > 0 (use_vuv): column 0 of y, not column 1 -- that is how the reference has it"""
    path = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    if not strict:
        return path
    cells = [path[0]]
    for x, y in path[1:-1]:
        y_class = fy[y, 0] > 0
        if use_power and (fx[x, 0] > 0) != y_class:
            continue
        if use_vuv and (fx[x, 1] > 0) != y_class:
            continue
        cells.append((x, y))
    cells.append(path[-1])
    return np.array(cells, dtype=np.int64).reshape(-1, 2)


def even(path, fx, fy, strict, use_power, use_vuv, Tx, Ty, pad_len):
    """-> (xs, ys) int32: the filtered path, cut -- when pad_len > 0 -- to [begin, end): begin the first cell with
    x >= pad_len and y >= pad_len, end the first with x >= Tx - pad_len and y >= Ty - pad_len, either one 0 when no
    cell qualifies.  pad_len == 0: no cut"""
    p = strict_filter(path, fx, fy, strict, use_power, use_vuv)
    if pad_len > 0:
        def first(mask):
            hits = np.flatnonzero(mask)
            return int(hits[0]) if len(hits) else 0
        begin = first((p[:, 0] >= pad_len) & (p[:, 1] >= pad_len))
        end = first((p[:, 0] >= Tx - pad_len) & (p[:, 1] >= Ty - pad_len))
        p = p[begin:end]
    return p[:, 0].astype(np.int32), p[:, 1].astype(np.int32)


def delta(x):
    """[x | -0.5 x[t-1] + 0.0 x[t] + 0.5 x[t+1] | x[t-1] - 2 x[t] + x[t+1]] with zeros outside the rows; the three
    products are added in this order (so an infinite x[t] makes the delta of its own row NaN)"""
    x = np.asarray(x, dtype=np.float64)
    before, after = np.zeros_like(x), np.zeros_like(x)
    before[1:], after[:-1] = x[:-1], x[1:]
    with np.errstate(invalid='ignore'):
        d1 = (-0.5 * before + 0.0 * x) + 0.5 * after
        d2 = (1.0 * before + -2.0 * x) + 1.0 * after
    return np.hstack((x, d1, d2))


def joint(xd, yd, eps=EPS):
    """[xd | yd] without the rows whose L1 norm is below eps"""
    rows = np.hstack((xd, yd))
    return rows[~frame_is_zero(rows, eps)]


def train_rows(path, fx, fy, mc_x, mc_y, strict, use_power, use_vuv, pad_len, eps=EPS):
    """one pair's rows of the training matrix: filter and cut, the selected mel-cepstra without c0, their delta
    features, side by side without the zero rows"""
    xs, ys = even(path, fx, fy, strict, use_power, use_vuv, len(fx), len(fy), pad_len)
    return joint(delta(mc_x[xs][:, 1:]), delta(mc_y[ys][:, 1:]), eps)


# ---- rows around eps --------------------------------------------------------------------------------------------------
def eps_rows(K, eps):
    """-> (3 x K rows, is-zero flags): L1 norms exactly eps, one ulp below, one ulp above, each exact in any order
    of summation -- one entry, or for EPS_TWO and K >= 2 two entries (the second negative: the norm takes |.|)"""
    rows = np.zeros((3, K))
    targets = (eps, np.nextafter(eps, 0.0), np.nextafter(eps, 1.0))
    for r, v in zip(rows, targets):
        if eps == EPS_TWO and K >= 2:
            r[0], r[K - 1] = 2.0 ** -23, -(v - 2.0 ** -23)
            assert abs(r[0]) + abs(r[K - 1]) == v
        else:
            r[K // 2] = v
    return rows, np.array([False, True, False])


# ---- paths ------------------------------------------------------------------------------------------------------------
def dtw_like(rng, steps):
    """a path of steps + 1 cells from (0, 0) that moves by one in x, in y or in both"""
    kind = rng.integers(0, 3, steps)
    return np.stack([np.r_[0, np.cumsum(kind != 1)], np.r_[0, np.cumsum(kind != 0)]], 1)


def cut_gap(path, y0, missing):
    """the path without the cells of the `missing` target frames behind y0: y jumps from y0 to y0 + missing + 1"""
    return path[(path[:, 1] <= y0) | (path[:, 1] > y0 + missing)]


def project_cases():
    """name -> (path, trim_len).  The first six are the kinds of test_align_project_matches_generator; 'long' is its
    9001-cell path, for which trim_len 7 leaves 5972 indices, and the gap cases are cut out of that path"""
    def fresh():
        return np.random.default_rng(5)
    rng = fresh()
    cases = {'unit': (dtw_like(rng, 400), 7)}
    cases['unit_trim0'] = (dtw_like(fresh(), 300), 0)
    cases['gaps'] = (np.delete(dtw_like(fresh(), 400), [50, 51, 52, 200, 201, 350], axis=0), 7)
    p = dtw_like(fresh(), 300)
    p[120:125, 1] = p[119, 1] - 2
    cases['backsteps'] = (p, 7)
    cases['late_start'] = (dtw_like(fresh(), 300) + np.array([3, 4]), 7)
    long = dtw_like(fresh(), 9000)
    cases['long'] = (long, 7)
    last_y = int(long[-1, 1])
    cases['gap_1500'] = (cut_gap(long, 2000, 1500), 7)
    cases['gap_tile_plus_1'] = (cut_gap(long, 2000, AL_TILE), 7)            # y jumps by AL_TILE + 1
    cases['gap_tile_plus_2'] = (cut_gap(long, 2000, AL_TILE + 1), 7)        # AL_TILE + 1 frames missing
    cases['gap_tile'] = (cut_gap(long, 2000, AL_TILE - 1), 7)               # y jumps by exactly AL_TILE
    cases['gap_900_behind_600'] = (cut_gap(long, 7 + 600 - 1, 899), 7)      # 600 indices are out when the jump comes
    cases['gap_3000_two_flushes'] = (cut_gap(long, 1000, 3000), 7)
    cases['two_long_gaps'] = (cut_gap(cut_gap(long, 500, 1100), 3000, 1300), 7)
    cases['gap_to_end'] = (cut_gap(long, last_y - 1200, 1199), 7)           # the jump lands on the last y: clipped
    cases['gap_to_end_short'] = (cut_gap(long[:600], int(long[599, 1]) - 40, 39), 7)
    mid = dtw_like(fresh(), 2999)
    p = mid.copy()
    for k in (500, AL_TILE - 2, 2 * AL_TILE - 1, 2500):
        p[k:k + 6, 1] = p[k - 1, 1] - 3
    cases['backsteps_3000'] = (p, 7)
    cases['late_start_3000'] = (mid + np.array([3, 40]), 7)
    cases['irregular_3000_trim0'] = (np.delete(mid, [0, 1, 2, 700, 701, 1023, 1024, 1025, 2047, 2900], axis=0), 0)
    cases['one_cell_trim0'] = (np.array([[0, 0]]), 0)
    cases['one_cell_trim3'] = (np.array([[0, 0]]), 3)
    cases['one_cell_far_trim0'] = (np.array([[5, 9]]), 0)
    cases['one_cell_far_trim3'] = (np.array([[5, 9]]), 3)
    cases['last_y_below_trim'] = (dtw_like(fresh(), 20), 30)
    cases['last_y_below_trim_gaps'] = (np.delete(dtw_like(fresh(), 40), [5, 6, 20], axis=0), 60)
    return {k: (np.ascontiguousarray(v[0], dtype=np.int32), v[1]) for k, v in cases.items()}


LONG_INDICES = 5972                          # what every case cut out of 'long' yields
PROJECT_BATCH = 65                           # > AL_BATCH


def project_batch(trim_len=7):
    """65 paths for one batched call (one trim_len for all): the cases with that trim_len, then short regular and
    irregular paths"""
    paths = [p for p, t in project_cases().values() if t == trim_len]
    rng = np.random.default_rng(11)
    while len(paths) < PROJECT_BATCH:
        p = dtw_like(rng, int(rng.integers(30, 200)))
        if len(paths) % 2:
            p = np.delete(p, [10, 11, 25], axis=0)
        paths.append(np.ascontiguousarray(p, dtype=np.int32))
    return paths[:PROJECT_BATCH]


# ---- DTW feature inputs -----------------------------------------------------------------------------------------------
FEATURE_T = (1, 7, 8, 9, 300, 1100)
FEATURE_NCOEF = (1, 2, 25, 33, 40)
FEATURE_MODES = ('first', 'last', 'tied', 'edge')
F0_SPECIALS = (0.0, -0.0, 5e-324, -120.0, 150.0)


def feature_case(T, ncoef, mode, seed=0):
    """-> (mc, f0).  c0 is a multiple of 1/8 below 5, the maximum 6 sits at the first frame, the last one or
    several; 'edge' adds a frame exactly at max - POWER_THRESHOLD (kept: the test is >=) and one an ulp below it"""
    rng = np.random.default_rng([seed, T, ncoef])
    mc = rng.standard_normal((T, ncoef))
    mc[:, 0] = rng.integers(-40, 40, T) / 8.0
    where = {'first': [0], 'last': [T - 1], 'tied': [0, T // 2, T - 1], 'edge': [T // 3]}[mode]
    mc[where, 0] = 6.0
    if mode == 'edge' and T >= 7:
        mc[T // 3 + 1, 0] = 6.0 - POWER_THRESHOLD
        mc[T // 3 + 2, 0] = np.nextafter(6.0 - POWER_THRESHOLD, -np.inf)
    f0 = np.where(rng.random(T) < 0.5, 0.0, rng.uniform(70, 400, T))
    special = np.array(F0_SPECIALS)
    f0[:min(T, len(special))] = special[(np.arange(min(T, len(special))) + seed) % len(special)]
    return np.ascontiguousarray(mc), f0


# ---- trim / joint inputs ----------------------------------------------------------------------------------------------
TRIM_T = (1, 3, 4, 5, 256, 257, 700)
TRIM_K = (1, 63, 64, 65, 513)
TRIM_KINDS = ('zeros', 'first', 'last', 'runs', 'nan', 'eps', 'eps_two')


def trim_case(T, K, kind, seed=0):
    """-> (sp, eps).  Rows are exactly zero or a row of 1/8s, except the NaN row and the rows around eps"""
    sp = np.zeros((T, K))
    eps = EPS_TWO if kind == 'eps_two' else EPS
    full = np.full(K, 0.125)
    if kind == 'first':
        sp[0] = full
    elif kind == 'last':
        sp[T - 1] = full
    elif kind == 'runs':                                     # zero runs at both ends, zero rows inside
        a, b = T // 5, T - 1 - T // 4
        sp[a:b + 1] = full
        sp[a + 1:b:3] = 0.0
    elif kind == 'nan':                                      # the NaN row ends the leading run
        sp[T // 3, K // 2] = np.nan
        sp[T // 2] = full
    elif kind in ('eps', 'eps_two'):                         # [below, at, ..., zero, above, below]
        rows, _ = eps_rows(K, eps)
        order = [1, 0] + [None] * max(T - 5, 0) + [None, 2, 1]
        order = order[:T] if T < 5 else order
        for t, r in enumerate(order):
            if r is not None:
                sp[t] = rows[r]
        if T >= 7:
            sp[T // 2] = full
    return sp, eps


JOINT_N = (0, 1, 63, 64, 65, 256, 257, 600)
JOINT_W = (1, 64, 65, 72, 144)
JOINT_KINDS = ('marks', 'all_dropped', 'none_dropped', 'nan_eps', 'nan_eps_two')


def joint_case(n, w, kind, seed=0):
    """-> (xd, yd, eps), n x w each.  'marks': zero rows at the first and last position, at the multiples of 64 and
    256 and in runs across the rounds' ends; 'nan_eps': a NaN row and the three rows around eps among zero rows"""
    rng = np.random.default_rng([seed, n, w])
    xd, yd = rng.standard_normal((n, w)) + 3.0, rng.standard_normal((n, w)) - 3.0
    eps = EPS_TWO if kind == 'nan_eps_two' else EPS
    if kind == 'marks':
        zero = [t for t in range(n) if t in (0, n - 1) or t % 64 == 0 or 250 <= t < 262 or 509 <= t < 515]
        xd[zero], yd[zero] = 0.0, 0.0
    elif kind == 'all_dropped':
        xd[:], yd[:] = 0.0, 0.0
    elif kind in ('nan_eps', 'nan_eps_two'):
        rows, _ = eps_rows(2 * w, eps)
        xd[1::2], yd[1::2] = 0.0, 0.0
        for k, t in enumerate(range(0, min(n, 3))):          # first rows; again around a round's end when n allows
            xd[t], yd[t] = rows[k, :w], rows[k, w:]
        for k, t in enumerate(range(254, min(n, 257))):
            xd[t], yd[t] = rows[k, :w], rows[k, w:]
        if n > 5:
            xd[5] = 0.0
            yd[5] = 0.0
            yd[5, w - 1] = np.nan
    return xd, yd, eps


# ---- voicing / pad inputs ---------------------------------------------------------------------------------------------
VOICED_SHAPES = ((16000, 513), (48000, 1025), (8000, 3))
PAD_N = (0, 1, 300)
PAD_LEN = (0, 1, 100, 300)                  # 300 > ceil((n + 600) / 256); 1 < ceil(302 / 256) for n = 300


def voiced_case(fs, K, T=300, seed=0):
    """-> (f0, ap): the nine combinations of f0 at the lowest voiced f0 and an ulp around it with ap[:, 0] at 0.999 and
    an ulp around it come first (as far as T goes), random frames behind"""
    rng = np.random.default_rng([seed, fs, K, T])
    low = lowest_f0(fs, K)
    f0 = np.where(rng.random(T) < 0.4, 0.0, rng.uniform(low - 30, low + 200, T))
    ap = rng.uniform(0.0, 1.0, (T, K))
    ap[rng.random(T) < 0.3, 0] = PAD_ONE
    edges = list(itertools.product((low, np.nextafter(low, 0), np.nextafter(low, np.inf)),
                                   (0.999, np.nextafter(0.999, 0), np.nextafter(0.999, 1))))
    for t, (f, a) in enumerate(edges[:T]):
        f0[t], ap[t, 0] = f, a
    return f0, ap


# ---- filter / cut inputs ----------------------------------------------------------------------------------------------
EVEN_CELLS = (1, 2, 3, 255, 256, 257, 1300)
FLAGS = tuple(itertools.product((0, 1), repeat=3))          # (strict, use_power, use_vuv)


def class_features(rng, T, width):
    """T x width DTW-feature-like rows: column 0 is 9.4 or 0, column 1 is 9.0 or 0, and the two disagree on about
    half of the frames -- a filter that read y's column 1 in the voicing test would keep other cells"""
    f = rng.standard_normal((T, width))
    f[:, 0] = np.where(rng.random(T) < 0.6, POWER_WEIGHT, 0.0)
    f[:, 1] = np.where(rng.random(T) < 0.5, VUV_WEIGHT, 0.0)
    return f


def even_case(cells, seed=0, width=4):
    """-> (path, fx, fy) for a DTW-shaped path of `cells` cells over all frames of fx and fy"""
    rng = np.random.default_rng([seed, cells])
    path = dtw_like(rng, cells - 1).astype(np.int32)
    Tx, Ty = int(path[-1, 0]) + 1, int(path[-1, 1]) + 1
    return path, class_features(rng, Tx, width), class_features(rng, Ty, width)


BOUNDARY_DROPS = (1, 63, 64, 65, 127, 128, 191, 192, 254, 255, 256, 257, 511, 512, 513, 767, 768, 1023, 1024, 1279,
                  1280, 1281, 1298)


def even_boundary_case(cells=1300, width=4):
    """a diagonal path (cell v = frames (v, v)) on features that agree everywhere but at BOUNDARY_DROPS, and at a run
    across the second round's end: exactly those cells are dropped by the power test"""
    v = np.arange(cells, dtype=np.int32)
    path = np.stack([v, v], 1)
    fx, fy = np.ones((cells, width)), np.ones((cells, width))
    drop = sorted(set(BOUNDARY_DROPS) | set(range(505, 520)))
    fy[drop, 0] = 0.0
    return np.ascontiguousarray(path), fx, fy, drop


def even_cut_cases():
    """(name, path, fx, fy, pad_len) whose cut comes out empty under every flag combination: nothing reaches the
    un-padded stretch (begin = end = 0); the signal is reached but the trailing pad is not (begin > end = 0); pads
    longer than half the frames (end before begin, end at begin); one cell with a cut"""
    rng = np.random.default_rng(3)
    v = np.arange(40, dtype=np.int32)
    diag = np.ascontiguousarray(np.stack([v, v], 1))
    fx, fy = class_features(rng, 40, 4), class_features(rng, 40, 4)
    return [('begin = end = 0', diag[:7], fx, fy, 8), ('begin > end = 0', diag[:20], fx, fy, 8),
            ('end < begin', diag, fx, fy, 30), ('end = begin', diag, fx, fy, 20),
            ('one cell, cut', diag[:1], fx[:1], fy[:1], 3)]


# ---- training pairs ---------------------------------------------------------------------------------------------------
def train_pair(steps, d, seed):
    """-> (path, fx, fy, mc_x, mc_y): a DTW-shaped path, class features and mel-cepstra whose first frames (15, or a third of a short
    side) are zero on both sides, so that some joint rows are zero rows"""
    rng = np.random.default_rng([seed, steps, d])
    path = dtw_like(rng, steps).astype(np.int32)
    Tx, Ty = int(path[-1, 0]) + 1, int(path[-1, 1]) + 1
    fx, fy = class_features(rng, Tx, d + 2), class_features(rng, Ty, d + 2)
    mc_x, mc_y = rng.standard_normal((Tx, d + 1)), rng.standard_normal((Ty, d + 1))
    mc_x[:min(15, Tx // 3), 1:], mc_y[:min(15, Ty // 3), 1:] = 0.0, 0.0
    return np.ascontiguousarray(path), fx, fy, mc_x, mc_y


TRAIN_STEPS = (40, 700, 1, 90, 300, 2, 33, 256, 511, 64, 120, 0, 75, 410, 57, 130, 29)   # 17 pairs > TR_PAIRS
