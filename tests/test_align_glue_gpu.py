"""The alignment and training-set glue kernels (kwy_align.hip, kwy_train.hip) on the MI355X, through the C ABI, against
their numpy statements (tests/align_cases.py) at the edges of their tiles: AL_TILE 1024 cells and indices, AL_BATCH 64
jobs, TR_NT 256 rows a round, TR_BATCH 32 jobs, TR_PAIRS 16 pairs, 64 rows per wavefront.

Every comparison is exact (`ac.same`: equal values, NaN in the same places): these are index, copy and fixed-expression
kernels, no tolerance appears.  Every output buffer is uploaded full of a sentinel and comes back whole, so that what
lies outside the documented extent -- rows beyond n_out, indices beyond the capacity, ap_pad's head rows, joint rows
before the cursor -- is seen to be untouched.  Every batched entry is also compared with the single entry, job by job.
Buffers are made on the host and uploaded (complete on return); results are read after the context's stream is done."""
import numpy as np
import pytest

import align_cases as ac

pytestmark = pytest.mark.gpu

I_SENT = -77                    # sentinel of index and count buffers
F_SENT = -7.25                  # sentinel of double buffers
GUARD = 16                      # sentinel elements / rows behind every output


class Glue:
    """uploads, the calls, read-back"""

    def __init__(self):
        import torch
        from kwiiyatta_amd import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.lib
        self.dev = torch.device('cuda', 0)
        self.ctx = _lib.Context(0)
        self.OK, self.EINVAL = _lib.KWY_OK, _lib.KWY_EINVAL

    def up(self, a, dtype=None):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)

    def fill(self, shape, value, dtype=np.float64):
        return self.up(np.full(shape, value, dtype=dtype))

    def down(self, *tensors):
        self.ctx.sync()
        out = [t.cpu().numpy() for t in tensors]
        return out[0] if len(out) == 1 else out

    def call(self, name, *args):
        """-> the status of lib.<name>(ctx, ...): tensors go as their device pointers, None as NULL"""
        return getattr(self.lib, name)(self.ctx.handle, *[a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args])

    def ok(self, name, *args):
        rc = self.call(name, *args)
        assert rc == self.OK, (name, rc, self.ctx.error())

    def jobs(self, struct, rows):
        return self._lib.job_array(getattr(self._lib, struct), rows)


@pytest.fixture(scope='module')
def g():
    return Glue()


def untouched(buf, sentinel=None):
    sentinel = (I_SENT if buf.dtype.kind == 'i' else F_SENT) if sentinel is None else sentinel
    return bool((buf == sentinel).all())


# ---- kwy_align_features(_batch)_dev -----------------------------------------------------------------------------------
def _features_single(g, mc, f0):
    T, ncoef = mc.shape
    out = g.fill((T + GUARD, ncoef + 1), F_SENT)
    g.ok('kwy_align_features_dev', g.up(mc), T, ncoef, g.up(f0), ac.POWER_WEIGHT, ac.POWER_THRESHOLD, ac.VUV_WEIGHT, out)
    out = g.down(out)
    assert untouched(out[T:]), (T, ncoef)
    return out[:T]


def test_features_against_the_statement(g):
    for T in ac.FEATURE_T:
        for ncoef in ac.FEATURE_NCOEF:
            for mode in ac.FEATURE_MODES:
                mc, f0 = ac.feature_case(T, ncoef, mode)
                assert ac.same(_features_single(g, mc, f0), ac.align_features(mc, f0)), (T, ncoef, mode)


def test_features_batch_of_65_ragged_jobs(g):
    Ts = [(1, 300, 7, 8, 9, 1100, 1, 2, 63)[k % 9] for k in range(65)]
    assert len(Ts) > ac.AL_BATCH and Ts[0] == 1 and Ts[1] == 300 and Ts[64] == 300
    for ncoef in (2, 33):
        cases = [ac.feature_case(T, ncoef, ac.FEATURE_MODES[k % 4], seed=k) for k, T in enumerate(Ts)]
        mcs, f0s = [g.up(mc) for mc, _ in cases], [g.up(f0) for _, f0 in cases]
        outs = [g.fill((T + GUARD, ncoef + 1), F_SENT) for T in Ts]
        jobs = g.jobs('AlignJob', [(mcs[k], f0s[k], Ts[k], outs[k]) for k in range(65)])
        g.ok('kwy_align_features_batch_dev', jobs, 65, ncoef, ac.POWER_WEIGHT, ac.POWER_THRESHOLD, ac.VUV_WEIGHT)
        for k, out in enumerate(g.down(*outs)):
            assert untouched(out[Ts[k]:]), k                   # (workgroups beyond a short job's frames do nothing)
            assert ac.same(out[:Ts[k]], ac.align_features(*cases[k])), k
            assert ac.same(out[:Ts[k]], _features_single(g, *cases[k])), k


def test_features_refusals(g):
    mc, f0 = ac.feature_case(9, 2, 'first')
    dmc, df0, out = g.up(mc), g.up(f0), g.fill((9, 3), F_SENT)
    w = (ac.POWER_WEIGHT, ac.POWER_THRESHOLD, ac.VUV_WEIGHT)
    assert g.call('kwy_align_features_dev', None, 9, 2, df0, *w, out) == g.EINVAL
    assert g.call('kwy_align_features_dev', dmc, 9, 2, None, *w, out) == g.EINVAL
    assert g.call('kwy_align_features_dev', dmc, 9, 2, df0, *w, None) == g.EINVAL
    assert g.call('kwy_align_features_dev', dmc, 0, 2, df0, *w, out) == g.EINVAL
    assert g.call('kwy_align_features_dev', dmc, -3, 2, df0, *w, out) == g.EINVAL
    assert g.call('kwy_align_features_dev', dmc, 9, 0, df0, *w, out) == g.EINVAL
    jobs = g.jobs('AlignJob', [(dmc, df0, 9, out), (dmc, df0, 0, out)])
    assert g.call('kwy_align_features_batch_dev', jobs, 2, 2, *w) == g.EINVAL      # one bad job refuses the batch
    assert g.call('kwy_align_features_batch_dev', jobs, -1, 2, *w) == g.EINVAL
    assert g.call('kwy_align_features_batch_dev', None, 1, 2, *w) == g.EINVAL
    assert g.call('kwy_align_features_batch_dev', jobs, 0, 2, *w) == g.OK
    assert untouched(g.down(out))


# ---- kwy_align_project(_batch)_dev ------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def project_cases():
    cases = ac.project_cases()
    return {name: (path, trim, ac.project(path, trim)) for name, (path, trim) in cases.items()}


def _project_single(g, path, trim_len, capacity):
    """-> (n_out, the whole index buffer: `capacity` told to the call, GUARD more behind)"""
    idx, n = g.fill(capacity + GUARD, I_SENT, np.int32), g.fill(3, I_SENT, np.int64)
    g.ok('kwy_align_project_dev', g.up(path), g.up([len(path)], np.int64), trim_len, idx, capacity, n[1:])
    idx, n = g.down(idx, n)
    assert n[0] == n[2] == I_SENT
    return int(n[1]), idx


PROJECT_NAMES = sorted(ac.project_cases())


@pytest.mark.parametrize('name', PROJECT_NAMES)
def test_project_against_the_statement(g, project_cases, name):
    path, trim_len, want = project_cases[name]
    n, idx = _project_single(g, path, trim_len, len(want) + 8)
    print(f'{name}: {len(path)} cells, trim_len {trim_len}: n_out = {n}, the statement has {len(want)}')
    assert n == len(want)
    assert ac.same(idx[:n], want) and untouched(idx[n:])


@pytest.mark.parametrize('name', ['unit', 'gaps', 'long', 'gap_1500', 'gap_to_end', 'irregular_3000_trim0'])
def test_project_capacity_below_the_result(g, project_cases, name):
    """the first `capacity` indices, nothing behind them, and n_out = what the projection has (include/kwy.h)"""
    path, trim_len, want = project_cases[name]
    for capacity in (1, 100, ac.AL_TILE - 1, ac.AL_TILE, ac.AL_TILE + 1):
        if capacity >= len(want):
            continue
        n, idx = _project_single(g, path, trim_len, capacity)
        assert n == len(want), (name, capacity)
        assert ac.same(idx[:capacity], want[:capacity]) and untouched(idx[capacity:]), (name, capacity)


def test_project_batch_of_65_paths(g):
    paths = ac.project_batch()
    wants = [ac.project(p, 7) for p in paths]
    assert len(paths) == 65 > ac.AL_BATCH
    dpaths, dlens = [g.up(p) for p in paths], [g.up([len(p)], np.int64) for p in paths]
    caps = [len(w) + 8 if k % 5 else max(len(w) // 2, 1) for k, w in enumerate(wants)]     # every fifth job is short of room
    idxs = [g.fill(c + GUARD, I_SENT, np.int32) for c in caps]
    ns = g.fill(65 + 2, I_SENT, np.int64)
    jobs = g.jobs('ProjectJob', [(dpaths[k], dlens[k], idxs[k], caps[k], ns[1 + k:]) for k in range(65)])
    g.ok('kwy_align_project_batch_dev', jobs, 65, 7)
    ns_h = g.down(ns)
    assert ns_h[0] == ns_h[66] == I_SENT and ns_h[1:66].tolist() == [len(w) for w in wants]
    for k, idx in enumerate(g.down(*idxs)):
        m = min(caps[k], len(wants[k]))
        assert ac.same(idx[:m], wants[k][:m]) and untouched(idx[m:]), k
        n1, idx1 = _project_single(g, paths[k], 7, caps[k])
        assert n1 == ns_h[1 + k] and ac.same(idx1, idx), k
    g.ok('kwy_align_project_batch_dev', jobs, 0, 7)


def test_project_refusals(g, project_cases):
    path, trim_len, want = project_cases['gaps']
    dp, dl, idx, n = g.up(path), g.up([len(path)], np.int64), g.fill(len(want) + 8, I_SENT, np.int32), g.fill(1, I_SENT, np.int64)
    cap = len(want) + 8
    assert g.call('kwy_align_project_dev', None, dl, trim_len, idx, cap, n) == g.EINVAL
    assert g.call('kwy_align_project_dev', dp, None, trim_len, idx, cap, n) == g.EINVAL
    assert g.call('kwy_align_project_dev', dp, dl, trim_len, None, cap, n) == g.EINVAL
    assert g.call('kwy_align_project_dev', dp, dl, trim_len, idx, cap, None) == g.EINVAL
    assert g.call('kwy_align_project_dev', dp, dl, trim_len, idx, 0, n) == g.EINVAL
    assert g.call('kwy_align_project_dev', dp, dl, -1, idx, cap, n) == g.EINVAL
    jobs = g.jobs('ProjectJob', [(dp, dl, idx, cap, n), (dp, dl, idx, -5, n)])
    assert g.call('kwy_align_project_batch_dev', jobs, 2, trim_len) == g.EINVAL
    assert g.call('kwy_align_project_batch_dev', jobs, -1, trim_len) == g.EINVAL
    assert g.call('kwy_align_project_batch_dev', None, 1, trim_len) == g.EINVAL
    idx, n = g.down(idx, n)
    assert untouched(idx) and untouched(n)
    # an empty path (path_len 0) is no refusal: nothing comes out
    idx, n = g.fill(8, I_SENT, np.int32), g.fill(1, I_SENT, np.int64)
    g.ok('kwy_align_project_dev', dp, g.up([0], np.int64), trim_len, idx, 8, n)
    idx, n = g.down(idx, n)
    assert n[0] == 0 and untouched(idx)


# ---- kwy_gather_rows(_batch)_dev --------------------------------------------------------------------------------------
GATHER_N = (0, 1, 300)
GATHER_W = (1, 26, 64, 255, 256, 513)       # 64 threads a row below 256 columns, 256 from there on
SRC_ROWS = 37


def _gather_case(n, width, seed):
    """repeated, unordered indices; every seventh below 0, every seventh + 3 at or above the rows"""
    rng = np.random.default_rng([seed, n, width])
    src = rng.standard_normal((SRC_ROWS, width))
    idx = rng.integers(0, SRC_ROWS, n).astype(np.int32)
    idx[0::7] = -1 - rng.integers(0, 5, len(idx[0::7]))
    idx[3::7] = SRC_ROWS + rng.integers(0, 5, len(idx[3::7]))
    if n > 20:
        idx[10], idx[11], idx[12], idx[13] = -2 ** 31, 2 ** 31 - 1, SRC_ROWS, SRC_ROWS - 1
    return src, idx


def _gather_single(g, src, idx):
    n, width = len(idx), src.shape[1]
    dst = g.fill((n + GUARD, width), F_SENT)
    g.ok('kwy_gather_rows_dev', g.up(src), len(src), width, g.up(np.r_[idx, np.int32(I_SENT)]), n, dst)
    dst = g.down(dst)
    assert untouched(dst[n:]), (n, width)
    return dst[:n]


def test_gather_against_the_statement(g):
    for n in GATHER_N:
        for width in GATHER_W:
            src, idx = _gather_case(n, width, 0)
            want = ac.gather(src, idx)
            assert ac.same(_gather_single(g, src, idx), want), (n, width)
    src, idx = _gather_case(300, 26, 1)
    inside = np.clip(idx, 0, SRC_ROWS - 1)
    assert (idx < 0).sum() > 30 and (idx >= SRC_ROWS).sum() > 30 and len(np.unique(inside)) < 38     # clamped, repeated
    assert ac.same(_gather_single(g, src, idx), src[inside])


def test_gather_batches(g):
    ns = [(0, 1, 300, 17, 0, 64)[k % 6] for k in range(65)]
    for width in (26, 256):
        cases = [_gather_case(n, width, k) for k, n in enumerate(ns)]
        srcs = [g.up(src) for src, _ in cases]
        idxs = [g.up(np.r_[idx, np.int32(I_SENT)]) for _, idx in cases]
        for lengths in (ns, [0] * 65):                           # ragged with empty jobs among them; all empty
            dsts = [g.fill((n + GUARD, width), F_SENT) for n in ns]
            jobs = g.jobs('GatherJob', [(srcs[k], SRC_ROWS, idxs[k], lengths[k], dsts[k]) for k in range(65)])
            g.ok('kwy_gather_rows_batch_dev', jobs, 65, width)
            for k, dst in enumerate(g.down(*dsts)):
                m = lengths[k]
                assert untouched(dst[m:]), (k, width)
                assert ac.same(dst[:m], ac.gather(cases[k][0], cases[k][1][:m])), (k, width)
                if m and k < 12:
                    assert ac.same(dst[:m], _gather_single(g, cases[k][0], cases[k][1])), (k, width)


def test_gather_refusals(g):
    src, idx = _gather_case(17, 26, 0)
    ds, di, dst = g.up(src), g.up(idx), g.fill((17, 26), F_SENT)
    assert g.call('kwy_gather_rows_dev', None, SRC_ROWS, 26, di, 17, dst) == g.EINVAL
    assert g.call('kwy_gather_rows_dev', ds, SRC_ROWS, 26, None, 17, dst) == g.EINVAL
    assert g.call('kwy_gather_rows_dev', ds, SRC_ROWS, 26, di, 17, None) == g.EINVAL
    assert g.call('kwy_gather_rows_dev', ds, 0, 26, di, 17, dst) == g.EINVAL
    assert g.call('kwy_gather_rows_dev', ds, SRC_ROWS, 0, di, 17, dst) == g.EINVAL
    assert g.call('kwy_gather_rows_dev', ds, SRC_ROWS, 26, di, -1, dst) == g.EINVAL
    jobs = g.jobs('GatherJob', [(ds, SRC_ROWS, di, 17, dst), (ds, SRC_ROWS, di, -1, dst)])
    assert g.call('kwy_gather_rows_batch_dev', jobs, 2, 26) == g.EINVAL
    assert g.call('kwy_gather_rows_batch_dev', jobs, -1, 26) == g.EINVAL
    assert g.call('kwy_gather_rows_batch_dev', None, 1, 26) == g.EINVAL
    assert g.call('kwy_gather_rows_batch_dev', jobs, 0, 26) == g.OK
    assert untouched(g.down(dst))


# ---- kwy_trim_length(_batch)_dev --------------------------------------------------------------------------------------
def _trim_single(g, sp, eps):
    n = g.fill(3, I_SENT, np.int64)
    g.ok('kwy_trim_length_dev', g.up(sp), sp.shape[0], sp.shape[1], eps, n[1:])
    n = g.down(n)
    assert n[0] == n[2] == I_SENT
    return int(n[1])


def test_trim_length_against_the_statement(g):
    for T in ac.TRIM_T:
        for K in ac.TRIM_K:
            for kind in ac.TRIM_KINDS:
                sp, eps = ac.trim_case(T, K, kind)
                assert _trim_single(g, sp, eps) == ac.trim_length(sp, eps), (T, K, kind)


def test_trim_length_batch_of_33_ragged_jobs(g):
    for K, eps_kind in ((65, 'eps'), (513, 'eps_two')):
        kinds = [k if not k.startswith('eps') else eps_kind for k in ac.TRIM_KINDS if k != 'eps_two']
        cases = [(ac.TRIM_T[k % 7], kinds[k % len(kinds)]) for k in range(33)]
        sps = [ac.trim_case(T, K, kind)[0] for T, kind in cases]
        eps = ac.trim_case(1, K, eps_kind)[1]
        assert len(cases) > ac.TR_BATCH and len({len(sp) for sp in sps}) == 7
        dsps, ns = [g.up(sp) for sp in sps], g.fill(33 + 2, I_SENT, np.int64)
        jobs = g.jobs('TrimJob', [(dsps[k], len(sps[k]), ns[1 + k:]) for k in range(33)])
        g.ok('kwy_trim_length_batch_dev', jobs, 33, K, eps)
        ns = g.down(ns)
        assert ns[0] == ns[34] == I_SENT
        assert ns[1:34].tolist() == [ac.trim_length(sp, eps) for sp in sps]
        assert ns[1:34].tolist() == [_trim_single(g, sp, eps) for sp in sps]
        assert len(set(ns[1:34].tolist())) >= 6


def test_trim_length_refusals(g):
    sp, eps = ac.trim_case(5, 63, 'runs')
    dsp, n = g.up(sp), g.fill(1, I_SENT, np.int64)
    assert g.call('kwy_trim_length_dev', None, 5, 63, eps, n) == g.EINVAL
    assert g.call('kwy_trim_length_dev', dsp, 5, 63, eps, None) == g.EINVAL
    assert g.call('kwy_trim_length_dev', dsp, 0, 63, eps, n) == g.EINVAL
    assert g.call('kwy_trim_length_dev', dsp, 5, 0, eps, n) == g.EINVAL
    jobs = g.jobs('TrimJob', [(dsp, 5, n), (dsp, -1, n)])
    assert g.call('kwy_trim_length_batch_dev', jobs, 2, 63, eps) == g.EINVAL
    assert g.call('kwy_trim_length_batch_dev', jobs, -1, 63, eps) == g.EINVAL
    assert g.call('kwy_trim_length_batch_dev', None, 1, 63, eps) == g.EINVAL
    assert g.call('kwy_trim_length_batch_dev', jobs, 0, 63, eps) == g.OK
    assert untouched(g.down(n))


# ---- kwy_is_voiced_dev, kwy_train_pad_batch_dev -----------------------------------------------------------------------
def test_is_voiced_against_the_statement(g):
    for fs, K in ac.VOICED_SHAPES:
        for T in (1, 9, 256, 257, 300):
            f0, ap = ac.voiced_case(fs, K, T)
            out = g.fill(T + GUARD, F_SENT)
            g.ok('kwy_is_voiced_dev', g.up(f0), g.up(ap), T, K, fs, out)
            out = g.down(out)
            assert untouched(out[T:]) and ac.same(out[:T], ac.is_voiced(f0, ap[:, 0], fs, K)), (fs, K, T)
            if T >= 9:
                assert out[:9].tolist() == [1, 1, 0, 0, 0, 0, 1, 1, 0]       # both comparisons include their edge


def test_is_voiced_refusals(g):
    f0, ap = ac.voiced_case(8000, 3, 9)
    df, da, out = g.up(f0), g.up(ap), g.fill(9, F_SENT)
    assert g.call('kwy_is_voiced_dev', None, da, 9, 3, 8000, out) == g.EINVAL
    assert g.call('kwy_is_voiced_dev', df, None, 9, 3, 8000, out) == g.EINVAL
    assert g.call('kwy_is_voiced_dev', df, da, 9, 3, 8000, None) == g.EINVAL
    assert g.call('kwy_is_voiced_dev', df, da, 0, 3, 8000, out) == g.EINVAL
    assert g.call('kwy_is_voiced_dev', df, da, 9, 1, 8000, out) == g.EINVAL
    assert g.call('kwy_is_voiced_dev', df, da, 9, 3, 0, out) == g.EINVAL
    assert untouched(g.down(out))


class PadCase:
    """one job of kwy_train_pad_batch_dev: inputs, sentinel-filled outputs with GUARD rows behind, expectations"""

    def __init__(self, g, n, pad_len, fs, K, with_voiced, seed):
        self.n, self.Tp, self.with_voiced = n, n + 2 * pad_len, with_voiced
        f0, ap = ac.voiced_case(fs, K, max(n, 1), seed)
        ap_pad = np.full((self.Tp + GUARD, K), F_SENT)
        ap_pad[pad_len:pad_len + n] = ap[:n]
        self.want = ac.pad(f0, n, ap_pad[:self.Tp], pad_len, fs, with_voiced)
        self.ap_in = ap_pad
        self.f0, self.ap_pad = g.up(f0), g.up(ap_pad)
        self.f0_pad, self.voiced = g.fill(self.Tp + GUARD, F_SENT), g.fill(self.Tp + GUARD, F_SENT)

    def job(self):
        return (self.f0, self.n, self.f0_pad, self.ap_pad, self.voiced if self.with_voiced else None)

    def check(self, g, pad_len, where):
        f0_pad, ap_pad, voiced = g.down(self.f0_pad, self.ap_pad, self.voiced)
        Tp, n = self.Tp, self.n
        assert ac.same(f0_pad[:Tp], self.want[0]) and untouched(f0_pad[Tp:]), where
        assert ac.same(ap_pad[:Tp], self.want[1]) and untouched(ap_pad[Tp:]), where
        assert untouched(ap_pad[:pad_len]), where                                     # the head rows are the caller's
        assert ac.same(ap_pad[pad_len:pad_len + n], self.ap_in[pad_len:pad_len + n]), where
        assert (ap_pad[pad_len + n:Tp] == 1 - 1e-12).all(), where
        if self.with_voiced:
            assert ac.same(voiced[:Tp], self.want[2]) and untouched(voiced[Tp:]), where
        else:
            assert untouched(voiced), where
        return f0_pad, ap_pad, voiced


def test_pad_against_the_statement(g):
    for fs, K in ((16000, 65), (8000, 3)):
        for n in ac.PAD_N:
            for pad_len in ac.PAD_LEN:
                for with_voiced in (False, True):
                    c = PadCase(g, n, pad_len, fs, K, with_voiced, 0)
                    # n = 0 with pad_len = 0 has nothing to write and is no error
                    g.ok('kwy_train_pad_batch_dev', g.jobs('PadJob', [c.job()]), 1, K, fs, pad_len)
                    c.check(g, pad_len, (fs, K, n, pad_len, with_voiced))


def test_pad_batch_of_33_ragged_jobs(g):
    fs, K = 16000, 65
    ns = [(300, 0, 1, 17, 256, 700, 5)[k % 7] for k in range(33)]
    assert len(ns) > ac.TR_BATCH
    for pad_len in (0, 1, 100):
        for with_voiced in (False, True):
            batch = [PadCase(g, n, pad_len, fs, K, with_voiced, k) for k, n in enumerate(ns)]
            g.ok('kwy_train_pad_batch_dev', g.jobs('PadJob', [c.job() for c in batch]), 33, K, fs, pad_len)
            for k, c in enumerate(batch):
                got = c.check(g, pad_len, (pad_len, with_voiced, k))
                if k < 8:
                    one = PadCase(g, ns[k], pad_len, fs, K, with_voiced, k)
                    g.ok('kwy_train_pad_batch_dev', g.jobs('PadJob', [one.job()]), 1, K, fs, pad_len)
                    assert all(ac.same(a, b) for a, b in zip(got, one.check(g, pad_len, k))), (pad_len, with_voiced, k)
    # a batch of nothing but n = 0 jobs without pads
    batch = [PadCase(g, 0, 0, fs, K, True, k) for k in range(3)]
    g.ok('kwy_train_pad_batch_dev', g.jobs('PadJob', [c.job() for c in batch]), 3, K, fs, 0)
    for c in batch:
        c.check(g, 0, 'empty')


def test_pad_refusals(g):
    c = PadCase(g, 17, 5, 16000, 65, True, 0)
    f0, n, f0_pad, ap_pad, voiced = c.job()

    def rc(job, count=1, K=65, fs=16000, pad_len=5):
        return g.call('kwy_train_pad_batch_dev', g.jobs('PadJob', [job]) if job else None, count, K, fs, pad_len)
    assert rc((None, n, f0_pad, ap_pad, voiced)) == g.EINVAL
    assert rc((f0, n, None, ap_pad, voiced)) == g.EINVAL
    assert rc((f0, n, f0_pad, None, voiced)) == g.EINVAL
    assert rc((f0, -1, f0_pad, ap_pad, voiced)) == g.EINVAL
    assert rc(c.job(), pad_len=-1) == g.EINVAL
    assert rc(c.job(), K=1) == g.EINVAL
    assert rc(c.job(), fs=0) == g.EINVAL
    assert rc(c.job(), count=-1) == g.EINVAL
    assert rc(None) == g.EINVAL
    assert rc(c.job(), count=0) == g.OK
    f0_pad, ap_pad, voiced = g.down(c.f0_pad, c.ap_pad, c.voiced)
    assert untouched(f0_pad) and untouched(voiced) and ac.same(ap_pad, c.ap_in)


# ---- kwy_align_even_dev -----------------------------------------------------------------------------------------------
def _even(g, path, fx, fy, flags, pad_len, capacity=None, Tx=None, Ty=None):
    """-> (n_out, idx_x, idx_y: whole buffers, `capacity` told to the call and GUARD more behind)"""
    Tx, Ty = len(fx) if Tx is None else Tx, len(fy) if Ty is None else Ty
    capacity = Tx + Ty + 4 if capacity is None else capacity
    assert len(path) <= Tx + Ty + 4                                       # (the call's scratch: include/kwy.h)
    ix, iy = g.fill(capacity + GUARD, I_SENT, np.int32), g.fill(capacity + GUARD, I_SENT, np.int32)
    n = g.fill(3, I_SENT, np.int64)
    g.ok('kwy_align_even_dev', g.up(path, np.int32), g.up([len(path)], np.int64), g.up(fx), g.up(fy), fx.shape[1], *flags, Tx, Ty,
         pad_len, ix, iy, capacity, n[1:])
    ix, iy, n = g.down(ix, iy, n)
    assert n[0] == n[2] == I_SENT
    return int(n[1]), ix, iy


def _check_even(g, path, fx, fy, flags, pad_len, where):
    wx, wy = ac.even(path, fx, fy, *flags, len(fx), len(fy), pad_len)
    n, ix, iy = _even(g, path, fx, fy, flags, pad_len)
    assert n == len(wx), (where, n, len(wx))
    assert ac.same(ix[:n], wx) and ac.same(iy[:n], wy) and untouched(ix[n:]) and untouched(iy[n:]), where
    return n


def test_even_against_the_statement(g):
    for cells in ac.EVEN_CELLS:
        path, fx, fy = ac.even_case(cells)
        for flags in ac.FLAGS:
            for pad_len in (0, 5):
                _check_even(g, path, fx, fy, flags, pad_len, (cells, flags, pad_len))


def test_even_one_cell_path_under_both_strict_values(g):
    path, fx, fy = ac.even_case(1)
    for use_power, use_vuv in ((0, 0), (1, 1)):
        assert _check_even(g, path, fx, fy, (1, use_power, use_vuv), 0, 'strict') == 2     # chain(path[0], path[-1])
        assert _check_even(g, path, fx, fy, (0, use_power, use_vuv), 0, 'not strict') == 1  # np.array(path)


def test_even_drops_on_round_and_wavefront_boundaries(g):
    path, fx, fy, drop = ac.even_boundary_case()
    assert _check_even(g, path, fx, fy, (1, 1, 0), 0, 'boundary') == 1300 - len(drop)
    assert _check_even(g, path, fx, fy, (1, 1, 1), 5, 'boundary, cut') == 1290 - len([v for v in drop if 5 <= v < 1295])
    assert _check_even(g, path, fx, fy, (0, 1, 1), 0, 'boundary, not strict') == 1300
    assert _check_even(g, path, fx, fy, (1, 0, 0), 5, 'boundary, no test') == 1290


def test_even_cuts_that_come_out_empty(g):
    for name, path, fx, fy, pad_len in ac.even_cut_cases():
        for flags in ac.FLAGS:
            assert _check_even(g, path, fx, fy, flags, pad_len, (name, flags)) == 0


def test_even_capacity_below_the_result(g):
    """the first `capacity` cells, nothing behind them, n_out = capacity (include/kwy.h)"""
    path, fx, fy = ac.even_case(1300)
    for flags, pad_len in (((1, 1, 1), 5), ((0, 0, 0), 0)):
        wx, wy = ac.even(path, fx, fy, *flags, len(fx), len(fy), pad_len)
        for capacity in (1, 255, 256, 257):
            assert capacity < len(wx)
            n, ix, iy = _even(g, path, fx, fy, flags, pad_len, capacity)
            assert n == capacity
            assert ac.same(ix[:n], wx[:n]) and ac.same(iy[:n], wy[:n]) and untouched(ix[n:]) and untouched(iy[n:])


def test_even_refusals(g):
    path, fx, fy = ac.even_case(3)
    dp, dl, dx, dy = g.up(path), g.up([3], np.int64), g.up(fx), g.up(fy)
    ix, iy, n = g.fill(16, I_SENT, np.int32), g.fill(16, I_SENT, np.int32), g.fill(1, I_SENT, np.int64)
    good = [dp, dl, dx, dy, 4, 1, 1, 1, len(fx), len(fy), 0, ix, iy, 16, n]
    for k in (0, 1, 2, 3, 11, 12, 14):                       # each pointer NULL in turn
        assert g.call('kwy_align_even_dev', *[None if i == k else a for i, a in enumerate(good)]) == g.EINVAL
    for k, bad in ((4, 1), (8, 0), (9, 0), (10, -1), (13, 0)):  # width < 2, Tx, Ty, pad_len < 0, capacity
        assert g.call('kwy_align_even_dev', *[bad if i == k else a for i, a in enumerate(good)]) == g.EINVAL
    ix, iy, n = g.down(ix, iy, n)
    assert untouched(ix) and untouched(iy) and untouched(n)


# ---- kwy_delta_features_dev -------------------------------------------------------------------------------------------
def _delta_input(rng, rows, d):
    x = rng.standard_normal((rows, d))
    if rows >= 3:
        x[1, 0], x[rows - 1, d - 1], x[0, d // 2] = -0.0, np.inf, -np.inf
        x[2] = 0.0
    return x


def _delta(g, x, n, capacity):
    """-> the whole output: `capacity` rows told to the call, GUARD more behind"""
    d = x.shape[1]
    out = g.fill((capacity + GUARD, 3 * d), F_SENT)
    g.ok('kwy_delta_features_dev', g.up(x), g.up([n], np.int64), capacity, d, out)
    return g.down(out)


def test_delta_against_the_statement(g):
    rng = np.random.default_rng(0)
    for d in (1, 24, 64, 65):
        for n, capacity in ((0, 4), (1, 1), (1, 5), (2, 2), (3, 3), (3, 8), (300, 300), (300, 310), (300, 200), (5, 1)):
            x = _delta_input(rng, max(n, capacity), d)
            out = _delta(g, x, n, capacity)
            m = min(n, capacity)                                # a count above the capacity is clamped to it
            assert ac.same(out[:m], ac.delta(x[:m])), (d, n, capacity)
            assert untouched(out[m:]), (d, n, capacity)         # (rows in [n, capacity) included)
    x = np.array([[1.0], [np.inf], [2.0], [-0.0], [-np.inf]])
    out = _delta(g, x, 5, 5)[:5]
    assert np.isnan(out[1, 1]) and out[0, 1] == np.inf and ac.same(out, ac.delta(x))     # the 0.0 * x[t] term is there


def test_delta_refusals(g):
    x, n, out = g.up(np.ones((4, 3))), g.up([4], np.int64), g.fill((4, 9), F_SENT)
    assert g.call('kwy_delta_features_dev', None, n, 4, 3, out) == g.EINVAL
    assert g.call('kwy_delta_features_dev', x, None, 4, 3, out) == g.EINVAL
    assert g.call('kwy_delta_features_dev', x, n, 4, 3, None) == g.EINVAL
    assert g.call('kwy_delta_features_dev', x, n, 0, 3, out) == g.EINVAL
    assert g.call('kwy_delta_features_dev', x, n, 4, 0, out) == g.EINVAL
    assert untouched(g.down(out))


# ---- kwy_joint_rows_dev -----------------------------------------------------------------------------------------------
def _joint(g, xd, yd, n, capacity, eps):
    """-> (n_out, the whole joint buffer of capacity + GUARD rows)"""
    w = xd.shape[1]
    rows = max(len(xd), 1)
    dx, dy = g.up(np.vstack((xd, np.zeros((rows - len(xd), w))))), g.up(np.vstack((yd, np.zeros((rows - len(yd), w)))))
    joint, n_out = g.fill((capacity + GUARD, 2 * w), F_SENT), g.fill(3, I_SENT, np.int64)
    g.ok('kwy_joint_rows_dev', dx, dy, g.up([n], np.int64), capacity, w, eps, joint, n_out[1:])
    joint, n_out = g.down(joint, n_out)
    assert n_out[0] == n_out[2] == I_SENT
    return int(n_out[1]), joint


def test_joint_against_the_statement(g):
    for n in ac.JOINT_N:
        for w in ac.JOINT_W:
            for kind in ac.JOINT_KINDS:
                xd, yd, eps = ac.joint_case(n, w, kind)
                want = ac.joint(xd, yd, eps)
                m, joint = _joint(g, xd, yd, n, max(n, 1), eps)
                assert m == len(want), (n, w, kind, m, len(want))
                assert ac.same(joint[:m], want) and untouched(joint[m:]), (n, w, kind)
    xd, yd, eps = ac.joint_case(600, 72, 'nan_eps')
    assert np.isnan(ac.joint(xd, yd, eps)).any()                        # (the NaN row is among the kept ones)


def test_joint_count_above_the_capacity_is_clamped(g):
    xd, yd, eps = ac.joint_case(600, 65, 'marks')
    for capacity in (1, 256, 300):
        want = ac.joint(xd[:capacity], yd[:capacity], eps)
        m, joint = _joint(g, xd, yd, 600, capacity, eps)
        assert m == len(want) and ac.same(joint[:m], want) and untouched(joint[m:]), capacity


def test_joint_refusals(g):
    xd, yd, eps = ac.joint_case(5, 3, 'none_dropped')
    dx, dy, n = g.up(xd), g.up(yd), g.up([5], np.int64)
    joint, n_out = g.fill((5, 6), F_SENT), g.fill(1, I_SENT, np.int64)
    good = [dx, dy, n, 5, 3, eps, joint, n_out]
    for k in (0, 1, 2, 6, 7):
        assert g.call('kwy_joint_rows_dev', *[None if i == k else a for i, a in enumerate(good)]) == g.EINVAL
    for k in (3, 4):
        assert g.call('kwy_joint_rows_dev', *[0 if i == k else a for i, a in enumerate(good)]) == g.EINVAL
    joint, n_out = g.down(joint, n_out)
    assert untouched(joint) and untouched(n_out)


# ---- kwy_train_rows_batch_dev -----------------------------------------------------------------------------------------
class TrainPair:
    def __init__(self, g, steps, d, seed):
        self.host = ac.train_pair(steps, d, seed)
        path, fx, fy, mc_x, mc_y = self.host
        self.Tx, self.Ty = len(fx), len(fy)
        self.dev = [g.up(path), g.up([len(path)], np.int64), g.up(fx), g.up(fy), g.up(mc_x), g.up(mc_y)]


def _train_rows(g, pairs, d, flags, pad_len, eps, capacity_rows, cursor0):
    """-> (the whole matrix of capacity_rows + GUARD rows, the pairs' n_rows, the cursor)"""
    joint = g.fill((capacity_rows + GUARD, 6 * d), F_SENT)
    n_rows, cursor = g.fill(len(pairs) + 2, I_SENT, np.int64), g.up([I_SENT, cursor0, I_SENT], np.int64)
    jobs = g.jobs('TrainJob', [(*p.dev, p.Tx, p.Ty, n_rows[1 + k:]) for k, p in enumerate(pairs)])
    g.ok('kwy_train_rows_batch_dev', jobs, len(pairs), d, *flags, pad_len, eps, joint, capacity_rows, cursor[1:])
    joint, n_rows, cursor = g.down(joint, n_rows, cursor)
    assert n_rows[0] == n_rows[-1] == I_SENT and cursor[0] == cursor[2] == I_SENT
    return joint, n_rows[1:-1].tolist(), int(cursor[1])


def _composed_rows(g, p, d, flags, pad_len, eps):
    """one pair through the single entries, as the stream driver chains them: the filter and cut, a gather of the
    whole capacity (the stale tail of the index lists clamps), the delta features of the counted rows, the joint rows"""
    path, fx, fy, mc_x, mc_y = p.host
    cap = p.Tx + p.Ty + 4
    ix, iy = g.fill(cap, -5, np.int32), g.fill(cap, -5, np.int32)
    n_sel, n_out = g.fill(1, I_SENT, np.int64), g.fill(1, I_SENT, np.int64)
    g.ok('kwy_align_even_dev', p.dev[0], p.dev[1], p.dev[2], p.dev[3], d + 2, *flags, p.Tx, p.Ty, pad_len, ix, iy, cap, n_sel)
    halves = []
    for mc, T, idx in ((p.dev[4], p.Tx, ix), (p.dev[5], p.Ty, iy)):
        sel = g.fill((cap, d + 1), F_SENT)
        g.ok('kwy_gather_rows_dev', mc, T, d + 1, idx, cap, sel)
        static = g.up(g.down(sel)[:, 1:])
        out = g.fill((cap, 3 * d), F_SENT)
        g.ok('kwy_delta_features_dev', static, n_sel, cap, d, out)
        halves.append(out)
    joint = g.fill((cap, 6 * d), F_SENT)
    g.ok('kwy_joint_rows_dev', halves[0], halves[1], n_sel, cap, 3 * d, eps, joint, n_out)
    joint, n_out = g.down(joint, n_out)
    assert untouched(joint[n_out[0]:])
    return joint[:n_out[0]]


def _check_train(g, pairs, d, flags, pad_len, capacity_rows, cursor0, compose=True):
    """the batched call against the numpy statement and the single entries, pair by pair; -> the pairs' n_rows"""
    wants = [ac.train_rows(*p.host, *flags, pad_len) for p in pairs]
    joint, n_rows, cursor = _train_rows(g, pairs, d, flags, pad_len, ac.EPS, capacity_rows, cursor0)
    assert untouched(joint[:cursor0])                                    # the rows before the cursor
    at = cursor0
    for k, (p, want) in enumerate(zip(pairs, wants)):
        if at + len(want) > capacity_rows:                               # dropped whole and flagged, the cursor stays
            assert n_rows[k] == -1 - len(want), (k, n_rows[k], len(want))
            continue
        assert n_rows[k] == len(want), (k, n_rows[k], len(want))
        assert ac.same(joint[at:at + len(want)], want), k
        if compose:
            assert ac.same(joint[at:at + len(want)], _composed_rows(g, p, d, flags, pad_len, ac.EPS)), k
        at += len(want)
    assert cursor == at and untouched(joint[at:])
    return n_rows


def test_train_rows_17_ragged_pairs(g):
    d = 3
    pairs = [TrainPair(g, steps, d, k) for k, steps in enumerate(ac.TRAIN_STEPS)]
    assert len(pairs) == 17 > ac.TR_PAIRS
    n_rows = _check_train(g, pairs, d, (1, 1, 1), 5, 4000, 0)
    assert min(n_rows) >= 0 and len(set(n_rows)) > 10 and sum(n_rows) > 600
    n_rows = _check_train(g, pairs, d, (0, 1, 1), 0, 6000, 7)           # no filter, no cut, a cursor above 0
    assert n_rows[11] == 1 and n_rows[2] == 2                            # the one-cell path comes out once; two cells twice


def test_train_rows_all_flags_on_one_pair(g):
    d = 24
    pair = TrainPair(g, 120, d, 3)
    counts = []
    for flags in ac.FLAGS:
        for pad_len in (0, 5):
            counts.append(_check_train(g, [pair], d, flags, pad_len, 400, 3)[0])
    assert len(set(counts)) >= 4 and min(counts) > 0
    one = TrainPair(g, 0, d, 4)                                           # a one-cell path
    assert ac.train_rows(*one.host, 1, 1, 1, 0).shape == (2, 6 * d)
    assert _check_train(g, [one], d, (1, 1, 1), 0, 8, 0) == [2] and _check_train(g, [one], d, (0, 1, 1), 0, 8, 0) == [1]


def test_train_rows_pair_that_does_not_fit(g):
    d = 3
    pairs = [TrainPair(g, steps, d, 20 + k) for k, steps in enumerate((90, 60, 700, 40, 300, 33))]
    rows = [len(ac.train_rows(*p.host, 1, 1, 1, 5)) for p in pairs]
    assert rows[2] > rows[3] + rows[5] and rows[4] > rows[5] > 0
    cursor0 = 11
    capacity_rows = cursor0 + rows[0] + rows[1] + rows[3] + rows[5]      # the third and the fifth pair do not fit
    n_rows = _check_train(g, pairs, d, (1, 1, 1), 5, capacity_rows, cursor0, compose=False)
    assert n_rows == [rows[0], rows[1], -1 - rows[2], rows[3], -1 - rows[4], rows[5]]
    # a matrix that is full already: every pair with rows is dropped, nothing is written
    n_rows = _check_train(g, pairs[:2], d, (1, 1, 1), 5, cursor0, cursor0, compose=False)
    assert n_rows == [-1 - rows[0], -1 - rows[1]]


def test_train_rows_count_zero_and_refusals(g):
    d = 3
    p = TrainPair(g, 40, d, 0)
    joint, n_rows, cursor = g.fill((50, 6 * d), F_SENT), g.fill(1, I_SENT, np.int64), g.up([4], np.int64)

    def rc(job=None, count=1, d=d, pad_len=5, joint=joint, capacity_rows=50, cursor=cursor, jobs=True):
        job = (*p.dev, p.Tx, p.Ty, n_rows) if job is None else job
        return g.call('kwy_train_rows_batch_dev', g.jobs('TrainJob', [job]) if jobs else None, count, d, 1, 1, 1, pad_len, ac.EPS,
                      joint, capacity_rows, cursor)
    assert rc(count=0) == g.OK
    assert rc(count=-1) == g.EINVAL and rc(jobs=False) == g.EINVAL
    assert rc(d=0) == g.EINVAL and rc(pad_len=-1) == g.EINVAL and rc(capacity_rows=-1) == g.EINVAL
    assert rc(joint=None) == g.EINVAL and rc(cursor=None) == g.EINVAL
    good = [*p.dev, p.Tx, p.Ty, n_rows]
    for k in (0, 1, 2, 3, 4, 5, 8):
        assert rc(job=[None if i == k else a for i, a in enumerate(good)]) == g.EINVAL
    for k in (6, 7):
        assert rc(job=[0 if i == k else a for i, a in enumerate(good)]) == g.EINVAL
    joint, n_rows, cursor = g.down(joint, n_rows, cursor)
    assert untouched(joint) and untouched(n_rows) and cursor[0] == 4
