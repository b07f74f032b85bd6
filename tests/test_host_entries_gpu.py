"""Every host-pointer entry of include/kwy.h against its device-pointer twin, bit for bit.

A host entry stages its buffers through kwy_staging (kwy_internal.hpp) and runs the pass its `_dev` twin runs, so on
the same inputs both have to leave the same bytes: the results, the status words and the returned lengths.  Every
output is an interior view of a larger array filled with a sentinel (64 guard bytes on either side, on the host and on
the device), so a download that is too long, or a kernel that writes past its buffer, shows in the guards.  A refused
call gives the twin's return code and message and leaves every output as it was.

Flat entries: 0.1 s at 16 kHz, the smallest transform the entry accepts, order 4.  Job lists: rows 0, 1, 3 and one job
longer than the kernel's chunk, one job whose base aliases x and one whose base does not; and one call with one job
more than a launch takes.

Held elsewhere, and left out here: kwy_dio and kwy_stonemask (test_f0_finish_gpu.py::test_f0_batch_equals_host_entries_*),
kwy_synthesize (test_synth_edges_gpu.py::test_entries_agree), kwy_gmm_mlpg, kwy_gmm_mlpg_em, kwy_gmm_mlpg_gv and
kwy_gmm_convert_frames (test_mlpg_entry_bits_gpu.py, test_em_gpu.py::test_host_entry_equals_device_entry_bit_for_bit).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD_BYTES = 64
SENTINEL = {np.dtype(np.float64): -1234.5, np.dtype(np.int32): -77, np.dtype(np.int64): -77, np.dtype(np.uint8): 0xA5}
FS, ORDER, COLS, L_MS = 16000, 4, 5, 512
GV_CHUNK, GV_GROUP, MS_GROUP, FS_CHUNK, FS_GROUP = 2048, 32, 64, 2048, 32     # kwy_gv.hip, kwy_ms.hip, kwy_formant.hip


class Side:
    """The buffers of one call, in host memory or (dev) in device memory: i() an input, o() a guarded output."""

    def __init__(self, ctx, dev):
        self.ctx, self.dev, self.keep, self.outs = ctx, dev, [], []

    def fn(self, host, dev):
        from kwiiyatta_amd import _lib
        return getattr(_lib.lib, dev if self.dev else host)

    def i(self, a):
        if a is None or a.size == 0:
            return None
        a = np.ascontiguousarray(a)
        if self.dev:
            import torch
            a = torch.from_numpy(a.copy()).cuda()
        self.keep.append(a)
        return a.data_ptr() if self.dev else a.ctypes.data

    def o(self, n, dtype=np.float64, init=None):
        dtype = np.dtype(dtype)
        if n == 0:
            return None
        g = GUARD_BYTES // dtype.itemsize
        big = np.full(n + 2 * g, SENTINEL[dtype], dtype)
        if init is not None:
            big[g:g + n] = np.asarray(init).view(dtype).ravel() if dtype == np.uint8 else np.asarray(init).ravel()
        before = big.copy()
        if self.dev:
            import torch
            big = torch.from_numpy(big).cuda()
        self.outs.append((big, before, g, n))
        return (big.data_ptr() if self.dev else big.ctypes.data) + GUARD_BYTES

    def results(self):
        """[(whole array after the call, as it was before, guard elements, interior elements)]"""
        return [(b.cpu().numpy() if self.dev else b, before, g, n) for b, before, g, n in self.outs]


def _jobs(struct, rows):
    from kwiiyatta_amd import _lib
    return _lib.job_array(struct, rows)


# ------------------------------------------------------------------------------------------------------------ inputs
class Data:
    def __init__(self):
        from kwiiyatta_amd.synthetic import make_utterance
        rng = np.random.default_rng(11)
        self.rng = rng
        self.x, self.f0, self.t = make_utterance(seed=7, fs=FS, seconds=0.1)
        self.f0[::5] = 0.0                                        # some unvoiced frames
        self.T = len(self.f0)
        self.fft = 512
        self.K = self.fft // 2 + 1
        self.sp = np.exp(rng.standard_normal((self.T, self.K)) * 0.3 - 8.0)
        self.ap = np.clip(rng.uniform(0.001, 0.999, (self.T, self.K)), 0.001, 0.999)
        self.mc = rng.standard_normal((self.T, ORDER + 1)) * 0.2
        # ragged job lists: rows 0, 1, 3 and one longer than a chunk of the kernel
        self.rows_gv = (0, 1, 3, GV_CHUNK // COLS + 2)
        self.rows_ms = (0, 1, 3, L_MS)
        self.mats_gv = [rng.standard_normal((r, COLS)) for r in self.rows_gv]
        self.base_gv = [rng.standard_normal((r, COLS)) for r in self.rows_gv]
        self.mats_ms = [rng.standard_normal((r, COLS)) for r in self.rows_ms]
        self.base_ms = [rng.standard_normal((r, COLS)) for r in self.rows_ms]
        self.gv = rng.uniform(0.5, 2.0, COLS)
        self.moments = self.triples(6 * COLS).reshape(6, COLS, 3)
        self.tracks = [np.where(rng.uniform(size=n) < 0.3, 0.0, rng.uniform(80.0, 300.0, n)) for n in (0, 1, 3, 700)]
        self.KF = 65
        self.rows_fs = (0, 1, 3, FS_CHUNK // self.KF + 2)
        self.envs = [np.exp(rng.standard_normal((r, self.KF))) for r in self.rows_fs]

    def triples(self, n):
        """n valid (count, mean, M2) triples"""
        return np.stack([self.rng.integers(1, 50, n).astype(np.float64), self.rng.standard_normal(n),
                         self.rng.uniform(0.1, 9.0, n)], axis=1)


@pytest.fixture(scope='module')
def d():
    return Data()


@pytest.fixture(scope='module')
def ctx():
    from kwiiyatta_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope='module')
def ms_stats(ctx, d):
    """two accumulators of the modulation-spectrum statistics (host entries), for the filter's cases"""
    from kwiiyatta_amd import _lib
    out = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        mats = [rng.standard_normal((r, COLS)) for r in (40, 64, 100)]
        Kh = L_MS // 2 + 1
        spectra, valid = np.zeros((3, COLS, Kh)), np.zeros((3, COLS), np.int32)
        arr = _jobs(_lib.GvMatrix, [(m.ctypes.data, m.shape[0]) for m in mats])
        _lib.check(ctx, _lib.lib.kwy_ms_logspectra(ctx.handle, arr, 3, COLS, L_MS, _lib.ptr(spectra), _lib.ptr(valid)))
        acc = np.zeros((COLS, Kh, 3))
        _lib.check(ctx, _lib.lib.kwy_ms_stats_update(ctx.handle, _lib.ptr(acc), _lib.ptr(spectra), _lib.ptr(valid), 3, COLS, L_MS))
        out.append((acc, spectra, valid))
    return out


# ------------------------------------------------------------------------------------------------------------- cases
# case(s, d, bad) -> return code: the call of the entry (s.dev: of its twin) on the buffers of side s; bad: with one
# argument both forms refuse in the same check
def c_cheaptrick(s, d, bad):
    return s.fn('kwy_cheaptrick', 'kwy_cheaptrick_dev')(
        s.ctx.handle, s.i(d.x), len(d.x), 0 if bad else FS, s.i(d.t), s.i(d.f0), d.T, -0.15, 71.0, d.fft, 1.0,
        s.o(d.T * d.K))


def c_d4c(s, d, bad):
    return s.fn('kwy_d4c', 'kwy_d4c_dev')(
        s.ctx.handle, s.i(d.x), len(d.x), 0 if bad else FS, s.i(d.t), s.i(d.f0), d.T, 0.85, d.fft, s.o(d.T * d.K))


def c_logf0_moments(s, d, bad):
    from kwiiyatta_amd import _lib
    arr = _jobs(_lib.F0Track, [(s.i(t), len(t)) for t in d.tracks])
    return s.fn('kwy_logf0_moments', 'kwy_logf0_moments_batch_dev')(
        s.ctx.handle, arr, 0 if bad else len(d.tracks), s.o(3 * len(d.tracks)))


def c_logf0_moments_merge(s, d, bad):
    m = d.moments[:, 0]
    return s.fn('kwy_logf0_moments_merge', 'kwy_logf0_moments_merge_dev')(s.ctx.handle, s.i(m), 0 if bad else len(m), s.o(3))


def c_f0_map(s, d, bad):
    from kwiiyatta_amd import _lib
    arr = _jobs(_lib.F0MapJob, [(s.i(t), len(t), s.o(len(t))) for t in d.tracks])
    stats = np.array([5.0, 0.2, 5.3, 0.3])
    return s.fn('kwy_f0_map', 'kwy_f0_map_batch_dev')(
        s.ctx.handle, arr, len(d.tracks), FS, s.i(stats), 0.0 if bad else 2.0 ** (2 / 12), s.o(len(d.tracks), np.int32))


def c_column_moments(s, d, bad):
    from kwiiyatta_amd import _lib
    arr = _jobs(_lib.GvMatrix, [(s.i(m), m.shape[0]) for m in d.mats_gv])
    return s.fn('kwy_column_moments', 'kwy_column_moments_batch_dev')(
        s.ctx.handle, arr, len(d.mats_gv), 65 if bad else COLS, s.o(3 * COLS * len(d.mats_gv)))


def c_gv_from_moments(s, d, bad):
    return s.fn('kwy_gv_from_moments', 'kwy_gv_from_moments_dev')(
        s.ctx.handle, s.i(d.moments), len(d.moments), 0 if bad else COLS, s.o(COLS))


def _gv_postfilter(s, d, bad, mats, bases):
    """bases[i] is None: base aliases x.  The device twin takes the moments the host entry computes for itself."""
    from kwiiyatta_amd import _lib
    n, rows = len(mats), []
    moments = None
    if s.dev:
        import torch
        moments = torch.zeros(n * 3 * COLS, dtype=torch.float64, device='cuda')
        s.keep.append(moments)
    for k, (m, b) in enumerate(zip(mats, bases)):
        x = s.i(m)
        rows.append((x, m.shape[0], moments.data_ptr() + 8 * 3 * COLS * k if s.dev else None,
                     x if b is None else s.i(b), s.o(m.size)))
    arr = _jobs(_lib.GvJob, rows)
    gv, status = s.i(d.gv), s.o(n, np.int32)
    if s.dev and not bad:
        mats_arr = _jobs(_lib.GvMatrix, [(r[0], r[1]) for r in rows])
        _lib.check(s.ctx, _lib.lib.kwy_column_moments_batch_dev(s.ctx.handle, mats_arr, n, COLS, moments.data_ptr()))
    return s.fn('kwy_gv_postfilter', 'kwy_gv_postfilter_batch_dev')(
        s.ctx.handle, arr, n, COLS, 1, gv, 2.0 if bad else 0.7, status)


def c_gv_postfilter(s, d, bad):
    return _gv_postfilter(s, d, bad, d.mats_gv, [d.base_gv[0], None, d.base_gv[2], d.base_gv[3]])


def c_gv_postfilter_group(s, d, bad):
    mats = [d.mats_gv[1 + k % 2] for k in range(GV_GROUP + 1)]
    return _gv_postfilter(s, d, bad, mats, [None if k % 3 else d.base_gv[1 + k % 2] for k in range(GV_GROUP + 1)])


def c_ms_logspectra(s, d, bad):
    from kwiiyatta_amd import _lib
    n = len(d.mats_ms)
    arr = _jobs(_lib.GvMatrix, [(s.i(m), m.shape[0]) for m in d.mats_ms])
    return s.fn('kwy_ms_logspectra', 'kwy_ms_logspectra_batch_dev')(
        s.ctx.handle, arr, n, COLS, 500 if bad else L_MS, s.o(n * COLS * (L_MS // 2 + 1)), s.o(n * COLS, np.int32))


def c_ms_stats_update(s, d, bad, ms_stats=None):
    acc, spectra, valid = ms_stats[0]
    return s.fn('kwy_ms_stats_update', 'kwy_ms_stats_update_dev')(
        s.ctx.handle, s.o(acc.size, init=acc), s.i(ms_stats[1][1]), s.i(ms_stats[1][2]), 3, COLS, 500 if bad else L_MS)


def _ms_postfilter(s, d, bad, ms_stats, mats, bases):
    from kwiiyatta_amd import _lib
    rows = []
    for m, b in zip(mats, bases):
        x = s.i(m)
        rows.append((x, m.shape[0], x if b is None else s.i(b), s.o(m.size)))
    arr = _jobs(_lib.MsJob, rows)
    return s.fn('kwy_ms_postfilter', 'kwy_ms_postfilter_batch_dev')(
        s.ctx.handle, arr, len(mats), COLS, 1, L_MS, s.i(ms_stats[0][0]), s.i(ms_stats[1][0]), -1.0 if bad else 0.8,
        s.o(len(mats), np.int32))


def c_ms_postfilter(s, d, bad, ms_stats=None):
    return _ms_postfilter(s, d, bad, ms_stats, d.mats_ms, [d.base_ms[0], None, d.base_ms[2], d.base_ms[3]])


def c_ms_postfilter_group(s, d, bad, ms_stats=None):
    mats = [d.mats_ms[1 + k % 2] for k in range(MS_GROUP + 1)]
    return _ms_postfilter(s, d, bad, ms_stats, mats, [None if k % 3 else d.base_ms[1 + k % 2] for k in range(MS_GROUP + 1)])


def c_pitch_shift(s, d, bad):
    from kwiiyatta_amd import _lib
    rate = 3.0 if bad else 1.25
    n = len(d.x)
    frames = int(_lib.lib.kwy_pitch_frames(n, FS, 1.25))
    x, y, pos = s.i(d.x), s.o(n), s.o(frames, np.int32)
    if s.dev:
        return _lib.lib.kwy_pitch_shift_batch_dev(s.ctx.handle, _jobs(_lib.PitchJob, [(x, n, y, pos)]), 1, FS, rate)
    return _lib.lib.kwy_pitch_shift(s.ctx.handle, x, n, FS, rate, y, pos)


def _formant_shift(s, d, bad, envs):
    from kwiiyatta_amd import _lib
    arr = _jobs(_lib.FormantJob, [(s.i(e), e.shape[0], s.o(e.size)) for e in envs])
    return s.fn('kwy_formant_shift', 'kwy_formant_shift_batch_dev')(
        s.ctx.handle, arr, len(envs), d.KF, 3.0 if bad else 1.1, s.o(len(envs), np.int32))


def c_formant_shift(s, d, bad):
    return _formant_shift(s, d, bad, d.envs)


def c_formant_shift_group(s, d, bad):
    return _formant_shift(s, d, bad, [d.envs[1 + k % 2] for k in range(FS_GROUP + 1)])


def c_mcd(s, d, bad):
    from kwiiyatta_amd import _lib
    rng = np.random.default_rng(3)
    rows = []
    for r, listed, masked, per_row in ((0, False, False, False), (1, True, False, True), (3, False, True, True),
                                       (300, True, True, True)):
        a, b = rng.standard_normal((r + 2, COLS)), rng.standard_normal((r + 1, COLS))
        ia = rng.integers(0, r + 2, r).astype(np.int32) if listed else None
        ib = rng.integers(0, r + 1, r).astype(np.int32) if listed else None
        mask = (rng.uniform(size=r + 1) < 0.7).astype(np.float64) if masked else None
        rows.append((s.i(a), r + 2, COLS, s.i(b), r + 1, COLS, s.i(ia) if listed else None, s.i(ib) if listed else None,
                     0, 0, r, None, s.i(mask) if masked else None, 1, r + 1 if masked else 0, s.o(r) if per_row else None))
    arr = _jobs(_lib.McdJob, rows)
    return s.fn('kwy_mcd', 'kwy_mcd_batch_dev')(
        s.ctx.handle, arr, len(rows), 65 if bad else COLS, 1, s.o(3 * len(rows)), s.o(len(rows), np.int32))


def c_f0_error(s, d, bad):
    from kwiiyatta_amd import _lib
    rng = np.random.default_rng(4)
    rows = []
    for r, listed in ((0, False), (1, True), (3, False), (300, True)):
        fa = np.where(rng.uniform(size=r + 2) < 0.3, 0.0, rng.uniform(80.0, 300.0, r + 2))
        fb = np.where(rng.uniform(size=r + 1) < 0.3, 0.0, rng.uniform(80.0, 300.0, r + 1))
        ia = rng.integers(0, r + 2, r).astype(np.int32) if listed else None
        ib = rng.integers(0, r + 1, r).astype(np.int32) if listed else None
        rows.append((s.i(fa), r + 2, s.i(fb), r + 1, s.i(ia) if listed else None, s.i(ib) if listed else None, 0, 0, r, None))
    arr = _jobs(_lib.F0ErrorJob, rows)
    n = len(rows)
    return s.fn('kwy_f0_error', 'kwy_f0_error_batch_dev')(
        s.ctx.handle, arr, 0 if bad else n, s.o(4 * n, np.int64), s.o(3 * n), s.o(n, np.int32))


def c_moments_merge(s, d, bad):
    return s.fn('kwy_moments_merge', 'kwy_moments_merge_dev')(
        s.ctx.handle, s.i(d.moments), len(d.moments), 0 if bad else COLS, s.o(3 * COLS))


def c_sp2mc(s, d, bad):
    return s.fn('kwy_sp2mc', 'kwy_sp2mc_dev')(
        s.ctx.handle, s.i(d.sp), d.T, d.K, ORDER, 1.0 if bad else 0.41, s.o(d.T * (ORDER + 1)))


def c_mc2sp(s, d, bad):
    return s.fn('kwy_mc2sp', 'kwy_mc2sp_dev')(
        s.ctx.handle, s.i(d.mc), d.T, ORDER, 1.0 if bad else 0.41, d.fft, s.o(d.T * d.K))


def c_code_aperiodicity(s, d, bad):
    from kwiiyatta_amd import _lib
    nb = int(_lib.lib.kwy_aperiodicity_bands(FS))
    assert nb >= 1
    return s.fn('kwy_code_aperiodicity', 'kwy_code_aperiodicity_dev')(
        s.ctx.handle, s.i(d.ap), d.T, FS, 3 if bad else d.fft, s.o(d.T * nb))


def c_decode_aperiodicity(s, d, bad):
    from kwiiyatta_amd import _lib
    nb = int(_lib.lib.kwy_aperiodicity_bands(FS))
    coded = -np.random.default_rng(5).uniform(0.1, 40.0, (d.T, nb))
    coded[::4] = -0.1                                             # frames the decoder takes as unvoiced
    return s.fn('kwy_decode_aperiodicity', 'kwy_decode_aperiodicity_dev')(
        s.ctx.handle, s.i(coded), d.T, FS, d.fft, -1 if bad else nb, s.o(d.T * d.K))


def c_stretch_log(s, d, bad):
    new_K = 513
    return s.fn('kwy_stretch_log', 'kwy_stretch_log_dev')(
        s.ctx.handle, s.i(d.sp), d.T, d.K, 0 if bad else new_K, s.o(d.T * new_K))


def c_mc2b(s, d, bad):
    return s.fn('kwy_mc2b', 'kwy_mc2b_dev')(s.ctx.handle, s.i(d.mc), d.T, 0 if bad else ORDER, 0.41, s.o(d.mc.size))


def c_mlsa_synthesis(s, d, bad):
    return s.fn('kwy_mlsa_synthesis', 'kwy_mlsa_synthesis_dev')(
        s.ctx.handle, s.i(d.x), len(d.x), s.i(d.mc), d.T, ORDER, 0.41, 3 if bad else 5, 80, s.o(len(d.x)))


def c_mcep_filter_fft(s, d, bad):
    return s.fn('kwy_mcep_filter_fft', 'kwy_mcep_filter_fft_dev')(
        s.ctx.handle, s.i(d.x), len(d.x), s.i(d.mc), d.T, ORDER, 0.41, 80, 1000 if bad else 1024, 1, s.o(len(d.x)))


def c_fastdtw(s, d, bad):
    rng = np.random.default_rng(6)
    Tx, Ty, dim = 21, 17, ORDER + 1
    a, b = rng.standard_normal((Tx, dim)), rng.standard_normal((Ty, dim))
    return s.fn('kwy_fastdtw', 'kwy_fastdtw_dev')(
        s.ctx.handle, s.i(a), Tx, s.i(b), Ty, dim, 0 if bad else 1, s.o(1), s.o(2 * (Tx + Ty), np.int32), s.o(1, np.int64))


def c_np_normal(s, d, bad):
    from kwiiyatta_amd import _lib
    _, key, pos, has_gauss, cached = np.random.RandomState(12345).get_state()
    state = np.concatenate([key.astype(np.uint32).view(np.uint8), np.array([pos, has_gauss], np.int32).view(np.uint8),
                            np.array([cached], np.float64).view(np.uint8)])
    assert state.size == int(_lib.lib.kwy_np_state_bytes())
    n = 1001
    return s.fn('kwy_np_normal', 'kwy_np_normal_dev')(
        s.ctx.handle, s.o(state.size, np.uint8, init=state), 0.0, 1e-3, 1, -1 if bad else n, s.o(n))


def c_gv_ascent(s, d, bad):
    from kwiiyatta_amd import _lib
    rng = np.random.default_rng(8)
    iterations, rows = 3, []
    for k, T in enumerate((1, 3, 5, 600)):
        band = rng.uniform(0.5, 2.0, (T, COLS, 4))
        band[..., 1:3] *= 0.1                                      # a diagonally dominant band
        y = rng.standard_normal((T, COLS))
        offset = rng.standard_normal((T, COLS)) if k % 2 else None
        rows.append((s.i(band), s.i(offset) if k % 2 else None, s.o(y.size, init=y), T,
                     s.o(iterations + 1) if k != 1 else None))
    arr = _jobs(_lib.GvAscentJob, rows)
    return s.fn('kwy_gv_ascent', 'kwy_gv_ascent_batch_dev')(
        s.ctx.handle, arr, len(rows), COLS, s.i(rng.uniform(0.5, 2.0, COLS)), s.i(rng.uniform(0.01, 0.1, COLS)),
        0.0 if bad else 1.0, iterations, s.o(len(rows), np.int32))


def c_gv_stats_from_moments(s, d, bad):
    return s.fn('kwy_gv_stats_from_moments', 'kwy_gv_stats_from_moments_dev')(
        s.ctx.handle, s.i(d.moments), len(d.moments), 0 if bad else COLS, s.o(COLS), s.o(COLS))


CASES = [c_cheaptrick, c_d4c, c_logf0_moments, c_logf0_moments_merge, c_f0_map, c_column_moments, c_gv_from_moments,
         c_gv_postfilter, c_ms_logspectra, c_ms_stats_update, c_ms_postfilter, c_pitch_shift, c_formant_shift, c_mcd,
         c_f0_error, c_moments_merge, c_sp2mc, c_mc2sp, c_code_aperiodicity, c_decode_aperiodicity, c_stretch_log, c_mc2b,
         c_mlsa_synthesis, c_mcep_filter_fft, c_fastdtw, c_np_normal, c_gv_ascent, c_gv_stats_from_moments]
GROUP_CASES = [c_gv_postfilter_group, c_ms_postfilter_group, c_formant_shift_group]
USES_MS_STATS = {c_ms_stats_update, c_ms_postfilter, c_ms_postfilter_group}


def _run(ctx, case, d, dev, bad, ms_stats):
    from kwiiyatta_amd import _lib
    s = Side(ctx, dev)
    rc = case(s, d, bad, ms_stats) if case in USES_MS_STATS else case(s, d, bad)
    err = ctx.error() if rc != _lib.KWY_OK else ''
    if dev:
        ctx.sync()
    return rc, err, s.results()


def _name(case):
    return case.__name__[2:]


@pytest.mark.parametrize('case', CASES + GROUP_CASES, ids=_name)
def test_host_entry_equals_its_device_twin(ctx, d, ms_stats, case):
    from kwiiyatta_amd import _lib
    rc_h, err_h, host = _run(ctx, case, d, False, False, ms_stats)
    rc_d, err_d, dev = _run(ctx, case, d, True, False, ms_stats)
    assert rc_h == _lib.KWY_OK, err_h
    assert rc_d == _lib.KWY_OK, err_d
    assert len(host) == len(dev) > 0
    written = 0
    for k, ((h, before, g, n), (v, _, _, _)) in enumerate(zip(host, dev)):
        assert h.dtype == v.dtype and h.tobytes() == v.tobytes(), f'{_name(case)}: output {k} differs'
        for side, a in (('host', h), ('device', v)):
            assert np.array_equal(a[:g], before[:g]) and np.array_equal(a[g + n:], before[g + n:]), \
                f'{_name(case)}: the {side} form wrote outside output {k}'
        written += h.tobytes() != before.tobytes()
    assert written > 0, 'the call wrote nothing'


@pytest.mark.parametrize('case', CASES, ids=_name)
def test_refusal_equals_the_device_twins_and_writes_nothing(ctx, d, ms_stats, case):
    from kwiiyatta_amd import _lib
    rc_h, err_h, host = _run(ctx, case, d, False, True, ms_stats)
    rc_d, err_d, dev = _run(ctx, case, d, True, True, ms_stats)
    assert rc_h == rc_d == _lib.KWY_EINVAL
    assert err_h == err_d and err_h
    for a, before, _, _ in host + dev:
        assert a.tobytes() == before.tobytes(), f'{_name(case)}: a refused call wrote to an output'
