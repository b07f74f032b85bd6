"""The band-aperiodicity conversion on the device (include/kwy.h, "aperiodicity conversion"; kwy_bap.hip): band track,
training rows, apply and band error at their edges, the device forms against the host forms, the per-file conversion
against the oracle chain, training through the converter, the model file, and a synthetic sanity check.

Inputs, restatement and bounds: tests/bap_cases.py (checked on the CPU in test_bap_cases.py).  Where the contract asks
for the arithmetic of an existing kernel the comparison is bit for bit against that kernel (kwy_code_aperiodicity,
kwy_decode_aperiodicity, kwy_delta_features_dev).  Every test with a tolerance prints its measured maxima."""
from types import SimpleNamespace

import numpy as np
import pytest

import bap_cases as bc
import codec_cases as cc

pytestmark = pytest.mark.gpu

P = bc.PASS_FRAMES        # 256 = BAP_PASS, the track kernel's frames per pass


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


@pytest.fixture(autouse=True)
def numpy_state_as_found():
    """the tests here seed numpy's global generator (the silence pads are drawn from it): later test files find it as
    they would without this one"""
    state = np.random.get_state()
    yield
    np.random.set_state(state)


def _device_delta(g):
    """kwy_delta_features_dev on a gathered sequence (n, B) -> (n, 3 B)"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import c_vp, lib
    n, B = g.shape
    if n == 0:
        return np.zeros((0, 3 * B))
    x = torch.from_numpy(np.ascontiguousarray(g)).cuda()
    count = torch.tensor([n], dtype=torch.int64, device='cuda')
    out = torch.empty((n, 3 * B), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    ctx = _lib.default_context()
    _lib.check(ctx, lib.kwy_delta_features_dev(ctx.handle, c_vp(x.data_ptr()), c_vp(count.data_ptr()), n, B,
                                               c_vp(out.data_ptr())))
    ctx.sync()
    return out.cpu().numpy()


# ---- band track ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fs,fft_size', bc.PAIRS)
def test_track(ko, fs, fft_size):
    """every pattern at T in {1, 2, P, P + 1, 2 P + 1}, the patterns of one T as one batched call: flags and fill
    bit-equal to the restatement on the device's own coded values (so voiced rows are the coder's bits), the voicing
    the pattern's, voiced rows within CODE_ABS of the oracle.  The device's own coded values come from
    kw.code_aperiodicity, the host form: kwy_code_aperiodicity_dev's kernel behind a staging copy."""
    from kwiiyatta_amd.backend import bap, world as kw
    B = cc.bands(fs)
    worst = 0.0
    for T in bc.FRAMES:
        pats = bc.patterns(T)
        aps = [bc.ap_for(v, fs, fft_size, seed=i) for i, v in enumerate(pats.values())]
        tracks = bap.track(aps, fs)
        for (name, v), ap, S in zip(pats.items(), aps, tracks):
            coded = kw.code_aperiodicity(ap, fs)
            assert S.shape == (T, B + 1), (T, name)
            assert np.array_equal(S[:, 0] == 1.0, v), (T, name)
            assert np.array_equal(S, bc.fill(coded)), (T, name)
            assert np.array_equal(S[v, 1:], coded[v]), (T, name)
            if v.any():
                worst = max(worst, np.abs(S[v, 1:] - ko.code_aperiodicity(ap, fs)[v]).max())
    print(f'band track fs={fs} fft_size={fft_size}: voiced rows max |got - oracle| = {worst:.3e} dB')
    assert worst <= cc.CODE_ABS


def test_track_classifies_threshold_rows_to_the_ulp():
    """129 constant rows whose one band steps through -0.5 dB, 9 ulp apart: both classes occur and every row is
    classified as the restatement classifies the device's own coded value (> -0.5 is unvoiced, -0.5 is not)"""
    from kwiiyatta_amd.backend import bap, world as kw
    rows = bc.threshold_ap()
    coded = kw.code_aperiodicity(rows, 16000)
    S = bap.track(rows, 16000)
    flags = bc.flags(coded)
    assert 0 < flags.sum() < len(flags)
    assert np.array_equal(S[:, 0], flags)
    assert np.array_equal(S, bc.fill(coded))
    print(f'threshold rows: coded values within {np.abs(coded + 0.5).max():.3e} dB of -0.5, {int(flags.sum())} voiced')


def test_track_batch_beyond_one_table_equals_single_calls():
    """one job more than a by-value table holds (16): a second launch; every job equals its single call bit for bit,
    through the host form and through the device forms"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import c_vp, lib
    from kwiiyatta_amd.backend import bap
    fs, fft_size = 44100, 2048
    B = cc.bands(fs)
    n = bc.TABLE_JOBS + 1
    voicings = [np.random.default_rng(i).random(3 + 31 * i) < 0.6 for i in range(n)]
    aps = [bc.ap_for(v, fs, fft_size, seed=i) for i, v in enumerate(voicings)]
    single = [bap.track(ap, fs) for ap in aps]
    batched = bap.track(aps, fs)
    assert all(np.array_equal(a, b) for a, b in zip(single, batched))
    ctx = _lib.default_context()
    d_ap = [torch.from_numpy(ap).cuda() for ap in aps]
    d_tr = [torch.full((len(ap), B + 1), float('nan'), dtype=torch.float64, device='cuda') for ap in aps]
    torch.cuda.synchronize()
    bap.track_batch_dev(ctx, list(zip(d_ap, d_tr)), fs, fft_size)
    ctx.sync()
    assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(single, d_tr))
    one = torch.full_like(d_tr[5], float('nan'))
    _lib.check(ctx, lib.kwy_bap_track_dev(ctx.handle, c_vp(d_ap[5].data_ptr()), len(aps[5]), fs, fft_size,
                                          c_vp(one.data_ptr())))
    ctx.sync()
    assert np.array_equal(single[5], one.cpu().numpy())


# ---- training rows ---------------------------------------------------------------------------------------------------
def _pair(B, seed, Tx=300, Ty=310, n=700):
    X, Y = bc.random_track(Tx, B, seed), bc.random_track(Ty, B, seed + 1000)
    ix, iy = bc.random_lists(n, Tx, Ty, seed)
    return X, Y, ix, iy


@pytest.mark.parametrize('B', [1, 5])
def test_rows(B):
    """700 cells (two full rounds of 256 and a part): kept rows bit-equal to kwy_delta_features_dev on the gathered
    sequences, selected by the restatement; n = 0, no cell voiced on both sides, all cells voiced; a cursor above 0; a
    pair that overflows the capacity"""
    from kwiiyatta_amd.backend import bap
    X, Y, ix, iy = _pair(B, 10 * B)
    want = bc.joint_rows(X, Y, ix, iy, _device_delta)
    assert 0 < len(want) < len(ix)
    joint, cursor, n = bap.rows(X, Y, ix, iy)
    assert cursor == n == len(want) and np.array_equal(joint[:n], want)
    assert not joint[n:].any()                                           # nothing written behind the rows
    # n = 0
    none = np.zeros(0, dtype=np.int32)
    joint, cursor, n = bap.rows(X, Y, none, none, joint=np.full((4, 6 * B), np.nan), cursor=2)
    assert (cursor, n) == (2, 0) and np.isnan(joint).all()
    # no cell voiced on both sides
    Y0 = Y.copy()
    Y0[:, 0] = 0.0
    joint, cursor, n = bap.rows(X, Y0, ix, iy)
    assert (cursor, n) == (0, 0) and not joint.any()
    # all cells voiced
    X1, Y1 = X.copy(), Y.copy()
    X1[:, 0] = Y1[:, 0] = 1.0
    joint, cursor, n = bap.rows(X1, Y1, ix, iy)
    assert cursor == n == len(ix)
    assert np.array_equal(joint, np.hstack((_device_delta(X1[ix, 1:]), _device_delta(Y1[iy, 1:]))))
    # a cursor that starts above 0
    room = np.full((len(want) + 5, 6 * B), np.nan)
    joint, cursor, n = bap.rows(X, Y, ix, iy, joint=room, cursor=3)
    assert cursor == 3 + len(want) and n == len(want)
    assert np.isnan(joint[:3]).all() and np.array_equal(joint[3:cursor], want) and np.isnan(joint[cursor:]).all()
    # overflow: the first pair fits, the second is dropped whole, the third (small) still fits behind the first
    X2, Y2, ix2, iy2 = _pair(B, 10 * B + 1, n=40)
    small = bc.joint_rows(X2, Y2, ix2, iy2, _device_delta)
    assert 0 < len(small) < len(want)
    room = np.full((len(want) + len(small), 6 * B), np.nan)
    joint, cursor, ns = bap.rows([X, X, X2], [Y, Y, Y2], [ix, ix, ix2], [iy, iy, iy2], joint=room)
    assert ns.tolist() == [len(want), -1 - len(want), len(small)] and cursor == len(want) + len(small)
    assert np.array_equal(joint[:len(want)], want) and np.array_equal(joint[len(want):], small)


def test_rows_device_form_with_device_counts():
    """17 pairs (one more than a table holds) through kwy_bap_rows_batch_dev with the cell counts as device words, some
    below the lists' capacity: the matrix of the host form on the truncated lists, in job order"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import bap
    B, n_pairs = 2, bc.TABLE_JOBS + 1
    pairs = [_pair(B, 50 + k, Tx=40 + k, Ty=45 + k, n=60 + 3 * k) for k in range(n_pairs)]
    used = [len(p[2]) - (k % 3) * 7 for k, p in enumerate(pairs)]
    want, _, n_want = bap.rows([p[0] for p in pairs], [p[1] for p in pairs], [p[2][:u].copy() for p, u in zip(pairs, used)],
                               [p[3][:u].copy() for p, u in zip(pairs, used)])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tensors = [[dev(a) for a in p] for p in pairs]
    n_dev = dev(np.array(used, dtype=np.int64))
    n_rows = torch.zeros(n_pairs, dtype=torch.int64, device='cuda')
    joint = torch.zeros(want.shape, dtype=torch.float64, device='cuda')
    cursor = torch.zeros(1, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    ctx = _lib.default_context()
    jobs = [bap.rows_job(t[0], t[1], t[2], t[3], n_rows[k:k + 1], n_dev=n_dev[k:k + 1]) for k, t in enumerate(tensors)]
    bap.rows_batch_dev(ctx, jobs, B, joint, cursor)
    ctx.sync()
    assert n_rows.tolist() == n_want.tolist() and int(cursor[0]) == int(n_want.sum())
    assert np.array_equal(joint.cpu().numpy(), want)


# ---- apply -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fs,fft_size', [(16000, 1024), (44100, 2048), (48000, 742), (48000, 6)])
def test_apply(fs, fft_size):
    """a NaN buffer: unvoiced rows stay NaN, voiced rows are kwy_decode_aperiodicity's bits on the clamped row --
    converted values of +3, -80, exactly -60 and exactly -1e-12 dB, a mixed row, a row whose mean lies above -0.5 dB
    (the decoder's flat row) and random rows"""
    from kwiiyatta_amd.backend import bap, world as kw
    B, K = cc.bands(fs), fft_size // 2 + 1
    rng = np.random.default_rng([fs, fft_size])
    mixed = np.resize([3.0, -80.0, -60.0, -1e-12, -7.0], B)
    fixed = [np.full(B, 3.0), np.full(B, -80.0), np.full(B, -60.0), np.full(B, -1e-12), mixed, np.full(B, -0.1)]
    bands = np.vstack(fixed + [-rng.uniform(1.0, 70.0, (10, B))])
    bands = np.vstack((bands, bands))                      # every row once voiced, once unvoiced
    T = len(bands)
    v = np.r_[np.ones(T // 2), np.zeros(T // 2)]
    src = np.hstack((v[:, None], -rng.uniform(5.0, 40.0, (T, B))))
    conv = np.ascontiguousarray(np.hstack((v[:, None], bands)))
    ap = np.full((T, K), np.nan)
    assert bap.apply(src, conv, ap, fs) is ap
    voiced = v == 1.0
    assert np.isnan(ap[~voiced]).all()
    want = kw.decode_aperiodicity(np.ascontiguousarray(bc.clamp(bands)), fs, fft_size)
    assert np.array_equal(ap[voiced], want[voiced])
    flat = (ap[voiced] == cc.UNVOICED).all(axis=1)
    expect = [True, False, False, True, bool(np.mean(bc.clamp(mixed)) > -0.5), True]
    assert flat[:6].tolist() == expect and not flat[6:].any()
    # no voiced frame: the buffer is left as it is; a list of two jobs equals the single calls
    untouched = np.full((T, K), np.nan)
    bap.apply(np.hstack((np.zeros((T, 1)), src[:, 1:])), conv, untouched, fs)
    assert np.isnan(untouched).all()
    a1, a2 = np.full((T, K), np.nan), np.full((5, K), np.nan)
    bap.apply([src, src[:5].copy()], [conv, conv[:5].copy()], [a1, a2], fs)
    assert np.array_equal(a1[voiced], ap[voiced]) and np.array_equal(a2, ap[:5])


def test_apply_device_forms():
    """17 utterances through kwy_bap_apply_batch_dev and one through kwy_bap_apply_dev: the host form's bits"""
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import c_vp, lib
    from kwiiyatta_amd.backend import bap
    fs, fft_size = 32000, 1024
    B, K = cc.bands(fs), fft_size // 2 + 1
    n = bc.TABLE_JOBS + 1
    srcs = [bc.random_track(2 + 9 * i, B, 70 + i) for i in range(n)]
    convs = [np.ascontiguousarray(np.hstack((s[:, :1], s[:, 1:] - 6.0))) for s in srcs]
    want = [np.full((len(s), K), np.nan) for s in srcs]
    bap.apply(srcs, convs, want, fs)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    d_src, d_conv = [dev(s) for s in srcs], [dev(c) for c in convs]
    d_ap = [torch.full((len(s), K), float('nan'), dtype=torch.float64, device='cuda') for s in srcs]
    torch.cuda.synchronize()
    ctx = _lib.default_context()
    bap.apply_batch_dev(ctx, list(zip(d_src, d_conv, d_ap)), fs, fft_size)
    ctx.sync()
    assert all(np.array_equal(w, a.cpu().numpy(), equal_nan=True) for w, a in zip(want, d_ap))
    one = torch.full_like(d_ap[7], float('nan'))
    _lib.check(ctx, lib.kwy_bap_apply_dev(ctx.handle, c_vp(d_src[7].data_ptr()), c_vp(d_conv[7].data_ptr()), len(srcs[7]),
                                          fs, fft_size, c_vp(one.data_ptr())))
    ctx.sync()
    assert np.array_equal(want[7], one.cpu().numpy(), equal_nan=True)


# ---- band error ------------------------------------------------------------------------------------------------------
def _check_error(got, cells, want, want_cells, what):
    assert got[0] == want[0], what
    assert np.array_equal(np.isnan(cells), np.isnan(want_cells)), what
    live = ~np.isnan(want_cells)
    e_cell = (np.abs(cells[live] - want_cells[live]) / np.maximum(want_cells[live], 1e-300)).max() if live.any() else 0.0
    e_mean = abs(got[1] / want[1] - 1) if want[0] else abs(got[1])
    e_m2 = abs(got[2] - want[2]) / max(want[2], 1e-300) if want[0] > 1 else abs(got[2])
    print(f'band error {what}: n = {int(got[0])}, per cell {e_cell:.3e}, mean {e_mean:.3e}, M2 {e_m2:.3e} (relative)')
    assert e_cell <= bc.ERROR_CELL_REL and e_mean <= bc.ERROR_SUM_REL and e_m2 <= 100 * bc.ERROR_SUM_REL, what


@pytest.mark.parametrize('B', [1, 5])
def test_error(B):
    """without lists, with lists, with offsets that put cells outside either track (passed over), no cell voiced on both
    sides; a list of 17 jobs equals the single calls.  M2 is a sum of squared deviations from the mean: its relative
    error takes the mean's error twice over the spread, bounded here by 100 times the sum bound."""
    from kwiiyatta_amd.backend import bap
    X, Y, ix, iy = _pair(B, 30 + B)
    m, cells = bap.error(X, X[::-1].copy(), per_row=True)
    _check_error(m, cells, *bc.band_error(X, X[::-1].copy()), 'no lists')
    m, cells = bap.error(X, Y, idx_a=ix, idx_b=iy, per_row=True)
    want = bc.band_error(X, Y, ix, iy)
    assert 0 < want[0][0] < len(ix)
    _check_error(m, cells, *want, 'lists')
    off = 7
    inside = (ix >= off) & (iy >= off)
    assert 0 < inside.sum() < len(ix)
    m, cells = bap.error(X, Y, idx_a=ix, idx_b=iy, off_a=off, off_b=off, per_row=True)
    w_m, w_cells = bc.band_error(X, Y, ix[inside] - off, iy[inside] - off)
    full = np.full(len(ix), np.nan)
    full[inside] = w_cells
    _check_error(m, cells, w_m, full, 'offsets')
    Y0 = Y.copy()
    Y0[:, 0] = 0.0
    assert bap.error(X, Y0, idx_a=ix, idx_b=iy).tolist() == [0.0, 0.0, 0.0]
    n = bc.TABLE_JOBS + 1
    many = bap.error([X] * n, [Y] * n, idx_a=[ix[:40 + k].copy() for k in range(n)], idx_b=[iy[:40 + k].copy() for k in range(n)])
    for k in range(n):
        assert np.array_equal(many[k], bap.error(X, Y, idx_a=ix[:40 + k].copy(), idx_b=iy[:40 + k].copy())), k


def test_error_device_form_with_device_counts():
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import bap
    B = 3
    X, Y, ix, iy = _pair(B, 90)
    used = [len(ix), 300, 0]
    want = np.array([bap.error(X, Y, idx_a=ix[:u].copy(), idx_b=iy[:u].copy()) if u else np.zeros(3) for u in used])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dX, dY, dix, diy, n_dev = dev(X), dev(Y), dev(ix), dev(iy), dev(np.array(used, dtype=np.int64))
    moments = torch.full((3, 3), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    ctx = _lib.default_context()
    bap.error_batch_dev(ctx, [bap.error_job(dX, dY, dix, diy, n_dev=n_dev[k:k + 1]) for k in range(3)], B, moments)
    ctx.sync()
    assert np.array_equal(moments.cpu().numpy(), want)


# ---- end to end, per file --------------------------------------------------------------------------------------------
def _banded_converter(fs, gmm, frame_period=5):
    """a converter stack that holds nothing but a band mixture"""
    import kwiiyatta_amd as k
    conv = k.MelCepstrumConverter(components=1)
    conv.order, conv.fs = 2, fs
    conv.base.frame_period = frame_period
    stack = conv._band_stack(len(gmm.weights_))
    stack.gmm.weights_, stack.gmm.means_, stack.gmm.covariances_ = gmm.weights_, gmm.means_, gmm.covariances_
    stack.frame_period = frame_period
    conv.ap_converter = stack
    return conv


def _smooth_ap(fs, fft_size, T=40):
    """T frames whose level moves smoothly between -12 and -52 dB, unvoiced at both ends and in a run inside"""
    rng = np.random.default_rng([fs, fft_size, T])
    level = -(0.6 + (1.0 + np.sin(np.arange(T) / 5.0)))
    ap = 10.0 ** (level[:, None] + 0.05 * rng.random((T, fft_size // 2 + 1)))
    v = np.ones(T, dtype=bool)
    v[:3] = v[17:22] = v[-2:] = False
    ap[~v] = cc.UNVOICED
    return ap, v


@pytest.mark.parametrize('fs,fft_size', [(16000, 1024), (48000, 2048)])
def test_convert_aperiodicity_against_the_oracle_chain(ko, fs, fft_size):
    """convert_aperiodicity against ko.code_aperiodicity, the restated fill, ko.gmm_mlpg at d = B, clamp and
    ko.decode_aperiodicity; a random well-conditioned mixture, M = 2, T = 40.  The dB bound is the one of
    test_backends_gpu.py::test_gmm_mlpg / ::test_mlpg_solve_partition_edges (1e-10 relative to the data's scale) at
    60 dB; the decoded bound DECODE_REL + ln 10 / 20 times it.  Unvoiced rows are the input's bits."""
    B = cc.bands(fs)
    gmm = bc.BandGMM(B, M=2, seed=fs)
    conv = _banded_converter(fs, gmm)
    ap, v = _smooth_ap(fs, fft_size)
    feature = SimpleNamespace(fs=fs, frame_period=5, aperiodicity=ap)
    S = bc.fill(ko.code_aperiodicity(ap, fs))
    assert np.array_equal(S[:, 0] == 1.0, v)
    y, mix = ko.gmm_mlpg(np.ascontiguousarray(S[:, 1:]), gmm.weights_, gmm.means_, gmm.covariances_, return_mix=True)
    assert len(np.unique(mix)) == 2                                     # both components are chosen somewhere
    want_db = bc.clamp(y)
    assert np.abs(y).max() <= bc.SCALE_DB and (want_db[v].mean(axis=1) < -1.0).all()
    own, mapped = conv.convert_band_track(feature)
    assert np.array_equal(own[:, 0], S[:, 0]) and np.array_equal(mapped[:, 0], S[:, 0])
    e_db = np.abs(mapped[:, 1:] - want_db).max()
    got = conv.convert_aperiodicity(feature)
    assert got is not ap and got.shape == ap.shape and np.array_equal(got[~v], ap[~v])
    want = ko.decode_aperiodicity(np.ascontiguousarray(want_db), fs, fft_size)
    e_dec = np.abs(got[v] / want[v] - 1).max()
    print(f'convert_aperiodicity fs={fs}: bands max |got - oracle| = {e_db:.3e} dB (bound {bc.E2E_DB:.1e}), decoded max '
          f'|got / oracle - 1| = {e_dec:.3e} (bound {bc.E2E_DECODED_REL:.2e})')
    assert e_db <= bc.E2E_DB and e_dec <= bc.E2E_DECODED_REL


# ---- training through the converter, the model file -----------------------------------------------------------------
FS = 16000


@pytest.fixture(scope='module')
def pairs():
    """two short synthetic parallel pairs at 16 kHz (one band)"""
    import kwiiyatta_amd as kw
    from kwiiyatta_amd.synthetic import make_utterance
    out = {}
    for k in range(2):
        sides = [make_utterance(seed=seed + k, fs=FS, seconds=1.0 + 0.1 * k, time_warp=warp, formant_scale=form)[0]
                 for seed, warp, form in ((300, 1.0, 1.0), (400, 1.1, 1.12))]
        out[f'{k:02}'] = tuple(kw.Analyzer(kw.Wavdata(FS, x)) for x in sides)
    return out


def test_training_fits_the_band_mixture_on_the_restated_rows(pairs, tmp_path):
    """train(ap_model=True): the mel-cepstrum mixture is the one of a training without it (same pads, same rows); the
    band mixture is the fit of the restated rows -- the sides' own band tracks along the index lists of the same
    alignment, kwy_delta_features_dev on the gathered sequences --; convert_aperiodicity is track, mixture, apply; the
    model file brings all of it back"""
    import kwiiyatta_amd as kw
    from kwiiyatta_amd.backend import bap
    from kwiiyatta_amd.converter import PaddedDataset, TrimmedDataset, align_dataset
    from kwiiyatta_amd.vocoder.align import even_indices
    keys = sorted(pairs)
    make = lambda: kw.MelCepstrumConverter(use_delta=True, components=2, random_state=0, max_iter=5)  # noqa: E731
    np.random.seed(4)
    plain = make()
    plain.train(align_dataset(pairs), keys)
    assert plain.ap_converter is None
    np.random.seed(4)
    conv = make()
    conv.train(align_dataset(pairs), keys, ap_model=True, ap_components=2)
    assert np.array_equal(conv.gmm.means_, plain.gmm.means_) and np.array_equal(conv.gmm.covariances_, plain.gmm.covariances_)
    assert conv.align_iterations == 0 and conv.fs == FS
    # the restated rows, from the padded sides' own tracks and index lists
    np.random.seed(4)
    padded = PaddedDataset(TrimmedDataset(pairs), bands=True)
    blocks = []
    for key in keys:
        padded[key]
        x, y = padded.sides[key]
        assert x.band_track.shape == (x.frame_len, 2) and not x.band_track[:100, 0].any()       # pads are unvoiced
        xs, ys = even_indices(x, y, padded.pad_len)
        blocks.append(bc.joint_rows(x.band_track, y.band_track, xs, ys, _device_delta))
    matrix = np.concatenate(blocks)
    assert conv.ap_rows == len(matrix) > 20
    ref = conv._band_stack(2)
    ref._train(matrix)
    band = conv.ap_converter.gmm
    assert np.array_equal(band.means_, ref.gmm.means_) and np.array_equal(band.covariances_, ref.gmm.covariances_)
    assert band.means_.shape == (2, 6) and band.max_iter == 5 and band.random_state == 0
    # conversion: unvoiced frames are the source's, voiced frames the decode of the converted track
    source = pairs[keys[0]][0]
    ap = np.ascontiguousarray(source.aperiodicity, dtype=np.float64)
    got = conv.convert_aperiodicity(source)
    own, mapped = conv.convert_band_track(source)
    v = own[:, 0] == 1.0
    assert 0 < v.sum() < len(v) and np.array_equal(got[~v], ap[~v]) and not np.array_equal(got[v], ap[v])
    again = ap.copy()
    bap.apply(own, mapped, again, FS)
    assert np.array_equal(got, again) and np.array_equal(np.ascontiguousarray(source.aperiodicity), ap)
    # the model file
    path = tmp_path / 'model.npz'
    conv.save(path)
    loaded = kw.MelCepstrumConverter(use_delta=True).load(path)
    assert loaded.ap_converter.gmm.n_components == 2
    assert np.array_equal(loaded.convert_aperiodicity(source), got)
    plain.save(path)
    assert kw.MelCepstrumConverter(use_delta=True).load(path).ap_converter is None
    with pytest.raises(ValueError, match='no band mixture'):
        plain.convert_aperiodicity(source)
    # the commands' per-file paths
    from kwiiyatta_amd import convert_voice, evaluate_voice
    # (a synthetic utterance may have no frame whose 3 kHz band is coded below -0.5 dB: such a pair has no band frames)
    results, total = evaluate_voice.evaluate(conv, TrimmedDataset(pairs), keys, convert_ap=True)
    assert all({'bap', 'bap_source', 'bap_frames'} <= set(r.as_dict()) for r in results)
    assert all(np.isfinite(r.bap) and np.isfinite(r.bap_source) if r.bap_frames else np.isnan(r.bap) for r in results)
    assert total.bap_frames == sum(r.bap_frames for r in results) > 0
    assert np.isfinite(total.bap) and np.isfinite(total.bap_source)
    assert min(r.bap for r in results if r.bap_frames) <= total.bap <= max(r.bap for r in results if r.bap_frames)
    off = evaluate_voice.evaluate_pair(conv, *TrimmedDataset(pairs)[keys[0]])
    assert off.bap_frames == 0 and np.isnan(off.bap) and np.isnan(off.bap_source) and 'bap' not in off.as_dict()
    print(f'evaluate: band error {total.bap:.3f} dB (source {total.bap_source:.3f} dB) over {total.bap_frames} frames '
          f'of {[r.bap_frames for r in results]}')


def test_convert_command_renders_with_the_converted_aperiodicity(pairs, tmp_path):
    """convert_voice.convert(convert_ap=True): the synthesised output differs from the one on the source's aperiodicity
    and is the synthesis of the feature set with `convert_aperiodicity` in place; the differential output does not
    change"""
    import kwiiyatta_amd as kw
    from kwiiyatta_amd import convert_voice
    from kwiiyatta_amd.converter import align_dataset
    keys = sorted(pairs)
    np.random.seed(4)
    conv = kw.MelCepstrumConverter(use_delta=True, components=2, random_state=0, max_iter=5)
    conv.train(align_dataset(pairs), keys, ap_model=True, ap_components=2)
    wav = tmp_path / 'source.wav'
    pairs[keys[0]][0].wavdata.save(wav)
    conf = SimpleNamespace(create_analyzer=lambda path, Analyzer=None: Analyzer(path, frame_period=5, mcep_order=24))
    off = convert_voice.convert(conf, conv, wav, diffvc=False)
    on = convert_voice.convert(conf, conv, wav, diffvc=False, convert_ap=True)
    assert on.data.shape == off.data.shape and not np.array_equal(on.data, off.data)
    source = convert_voice.analyze_source(conf, conv, wav)
    rendered = kw.feature(source)
    rendered.mel_cepstrum = conv.convert(source.mel_cepstrum, diff=False)
    rendered.aperiodicity = conv.convert_aperiodicity(source)
    assert np.array_equal(rendered.synthesize().data, on.data)
    d_off = convert_voice.convert(conf, conv, wav, diffvc=True)
    d_on = convert_voice.convert(conf, conv, wav, diffvc=True, convert_ap=True)
    assert np.array_equal(d_on.data, d_off.data)


# ---- sanity, synthetic -----------------------------------------------------------------------------------------------
def test_conversion_moves_the_bands_towards_the_target():
    """pairs whose target bands are the source's minus 10 dB plus N(0, 0.5 dB), M = 2: the converted band error must be
    below the unconverted source's (about 10 dB); the ratio is printed, not asserted"""
    from kwiiyatta_amd.backend import bap
    from kwiiyatta_amd.backend.mlpg import MLPG
    from kwiiyatta_amd.converter import GMMFeatureConverter
    B, T = 3, 300
    rng = np.random.default_rng(11)

    def pair(seed):
        X = bc.random_track(T, B, seed)
        Y = X.copy()
        Y[:, 1:] = X[:, 1:] - 10.0 + 0.5 * rng.standard_normal((T, B))
        return X, np.ascontiguousarray(Y)
    line = np.arange(T, dtype=np.int32)
    train = [pair(s) for s in range(6)]
    joint, cursor, _ = bap.rows([p[0] for p in train], [p[1] for p in train], [line] * 6, [line] * 6)
    stage = GMMFeatureConverter(components=2, random_state=0)
    stage._train(joint[:cursor])
    X, Y = pair(99)
    bands = MLPG(stage.gmm, diff=False).transform(np.ascontiguousarray(X[:, 1:]))
    mapped = np.ascontiguousarray(np.hstack((X[:, :1], bap.clamp(bands))))
    m = bap.error([mapped, X], [Y, Y])
    assert m[0, 0] == m[1, 0] == (X[:, 0] == 1.0).sum() > 0
    print(f'synthetic sanity: band error converted {m[0, 1]:.3f} dB, source {m[1, 1]:.3f} dB, ratio {m[0, 1] / m[1, 1]:.3f} '
          f'over {int(m[0, 0])} frames, {cursor} training rows')
    assert m[0, 1] < m[1, 1]


# ---- device drivers --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def triples():
    """the (x, f0, t) triples of two short synthetic parallel pairs at 16 kHz, as the corpus drivers take them"""
    from kwiiyatta_amd.backend import world
    from kwiiyatta_amd.synthetic import make_utterance
    out = []
    for k in range(2):
        pair = []
        for seed, warp, form in ((300 + k, 1.0, 1.0), (400 + k, 1.1, 1.12)):
            x, _, _ = make_utterance(seed=seed, fs=FS, seconds=1.0 + 0.1 * k, time_warp=warp, formant_scale=form)
            f0, t = world.dio(x, FS, frame_period=5)
            pair.append((x, world.stonemask(x, f0, t, FS), t))
        out.append(tuple(pair))
    return out


def test_convert_wave_equals_the_per_file_path(triples):
    """ConvertWave(ap_gmm=...) on the (x, f0, t) triples of two utterances: the rows of `ap_all` are bit-equal to
    `convert_aperiodicity` on the aperiodicity the same wave analyses without ap_gmm; without ap_gmm the wave has no
    band buffers and `ap_all` is D4C's; a mixture of another band count is refused"""
    import torch
    from kwiiyatta_amd import corpus as cp
    from kwiiyatta_amd.pipeline import DeviceGMM
    gmm = bc.BandGMM(1, M=2, seed=3)
    conv = _banded_converter(FS, gmm)
    utterances = [pair[0] for pair in triples]
    ls = cp._Lockstep(0)
    plain = cp.ConvertWave(ls, FS, utterances)
    plain.run()
    ls.sync()
    assert plain.ap_gmm is None and not hasattr(plain, 'ap_src') and not hasattr(plain, 'j_bap')
    dg = DeviceGMM(gmm.weights_, gmm.means_, gmm.covariances_, ls.dev)
    wave = cp.ConvertWave(ls, FS, utterances, ap_gmm=dg)
    wave.run()
    ls.sync()
    analysed, got = plain.ap_all.cpu().numpy(), wave.ap_all.cpu().numpy()
    r0 = 0
    for T in wave.T:
        ap = np.ascontiguousarray(analysed[r0:r0 + T])
        want = conv.convert_aperiodicity(SimpleNamespace(fs=FS, frame_period=5, aperiodicity=ap))
        voiced = wave.ap_src[r0:r0 + T, 0].cpu().numpy() == 1.0
        assert 0 < voiced.sum() < T and not np.array_equal(want[voiced], ap[voiced])
        assert np.array_equal(got[r0:r0 + T], want)
        r0 += T
    assert not torch.equal(wave.wave_all, plain.wave_all)              # the rendering read the converted rows
    wide = bc.BandGMM(2, M=2, seed=3)
    with pytest.raises(ValueError, match='band'):
        cp.ConvertWave(ls, FS, utterances, ap_gmm=DeviceGMM(wide.weights_, wide.means_, wide.covariances_, ls.dev))
    # the batch driver: the same waveforms as the wave's, and the stream driver refuses the option
    full = bc.BandGMM(24, M=1, seed=1)
    out = cp.convert_batch(utterances, FS, full, ap_gmm=gmm)
    off = cp.convert_batch(utterances, FS, full)
    assert all(a.shape == b.shape and not torch.equal(a, b) for a, b in zip(out, off))
    with pytest.raises(ValueError, match='ap_gmm needs the lockstep driver'):
        cp.convert_batch(utterances, FS, full, ap_gmm=gmm, driver='streams')


def test_training_matrix_with_bands_equals_the_restatement(triples):
    """build_training_matrix(bands=True) on two pairs: the mel-cepstrum matrix is the one without bands; the band matrix
    is bit-equal to the restatement fed with the wave's own read-back tracks -- every padded item coded as ONE job -- and
    index lists; the tracks are the host form's on the padded aperiodicity; a re-alignment pass gives band rows along
    ITS alignment, and a cache without tracks says why it cannot"""
    import torch
    from kwiiyatta_amd import corpus as cp
    from kwiiyatta_amd.backend import bap
    silence = np.random.RandomState(7)
    saved = np.random.get_state()
    np.random.set_state(silence.get_state())
    from kwiiyatta_amd.pipeline import draw_silence
    table = [[draw_silence(FS, 513) for _ in range(4)] for _ in triples]
    np.random.set_state(saved)
    pads = lambda i: table[i]  # noqa: E731
    X, frames = cp.build_training_matrix(triples, FS, silence_for=pads)
    Xb0, frames_b, cache, Xb = cp.build_training_matrix(triples, FS, silence_for=pads, keep=True, bands=True)
    assert frames == frames_b and torch.equal(X, Xb0) and Xb.shape[1] == 6 and len(Xb) > 20
    w = cache.waves[0]
    assert w.track.shape == (w.layout.total, 2) and cache.nbytes == w.layout.total * 8 * (2 * 24 + 4 + 2)
    # the same wave again, by hand: tracks, index lists and rows read back
    ls = cp._Lockstep(0)
    wave = cp.TrainWave(ls, FS, [tuple(tuple(s) for s in pair) for pair in triples], bands=True)
    wave.analyse()

    def fill_pads(rows):
        for k in range(len(rows) // 4):
            for dst, a in zip(rows[4 * k:4 * k + 4], table[k]):
                dst.copy_(torch.from_numpy(a).to(dst.device))
    a = wave.align(fill_pads)
    idx_x, idx_y, cap, n_sel = a.index_lists()
    ls.sync()
    blocks = []
    for k in range(wave.n):
        Tp = a.inputs.Tp
        tx, ty = (wave.reg(wave.track, 2 * k + s)[:Tp[2 * k + s]].cpu().numpy() for s in (0, 1))
        for s, tr in ((0, tx), (1, ty)):
            ap_pad = wave.reg(wave.ap_pad, 2 * k + s)[:Tp[2 * k + s]].cpu().numpy()
            assert np.array_equal(tr, bap.track(np.ascontiguousarray(ap_pad), FS))          # a padded item is one job
            assert not tr[:100, 0].any() and not tr[-100:, 0].any()                         # pads are unvoiced
        n = int(n_sel[k])
        blocks.append(bc.joint_rows(tx, ty, idx_x[k][:n].cpu().numpy(), idx_y[k][:n].cpu().numpy(), _device_delta))
    assert np.array_equal(Xb.cpu().numpy(), np.concatenate(blocks))
    # a re-alignment pass
    g = cp.fit_converter(X, components=2, seed=0, max_iter=3)
    X1, mcd1, Xb1 = cp.realign_training_matrix(cache, g, bands=True)
    assert Xb1.shape[1] == 6 and len(Xb1) > 0 and np.isfinite(mcd1)
    X1p, mcd1p = cp.realign_training_matrix(cache, g)
    assert torch.equal(X1, X1p) and mcd1 == mcd1p
    _, _, bare = cp.build_training_matrix(triples, FS, silence_for=pads, keep=True)
    assert bare.waves[0].track is None
    with pytest.raises(ValueError, match='holds no band tracks'):
        cp.realign_training_matrix(bare, g, bands=True)
    with pytest.raises(ValueError, match='12 kHz'):
        cp.build_training_matrix(triples, 8000, bands=True)
    g2, history, band = cp.train_converter_realigned(triples, FS, components=2, seed=0, max_iter=3, silence_for=pads,
                                                     align_iterations=1, ap_components=2)
    assert len(history) == 2 and band.means_.shape == (2, 6)
    ref = cp.fit_converter(cp.realign_training_matrix(cache, cp.fit_converter(X, components=2, seed=0, max_iter=3),
                                                      bands=True)[2], components=2, seed=0, max_iter=3)
    assert np.array_equal(band.means_, ref.means_)                      # fitted on the LAST alignment's band rows


def test_evaluate_batch_reports_the_band_error(triples, pairs):
    """evaluate_batch(ap_gmm=...): the band error of every pair and the pooled one, equal to evaluate_pair's under the
    same pads (bit-equal counts; means within the sum bound); without ap_gmm the records have no band keys"""
    import kwiiyatta_amd as kw
    from kwiiyatta_amd import corpus as cp, evaluate_voice
    from kwiiyatta_amd.converter import TrimmedDataset, align_dataset
    keys = sorted(pairs)
    np.random.seed(4)
    conv = kw.MelCepstrumConverter(use_delta=True, components=2, random_state=0, max_iter=5)
    conv.train(align_dataset(pairs), keys, ap_model=True, ap_components=2)
    np.random.seed(9)
    records, total = cp.evaluate_batch(triples, FS, conv.gmm, ap_gmm=conv.ap_converter.gmm)
    np.random.seed(9)
    plain, _ = cp.evaluate_batch(triples, FS, conv.gmm)
    assert all('bap_moments' not in r for r in plain) and all('bap_moments' in r for r in records)
    assert [r['mcd_moments'] for r in plain] == [r['mcd_moments'] for r in records]
    np.random.seed(9)
    want = [evaluate_voice.evaluate_pair(conv, *TrimmedDataset(pairs)[key], convert_ap=True) for key in keys]
    worst = 0.0
    for rec, w in zip(records, want):
        for got, ref in ((rec['bap_moments'], w.bap_moments), (rec['bap_source_moments'], w.bap_source_moments)):
            assert got[0] == ref[0]
            if ref[0]:
                worst = max(worst, abs(got[1] / ref[1] - 1))
    print(f'evaluate_batch band error against evaluate_pair: mean max relative difference {worst:.3e}; frames '
          f'{[int(r["bap_moments"][0]) for r in records]}, pooled {total["bap_moments"][1]:.3f} dB '
          f'(source {total["bap_source_moments"][1]:.3f} dB)')
    assert worst <= bc.ERROR_SUM_REL and total['bap_moments'][0] == sum(r['bap_moments'][0] for r in records) > 0
