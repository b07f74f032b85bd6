"""Formant shift on the MI355X: the warp kernel of kwy_formant.hip through the C ABI against its numpy statement
(tests/formant_cases.py), its in-place, batched and host forms, its status words and argument checks, and the lockstep
drivers and Feature.shift_formants on top of it.

Measured on an MI355X over test_kernel_against_the_statement's cases (K in {2, 3, 65, 513, 1025, 2049}, rows in
{0, 1, 3, 67}, six ratios, values exp(uniform(-30, 2))): the largest relative deviation from the statement where it
interpolates is 3.664e-15 (MEASURED_DEVIATION below); KERNEL_BOUND is four times that, 1.47e-14, rounded up to one
significant digit: 2e-14.
Where the statement copies, the kernel is bit-equal."""

import numpy as np
import pytest

import formant_cases as fc
from conftest import CLB_WAV

pytestmark = pytest.mark.gpu

MEASURED_DEVIATION = 3.664e-15          # at (K, rows, ratio) = (1025, 67, 2 ** (-3 / 12))
KERNEL_BOUND = 2e-14
FS = 16000


def _device():
    """device, stream, context: the tests upload from pageable memory (complete on return), launch on the stream,
    synchronise it and read back"""
    import torch
    from kwiiyatta_amd import _lib
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    return dev, stream, _lib.Context(0, stream=stream.cuda_stream)


def _compare(got, sp, ratio, where):
    """bit-equal where the statement copies; -> the largest relative deviation elsewhere"""
    want, _ = fc.shift(sp, ratio)
    assert got.shape == want.shape, where
    if ratio == 1 or not len(sp):
        assert got.tobytes() == want.tobytes(), where
        return 0.0
    _, _, copied = fc.taps(sp.shape[1], ratio)
    assert got[:, copied].tobytes() == want[:, copied].tobytes(), where
    if copied.all():
        return 0.0
    return float(np.abs(got[:, ~copied] / want[:, ~copied] - 1).max())


def test_kernel_against_the_statement():
    from kwiiyatta_amd.backend import formant
    rng = np.random.RandomState(0)
    worst, at = 0.0, None
    for K in fc.WIDTHS:
        mats = [fc.envelope(rng, rows, K) for rows in fc.ROWS]
        for ratio in fc.RATIOS:
            for sp in mats:
                got = formant.shift_formants(sp, ratio)
                assert got is not sp
                dev = _compare(got, sp, ratio, (K, len(sp), ratio))
                if dev > worst:
                    worst, at = dev, (K, len(sp), ratio)
    print(f'formant shift: largest relative deviation from the statement = {worst:.3e} at (K, rows, ratio) = {at}')
    assert worst <= KERNEL_BOUND, (worst, at)
    assert worst > 0                                     # (the interpolating branch did run)


def _shift_dev(ctx, sp_t, ratio, out_t, status_t=None):
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    _lib.check(ctx, lib.kwy_formant_shift_dev(ctx.handle, sp_t.data_ptr(), sp_t.shape[0], sp_t.shape[1], ratio,
                                              out_t.data_ptr(), None if status_t is None else status_t.data_ptr()))


def test_in_place_host_and_device_forms_are_bit_equal():
    import torch
    from kwiiyatta_amd.backend import formant
    dev, stream, ctx = _device()
    rng = np.random.RandomState(1)
    for K in (2, 65, 1025, 2048, fc.MAX_K):            # (2048: the widest row of the kernel's smaller staging buffer)
        for rows in (1, 67, 200):
            sp = fc.envelope(rng, rows, K)
            for ratio in (0.5, 2.0 ** (-3 / 12), 1.0, 2.0 ** (1 / 12), 2.0):
                host = formant.shift_formants(sp, ratio)
                assert _compare(host, sp, ratio, (K, rows, ratio)) <= KERNEL_BOUND
                src = torch.from_numpy(sp).to(dev)
                out = torch.full_like(src, -1.0)
                inplace = src.clone()
                status = torch.full((2,), -1, dtype=torch.int32, device=dev)
                _shift_dev(ctx, src, ratio, out, status[0:1])
                _shift_dev(ctx, inplace, ratio, inplace, status[1:2])
                stream.synchronize()
                assert src.cpu().numpy().tobytes() == sp.tobytes()
                assert out.cpu().numpy().tobytes() == host.tobytes(), (K, rows, ratio)
                assert inplace.cpu().numpy().tobytes() == host.tobytes(), (K, rows, ratio)
                assert status.cpu().tolist() == [0, 0]


def test_a_batch_equals_the_single_calls():
    import torch
    from kwiiyatta_amd.backend import formant
    dev, stream, ctx = _device()
    rng = np.random.RandomState(2)
    for K, row_counts in ((65, (0, 1, 67, 3)), (1025, (0, 1, 67, 3)), (513, tuple(range(35)))):   # (35 jobs: two launches)
        mats = [fc.envelope(rng, rows, K) for rows in row_counts]
        for ratio in (2.0 ** (-3 / 12), 1.5):
            singles = [formant.shift_formants(m, ratio) for m in mats]
            listed = formant.shift_formants(mats, ratio)
            srcs = [torch.from_numpy(m).to(dev) for m in mats]
            outs = [torch.full_like(s, -1.0) for s in srcs]
            status = torch.full((len(mats),), -1, dtype=torch.int32, device=dev)
            formant.shift_formants_batch_dev(ctx, srcs, outs, ratio, status=status)
            inplace = [s.clone() for s in srcs]
            formant.shift_formants_batch_dev(ctx, inplace, inplace, ratio)
            stream.synchronize()
            assert status.cpu().tolist() == [0] * len(mats)
            for one, a, b, c in zip(singles, listed, outs, inplace):
                assert a.tobytes() == one.tobytes() and b.cpu().numpy().tobytes() == one.tobytes()
                assert c.cpu().numpy().tobytes() == one.tobytes()


def test_status_words_count_the_unusable_rows():
    import torch
    from kwiiyatta_amd.backend import formant
    dev, stream, ctx = _device()
    rng = np.random.RandomState(3)
    for K in (3, 65, 1025):
        mats = [fc.envelope(rng, rows, K) for rows in (67, 1, 200, 3, 0)]
        clean = [m.copy() for m in mats]
        planted = [fc.plant(mats[0], rng, 9), fc.plant(mats[1], rng, 1), fc.plant(mats[2], rng, 4), [], []]
        for ratio in (2.0 ** (1 / 12), 0.5, 1.0):
            srcs = [torch.from_numpy(m).to(dev) for m in mats]
            outs = [torch.full_like(s, -1.0) for s in srcs]
            status = torch.full((len(mats),), -1, dtype=torch.int32, device=dev)
            formant.shift_formants_batch_dev(ctx, srcs, outs, ratio, status=status)
            stream.synchronize()
            words = [0] * 5 if ratio == 1 else [len(p) for p in planted]      # (at 1 nothing is examined)
            assert status.cpu().tolist() == words, (K, ratio)
            for m, c, o, bad in zip(mats, clean, outs, planted):
                got = o.cpu().numpy()
                want, count = fc.shift(m, ratio)
                assert count == (0 if ratio == 1 else len(bad))
                for r in range(len(m)):
                    if r in bad or ratio == 1:
                        assert got[r].tobytes() == m[r].tobytes(), (K, ratio, r)
                good = [r for r in range(len(m)) if r not in bad]
                assert _compare(got[good], c[good], ratio, (K, ratio)) <= KERNEL_BOUND
            if ratio != 1:
                with pytest.raises(ValueError, match=r'14 row\(s\) of matrix / matrices \[0, 1, 2\]'):
                    formant.check_status(status)
                with pytest.raises(ValueError, match=r'9 row\(s\) of matrix / matrices \[0\]'):
                    formant.shift_formants(mats[0], ratio)


@pytest.mark.parametrize('ratio', [0.49, 2.01, float('nan'), float('inf')])
def test_a_ratio_out_of_range_is_refused_and_nothing_is_written(ratio):
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    dev, stream, ctx = _device()
    sp = fc.envelope(np.random.RandomState(4), 5, 65)
    src = torch.from_numpy(sp).to(dev)
    out = torch.full_like(src, -7.0)
    status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    rc = lib.kwy_formant_shift_dev(ctx.handle, src.data_ptr(), 5, 65, ratio, out.data_ptr(), status.data_ptr())
    assert rc == _lib.KWY_EINVAL and 'ratio' in ctx.error()
    jobs = _lib.job_array(_lib.FormantJob, [(src, 5, out)])
    assert lib.kwy_formant_shift_batch_dev(ctx.handle, jobs, 1, 65, ratio, status.data_ptr()) == _lib.KWY_EINVAL
    stream.synchronize()
    assert bool((out == -7.0).all()) and status.cpu().tolist() == [-7]
    host_out = np.full_like(sp, -7.0)
    host_status = np.full(1, -7, dtype=np.int32)
    jobs = _lib.job_array(_lib.FormantJob, [(sp.ctypes.data, 5, host_out.ctypes.data)])
    assert lib.kwy_formant_shift(ctx.handle, jobs, 1, 65, ratio, _lib.ptr(host_status)) == _lib.KWY_EINVAL
    assert np.all(host_out == -7.0) and host_status[0] == -7


def test_shapes_and_types_the_shim_refuses():
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    from kwiiyatta_amd.backend import formant
    sp = fc.envelope(np.random.RandomState(5), 4, 10)
    with pytest.raises(ValueError, match='C-contiguous'):
        formant.shift_formants(sp[:, ::2], 1.5)
    with pytest.raises(ValueError, match='dtype mismatch'):
        formant.shift_formants(sp.astype(np.float32), 1.5)
    with pytest.raises(ValueError, match='bins'):
        formant.shift_formants(np.ones((4, 1)), 1.5)
    with pytest.raises(ValueError, match='bins'):
        formant.shift_formants(np.ones((1, fc.MAX_K + 1)), 1.5)
    with pytest.raises(ValueError, match='differ'):
        formant.shift_formants([sp, np.ones((2, 11))], 1.5)
    assert formant.shift_formants([], 1.5) == []
    ctx = _lib.default_context()
    out = np.full((1, fc.MAX_K + 1), -7.0)
    big = np.ones((1, fc.MAX_K + 1))
    jobs = _lib.job_array(_lib.FormantJob, [(big.ctypes.data, 1, out.ctypes.data)])
    assert lib.kwy_formant_shift(ctx.handle, jobs, 1, fc.MAX_K + 1, 1.5, None) == _lib.KWY_EINVAL
    assert lib.kwy_formant_shift(ctx.handle, jobs, 1, 1, 1.5, None) == _lib.KWY_EINVAL
    assert np.all(out == -7.0)
    assert fc.MAX_K == 4096 // 2 + 1                      # (CheapTrick's longest transform)


# ---- drivers -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def utterances():
    from kwiiyatta_amd.synthetic import make_utterance
    return [make_utterance(seed=31, fs=FS, seconds=0.25), make_utterance(seed=32, fs=FS, seconds=0.25, f0_base=190.0)]


@pytest.fixture(scope='module')
def mixture():
    from kwiiyatta_amd import pipeline as pl
    return pl.synthetic_gmm(order=24, components=4, seed=0, n_frames=3000)


RATIO = 2.0 ** (3 / 12)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _wave(utterances, gmm=None, **options):
    """one ConvertWave run: (the envelope rows its rendering read, the wave)"""
    from kwiiyatta_amd import corpus
    ls = corpus._Lockstep(0)
    wv = corpus.ConvertWave(ls, FS, utterances, gmm=gmm, **options)
    wv.run()
    ls.sync()
    rendered = wv.sp_all if gmm is None else wv.sp_conv
    return rendered.cpu().numpy().copy(), wv


def test_resynthesize_batch_with_a_ratio(utterances):
    import torch
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd.backend import formant
    plain, frames = corpus.resynthesize_batch(utterances, FS)
    same, _ = corpus.resynthesize_batch(utterances, FS, formant_ratio=1.0)
    shifted, frames_s = corpus.resynthesize_batch(utterances, FS, formant_ratio=RATIO)
    assert frames == frames_s == sum(len(u[1]) for u in utterances)
    sp_plain, wv_plain = _wave(utterances)
    sp_shift, wv_shift = _wave(utterances, formant_ratio=RATIO)
    assert wv_plain.formant_status is None and wv_shift.formant_status.cpu().tolist() == [0]
    assert sp_shift.tobytes() == formant.shift_formants(sp_plain, RATIO).tobytes()
    for i in range(len(utterances)):
        assert _bytes(same[i]) == _bytes(plain[i]) == _bytes(wv_plain.wave[i]), i
        assert _bytes(shifted[i]) == _bytes(wv_shift.wave[i]), i
        assert plain[i].shape == shifted[i].shape and _bytes(shifted[i]) != _bytes(plain[i]), i
        assert bool(torch.isfinite(shifted[i]).all()), i


def test_convert_batch_with_a_ratio(utterances, mixture):
    import torch
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd import pipeline as pl
    from kwiiyatta_amd.backend import formant
    plain = corpus.convert_batch(utterances, FS, mixture, diff=True)
    same = corpus.convert_batch(utterances, FS, mixture, diff=True, formant_ratio=1.0)
    shifted = corpus.convert_batch(utterances, FS, mixture, diff=True, formant_ratio=RATIO)
    dg = pl.DeviceGMM(mixture.weights_, mixture.means_, mixture.covariances_, torch.device('cuda', 0))
    sp_plain, wv_plain = _wave(utterances, gmm=dg, diff=True)
    sp_shift, wv_shift = _wave(utterances, gmm=dg, diff=True, formant_ratio=RATIO)
    assert wv_shift.formant_status.cpu().tolist() == [0]
    assert sp_shift.tobytes() == formant.shift_formants(sp_plain, RATIO).tobytes()
    for i in range(len(utterances)):
        assert _bytes(same[0][i]) == _bytes(plain[0][i]) == _bytes(wv_plain.wave[i]), i
        assert _bytes(shifted[0][i]) == _bytes(wv_shift.wave[i]) and _bytes(shifted[0][i]) != _bytes(plain[0][i]), i
        # the differential outputs do not see the ratio
        assert _bytes(shifted[2][i]) == _bytes(plain[2][i]) == _bytes(same[2][i]) == _bytes(wv_shift.wave_diff[i]), i
    # a row the kernel cannot warp is reported after the batch, by wave
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    ls = corpus._Lockstep(0)
    wv = corpus.ConvertWave(ls, FS, utterances, formant_ratio=RATIO)
    wv.run()
    ls.sync()
    wv.sp_all[3, 7] = 0.0
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(ls.main):
        _lib.check(ls.ctx, lib.kwy_formant_shift_dev(ls.ctx.handle, wv.sp_all.data_ptr(), wv.rows, wv.K, RATIO,
                                                     wv.sp_all.data_ptr(), wv.formant_status.data_ptr()))
    ls.sync()
    with pytest.raises(ValueError, match=r'1 row\(s\) of wave\(s\) \[0\]'):
        formant.check_status(wv.formant_status, what='wave(s)')


def test_feature_shift_formants_on_an_analysed_file():
    import kwiiyatta_amd as k
    analysed = k.analyze_wav(CLB_WAV)
    sp = np.ascontiguousarray(analysed.spectrum_envelope).copy()
    f0, ap = analysed.f0, analysed.aperiodicity
    for semitones in (3.0, -5.0):
        ratio = 2.0 ** (semitones / 12)
        warped = k.shift_formants(analysed, ratio)
        dev = _compare(np.ascontiguousarray(warped.spectrum_envelope), sp, ratio, semitones)
        print(f'analysed file, {semitones:+g} semitones: relative deviation from the statement = {dev:.3e}')
        assert 0 < dev <= KERNEL_BOUND
        assert warped.f0 is f0 and warped.aperiodicity is ap
        assert analysed.spectrum_envelope.tobytes() == sp.tobytes()
        mc = warped.mel_cepstrum.data
        fresh = k.feature(analysed.fs)
        fresh.spectrum_envelope = warped.spectrum_envelope
        assert mc.tobytes() == fresh.mel_cepstrum.data.tobytes()
        assert np.abs(mc - analysed.mel_cepstrum.data).max() > 1e-2
