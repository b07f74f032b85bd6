"""k_code_aperiodicity / k_decode_aperiodicity at their edges (tests/codec_cases.py; the inputs are checked on the CPU
in test_codec_cases.py): every band count from 0 to 5, transform lengths that are no power of two, one frame, rows at
both ends of the value range and a 114 dB step under a band centre, the -0.5 dB voicing threshold to the ulp, and the
refusal of more coded columns than the rate has bands.

Checker: the CPU oracle.  Bounds (derived in codec_cases.py, not measured): code within 1e-12 dB, decode within 1e-13
relative, the same frames unvoiced bit for bit.  Every test prints its measured maxima."""
import numpy as np
import pytest

import codec_cases as cc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('fs,fft_size', cc.PAIRS)
def test_code_then_decode(fs, fft_size):
    from oracle import oracle as ko
    from kwiiyatta_amd.backend import world as kw
    nb = cc.bands(fs)
    assert kw.get_num_aperiodicities(fs) == nb
    e_code = e_dec = 0.0
    for name, ap in cc.inputs(fs, fft_size).items():
        ref = ko.code_aperiodicity(ap, fs)
        got = kw.code_aperiodicity(ap, fs)
        assert got.shape == ref.shape == (len(ap), nb), name
        e_code = max(e_code, np.abs(got - ref).max())
        for cols in sorted({nb, 1}):                         # all bands; truncated to one, as when the rate is lowered
            coded = np.ascontiguousarray(ref[:, :cols])
            want = ko.decode_aperiodicity(coded, fs, fft_size)
            back = kw.decode_aperiodicity(coded, fs, fft_size)
            assert back.shape == want.shape, name
            assert np.array_equal(back == cc.UNVOICED, want == cc.UNVOICED), (name, cols)
            e_dec = max(e_dec, np.abs(back / want - 1).max())
    print(f'codec fs={fs} fft_size={fft_size}: code max |got - ref| = {e_code:.3e} dB, '
          f'decode max |got / ref - 1| = {e_dec:.3e}')
    assert e_code <= cc.CODE_ABS, e_code
    assert e_dec <= cc.DECODE_REL, e_dec


@pytest.mark.parametrize('T', cc.FRAMES)
def test_rate_without_bands(T):
    """8 kHz has no band: code returns KWY_OK and writes nothing, decode of no columns gives 1 - 1e-12 everywhere"""
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, ptr
    fs, fft_size = 8000, 1024
    assert cc.bands(fs) == 0
    ctx = _lib.Context(0)
    ap = cc.random_rows(fs, fft_size, T)
    coded = np.full((T, 1), np.nan)
    assert lib.kwy_code_aperiodicity(ctx.handle, ptr(ap), T, fs, fft_size, ptr(coded)) == _lib.KWY_OK
    ctx.sync()
    assert np.isnan(coded).all()
    out = np.full_like(ap, np.nan)
    _lib.check(ctx, lib.kwy_decode_aperiodicity(ctx.handle, ptr(coded), T, fs, fft_size, 0, ptr(out)))
    assert np.all(out == cc.UNVOICED)


def test_voicing_threshold_to_the_ulp():
    """a frame is unvoiced when the mean of its coded values is above -0.5 dB, not when it is -0.5 dB"""
    from oracle import oracle as ko
    from kwiiyatta_amd.backend import world as kw
    for fs, coded, flags in cc.threshold_cases():
        got, want = kw.decode_aperiodicity(coded, fs, 1024), ko.decode_aperiodicity(coded, fs, 1024)
        assert np.array_equal(got == cc.UNVOICED, want == cc.UNVOICED), fs
        assert (got == cc.UNVOICED).all(axis=1).tolist() == flags, fs
        err = np.abs(got / want - 1).max()
        print(f'codec threshold rows fs={fs}: decode max |got / ref - 1| = {err:.3e}')
        assert err <= cc.DECODE_REL


def test_more_columns_than_bands_is_refused():
    """5 coded columns at 16 kHz (one band): the centres 6 kHz .. 15 kHz lie at or above fs/2 = 8 kHz, the node grid
    does not increase -- KWY_EINVAL from the host and the device entry, nothing written; the band count itself passes"""
    import torch
    from oracle import oracle as ko
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, c_vp, ptr
    fs, fft_size, T = 16000, 1024, 4
    K = fft_size // 2 + 1
    ctx = _lib.Context(0)
    coded = -np.random.default_rng(0).uniform(3.0, 40.0, (T, 5))
    out = np.full((T, K), np.nan)
    rc = lib.kwy_decode_aperiodicity(ctx.handle, ptr(coded), T, fs, fft_size, 5, ptr(out))
    assert rc == _lib.KWY_EINVAL and 'more bands' in ctx.error()
    assert np.isnan(out).all()
    d_coded = torch.from_numpy(coded).cuda()
    d_out = torch.full((T, K), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    rc = lib.kwy_decode_aperiodicity_dev(ctx.handle, c_vp(d_coded.data_ptr()), T, fs, fft_size, 5, c_vp(d_out.data_ptr()))
    ctx.sync()
    assert rc == _lib.KWY_EINVAL and bool(torch.isnan(d_out).all())
    one = np.ascontiguousarray(coded[:, :1])
    _lib.check(ctx, lib.kwy_decode_aperiodicity(ctx.handle, ptr(one), T, fs, fft_size, 1, ptr(out)))
    assert np.abs(out / ko.decode_aperiodicity(one, fs, fft_size) - 1).max() <= cc.DECODE_REL
