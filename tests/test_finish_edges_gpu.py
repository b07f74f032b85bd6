"""kwy_finish_pcm16_batch_dev where the last 1 ms piece starts inside the waveform and ends beyond it.

The reference's loop limits `data[fs * i // 1000 : fs * (i + 1) // 1000]` for every frame i, and numpy clips a slice
that runs past the end.  k_fin_pieces scans the piece in LDS; before it clipped the piece's end to the staged sample
count it also scanned LDS words behind the waveform that the workgroup had not written.  Whatever lay there took part
in the piece's peak, and a large leftover scaled the waveform's last samples down.

Checker: the package's host path (Synthesizer.finish + Wavdata._pcm16), int16 for int16.  So that the leftover
matters, the last in-range samples lie below the piece ceiling (the right gain is 1), and every call is preceded, on the
same context, by a post-step call on 64 one-second waveforms of amplitude ~1e3 whose pieces are not limited: that
leaves large values in the LDS of most compute units.  What a workgroup finds in LDS it has not written is not
guaranteed by anything -- the fix in the kernel rests on reading the code; this module is the regression guard (run
once against the kernel without the clip on an MI355X, every straddling case here failed)."""
import numpy as np
import pytest

from test_f0_finish_gpu import _device_pcm, _host_pcm

pytestmark = pytest.mark.gpu

CEILING = 10 ** (-1 / 10)                     # normalize_data's default peak_lv = -1
FIN_MS = 64                                   # 1 ms pieces per workgroup of k_fin_pieces

# (fs, frames, samples): the last piece [fs (F-1) // 1000, fs F // 1000) holds sample n - 1 and ends behind n
STRADDLING = [(16000, 40, 631),
              (44100, 30, 44100 * 29 // 1000 + 1),             # one sample in the piece
              (48000, 1, 5),
              (16000, 65, 16000 * 64 // 1000 + 3),             # the piece is the first one of the second workgroup
              (44100, 65, 44100 * 64 // 1000 + 3)]


def _wave(fs, frames, n):
    """quiet noise with an offset; a loud start, so that some other piece is limited (and the save step's gain is not
    1), while the last piece stays below the ceiling"""
    rng = np.random.default_rng([fs, frames, n])
    y = rng.standard_normal(n) * 0.1 + 0.05
    lo = fs * (frames - 1) // 1000
    if lo > 8:
        y[:4] = (2.0, -1.5, 1.0, 3.0)
    y[-1] = 0.45
    assert lo < n < fs * frames // 1000
    assert np.abs(y[lo:] - y.mean()).max() < 0.75 * CEILING
    return y


def _prime(ctx, fs):
    """64 loud one-second waveforms through the post-step, no piece limited (frame_len 0): their samples stay in LDS"""
    import torch
    from kwiiyatta_amd.backend import finish
    gen = torch.Generator(device='cuda').manual_seed(fs)
    ys = [torch.randn(fs, dtype=torch.float64, device='cuda', generator=gen) * 1e3 for _ in range(64)]
    pcm = [torch.empty(fs, dtype=torch.int16, device='cuda') for _ in ys]
    torch.cuda.synchronize()
    finish.pcm16_batch_dev(ctx, ys, [0] * len(ys), fs, pcm)
    ctx.sync()


def _primed_pcm(ctx, ys, frames, fs):
    _prime(ctx, fs)
    return _device_pcm(ctx, ys, frames, fs)


@pytest.mark.parametrize('fs,frames,n', STRADDLING)
def test_last_piece_ends_beyond_the_waveform(fs, frames, n):
    from kwiiyatta_amd import _lib
    assert (frames - 1) // FIN_MS == (0 if frames < 65 else 1)
    y = _wave(fs, frames, n)
    want = _host_pcm(y, frames, fs)
    lo = fs * (frames - 1) // 1000
    assert np.abs(want[lo:]).max() > 300                     # a tail scaled by a stale peak would be a few units
    got = _primed_pcm(_lib.Context(0), [y], [frames], fs)[0]
    assert np.array_equal(got, want), (int(np.abs(got.astype(int) - want.astype(int)).max()), got[lo:], want[lo:])


@pytest.mark.parametrize('fs,frames', [(fs, frames) for fs, frames, _ in STRADDLING])
def test_acceptance_boundary(fs, frames):
    """n = fs (F - 1) // 1000 samples: the last piece is empty, refused by both paths as before; one sample more: the
    piece holds that one sample, accepted and equal"""
    import kwiiyatta_amd as k
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    n0 = fs * (frames - 1) // 1000
    if n0 > 0:                                               # (frames = 1: no waveform at all)
        y = _wave(fs, frames, n0 + 1)[:n0].copy()
        with pytest.raises(ValueError):
            _device_pcm(ctx, [y], [frames], fs)
        with pytest.raises(ValueError):
            k.Synthesizer.finish(k.Wavdata(fs, y.copy()), frames)
    y = _wave(fs, frames, n0 + 1)
    got = _primed_pcm(ctx, [y], [frames], fs)[0]
    assert np.array_equal(got, _host_pcm(y, frames, fs))


@pytest.mark.parametrize('fs', sorted({fs for fs, _, _ in STRADDLING}))
def test_batch_equals_single_calls(fs):
    """a batch has one sampling rate: every case of that rate above, its boundary case and two ordinary waveforms in
    one call equal the single calls and the host path"""
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    rng = np.random.default_rng(fs)
    jobs = [(frames, n) for f, frames, n in STRADDLING if f == fs]
    jobs += [(frames, fs * (frames - 1) // 1000 + 1) for frames, _ in list(jobs)]
    ys = [_wave(fs, frames, n) for frames, n in jobs]
    frames = [f for f, _ in jobs]
    for n, F in ((fs // 2 + 77, 100), (9000, 9000 * 1000 // fs)):
        y = rng.standard_normal(n) * 0.3 + 0.1
        y[n // 3:n // 3 + 50] *= 6.0
        ys.append(y)
        frames.append(F)
    got = _primed_pcm(ctx, ys, frames, fs)
    for i, (y, F) in enumerate(zip(ys, frames)):
        assert np.array_equal(got[i], _host_pcm(y, F, fs)), (i, len(y), F)
        assert np.array_equal(got[i], _primed_pcm(ctx, [y], [F], fs)[0]), (i, len(y), F)
