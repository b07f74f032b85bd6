"""The frame-parallel FFT differential filter without a GPU: the numpy restatement of its contract
(tests/fftfilt_cases.py) against the MLSA oracle, the size helper, and the host logic that carries --diff-filter from
the command lines to the filters.  The kernel itself is held to the restatement in test_fftfilt_gpu.py.

Measured over the committed cases (printed by the tests, -s shows them):
  constant coefficients, restatement (the exact LTI filter) against the oracle's Pade approximant, maximum difference
  over the reference's peak, seeds 10..12:
      fs     order  N     pd 4                       pd 5
      16000  24     1024  4.8e-05 3.8e-05 4.6e-05    4.0e-05 3.2e-05 3.9e-05
      22050  33     1024  4.7e-05 4.0e-05 4.4e-05    3.9e-05 3.3e-05 3.7e-05
      48000  48     2048  3.9e-05 4.7e-05 5.0e-05    3.2e-05 3.9e-05 4.2e-05
      96000  60     4096  4.0e-05 3.3e-05 3.6e-05    3.4e-05 2.8e-05 3.0e-05
  largest 4.987e-05 -> asserted 1.0e-04 (twice, room for other seeds).  The values do not shrink from Pade order 4 to
  5: SPTK's rounded Pade constants, not the approximation order, set them.
  slowly varying coefficients (the random walk of test_hip_mlsa_on_speech on arctic_a0001, 16 kHz, 738 frames), output
  crossfade against coefficient interpolation: RMS of the difference over the RMS of the reference 2.449e-03, maximum
  over the peak 4.540e-03 -> asserted 4.9e-03 and 9.1e-03.  This is the model difference between the two filters, not
  an error of either; a transform four times as long changes the restatement by 1e-15.  Crossfading one frame early or
  late gives 2.1e-02 / 2.2e-02 RMS: the contract's alignment is the one the MLSA filter's interpolation has.
  Independently drawn frames (scale 0.4) differ by 1.1e-01 RMS; not asserted."""
import copy
import inspect
import types

import numpy as np
import pytest
from scipy.io import wavfile

import fftfilt_cases as fc
from conftest import CLB_WAV

CONSTANT_BOUND = 1.0e-4          # twice the largest value of the table above
WALK_RMS_BOUND, WALK_PEAK_BOUND = 4.9e-3, 9.1e-3


@pytest.mark.parametrize('fs,order', [(16000, 24), (22050, 33), (48000, 48), (96000, 60)])
@pytest.mark.parametrize('pd', [4, 5])
def test_restatement_is_the_lti_filter_the_mlsa_filter_approximates(fs, order, pd):
    from oracle import oracle as ko
    hop = fs // 200
    N = fc.fft_size(fs, hop)
    alpha = ko.mcepalpha(fs)
    T = 60
    for seed in (10, 11, 12):
        rng = np.random.default_rng(seed)
        mc = np.tile(fc.mcep(rng, order, 0.4), (T, 1))
        x = fc.signal(rng, T * hop + 5)
        ref = ko.mlsa_synthesis(x, ko.mc2b(mc, alpha), alpha, hop, pd)
        got = fc.fft_filter(x, mc, alpha, hop, N)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f'constant fs={fs} order={order} N={N} pd={pd} seed={seed}: {err:.3e}')
        assert err <= CONSTANT_BOUND, err


def test_crossfade_against_interpolation_on_speech():
    from oracle import oracle as ko
    fs, d = wavfile.read(CLB_WAV)
    x = np.ascontiguousarray(d.astype(np.float64) / 2 ** 15)
    rng = np.random.default_rng(4)
    hop, order = 80, 24
    T = len(x) // hop + 1
    alpha = ko.mcepalpha(fs)
    walk = np.cumsum(rng.standard_normal((T, order)) * 0.02, axis=0) / np.arange(1, order + 1)
    mc = np.hstack([np.zeros((T, 1)), walk])
    ref = ko.mlsa_synthesis(x, ko.mc2b(mc, alpha), alpha, hop)
    got = fc.fft_filter(x, mc, alpha, hop, fc.fft_size(fs, hop))
    rms = np.sqrt(np.mean((got - ref) ** 2)) / np.sqrt(np.mean(ref ** 2))
    peak = np.abs(got - ref).max() / np.abs(ref).max()
    print(f'random walk on speech, {T} frames: rms {rms:.3e} peak {peak:.3e}')
    assert rms <= WALK_RMS_BOUND and peak <= WALK_PEAK_BOUND, (rms, peak)


@pytest.mark.parametrize('name,n_of,T', fc.EDGES, ids=[e[0] for e in fc.EDGES])
def test_zero_tail_equals_the_oracles(name, n_of, T):
    from oracle import oracle as ko
    fs, order, N, hop = fc.RATES[0]
    alpha = ko.mcepalpha(fs)
    rng = np.random.default_rng(20)
    n = n_of(hop)
    mc = fc.frames(rng, T, order)
    x = fc.signal(rng, n) + 0.5                          # (no sample is zero: a processed frame shows)
    ref = ko.mlsa_synthesis(x, ko.mc2b(mc, alpha), alpha, hop)
    got = fc.fft_filter(x, mc, alpha, hop, N)
    nproc = min(T, (n - 1) // hop)
    assert got.shape == ref.shape == (n,)
    assert np.array_equal(got == 0.0, ref == 0.0)
    assert np.all(got[nproc * hop:] == 0.0) and np.all(got[:nproc * hop] != 0.0)
    if n <= hop:
        assert not got.any()


def test_fft_size_helper_needs_no_device():
    from kwiiyatta_amd import _lib
    size = _lib.lib.kwy_mcep_filter_fft_size
    for fs, want in ((16000, 1024), (22050, 1024), (44100, 2048), (48000, 2048), (96000, 4096)):
        hop = int(fs * 0.005)
        assert size(fs, hop) == want == fc.fft_size(fs, hop), fs
    assert size(48000, 8192 - 1200) == 8192 and size(48000, 8192 - 1199) == 0      # hop + 25 ms beyond 8192
    assert size(16000, 8000) == 0 and size(0, 80) == 0 and size(16000, 0) == 0
    for fs in (8000, 11025, 32000, 192000):
        for hop in (1, fs // 200, fs // 100, 3000):
            assert size(fs, hop) == fc.fft_size(fs, hop), (fs, hop)
    from kwiiyatta_amd.backend import fftfilt
    assert fftfilt.fft_filter_size(48000, 240) == 2048
    with pytest.raises(ValueError, match='8192'):
        fftfilt.fft_filter_size(48000, 8000)


def test_new_entry_points_are_in_the_ctypes_table():
    from kwiiyatta_amd import _lib
    for name, args in (('kwy_mcep_filter_fft_size', 2), ('kwy_mcep_filter_fft', 11), ('kwy_mcep_filter_fft_dev', 11),
                       ('kwy_mcep_filter_fft_batch_dev', 8)):
        assert name in _lib.SIGNATURES and name not in _lib.MISSING
        assert len(_lib.SIGNATURES[name][1]) == args, name


# ---------------------------------------------------------------------------------- the option's way down
def test_the_option_and_its_defaults():
    import kwiiyatta_amd as k
    from kwiiyatta_amd import config, convert_voice, corpus, resynthesize_voice

    def parsed(args):
        conf = k.Config()
        conf.add_diff_filter_argument()
        conf.parser.parse_args(args=args, namespace=conf)
        return conf
    assert config.DIFF_FILTER_OPTION[0] == '--diff-filter'
    assert parsed([]).diff_filter == 'mlsa' and parsed(['--diff-filter', 'fft']).diff_filter == 'fft'
    assert parsed(['--diff-filter', 'mlsa']).diff_filter == 'mlsa'
    with pytest.raises(SystemExit):
        parsed(['--diff-filter', 'iir'])
    for main in (convert_voice.main, resynthesize_voice.main):
        assert 'add_diff_filter_argument' in inspect.getsource(main)
    for fn in (corpus.convert_batch, corpus.ConvertWave.__init__, convert_voice.convert, convert_voice.convert_synth_batch):
        assert inspect.signature(fn).parameters['diff_filter'].default == 'mlsa'
    assert inspect.signature(k.apply_diff_filter).parameters['method'].default == 'mlsa'
    assert 'apply_diff_filter' in k.__all__
    with pytest.raises(ValueError, match='iir'):
        k.apply_diff_filter(None, None, method='iir')
    with pytest.raises(ValueError, match='iir'):
        corpus.convert_batch([], 16000, None, diff_filter='iir')


def test_apply_diff_filter_mlsa_is_apply_mlsa_filter(monkeypatch):
    import kwiiyatta_amd as k
    import kwiiyatta_amd.filter as flt
    calls = []
    monkeypatch.setattr(flt, 'apply_mlsa_filter', lambda wav, mcep: calls.append((wav, mcep)) or 'mlsa')
    assert k.apply_diff_filter('w', 'm') == 'mlsa' and k.apply_diff_filter('w', 'm', method='mlsa') == 'mlsa'
    assert calls == [('w', 'm')] * 2


def test_apply_diff_filter_fft_shares_the_rate_and_c0_handling(monkeypatch):
    """method='fft': the mel-cepstrum goes through _at_waveform_rate, c0 is zeroed, alpha / hop / transform length are
    the waveform rate's, and the backend gets the waveform as it is"""
    import kwiiyatta_amd as k
    import kwiiyatta_amd.filter as flt
    from kwiiyatta_amd.backend import fftfilt
    fs = 16000
    mcep = k.MelCepstrum(fs, 5.0)
    mcep.data = np.random.default_rng(0).standard_normal((7, 25))
    seen = []
    monkeypatch.setattr(flt, '_at_waveform_rate', lambda m, rate: seen.append(('rate', rate)) or m)

    def backend(x, mc, alpha, hop, size, ignore_c0=True, ctx=None):
        seen.append((x, mc.copy(), alpha, hop, size, ignore_c0))
        return x * 2
    monkeypatch.setattr(fftfilt, 'mcep_fft_filter', backend)
    wav = k.Wavdata(fs, np.arange(100.0))
    out = k.apply_diff_filter(wav, mcep, method='fft')
    assert seen[0] == ('rate', fs)
    x, mc, alpha, hop, size, ignore = seen[1]
    assert x is wav.data and hop == 80 and size == 1024 and ignore is True and alpha == mcep.alpha()
    assert not mc[:, 0].any() and np.array_equal(mc[:, 1:], mcep.data[:, 1:]) and mcep.data[:, 0].any()
    assert out.fs == fs and np.array_equal(out.data, wav.data * 2)


def _Source(fs=16000, frames=20, order=24):
    """what the commands take for an analysed file: a feature set (mel-cepstrum only) with a waveform"""
    import kwiiyatta_amd as k
    f = k.feature(fs)
    mcep = k.MelCepstrum(fs, 5.0)
    mcep.data = np.zeros((frames, order + 1))
    f.mel_cepstrum = mcep
    f.mel_cepstrum_order = order
    f.wavdata = k.Wavdata(fs, np.zeros(frames * 80))
    return f


class _Converter:
    fs, order, gmm, f0_stats, ms_length = 16000, 24, 'gmm', None, None

    def convert(self, mcep, diff=False):
        return copy.copy(mcep)


@pytest.fixture
def filters(monkeypatch):
    import kwiiyatta_amd as k
    calls = []
    monkeypatch.setattr(k, 'apply_mlsa_filter', lambda wav, mcep: calls.append(('mlsa', wav)) or 'by mlsa')
    monkeypatch.setattr(k, 'apply_diff_filter',
                        lambda wav, mcep, method='mlsa': calls.append((method, wav)) or f'by {method}')
    return calls


def test_convert_takes_the_filter(filters, monkeypatch):
    import kwiiyatta_amd.convert_voice as cv
    source = _Source()
    monkeypatch.setattr(cv, 'analyze_source', lambda conf, converter, path: source)
    assert cv.convert(None, _Converter(), 'a.wav', diffvc=True) == 'by mlsa'
    assert cv.convert(None, _Converter(), 'a.wav', diffvc=True, diff_filter='mlsa') == 'by mlsa'
    assert cv.convert(None, _Converter(), 'a.wav', diffvc=True, diff_filter='fft') == 'by fft'
    assert filters == [('mlsa', source), ('mlsa', source), ('fft', source)]


def test_convert_synth_batch_hands_the_filter_to_the_batch_driver(filters, monkeypatch):
    import torch
    import kwiiyatta_amd.convert_voice as cv
    from kwiiyatta_amd import corpus
    source = _Source()
    conf = types.SimpleNamespace(create_analyzer=lambda path, Analyzer=None: source)
    seen = []

    def convert_batch(waves, fs, gmm, **kw):
        seen.append(kw)
        z = [torch.zeros(4, dtype=torch.int16) for _ in waves]
        return z, z, z, z
    monkeypatch.setattr(corpus, 'convert_batch', convert_batch)
    out = cv.convert_synth_batch(conf, _Converter(), ['a.wav', 'b.wav'], diffvc=True, diff_filter='fft')
    assert seen[0]['diff_filter'] == 'fft' and seen[0]['diff'] is True and seen[0]['pcm'] is True
    assert set(out) == {('a.wav', False), ('a.wav', True), ('b.wav', False), ('b.wav', True)}
    cv.convert_synth_batch(conf, _Converter(), ['a.wav'], diffvc=True)
    assert 'diff_filter' not in seen[1]                      # the default: the driver's own, the MLSA filter
    assert filters == []


def test_render_takes_the_filter_on_both_diffvc_paths(filters, monkeypatch):
    import kwiiyatta_amd as k
    import kwiiyatta_amd.resynthesize_voice as rv
    source, carrier = _Source(), _Source()
    monkeypatch.setattr(k, 'align', lambda a, b: a)                      # (equal lengths: the picture is the source's)
    monkeypatch.setattr(k, 'feature', lambda f: f)                       # (no snapshot: it would derive the envelope)

    def conf(**options):
        base = dict(carrier=None, diffvc=True, mcep=False, transpose_key=0.0, result_fs=None, formant_shift=0.0)
        c = types.SimpleNamespace(**{**base, **options})
        c.create_analyzer = lambda path, Analyzer=None: carrier
        return c
    # --carrier --diffvc
    assert rv.render(conf(carrier='c.wav', diff_filter='fft'), source) == 'by fft'
    assert rv.render(conf(carrier='c.wav', diff_filter='mlsa'), source) == 'by mlsa'
    assert rv.render(conf(carrier='c.wav'), source) == 'by mlsa'                  # (no such option on the namespace)
    assert [m for m, _ in filters] == ['fft', 'mlsa', 'mlsa'] and all(w is carrier.wavdata for _, w in filters)
    # --diffvc --formant-shift without a carrier: the source's own waveform by the warp's difference
    del filters[:]
    shifted = []
    monkeypatch.setattr(type(source), 'shift_formants', lambda self, ratio: shifted.append(ratio))
    assert rv.render(conf(formant_shift=2.0, diff_filter='fft'), source) == 'by fft'
    assert rv.render(conf(formant_shift=2.0), source) == 'by mlsa'
    assert filters == [('fft', source.wavdata), ('mlsa', source.wavdata)] and len(shifted) == 2
