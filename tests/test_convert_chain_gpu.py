"""The options of the device conversion driver in combination and across waves, on the MI355X (tests/chain_cases.py
holds the inputs, the table, the numpy composite and its bound):

A  the filter chain of one `corpus.ConvertWave` -- MS, GV, power / emphasis over the plain and the differential rows --
   bit for bit against the single-purpose wrappers applied by hand in the documented order, and against the float64
   composite of the three statements within the bound put together from the single filters' stated bounds;
B  the rendering side with every option on: each intermediate against the single call that the option's own test uses;
C  across waves: the outputs do not depend on how a batch is cut into waves, the status words name global positions,
   an utterance longer than the modulation-spectrum transform is refused before anything is enqueued;
D  `MelCepstrumConverter.convert`, the second implementation of the same chain, against the same composite.

Worst error / bound as printed on an MI355X (the bound: chain_cases.bounds):
    A  ms+gv+power              plain 1.541e-06   differential 1.540e-06
       ms+gv+power, plain only  plain 1.541e-06
       gv+power                 plain 2.444e-04   differential 2.387e-04
    D  arg-max                  plain 2.272e-08   differential 2.272e-08
       em=1                     plain 2.629e-08   differential 2.629e-08
(the bounds are the stated ones carried through three filters, worst case on worst case: the kernels sit far inside)"""
from types import SimpleNamespace

import numpy as np
import pytest

import chain_cases as ch
import power_cases as pc

pytestmark = pytest.mark.gpu

FS, ORDER = ch.FS, ch.ORDER
RATIO = 2.0 ** (3 / 12)
F0_STATS = (float(np.log(150.0)), 0.2, float(np.log(200.0)), 0.25)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _up(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope='module')
def shared():
    """one lockstep pair of streams, the mixtures, the three utterances, the plain wave of the table and the statistics
    made from its converted rows; `waves`: the table's runs, made once each"""
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd.backend import bap
    ls = corpus._Lockstep(0)
    mix = ch.mixture()
    band = ch.band_mixture(bap.check_rate(FS))
    s = SimpleNamespace(ls=ls, mix=mix, band=band, triples=ch.utterances(), waves={}, plain={},
                        dg=corpus.DeviceGMM(mix.weights_, mix.means_, mix.covariances_, ls.dev),
                        band_dg=corpus.DeviceGMM(band.weights_, band.means_, band.covariances_, ls.dev))
    base = _run(s, s.triples, diff=True)
    s.plain[()] = base
    s.rows = corpus.Ragged(base.T)
    assert tuple(base.T) == ch.FRAMES and base.fft == ch.FFT
    s.stats = ch.statistics([v.cpu().numpy() for v in s.rows.views(base.mc_conv)])
    s.dev_stats = SimpleNamespace(G=_up(s.stats.ms[0], ls.dev), N=_up(s.stats.ms[1], ls.dev), gv=_up(s.stats.gv, ls.dev))
    return s


def _run(s, utterances, **options):
    from kwiiyatta_amd import corpus
    wave = corpus.ConvertWave(s.ls, FS, utterances, gmm=s.dg, order=ORDER, frame_period=ch.FRAME_PERIOD, **options)
    wave.run()
    s.ls.sync()
    return wave


def _conversion(s, conv):
    """the keywords of the conversion's own options (the GV ascent takes the statistics too)"""
    return dict(conv, gv_stats=s.stats.gv, gv_var=s.stats.gv_var) if 'mlpg_gv' in conv else dict(conv)


def _plain(s, conv):
    key = tuple(sorted(conv.items()))
    if key not in s.plain:
        s.plain[key] = _run(s, s.triples, diff=True, **_conversion(s, conv))
    return s.plain[key]


def _entry(s, name):
    if name not in s.waves:
        filters, diff, conv = ch.TABLE[name]
        s.waves[name] = _run(s, s.triples, diff=diff, **ch.options(s.stats, **filters), **_conversion(s, conv))
    return s.waves[name]


def _by_hand(s, plain, filters, diff):
    """the chain on clones of the plain wave's rows through the single-purpose wrappers: (plain rows, differential rows)
    as whole blocks"""
    import torch
    from kwiiyatta_amd.backend import gv, ms, power
    ls, rows, d = s.ls, s.rows, s.dev_stats
    n = len(rows)
    with torch.cuda.stream(ls.main):
        p_all, b_all = plain.mc_conv.clone(), plain.mc_diff.clone()
        p, b, src = rows.views(p_all), rows.views(b_all), rows.views(plain.mc)
        if filters.get('ms'):
            if diff:
                ms.postfilter_batch_dev(ls.ctx, p, d.G, d.N, ch.MS_STRENGTH, b, bases=b)
            ms.postfilter_batch_dev(ls.ctx, p, d.G, d.N, ch.MS_STRENGTH, p)
        if filters.get('gv'):
            moments = torch.empty((n, ORDER + 1, 3), dtype=torch.float64, device=ls.dev)
            gv.column_moments_batch_dev(ls.ctx, p, moments)               # of the rows MS has filtered
            if diff:
                gv.postfilter_batch_dev(ls.ctx, p, moments, d.gv, ch.GV_STRENGTH, b, bases=b)
            gv.postfilter_batch_dev(ls.ctx, p, moments, d.gv, ch.GV_STRENGTH, p)
        beta, keep = filters.get('beta', 0.0), filters.get('keep_power', False)
        if beta or keep:
            refs = src if keep else None
            power.postfilter_batch_dev(ls.ctx, p, p, plain.alpha, plain.fft, beta, refs=refs)
            if diff:
                b_all[:, 0] = 0.0
                absolute = rows.views(plain.mc + b_all)
                power.postfilter_batch_dev(ls.ctx, absolute, b, plain.alpha, plain.fft, beta, refs=refs, bases=b)
    ls.sync()
    return p_all, b_all


# ---- A: the filter chain inside one wave -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ch.TABLE))
def test_the_chain_of_a_wave_by_value(shared, name):
    s = shared
    filters, diff, conv = ch.TABLE[name]
    plain, wave = _plain(s, conv), _entry(s, name)
    n, power_on = len(s.rows), bool(filters.get('beta') or filters.get('keep_power'))
    # the status words: exactly the kinds switched on, two words per utterance where there are two conversions; all 0
    expected = {kind: 1 for kind in ('ms', 'gv') if filters.get(kind)}
    if power_on:
        expected['power'] = 2 if diff else 1
    if 'mlpg_gv' in conv:
        expected['gvgen'] = 2
    assert {kind: per for kind, _, per in wave.status_words()} == expected
    for kind, words, per in wave.status_words():
        assert words.cpu().tolist() == [0] * (per * n), kind
    assert wave.ignore_c0 == (0 if power_on else 1)
    assert _bytes(wave.mc) == _bytes(plain.mc)
    if not diff:
        # the plain rows and the waveforms do not know of the differential conversion
        other = _entry(s, ch.PLAIN_ONLY_OF[name])
        assert wave.mc_diff is None
        assert _bytes(wave.mc_conv) == _bytes(other.mc_conv) and _bytes(wave.wave_all) == _bytes(other.wave_all)
    # 1. bit for bit against the chain made by hand
    want_p, want_b = _by_hand(s, plain, filters, diff)
    assert _bytes(wave.mc_conv) == _bytes(want_p)
    if diff:
        assert _bytes(wave.mc_diff) == _bytes(want_b)
        if not (filters.get('ms') or filters.get('gv')):
            # no early filter: the differential conversion ran after the rendering, and is the plain wave's
            if not power_on:
                assert _bytes(wave.mc_diff) == _bytes(plain.mc_diff)
            elif not filters.get('beta'):
                assert _bytes(wave.mc_diff[:, 1:]) == _bytes(plain.mc_diff[:, 1:] + 0.0)
    if filters:
        assert _bytes(wave.mc_conv) != _bytes(plain.mc_conv)
    # 2. against the float64 composite, and the energy it promises
    views = lambda t: [v.cpu().numpy() for v in s.rows.views(t)]  # noqa: E731
    src, x, b = views(plain.mc), views(plain.mc_conv), views(plain.mc_diff)
    got_p, got_b = views(wave.mc_conv), views(wave.mc_diff) if diff else [None] * n
    if name in ch.NUMERIC:
        worst = [0.0, 0.0]
        for i in range(n):
            base = b[i] if diff else None
            want = ch.composite(src[i], x[i], base, s.stats, plain.alpha, **filters)
            bound = ch.bounds(src[i], x[i], base, s.stats, **filters)
            for q, got in enumerate((got_p[i], got_b[i])):
                if got is not None:
                    worst[q] = max(worst[q], (np.abs(got - want[q]).max(axis=0) / bound[q]).max())
        print(f'{name}: worst error / bound: plain {worst[0]:.3e}, differential {worst[1]:.3e}')
        assert 0 < worst[0] <= 1 and worst[1] <= 1 and (worst[1] > 0) == diff
        if name == 'ms+gv+power':
            # the rows these inputs give tell the documented order from its near misses, as the host rows do
            for variant in ch.MUTANTS:
                off = max((np.abs(got_b[i] - ch.composite(src[i], x[i], b[i], s.stats, plain.alpha, variant=variant,
                                                          **filters)[1]).max(axis=0)
                           / ch.bounds(src[i], x[i], b[i], s.stats, **filters)[1]).max() for i in range(n))
                print(f'{name}: the wave against the composite with {variant}: {off:.3e} bounds')
                assert off >= 1e3, variant
    if filters.get('keep_power'):
        for i in range(n):
            e = pc.energy(src[i], plain.alpha, ch.FFT)
            assert np.abs(pc.energy(got_p[i], plain.alpha, ch.FFT) / e - 1).max() <= 2 * ch.KERNEL_BOUND, i
            if diff:
                assert np.abs(pc.energy(src[i] + got_b[i], plain.alpha, ch.FFT) / e - 1).max() <= 2 * ch.KERNEL_BOUND, i


# ---- B: the rendering side with everything on --------------------------------------------------------------------------
def _everything(s, **over):
    return dict(dict(ch.options(s.stats, ms=True, gv=True, **ch.BOTH), mlpg_em=1, f0_stats=F0_STATS, transpose_key=-2.0,
                     formant_ratio=RATIO), **over)


@pytest.mark.parametrize('estimator', ('dio', 'pyin'))
def test_the_rendering_side_with_everything_on(shared, estimator):
    import kwiiyatta_amd as k
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._blocks import Ragged
    from kwiiyatta_amd.backend import bap, f0 as f0map, formant, sptk, world
    import convert_cases as cc
    s = shared
    waves_in = [np.ascontiguousarray(u[0]) for u in s.triples]
    common = dict(pcm=True, diff=True, f0_estimator=estimator)
    wave = _run(s, waves_in, ap_gmm=s.band_dg, **common, **_everything(s))
    fft = _run(s, waves_in, ap_gmm=s.band_dg, **common, **_everything(s, diff_filter='fft'))
    rest = _run(s, waves_in, **common, **_everything(s, f0_stats=None, transpose_key=0.0, formant_ratio=1.0))
    n = wave.n
    for kind, words, per in wave.status_words():
        assert words.cpu().tolist() == [0] * words.numel(), kind
    assert [kind for kind, _, _ in wave.status_words()] == [estimator, 'f0_map', 'formant', 'ms', 'gv', 'power']
    rows = Ragged(wave.T)
    views = lambda t: [v.cpu().numpy() for v in rows.views(t)]  # noqa: E731
    # the band mixture's prepared model, for the aperiodicity the rendering read
    ctx = _lib.default_context()
    B = bap.check_rate(FS)
    rc, model = cc.prepare(ctx, B, s.band.weights_, s.band.means_, s.band.covariances_)
    assert rc == _lib.KWY_OK
    analysed = views(rest.ap_all)
    tracks = bap.track(analysed, FS)
    mapped = cc.convert_mcep(ctx, model, len(s.band.weights_), [np.ascontiguousarray(t) for t in tracks])
    sp_want = formant.shift_formants(sptk.mc2sp(wave.mc_conv.cpu().numpy(), wave.alpha, wave.fft), RATIO)
    assert _bytes(wave.sp_conv) == sp_want.tobytes()
    sp, ap, mc_diff = views(wave.sp_conv), views(wave.ap_all), views(wave.mc_diff)
    compared, mapped_tracks = set(), 0
    for i, x in enumerate(waves_in):
        wav = k.Wavdata(FS, x.copy())
        f0 = wave.f0[i].cpu().numpy()
        assert np.array_equal(f0, k.Analyzer(wav, f0_estimator=estimator).f0), i
        f0_synth = wave.f0_synth[i].cpu().numpy()
        assert np.array_equal(f0_synth, f0map.map_f0(f0, FS, stats=F0_STATS, key=-2.0)), i
        # (an estimator may find no voiced frame in so short an utterance: the map leaves such a track as it is)
        assert np.array_equal(f0_synth, f0) == (not (f0 > 0).any()), i
        mapped_tracks += int((f0 > 0).any())
        converted = np.ascontiguousarray(np.hstack((tracks[i][:, :1], bap.clamp(mapped[i][:, 1:]))))
        want_ap = bap.apply(tracks[i], converted, analysed[i].copy(), FS)
        assert np.array_equal(ap[i], want_ap), i
        assert np.array_equal(ap[i], analysed[i]) == (not (tracks[i][:, 0] == 1.0).any()), i
        y = wave.wave[i].cpu().numpy()
        # (the wave's envelopes are CheapTrick's over fs, and its rendering multiplies them back)
        want_y = world.synthesize(f0_synth, sp[i], ap[i], FS, ch.FRAME_PERIOD, sp_mul=float(FS))
        assert y.shape == want_y.shape and np.array_equal(y, want_y), i
        out = k.Wavdata(FS, y.copy())
        k.Synthesizer.finish(out, len(f0))
        assert np.array_equal(wave.pcm[i].cpu().numpy(), out._pcm16(True, {})), i
        # the differential outputs: the input through the filter of the wave's own differential rows, c0 in play
        rec = k.MelCepstrum(FS, ch.FRAME_PERIOD, mc_diff[i])
        for run, method in ((wave, 'mlsa'), (fft, 'fft')):
            got = run.wave_diff[i].cpu().numpy()
            ref = k.apply_mlsa_filter(wav, rec, use_c0=True) if method == 'mlsa' else \
                k.apply_diff_filter(wav, rec, method='fft', use_c0=True)
            assert got.shape == ref.data.shape
            # (the table's mixture has random means, far from any speech: the differential filter of the 0.4 s
            # utterance overflows, in the wave and in the single call alike.  Where the single call's output is not
            # finite only that is compared; every method is held to the bound on at least one utterance)
            finite = np.isfinite(ref.data)
            assert np.array_equal(np.isfinite(got), finite), (i, method)
            if not finite.all():
                continue
            compared.add(method)
            assert np.abs(got - ref.data).max() <= 1e-12 * max(1.0, np.abs(ref.data).max()), (i, method)
            assert np.array_equal(run.pcm_diff[i].cpu().numpy(), k.Wavdata(FS, got.copy())._pcm16(True, {})), (i, method)
    print(f'{estimator}: voiced frames per utterance {[int((wave.f0[i] > 0).sum()) for i in range(n)]}')
    assert compared == {'mlsa', 'fft'} and mapped_tracks >= 1
    # the differential outputs do not move with the rendering's options, the synthesised ones not with the filter
    assert _bytes(fft.mc_diff) == _bytes(wave.mc_diff) == _bytes(rest.mc_diff)
    assert _bytes(rest.wave_diff_all) == _bytes(wave.wave_diff_all) and _bytes(rest.pcm_diff_all) == _bytes(wave.pcm_diff_all)
    assert _bytes(fft.wave_all) == _bytes(wave.wave_all) and _bytes(fft.pcm_all) == _bytes(wave.pcm_all)
    assert _bytes(fft.wave_diff_all) != _bytes(wave.wave_diff_all) and _bytes(rest.wave_all) != _bytes(wave.wave_all)


# ---- C: across waves ---------------------------------------------------------------------------------------------------
def _batch(s, utterances, wave_size, options, **driver):
    """`corpus._lockstep_batch` with the table's mixture: the four outputs of every utterance as bytes"""
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd._convert_options import ConvertOptions
    out = [None] * len(utterances)

    def keep(i, *views):
        out[i] = views
    corpus._lockstep_batch(utterances, FS, 0, s.dg, ORDER, ch.FRAME_PERIOD, s.ls, keep,
                           ConvertOptions(**options).check(ORDER), wave_size=wave_size, **driver)
    return [tuple(None if v is None else _bytes(v) for v in views) for views in out]


def _five(s):
    return [np.ascontiguousarray(u[0]) for u in ch.utterances(5, seed=80)]


@pytest.mark.parametrize('diff_filter', ('mlsa', 'fft'))
def test_the_outputs_do_not_depend_on_the_waves(shared, diff_filter):
    """five utterances, all options on, in waves of 1, 2 and 16: with 2 a wave leaves `held` while the deferred MLSA
    records of all three wait for the last one"""
    s = shared
    driver = dict(pcm=True, diff=True, ap_gmm=s.band_dg)
    options = _everything(s, diff_filter=diff_filter)
    by_size = {size: _batch(s, _five(s), size, options, **driver) for size in (1, 2, 16)}
    assert all(len(v) == 4 and None not in v for v in by_size[16])
    assert by_size[1] == by_size[16] and by_size[2] == by_size[16]
    two = _five(s)[:2]
    assert _batch(s, two, 2, options, **driver) == _batch(s, two, 2, options, **driver) == by_size[16][:2]


def test_the_default_waves_of_a_batch_of_seventeen(shared):
    from kwiiyatta_amd import corpus
    s = shared
    waves_in = [np.ascontiguousarray(u[0]) for u in ch.utterances(17, seconds=(0.25,), seed=100)]
    options = _everything(s, diff_filter='mlsa')
    res = corpus.convert_batch(waves_in, FS, s.mix, order=ORDER, frame_period=ch.FRAME_PERIOD, pcm=True, diff=True,
                               ap_gmm=s.band, **options)
    one_by_one = _batch(s, waves_in, 1, options, pcm=True, diff=True, ap_gmm=s.band_dg)
    assert len(one_by_one) == 17
    for i in range(17):
        assert tuple(_bytes(part[i]) for part in res) == one_by_one[i], i


def test_a_bad_f0_track_is_named_by_its_global_position(shared):
    s = shared
    triples = ch.utterances(5, seed=80)
    x, f0, t = triples[3]
    triples[3] = (x, np.full_like(f0, 1500.0), t)                # an octave up: 3000 Hz >= fs/8
    with pytest.raises(ValueError, match=rf'f0 map: {len(f0)} frame\(s\) of track\(s\) \[3\] are'):
        _batch(s, triples, 2, dict(transpose_key=12.0))


def test_an_unusable_formant_row_is_named_by_its_wave(shared, monkeypatch):
    """one value of one envelope row of the SECOND wave is zeroed right before that wave's formant shift and put back
    right after it (on the wave's stream): the kernel copies the row as it is and counts it"""
    from kwiiyatta_amd import corpus
    s = shared
    built, waves, real = corpus.ConvertWave.__init__, [], corpus.lib

    def init(self, *args, **kwargs):
        built(self, *args, **kwargs)
        waves.append(self)

    class Spoiling:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != 'kwy_formant_shift_dev':
                return fn

            def call(*args):
                if len(waves) != 2:
                    return fn(*args)
                rendered = waves[-1].sp_conv
                saved = rendered[3, 7].clone()
                rendered[3, 7] = 0.0
                rc = fn(*args)
                rendered[3, 7] = saved
                return rc
            return call
    monkeypatch.setattr(corpus.ConvertWave, '__init__', init)
    monkeypatch.setattr(corpus, 'lib', Spoiling())
    with pytest.raises(ValueError, match=r'formant shift: 1 row\(s\) of wave\(s\) \[1\] were'):
        _batch(s, ch.utterances(5, seed=80), 2, dict(formant_ratio=RATIO))
    assert len(waves) == 3


@pytest.mark.parametrize('bare', (False, True), ids=('triples', 'waveforms'))
def test_an_utterance_longer_than_ms_length_in_a_later_wave(shared, monkeypatch, bare):
    """`ConvertOptions`: an utterance of more than ms_length frames is a ValueError BEFORE the batch.  `_MsFilter` checks
    wave by wave, so without the check of `_lockstep_batch` the two waves in front of the long utterance have run when it
    fires (on an MI355X, before that check: the ValueError with 18 calls enqueued).  The per-wave check stays."""
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd.synthetic import make_utterance
    from test_convert_trace_gpu import _Recorder
    s = shared
    long = make_utterance(seed=90, fs=FS, seconds=2.6)
    frames = len(long[1])
    assert frames > ch.MS_LENGTH and int(corpus.lib.kwy_dio_frames(FS, len(long[0]), ch.FRAME_PERIOD)) == frames
    utterances = s.triples[:2] + [long]
    if bare:
        utterances = [np.ascontiguousarray(u[0]) for u in utterances]
    options = ch.options(s.stats, ms=True)
    calls = []
    with monkeypatch.context() as m:
        m.setattr(corpus, 'lib', _Recorder(corpus.lib, s.ls, calls))
        with pytest.raises(ValueError, match=rf'T = {frames} frames is longer than the transform length L = 512'):
            _batch(s, utterances, 1, options, diff=True)
    s.ls.sync()
    assert calls == []
    with pytest.raises(ValueError, match=rf'T = {frames} frames'):
        corpus.ConvertWave(s.ls, FS, [long], gmm=s.dg, order=ORDER, **options)
    assert len(_batch(s, utterances[:2], 1, options, diff=True)) == 2


# ---- D: the per-file path on the same table ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """a converter of 2 components trained on four synthetic parallel pairs of about a second (16 kHz: every utterance
    fits the shortest transform) with global-variance and modulation-spectrum statistics at length 512"""
    import kwiiyatta_amd as k
    from kwiiyatta_amd.synthetic import make_utterance
    root = tmp_path_factory.mktemp('chain')
    for side, warp, scale, base in (('src', 1.0, 1.0, 140.0), ('tgt', 1.1, 1.12, 190.0)):
        (root / side).mkdir()
        for i in range(4):
            x = make_utterance(seed=500 + i, fs=FS, seconds=0.9 + 0.1 * i, time_warp=warp, formant_scale=scale,
                               f0_base=base)[0]
            k.Wavdata(FS, x.copy()).save(root / side / f'u{i}.wav')
    dataset = k.align(k.WavFileDataset(root / 'src'), k.WavFileDataset(root / 'tgt'))
    conv = k.MelCepstrumConverter(use_delta=True, components=2, random_state=0)
    np.random.seed(0)
    conv.train(dataset, sorted(dataset.keys()), gv_stats=True, ms_stats=True, ms_length=ch.MS_LENGTH)
    return root, conv


@pytest.mark.parametrize('em', (None, 1), ids=('arg-max', 'em=1'))
def test_the_converter_composes_the_same_chain(trained, em):
    import kwiiyatta_amd as k
    root, conv = trained
    assert conv.ms_length == ch.MS_LENGTH and conv.fs == FS and conv.order == ORDER
    stats = SimpleNamespace(ms=conv.ms_stats, gv=conv.gv_stats)
    filters = ch.TABLE['ms+gv+power'][0]
    options = dict(ms=ch.MS_STRENGTH, gv=ch.GV_STRENGTH, postfilter=ch.BETA, keep_power=True)
    how = {} if em is None else dict(em=em)
    mcep_in = k.analyze_wav(root / 'src' / 'u1.wav').mel_cepstrum
    src = np.ascontiguousarray(mcep_in.data)
    alpha = mcep_in.alpha()
    x = np.ascontiguousarray(conv.convert(mcep_in, **how).data)
    b = np.ascontiguousarray(conv.convert(mcep_in, diff=True, **how).data)
    assert x[:, 0].tobytes() == src[:, 0].tobytes() and 2 <= len(src) <= ch.MS_LENGTH
    want = ch.composite(src, x, b, stats, alpha, **filters)
    bound = ch.bounds(src, x, b, stats, **filters)
    e = pc.energy(src, alpha, ch.FFT)
    worst = []
    for q, diff in enumerate((False, True)):
        got = conv.convert(mcep_in, diff=diff, **options, **how).data
        assert got.tobytes() != (b if diff else x).tobytes()
        worst.append((np.abs(got - want[q]).max(axis=0) / bound[q]).max())
        kept = pc.energy(src + got if diff else got, alpha, ch.FFT)
        assert np.abs(kept / e - 1).max() <= 2 * ch.KERNEL_BOUND, diff
    print(f'convert(), em={em}: worst error / bound: plain {worst[0]:.3e}, differential {worst[1]:.3e}')
    assert 0 < worst[0] <= 1 and 0 < worst[1] <= 1
