"""Formant shift, host side (no GPU): the claims of its numpy statement (tests/formant_cases.py), the --formant-shift
option and its checks in both command-line tools, the drivers' refusal on the stream driver, and -- with
backend.formant.shift_formants replaced by the numpy statement and the other numerics served by the CPU oracle -- the
wiring of Feature.shift_formants and of kwiieiya's render()."""
import argparse
import copy
import sys
import types

import numpy as np
import pytest

import formant_cases as fc
from conftest import CLB_WAV, _install_oracle_backend


def _run_cli(main, argv):
    old = sys.argv
    sys.argv = ['prog'] + argv
    try:
        main()
    finally:
        sys.argv = old


def _parser_error(main, argv, capsys):
    with pytest.raises(SystemExit) as e:
        _run_cli(main, argv)
    assert e.value.code == 2
    return capsys.readouterr().err


# ---- the numpy statement's own claims -------------------------------------------------------------------------------
def _matrices(seed):
    rng = np.random.RandomState(seed)
    for K in fc.WIDTHS:
        for rows in fc.ROWS:
            yield fc.envelope(rng, rows, K)


def test_ratio_one_returns_the_input_bit_for_bit():
    for sp in _matrices(0):
        if len(sp):
            sp[0, 0] = np.nan                            # nothing is examined
        out, status = fc.shift(sp, 1.0)
        assert status == 0 and out.tobytes() == sp.tobytes() and out is not sp


def test_half_and_double_are_exact_decimation_and_spreading():
    for sp in _matrices(1):
        K = sp.shape[1]
        down, status = fc.shift(sp, 0.5)
        assert status == 0
        n = (K - 1) // 2 + 1                             # the bins with 2 k <= K - 1
        assert down[:, :n].tobytes() == sp[:, 0:2 * n:2].tobytes()
        assert np.array_equal(down[:, n:], np.repeat(sp[:, K - 1:], K - n, axis=1))
        up, status = fc.shift(sp, 2.0)
        assert status == 0
        assert up[:, 0::2].tobytes() == sp[:, :(K + 1) // 2].tobytes()


def test_taps_depend_on_bin_and_ratio_and_stay_inside_the_row():
    for K in fc.WIDTHS:
        for ratio in fc.RATIOS + (0.5000001, 1.9999999):
            j, a, copied = fc.taps(K, ratio)
            assert j[0] == 0 and copied[0]
            assert np.all((0 <= j) & (j <= K - 1)) and np.all((0 <= a) & (a < 1))
            assert np.all(copied[j == K - 1])            # the upper tap j + 1 is never read beyond the row
            assert np.all(np.diff(j) >= 0)


def test_a_bump_moves_by_the_ratio():
    worst, count = 0.0, 0
    for K, semitones, centre in fc.bump_cases():
        ratio = 2.0 ** (semitones / 12)
        out, status = fc.shift(fc.bump(K, centre, max(2.0, 0.02 * (K - 1))), ratio)
        err = abs(float(np.argmax(out[0])) - centre * ratio)
        worst, count = max(worst, err), count + 1
        assert status == 0 and err <= 1.0, (K, semitones, centre, err)
    print(f'bump maximum: worst distance from centre * ratio = {worst:.3f} bins over {count} cases')
    assert count >= 80


def test_outputs_stay_within_the_rows_range():
    worst = 0.0
    for sp in _matrices(2):
        if not len(sp):
            continue
        lo, hi, slack = sp.min(axis=1)[:, None], sp.max(axis=1)[:, None], fc.range_slack(sp)[:, None]
        for ratio in fc.RATIOS:
            out, _ = fc.shift(sp, ratio)
            over = np.maximum(out / hi - 1, 1 - out / lo)
            worst = max(worst, float((over / slack).max()))
            assert np.all(over <= slack), (sp.shape, ratio)
    print(f'range claim: worst excess / slack = {worst:.3f}')


def test_a_constant_row_comes_back_within_4_ulp():
    # exp(log x): a logarithm within 1 ulp is off by at most |log x| EPS, which exp turns into that relative error, plus
    # its own ulp: (|log x| + 1) EPS <= 4 EPS for |log x| <= 3
    worst = 0.0
    for value in (0.05, 0.3, 1.0, 7.5, 20.0):
        assert abs(np.log(value)) <= 3
        for K in fc.WIDTHS:
            sp = np.full((3, K), value)
            for ratio in fc.RATIOS:
                out, status = fc.shift(sp, ratio)
                err = float(np.abs(out / value - 1).max())
                worst = max(worst, err)
                assert status == 0 and err <= 4 * fc.EPS, (value, K, ratio, err)
    print(f'constant rows: worst relative deviation = {worst:.3e}')


def test_unusable_rows_are_copied_and_counted():
    rng = np.random.RandomState(3)
    for K in (2, 65, 1025):
        sp = fc.envelope(rng, 67, K)
        clean = sp.copy()
        rows = fc.plant(sp, rng, 9)
        for ratio in (0.5, 2.0 ** (1 / 12), 2.0):
            out, status = fc.shift(sp, ratio)
            want, _ = fc.shift(clean, ratio)
            assert status == 9
            for r in range(67):
                assert out[r].tobytes() == (sp if r in rows else want)[r].tobytes(), (K, ratio, r)


@pytest.mark.parametrize('ratio', [0.49, 2.01, np.nan, np.inf, -1.0])
def test_the_statement_refuses_ratios_out_of_range(ratio):
    with pytest.raises(ValueError):
        fc.shift(np.ones((2, 5)), ratio)


# ---- options ---------------------------------------------------------------------------------------------------------
def test_formant_shift_option_parses_and_checks_range():
    import kwiiyatta_amd as k
    for text, value in (('-5', -5.0), ('12', 12.0), ('-12', -12.0), ('0.5', 0.5), ('0', 0.0)):
        conf = k.Config(argparse.ArgumentParser())
        conf.add_formant_shift_argument()
        conf.parser.parse_args(['--formant-shift', text], namespace=conf)
        assert conf.formant_shift == value
        assert conf.formant_ratio == 2.0 ** (value / 12)
    conf = k.Config(argparse.ArgumentParser())
    conf.add_formant_shift_argument()
    conf.parser.parse_args([], namespace=conf)
    assert conf.formant_shift == 0.0 and conf.formant_ratio == 1.0
    assert 2.0 ** (12 / 12) == 2.0 and 2.0 ** (-12 / 12) == 0.5          # the ends of the range are the kernel's


@pytest.mark.parametrize('value', ['12.01', '-12.5', '100', 'nan', 'inf', 'up'])
def test_formant_shift_out_of_range_is_a_parser_error(value, capsys):
    import kwiiyatta_amd.convert_voice as cv
    import kwiiyatta_amd.resynthesize_voice as rv
    assert '--formant-shift' in _parser_error(rv.main, [CLB_WAV, '--formant-shift', value], capsys)
    assert '--formant-shift' in _parser_error(cv.main, ['--formant-shift', value, CLB_WAV], capsys)


def test_check_ratio():
    from kwiiyatta_amd.backend import formant
    for ratio in (0.5, 1, 1.25, 2.0, np.float64(0.75)):
        assert formant.check_ratio(ratio) == float(ratio)
    for ratio in (0.49, 2.01, np.nan, np.inf, -np.inf, 0, 'fast', None):
        with pytest.raises(ValueError, match='formant shift'):
            formant.check_ratio(ratio)
    assert formant.MAX_K == fc.MAX_K and formant.RATIO_RANGE == fc.RATIO_RANGE
    with pytest.raises(ValueError, match=r'2 row\(s\) of matrix / matrices \[1\]'):
        formant.check_status(np.array([0, 2, 0], dtype=np.int32))
    formant.check_status(np.zeros(3, dtype=np.int32))


def test_stream_drivers_refuse_a_ratio():
    from kwiiyatta_amd import corpus
    for ratio in (1.2, 0.5):
        with pytest.raises(ValueError, match='formant_ratio needs the lockstep driver'):
            corpus.convert_batch([], 16000, None, driver='streams', formant_ratio=ratio)
        with pytest.raises(ValueError, match='formant_ratio needs the lockstep driver'):
            corpus.resynthesize_batch([], 16000, driver='streams', formant_ratio=ratio)
        with pytest.raises(ValueError, match='formant_ratio needs the lockstep driver'):
            corpus.resynthesize_batch([], 16000, pool=object(), formant_ratio=ratio)
    for ratio in (2.5, np.nan):                                              # (whatever the driver)
        with pytest.raises(ValueError, match='outside'):
            corpus.convert_batch([], 16000, None, formant_ratio=ratio)
        with pytest.raises(ValueError, match='outside'):
            corpus.resynthesize_batch([], 16000, driver='streams', formant_ratio=ratio)


# ---- wiring: the numpy statement in place of the kernel, the CPU oracle for the rest --------------------------------
FS, FRAMES, BINS = 16000, 12, 513


@pytest.fixture
def statement(monkeypatch):
    """backend.formant.shift_formants served by tests/formant_cases.shift; the calls it got as (shape, ratio)"""
    from kwiiyatta_amd.backend import formant
    _install_oracle_backend(monkeypatch)
    calls = []

    def shift_formants(sp, ratio, ctx=None):
        calls.append((np.shape(sp), ratio))
        out, status = fc.shift(sp, ratio)
        assert status == 0
        return out
    monkeypatch.setattr(formant, 'shift_formants', shift_formants)
    return calls


def _envelope(seed=0):
    rng = np.random.RandomState(seed)
    k = np.arange(BINS)
    rows = [np.exp(-9 + 5 * np.exp(-0.5 * ((k - c) / 18.0) ** 2) + 3 * np.exp(-0.5 * ((k - 3.1 * c) / 30.0) ** 2))
            for c in rng.uniform(40, 90, size=FRAMES)]
    return np.ascontiguousarray(rows)


def _feature(seed=0):
    import kwiiyatta_amd as k
    f = k.feature(FS)
    f.f0 = np.full(FRAMES, 120.0 + seed)
    f.spectrum_envelope = _envelope(seed)
    f.aperiodicity = np.full((FRAMES, BINS), 0.25)
    return f


def _mcep_of(sp):
    import kwiiyatta_amd as k
    f = k.feature(FS)
    f.spectrum_envelope = np.ascontiguousarray(sp)
    return f.mel_cepstrum.data


def test_feature_shift_formants_warps_the_envelope_and_rederives_the_mel_cepstrum(statement):
    import kwiiyatta_amd as k
    f = _feature()
    sp, f0, ap = f.spectrum_envelope, f.f0, f.aperiodicity
    before = f.mel_cepstrum.data.copy()
    ratio = 2.0 ** (3 / 12)
    assert f.shift_formants(ratio) is None
    assert statement == [((FRAMES, BINS), ratio)]
    want, _ = fc.shift(sp, ratio)
    assert f.spectrum_envelope.tobytes() == want.tobytes()
    assert f._mel_cepstrum.data is None                                  # cleared: derived again on demand
    assert f.mel_cepstrum.data.tobytes() == _mcep_of(want).tobytes()
    assert np.abs(f.mel_cepstrum.data - before).max() > 1e-3
    assert f.f0 is f0 and f.aperiodicity is ap
    # ratio 1: nothing happens, not even the call
    g = _feature()
    g.mel_cepstrum                                                        # noqa: B018 (fills the slot)
    held = g._mel_cepstrum.data
    g.shift_formants(1.0)
    assert len(statement) == 1 and g._mel_cepstrum.data is held and g.spectrum_envelope.tobytes() == sp.tobytes()
    for bad in (0.4, 2.5, np.nan):
        with pytest.raises(ValueError, match='formant shift'):
            g.shift_formants(bad)
    # the package-level form: a warped copy, the input untouched
    h = k.shift_formants(g, ratio)
    assert h is not g and h.spectrum_envelope.tobytes() == want.tobytes()
    assert g.spectrum_envelope.tobytes() == sp.tobytes() and g._mel_cepstrum.data is held
    assert h.f0 is g.f0 and h.aperiodicity is g.aperiodicity
    assert 'shift_formants' in k.__all__


def test_feature_shift_formants_on_a_mel_cepstrum_only(statement):
    import kwiiyatta_amd as k
    mc = _feature().mel_cepstrum.data.copy()
    f = k.feature(FS)
    f.f0 = np.full(FRAMES, 150.0)
    f.aperiodicity = np.full((FRAMES, BINS), 0.25)
    f.mel_cepstrum = mc
    assert f._spectrum_envelope is None
    implied = f.spectrum_envelope
    assert implied.shape == (FRAMES, BINS)
    ratio = 2.0 ** (-4 / 12)
    f.shift_formants(ratio)
    want, _ = fc.shift(np.ascontiguousarray(implied), ratio)
    assert statement == [((FRAMES, BINS), ratio)]
    assert f._spectrum_envelope.tobytes() == want.tobytes() and f._mel_cepstrum.data is None
    assert f.mel_cepstrum.data.tobytes() == _mcep_of(want).tobytes()
    empty = k.feature(FS)
    with pytest.raises(ValueError, match='neither'):
        empty.shift_formants(ratio)


class _Source:
    """what render() takes for an analysed file: a feature set with a waveform"""

    def __new__(cls, seed):
        import kwiiyatta_amd as k
        f = _feature(seed)
        f.wavdata = k.Wavdata(FS, np.random.RandomState(seed).standard_normal(FS * FRAMES * 5 // 1000) * 0.1)
        return f


def _conf(**options):
    base = dict(carrier=None, diffvc=False, mcep=False, transpose_key=0.0, result_fs=None)
    return types.SimpleNamespace(**{**base, **options})


def test_render_at_shift_zero_is_todays_render(statement, monkeypatch):
    import kwiiyatta_amd as k
    import kwiiyatta_amd.resynthesize_voice as rv
    filtered = []
    monkeypatch.setattr(k, 'apply_mlsa_filter', lambda wav, mcep: filtered.append((wav, mcep)))
    source = _Source(1)
    today = rv.render(_conf(), source)                                   # (no such option on the namespace at all)
    for options in (dict(formant_shift=0.0), dict(formant_shift=0.0, diffvc=True), dict(formant_shift=0.0, mcep=True)):
        got = rv.render(_conf(**options), source)
        if not options.get('mcep'):
            assert got.data.tobytes() == today.data.tobytes()
    assert statement == [] and filtered == []
    shifted = rv.render(_conf(formant_shift=3.0), source)
    assert statement == [((FRAMES, BINS), 2.0 ** (3 / 12))] and filtered == []
    assert shifted.data.shape == today.data.shape and shifted.data.tobytes() != today.data.tobytes()
    # --mcep: the envelope implied by the mel-cepstrum is what gets warped
    rv.render(_conf(formant_shift=-2.0, mcep=True), source)
    assert statement[1:] == [((FRAMES, BINS), 2.0 ** (-2 / 12))]
    assert source.spectrum_envelope.tobytes() == _envelope(1).tobytes()     # the source is never changed


def test_render_diffvc_without_a_carrier_filters_the_source_by_the_warps_difference(statement, monkeypatch):
    import kwiiyatta_amd as k
    import kwiiyatta_amd.resynthesize_voice as rv
    filtered = []
    monkeypatch.setattr(k, 'apply_mlsa_filter', lambda wav, mcep: filtered.append((wav, mcep)) or 'filtered')
    source = _Source(2)
    ratio = 2.0 ** (5 / 12)
    assert rv.render(_conf(diffvc=True, formant_shift=5.0), source) == 'filtered'
    assert statement == [((FRAMES, BINS), ratio)]
    (wav, difference), = filtered
    assert wav.data.tobytes() == source.wavdata.data.tobytes() and wav.fs == FS
    sp = _envelope(2)
    want = _mcep_of(fc.shift(sp, ratio)[0]) - _mcep_of(sp)
    assert difference.data.tobytes() == want.tobytes() and np.abs(want).max() > 1e-3
    assert source.mel_cepstrum.data.tobytes() == _mcep_of(sp).tobytes()


def test_render_carrier_diffvc_warps_the_picture_before_the_difference(statement, monkeypatch):
    import kwiiyatta_amd as k
    import kwiiyatta_amd.resynthesize_voice as rv
    filtered = []
    monkeypatch.setattr(k, 'apply_mlsa_filter', lambda wav, mcep: filtered.append((wav, mcep)) or 'filtered')
    source, carrier = _Source(3), _Source(4)
    monkeypatch.setattr(k, 'align', lambda a, b: k.feature(a))           # (equal lengths: the picture is the source's)
    carrier_mcep = carrier.mel_cepstrum.data.copy()

    def conf(**options):
        c = _conf(carrier='carrier.wav', diffvc=True, **options)
        c.create_analyzer = lambda path, Analyzer=None: carrier
        return c
    sp = _envelope(3)
    assert rv.render(conf(formant_shift=0.0), source) == 'filtered'
    assert statement == []
    assert filtered[0][1].data.tobytes() == (_mcep_of(sp) - carrier_mcep).tobytes()
    ratio = 2.0 ** (-3 / 12)
    assert rv.render(conf(formant_shift=-3.0), source) == 'filtered'
    assert statement == [((FRAMES, BINS), ratio)]
    wav, difference = filtered[1]
    assert wav.data.tobytes() == carrier.wavdata.data.tobytes()
    assert difference.data.tobytes() == (_mcep_of(fc.shift(sp, ratio)[0]) - carrier_mcep).tobytes()
    # without --diffvc the carrier's f0 is taken and the warped picture synthesised
    c = conf(formant_shift=-3.0)
    c.diffvc = False
    out = rv.render(c, source)
    assert len(filtered) == 2 and len(statement) == 2 and out.data.size > 0


def test_convert_passes_the_shift_to_the_synthesised_output_only(statement, monkeypatch):
    import kwiiyatta_amd as k
    import kwiiyatta_amd.convert_voice as cv
    source = _Source(5)
    monkeypatch.setattr(cv, 'analyze_source', lambda conf, converter, path: source)
    monkeypatch.setattr(k, 'apply_mlsa_filter', lambda wav, mcep: 'filtered')

    class Converter:
        def convert(self, mcep, diff=False):
            out = copy.copy(mcep)
            out.data = mcep.data * (0.0 if diff else 1.0)
            return out
    plain = cv.convert(None, Converter(), 'a.wav', diffvc=False)
    assert statement == []
    assert cv.convert(None, Converter(), 'a.wav', diffvc=True, formant_shift=4.0) == 'filtered'
    assert statement == []
    shifted = cv.convert(None, Converter(), 'a.wav', diffvc=False, formant_shift=4.0)
    assert statement == [((FRAMES, BINS), 2.0 ** (4 / 12))]
    assert shifted.data.shape == plain.data.shape and shifted.data.tobytes() != plain.data.tobytes()
