"""The numpy statement of the mel-cepstral energy and its postfilter (tests/power_cases.py) against closed forms, and the
way of --postfilter / --keep-power down to the converter.  No GPU."""
import inspect
import sys

import numpy as np
import pytest

import power_cases as pc


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


def test_energy_of_a_flat_spectrum_is_exp_2_c0():
    for order, N, alpha in pc.CONFIGS:
        c = np.zeros((9, order + 1))
        c[:, 0] = np.linspace(-20.0, 3.0, 9)
        e = pc.energy(c, alpha, N)
        assert _ulps(e, np.exp(2.0 * c[:, 0])).max() <= 4, (order, N, alpha)


def test_energy_of_a_tilt_is_a_bessel_function():
    """alpha = 0, order 1: |H|^2 = exp(2 c0 + 2 c1 cos w), whose mean over N >= 512 equally spaced w is exp(2 c0) I0(2 c1)
    to rounding for |c1| <= 3.4 (the aliased terms I_N are below 1e-300).  Observed 6e-16 relative."""
    from scipy.special import i0
    rng = np.random.default_rng(5)
    c = np.stack((rng.uniform(-12.0, 2.0, 200), rng.uniform(-3.4, 3.4, 200)), axis=1)
    c[:2, 1] = (3.4, -3.4)
    e = pc.energy(c, 0.0, 512)
    dev = np.abs(e / (np.exp(2.0 * c[:, 0]) * i0(2.0 * c[:, 1])) - 1.0).max()
    print(f'E against exp(2 c0) I0(2 c1): {dev:.2e}')
    assert dev <= 1e-14


@pytest.mark.parametrize('beta', (0.0, 0.1, 1.0))
def test_keep_power_gives_the_reference_energy(beta):
    """E(out) / E(ref) - 1: observed 3.8e-15 at worst"""
    worst = 0.0
    for i, (order, N, alpha) in enumerate(pc.CONFIGS):
        rng = np.random.default_rng(100 + i)
        x, ref = (pc.rows_like_speech(rng, pc.ROWS, order) for _ in range(2))
        out, status = pc.postfilter(x, alpha, N, beta, ref=ref)
        assert status == 0
        worst = max(worst, np.abs(pc.energy(out, alpha, N) / pc.energy(ref, alpha, N) - 1.0).max())
        own, status = pc.postfilter(x, alpha, N, beta)                    # without a reference: its own energy
        assert status == 0
        worst = max(worst, np.abs(pc.energy(own, alpha, N) / pc.energy(x, alpha, N) - 1.0).max())
    print(f'beta {beta}: E(out) / E(ref) - 1 = {worst:.2e}')
    assert worst <= 2e-14


def test_emphasis_scales_the_upper_coefficients():
    for i, (order, N, alpha) in enumerate(pc.CONFIGS):
        x = pc.rows_like_speech(np.random.default_rng(200 + i), pc.ROWS, order)
        for beta in (0.1, 0.5, 1.0):
            y0, _ = pc.emphasis(x, 0.0, beta)
            assert y0[:, 1].tobytes() == x[:, 1].tobytes()
            assert y0[:, 2:].tobytes() == (x[:, 2:] * (1.0 + beta)).tobytes()
            y, bmax = pc.emphasis(x, alpha, beta)
            assert np.all(np.abs(y[:, 1] - x[:, 1]) <= 8 * pc.EPS * bmax), (order, beta)
            if order >= 2 and alpha:
                assert not np.array_equal(y[:, 2:], x[:, 2:])
            # differential form: base + (y - x)
            base = pc.rows_like_speech(np.random.default_rng(300 + i), pc.ROWS, order, c0=0.0)
            plain, _ = pc.postfilter(x, alpha, N, beta)
            diff, _ = pc.postfilter(x, alpha, N, beta, base=base)
            assert diff.tobytes() == (base + (plain - x)).tobytes()


def test_neutral_filter_copies_bit_for_bit():
    for i, (order, N, alpha) in enumerate(pc.CONFIGS):
        x = pc.rows_like_speech(np.random.default_rng(400 + i), pc.ROWS, order)
        x[5] = np.nan                                       # (no energy is formed: nothing to count)
        out, status = pc.postfilter(x, alpha, N, 0.0)
        assert out.tobytes() == x.tobytes() and status == 0 and out is not x
        base = x + 1.0
        out, status = pc.postfilter(x, alpha, N, 0.0, base=base)
        assert out.tobytes() == base.tobytes() and status == 0
        x[5] = x[6]
        out, status = pc.postfilter(x, alpha, N, 0.0, ref=x.copy())     # log 1 = +0
        assert out.tobytes() == x.tobytes() and status == 0
        y, _ = pc.emphasis(x, alpha, 0.0)
        assert y.tobytes() == x.tobytes()


@pytest.mark.parametrize('kind', pc.BAD_KINDS)
def test_bad_rows_are_copied_and_counted_once(kind):
    order, N, alpha = pc.CONFIGS[1]
    rng = np.random.default_rng(7)
    x, ref = (pc.rows_like_speech(rng, pc.ROWS, order) for _ in range(2))
    good, status = pc.postfilter(x, alpha, N, 0.3, ref=ref)
    assert status == 0
    for rows in ((0,), (33,), (pc.ROWS - 1,), (0, 33, pc.ROWS - 1)):
        bx, bref = x, ref
        for r in rows:
            bx, bref = pc.spoil(bx, bref, kind, r)
        out, status = pc.postfilter(bx, alpha, N, 0.3, ref=bref)
        assert status == len(rows)
        rest = np.setdiff1d(np.arange(pc.ROWS), rows)
        assert out[list(rows)].tobytes() == bx[list(rows)].tobytes()
        assert out[rest].tobytes() == good[rest].tobytes()                 # a row depends on itself and its reference
        base = x * 0.5
        out, status = pc.postfilter(bx, alpha, N, 0.3, ref=bref, base=base)
        assert status == len(rows) and out[list(rows)].tobytes() == base[list(rows)].tobytes()


def test_kernel_ceiling_at_order_24_is_about_4e_12():
    x = pc.rows_like_speech(np.random.default_rng(1), pc.ROWS, 24)
    c = pc.kernel_ceiling(x, x, 24)
    assert 1e-12 < c.max() < 1e-11


# ---------------------------------------------------------------------------------- the options' way down
def test_options_parse_and_refuse():
    import kwiiyatta_amd as k
    from kwiiyatta_amd import config, convert_voice, corpus

    def parsed(args):
        conf = k.Config()
        conf.add_power_arguments()
        conf.parser.parse_args(args=args, namespace=conf)
        return conf
    assert [o[0] for o in config.POWER_OPTIONS] == ['--postfilter', '--keep-power']
    neutral = parsed([])
    assert neutral.postfilter == 0.0 and neutral.keep_power is False
    both = parsed(['--postfilter', '0.2', '--keep-power'])
    assert both.postfilter == 0.2 and both.keep_power is True
    assert parsed(['--postfilter', '1']).postfilter == 1.0 and parsed(['--postfilter', '0']).postfilter == 0.0
    for bad in ('1.5', '-0.1', 'much'):
        with pytest.raises(SystemExit):
            parsed([f'--postfilter={bad}'])
    assert 'add_power_arguments' in inspect.getsource(convert_voice.main)
    for fn in (convert_voice.convert, convert_voice.convert_synth_batch):
        p = inspect.signature(fn).parameters
        assert p['postfilter'].default == 0.0 and p['keep_power'].default is False
    for fn in (corpus.convert_batch, corpus.ConvertWave.__init__):
        p = inspect.signature(fn).parameters
        assert p['postfilter_beta'].default == 0.0 and p['keep_power'].default is False
    p = inspect.signature(k.MelCepstrumConverter().convert).parameters
    assert p['postfilter'].default == 0.0 and p['keep_power'].default is False
    for fn in (k.apply_mlsa_filter, k.apply_diff_filter):
        assert inspect.signature(fn).parameters['use_c0'].default is False
    assert 'mcep_energy' in k.__all__ and 'postfilter_mcep' in k.__all__
    # argument checks come before any file is read or anything is put on the device
    for beta in (1.5, -0.1):
        with pytest.raises(ValueError, match='outside'):
            corpus.convert_batch([], 16000, None, postfilter_beta=beta)
        with pytest.raises(ValueError, match='outside'):
            convert_voice.convert(None, None, 'no such file.wav', postfilter=beta)
        with pytest.raises(ValueError, match='outside'):
            convert_voice.convert_synth_batch(None, None, ['no such file.wav'], postfilter=beta)
    with pytest.raises(ValueError, match='lockstep driver'):
        corpus.convert_batch([], 16000, None, driver='streams', keep_power=True)
    with pytest.raises(ValueError, match='lockstep driver'):
        corpus.convert_batch([], 16000, None, driver='streams', postfilter_beta=0.5)


def test_new_entry_points_are_in_the_ctypes_table():
    from kwiiyatta_amd import _lib
    for name, args in (('kwy_mcep_energy', 7), ('kwy_mcep_energy_dev', 7), ('kwy_mcep_energy_batch_dev', 6),
                       ('kwy_mcep_postfilter', 8), ('kwy_mcep_postfilter_dev', 11), ('kwy_mcep_postfilter_batch_dev', 8)):
        assert name in _lib.SIGNATURES and name not in _lib.MISSING
        assert len(_lib.SIGNATURES[name][1]) == args, name


def test_energy_fft_size_follows_the_vocoder():
    from kwiiyatta_amd.backend import power
    for fs, want in ((16000, 1024), (22050, 1024), (44100, 2048), (48000, 2048), (96000, 4096)):
        assert power.energy_fft_size(fs) == want, fs


def test_neutral_convert_never_imports_the_backend(monkeypatch):
    """convert() with postfilter=0.0 and keep_power=False takes the path it always took: backend.power is not imported
    and the result is what the conversion and the source's c0 give"""
    import kwiiyatta_amd as k
    from kwiiyatta_amd.converter import mcep as cm
    conv = cm.MelCepstrumFeatureConverter.__new__(cm.MelCepstrumFeatureConverter)
    conv.order, conv.fs, conv.gv_stats, conv.ms_stats = 3, 16000, None, None
    monkeypatch.setattr(cm.MelCepstrumFeatureConverter.__mro__[1], 'convert',
                        lambda self, shape, raw=None, **kw: shape * 2.0)
    for name in [n for n in sys.modules if n.endswith('backend.power')]:
        monkeypatch.delitem(sys.modules, name)
    import kwiiyatta_amd.backend as backend
    monkeypatch.delattr(backend, 'power', raising=False)
    rec =k.MelCepstrum(16000, 5.0, np.arange(20.0).reshape(5, 4))
    plain = conv.convert(rec).data
    assert conv.convert(rec, postfilter=0.0, keep_power=False).data.tobytes() == plain.tobytes()
    assert np.array_equal(plain[:, 0], rec.data[:, 0]) and np.array_equal(plain[:, 1:], rec.data[:, 1:] * 2.0)
    assert not [n for n in sys.modules if n.endswith('backend.power')]
    for beta in (1.5, -0.1):
        with pytest.raises(ValueError, match='outside'):
            conv.convert(rec, postfilter=beta)
