"""Mel-cepstral energy, formant-emphasis postfilter and power-preserving c0 on the MI355X: the kernels of
kwy_mcpower.hip through the C ABI against their numpy statement (tests/power_cases.py), their determinism, aliasing and
input edges, the converter, the differential filters with c0 in play, the lockstep batch driver and what
`convert_voice --batch --keep-power --postfilter` writes.

Columns 1..order of the filter are bit-equal to the statement.  Column 0 and kwy_mcep_energy differ from it by the order
of the sums over the bins and by cos / exp / log in the last place.  Measured on an MI355X over
test_kernel_against_the_statement's grid (rows in {0, 1, 3, 67}, order in {1, 2, 24, 25, 63}, N in {512, 2048, 8192},
alpha in {0, 0.41, 0.554}, beta in {0, 0.1, 1}, with and without ref and base): the largest deviation -- relative for E,
absolute for c0 -- is MEASURED_DEVIATION below; KERNEL_BOUND is four times that, rounded up to one significant digit.
It stays below the derived ceiling 32 eps (order + 2)(1 + sum|x| + sum|ref|) per row (power_cases.kernel_ceiling), which
every row is checked against as well."""
import pathlib
import shutil
import sys

import numpy as np
import pytest

import power_cases as pc
from conftest import CLB_DIR, SLT_DIR

pytestmark = pytest.mark.gpu

MEASURED_DEVIATION = 2.665e-15          # c0, at (order, N, alpha, beta, ref, base, rows) = (63, 512, 0.41, 1.0, yes, no, 67);
#                                         E: 1.554e-15 at (order, N, alpha, rows) = (63, 512, 0.554, 1)
KERNEL_BOUND = 2e-14                    # 4 x 2.665e-15 = 1.07e-14, rounded up to one digit

ROWS = (0, 1, 3, 67)
ALPHAS = (0.0, 0.41, 0.554)
BETAS = (0.0, 0.1, 1.0)


def _run_cli(main, argv):
    old = sys.argv
    sys.argv = ['prog'] + argv
    try:
        main()
    finally:
        sys.argv = old


def _device():
    import torch
    from kwiiyatta_amd import _lib
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    return dev, stream, _lib.Context(0, stream=stream.cuda_stream)


def _inputs(seed, order, rows=ROWS):
    rng = np.random.default_rng(seed)
    xs = [pc.rows_like_speech(rng, r, order) for r in rows]
    refs = [pc.rows_like_speech(rng, r, order, c0=-6.0) for r in rows]
    bases = [pc.rows_like_speech(rng, r, order, c0=0.0) for r in rows]
    return xs, refs, bases


# ---- the kernel against the statement ------------------------------------------------------------------------------
@pytest.mark.parametrize('N', (512, 2048, 8192))
@pytest.mark.parametrize('order', (1, 2, 24, 25, 63))
def test_kernel_against_the_statement(order, N):
    from kwiiyatta_amd.backend import power
    xs, refs, bases = _inputs(1000 * order + N, order)
    worst_c0, worst_e, at_c0, at_e = 0.0, 0.0, None, None
    for alpha in ALPHAS:
        tab = pc.cos_table(order, N, alpha)
        for x in xs:
            if len(x) == 0:
                assert power.frame_energy(x, alpha, N).shape == (0,)
                continue
            got, want = power.frame_energy(x, alpha, N), pc.energy(x, alpha, N, tab)
            dev = np.abs(got / want - 1.0)
            assert np.all(dev <= pc.kernel_ceiling(x, None, order))
            if dev.max() > worst_e:
                worst_e, at_e = dev.max(), (order, N, alpha, len(x))
        for beta in BETAS:
            for with_ref in (False, True):
                ref = refs if with_ref else None
                stated = [pc.filtered(x, alpha, N, beta, r if with_ref else None, tab) if len(x) else None
                          for x, r in zip(xs, refs)]
                for with_base in (False, True):
                    base = bases if with_base else None
                    got = power.postfilter(xs, beta, ref=ref, base=base, alpha=alpha, fft_size=N)
                    for i, (x, g) in enumerate(zip(xs, got)):
                        where = (order, N, alpha, beta, with_ref, with_base, len(x))
                        assert g.shape == x.shape
                        if len(x) == 0:
                            continue
                        b = bases[i] if with_base else None
                        if beta == 0 and not with_ref:
                            assert g.tobytes() == (x if b is None else b).tobytes(), where
                            continue
                        want, status = pc.compose(x, *stated[i], b)
                        assert status == 0
                        assert g[:, 1:].tobytes() == want[:, 1:].tobytes(), where
                        dev = np.abs(g[:, 0] - want[:, 0])
                        assert np.all(dev <= pc.kernel_ceiling(x, refs[i] if with_ref else x, order)), where
                        if dev.max() > worst_c0:
                            worst_c0, at_c0 = dev.max(), where
    print(f'mcpower order {order} N {N}: largest deviation from the statement: E relative {worst_e:.3e} at {at_e}, '
          f'c0 absolute {worst_c0:.3e} at {at_c0}')
    assert worst_e <= KERNEL_BOUND and worst_c0 <= KERNEL_BOUND
    assert worst_e > 0 or worst_c0 > 0                   # (the comparison did run)


# ---- one result, whatever the form, the batch, the run or the aliasing -----------------------------------------------
def test_forms_batches_runs_and_aliasing_are_bit_equal():
    import torch
    from kwiiyatta_amd.backend import power
    order, N, alpha, beta = 24, 2048, 0.554, 0.3
    dev, stream, ctx = _device()
    rng = np.random.default_rng(11)
    x, ref, base = (pc.rows_like_speech(rng, 67, order, c0=c) for c in (-8.0, -6.0, 0.0))
    host = power.postfilter(x, beta, ref=ref, base=base, alpha=alpha, fft_size=N, ctx=ctx)
    host_e = power.frame_energy(x, alpha, N, ctx=ctx)
    assert host.tobytes() != base.tobytes()
    dx, dref, dbase = (torch.from_numpy(a).to(dev) for a in (x, ref, base))
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, c_vp

    def single(xt, out, rows=67, status=None):
        _lib.check(ctx, lib.kwy_mcep_postfilter_dev(ctx.handle, c_vp(xt.data_ptr()), rows, order, alpha, N, beta,
                                                    c_vp(dref.data_ptr()), c_vp(dbase.data_ptr()), c_vp(out.data_ptr()),
                                                    None if status is None else c_vp(status.data_ptr())))
        stream.synchronize()
    # the _dev form, twice, with guard rows around the output and rows beyond `rows` left alone
    for _ in range(2):
        guarded = torch.full((67 + 8, order + 1), -7.0, dtype=torch.float64, device=dev)
        single(dx, guarded[4:])
        g = guarded.cpu().numpy()
        assert g[4:71].tobytes() == host.tobytes()
        assert np.all(g[:4] == -7.0) and np.all(g[71:] == -7.0)
    short = torch.full((67, order + 1), -7.0, dtype=torch.float64, device=dev)
    single(dx, short, rows=50)
    assert short.cpu().numpy()[:50].tobytes() == host[:50].tobytes() and bool((short[50:] == -7.0).all())
    e = torch.full((67 + 2,), -7.0, dtype=torch.float64, device=dev)
    _lib.check(ctx, lib.kwy_mcep_energy_dev(ctx.handle, c_vp(dx.data_ptr()), 67, order, alpha, N, c_vp(e[1:].data_ptr())))
    stream.synchronize()
    assert e.cpu().numpy()[1:68].tobytes() == host_e.tobytes() and float(e[0]) == -7.0 and float(e[68]) == -7.0
    # out == x and out == base
    inplace = dx.clone()
    single(inplace, inplace)
    assert inplace.cpu().numpy().tobytes() == host.tobytes()
    saved = dbase.clone()
    single(dx, dbase)
    assert dbase.cpu().numpy().tobytes() == host.tobytes()
    dbase.copy_(saved)
    # the job inside batches of 1, 3, 40 and 70 jobs (the last: more than one launch holds) of unequal rows
    for count in (1, 3, 40, 70):
        rows = [(7 * i) % 23 for i in range(count)]
        rows[count // 2] = 67
        xs, refs, bases, outs, es = [], [], [], [], []
        for i, r in enumerate(rows):
            if r == 67:
                xs.append(dx), refs.append(dref), bases.append(dbase)
            else:
                a, b, c = (pc.rows_like_speech(rng, r, order) for _ in range(3))
                xs.append(torch.from_numpy(a).to(dev)), refs.append(torch.from_numpy(b).to(dev))
                bases.append(torch.from_numpy(c).to(dev) if i % 2 else None)
                if i % 3 == 0:
                    refs[-1] = None
            outs.append(torch.full((r, order + 1), -7.0, dtype=torch.float64, device=dev))
            es.append(torch.full((r,), -7.0, dtype=torch.float64, device=dev))
        status = torch.full((count,), -1, dtype=torch.int32, device=dev)
        power.postfilter_batch_dev(ctx, xs, outs, alpha, N, beta, refs=refs, bases=bases, status=status)
        power.frame_energy_batch_dev(ctx, xs, es, alpha, N)
        stream.synchronize()
        assert status.cpu().tolist() == [0] * count
        k = count // 2
        assert outs[k].cpu().numpy().tobytes() == host.tobytes(), count
        assert es[k].cpu().numpy().tobytes() == host_e.tobytes(), count
        for i, r in enumerate(rows):                      # every other job against its own single call
            if r in (0, 67) or i % 5:
                continue
            alone = power.postfilter(xs[i].cpu().numpy(), beta, ref=None if refs[i] is None else refs[i].cpu().numpy(),
                                     base=None if bases[i] is None else bases[i].cpu().numpy(), alpha=alpha, fft_size=N,
                                     ctx=ctx)
            assert outs[i].cpu().numpy().tobytes() == alone.tobytes(), (count, i)


MP_JOBS_MAX = 64             # matrices per launch (kwy_mcpower.hip)


def test_energies_of_one_matrix_more_than_a_launch_holds():
    """kwy_mcep_energy_batch_dev on MP_JOBS_MAX + 1 tiny matrices of unequal rows in ONE call, the matrix that falls
    into the second launch without rows: every matrix equals the same matrix through the single call, bit for bit"""
    import torch
    from kwiiyatta_amd.backend import power
    order, N, alpha = 24, 1024, 0.41
    dev, stream, ctx = _device()
    rng = np.random.default_rng(23)
    xs = [pc.rows_like_speech(rng, 1 + i % 5, order) for i in range(MP_JOBS_MAX)] + [np.zeros((0, order + 1))]
    dxs = [torch.from_numpy(x).to(dev) for x in xs]
    es = [torch.full((len(x) + 1,), -7.0, dtype=torch.float64, device=dev) for x in xs]
    power.frame_energy_batch_dev(ctx, dxs, es, alpha, N)
    stream.synchronize()
    for i, (x, e) in enumerate(zip(xs, es)):
        got = e.cpu().numpy()
        assert got[:-1].tobytes() == power.frame_energy(x, alpha, N, ctx=ctx).tobytes() and got[-1] == -7.0, i


# ---- rows that cannot be filtered ------------------------------------------------------------------------------------
def test_status_words_count_the_bad_rows():
    import torch
    from kwiiyatta_amd.backend import power
    order, N, alpha, beta = 24, 1024, 0.41, 0.3
    dev, stream, ctx = _device()
    rng = np.random.default_rng(21)
    x, ref = (pc.rows_like_speech(rng, 67, order) for _ in range(2))
    base = x * 0.5
    mats = [(x, ref)]
    for kind in pc.BAD_KINDS:
        bx, bref = x, ref
        for r in (0, 33, 66):
            bx, bref = pc.spoil(bx, bref, kind, r)
        mats.append((bx, bref))
    for with_base in (False, True):
        want = [pc.postfilter(a, alpha, N, beta, ref=b, base=base if with_base else None) for a, b in mats]
        assert [s for _, s in want] == [0, 3, 3, 3]
        xs = [torch.from_numpy(a).to(dev) for a, _ in mats]
        refs = [torch.from_numpy(b).to(dev) for _, b in mats]
        bases = [torch.from_numpy(base).to(dev) for _ in mats] if with_base else None
        outs = [torch.full_like(a, -7.0) for a in xs]
        status = torch.full((4,), -1, dtype=torch.int32, device=dev)
        power.postfilter_batch_dev(ctx, xs, outs, alpha, N, beta, refs=refs, bases=bases, status=status)
        stream.synchronize()
        assert status.cpu().tolist() == [0, 3, 3, 3]
        for (w, _), o, (a, _) in zip(want, outs, mats):
            g = o.cpu().numpy()
            assert g[:, 1:].tobytes() == w[:, 1:].tobytes()
            assert g[[0, 33, 66]].tobytes() == w[[0, 33, 66]].tobytes()
            assert np.abs(np.delete(g, [0, 33, 66], axis=0)[:, 0] - np.delete(w, [0, 33, 66], axis=0)[:, 0]).max() <= KERNEL_BOUND
        with pytest.raises(ValueError, match=r'9 frame\(s\) of utterance\(s\) \[1, 2, 3\]'):
            power.check_status(status)
    with pytest.raises(ValueError, match=r'3 frame\(s\) of utterance\(s\) \[0\]'):
        power.postfilter(mats[1][0], beta, ref=mats[1][1], alpha=alpha, fft_size=N, ctx=ctx)
    # beta == 0 without a reference forms no energy: the rows are copied, nothing is counted
    nan = torch.from_numpy(mats[1][0]).to(dev)
    out = torch.full_like(nan, -7.0)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    power.postfilter_batch_dev(ctx, [nan], [out], alpha, N, 0.0, status=status)
    stream.synchronize()
    assert status.cpu().tolist() == [0] and out.cpu().numpy().tobytes() == mats[1][0].tobytes()


def test_bad_arguments_write_nothing():
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib, c_vp
    from kwiiyatta_amd.backend import power
    dev, stream, ctx = _device()
    x = torch.from_numpy(pc.rows_like_speech(np.random.default_rng(3), 67, 63)).to(dev)
    out = torch.full_like(x, 9.0)
    e = torch.full((67,), 9.0, dtype=torch.float64, device=dev)
    status = torch.full((3,), 9, dtype=torch.int32, device=dev)
    stream.synchronize()
    torch.cuda.synchronize()

    def single(order=24, alpha=0.41, N=1024, beta=0.5, rows=67, x_=True, out_=True):
        return lib.kwy_mcep_postfilter_dev(ctx.handle, c_vp(x.data_ptr()) if x_ else None, rows, order, alpha, N, beta, None,
                                           None, c_vp(out.data_ptr()) if out_ else None, c_vp(status.data_ptr()))

    def energy(order=24, alpha=0.41, N=1024, rows=67, x_=True, out_=True):
        return lib.kwy_mcep_energy_dev(ctx.handle, c_vp(x.data_ptr()) if x_ else None, rows, order, alpha, N,
                                       c_vp(e.data_ptr()) if out_ else None)

    def batch(call, struct, row, **kw):
        """the bad job as the middle one of three"""
        good = struct.__name__ == 'McPowerJob' and (x, None, None, out, 0) or (x, 0, e)
        jobs = _lib.job_array(struct, [good, row, good])
        return call(ctx.handle, jobs, 3, *kw.values())
    common = [dict(order=0), dict(order=64), dict(order=-1), dict(N=256), dict(N=1000), dict(N=1536), dict(N=16384),
              dict(N=0), dict(alpha=1.0), dict(alpha=float('nan')), dict(rows=-1), dict(x_=False), dict(out_=False)]
    for kw in common + [dict(beta=-0.1), dict(beta=1.5), dict(beta=float('nan'))]:
        assert single(**kw) == _lib.KWY_EINVAL, kw
        assert 'mcep_postfilter' in ctx.error()
    for kw in common:
        assert energy(**kw) == _lib.KWY_EINVAL, kw
        assert 'mcep_energy' in ctx.error()
    args = dict(order=24, alpha=0.41, N=1024, beta=0.5, status=c_vp(status.data_ptr()))
    for row in ((x, None, None, out, -1), (None, None, None, out, 67), (x, None, None, None, 67)):
        assert batch(lib.kwy_mcep_postfilter_batch_dev, _lib.McPowerJob, row, **args) == _lib.KWY_EINVAL, row
    args = dict(order=24, alpha=0.41, N=1024)
    for row in ((x, -1, e), (None, 67, e), (x, 67, None)):
        assert batch(lib.kwy_mcep_energy_batch_dev, _lib.EnergyJob, row, **args) == _lib.KWY_EINVAL, row
    assert lib.kwy_mcep_postfilter_batch_dev(ctx.handle, None, 3, 24, 0.41, 1024, 0.5, None) == _lib.KWY_EINVAL
    assert lib.kwy_mcep_postfilter_batch_dev(ctx.handle, None, -1, 24, 0.41, 1024, 0.5, None) == _lib.KWY_EINVAL
    assert lib.kwy_mcep_energy_batch_dev(ctx.handle, None, 3, 24, 0.41, 1024) == _lib.KWY_EINVAL
    assert lib.kwy_mcep_energy_batch_dev(ctx.handle, None, -1, 24, 0.41, 1024) == _lib.KWY_EINVAL
    ctx.sync()
    assert bool((out == 9.0).all()) and bool((e == 9.0).all()) and status.cpu().tolist() == [9, 9, 9]
    # count == 0 is not an error
    assert lib.kwy_mcep_postfilter_batch_dev(ctx.handle, None, 0, 24, 0.41, 1024, 0.5, None) == _lib.KWY_OK
    assert lib.kwy_mcep_energy_batch_dev(ctx.handle, None, 0, 24, 0.41, 1024) == _lib.KWY_OK
    # the host entries: the same checks, as ValueError
    xh = np.zeros((5, 25))
    for kw in (dict(beta=1.5), dict(beta=-0.1), dict(fft_size=1000), dict(alpha=1.0)):
        with pytest.raises(ValueError):
            power.postfilter(xh, **{**dict(beta=0.5, alpha=0.41, fft_size=1024), **kw}, ctx=ctx)
    with pytest.raises(ValueError, match='order'):
        power.postfilter(np.zeros((5, 65)), 0.5, alpha=0.41, fft_size=1024, ctx=ctx)
    with pytest.raises(ValueError, match='same shapes'):
        power.postfilter(xh, 0.5, ref=np.zeros((4, 25)), alpha=0.41, fft_size=1024, ctx=ctx)
    with pytest.raises(ValueError, match='dtype mismatch'):
        power.frame_energy(xh.astype(np.float32), 0.41, 1024, ctx=ctx)


# ---- converter, filters, batch driver, command line -------------------------------------------------------------------
@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """convert_voice trained on 4 CLB -> SLT files (16 kHz) with 2 components and seed 0, its one run the batch
    conversion of two of them with both options; the model file"""
    import kwiiyatta_amd.convert_voice as cv
    root = tmp_path_factory.mktemp('power')
    src = root / 'src'
    src.mkdir()
    for n in range(1, 5):
        shutil.copy(pathlib.Path(CLB_DIR) / f'arctic_a{n:04}.wav', src)
    inputs = [str(src / f'arctic_a{n:04}.wav') for n in range(1, 3)]
    np.random.seed(0)
    _run_cli(cv.main, ['--source', str(src), '--target', SLT_DIR, '--converter-seed', '0', '--converter-components', '2',
                       '--max-files', '4', '--result-dir', str(root / 'out'), '--converter-model', str(root / 'model.npz'),
                       '--batch', '--keep-power', '--postfilter', '0.2'] + inputs)
    return root, inputs


def _converter(root):
    import kwiiyatta_amd as k
    return k.MelCepstrumConverter(use_delta=True, components=2).load(root / 'model.npz')


def test_convert_voice_batch_writes_both_outputs(trained):
    from scipy.io import wavfile as sio
    root, inputs = trained
    for p in inputs:
        for kind in ('synth', 'diff'):
            fs, pcm = sio.read(root / 'out' / f'{pathlib.Path(p).stem}.{kind}.wav')
            assert fs == 16000 and pcm.dtype == np.int16 and len(pcm) > 16000 and np.abs(pcm).max() > 1000, (p, kind)
    with np.load(root / 'model.npz') as z:
        assert not [n for n in z.files if 'power' in n or 'postfilter' in n or 'beta' in n]


def test_converter_keeps_the_power(trained):
    import kwiiyatta_amd as k
    root, inputs = trained
    conv = _converter(root)
    N = 1024
    for p in inputs:
        mcep = k.analyze_wav(p).mel_cepstrum
        src = np.ascontiguousarray(mcep.data)
        alpha = mcep.alpha()
        e_src = pc.energy(src, alpha, N)
        plain = conv.convert(mcep).data
        assert conv.convert(mcep, postfilter=0.0, keep_power=False).data.tobytes() == plain.tobytes()
        d_plain = conv.convert(mcep, diff=True).data
        assert conv.convert(mcep, diff=True, postfilter=0.0, keep_power=False).data.tobytes() == d_plain.tobytes()
        e_plain = pc.energy(plain, alpha, N)
        db = 10 * np.abs(np.log10(e_plain / e_src))
        print(f'{pathlib.Path(p).stem}: the conversion moves the frame energy by up to {db.max():.2f} dB '
              f'(median {np.median(db):.2f} dB)')
        assert db.max() > 0.1
        assert np.allclose(k.mcep_energy(mcep), e_src, rtol=KERNEL_BOUND, atol=0)
        kept = conv.convert(mcep, keep_power=True).data
        assert kept[:, 1:].tobytes() == plain[:, 1:].tobytes()
        dev = np.abs(pc.energy(kept, alpha, N) / e_src - 1.0).max()
        print(f'  keep_power: E / E(source) - 1 = {dev:.2e}')
        assert dev <= 2 * KERNEL_BOUND
        d_kept = conv.convert(mcep, diff=True, keep_power=True).data
        assert d_kept[:, 1:].tobytes() == (d_plain[:, 1:] + 0.0).tobytes()
        dev = np.abs(pc.energy(src + d_kept, alpha, N) / e_src - 1.0).max()
        print(f'  diff, keep_power: E(source + differential) / E(source) - 1 = {dev:.2e}')
        assert dev <= 2 * KERNEL_BOUND
        sharp = conv.convert(mcep, postfilter=0.3).data
        assert sharp[:, 2:].tobytes() != plain[:, 2:].tobytes()
        dev = np.abs(pc.energy(sharp, alpha, N) / e_plain - 1.0).max()
        print(f'  postfilter 0.3: E / E(convert()) - 1 = {dev:.2e}')
        assert dev <= 2 * KERNEL_BOUND
        both = conv.convert(mcep, postfilter=0.3, keep_power=True).data
        assert both[:, 1:].tobytes() == sharp[:, 1:].tobytes()
        assert np.abs(pc.energy(both, alpha, N) / e_src - 1.0).max() <= 2 * KERNEL_BOUND
        rec = k.postfilter_mcep(k.MelCepstrum(mcep.fs, mcep.frame_period, plain), 0.3, power_of=mcep)
        assert rec.data.tobytes() == both.tobytes()


@pytest.mark.parametrize('method', ('mlsa', 'fft'))
def test_filters_take_c0_into_account(trained, method):
    """a constant column 0 of g scales the output by exp(g); without use_c0 the call is today's.
    Where every output sample is a chain of products -- the MLSA filter of a mel-cepstrum with nothing but c0 -- the two
    agree within 4 ulp of every sample.  With shape coefficients, and in the FFT form always, a sample is a sum that
    cancels: the two runs round their sums independently, and no bound in ulps of a sample near a zero crossing can
    hold (measured on an MI355X, g = 0.25: MLSA 20090 ulp of the worst sample, which is 5.0 ulp of the peak).  There the
    bound is the one the project's two evaluations of a differential filter agree to, 1e-12 of the peak
    (test_convert_batch_fft_diff_outputs)."""
    import kwiiyatta_amd as k
    root, inputs = trained
    a = k.analyze_wav(inputs[0])
    rng = np.random.default_rng(2)
    g = 0.25
    for shaped in (False, True):
        rec = k.MelCepstrum(a.fs, a.frame_period, pc.rows_like_speech(rng, len(a.mel_cepstrum.data), 24, c0=0.0) * 0.2)
        if not shaped:
            rec.data[:, 1:] = 0.0
        rec.data[:, 0] = g
        today = k.apply_diff_filter(a.wavdata, rec, method=method)
        assert k.apply_diff_filter(a.wavdata, rec, method=method, use_c0=False).data.tobytes() == today.data.tobytes()
        if method == 'mlsa':
            assert k.apply_mlsa_filter(a.wavdata, rec).data.tobytes() == today.data.tobytes()
            assert k.apply_mlsa_filter(a.wavdata, rec, use_c0=False).data.tobytes() == today.data.tobytes()
        scaled = k.apply_diff_filter(a.wavdata, rec, method=method, use_c0=True).data
        want = np.exp(g) * today.data
        assert np.abs(want).max() > 0
        live = want != 0
        ulps = np.abs(scaled - want)[live] / np.spacing(np.abs(want[live]))
        peak = np.abs(scaled - want).max() / np.spacing(np.abs(want).max())
        print(f'{method}, shape coefficients {shaped}: use_c0 against exp(g) x: {ulps.max():.1f} ulp of the sample at '
              f'worst, {peak:.2f} ulp of the peak')
        if method == 'mlsa' and not shaped:
            assert ulps.max() <= 4 and np.array_equal(scaled[~live], want[~live])
        assert np.abs(scaled - want).max() <= 1e-12 * np.abs(want).max()


def test_convert_batch_with_and_without_the_options(trained):
    import torch
    import kwiiyatta_amd as k
    from kwiiyatta_amd import corpus, pipeline as pl
    from kwiiyatta_amd.backend import power
    root, inputs = trained
    conv = _converter(root)
    an = [k.analyze_wav(p) for p in inputs]
    waves = [np.ascontiguousarray(a.wavdata.data) for a in an]
    opts = dict(order=conv.order, frame_period=5.0, pcm=True, diff=True)
    r0 = corpus.convert_batch(waves, 16000, conv.gmm, **opts)
    r1 = corpus.convert_batch(waves, 16000, conv.gmm, postfilter_beta=0.0, keep_power=False, **opts)
    for xs, ys in zip(r0, r1):
        for a, b in zip(xs, ys):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    active = dict(postfilter_beta=0.3, keep_power=True)
    r2 = corpus.convert_batch(waves, 16000, conv.gmm, **active, **opts)
    for xs, ys in zip(r0, r2):
        for a, b in zip(xs, ys):
            assert a.cpu().numpy().tobytes() != b.cpu().numpy().tobytes()
    r3 = corpus.convert_batch(waves, 16000, conv.gmm, diff_filter='fft', **active, **opts)
    # the waves themselves: the filtered mel-cepstra against the filter on the unfiltered wave's, and against convert()
    ls = corpus._Lockstep(0)
    dg = pl.DeviceGMM(conv.gmm.weights_, conv.gmm.means_, conv.gmm.covariances_, ls.dev)
    plain = corpus.ConvertWave(ls, 16000, waves, gmm=dg, order=conv.order, diff=True)
    plain.run()
    wave = corpus.ConvertWave(ls, 16000, waves, gmm=dg, order=conv.order, diff=True, **active)
    wave.run()
    ls.sync()
    assert plain.power_status is None and wave.power_status.cpu().tolist() == [0] * 4
    rows = corpus.Ragged(wave.T)
    alpha, N = wave.alpha, 1024
    views = lambda t: [v.cpu().numpy() for v in rows.views(t)]  # noqa: E731
    for i, (src, p, d, got_p, got_d) in enumerate(zip(views(wave.mc), views(plain.mc_conv), views(plain.mc_diff),
                                                      views(wave.mc_conv), views(wave.mc_diff))):
        assert np.array_equal(p[:, 0], src[:, 0])
        want_p = power.postfilter(p, 0.3, ref=src, alpha=alpha, fft_size=N)
        base = np.hstack((np.zeros_like(d[:, :1]), d[:, 1:]))
        want_d = power.postfilter(src + base, 0.3, ref=src, base=base, alpha=alpha, fft_size=N)
        assert got_p.tobytes() == want_p.tobytes() and got_d.tobytes() == want_d.tobytes(), i
        stated, status = pc.postfilter(p, alpha, N, 0.3, ref=src)
        assert status == 0 and np.abs(got_p - stated).max() <= KERNEL_BOUND
        assert np.abs(pc.energy(got_p, alpha, N) / pc.energy(src, alpha, N) - 1).max() <= 2 * KERNEL_BOUND
        assert np.abs(pc.energy(src + got_d, alpha, N) / pc.energy(src, alpha, N) - 1).max() <= 2 * KERNEL_BOUND
        # converter.convert of the same mel-cepstra: its conversion differs from the wave's by d0 (another entry of the
        # same MLPG), which the emphasis carries with a gain below (1 + beta)(1 + alpha)^2 < 4 per coefficient and the c0
        # correction with one below 1 per coefficient
        rec = k.MelCepstrum(16000, 5.0, src)
        d0 = max(np.abs(conv.convert(rec).data - p).max(), np.abs(conv.convert(rec, diff=True).data[:, 1:] - d[:, 1:]).max())
        bound = KERNEL_BOUND + 4 * (conv.order + 1) * d0
        dev_p = np.abs(conv.convert(rec, postfilter=0.3, keep_power=True).data - got_p).max()
        dev_d = np.abs(conv.convert(rec, diff=True, postfilter=0.3, keep_power=True).data - got_d).max()
        print(f'file {i}: wave against convert(): plain {dev_p:.2e}, differential {dev_d:.2e} (conversions differ by '
              f'{d0:.2e}; bound {bound:.2e})')
        assert dev_p <= bound and dev_d <= bound
        # the PCM outputs: test_convert_batch_fft_diff_outputs' comparison, with c0 in play
        rec.data = got_d
        ref = k.apply_diff_filter(an[i].wavdata, rec, method='fft', use_c0=True)
        got = r3[2][i].cpu().numpy()
        assert got.shape == ref.data.shape
        assert np.abs(got - ref.data).max() <= 1e-12 * max(1.0, np.abs(ref.data).max())
        assert np.array_equal(r3[3][i].cpu().numpy(), k.Wavdata(16000, got.copy())._pcm16(True, {}))
        ref = k.apply_mlsa_filter(an[i].wavdata, rec, use_c0=True)
        got = r2[2][i].cpu().numpy()
        assert np.abs(got - ref.data).max() <= 1e-12 * max(1.0, np.abs(ref.data).max())
        assert np.array_equal(r2[3][i].cpu().numpy(), k.Wavdata(16000, got.copy())._pcm16(True, {}))
    assert all(torch.equal(a, b) for a, b in zip(r2[1], r3[1]))          # (the synthesised outputs ignore the filter)
    with pytest.raises(ValueError, match='outside'):
        corpus.convert_batch(waves, 16000, conv.gmm, postfilter_beta=1.5, **opts)
