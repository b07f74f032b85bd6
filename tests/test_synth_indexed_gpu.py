"""kwy_synth_job.ap_rows: the renderer reads the aperiodicity through a row index (row clamp(ap_rows[t], 0,
ap_src_rows - 1) of a source matrix wherever it read row t), so that an aligned conversion need not copy the source's
rows along its DTW index first.  The copy it replaces is kwy_gather_rows_dev, so everything here is bit equality
(torch.equal) between two kwy_synth_render_batch_dev calls through the C ABI: one on (ap_src, ap_rows), one on the rows
gathered beforehand by kwy_gather_rows_dev with the same index.  40 target frames from a 55-row source at 16 kHz (1024
points) and 48 kHz (2048 points):

  * an index with repeats, an index that runs backwards;
  * an index whose last entries are negative or >= ap_src_rows: the clamp.  The source is the middle of a larger
    block of other (valid) values, and the bad entries stay inside that block: a build that does not clamp reads the
    wrong rows, not foreign memory;
  * a batch of three: one job without an index, one unvoiced throughout, one of a single frame (no pulse is placed);
  * a track dense enough to overflow its response slots, as tests/test_syn_queue_gpu.py reaches them: the pulses beyond
    are rendered by k_syn_pulse<., true> straight onto y.

Every fifth source row has ap[:, 0] = 0.9999 (its square above the gate: no periodic response), so which row column 0
is read from shows as well.  Tried on scratch builds: without the two clamps `test_clamp` and
`test_pulses_beyond_the_slots` (whose index ends in -2 and ROWS + 2) fail at both rates and nothing else does; with the
floor row indexed and the ceiling row taken as row `ce` of the source, every rendering test fails at both rates (a
pulse between two frame times reads both rows).
"""
import numpy as np
import pytest

from synth_cases import slots

pytestmark = pytest.mark.gpu

RATES = ((16000, 1024), (48000, 2048))
FP = 5.0
T, ROWS, MARGIN = 40, 55, 64


def _source(fs, K, seed):
    """(block, ap_src): ap_src is rows MARGIN .. MARGIN + ROWS of a block whose rows all differ"""
    import torch
    rng = np.random.default_rng([seed, fs])
    k = np.arange(K)
    block = np.clip(0.1 + 0.8 * k[None, :] / K * rng.random((ROWS + 2 * MARGIN, 1)) + 0.05 * rng.standard_normal(
        (ROWS + 2 * MARGIN, K)), 0.001, 0.999)
    block[::5, 0] = 0.9999
    block = torch.from_numpy(np.ascontiguousarray(block)).cuda()
    return block, block[MARGIN:MARGIN + ROWS]


def _envelope(n, K, seed):
    rng = np.random.default_rng([seed, n, K])
    k = np.arange(K)
    return np.ascontiguousarray(np.exp(-k[None, :] / (K / 6.0)) * (1.0 + 0.3 * rng.random((n, 1))) * 1e-3 + 1e-9)


def _track(n=T):
    """voiced with a glide, unvoiced at both ends"""
    f0 = 150.0 + 60.0 * np.sin(np.arange(n) * 0.21)
    f0[:3] = 0.0
    f0[n - 4:] = 0.0
    return f0


def _render(fs, fft, jobs):
    """jobs: (f0, sp, ap_src or None, rows or None, ap or None); returns (indexed, gathered) lists of device waveforms.
    A job without rows is rendered from `ap` in both calls."""
    import torch
    from kwiiyatta_amd import _lib
    lib, K = _lib.lib, fft // 2 + 1
    ctx = _lib.Context(0)
    f0s = [torch.from_numpy(np.ascontiguousarray(j[0], dtype=np.float64)).cuda() for j in jobs]
    sps = [torch.from_numpy(j[1]).cuda() for j in jobs]
    ylens = [int(lib.kwy_synth_length(len(j[0]), FP, fs)) for j in jobs]
    plans = [torch.zeros(max(1, lib.kwy_synth_plan_bytes(n)), dtype=torch.uint8, device='cuda') for n in ylens]
    gathered = []
    for (f0, _, src, rows, ap) in jobs:
        if rows is None:
            gathered.append(ap)
            continue
        dst = torch.full((len(f0), K), float('nan'), dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        _lib.check(ctx, lib.kwy_gather_rows_dev(ctx.handle, src.data_ptr(), src.shape[0], K, rows.data_ptr(), len(f0),
                                                dst.data_ptr()))
        gathered.append(dst)
    torch.cuda.synchronize()
    parr = _lib.job_array(_lib.SynthPlanJob, [(f, len(j[0]), n, pl) for f, j, n, pl in zip(f0s, jobs, ylens, plans)])
    _lib.check(ctx, lib.kwy_synth_plan_batch_dev(ctx.handle, parr, len(jobs), fft, FP, fs))
    out = []
    for indexed in (True, False):
        ys = [torch.full((n,), float('nan'), dtype=torch.float64, device='cuda') for n in ylens]
        torch.cuda.synchronize()
        items = [(pl, sp, j[2], y, j[3]) if indexed and j[3] is not None else (pl, sp, g, y)
                 for pl, sp, j, g, y in zip(plans, sps, jobs, gathered, ys)]
        arr = _lib.synth_job_array(items)
        assert all((q.ap_rows is not None) == (indexed and j[3] is not None) for q, j in zip(arr, jobs))
        _lib.check(ctx, lib.kwy_synth_render_batch_dev(ctx.handle, arr, len(jobs), fft, FP, fs, 1.0))
        ctx.sync()
        out.append(ys)
    return out[0], out[1], gathered


def _rows(values):
    import torch
    return torch.tensor(np.asarray(values, dtype=np.int64).astype(np.int32), dtype=torch.int32, device='cuda')


def _check(a, b):
    import torch
    assert len(a) == len(b)
    for n, (x, y) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(y).all()), n
        assert torch.equal(x, y), n


def _one(fs, fft, index, seed, f0=None):
    K = fft // 2 + 1
    f0 = _track() if f0 is None else f0
    _, src = _source(fs, K, seed)
    rows = _rows(index)
    got, want, gathered = _render(fs, fft, [(f0, _envelope(len(f0), K, seed), src, rows, None)])
    _check(got, want)
    assert float(want[0].abs().max()) > 0
    return src, gathered[0], want[0]


@pytest.mark.parametrize('fs,fft', RATES)
def test_repeats(fs, fft):
    index = (np.arange(T) * 2) // 3 + 11            # 11, 11, 12, 13, 13, ...
    assert len(set(index.tolist())) < T and index.max() < ROWS
    src, gathered, _ = _one(fs, fft, index, 1)
    import torch
    assert torch.equal(gathered, src[torch.from_numpy(index).cuda()])          # (the copy is the plain row gather)


@pytest.mark.parametrize('fs,fft', RATES)
def test_backwards(fs, fft):
    index = ROWS - 1 - np.arange(T) - np.arange(T) // 3
    assert (np.diff(index) < 0).all() and index.min() >= 0
    _one(fs, fft, index, 2)


@pytest.mark.parametrize('fs,fft', RATES)
def test_clamp(fs, fft):
    """entries below 0 and from ap_src_rows on, among the VOICED frames and at the end: they read rows 0 and ROWS - 1"""
    import torch
    index = np.arange(T) + 7
    index[10:14] = (-1, -MARGIN, ROWS, ROWS + MARGIN - 1)
    index[T - 6:] = (-3, ROWS + 5, -MARGIN + 1, ROWS, -1, ROWS + 17)
    f0 = _track()
    assert (f0[10:14] > 0).all() and index.min() >= -MARGIN and index.max() < ROWS + MARGIN
    src, gathered, _ = _one(fs, fft, index, 3)
    assert torch.equal(gathered[11], src[0]) and torch.equal(gathered[13], src[ROWS - 1])


@pytest.mark.parametrize('fs,fft', RATES)
def test_batch_of_three(fs, fft):
    import torch
    K = fft // 2 + 1
    _, src = _source(fs, K, 4)
    plain = src[5:5 + T].clone()                                    # a job without an index: row t is row t
    index = (np.arange(T) * 5) // 4 + 2
    jobs = [(_track(), _envelope(T, K, 40), None, None, plain),
            (np.zeros(T), _envelope(T, K, 41), src, _rows(index), None),
            (np.full(1, 180.0), _envelope(1, K, 42), src, _rows([ROWS + 3]), None)]
    got, want, _ = _render(fs, fft, jobs)
    _check(got, want)
    assert float(want[0].abs().max()) > 0 and float(want[1].abs().max()) > 0
    assert len(want[2]) > 0 and bool((want[2] == 0).all())           # a single frame: nothing is placed
    # (and the job without an index equals the same rows through the identity index)
    ident, _, _ = _render(fs, fft, [(jobs[0][0], jobs[0][1], src, _rows(np.arange(T) + 5), None)])
    assert torch.equal(ident[0], want[0])


@pytest.mark.parametrize('fs,fft', RATES)
def test_pulses_beyond_the_slots(fs, fft):
    from oracle import oracle
    from kwiiyatta_amd import _lib
    f0 = np.full(T, 0.98 * fs / 12.0)                               # tests/test_syn_queue_gpu.py, job 3
    ylen = int(_lib.lib.kwy_synth_length(T, FP, fs))
    assert len(oracle.synth_timebase(f0, fs, FP, ylen, fft)[0]) > slots(ylen, fs)
    index = ROWS - 1 - (np.arange(T) * 4) // 3
    index[T - 2:] = (-2, ROWS + 2)
    _one(fs, fft, index, 5, f0=f0)


def test_refusals():
    """an index needs a row count; without an index the count is not looked at"""
    import torch
    from kwiiyatta_amd import _lib
    fs, fft = RATES[0]
    K = fft // 2 + 1
    lib, ctx = _lib.lib, _lib.Context(0)
    _, src = _source(fs, K, 6)
    f0 = torch.from_numpy(_track()).cuda()
    sp = torch.from_numpy(_envelope(T, K, 6)).cuda()
    ylen = int(lib.kwy_synth_length(T, FP, fs))
    plan = torch.zeros(lib.kwy_synth_plan_bytes(ylen), dtype=torch.uint8, device='cuda')
    y = torch.zeros(ylen, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    parr = _lib.job_array(_lib.SynthPlanJob, [(f0, T, ylen, plan)])
    _lib.check(ctx, lib.kwy_synth_plan_batch_dev(ctx.handle, parr, 1, fft, FP, fs))
    arr = _lib.synth_job_array([(plan, sp, src, y, _rows(np.arange(T)))])
    for bad in (0, -1, 2 ** 31):
        arr[0].ap_src_rows = bad
        assert lib.kwy_synth_render_batch_dev(ctx.handle, arr, 1, fft, FP, fs, 1.0) == -1
    arr = _lib.synth_job_array([(plan, sp, src, y)])
    arr[0].ap_src_rows = -5
    _lib.check(ctx, lib.kwy_synth_render_batch_dev(ctx.handle, arr, 1, fft, FP, fs, 1.0))
    ctx.sync()
    with pytest.raises(ValueError):
        _lib.synth_job_array([(plan, sp, src, y, _rows(np.arange(T - 1)))])
