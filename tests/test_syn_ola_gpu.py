"""k_syn_ola (kwy_synth.hip): a workgroup adds, for one tile of 1024 output samples, the stored responses of the
candidate pulses -- those of the tiles within reach of a response -- in pulse order.  It reads the candidates'
positions 256 at a time and walks them in groups of four.  kw.synthesize against the oracle at the tolerance of
tests/test_synth_edges_gpu.py (synth_cases.assert_wave_close) on the tracks that stretch that walk: the most pulses
per tile the default 500 Hz pulses of an unvoiced track give, more candidates than one read of positions holds (f0
near fs / 12 with responses that reach two tiles), fewer samples than one tile, candidate counts that are no multiple
of the group; and one batched render of five utterances (two render groups) equal to the single calls.  The bits
themselves are tied to the kernel before by synth_bits_parent.npz and syn_zero_bits_parent.npz in the existing
tests."""
import numpy as np
import pytest

from synth_cases import _features, assert_wave_close, conditioned_samples, edge_case, y_length_of
from test_synth_edges_gpu import _batched_entries

pytestmark = pytest.mark.gpu

FS = 16000
TILE, GROUP, CHUNK = 1024, 4, 256               # SYN_TILE, SYN_OLA_GROUP, positions per read (kwy_synth.hip)


@pytest.fixture(scope='module')
def ko():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def kw():
    from kwiiyatta_amd.backend import world
    return world


def _track(f0, fft, seed):
    f0 = np.ascontiguousarray(f0, dtype=np.float64)
    sp, ap = _features(len(f0), fft // 2 + 1, np.random.default_rng([seed, len(f0), fft]))
    return f0, sp, ap


def candidates(ko, f0, fft, fs=FS):
    """per output tile: how many pulses lie in the tiles within reach of a response (fft / 2 samples)"""
    ylen = y_length_of(len(f0), fs)
    idx = ko.synth_timebase(f0, fs, 5.0, ylen, fft)[0]
    nt = (ylen + TILE - 1) // TILE
    reach = (fft // 2 + TILE - 1) // TILE
    per_tile = np.bincount(np.minimum(idx // TILE, nt - 1), minlength=nt)
    return [int(per_tile[max(0, t - reach):t + reach + 1].sum()) for t in range(nt)]


CASES = {
    # all unvoiced: a pulse every 32 samples, 32 per tile, 96 candidates
    'unvoiced': lambda: _track(np.zeros(60), 1024, 1),
    # 0.95 fs / 12 at 4096 points: 81 pulses per tile, responses reach two tiles -- ~400 candidates, two reads
    'dense_two_reads': lambda: _track(np.full(120, 0.95 * FS / 12.0), 4096, 2),
    # 800 samples: less than one tile
    'short': lambda: _track(np.full(10, 210.0), 1024, 3),
    # a varied track: the tiles' candidate counts differ
    'varied': lambda: edge_case(FS, 5)[:3],
}


@pytest.mark.parametrize('name', list(CASES))
def test_synthesis_against_the_oracle(ko, kw, name):
    f0, sp, ap = CASES[name]()
    fft = (sp.shape[1] - 1) * 2
    cand = candidates(ko, f0, fft)
    if name == 'unvoiced':
        assert max(cand) == 96
    elif name == 'dense_two_reads':
        assert max(cand) > CHUNK
    elif name == 'short':
        assert len(cand) == 1 and y_length_of(len(f0), FS) < TILE and cand[0] > 0
    else:
        assert any(c % GROUP for c in cand) and len(set(cand)) > 2
    cond = conditioned_samples(edge_case(FS, 5)[3], FS, fft) if name == 'varied' else ()
    got, ref = kw.synthesize(f0, sp, ap, FS, 5.0), ko.synthesize(f0, sp, ap, FS, 5.0)
    e = assert_wave_close(got, ref, fft, f'ola {name}', conditioned=cond)
    assert np.abs(got).max() > 0
    print(f'\nsyn ola {name}: candidates per tile {min(cand)}..{max(cand)}  local rel {e[0]:.3e}  abs rel {e[1]:.3e}')


def test_batch_of_five_equals_the_single_calls(kw):
    """kwy_synth_render_batch_dev renders four utterances per pass: five make two passes.  Every waveform equals its
    own kw.synthesize call, bit for bit."""
    from kwiiyatta_amd import _lib
    fft = 1024
    jobs = [_track(np.zeros(30), fft, 11), _track(np.full(10, 210.0), fft, 12), edge_case(FS, 13)[:3],
            _track(np.full(45, 0.9 * FS / 12.0), fft, 14), _track(np.r_[np.zeros(20), np.full(33, 333.0)], fft, 15)]
    got = _batched_entries(_lib.Context(0), jobs, FS, fft)
    for n, ((f0, sp, ap), g) in enumerate(zip(jobs, got)):
        assert np.array_equal(g, kw.synthesize(f0, sp, ap, FS, 5.0)), n
        assert np.abs(g).max() > 0, n
