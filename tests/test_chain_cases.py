"""The composite of tests/chain_cases.py on the host: the reference alone stays well inside the bound it is used with,
the bound tells the documented order of the filters from its near misses, and `corpus._check_status_words` folds the
waves' status words into global positions.  No GPU."""
import numpy as np
import pytest

import chain_cases as ch
import power_cases as pc
from kwiiyatta_amd.backend import sptk

ALPHA = sptk.mcepalpha(ch.FS)


def _cases():
    rows = ch.host_rows()
    stats = ch.statistics([plain for _, plain, _ in rows])
    return rows, stats


def test_the_constants_are_the_projects():
    import test_power_gpu
    from kwiiyatta_amd.backend import bap
    from kwiiyatta_amd.synthetic import make_utterance
    assert ch.KERNEL_BOUND == test_power_gpu.KERNEL_BOUND
    assert 0.4 < ALPHA < 0.42 and bap.check_rate(ch.FS) >= 1
    assert tuple(len(make_utterance(seed=1, fs=ch.FS, seconds=s)[1]) for s in ch.SECONDS) == ch.FRAMES
    assert set(ch.NUMERIC) <= set(ch.TABLE) and set(ch.PLAIN_ONLY_OF.values()) <= set(ch.TABLE)
    subsets = {tuple(sorted(k for k, v in f.items() if v)) for f, diff, conv in ch.TABLE.values() if diff and not conv}
    assert len(subsets) == 10                   # every subset of {ms, gv, power}, power alone in its three variants


@pytest.mark.parametrize('name', ch.NUMERIC)
def test_the_composite_alone_stays_within_a_quarter_of_the_bound(name):
    """the composite on rows moved by one ulp with random signs, three draws, against the composite of the rows as
    they are: what the reference itself can be off by.  (The statements cast to float64 and transform with np.fft, so
    none of them can be evaluated in np.longdouble.)"""
    rows, stats = _cases()
    filters, diff, _ = ch.TABLE[name]
    rng = np.random.default_rng(5)
    worst = 0.0
    for src, plain, d in rows:
        d = d if diff else None
        want = ch.composite(src, plain, d, stats, ALPHA, **filters)
        bound = ch.bounds(src, plain, d, stats, **filters)
        for _ in range(3):
            moved = [ch.one_ulp(rng, a) if a is not None else None for a in (src, plain, d)]
            got = ch.composite(*moved, stats, ALPHA, **filters)
            for g, w, b in zip(got, want, bound):
                if w is None:
                    continue
                first = 0 if filters.get('beta') or filters.get('keep_power') else 1     # (c0 moves with the power filter)
                worst = max(worst, (np.abs(g - w).max(axis=0)[first:] / b[first:]).max())
    print(f'{name}: composite of rows one ulp away / bound = {worst:.3e}')
    assert 0 < worst <= 0.25


@pytest.mark.parametrize('variant', ch.MUTANTS)
def test_the_bound_tells_the_order_from_its_near_misses(variant):
    rows, stats = _cases()
    filters = ch.TABLE['ms+gv+power'][0]
    least = np.inf
    for src, plain, d in rows:
        want = ch.composite(src, plain, d, stats, ALPHA, **filters)
        got = ch.composite(src, plain, d, stats, ALPHA, variant=variant, **filters)
        bound = ch.bounds(src, plain, d, stats, **filters)
        # the plain rows of 'base_not_updated' are the right ones: that mutant shows in the differential rows alone
        which = (1,) if variant == 'base_not_updated' else (0, 1)
        if variant == 'base_not_updated':
            assert got[0].tobytes() == want[0].tobytes()
        for q in which:
            least = min(least, (np.abs(got[q] - want[q]).max(axis=0)[1:] / bound[q][1:]).max())
    print(f'{variant}: deviation / bound >= {least:.3e}')
    assert least >= 1e6


def test_the_energy_claim_holds_for_the_composite():
    rows, stats = _cases()
    filters = ch.TABLE['ms+gv+power'][0]
    for src, plain, d in rows:
        P, D = ch.composite(src, plain, d, stats, ALPHA, **filters)
        e = pc.energy(src, ALPHA, ch.FFT)
        assert np.abs(pc.energy(P, ALPHA, ch.FFT) / e - 1).max() <= 2 * ch.KERNEL_BOUND
        assert np.abs(pc.energy(src + D, ALPHA, ch.FFT) / e - 1).max() <= 2 * ch.KERNEL_BOUND


# ---- the status words of a batch's waves -----------------------------------------------------------------------------
MESSAGES = dict(dio=(RuntimeError, r'dio: zero-crossing buffer overflow in utterance\(s\) {}'),
                pyin=(ValueError, r'pyin: a sample of the signal is not finite in utterance\(s\) {}'),
                f0_map=(ValueError, r'f0 map: {} frame\(s\) of track\(s\) {} are'),
                gv=(ValueError, r'global variance: {} coefficient\(s\) of utterance\(s\) {} were'),
                ms=(ValueError, r'modulation spectrum: {} bin\(s\) of utterance\(s\) {} were'),
                formant=(ValueError, r'formant shift: {} row\(s\) of wave\(s\) {} were'),
                gvgen=(ValueError, r'GV ascent: coefficients of utterance\(s\) {} were'),
                power=(ValueError, r'postfilter: {} frame\(s\) of utterance\(s\) {} were'))
WAVES = ((3,), (2, 3), (4, 1, 2))               # the utterances per wave: one, two and three waves of unequal size


def _words(kind, sizes, marks):
    """the (kind, words, words per utterance) items of waves of the given sizes, all zero but `marks`: {global position
    of an utterance (of a wave, for 'formant'): count}, set in the LAST word of the utterance"""
    import torch
    per = 2 if kind in ('power', 'gvgen') else 1
    items, first = [], 0
    for w, n in enumerate(sizes):
        count = 1 if kind == 'formant' else n
        words = torch.zeros(per * count, dtype=torch.int32)
        for pos, value in marks.items():
            local = pos - (w if kind == 'formant' else first)
            if 0 <= local < count:
                words[(per - 1) * count + local] = value          # the differential word: behind the wave's plain ones
        items.append((kind, words, per))
        first += n
    return items


def _pattern(kind, marks):
    where = str(sorted(marks)).replace('[', r'\[').replace(']', r'\]')
    fields = (where,) if kind in ('dio', 'pyin', 'gvgen') else (sum(marks.values()), where)
    return MESSAGES[kind][1].format(*fields)


@pytest.mark.parametrize('sizes', WAVES, ids=str)
def test_status_words_name_global_positions(sizes):
    from kwiiyatta_amd import corpus
    assert tuple(MESSAGES) == corpus._STATUS_KINDS
    total = sum(sizes)
    for kind in corpus._STATUS_KINDS:
        count = len(sizes) if kind == 'formant' else total
        corpus._check_status_words(_words(kind, sizes, {}), ch.FS)                # all zero: nothing raised
        for marks in ({count - 1: 3}, {0: 1, count - 1: 2}, {count // 2: 5}):
            error, _ = MESSAGES[kind]
            with pytest.raises(error, match=_pattern(kind, marks)):
                corpus._check_status_words(_words(kind, sizes, marks), ch.FS)
    corpus._check_status_words([], ch.FS)


def test_status_kinds_are_checked_in_their_order():
    """every kind marked at once, the items handed over in the reverse order: the first kind of `_STATUS_KINDS` that is
    still marked is the one that raises"""
    from kwiiyatta_amd import corpus
    sizes = (2, 3)
    kinds = list(corpus._STATUS_KINDS)
    for first in range(len(kinds)):
        items = []
        for kind in reversed(kinds):
            marks = {1: 2} if kinds.index(kind) >= first else {}
            items += _words(kind, sizes, marks)
        # (a wave's items come together: sort by wave, keeping the reversed order of kinds within one)
        items = items[0::2] + items[1::2]
        error, _ = MESSAGES[kinds[first]]
        with pytest.raises(error, match=_pattern(kinds[first], {1: 2})):
            corpus._check_status_words(items, ch.FS)
