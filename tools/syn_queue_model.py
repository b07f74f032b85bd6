#!/usr/bin/env python
"""tools/syn_queue_model.py [--unvoiced COST] [--slots N] : how the pulses of a rendering pass are dealt to workgroups,
as a scheduling model on the CPU ("the pulse queue").  Needs numpy and kwiiyatta_amd/synthetic.py.

The pulses are those of the benchmark's own 16 target f0 tracks of a wave (make_utterance, seeds 4321 + 2 i, warped to
11 s): one at every wrap of the per-sample phase, 500 Hz where unvoiced, as k_syn_phase places them.  A voiced pulse
costs 1, an unvoiced one COST (default 0.55: four transforms against seven -- an assumption, not a measurement).  The
chip is N equal slots (default 1536 = 256 CUs x 6 resident workgroups), every slot runs one workgroup at a time, and a
free slot takes the next workgroup of the grid (list scheduling).  A wave is rendered in 16 / G passes of G utterances;
the figure is the summed makespan of its passes in units of one voiced pulse.

  slices   each utterance a slice of max(64, 4096 / G) workgroups, workgroup b of it the pulses b, b + slice, ...
           (the mapping before the queue)
  stride   a grid of N workgroups over the pass's pulses laid end to end, workgroup w the pulses w, w + N, ...
  queue    a grid of N workgroups, each pulls the next pulse when it is free (k_syn_pulse<LOG2N, false> now)
  ideal    the wave's summed cost / N

The model knows nothing of what co-resident workgroups share (issue slots, LDS bandwidth, the instruction cache), which
on the chip makes a lonely straggler faster than one among six: read its gains as an upper bound."""
import argparse
import heapq
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from kwiiyatta_amd.synthetic import make_utterance  # noqa: E402

FS, FRAME_PERIOD, UNVOICED_HZ = 48000, 0.005, 500.0


def pulse_costs(f0, unvoiced_cost):
    """cost of every pulse of the track, in pulse order"""
    n = int(len(f0) * FRAME_PERIOD * FS)
    t = np.arange(n) / FS
    frames = np.arange(len(f0)) * FRAME_PERIOD
    voiced = np.interp(t, frames, (f0 > 0).astype(float)) > 0.5
    f = np.where(voiced, np.interp(t, frames, f0), UNVOICED_HZ)
    wraps = np.flatnonzero(np.diff(np.floor(np.cumsum(f) / FS)) > 0) + 1
    return np.where(voiced[wraps], 1.0, unvoiced_cost)


def list_schedule(jobs, slots):
    """makespan of `jobs` (in grid order) on `slots` equal slots, a free slot taking the next job"""
    free = [0.0] * slots
    for c in jobs:
        heapq.heapreplace(free, free[0] + c)
    return max(free)


def slices(tracks, slots, group):
    share = max(64, 4096 // group)
    return list_schedule([c[b::share].sum() for c in tracks for b in range(min(share, len(c)))], slots)


def stride(tracks, slots, group):
    c = np.concatenate(tracks)
    return max(c[w::slots].sum() for w in range(slots))


def queue(tracks, slots, group):
    return list_schedule(np.concatenate(tracks), slots)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--unvoiced', type=float, default=0.55, help='cost of an unvoiced pulse (a voiced one is 1)')
    ap.add_argument('--slots', type=int, default=1536, help='resident workgroups of the chip')
    ap.add_argument('--utterances', type=int, default=16, help='target tracks of a wave')
    a = ap.parse_args()
    tracks = [pulse_costs(make_utterance(seed=4321 + 2 * i, fs=FS, seconds=10.0, time_warp=1.1)[1], a.unvoiced)
              for i in range(a.utterances)]
    pulses = sum(len(c) for c in tracks)
    voiced = sum(int((c == 1.0).sum()) for c in tracks)
    ideal = sum(c.sum() for c in tracks) / a.slots
    print(f'{a.utterances} tracks, {pulses} pulses ({pulses / a.utterances:.0f} a track), {100.0 * voiced / pulses:.0f} % voiced; '
          f'unvoiced cost {a.unvoiced:g}, {a.slots} slots; ideal {ideal:.1f}')
    groups = [g for g in (4, 8, 16) if g <= a.utterances]
    print('| assignment | ' + ' | '.join(f'G = {g}' for g in groups) + ' |')
    print('|---|' + '---|' * len(groups))
    for name, fn in (('slices', slices), ('stride', stride), ('queue', queue)):
        row = [sum(fn(tracks[i:i + g], a.slots, g) for i in range(0, a.utterances, g)) for g in groups]
        print(f'| {name} | ' + ' | '.join(f'{v:.1f} ({100.0 * ideal / v:.0f} %)' for v in row) + ' |')


if __name__ == '__main__':
    main()
