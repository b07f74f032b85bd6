#!/usr/bin/env python
"""Companion benchmark of the waveform pitch shifter (kwy_pitch_shift_batch_dev): the time of ONE call for 16 and for
256 ten-second 48 kHz utterances of kwiiyatta_amd.synthetic.make_utterance.

    python bench_pitch.py [--rate R] [--counts 16,256] [--seconds 10] [--repeats 5]

Device events around the call on the context's stream, after a warm-up call per batch size; the two kernels' own
durations come from the context's per-kernel events (kwy_ctx_profile) in a pass of its own, and from
`rocprofv3 --kernel-trace --stats -- python bench_pitch.py` when traced.  16 distinct utterances are generated (seeds
0..15); a larger batch reads them again in turn (every job writes an output of its own), which keeps the host out of
the way and changes nothing a chain does.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rate', type=float, default=1.4983, help='pitch ratio (default: a fifth up)')
    ap.add_argument('--counts', type=str, default='16,256')
    ap.add_argument('--fs', type=int, default=48000)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--distinct', type=int, default=16, help='utterances generated; larger batches reuse them')
    args = ap.parse_args()
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import pitch
    from kwiiyatta_amd.synthetic import make_utterance
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    base = [torch.from_numpy(make_utterance(seed=s, fs=args.fs, seconds=args.seconds)[0]).to(dev)
            for s in range(args.distinct)]
    n = base[0].numel()
    steps = pitch.frames(n, args.fs, args.rate) - 1
    H = int(args.fs * 0.010)
    cases = []
    for count in (int(c) for c in args.counts.split(',')):
        xs = [base[i % len(base)] for i in range(count)]
        ys = [torch.empty_like(x) for x in xs]
        torch.cuda.synchronize()

        def call():
            pitch.shift_pitch_batch_dev(ctx, xs, ys, args.fs, args.rate)
        with torch.cuda.stream(stream):
            call()                                      # warm-up: code objects, the arena
            ctx.sync()
            times = []
            for _ in range(args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call()
                b.record(stream)
                b.synchronize()
                times.append(a.elapsed_time(b))
            ctx.profile(True)                           # the kernels' own durations, in a call of its own
            call()
            chain_ms, _ = ctx.profile_read('k_pitch_positions')
            resample_ms, _ = ctx.profile_read('k_pitch_resample')
            ctx.profile(False)
        cases.append(dict(utterances=count, call_ms=float(np.median(times)), call_ms_min=min(times), call_ms_max=max(times),
                          k_pitch_positions_ms=chain_ms, k_pitch_resample_ms=resample_ms,
                          chain_step_us=1e3 * chain_ms / steps,
                          ms_per_utterance=float(np.median(times)) / count))
    print(json.dumps({'metric': 'waveform pitch shift, one batched call', 'unit': 'ms', 'higher_is_better': False,
                      'value': cases[-1]['call_ms'], 'fs': args.fs, 'seconds': args.seconds, 'rate': args.rate,
                      'samples': n, 'chain_steps': steps, 'candidates_per_step': 2 * H + 1, 'terms_per_candidate': 2 * H,
                      'repeats': args.repeats, 'dtype': 'f64', 'cases': cases}))


if __name__ == '__main__':
    main()
