#!/usr/bin/env python
"""Companion benchmark of the formant shift (kwy_formant_shift_batch_dev): the time of ONE call over 16 and over 256
envelope matrices of 2000 x 1025 (ten-second utterances at 48 kHz), out of place and in place, and of one
kwy_formant_shift_dev call over the same rows as a single matrix (what ConvertWave makes), beside a plain device copy
of the same bytes (torch.Tensor.copy_ of the block) as the yardstick.

    python bench_formant.py [--counts 16,256] [--frames 2000] [--bins 1025] [--semitones 3] [--repeats 10] [--inner 10]

The matrices of a batch are consecutive views of one block, filled on the device with exp(uniform(-30, 2)) from a
seed.  Device events on the context's stream around `--inner` back-to-back calls (the job arrays are built once, outside
the window), `--repeats` windows per variant after a warm-up call each; the variants alternate inside one loop, so that
whatever else the machine does hits them alike.  Reported per variant: the median, minimum and maximum time of one
call and the achieved bytes/s at the median, counting every value read once and written once (2 * 8 * frames * bins
bytes per matrix) -- for the copy as well.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', type=str, default='16,256')
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--bins', type=int, default=1025)
    ap.add_argument('--semitones', type=float, default=3.0)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--inner', type=int, default=10)
    args = ap.parse_args()
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    from kwiiyatta_amd.backend import formant
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    ratio = formant.semitone_ratio(args.semitones)
    T, K = args.frames, args.bins
    cases = []
    for count in (int(c) for c in args.counts.split(',')):
        gen = torch.Generator(device=dev).manual_seed(count)
        src = torch.exp(torch.rand((count * T, K), dtype=torch.float64, device=dev, generator=gen) * 32.0 - 30.0)
        dst, work = torch.empty_like(src), src.clone()
        status = torch.zeros(count, dtype=torch.int32, device=dev)
        views = lambda block: [block[i * T:(i + 1) * T] for i in range(count)]  # noqa: E731
        j_out = _lib.job_array(_lib.FormantJob, [(a, T, o) for a, o in zip(views(src), views(dst))])
        j_in = _lib.job_array(_lib.FormantJob, [(a, T, a) for a in views(work)])
        torch.cuda.synchronize()

        def batch(jobs):
            return lambda: _lib.check(ctx, lib.kwy_formant_shift_batch_dev(ctx.handle, jobs, count, K, ratio,
                                                                           status.data_ptr()))
        variants = {
            'out_of_place': batch(j_out),
            'in_place': batch(j_in),
            'one_matrix_in_place': lambda: _lib.check(ctx, lib.kwy_formant_shift_dev(
                ctx.handle, work.data_ptr(), count * T, K, ratio, work.data_ptr(), status.data_ptr())),
            'copy': lambda: dst.copy_(src),
        }
        times = {name: [] for name in variants}
        with torch.cuda.stream(stream):
            for call in variants.values():                      # warm-up: code objects
                call()
            stream.synchronize()
            for _ in range(args.repeats):
                for name, call in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    for _ in range(args.inner):
                        call()
                    b.record(stream)
                    b.synchronize()
                    times[name].append(a.elapsed_time(b) / args.inner)
            assert not status.cpu().numpy().any()
        moved = 2 * 8 * T * K * count
        case = dict(matrices=count, bytes_moved=moved)
        for name, ts in times.items():
            med = float(np.median(ts))
            case[name] = dict(call_ms=med, call_ms_min=min(ts), call_ms_max=max(ts), tbytes_per_s=moved / med / 1e9)
        case['out_of_place_over_copy'] = case['out_of_place']['call_ms'] / case['copy']['call_ms']
        case['in_place_over_copy'] = case['in_place']['call_ms'] / case['copy']['call_ms']
        cases.append(case)
        del src, dst, work
    print(json.dumps({'metric': 'formant shift, one batched call out of place', 'unit': 'ms', 'higher_is_better': False,
                      'value': cases[-1]['out_of_place']['call_ms'], 'frames': T, 'bins': K, 'ratio': ratio,
                      'repeats': args.repeats, 'inner': args.inner, 'dtype': 'f64', 'cases': cases}))


if __name__ == '__main__':
    main()
