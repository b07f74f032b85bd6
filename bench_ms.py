#!/usr/bin/env python
"""Companion benchmark of the modulation-spectrum postfilter (kwy_ms_postfilter_batch_dev): the time of ONE call for 16
and for 256 mel-cepstrum matrices of 2000 x 25 at L = 4096, beside kwy_gv_postfilter_batch_dev (with its moments
call) on the same input and the time the bytes moved would take at the HBM rate.

    python bench_ms.py [--counts 16,256] [--frames 2000] [--cols 25] [--length 4096] [--repeats 5]

Device events around the call on the context's stream, after a warm-up call per batch size (the call includes the
host's work of describing the jobs, which a stream of short kernels does not hide); the kernels' own durations come
from the context's per-kernel events (kwy_ctx_profile) in a pass of its own.  16 distinct matrices are
generated (seeds 0..15: a random walk per coefficient, which has the red spectrum of a converted trajectory); a
larger batch reads them again in turn (every job writes an output of its own).  The statistics are those of the
matrices themselves (G) and of their first differences rescaled (N), so the gains stay finite.  The floor counts
every matrix read once and written once, 2 * 8 * frames * cols bytes per matrix, at `--hbm-tbps` (default 6.29, a
measured copy rate of the MI355X; its specification says 8.0).  Prints one JSON line."""
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
    ap.add_argument('--cols', type=int, default=25)
    ap.add_argument('--length', type=int, default=4096)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--distinct', type=int, default=16, help='matrices generated; larger batches reuse them')
    ap.add_argument('--hbm-tbps', type=float, default=6.29)
    args = ap.parse_args()
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import gv, ms
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    host = [np.ascontiguousarray(np.cumsum(np.random.RandomState(s).standard_normal((args.frames, args.cols)), axis=0))
            for s in range(args.distinct)]
    stats_g = ms.statistics(host, args.length)
    stats_n = ms.statistics([np.ascontiguousarray(np.diff(m, axis=0, prepend=0.0) * 8.0) for m in host], args.length)
    gv_stat = gv.gv_from_moments(gv.column_moments(host)) * 1.5
    base = [torch.from_numpy(m).to(dev) for m in host]
    d_g, d_n, d_gv = (torch.from_numpy(a).to(dev) for a in (stats_g, stats_n, gv_stat))
    cases = []
    for count in (int(c) for c in args.counts.split(',')):
        xs = [base[i % len(base)] for i in range(count)]
        outs = [torch.empty_like(x) for x in xs]
        status = torch.zeros(count, dtype=torch.int32, device=dev)
        moments = torch.empty((count, args.cols, 3), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def call_ms():
            ms.postfilter_batch_dev(ctx, xs, d_g, d_n, 1.0, outs, status=status)

        def call_gv():
            gv.column_moments_batch_dev(ctx, xs, moments)
            gv.postfilter_batch_dev(ctx, xs, moments, d_gv, 1.0, outs, status=status)
        timed = {}
        with torch.cuda.stream(stream):
            for name, call in (('ms', call_ms), ('gv', call_gv)):
                call()                                      # warm-up: code objects, twiddle tables
                ctx.sync()
                times = []
                for _ in range(args.repeats):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    call()
                    b.record(stream)
                    b.synchronize()
                    times.append(a.elapsed_time(b))
                timed[name] = times
                assert not status.cpu().numpy().any(), name
            ctx.profile(True)                               # the kernels' own durations, in a call of its own each
            call_ms()
            kernel_ms, launches = ctx.profile_read('k_ms_filter')
            call_gv()
            gv_kernels_ms = ctx.profile_read('k_gv_moments')[0] + ctx.profile_read('k_gv_apply')[0]
            ctx.profile(False)
        moved = 2 * 8 * args.frames * args.cols * count
        cases.append(dict(matrices=count, call_ms=float(np.median(timed['ms'])), call_ms_min=min(timed['ms']),
                          call_ms_max=max(timed['ms']), k_ms_filter_ms=kernel_ms, k_ms_filter_launches=launches,
                          gv_kernels_ms=gv_kernels_ms, gv_call_ms=float(np.median(timed['gv'])),
                          gv_call_ms_min=min(timed['gv']), gv_call_ms_max=max(timed['gv']), bytes_moved=moved,
                          hbm_floor_ms=1e3 * moved / (args.hbm_tbps * 1e12),
                          us_per_column=1e3 * kernel_ms / (count * (args.cols - 1))))
    print(json.dumps({'metric': 'modulation-spectrum postfilter, one batched call', 'unit': 'ms',
                      'higher_is_better': False, 'value': cases[-1]['call_ms'], 'frames': args.frames, 'cols': args.cols,
                      'length': args.length, 'repeats': args.repeats, 'hbm_tbps': args.hbm_tbps, 'dtype': 'f64',
                      'cases': cases}))


if __name__ == '__main__':
    main()
