#!/usr/bin/env python
"""Companion benchmark of the two differential filters: 16 and 256 signals of ten seconds at 48 kHz (order 24, 5 ms
frames) through the MLSA filter (kwy_mlsa_filter_batch_dev: one wavefront per signal, serial in the sample) and through
the frame-parallel FFT filter (kwy_mcep_filter_fft_batch_dev: one workgroup per frame) on the SAME inputs.

    python bench_difffilt.py [--counts 16,256] [--seconds 10] [--fs 48000] [--order 24] [--repeats 5]

The signals are noise, the mel-cepstra a slow random walk (the one of tests/test_mlsa_codec.py's speech test), both made
on the device from a seed.  Per filter and count: the whole call (device events on the context's stream around one
batched call, `--repeats` of them after a warm-up call, the two filters alternating; median, minimum and maximum) and,
from a profiled call of its own afterwards, the filter kernel's time per launch (k_mlsa_filter / k_fft_filter: HIP
events around every launch, a call over more than 64 signals makes several).  Also the RMS difference of the two
outputs over the RMS of the MLSA output: the model difference between interpolating coefficients and crossfading
outputs.  Nothing is asserted about the times.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', type=str, default='16,256')
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--fs', type=int, default=48000)
    ap.add_argument('--order', type=int, default=24)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    from kwiiyatta_amd.backend import fftfilt, sptk
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    fs, order = args.fs, args.order
    hop = int(fs * 0.005)
    n = int(args.seconds * fs)
    T = n // hop + 1
    size = fftfilt.fft_filter_size(fs, hop)
    alpha = sptk.mcepalpha(fs)
    cases = []
    for count in (int(c) for c in args.counts.split(',')):
        gen = torch.Generator(device=dev).manual_seed(count)
        x = torch.randn((count, n), dtype=torch.float64, device=dev, generator=gen) * 0.1
        walk = torch.cumsum(torch.randn((count, T, order), dtype=torch.float64, device=dev, generator=gen) * 0.02, dim=1)
        mc = torch.zeros((count, T, order + 1), dtype=torch.float64, device=dev)
        mc[:, :, 1:] = walk / torch.arange(1, order + 1, dtype=torch.float64, device=dev)
        y = {name: torch.empty_like(x) for name in ('mlsa', 'fft')}
        jobs = {name: _lib.job_array(_lib.MlsaJob, [(x[i], n, mc[i], T, y[name][i]) for i in range(count)]) for name in y}
        torch.cuda.synchronize()
        calls = {
            'mlsa': lambda: _lib.check(ctx, lib.kwy_mlsa_filter_batch_dev(ctx.handle, jobs['mlsa'], count, order, alpha, 4,
                                                                         hop, 1)),
            'fft': lambda: _lib.check(ctx, lib.kwy_mcep_filter_fft_batch_dev(ctx.handle, jobs['fft'], count, order, alpha,
                                                                            hop, size, 1)),
        }
        kernels = {'mlsa': 'k_mlsa_filter', 'fft': 'k_fft_filter'}
        times = {name: [] for name in calls}
        with torch.cuda.stream(stream):
            for call in calls.values():                         # warm-up: code objects, tables, the scratch arena
                call()
            stream.synchronize()
            for _ in range(args.repeats):
                for name, call in calls.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    call()
                    b.record(stream)
                    b.synchronize()
                    times[name].append(a.elapsed_time(b))
            ctx.profile(True)
            kernel = {}
            for name, call in calls.items():
                ctx.profile_read(kernels[name])
                call()
                ms, launches = ctx.profile_read(kernels[name])
                kernel[name] = dict(launches=launches, launch_ms=ms / launches, kernel_ms=ms)
            ctx.profile(False)
        d = y['fft'] - y['mlsa']
        assert bool(torch.isfinite(d).all())
        case = dict(signals=count, samples=n, frames=T,
                    rms_difference_over_rms=float(torch.sqrt(torch.mean(d * d)) / torch.sqrt(torch.mean(y['mlsa'] ** 2))))
        for name, ts in times.items():
            case[name] = dict(call_ms=float(np.median(ts)), call_ms_min=min(ts), call_ms_max=max(ts), **kernel[name])
        case['mlsa_over_fft'] = case['mlsa']['call_ms'] / case['fft']['call_ms']
        cases.append(case)
        del x, walk, mc, y, d
    print(json.dumps({'metric': 'differential filter, one batched call, frame-parallel FFT form', 'unit': 'ms',
                      'higher_is_better': False, 'value': cases[-1]['fft']['call_ms'], 'fs': fs, 'order': order,
                      'hopsize': hop, 'fft_size': size, 'seconds': args.seconds, 'repeats': args.repeats, 'dtype': 'f64',
                      'cases': cases}))


if __name__ == '__main__':
    main()
