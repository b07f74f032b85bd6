#!/usr/bin/env python
"""Companion benchmark of the mel-cepstral energy kernels (kwy_mcpower.hip): the time of ONE call over 16 and over 256
mel-cepstrum matrices of 2000 x 25 (ten-second utterances at 48 kHz, N = 2048) of

    filter          kwy_mcep_postfilter_batch_dev, beta 0.3 with a reference (formant emphasis + power-preserving c0)
    keep_power      the same call at beta 0 (the c0 shift alone)
    energy          kwy_mcep_energy_batch_dev
    mc2sp_reduce    kwy_mc2sp_dev of the same rows (2000 x 1025 doubles written per matrix) and a row reduction of the
                    spectrum (torch.sum along the bins): the form the energy kernel avoids
    mc2sp           the kwy_mc2sp_dev call of that variant alone
    copy            a plain device copy of the matrices' bytes (torch.Tensor.copy_), the yardstick of a launch

    python bench_power.py [--counts 16,256] [--frames 2000] [--order 24] [--fft-size 2048] [--repeats 10] [--inner 10]

The matrices of a batch are consecutive views of one block, filled on the device from a seed with coefficients that
decay like speech.  Device events on the context's stream around `--inner` back-to-back calls (the job arrays are built
once, outside the window), `--repeats` windows per variant after a warm-up call each; the variants alternate inside one
loop, so that whatever else the machine does hits them alike.  Reported per variant: the median, minimum and maximum
time of one call.  Prints one JSON line."""
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
    ap.add_argument('--order', type=int, default=24)
    ap.add_argument('--fft-size', type=int, default=2048)
    ap.add_argument('--alpha', type=float, default=0.554)
    ap.add_argument('--beta', type=float, default=0.3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--inner', type=int, default=10)
    args = ap.parse_args()
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    T, cols, N, alpha = args.frames, args.order + 1, args.fft_size, args.alpha
    K = N // 2 + 1
    cases = []
    for count in (int(c) for c in args.counts.split(',')):
        gen = torch.Generator(device=dev).manual_seed(count)
        scale = torch.cat((torch.ones(1, dtype=torch.float64),
                           1.5 / (1.0 + torch.arange(args.order, dtype=torch.float64)) ** 0.9)).to(dev)

        def block():
            m = torch.randn((count * T, cols), dtype=torch.float64, device=dev, generator=gen) * scale
            m[:, 0] -= 8.0
            return m
        src, ref = block(), block()
        dst = torch.empty_like(src)
        energy = torch.empty(count * T, dtype=torch.float64, device=dev)
        sp = torch.empty((count * T, K), dtype=torch.float64, device=dev)
        status = torch.zeros(count, dtype=torch.int32, device=dev)
        views = lambda b: [b[i * T:(i + 1) * T] for i in range(count)]  # noqa: E731
        j_filter = _lib.job_array(_lib.McPowerJob, [(x, r, None, o, T)
                                                    for x, r, o in zip(views(src), views(ref), views(dst))])
        j_energy = _lib.job_array(_lib.EnergyJob, [(x, T, e) for x, e in zip(views(src), views(energy))])
        torch.cuda.synchronize()

        def filt(beta):
            return lambda: _lib.check(ctx, lib.kwy_mcep_postfilter_batch_dev(
                ctx.handle, j_filter, count, args.order, alpha, N, beta, status.data_ptr()))

        def mc2sp():
            _lib.check(ctx, lib.kwy_mc2sp_dev(ctx.handle, src.data_ptr(), count * T, args.order, alpha, N, sp.data_ptr()))

        def mc2sp_reduce():
            mc2sp()
            torch.sum(sp, dim=1, out=energy)
        variants = {
            'filter': filt(args.beta),
            'keep_power': filt(0.0),
            'energy': lambda: _lib.check(ctx, lib.kwy_mcep_energy_batch_dev(ctx.handle, j_energy, count, args.order, alpha,
                                                                           N)),
            'mc2sp_reduce': mc2sp_reduce,
            'mc2sp': mc2sp,
            'copy': lambda: dst.copy_(src),
        }
        times = {name: [] for name in variants}
        with torch.cuda.stream(stream):
            for call in variants.values():                      # warm-up: code objects, the cosine table
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
        case = dict(matrices=count, matrix_bytes=8 * T * cols * count, spectrum_bytes=8 * T * K * count)
        for name, ts in times.items():
            case[name] = dict(call_ms=float(np.median(ts)), call_ms_min=min(ts), call_ms_max=max(ts))
        case['filter_over_copy'] = case['filter']['call_ms'] / case['copy']['call_ms']
        case['mc2sp_reduce_over_energy'] = case['mc2sp_reduce']['call_ms'] / case['energy']['call_ms']
        cases.append(case)
        del src, ref, dst, sp, energy
    print(json.dumps({'metric': 'mel-cepstral postfilter with power correction, one batched call', 'unit': 'ms',
                      'higher_is_better': False, 'value': cases[-1]['filter']['call_ms'], 'frames': T,
                      'order': args.order, 'fft_size': N, 'alpha': alpha, 'beta': args.beta, 'repeats': args.repeats,
                      'inner': args.inner, 'dtype': 'f64', 'cases': cases}))


if __name__ == '__main__':
    main()
