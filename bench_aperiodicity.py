#!/usr/bin/env python
"""Companion benchmark of the aperiodicity conversion (kwy_bap.hip): over 16 and over 256 aperiodicity matrices of
2000 x 1025 (ten-second utterances at 48 kHz, 5 bands) and a mixture of 16 components, the time of

    track          one kwy_bap_track_batch_dev call (the matrices read at the band centres, the tracks written)
    convert        kwy_convert_mcep_batch_dev over the tracks (d = 5, prepared model, calls of 16 utterances)
    apply          one kwy_bap_apply_batch_dev call (the voiced rows of every matrix rewritten)
    together       the three back to back
    codec_pair     kwy_code_aperiodicity_dev + kwy_decode_aperiodicity_dev looped over the same matrices: the existing
                   kernels that read and write the same bytes
    copy           torch.Tensor.copy_ of the block: the same bytes written (and read) once, the memory-bound yardstick

    python bench_aperiodicity.py [--counts 16,256] [--frames 2000] [--bins 1025] [--fs 48000] [--components 16]
                                 [--voiced 0.8] [--repeats 10] [--inner 3]

The matrices of a batch are consecutive views of one block, filled on the device from a seed: voiced rows
10 ** -uniform(0.5, 3), every fifth second unvoiced (1 - 1e-12).  Device events on the context's stream around `--inner`
back-to-back calls (job arrays built once, outside the window), `--repeats` windows per variant after a warm-up call
each; the variants alternate inside one loop.  Reported per variant: median, minimum and maximum time of one call;
for apply, codec_pair and copy also the achieved bytes/s at the median, counting the bytes written (8 * bins per frame
that is written; the copy reads as many).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def random_gmm(B, M, seed=0):
    """a well-conditioned joint mixture over 6 B dimensions on the dB scale"""
    rng = np.random.default_rng(seed)
    D2 = 6 * B
    means = np.zeros((M, D2))
    means[:, :B] = rng.uniform(-55.0, -8.0, (M, 1)) + rng.uniform(-2, 2, (M, B))
    means[:, 3 * B:4 * B] = means[:, :B] - 6.0
    a = rng.standard_normal((M, D2, D2)) * 0.5
    covs = a @ a.transpose(0, 2, 1) + np.eye(D2) * 6.0
    return np.full(M, 1.0 / M), means, covs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--counts', type=str, default='16,256')
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--bins', type=int, default=1025)
    ap.add_argument('--fs', type=int, default=48000)
    ap.add_argument('--components', type=int, default=16)
    ap.add_argument('--voiced', type=float, default=0.8)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--inner', type=int, default=3)
    args = ap.parse_args()
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    from kwiiyatta_amd.backend import bap
    from kwiiyatta_amd.pipeline import DeviceGMM
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    T, K, fs, M = args.frames, args.bins, args.fs, args.components
    fft_size, B = 2 * (K - 1), bap.check_rate(args.fs)
    f64 = dict(dtype=torch.float64, device=dev)
    cases = []
    with torch.cuda.stream(stream):
        gmm = DeviceGMM(*random_gmm(B, M), dev)
        model = gmm.model(diff=False)
    for count in (int(c) for c in args.counts.split(',')):
        with torch.cuda.stream(stream):
            gen = torch.Generator(device=dev).manual_seed(count)
            block = torch.pow(10.0, -(torch.rand((count * T, K), generator=gen, **f64) * 2.5 + 0.5))
            period = max(1, int(round(T / 10)))                      # a tenth of the utterance ...
            unvoiced = (torch.arange(count * T, device=dev) % period) >= int(period * args.voiced)
            block[unvoiced] = 1.0 - 1e-12                            # ... whose last fifth is unvoiced
            work, spare = block.clone(), torch.empty_like(block)
            src = torch.empty((count * T, B + 1), **f64)
            conv = torch.empty((count * T, B + 1), **f64)
            coded = torch.empty((count * T, B), **f64)
        views = lambda blk: [blk[i * T:(i + 1) * T] for i in range(count)]  # noqa: E731
        j_track = _lib.job_array(_lib.BapTrackJob, [(a, T, s) for a, s in zip(views(block), views(src))])
        j_conv = [_lib.job_array(_lib.ConvertJob, [(s, T, c) for s, c in list(zip(views(src), views(conv)))[g:g + 16]])
                  for g in range(0, count, 16)]
        j_apply = _lib.job_array(_lib.BapApplyJob, [(s, c, T, a) for s, c, a in zip(views(src), views(conv), views(work))])
        p = lambda t: t.data_ptr()  # noqa: E731
        chk = lambda rc: _lib.check(ctx, rc)  # noqa: E731
        torch.cuda.synchronize()

        def track():
            chk(lib.kwy_bap_track_batch_dev(ctx.handle, j_track, count, fs, fft_size))

        def convert():
            for jobs in j_conv:
                chk(lib.kwy_convert_mcep_batch_dev(ctx.handle, jobs, len(jobs), B, M, p(model)))

        def apply():
            chk(lib.kwy_bap_apply_batch_dev(ctx.handle, j_apply, count, fs, fft_size))

        def together():
            track(), convert(), apply()

        def codec_pair():
            for a, c, o in zip(views(block), views(coded), views(spare)):
                chk(lib.kwy_code_aperiodicity_dev(ctx.handle, p(a), T, fs, fft_size, p(c)))
                chk(lib.kwy_decode_aperiodicity_dev(ctx.handle, p(c), T, fs, fft_size, B, p(o)))

        variants = dict(track=track, convert=convert, apply=apply, together=together, codec_pair=codec_pair,
                        copy=lambda: spare.copy_(block))
        times = {name: [] for name in variants}
        with torch.cuda.stream(stream):
            for call in variants.values():                      # warm-up: code objects, the arena
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
            voiced_rows = int((src[:, 0] == 1.0).sum().item())
        written = dict(apply=8 * K * voiced_rows, codec_pair=8 * K * count * T, copy=8 * K * count * T)
        case = dict(matrices=count, voiced_rows=voiced_rows, rows=count * T)
        for name, ts in times.items():
            med = float(np.median(ts))
            case[name] = dict(call_ms=med, call_ms_min=min(ts), call_ms_max=max(ts))
            if name in written:
                case[name].update(bytes_written=written[name], tbytes_written_per_s=written[name] / med / 1e9)
        case['apply_over_copy'] = case['apply']['call_ms'] / case['copy']['call_ms']
        case['apply_over_codec_pair'] = case['apply']['call_ms'] / case['codec_pair']['call_ms']
        case['track_over_copy'] = case['track']['call_ms'] / case['copy']['call_ms']
        case['track_plus_apply_over_codec_pair'] = (case['track']['call_ms'] + case['apply']['call_ms']) / \
            case['codec_pair']['call_ms']
        case['together_over_copy'] = case['together']['call_ms'] / case['copy']['call_ms']
        cases.append(case)
        del block, work, spare, src, conv, coded
    print(json.dumps({'metric': 'aperiodicity conversion, track + convert + apply', 'unit': 'ms', 'higher_is_better': False,
                      'value': cases[-1]['together']['call_ms'], 'frames': T, 'bins': K, 'fs': fs, 'bands': B,
                      'components': M, 'repeats': args.repeats, 'inner': args.inner, 'dtype': 'f64', 'cases': cases}))


if __name__ == '__main__':
    main()
