#!/usr/bin/env python
"""The two f0 estimators side by side: pYIN + StoneMask against DIO + StoneMask.

    python bench_f0.py [--utterances 16 256] [--seconds 10] [--fs 48000] [--runs 20] [--warmup 3] [--out profiles/f0_bench.json]

Timed on one GPU, in one process, on the same synthetic utterances (kwiiyatta_amd.synthetic.make_utterance, resident on
the device): each figure the median of --runs runs after --warmup untimed ones, wall clock around the enqueue of
`pyin_batch_dev` (or `dio_batch_dev`) + `stonemask_batch_dev` in groups of 16 utterances and the synchronisation of the
context's stream.  There is no target time: DIO's stage is the yardstick, and the ratio is reported whichever way it
falls.  The per-kernel split comes from one more, untimed pass with the library's event timing on
(kwy_ctx_profile).

Prints ONE JSON line and, with --out, writes it to that file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

KERNELS = {'pyin': ('k_pyin_observe', 'k_pyin_decode', 'k_stonemask'),
           'dio': ('k_dio_filter', 'k_dio_zc', 'k_dio_candidates', 'k_dio_fix', 'k_stonemask')}


def median_seconds(run, sync, runs, warmup):
    for _ in range(warmup):
        run()
    sync()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        run()
        sync()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utterances', type=int, nargs='+', default=[16, 256])
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--fs', type=int, default=48000)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--shapes', type=int, default=8, help='distinct synthetic utterances (repeated up to the count)')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import pyin, world
    from kwiiyatta_amd.synthetic import make_utterance
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    ctx = _lib.Context(0)
    fs = args.fs
    base = [torch.from_numpy(np.ascontiguousarray(make_utterance(seed=k, fs=fs, seconds=args.seconds)[0])).to(dev)
            for k in range(args.shapes)]
    out = {}
    for count in args.utterances:
        xs = [base[k % len(base)] for k in range(count)]
        T = [world.dio_frames(fs, x.numel()) for x in xs]
        t, coarse, f0 = ([torch.empty(n, dtype=torch.float64, device=dev) for n in T] for _ in range(3))
        status = torch.zeros(count, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        _lib.check(ctx, _lib.lib.kwy_ctx_reserve(ctx.handle, pyin.scratch_bytes(max(T), pyin.bins(), 16) + (1 << 20)))

        def stage(coarse_track):
            def run():
                for g in range(0, count, 16):
                    sl = slice(g, g + 16)
                    coarse_track(ctx, xs[sl], fs, t[sl], coarse[sl], status=status[sl])
                    world.stonemask_batch_dev(ctx, xs[sl], t[sl], coarse[sl], fs, f0[sl])
            return run

        rec = {}
        for name, fn in (('dio', world.dio_batch_dev), ('pyin', world.pyin_batch_dev)):
            run = stage(fn)
            med, lo, hi = median_seconds(run, ctx.sync, args.runs, args.warmup)
            voiced = float(sum((v > 0).sum().item() for v in f0)) / float(sum(T))
            ctx.profile(True)
            run()
            split = {k: ctx.profile_read(k)[0] / 1000.0 for k in KERNELS[name]}
            ctx.profile(False)
            rec[name] = {'seconds': med, 'min_max': (lo, hi), 'voiced_share': voiced, 'kernel_seconds': split,
                         'status_words_set': int(status.sum().item())}
        rec['pyin_over_dio'] = rec['pyin']['seconds'] / rec['dio']['seconds']
        rec['frames'] = int(sum(T))
        out[str(count)] = rec
    last = out[str(args.utterances[-1])]
    line = json.dumps({'metric': f'seconds, pYIN + StoneMask of {args.utterances[-1]} utterances of {args.seconds:g} s at '
                                 f'{fs} Hz (DIO + StoneMask beside it)',
                       'value': last['pyin']['seconds'], 'unit': 's', 'n_gpus': 1,
                       'detail': {'fs': fs, 'seconds': args.seconds, 'runs': args.runs, 'warmup': args.warmup,
                                  'utterances': out}})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
