#!/usr/bin/env python
"""The nearest-neighbour search of non-parallel training (--nonparallel) beside its yardsticks.

    python bench_nonparallel.py [--sizes 32000 512000] [--dim 49] [--runs 20] [--warmup 3]

Timed on one GPU, each figure the median of --runs runs after --warmup untimed ones, wall clock around the enqueue
and the synchronisation of the context's stream (the shortest figure here is milliseconds):

    search     kwy_nn_search_dev at nq = nc = size, D = --dim, on N(0, 1) rows: 2 nq nc D flop
    km_assign  kwy_km_assign_dev at M = 256 on the same rows, in the same process: the same arithmetic with its B operand
               resident in LDS, 2 n 256 D flop -- the yardstick of the flop rate
    cdist      torch.cdist + argmin in float64 on the device, in chunks of queries that keep the distance block under
               --cdist-bytes

    inca       one full INCA iteration of corpus.train_converter_nonparallel (conversion of the source, delta features,
               two searches, gather, monitor read-back, fit from scratch) on --inca-utterances synthetic utterances of
               --inca-seconds a side at 48 kHz (16 of 10 s: 2 001 frames each), --inca-components components: the
               median over fits 1 .. --runs of one training (fit 0 converts nothing and is reported beside it), after
               an untimed training of one iteration (every training analyses the two sides again)

Prints ONE JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


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
    ap.add_argument('--sizes', type=int, nargs='+', default=[32000, 512000])
    ap.add_argument('--dim', type=int, default=49)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cdist-bytes', type=int, default=1 << 31)
    ap.add_argument('--cdist-runs', type=int, default=None, help='runs of the cdist leg (default: --runs)')
    ap.add_argument('--no-cdist', action='store_true')
    ap.add_argument('--no-inca', action='store_true')
    ap.add_argument('--inca-utterances', type=int, default=16)
    ap.add_argument('--inca-seconds', type=float, default=10.0)
    ap.add_argument('--inca-components', type=int, default=64)
    args = ap.parse_args()
    pairs = []
    if not args.no_inca:          # made by a pool of host processes before the GPU is touched
        import concurrent.futures as cf
        import multiprocessing as mp
        from bench_corpus import _make_pair_job
        nproc = max(1, min(len(os.sched_getaffinity(0)), 16, args.inca_utterances))
        with cf.ProcessPoolExecutor(nproc, mp_context=mp.get_context('spawn')) as ex:
            pairs = list(ex.map(_make_pair_job, [(k, args.inca_seconds, 48000) for k in range(args.inca_utterances)]))
    import torch
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import nn
    ctx = _lib.Context(0)
    D = args.dim
    out = {}
    for n in args.sizes:
        g = torch.Generator(device=dev).manual_seed(n)
        Q = torch.randn((n, D), dtype=torch.float64, device=dev, generator=g)
        C = torch.randn((n, D), dtype=torch.float64, device=dev, generator=g)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        dist2 = torch.empty(n, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        labels = torch.zeros(n, dtype=torch.int32, device=dev)
        changed = torch.zeros(1, dtype=torch.int64, device=dev)
        centers = C[:256].contiguous()
        torch.cuda.synchronize()
        _lib.check(ctx, _lib.lib.kwy_ctx_reserve(ctx.handle, max(nn.scratch_bytes(n), 2 * 4 * n * 12 + (1 << 20))))

        def search():
            nn.nearest_dev(ctx, Q, C, idx, dist2, status)

        def assign():
            _lib.check(ctx, _lib.lib.kwy_km_assign_dev(ctx.handle, Q.data_ptr(), n, D, centers.data_ptr(), 256,
                                                      labels.data_ptr(), None, changed.data_ptr()))

        t_s = median_seconds(search, ctx.sync, args.runs, args.warmup)
        t_a = median_seconds(assign, ctx.sync, args.runs, args.warmup)
        flop_s, flop_a = 2.0 * n * n * D, 2.0 * n * 256 * D
        rec = {'search_seconds': t_s[0], 'search_min_max': t_s[1:], 'search_flops': flop_s / t_s[0],
               'km_assign_seconds': t_a[0], 'km_assign_min_max': t_a[1:], 'km_assign_flops': flop_a / t_a[0],
               'search_over_km_assign_rate': (flop_s / t_s[0]) / (flop_a / t_a[0]), 'no_finite_score': int(status.item())}
        if not args.no_cdist:
            rows = max(1, min(n, args.cdist_bytes // (8 * n)))
            ref = torch.empty(n, dtype=torch.int64, device=dev)

            def cdist():
                for t0 in range(0, n, rows):
                    ref[t0:t0 + rows] = torch.cdist(Q[t0:t0 + rows], C).argmin(dim=1)

            t_c = median_seconds(cdist, torch.cuda.synchronize, args.cdist_runs or args.runs, min(args.warmup, 1))
            rec.update(cdist_seconds=t_c[0], cdist_min_max=t_c[1:], cdist_chunk_rows=rows,
                       cdist_over_search=t_c[0] / t_s[0], index_mismatches=int((ref != idx.long()).sum().item()))
        out[str(n)] = rec
        del Q, C, idx, dist2, labels
    if pairs:
        from kwiiyatta_amd import corpus as cp
        source, target = [p[0] for p in pairs], [p[1] for p in pairs][::-1]     # (nothing pairs them)
        ls = cp._Lockstep(0)
        how = dict(components=args.inca_components, seed=0, lockstep=ls)
        t0 = time.perf_counter()
        cp.train_converter_nonparallel(source, target, 48000, iterations=1, **how)
        warm = time.perf_counter() - t0
        _, history = cp.train_converter_nonparallel(source, target, 48000, iterations=args.runs, **how)
        later = [r['seconds'] for r in history[1:]]
        out['inca'] = {'utterances_a_side': len(pairs), 'rows': history[0]['rows'], 'components': args.inca_components,
                       'iteration_seconds': statistics.median(later), 'iteration_min_max': (min(later), max(later)),
                       'fit0_seconds': history[0]['seconds'], 'iterations_timed': len(later),
                       'em_iterations': [r['em_iterations'] for r in history],
                       'first_training_of_one_iteration_seconds': warm,
                       'monitor_db': [r['mcd'] for r in history]}
    last = out[str(args.sizes[-1])]
    print(json.dumps({'metric': f'seconds, nearest-neighbour search at nq = nc = {args.sizes[-1]}, D = {D}, float64',
                      'value': last['search_seconds'], 'unit': 's', 'n_gpus': 1,
                      'detail': {'dim': D, 'runs': args.runs, 'warmup': args.warmup, 'sizes': out}}))


if __name__ == '__main__':
    main()
