#!/usr/bin/env python
"""One re-alignment pass of the training set (--align-iterations) on bench_corpus.py's corpus, beside what it avoids.

    python bench_realign.py [--pairs 503] [--seconds 5] [--components 64] [--em-iters 10] [--passes 2]

The corpus is bench_corpus.py's (synthetic 48 kHz pairs, every pair its own pitch, formant shift and time warp, made
on the host before the GPU is touched).  Timed on one GPU, in this order:

    matrix     build_training_matrix(keep=True): analysis + first alignment of every pair -- bench_corpus.py's data-set
               phase with the alignment inputs kept (TrainCache).  This is what a second alignment would cost again if
               nothing were kept: the re-analysis a pass avoids
    fit        the converter fit on its rows (--em-iters EM iterations, as bench_corpus.py --em-iters)
    realign    realign_training_matrix on the cache with that mixture, --passes times: conversion of every source into
               its DTW features, FastDTW, joint rows, monitor; the median pass is the figure

Prints ONE JSON line.  --profile adds the summed HIP-event times of the tracked kernels of one more, untimed pass."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from bench_corpus import _make_pair_job  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=503)
    ap.add_argument('--seconds', type=float, default=5.0)
    ap.add_argument('--components', type=int, default=64)
    ap.add_argument('--em-iters', type=int, default=10, help='exactly this many EM iterations (tol = 0)')
    ap.add_argument('--passes', type=int, default=2, help='timed re-alignment passes (each with the same mixture)')
    ap.add_argument('--profile', action='store_true', help='HIP events around the tracked kernels of one more pass')
    args = ap.parse_args()
    fs = 48000
    import concurrent.futures as cf
    import multiprocessing as mp
    nproc = max(1, min(len(os.sched_getaffinity(0)), 16, args.pairs))
    with cf.ProcessPoolExecutor(nproc, mp_context=mp.get_context('spawn')) as ex:
        pairs = list(ex.map(_make_pair_job, [(k, args.seconds, fs) for k in range(args.pairs)], chunksize=2))
    import torch
    torch.cuda.set_device(0)
    from kwiiyatta_amd import corpus as cp
    from kwiiyatta_amd.backend.nprandom import DeviceRandomState
    from kwiiyatta_amd.converter.gmm_fit import GaussianMixtureHIP
    ls = cp._Lockstep(0)
    fit = dict(n_components=args.components, max_iter=args.em_iters, tol=0.0, random_state=0, device_index=0)

    # warm-up of every phase on one wave: tables, arenas, kernel attributes, the generator's jump polynomials
    X, _, cache = cp.build_training_matrix(pairs[:16], fs, rng=DeviceRandomState.from_seed(1), lockstep=ls, keep=True)
    g = GaussianMixtureHIP(**dict(fit, max_iter=1)).fit(X)
    cp.realign_training_matrix(cache, g)
    del X, cache
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    X, frames, cache = cp.build_training_matrix(pairs, fs, rng=DeviceRandomState.from_seed(1234), lockstep=ls, keep=True)
    torch.cuda.synchronize()
    t_matrix = time.perf_counter() - t0
    t0 = time.perf_counter()
    g = GaussianMixtureHIP(**fit).fit(X)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    rows0 = int(X.shape[0])
    times, kernels = [], None
    for _ in range(max(1, args.passes)):
        t0 = time.perf_counter()
        X1, mcd = cp.realign_training_matrix(cache, g)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    if args.profile:              # one more pass, not timed: the events serialise the launches
        ls.ctx.profile(True)
        cp.realign_training_matrix(cache, g)
        kernels = {}
        for name in ('k_gmm_logp', 'k_mlpg_chunks', 'k_mlpg_finish', 'k_eval_mcd'):
            ms, n = ls.ctx.profile_read(name)
            if n:
                kernels[name] = {'total_ms': ms, 'launches': n}
        ls.ctx.profile(False)
    t_pass = statistics.median(times)
    monitor0 = cache.monitor.tolist()
    print(json.dumps({
        'metric': 'seconds, one re-alignment pass of the training set beside the analysis it avoids, 48 kHz 5 ms hop',
        'value': t_pass, 'unit': 's', 'n_gpus': 1,
        'detail': {'pairs': args.pairs, 'seconds_per_utterance': args.seconds, 'components': args.components,
                   'em_iters': args.em_iters, 'source_frames': int(frames), 'padded_frames': int(cache.frames),
                   'cache_bytes': int(cache.nbytes), 'matrix_seconds': t_matrix, 'fit_seconds': t_fit,
                   'realign_seconds': times, 'realign_over_matrix': t_pass / t_matrix,
                   'rows_first_alignment': rows0, 'rows_realigned': int(X1.shape[0]),
                   'monitor_first_db': monitor0[0] / monitor0[1] if monitor0[1] else None, 'monitor_realigned_db': mcd,
                   'kernels': kernels}}))


if __name__ == '__main__':
    main()
