#!/usr/bin/env python
"""Companion benchmark of the EM trajectory conversion over soft mixture posteriors (kwy_convert_mcep_em_batch_dev): the
time of ONE call for 16 mel-cepstrum matrices of 2001 x 25 at M = 64 mixtures with N = 0, 1 and 4 re-estimations,
beside kwy_convert_mcep_batch_dev (one arg-max mixture per frame) on the same inputs and model.

    python bench_em.py [--count 16] [--frames 2001] [--order 24] [--mixtures 64] [--iterations 0,1,4] [--repeats 5]

The mixture is tests/convert_cases.mixture(3 * order, mixtures, tag, spread=0.2): x-means so close together that
several mixtures share the posterior of a frame (the case the EM form is for); every matrix is a track that dwells near
the static part of one x-mean after the other (seeds 0 .. count - 1).  Device events around the call on the context's
stream, after a warm-up call per form; the kernels' own durations come from the context's per-kernel events
(kwy_ctx_profile) in a pass of its own per form.  For the E-step kernel the line reports 2 T M D^2 / time per launch --
the flop of forming all M conditional means of T frames -- beside the same figure for k_gmm_logp (whose triangular
factor takes about 58 / 90 of those multiplications at D = 72) from the same run, and the share of the f64 matrix peak
(`--f64-matrix-tflops`, default 78.6, the MI355X's specification).  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

KERNELS = ('k_gmm_logp', 'k_em_estep', 'k_mlpg_chunks', 'k_mlpg_finish')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--count', type=int, default=16)
    ap.add_argument('--frames', type=int, default=2001)
    ap.add_argument('--order', type=int, default=24)
    ap.add_argument('--mixtures', type=int, default=64)
    ap.add_argument('--iterations', type=str, default='0,1,4')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--tag', type=int, default=8)
    ap.add_argument('--f64-matrix-tflops', type=float, default=78.6)
    args = ap.parse_args()
    import torch
    import convert_cases as cc
    from kwiiyatta_amd import _lib
    lib = _lib.lib
    d, M, T, n = args.order, args.mixtures, args.frames, args.count
    D = 3 * d
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    w, mu, cov = cc.mixture(D, M, args.tag, spread=0.2)
    host = []
    for seed in range(n):
        rng = np.random.default_rng([seed, T, d, M])
        mc = np.empty((T, d + 1))
        mc[:, 0] = rng.standard_normal(T)
        mc[:, 1:] = mu[(np.arange(T) // 5 + seed) % M, :d] + 0.3 * rng.standard_normal((T, d))
        host.append(mc)
    rc, model = cc.prepare(ctx, d, w, mu, cov)
    assert rc == 0
    ins = [torch.from_numpy(m).to(dev) for m in host]
    outs = [torch.full_like(x, float('nan')) for x in ins]
    plain = _lib.job_array(_lib.ConvertJob, [(a, T, o) for a, o in zip(ins, outs)])
    em = _lib.job_array(_lib.ConvertEmJob, [(a, T, o, None) for a, o in zip(ins, outs)])
    torch.cuda.synchronize()
    vp = lambda jobs: ctypes.cast(jobs, ctypes.c_void_p)  # noqa: E731

    def call_plain():
        _lib.check(ctx, lib.kwy_convert_mcep_batch_dev(ctx.handle, vp(plain), n, d, M, model.data_ptr()))

    def call_em(N):
        return lambda: _lib.check(ctx, lib.kwy_convert_mcep_em_batch_dev(ctx.handle, vp(em), n, d, M, model.data_ptr(), N))

    flop = 2.0 * n * T * M * D * D                 # all M conditional means of every frame, once
    cases = []
    with torch.cuda.stream(stream):
        forms = [('argmax', None, call_plain)] + [(f'em{N}', N, call_em(N)) for N in map(int, args.iterations.split(','))]
        for name, N, call in forms:
            call()                                  # warm-up: code objects, the arena at its size
            ctx.sync()
            assert all(bool(torch.isfinite(o).all()) for o in outs), name
            times = []
            for _ in range(args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call()
                b.record(stream)
                b.synchronize()
                times.append(a.elapsed_time(b))
            ctx.profile(True)                       # the kernels' own durations, in a call of its own
            call()
            kernels = {k: ctx.profile_read(k) for k in KERNELS}
            ctx.profile(False)
            case = dict(form=name, em_iterations=N, call_ms=float(np.median(times)), call_ms_min=min(times),
                        call_ms_max=max(times),
                        kernels_ms={k: dict(total_ms=ms, launches=cnt) for k, (ms, cnt) in kernels.items() if cnt})
            for k in ('k_em_estep', 'k_gmm_logp'):
                ms, cnt = kernels[k]
                if cnt:
                    tflops = flop * cnt / (ms * 1e-3) / 1e12
                    case[f'{k}_tflops'] = tflops
                    case[f'{k}_share_of_f64_matrix_peak'] = tflops / args.f64_matrix_tflops
            cases.append(case)
    print(json.dumps({'metric': 'EM trajectory conversion, one batched call', 'unit': 'ms', 'higher_is_better': False,
                      'value': cases[-1]['call_ms'], 'matrices': n, 'frames': T, 'cols': d + 1, 'mixtures': M,
                      'spread': 0.2, 'repeats': args.repeats, 'dtype': 'f64', 'flop_per_estep': flop,
                      'f64_matrix_tflops': args.f64_matrix_tflops, 'cases': cases}))


if __name__ == '__main__':
    main()
