#!/usr/bin/env python
"""Companion benchmark of the GV-considering trajectory generation (kwy_convert_mcep_gv_batch_dev): the time of ONE call
for 16 mel-cepstrum matrices of 2001 x 25 at M = 64 mixtures with gv_iterations = 0, 16 and 64 behind the arg-max
conversion, beside kwy_convert_mcep_batch_dev on the same inputs and model.

    python bench_gvgen.py [--count 16] [--frames 2001] [--order 24] [--mixtures 64] [--iterations 0,16,64] [--repeats 5]

Mixture and matrices are bench_em.py's (tests/convert_cases.mixture(3 * order, mixtures, tag, spread=0.2); tracks that
dwell near one x-mean after the other, seeds 0 .. count - 1).  The GV statistics are those of the inputs' own c1..cd:
mean and variance over the matrices of the per-matrix variance, so the over-smoothed trajectories are pulled towards the
variance of the tracks they were converted from.  Device events around the call on the context's stream, after a
warm-up call per form; the ascent kernel's own duration comes from the context's per-kernel events (kwy_ctx_profile) in
a pass of its own per form, beside k_mlpg_chunks + k_mlpg_finish -- one partitioned solve -- of the same run; the line
reports the ascent's time per iteration over that solve's.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

KERNELS = ('k_gv_ascent', 'k_mlpg_chunks', 'k_mlpg_finish')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--count', type=int, default=16)
    ap.add_argument('--frames', type=int, default=2001)
    ap.add_argument('--order', type=int, default=24)
    ap.add_argument('--mixtures', type=int, default=64)
    ap.add_argument('--iterations', type=str, default='0,16,64')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--tag', type=int, default=8)
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
    per = np.stack([m[:, 1:].var(axis=0) for m in host])
    gv_mean, gv_var = per.mean(axis=0), per.var(axis=0)
    assert (gv_var > 0).all()
    rc, model = cc.prepare(ctx, d, w, mu, cov)
    assert rc == 0
    ins = [torch.from_numpy(m).to(dev) for m in host]
    outs = [torch.full_like(x, float('nan')) for x in ins]
    objs = [torch.full((max(map(int, args.iterations.split(','))) + 1,), float('nan'), dtype=torch.float64, device=dev)
            for _ in ins]
    dmean, dvar = torch.from_numpy(gv_mean).to(dev), torch.from_numpy(gv_var).to(dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    plain = _lib.job_array(_lib.ConvertJob, [(a, T, o) for a, o in zip(ins, outs)])
    gv = _lib.job_array(_lib.ConvertGvJob, [(a, T, o, None, q) for a, o, q in zip(ins, outs, objs)])
    torch.cuda.synchronize()
    vp = lambda jobs: ctypes.cast(jobs, ctypes.c_void_p)  # noqa: E731

    def call_plain():
        _lib.check(ctx, lib.kwy_convert_mcep_batch_dev(ctx.handle, vp(plain), n, d, M, model.data_ptr()))

    def call_gv(N):
        return lambda: _lib.check(ctx, lib.kwy_convert_mcep_gv_batch_dev(ctx.handle, vp(gv), n, d, M, model.data_ptr(), -1,
                                                                         0, dmean.data_ptr(), dvar.data_ptr(), 1.0, N,
                                                                         status.data_ptr()))

    cases = []
    with torch.cuda.stream(stream):
        forms = [('argmax', None, call_plain)] + [(f'gv{N}', N, call_gv(N)) for N in map(int, args.iterations.split(','))]
        for name, N, call in forms:
            call()                                  # warm-up: code objects, the arena at its size
            ctx.sync()
            assert all(bool(torch.isfinite(o).all()) for o in outs), name
            assert not bool(status.any()), name
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
            case = dict(form=name, gv_iterations=N, call_ms=float(np.median(times)), call_ms_min=min(times),
                        call_ms_max=max(times),
                        kernels_ms={k: dict(total_ms=ms, launches=cnt) for k, (ms, cnt) in kernels.items() if cnt})
            solve = kernels['k_mlpg_chunks'][0] + kernels['k_mlpg_finish'][0]
            case['solve_ms'] = solve
            if N is not None:
                q = objs[0][:N + 1].cpu().numpy()
                case['objective_first_last'] = [float(q[0]), float(q[-1])]
                assert all(q[k + 1] >= q[k] for k in range(N)), name
                if N > 0:
                    case['ascent_ms_per_iteration'] = kernels['k_gv_ascent'][0] / N
                    case['iteration_over_solve'] = kernels['k_gv_ascent'][0] / N / solve
            cases.append(case)
    print(json.dumps({'metric': 'GV-considering trajectory generation, one batched call', 'unit': 'ms',
                      'higher_is_better': False, 'value': cases[-1]['call_ms'], 'matrices': n, 'frames': T,
                      'cols': d + 1, 'mixtures': M, 'spread': 0.2, 'repeats': args.repeats, 'dtype': 'f64',
                      'workgroups': n * d, 'cases': cases}))


if __name__ == '__main__':
    main()
