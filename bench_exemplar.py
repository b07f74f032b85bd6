#!/usr/bin/env python
"""The activation updates of the exemplar converter (--converter exemplar) beside the same updates in torch.

    python bench_exemplar.py [--frames 32000 512000] [--atoms 2048] [--bins 257] [--updates 100] [--runs 20] [--warmup 2]

Timed on one GPU, in one process, each figure the median of --runs runs after --warmup untimed ones, wall clock
around the enqueue and the synchronisation of the stream (the shortest figure here is tens of milliseconds):

    nmf     kwy_nmf_convert_dev: T frames (T = 32 000 is 16 utterances of 2000 frames as one ragged batch) against
            --atoms exemplars of --bins bins, --updates multiplicative updates and the closing Y = H Tg, on smooth
            positive unit-sum spectra; 4 T A B flop per update, the padding copies and the closing product included in
            the time but not in the flop
    torch   the same updates as float64 torch.mm calls with preallocated outputs, in the same process
    kernels one more run under the context's profiler: the summed and the mean duration of every kernel

The yardstick of the flop rate beside torch is the project's own streamed-operand f64 figure, k_nn_search at 30.0 / 36.8
TFLOP/s (bench_nonparallel.py, README.md).  Prints ONE JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

NN_SEARCH_TFLOPS = {32000: 30.0, 512000: 36.8}


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


def spectra(torch, n, B, dev, seed):
    """n smooth positive rows of unit sum: three Gaussian bumps on a floor of 1e-4"""
    g = torch.Generator(device=dev).manual_seed(seed)
    b = torch.arange(B, dtype=torch.float64, device=dev)[None, :]
    out = torch.full((n, B), 1e-4, dtype=torch.float64, device=dev)
    for _ in range(3):
        centre = torch.rand((n, 1), dtype=torch.float64, device=dev, generator=g) * B
        width = B / 40 + torch.rand((n, 1), dtype=torch.float64, device=dev, generator=g) * B / 8
        out += torch.exp(-0.5 * ((b - centre) / width) ** 2)
    return (out / out.sum(dim=1, keepdim=True)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='+', default=[32000, 512000])
    ap.add_argument('--atoms', type=int, default=2048)
    ap.add_argument('--bins', type=int, default=257)
    ap.add_argument('--updates', type=int, default=100)
    ap.add_argument('--sparsity', type=float, default=0.05)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd.backend import nmf
    ctx = _lib.Context(0)
    A, B, N, lam = args.atoms, args.bins, args.updates, args.sparsity
    S, Tg = spectra(torch, A, B, dev, 1), spectra(torch, A, B, dev, 2)
    out = {}
    for T in args.frames:
        X = spectra(torch, T, B, dev, 3 + T)
        Y = torch.empty((T, B), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        scratch = torch.empty(nmf.scratch_bytes(A, B, T), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def run():
            nmf.convert_dev(ctx, S, Tg, X, N, lam, scratch, Y=Y, status=status)

        t = median_seconds(run, ctx.sync, args.runs, args.warmup)
        flop = 4.0 * T * A * B * N
        rec = {'nmf_seconds': t[0], 'nmf_min_max': t[1:], 'nmf_tflops': flop / t[0] / 1e12,
               'status': int(status.item()), 'scratch_bytes': scratch.numel()}
        if T in NN_SEARCH_TFLOPS:
            rec['nmf_over_nn_search_rate'] = rec['nmf_tflops'] / NN_SEARCH_TFLOPS[T]
        ctx.profile(True)
        run()
        kernels = {}
        for name in ('k_nmf_ratio', 'k_nmf_update', 'k_nmf_apply'):
            ms, launches = ctx.profile_read(name)
            kernels[name] = {'total_ms': ms, 'launches': launches, 'mean_ms': ms / launches if launches else None}
        ctx.profile(False)
        rec['kernels'] = kernels
        if not args.no_torch:
            H, G = (torch.empty((T, A), dtype=torch.float64, device=dev) for _ in range(2))
            R = torch.empty((T, B), dtype=torch.float64, device=dev)
            Yt = torch.empty((T, B), dtype=torch.float64, device=dev)
            St = S.t().contiguous()
            tiny = torch.finfo(torch.float64).tiny

            def run_torch():
                H.fill_(1.0)
                for _ in range(N):
                    torch.mm(H, S, out=R)
                    torch.div(X, R.clamp_min_(tiny), out=R)
                    torch.mm(R, St, out=G)
                    H.mul_(G).div_(1.0 + lam)
                torch.mm(H, Tg, out=Yt)

            tt = median_seconds(run_torch, torch.cuda.synchronize, args.runs, args.warmup)
            scale = Yt.abs().amax(dim=1, keepdim=True)
            rec.update(torch_seconds=tt[0], torch_min_max=tt[1:], torch_tflops=flop / tt[0] / 1e12,
                       torch_over_nmf=tt[0] / t[0], y_max_rel_difference=float(((Y - Yt).abs() / scale).max().item()))
            del H, G, R, Yt, St
        out[str(T)] = rec
        del X, Y, scratch
        torch.cuda.empty_cache()
    last = out[str(args.frames[-1])]
    print(json.dumps({'metric': f'seconds, {N} activation updates of {args.frames[-1]} frames against {A} exemplars of '
                                f'{B} bins, float64',
                      'value': last['nmf_seconds'], 'unit': 's', 'n_gpus': 1,
                      'detail': {'atoms': A, 'bins': B, 'updates': N, 'sparsity': lam, 'runs': args.runs,
                                 'warmup': args.warmup, 'frames': out}}))


if __name__ == '__main__':
    main()
