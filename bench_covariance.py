#!/usr/bin/env python
"""Companion benchmark of the converter fit's covariance structures: one EM iteration with full covariances against
one with block-diagonal ones (`covariance_structure='block_diag'`), in ONE process on bench_fit.py's data and shapes
(5e5 x 144 and 5e4 x 144 frames, 64 components), after a warm-up, with the kernels' times through `kwy_ctx_profile`.

    python bench_covariance.py [--frames N [N ...]] [--iters K]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KERNELS = {'full': ('k_fit_logprob', 'k_fit_resp', 'k_fit_sums', 'k_fit_cov'),
           'block_diag': ('k_bd_logprob', 'k_fit_resp', 'k_fit_sums', 'k_bd_cov')}


def measure(X, labels, structure, M, iters):
    """-> (ms per EM iteration, {kernel: ms per launch}, lower bound after the last iteration)"""
    import torch
    from kwiiyatta_amd.converter.gmm_fit import HipStats, HipStatsBlockDiag
    st = (HipStatsBlockDiag if structure == 'block_diag' else HipStats)(X, M)
    n = st.n

    def m_step():
        s = st.sums()
        st.means_from(s)
        st.finalize(s, st.cov(s), 1e-6)

    def e_step():
        return torch.cat((st.estep(), st.estep_failed())).tolist()     # the host reads the log-likelihood, as the fit does

    with st.scope():
        st.set_resp_from_labels(labels)
        m_step()
        e_step(); m_step()                  # warm-up iteration
        torch.cuda.synchronize()
        st.ctx.profile(True)
        t0 = time.perf_counter()
        for _ in range(iters):
            ll, failed = e_step()
            m_step()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    assert not failed
    kernels = {}
    for name in KERNELS[structure]:
        ms, launches = st.ctx.profile_read(name)
        kernels[name + '_ms'] = ms / launches if launches else None
    st.ctx.profile(False)
    return elapsed / iters * 1e3, kernels, ll / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='+', default=[500000, 50000])
    ap.add_argument('--dim', type=int, default=144)
    ap.add_argument('--components', type=int, default=64)
    ap.add_argument('--iters', type=int, default=5)
    args = ap.parse_args()
    M, D = args.components, args.dim
    sizes = {}
    for n in args.frames:
        rng = np.random.default_rng(1000)                              # bench_fit.py's rank 0
        centres = np.random.default_rng(0).standard_normal((M, D)) * 2
        lab = rng.integers(0, M, n)
        X = centres[lab] + rng.standard_normal((n, D))
        row = {}
        for structure in ('full', 'block_diag'):
            ms, kernels, bound = measure(X, lab, structure, M, args.iters)
            row[structure] = dict(ms_per_iteration=ms, lower_bound=bound, **kernels)
        row['ratio'] = row['block_diag']['ms_per_iteration'] / row['full']['ms_per_iteration']
        sizes[str(n)] = row
    first = sizes[str(args.frames[0])]
    # what the two new kernels have to move and to compute per iteration at the first size
    n, h = args.frames[0], D // 2
    floor = {'k_bd_logprob': dict(bytes=8.0 * n * (D + M), f64_ops=8.0 * n * M * h),
             'k_bd_cov': dict(bytes=8.0 * n * (D + M), f64_ops=8.0 * n * M * h)}
    print(json.dumps({'metric': 'EM iteration time, block-diagonal covariance GMM fit', 'unit': 'ms/iteration',
                      'value': first['block_diag']['ms_per_iteration'], 'full_value': first['full']['ms_per_iteration'],
                      'ratio_to_full': first['ratio'], 'higher_is_better': False, 'frames': args.frames[0], 'dim': D,
                      'components': M, 'dtype': 'f64', 'iterations': args.iters, 'sizes': sizes, 'floor': floor}))


if __name__ == '__main__':
    main()
