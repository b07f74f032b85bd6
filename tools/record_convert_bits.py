"""Record tests/golden/convert_bits_parent.npz from the library that is built in the tree:

    python tools/record_convert_bits.py COMMIT [OUT_DIR]

Run on an MI355X with the build of COMMIT (the commit the conversion kernels' bits are to be held to); the inputs are
those of tests/convert_cases.py, and nothing outside the repository is read.  Frame-wise conversion and mc2sp work row
by row, so their outputs for the first T rows of a matrix are the first T rows of the output for the whole matrix: the
recorder checks that on the recorded build and keeps the longest output only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import convert_cases as cc  # noqa: E402


def main():
    commit = sys.argv[1]
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden')
    os.makedirs(out_dir, exist_ok=True)
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    g = {'commit': commit, 'seed': cc.SEED, 'bin_step': cc.MC2SP_BIN_STEP}
    for D, M, Ts in cc.FRAMES:
        w, mu, cov, X = cc.frames_case(D, M)
        full = cc.convert_frames(ctx, X, w, mu, cov)
        for T in Ts:
            assert np.array_equal(cc.convert_frames(ctx, X[:T], w, mu, cov), full[:T]), (D, M, T)
        g[cc.frames_key(D, M)] = full
    for d, M, Ts in cc.MCEP:
        w, mu, cov = cc.mixture(3 * d, M, 0)
        rc, model = cc.prepare(ctx, d, w, mu, cov)
        assert rc == 0, (d, M, rc)
        for T in Ts:
            g[cc.mcep_key(d, M, T)] = cc.convert_mcep(ctx, model, M, cc.mcep(T, d, M, 0))
    for d, M, T in cc.REFUSED:
        w, mu, cov = cc.mixture(3 * d, M, 0)
        rc, model = cc.prepare(ctx, d, w, mu, cov)
        mc = cc.mcep(T, d, M, 0)
        try:
            cc.convert_mcep(ctx, model, M, mc)
            rc2 = 0
        except ValueError:
            rc2 = _lib.KWY_EINVAL
        g[f'refused_{d}'] = np.array([rc, rc2])
    d, M, Ts = cc.BATCH
    w, mu, cov = cc.mixture(3 * d, M, 1)
    rc, model = cc.prepare(ctx, d, w, mu, cov)
    assert rc == 0
    for k, y in enumerate(cc.convert_mcep(ctx, model, M, [cc.mcep(T, d, M, 1) for T in Ts])):
        g[f'batch_{k}'] = y
    for fft, Ts in cc.MC2SP:
        mc = cc.mc2sp_rows(max(Ts))
        full = cc.mc2sp(ctx, mc, fft)
        for T in Ts:
            assert np.array_equal(cc.mc2sp(ctx, mc[:T], fft), full[:T]), (fft, T)
        g[f'mc2sp_{fft}'] = cc.mc2sp_sample(full)
    path = os.path.join(out_dir, 'convert_bits_parent.npz')
    np.savez(path, **g)
    print('recorded', len(g) - 3, 'arrays from', commit, '->', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
