"""Record tests/golden/mc2sp_bits_parent.npz from the library that is built in the tree:

    python tools/record_mc2sp_bits.py COMMIT [OUT_DIR]

Run on an MI355X with the build of COMMIT (the commit kwy_mc2sp_dev's bits are to be held to); the inputs are those of
tests/mc2sp_cases.py, and nothing outside the repository is read.  Every case runs twice; the recorder fails if the two
runs differ.  The fixture holds the SHA-256 of every case's output bytes and the whole output of the cases
mc2sp_cases.KEPT.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import mc2sp_cases as mc  # noqa: E402


def main():
    commit = sys.argv[1]
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden')
    os.makedirs(out_dir, exist_ok=True)
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    g = {'commit': commit, 'seed': mc.SEED}
    names, digests = [], []
    for case in mc.cases():
        a, b = mc.run(ctx, *case), mc.run(ctx, *case)
        T, fft, _ = case
        assert a.shape == (T, fft // 2 + 1) and np.isfinite(a).all() and (a > 0).all(), case
        assert np.array_equal(a, b), case
        names.append(mc.key(*case))
        digests.append(mc.digest(a))
        if case in mc.KEPT:
            g[mc.key(*case)] = a
    g['names'], g['sha256'] = np.array(names), np.array(digests)
    path = os.path.join(out_dir, 'mc2sp_bits_parent.npz')
    np.savez(path, **g)
    print('recorded', len(names), 'cases from', commit, '->', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
