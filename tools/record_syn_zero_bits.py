"""Record tests/golden/syn_zero_bits_parent.npz from the library that is built in the tree:

    python tools/record_syn_zero_bits.py COMMIT [OUT_DIR]

Run on an MI355X with the build of COMMIT (the commit the synthesis kernel's bits are to be held to); the inputs are
those of tests/syn_zero_cases.py, and nothing outside the repository is read.  The batched entry renders a pulse like
the single call: the recorder checks that on the recorded build and keeps the single call's waveforms.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import syn_zero_cases as zc  # noqa: E402


def main():
    commit = sys.argv[1]
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden')
    os.makedirs(out_dir, exist_ok=True)
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    g = {'commit': commit, 'seed': zc.SEED}
    for fs in zc.RATES:
        single = zc.render_single(fs, ctx)
        for k, (a, b) in enumerate(zip(single, zc.render_batch(ctx, fs))):
            assert a.shape == (zc.y_length(len(zc.batch(fs)[k][0]), fs),) and np.isfinite(a).all() and np.abs(a).max() > 0
            assert np.array_equal(a, b), (fs, k)
            g[zc.key(fs, k)] = a
    path = os.path.join(out_dir, 'syn_zero_bits_parent.npz')
    np.savez(path, **g)
    print('recorded', len(g) - 2, 'arrays from', commit, '->', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
