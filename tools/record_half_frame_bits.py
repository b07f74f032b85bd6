"""Record tests/golden/d4c_half_bits_48k_parent.npz and d4c_half_bits_rates_parent.npz from the library that is built in
the tree:

    python tools/record_half_frame_bits.py COMMIT [OUT_DIR]

Run on an MI355X with the build of COMMIT (the commit the bits of D4C are to be held to: the one before the body's
first FFT pass learnt to skip a zero half); the inputs are those of tests/half_frame_cases.py, and nothing outside
the repository is read.  The recorder checks on the recorded build that every D4C frame was analysed, that the cases
lie on the sides of the switch they are named for, and that the batched D4C entry gives the single calls' rows.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import half_frame_cases as hc  # noqa: E402
from d4c_cases import UNGATED  # noqa: E402


def main():
    commit = sys.argv[1]
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden')
    os.makedirs(out_dir, exist_ok=True)
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    files = {}
    for fs in hc.D4C_F0:
        g = files.setdefault(hc.D4C_FILE[fs], {'commit': commit, 'seed': hc.SEED})
        cases = hc.d4c_cases(fs)
        kinds = [hc.d4c_window(fs, f0)[1] for f0 in hc.D4C_F0[fs]]
        assert kinds[0] is False and all(kinds[1:]) and hc.d4c_window(fs, hc.D4C_F0[fs][1])[0] == hc.D4C_N[fs] // 2 + 1
        single = {name: hc.d4c_single(fs, c, ctx) for name, c in cases.items()}
        for (name, c), b in zip(cases.items(), hc.d4c_batch(ctx, fs, list(cases.values()))):
            a = single[name]
            assert np.isfinite(a).all() and not (a == UNGATED).all(axis=1).any(), (fs, name)
            assert np.array_equal(a, b), (fs, name)
            g[hc.d4c_key(fs, name)] = a
    for name, g in files.items():
        path = os.path.join(out_dir, name)
        np.savez_compressed(path, **g)
        print('recorded', len(g) - 2, 'arrays from', commit, '->', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
