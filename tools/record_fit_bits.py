"""Record tests/golden/fit_bits_parent.npz from the library that is built in the tree:

    python tools/record_fit_bits.py COMMIT [OUT_DIR]

Run on an MI355X with the build of COMMIT (the commit the bits of the mixture fit's and k-means' matrix-core kernels are
to be held to).  The inputs and the calls are those of tests/fit_cases.py (section 5), and nothing outside the
repository is read.  Every case runs twice; the recorder fails if the runs differ.  The covariance statistics are
symmetric to the bit (checked here): the fixture keeps their lower triangles, and the SHA-256 of the output bytes for
the two cases whose arrays are megabytes.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import fit_cases as fc  # noqa: E402


def twice(f, *args):
    a, b = f(*args), f(*args)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (f.__name__, args[1:], 'two runs differ')
    return a


def main():
    commit = sys.argv[1]
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden')
    os.makedirs(out_dir, exist_ok=True)
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    g = {'commit': commit}
    for name in fc.BITS_ESTEP:
        resp, parts, status = twice(fc.bits_estep, ctx, name)
        assert status[0] == 0, name
        g[f'estep_resp_{name}'], g[f'estep_parts_{name}'] = resp, parts
    for name in fc.BITS_STATS + fc.BITS_STATS_DIGEST:
        sums, cov, cov_stats = twice(fc.bits_stats, ctx, name)
        D = cov.shape[1]
        for c in (cov, cov_stats):
            assert c.tobytes() == fc.tril_unpack(fc.tril_pack(c), D).tobytes(), (name, 'not symmetric to the bit')
        if name in fc.BITS_STATS:
            g[f'sums_{name}'], g[f'cov_tril_{name}'] = sums, fc.tril_pack(cov)
        else:
            g[f'sums_sha256_{name}'], g[f'cov_sha256_{name}'] = fc.digest(sums), fc.digest(cov)
        g[f'cov_stats_sha256_{name}'] = fc.digest(cov_stats)
    for name in fc.BITS_KM:
        g[f'km_labels_{name}'], g[f'km_changed_{name}'] = twice(fc.bits_km, ctx, name)
    g['km_labels_tie'], g['km_changed_tie'] = twice(fc.bits_tie, ctx)
    path = os.path.join(out_dir, 'fit_bits_parent.npz')
    np.savez(path, **g)
    print('recorded', len(g) - 1, 'arrays from', commit, '->', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
