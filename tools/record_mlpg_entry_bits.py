"""Record tests/golden/mlpg_entry_bits_parent.npz from the library that is built in the tree:

    python tools/record_mlpg_entry_bits.py COMMIT [OUT_DIR]

Run on an MI355X with the build of COMMIT (the commit the conversion entries' bits are to be held to); the inputs and
the calls are those of tests/mlpg_entry_cases.py, and nothing outside the repository is read.  Every case runs twice: a
case whose two runs differ is not recorded, it is listed and the recorder fails after it has gone through all of them.
Outputs with the same bits are kept once (mlpg_entry_cases.pack).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import mlpg_entry_cases as mc  # noqa: E402


def main():
    commit = sys.argv[1]
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden')
    os.makedirs(out_dir, exist_ok=True)
    from kwiiyatta_amd import _lib
    ctx = _lib.Context(0)
    g = {'commit': commit, 'seed': mc.SEED}
    unstable, accepted, results = [], [], {}
    for key, _, call in mc.CASES:
        a, b = mc.run_case(ctx, call), mc.run_case(ctx, call)
        assert a.keys() == b.keys(), key
        if not all(np.isfinite(v).all() for v in a.values()):
            print('note:', key, 'has values that are not finite')
        if all(a[k].tobytes() == b[k].tobytes() for k in a):
            results[key] = a
        else:
            unstable.append(key)
    g.update(mc.pack(results))
    refused = []
    for key, call in mc.REFUSALS:
        a, b = mc.run_refusal(ctx, call), mc.run_refusal(ctx, call)
        refused.append(a)
        if a[0] == 0:
            accepted.append(key)
        elif a != b:
            unstable.append(key)
            refused[-1] = (0, '', False)                # (a return code of 0 stands for: not recorded)
    # by position in mc.REFUSALS: the return code, the message as an index into the distinct ones, the untouched outputs
    messages = sorted({r[1] for r in refused})
    g.update(refusal_digest=mc.refusal_digest(), refusal_messages=np.array(messages, dtype='S'),
             refusal_rc=np.array([r[0] for r in refused], dtype=np.int8),
             refusal_message=np.array([messages.index(r[1]) for r in refused], dtype=np.uint8),
             refusal_clean=np.array([r[2] for r in refused]))
    path = os.path.join(out_dir, 'mlpg_entry_bits_parent.npz')
    np.savez_compressed(path, **g)
    print('recorded', len(mc.CASES) + len(mc.REFUSALS) - len(unstable) - len(accepted), 'cases from', commit, '->',
          os.path.getsize(path), 'bytes')
    if unstable or accepted:
        sys.exit('left out: not repeatable on this build: ' + (', '.join(unstable) or 'none') +
                 '; not refused by this build: ' + (', '.join(accepted) or 'none'))


if __name__ == '__main__':
    main()
