"""Record tests/golden/d4c_bits_parent.npz and synth_bits_parent.npz from the library that is built in the tree:

    python tests/golden/make_bits_parent.py COMMIT [OUT_DIR]

Run on an MI355X with the build of COMMIT (the commit the bits are to be held to); the inputs are those of
tests/bits_cases.py.  Refuses to write a D4C case without a gated frame.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import bits_cases as bc  # noqa: E402
from d4c_cases import UNGATED  # noqa: E402


def d4c_dev(x, f0, t, fs):
    import torch
    from kwiiyatta_amd import _lib
    from kwiiyatta_amd._lib import lib
    ctx = _lib.Context(0)
    fft = lib.kwy_cheaptrick_fft_size(fs, 71.0)
    dx, df0, dt = (torch.from_numpy(a).cuda() for a in (x, f0, t))
    out = torch.empty((len(f0), fft // 2 + 1), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    _lib.check(ctx, lib.kwy_d4c_dev(ctx.handle, dx.data_ptr(), len(x), fs, dt.data_ptr(), df0.data_ptr(), len(f0),
                                    0.85, fft, out.data_ptr()))
    ctx.sync()
    return out.cpu().numpy()


def main():
    commit = sys.argv[1]
    out_dir = sys.argv[2] if len(sys.argv) > 2 else HERE
    os.makedirs(out_dir, exist_ok=True)
    from kwiiyatta_amd.backend import world
    d4c = {'commit': commit, 'seed': bc.SEED, 'bin_step': bc.D4C_BIN_STEP}
    for fs in bc.D4C_RATES:
        for f in bc.D4C_F0:
            x, f0, t = bc.d4c_case(fs, f)
            ap = world.d4c(x, f0, t, fs)
            assert not (ap == UNGATED).all(), (fs, f)
            d4c[bc.d4c_key(fs, f)] = bc.d4c_sample(ap)
    for fs, f in bc.D4C_HIGH:
        x, f0, t = bc.d4c_case(fs, f)
        ap = d4c_dev(x, f0, t, fs)
        assert not (ap == UNGATED).all(), (fs, f)
        d4c[bc.d4c_key(fs, f, dev=True)] = bc.d4c_sample(ap)
    np.savez(os.path.join(out_dir, 'd4c_bits_parent.npz'), **d4c)
    syn = {'commit': commit, 'seed': bc.SEED}
    for fs in bc.SYNTH_RATES:
        f0, sp, ap = bc.synth_case(fs)
        syn[f'y_{fs}'] = world.synthesize(f0, sp, ap, fs, 5.0)
    np.savez(os.path.join(out_dir, 'synth_bits_parent.npz'), **syn)
    print('recorded', len(d4c) - 3, 'D4C cases and', len(syn) - 2, 'utterances from', commit)


if __name__ == '__main__':
    main()
