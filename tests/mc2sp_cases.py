"""Inputs for the bits of kwy_mc2sp_dev (tests/test_mc2sp_bits_gpu.py, recorded by tools/record_mc2sp_bits.py into
tests/golden/mc2sp_bits_parent.npz).

k_mc2sp_mfma works on 16 frames x 16 bins per matrix product, a wavefront on four neighbouring products (64 bins) at a
time, and a spectrum has 16 m + 1 bins: the last product holds one bin, the last group of four one product (K = 257,
1025) or one product too (K = 513: 33 products, eight groups and one).  The frame counts sit on both sides of one and
two tiles of 16 frames, 70 leaves 6 frames to a fifth tile; the orders are the default, one that fills twelve and a
quarter k-steps of the product, and the largest the library takes (MC_MAX_ORDER = 63: all sixteen).
"""
import hashlib

import numpy as np

SEED = 61
FRAMES = (1, 15, 16, 17, 33, 70)
FFT_SIZES = (512, 1024, 2048)
ORDERS = (24, 48, 63)
ALPHA = {512: 0.31, 1024: 0.41, 2048: 0.55}
# the cases whose whole output is in the fixture (the others: the SHA-256 of its bytes), (T, fft size, order)
KEPT = ((17, 512, 24), (17, 1024, 48), (17, 2048, 63))


def cases():
    return [(T, fft, order) for fft in FFT_SIZES for order in ORDERS for T in FRAMES]


def mcep(T, fft, order):
    """T frames of order + 1 coefficients: a log-power term and a decaying tail, some frames much quieter"""
    rng = np.random.default_rng([SEED, T, fft, order])
    mc = rng.standard_normal((T, order + 1)) * (0.6 / (1.0 + np.arange(order + 1)))[None, :]
    mc[:, 0] = -6.0 + 3.0 * rng.standard_normal(T)
    mc[::4] *= 0.25
    return np.ascontiguousarray(mc)


def key(T, fft, order):
    return f'sp_{T}_{fft}_{order}'


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def run(ctx, T, fft, order):
    """kwy_mc2sp_dev on the case, into a NaN-filled buffer with guard rows around it: (T, K) doubles"""
    import torch
    from kwiiyatta_amd import _lib
    K = fft // 2 + 1
    mc = torch.from_numpy(mcep(T, fft, order)).cuda()
    buf = torch.full((T + 2, K), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    _lib.check(ctx, _lib.lib.kwy_mc2sp_dev(ctx.handle, mc.data_ptr(), T, order, ALPHA[fft], fft, buf[1].data_ptr()))
    ctx.sync()
    h = buf.cpu().numpy()
    assert np.isnan(h[0]).all() and np.isnan(h[T + 1]).all(), 'a write outside the output'
    return h[1:T + 1]
