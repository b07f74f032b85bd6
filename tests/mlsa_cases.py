"""The inputs of the MLSA filter's edge tests: the case lists that the CPU check of the inputs (test_mlsa_cases.py)
and the GPU test of the kernel (test_mlsa_edges_gpu.py) share.  The checker is the CPU oracle (ko.mc2b,
ko.mlsa_synthesis); nothing here imports the product.

What the cases are built around, in kwy_mlsa.hip:
* a frame is staged as `j = lane; j < hop; j += 64` and the input scale exp(b[0]) of sample j is formed by `lane`
  plus 64 r repeated additions of the slope: hop below 64, on either side of a multiple of 64 and at MLSA_MAX_HOP
  are separate paths.  c0 is kept (standard deviation 1), so b[0] moves by a few units from frame to frame and a
  wrong number of additions shows;
* the all-pass chain runs in NB = (order - 1 + 7) / 8 blocks of eight links: the orders sit on both sides of every
  block seam;
* nproc = min((n - 1) / hop, T) frames are filtered, what lies behind them is exactly zero."""
import collections

import numpy as np

MLSA_MAX_ORDER, MLSA_MAX_HOP, MLSA_JOBS_MAX = 62, 2048, 64
BOUND = 1e-11                                 # max |got - ref| <= BOUND * max |ref|: the project's bound for this kernel
ALPHA = 0.41                                  # pysptk's all-pass constant for 16 kHz

Case = collections.namedtuple('Case', 'name hop T order pd n alpha constant')


def _case(name, hop, T, order, pd, n=None, alpha=ALPHA, constant=False):
    return Case(name, hop, T, order, pd, T * hop + 1 if n is None else n, alpha, constant)


HOPS = (1, 2, 63, 64, 65, 127, 128, 129, 2048)
ORDERS = (2, 9, 10, 17, 18, 25, 26, 33, 34, 41, 42, 49, 50, 57, 58, 62)
GRID_HOP, GRID_T = 80, 3
GRID_N = (1, 80, 81, 160, 161, 240, 241, 900)
GRID_NPROC = (0, 0, 1, 1, 2, 2, 3, 3)
ALPHAS = (0.0, -0.3, 0.41, 0.77)

HOP_CASES = [_case(f'hop{hop}_pd{pd}', hop, 5 if hop <= 129 else 2, 24, pd) for hop in HOPS for pd in (4, 5)]
ORDER_CASES = [_case(f'order{order}_pd{pd}', 32, 6, order, pd) for order in ORDERS for pd in (4, 5)]
GRID_CASES = ([_case(f'n{n}', GRID_HOP, GRID_T, 24, 4, n=n) for n in GRID_N]
              + [_case('n200_T1', GRID_HOP, 1, 24, 4, n=200)])
COEF_CASES = ([_case(f'constant_pd{pd}', 80, 5, 24, pd, constant=True) for pd in (4, 5)]
              + [_case(f'alpha{a}', 80, 5, 24, 4, alpha=a) for a in ALPHAS])
ALL_CASES = HOP_CASES + ORDER_CASES + GRID_CASES + COEF_CASES

# one batched call: ragged in n and in T, one job without a processed frame
BATCH_JOBS = [_case(f'job_n{n}_T{T}', GRID_HOP, T, 24, 4, n=n) for n, T in ((80, 3), (81, 3), (161, 3), (900, 3), (200, 1))]


def nproc(case):
    """frames that are filtered: frame f is iff (f + 1) hop < n"""
    return min((case.n - 1) // case.hop, case.T)


def mcep(rng, order, scale=0.4):
    """test_mlsa_codec._mcep with c0 kept: c0 ~ N(0, 1), c_k ~ N(0, (scale / k)^2)"""
    mc = np.empty(order + 1)
    mc[0] = rng.standard_normal()
    mc[1:] = rng.standard_normal(order) * scale / np.arange(1, order + 1)
    return mc


def inputs(case):
    """-> (x, mc): n samples of 0.1 * randn, T x (order + 1) mel-cepstra (one row repeated for a constant case)"""
    rng = np.random.default_rng([case.hop, case.T, case.order, case.pd, case.n, int(round(case.alpha * 1000)) + 1000,
                                 int(case.constant)])
    if case.constant:
        mc = np.tile(mcep(rng, case.order), (case.T, 1))
    else:
        mc = np.stack([mcep(rng, case.order) for _ in range(case.T)])
    return rng.standard_normal(case.n) * 0.1, np.ascontiguousarray(mc)


def reference(case, ignore_c0=False):
    """-> (x, mc, b, y) by the oracle; ignore_c0: column 0 of mc taken as zero (apply_mlsa_filter)"""
    from oracle import oracle as ko
    x, mc = inputs(case)
    b = ko.mc2b(np.hstack((np.zeros((case.T, 1)), mc[:, 1:])) if ignore_c0 else mc, case.alpha)
    return x, mc, b, ko.mlsa_synthesis(x, b, case.alpha, case.hop, case.pd)


def deviation(got, ref):
    """max |got - ref| / max |ref|; 0 / 0 (nothing filtered, nothing written) counts as 0"""
    scale, err = np.abs(ref).max(), np.abs(got - ref).max()
    return 0.0 if err == 0.0 else err / scale


# every argument outside the accepted range, one at a time: (name, overrides of the good call)
GOOD = dict(order=24, pd=4, hop=80, alpha=ALPHA, n=401, T=5)
REFUSALS = [('order 1', dict(order=1)), ('order 63', dict(order=63)), ('pd 3', dict(pd=3)), ('pd 6', dict(pd=6)),
            ('hop 0', dict(hop=0)), ('hop 2049', dict(hop=2049)), ('alpha 1', dict(alpha=1.0)),
            ('alpha -1', dict(alpha=-1.0)), ('alpha NaN', dict(alpha=float('nan'))), ('n 0', dict(n=0)),
            ('T 0', dict(T=0))]
