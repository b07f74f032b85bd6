"""The exemplar converter's kernels (csrc/kwy_nmf.hip) against the numpy model of tests/nmf_cases.py.

Tolerance, computed here from the references alone: d is the larger of two deviations on the same inputs -- the
float64 model against the long-double model, and the float64 model against itself with the atoms permuted (another
summation order).  The kernel may deviate from the float64 model by 64 d (nmf_cases.bound), per frame and relative
to the frame's largest entry, for Y, for H and (relative to the call's largest value) for the objective; the bound
never goes below A 2^-52.  Tiny activations are not compared relatively: they underflow to 0 in the model."""
import ctypes
import functools

import numpy as np
import pytest

import nmf_cases as nc
from test_nmf_cases import fixed_point_case

pytestmark = pytest.mark.gpu

SHAPES = [(65, 48, 20, 50), (129, 200, 33, 100), (65, 130, 17, 300)]        # (B, A, T, N)
EDGES = ([(65, A, 33, 3) for A in (1, 15, 16, 17)] + [(65, 17, T, 3) for T in (1, 31, 32, 33)] +
         [(B, 17, 33, 3) for B in (2, 63, 65)] + [(65, 17, 33, N) for N in (0, 1)])


@pytest.fixture(scope='module')
def nmf():
    from kwiiyatta_amd.backend import nmf
    return nmf


def start(A, T):
    return np.random.default_rng(7 * A + T).uniform(0.2, 2.0, size=(T, A))


@functools.lru_cache(maxsize=None)
def case(B, A, T, N, sparsity, with_h0):
    S, Tg, X = nc.make_case(B, A, T)
    h0 = start(A, T) if with_h0 else None
    ref = nc.reference(S, Tg, X, N, sparsity, h0)
    for a in (S, Tg, X, h0, ref['Y'], ref['H'], ref['objective']):
        if a is not None:
            a.setflags(write=False)
    return S, Tg, X, h0, ref


def check_against_model(nmf, B, A, T, N, sparsity, with_h0):
    S, Tg, X, h0, ref = case(B, A, T, N, sparsity, with_h0)
    Y, H, obj = nmf.convert(S, Tg, X, N, sparsity, return_h=True, return_objective=True, h0=h0)
    assert Y.shape == (T, B) and H.shape == (T, A) and obj.shape == (T,)
    dev = {'Y': nc.frame_rel(Y, ref['Y']), 'H': nc.frame_rel(H, ref['H']),
           'objective': nc.vector_rel(obj, ref['objective'])}
    bounds = {k: nc.bound(ref['d'][k], A) for k in dev}
    print(f'B={B} A={A} T={T} N={N} lambda={sparsity} h0={with_h0}: '
          + ', '.join(f'{k} {dev[k]:.3g} (d {ref["d"][k]:.3g}, bound {bounds[k]:.3g})' for k in dev))
    for k in dev:
        assert dev[k] <= bounds[k], (k, dev[k], bounds[k])
    return Y, H, obj


@pytest.mark.parametrize('with_h0', [False, True])
@pytest.mark.parametrize('sparsity', [0.0, 0.1])
@pytest.mark.parametrize('shape', SHAPES)
def test_against_model(nmf, shape, sparsity, with_h0):
    check_against_model(nmf, *shape, sparsity, with_h0)


@pytest.mark.parametrize('with_h0', [False, True])
@pytest.mark.parametrize('shape', EDGES)
def test_edges_against_model(nmf, shape, with_h0):
    check_against_model(nmf, *shape, 0.1 if with_h0 else 0.0, with_h0)


def test_no_updates_is_the_start(nmf):
    S, Tg, X, h0, _ = case(65, 17, 33, 0, 0.1, True)
    assert np.array_equal(nmf.activations(S, X, 0, 0.1, h0=h0), h0)
    assert np.array_equal(nmf.activations(S, X, 0, 0.1), np.ones((33, 17)))


def test_two_runs_are_bit_equal(nmf):
    S, Tg, X, _, _ = case(129, 200, 33, 100, 0.1, False)
    a = nmf.convert(S, Tg, X, 100, 0.1, return_h=True, return_objective=True)
    b = nmf.convert(S, Tg, X, 100, 0.1, return_h=True, return_objective=True)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_chained_single_updates_are_bit_equal(nmf):
    """the prefix property on the device: N updates in one call = N calls of one update chained through h0"""
    S, Tg, X, _, _ = case(65, 48, 20, 50, 0.1, False)
    N = 12
    H = None
    for _ in range(N):
        H = nmf.activations(S, X, 1, 0.1, h0=H)
    Y, Hn = nmf.convert(S, Tg, X, N, 0.1, return_h=True)
    assert np.array_equal(H, Hn)
    assert np.array_equal(nmf.convert(S, Tg, X, 0, 0.1, h0=H), Y)     # and Y is a function of H alone
    assert np.array_equal(nmf.activations(S, X, 7, 0.1, h0=nmf.activations(S, X, 5, 0.1)), Hn)


def test_frames_never_interact(nmf):
    S, Tg, X, h0, _ = case(129, 200, 33, 100, 0.1, True)
    Y, H, obj = nmf.convert(S, Tg, X, 20, 0.1, return_h=True, return_objective=True, h0=h0)
    for rows in (slice(5, 6), slice(16, 33)):
        y, h, o = nmf.convert(S, Tg, np.ascontiguousarray(X[rows]), 20, 0.1, return_h=True, return_objective=True,
                              h0=np.ascontiguousarray(h0[rows]))
        assert np.array_equal(y, Y[rows]) and np.array_equal(h, H[rows]) and np.array_equal(o, obj[rows])


def test_fixed_point(nmf):
    """lambda = 0, X = W S, h0 = W: G is 1 in exact arithmetic, so H stays W to within 8 N ulp"""
    N = 50
    S, W, X = fixed_point_case(65, 48, 20)
    H = nmf.activations(S, X, N, 0.0, h0=W)
    print('fixed point: largest drift', (np.abs(H - W) / np.spacing(np.where(W > 0, W, 1.0))).max(), 'ulp of', 8 * N)
    assert (np.abs(H - W) <= 8 * N * np.spacing(W)).all()
    assert (H[W == 0] == 0).all()


def raw_call(nmf, gpu_ctx, S, Tg, X, N, sparsity):
    """kwy_nmf_convert itself: (return code, status word, Y, H) with Y and H pre-filled with -7"""
    from kwiiyatta_amd._lib import lib, ptr
    T, (A, B) = len(X), S.shape
    Y, H = np.full((T, B), -7.0), np.full((T, A), -7.0)
    status = np.full(1, 99, dtype=np.int32)
    rc = lib.kwy_nmf_convert(gpu_ctx.handle, ptr(S), ptr(Tg), ptr(X), A, B, T, N, sparsity, None, ptr(Y), ptr(H), None,
                             ptr(status))
    return rc, int(status[0]), Y, H


@pytest.mark.parametrize('value', [0.0, -1.0, np.nan, np.inf])
@pytest.mark.parametrize('which', ['X', 'S', 'Tg'])
def test_status_counts_entries_outside_the_contract(nmf, gpu_ctx, which, value):
    """the status word counts them, the outputs are written all the same (flagged, not withheld), nothing faults,
    and the shim raises"""
    S, Tg, X = (a.copy() for a in nc.make_case(65, 17, 33))
    {'X': X, 'S': S, 'Tg': Tg}[which][3, 5] = value
    rc, status, Y, H = raw_call(nmf, gpu_ctx, S, Tg, X, 3, 0.1)
    assert rc == 0 and status == 1
    assert not (Y == -7.0).any() and not (H == -7.0).any()
    if which == 'X':            # frames never interact: the others are what they are without the bad entry
        good = np.arange(33) != 3
        Yg = nmf.convert(S, Tg, np.ascontiguousarray(X[good]), 3, 0.1)
        assert np.array_equal(Y[good], Yg)
    with pytest.raises(ValueError, match='not finite and positive'):
        nmf.convert(S, Tg, X, 3, 0.1)
    nmf.convert(S, Tg, X, 3, 0.1, strict=False)


def test_status_is_set_not_accumulated(nmf, gpu_ctx):
    S, Tg, X = nc.make_case(65, 17, 33)
    rc, status, _, _ = raw_call(nmf, gpu_ctx, S, Tg, X, 1, 0.0)
    assert rc == 0 and status == 0
    h0 = start(17, 33)
    h0[2, 2] = 0.0                       # zero is a legal activation
    nmf.activations(S, X, 1, 0.0, h0=h0)
    h0[2, 2] = -1.0
    with pytest.raises(ValueError):
        nmf.activations(S, X, 1, 0.0, h0=h0)


def test_no_frames(nmf, gpu_ctx):
    S, Tg, _ = nc.make_case(65, 17, 33)
    X = np.empty((0, 65))
    Y, H, obj = nmf.convert(S, Tg, X, 10, 0.1, return_h=True, return_objective=True)
    assert Y.shape == (0, 65) and H.shape == (0, 17) and obj.shape == (0,)
    from kwiiyatta_amd._lib import lib, ptr
    assert lib.kwy_nmf_convert(gpu_ctx.handle, None, None, None, 17, 65, 0, 10, 0.1, None, None, None, None, None) == 0
    assert nmf.scratch_bytes(17, 65, 0) == 0


@pytest.mark.parametrize('A, B, N, sparsity', [(0, 65, 1, 0.0), (8193, 65, 1, 0.0), (17, 1, 1, 0.0), (17, 2050, 1, 0.0),
                                               (17, 65, -1, 0.0), (17, 65, 1001, 0.0), (17, 65, 1, -0.1),
                                               (17, 65, 1, np.inf), (17, 65, 1, np.nan)])
def test_limits_are_refused_before_any_launch(nmf, gpu_ctx, A, B, N, sparsity):
    from kwiiyatta_amd._lib import KWY_EINVAL, lib, ptr
    S, X = np.ones((max(A, 1), max(B, 1))), np.ones((4, max(B, 1)))
    Y = np.full((4, max(B, 1)), -7.0)
    rc = lib.kwy_nmf_convert(gpu_ctx.handle, ptr(S), ptr(S), ptr(X), A, B, 4, N, sparsity, None, ptr(Y), None, None, None)
    assert rc == KWY_EINVAL and (Y == -7.0).all()
    assert 'nmf_convert' in gpu_ctx.error()
    if A >= 1 and B >= 1:
        with pytest.raises(ValueError):
            nmf.convert(S, S, X, N, sparsity)


def test_pointer_combinations_are_refused(nmf, gpu_ctx):
    from kwiiyatta_amd._lib import KWY_EINVAL, lib, ptr
    S, _, X = nc.make_case(65, 17, 4)
    Y = np.empty((4, 65))
    call = lambda s, tg, x, y, h: lib.kwy_nmf_convert(gpu_ctx.handle, s, tg, x, 17, 65, 4, 1, 0.0, None, y, h, None, None)
    assert call(None, ptr(S), ptr(X), ptr(Y), None) == KWY_EINVAL
    assert call(ptr(S), None, ptr(X), ptr(Y), None) == KWY_EINVAL        # Y without Tg
    assert call(ptr(S), ptr(S), ptr(X), None, None) == KWY_EINVAL        # Tg without Y, and nothing asked for
    assert call(ptr(S), None, ptr(X), None, None) == KWY_EINVAL


def test_device_form_keeps_to_its_scratch(nmf, gpu_ctx):
    """convert_dev writes nothing outside kwy_nmf_scratch_bytes: guard words in front of and behind the scratch stay,
    and the results are those of the host form"""
    import torch
    B, A, T, N = 129, 200, 33, 10
    S, Tg, X, h0, _ = case(B, A, T, 100, 0.1, True)
    want = nmf.convert(S, Tg, X, N, 0.1, return_h=True, return_objective=True, h0=h0)
    need = nmf.scratch_bytes(A, B, T)
    assert need > 0 and need == nmf.scratch_bytes(A, B, T)
    guard = 4096
    dev = torch.device('cuda', gpu_ctx.device)
    buf = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    dS, dTg, dX, dh0 = t(S), t(Tg), t(X), t(h0)
    Y = torch.empty((T, B), dtype=torch.float64, device=dev)
    H = torch.empty((T, A), dtype=torch.float64, device=dev)
    obj = torch.empty(T, dtype=torch.float64, device=dev)
    status = torch.full((1,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    nmf.convert_dev(gpu_ctx, dS, dTg, dX, N, 0.1, buf[guard:guard + need], Y=Y, H=H, objective=obj, status=status, h0=dh0)
    gpu_ctx.sync()
    assert (buf[:guard] == 0xA5).all() and (buf[guard + need:] == 0xA5).all()
    nmf.check_status(status)
    for got, exp in zip((Y, H, obj), want):
        assert np.array_equal(got.cpu().numpy(), exp)
    with pytest.raises(ValueError, match='scratch'):
        nmf.convert_dev(gpu_ctx, dS, dTg, dX, N, 0.1, buf[:need - 1], Y=Y)
    from kwiiyatta_amd._lib import KWY_EINVAL, lib
    rc = lib.kwy_nmf_convert_dev(gpu_ctx.handle, dS.data_ptr(), dTg.data_ptr(), dX.data_ptr(), A, B, T, N, 0.1, None,
                                 Y.data_ptr(), None, None, None, buf.data_ptr(), ctypes.c_size_t(need - 1))
    assert rc == KWY_EINVAL


def test_scratch_bytes_grows_with_every_size(nmf):
    base = nmf.scratch_bytes(200, 129, 33)
    assert nmf.scratch_bytes(200, 129, 129) > base
    assert nmf.scratch_bytes(257, 129, 33) > base
    assert nmf.scratch_bytes(200, 193, 33) > base
    assert nmf.scratch_bytes(8193, 129, 33) == 0 and nmf.scratch_bytes(200, 1, 33) == 0
