"""The conversion stage's kernels in their register-fed (k_gmm_logp) and coalesced (k_gmm_cond) forms, through the C ABI:

  * bit for bit the outputs of the build before the change, recorded on an MI355X by tools/record_convert_bits.py into
    tests/golden/convert_bits_parent.npz (inputs: tests/convert_cases.py): frame-wise conversion -- a softmax over all
    log-densities, so every bit of every log-density counts --, mel-cepstrum conversion (hard arg-max, conditional
    means, MLPG) alone and as a ragged batch, and mc2sp;
  * against float64 numpy from the raw mixture parameters, within 1e-9 of the largest reference value, on inputs whose
    best and second-best log-density are at least 1e-6 apart in EVERY frame (asserted on the CPU first), so that the
    hard arg-max cannot flip by rounding;
  * mixtures with exactly equal log-densities, within one pass of the arg-max and across its passes: the lowest index
    wins.

Frame counts sit on the seams of the kernels' maps (16-frame sub-tiles, 32 frames per wavefront, 256 per workgroup
tile), feature widths on one to six 16-column blocks -- D = 82 is the widest mixture the library prepares, and six
blocks are all the log-density kernel is built for.  D = 144 and D = 150 (nine blocks and more) cannot reach a
log-density kernel: k_gmm_prep needs 3 D^2 doubles of LDS, so the library refuses them with KWY_EINVAL, as the recorded
build does; the fixture holds that build's return codes and the tree has to give the same.
"""
import os

import numpy as np
import pytest

import convert_cases as cc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'convert_bits_parent.npz')
GAP = 1e-6


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    assert int(g['seed']) == cc.SEED and int(g['bin_step']) == cc.MC2SP_BIN_STEP
    return g


@pytest.fixture(scope='module')
def ctx():
    from kwiiyatta_amd import _lib
    return _lib.Context(0)


def _same(got, want, golden, what):
    assert got.shape == want.shape, what
    assert np.isfinite(want).all() and np.abs(want).max() > 0, what
    assert np.array_equal(got, want), f"{what}: differs from the build at {golden['commit']}"


def _close(got, ref, what):
    err = np.abs(got - ref).max()
    print(f'{what}: max |got - numpy| = {err:.3e}, largest reference value {np.abs(ref).max():.3e}')
    assert err <= 1e-9 * np.abs(ref).max(), what


@pytest.mark.parametrize('D,M,Ts', cc.FRAMES, ids=lambda v: str(v) if isinstance(v, int) else 'T')
def test_frame_conversion_bits_and_values(ctx, golden, D, M, Ts):
    w, mu, cov, X = cc.frames_case(D, M)
    if M > 1:   # the posteriors are shared, so the output shows the log-densities' low bits
        assert cc.posterior(cc.ref_logp(X, w, mu, cov)).max(axis=1).mean() < 0.9
    want = golden[cc.frames_key(D, M)]
    for T in Ts:
        _same(cc.convert_frames(ctx, X[:T], w, mu, cov), want[:T], golden, f'D = {D}, M = {M}, T = {T}')
    _close(want, cc.ref_frames(X, w, mu, cov), f'frames D = {D}, M = {M}')


@pytest.mark.parametrize('d,M,Ts', cc.MCEP, ids=lambda v: str(v) if isinstance(v, int) else 'T')
def test_mcep_conversion_bits_and_values(ctx, golden, d, M, Ts):
    w, mu, cov = cc.mixture(3 * d, M, 0)
    rc, model = cc.prepare(ctx, d, w, mu, cov)
    assert rc == 0
    for T in Ts:
        mc = cc.mcep(T, d, M, 0)
        gap = cc.logp_gap(cc.ref_logp(cc.delta_features(mc[:, 1:]), w, mu, cov))
        assert gap >= GAP, f'd = {d}, M = {M}, T = {T}: best and second-best log-density {gap:.3e} apart'
        got = cc.convert_mcep(ctx, model, M, mc)
        _same(got, golden[cc.mcep_key(d, M, T)], golden, f'd = {d}, M = {M}, T = {T}')
        assert np.array_equal(got[:, 0], mc[:, 0])
        _close(got, cc.ref_mcep(mc, w, mu, cov), f'mcep d = {d}, M = {M}, T = {T}')


def test_ragged_batch_bits_and_values(ctx, golden):
    d, M, Ts = cc.BATCH
    w, mu, cov = cc.mixture(3 * d, M, 1)
    rc, model = cc.prepare(ctx, d, w, mu, cov)
    assert rc == 0
    mcs = [cc.mcep(T, d, M, 1) for T in Ts]
    for mc in mcs:
        assert cc.logp_gap(cc.ref_logp(cc.delta_features(mc[:, 1:]), w, mu, cov)) >= GAP
    outs = cc.convert_mcep(ctx, model, M, mcs)
    for k, (mc, y) in enumerate(zip(mcs, outs)):
        _same(y, golden[f'batch_{k}'], golden, f'utterance {k} of the batch')
        assert np.array_equal(y, cc.convert_mcep(ctx, model, M, mc)), 'a batch equals its utterances one by one'
        _close(y, cc.ref_mcep(mc, w, mu, cov), f'utterance {k} of the batch')


@pytest.mark.parametrize('d,M,T', cc.REFUSED)
def test_widths_the_preparation_cannot_hold_are_refused_as_before(ctx, golden, d, M, T):
    """D = 144 (nine column blocks) and D = 150 (ten): wider than k_gmm_prep admits (D <= 82), so the recorded build
    and the tree refuse them before a kernel runs."""
    from kwiiyatta_amd import _lib
    w, mu, cov = cc.mixture(3 * d, M, 0)
    rc, model = cc.prepare(ctx, d, w, mu, cov)
    with pytest.raises(ValueError, match='too large'):
        cc.convert_mcep(ctx, model, M, cc.mcep(T, d, M, 0))
    assert [rc, _lib.KWY_EINVAL] == golden[f'refused_{d}'].tolist()


@pytest.mark.parametrize('fft,Ts', cc.MC2SP, ids=lambda v: str(v) if isinstance(v, int) else 'T')
def test_mc2sp_bits(ctx, golden, fft, Ts):
    mc = cc.mc2sp_rows(max(Ts))
    want = golden[f'mc2sp_{fft}']
    for T in Ts:
        _same(cc.mc2sp_sample(cc.mc2sp(ctx, mc[:T], fft)), want[:T], golden, f'mc2sp fft = {fft}, T = {T}')


@pytest.mark.parametrize('M,low,T', ((2, 0, 1), (2, 0, 17), (2, 0, 70), (66, 3, 17), (130, 67, 17)))
def test_equal_log_densities_pick_the_lower_index(ctx, M, low, T):
    """Mixtures low .. M - 1 have the same weight, x-mean and x-covariance: their log-densities are the same bits, those
    of the mixtures below are smaller, and a serial walk with `>` keeps mixture `low`.  Only mu_y and the y blocks of the
    covariance differ, so the output shows which one was used: it has to be, bit for bit, the conversion under mixture
    `low` alone.  M = 66 ties mixture 3 with mixture 65, which the arg-max meets in another lane's second pass; M = 130
    ties mixture 67, the second pass of lane 3, with 68 .. 129."""
    d = 24
    w, mu, cov = cc.mixture(3 * d, M, 2, equal_x=True, low=low)
    for m in range(1, M):
        assert np.array_equal(mu[0, :3 * d], mu[m, :3 * d]) and np.array_equal(cov[0, :3 * d, :3 * d], cov[m, :3 * d, :3 * d])
    assert (w[low:] == w[low]).all() and (w[:low] < w[low]).all()
    mc = cc.mcep(T, d, 2, 2)
    rc, model = cc.prepare(ctx, d, w, mu, cov)
    assert rc == 0
    got = cc.convert_mcep(ctx, model, M, mc)
    alone = []
    for m in (low, low + 1):
        rc, one = cc.prepare(ctx, d, np.ones(1), mu[m:m + 1], cov[m:m + 1])
        assert rc == 0
        alone.append(cc.convert_mcep(ctx, one, 1, mc))
    scale = np.abs(alone[0]).max()
    assert np.abs(alone[0] - alone[1]).max() > 1e-3 * scale, 'the two mixtures must convert differently'
    assert np.array_equal(got, alone[0])
    _close(got, cc.ref_mcep(mc, w, mu, cov, mix=low), f'tie, M = {M}, T = {T}')
