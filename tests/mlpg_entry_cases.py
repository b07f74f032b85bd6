"""Inputs and calls of tests/test_mlpg_entry_bits_gpu.py and of the recorder of its fixture
(tools/record_mlpg_entry_bits.py): every exported entry of the trajectory conversion (kwy_mlpg.hip) through the C ABI,
on the options em in {none, 0, 2} x gv in {none, 0 iterations, 4 iterations}, and the refusals of each entry with their
return code and message.  A plain module, so the recorder and the tests make the same calls on the same arrays.

Shapes: prepared models at (d, M) = (2, 3) and (24, 3); T = 1 and 17 are the one-chunk edge of the partitioned solve and
its first chunk boundary, 65 is one frame past the 64-frame tile of the E-step.  The batch entries take 17 utterances of
T = 1 .. 17 frames at d = 2: the second pass of KWY_BATCH_MAX = 16 holds a single utterance.

A case is (key, group, call): call(ctx) gives {output name: array}.  Buffers the library is to fill start as FILL, so
an output (or a part of one) the entry leaves alone compares equal too, and a refused call shows it wrote nothing.
"""
import ctypes
import functools

import numpy as np

import convert_cases as cc

SEED = 47
FILL = -4242.5
KWY_BATCH_MAX = 16
EM_MAX, GV_MAX = 16, 256
EMS = (-1, 0, 2)               # -1: none (the arg-max conversion)
GVS = (-1, 0, 4)               # -1: none (no ascent behind the conversion)
SHAPES = ((2, 3, 1.0, 7), (24, 3, 0.2, 8))      # (d, M, spread of the x-means, tag) as tests/em_cases.py
TS = (1, 17, 65)
BATCH_TS = tuple(range(1, 18))
HOST = ((2, 3, 1.0, 7, 17), (24, 3, 0.2, 8, 33))
FRAMES_D = 6


# ---- inputs -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixture(d, M, spread, tag):
    return cc.mixture(3 * d, M, tag, spread=spread)


@functools.lru_cache(maxsize=None)
def mcep(T, d, M, tag):
    return cc.mcep(T, d, M, tag)


def static(T, d, M, tag):
    return np.ascontiguousarray(mcep(T, d, M, tag)[:, 1:])


def gv_stats(d):
    """target mean and variance of the global variance per coefficient"""
    rng = np.random.default_rng([SEED, d])
    mean = rng.uniform(0.3, 0.9, d)
    return mean, (0.3 * mean) ** 2


_models = {}


def model(ctx, key):
    """the prepared model (d, M, spread, tag, diff) on the device; for a d the library refuses, zeros of the size a
    model would have"""
    import torch
    d, M, spread, tag, diff = key
    if key not in _models:
        rc, m = cc.prepare(ctx, d, *mixture(d, M, spread, tag), diff)
        if rc != 0:
            D = 3 * d
            m = torch.zeros((3 * D * D + 3 * D + 8) * M, dtype=torch.float64, device='cuda')
        _models[key] = m
    return _models[key]


# ---- the calls ------------------------------------------------------------------------------------------------------
def _lib():
    from kwiiyatta_amd import _lib
    return _lib


def _fill(shape, dtype=None):
    import torch
    return torch.full(tuple(shape), FILL if dtype is None else -1, dtype=dtype or torch.float64, device='cuda')


def _p(t, null, name):
    return None if name in null or t is None else t.data_ptr()


def _hp(a, null, name):
    return None if name in null or a is None else _lib().ptr(a)


def _finish(ctx, rc, outs):
    import torch
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in outs.items() if v is not None}


def mlpg_dev(ctx, x, w, mu, cov, diff=0, T=None, null=(), d=None):
    """kwy_gmm_mlpg_dev: the raw mixture on the device"""
    import torch
    dx, dw, dmu, dcov = cc._dev(x, w, mu, cov)
    y = _fill(x.shape)
    torch.cuda.synchronize()
    rc = _lib().lib.kwy_gmm_mlpg_dev(ctx.handle, _p(dx, null, 'x'), x.shape[0] if T is None else T,
                                     x.shape[1] if d is None else d, len(w), _p(dw, null, 'w'), _p(dmu, null, 'mu'),
                                     _p(dcov, null, 'cov'), diff, _p(y, null, 'y'))
    return _finish(ctx, rc, {'y': y})


def mlpg_model_dev(ctx, x, mdl, M, T=None, null=()):
    """kwy_gmm_mlpg_model_dev: packed rows, a prepared model (mdl: the key of `model`, here and below)"""
    import torch
    mdl = model(ctx, mdl)
    dx, = cc._dev(x)
    y = _fill(x.shape)
    torch.cuda.synchronize()
    rc = _lib().lib.kwy_gmm_mlpg_model_dev(ctx.handle, _p(dx, null, 'x'), x.shape[0] if T is None else T, x.shape[1], M,
                                           _p(mdl, null, 'model'), _p(y, null, 'y'))
    return _finish(ctx, rc, {'y': y})


def convert_dev(ctx, mc, mdl, M, em=-1, gv=-1, offset=0, weight=1.0, stats=None, outputs=True, T=None, null=()):
    """one utterance through the device entry its options select: kwy_convert_mcep_dev (no em, no gv),
    kwy_convert_mcep_em_dev (em, no gv), kwy_convert_mcep_gv_dev (gv); outputs=False passes null for the optional
    loglik / objective / status"""
    import torch
    lib = _lib().lib
    mdl = model(ctx, mdl)
    d = mc.shape[1] - 1
    n = mc.shape[0] if T is None else T
    din, = cc._dev(mc)
    out = _fill(mc.shape)
    outs = {'mc_out': out}
    torch.cuda.synchronize()
    if gv == -1 and em == -1:
        rc = lib.kwy_convert_mcep_dev(ctx.handle, _p(din, null, 'x'), n, d, M, _p(mdl, null, 'model'), _p(out, null, 'y'))
        return _finish(ctx, rc, outs)
    lik = _fill((max(min(em, EM_MAX), 0) + 1,)) if outputs else None
    outs['loglik'] = lik
    if gv == -1:
        rc = lib.kwy_convert_mcep_em_dev(ctx.handle, _p(din, null, 'x'), n, d, M, _p(mdl, null, 'model'), em,
                                         _p(out, null, 'y'), _p(lik, null, 'loglik'))
        return _finish(ctx, rc, outs)
    mean, var = gv_stats(d) if stats is None else stats
    dm, dv = cc._dev(mean, var)
    obj = _fill((max(min(gv, GV_MAX), 0) + 1,)) if outputs else None
    status = _fill((1,), torch.int32) if outputs else None
    outs.update(objective=obj, status=status)
    torch.cuda.synchronize()
    rc = lib.kwy_convert_mcep_gv_dev(ctx.handle, _p(din, null, 'x'), n, d, M, _p(mdl, null, 'model'), em, offset,
                                     _p(dm, null, 'gv_mean'), _p(dv, null, 'gv_var'), weight, gv, _p(out, null, 'y'),
                                     _p(lik, null, 'loglik'), _p(obj, null, 'objective'), _p(status, null, 'status'))
    return _finish(ctx, rc, outs)


def convert_batch(ctx, mcs, mdl, M, em=-1, gv=-1, offset=0, weight=1.0, realign=False, Ts=None, null=(), count=None,
                  null_job=None):
    """a list of utterances through the batch entry the options select: kwy_convert_mcep_batch_dev,
    kwy_realign_features_batch_dev (realign: rows of d + 2, columns 2.. written), kwy_convert_mcep_em_batch_dev,
    kwy_convert_mcep_gv_batch_dev.  The outputs are those of the utterances one under the other.  Ts: the frame counts
    the jobs state; null_job: (index, field) of a job pointer passed as null"""
    import torch
    L = _lib()
    lib = L.lib
    mdl = model(ctx, mdl)
    d = mcs[0].shape[1] - 1
    ins = cc._dev(*mcs)
    Ts = [a.shape[0] for a in ins] if Ts is None else Ts
    outs = [_fill((a.shape[0], d + 2 if realign else d + 1)) for a in ins]
    liks = [_fill((max(em, 0) + 1,)) for _ in ins]
    objs = [_fill((max(gv, 0) + 1,)) for _ in ins]
    status = _fill((len(ins),), torch.int32)

    def ptr(j, name, t):
        return None if null_job == (j, name) else t
    res = {'out': outs}
    if gv != -1:
        struct = L.ConvertGvJob
        rows = [(ptr(j, 'mc', a), T, ptr(j, 'out', o), l, q) for j, (a, T, o, l, q) in enumerate(zip(ins, Ts, outs, liks, objs))]
        res.update(loglik=liks, objective=objs)
    elif em != -1:
        struct = L.ConvertEmJob
        rows = [(ptr(j, 'mc', a), T, ptr(j, 'out', o), l) for j, (a, T, o, l) in enumerate(zip(ins, Ts, outs, liks))]
        res.update(loglik=liks)
    else:
        struct = L.RealignJob if realign else L.ConvertJob
        rows = [(ptr(j, 'mc', a), T, ptr(j, 'out', o)) for j, (a, T, o) in enumerate(zip(ins, Ts, outs))]
    jobs = None if 'jobs' in null else ctypes.cast(L.job_array(struct, rows), ctypes.c_void_p)
    n = len(ins) if count is None else count
    m = _p(mdl, null, 'model')
    torch.cuda.synchronize()
    if gv != -1:
        dm, dv = cc._dev(*gv_stats(d))
        torch.cuda.synchronize()
        rc = lib.kwy_convert_mcep_gv_batch_dev(ctx.handle, jobs, n, d, M, m, em, offset, _p(dm, null, 'gv_mean'),
                                               _p(dv, null, 'gv_var'), weight, gv, _p(status, null, 'status'))
    elif em != -1:
        rc = lib.kwy_convert_mcep_em_batch_dev(ctx.handle, jobs, n, d, M, m, em)
    elif realign:
        rc = lib.kwy_realign_features_batch_dev(ctx.handle, jobs, n, d, M, m)
    else:
        rc = lib.kwy_convert_mcep_batch_dev(ctx.handle, jobs, n, d, M, m)
    torch.cuda.synchronize()
    got = {k: np.concatenate([t.cpu().numpy() for t in v]) for k, v in res.items()}
    if gv != -1:
        got['status'] = status.cpu().numpy()
    return rc, got


def mlpg_host(ctx, x, w, mu, cov, diff=0, em=-1, gv=-1, offset=0, weight=1.0, stats=None, T=None, null=()):
    """host pointers through the entry the options select: kwy_gmm_mlpg, kwy_gmm_mlpg_em, kwy_gmm_mlpg_gv"""
    L = _lib()
    x, w, mu, cov = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, w, mu, cov))
    n, d, M = x.shape[0] if T is None else T, x.shape[1], len(w)
    y = np.full(x.shape, FILL)
    outs = {'y': y}
    head = (ctx.handle, _hp(x, null, 'x'), n, d, M, _hp(w, null, 'w'), _hp(mu, null, 'mu'), _hp(cov, null, 'cov'), diff)
    if gv == -1 and em == -1:
        return L.lib.kwy_gmm_mlpg(*head, _hp(y, null, 'y')), outs
    lik = outs['loglik'] = np.full(max(min(em, EM_MAX), 0) + 1, FILL)
    if gv == -1:
        return L.lib.kwy_gmm_mlpg_em(*head, em, _hp(y, null, 'y'), _hp(lik, null, 'loglik')), outs
    mean, var = (np.ascontiguousarray(a) for a in (gv_stats(d) if stats is None else stats))
    obj = outs['objective'] = np.full(max(min(gv, GV_MAX), 0) + 1, FILL)
    status = outs['status'] = np.full(1, -1, dtype=np.int32)
    rc = L.lib.kwy_gmm_mlpg_gv(*head, em, offset, _hp(mean, null, 'gv_mean'), _hp(var, null, 'gv_var'), weight, gv,
                               _hp(y, null, 'y'), _hp(lik, null, 'loglik'), _hp(obj, null, 'objective'),
                               _hp(status, null, 'status'))
    return rc, outs


def frames(ctx, x, w, mu, cov, diff=0, host=True, T=None, null=()):
    """kwy_gmm_convert_frames (host pointers) / kwy_gmm_convert_frames_dev"""
    import torch
    L = _lib()
    n, D, M = x.shape[0] if T is None else T, x.shape[1], len(w)
    if host:
        x, w, mu, cov = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, w, mu, cov))
        y = np.full(x.shape, FILL)
        return L.lib.kwy_gmm_convert_frames(ctx.handle, _hp(x, null, 'x'), n, D, M, _hp(w, null, 'w'), _hp(mu, null, 'mu'),
                                            _hp(cov, null, 'cov'), diff, _hp(y, null, 'y')), {'y': y}
    dx, dw, dmu, dcov = cc._dev(x, w, mu, cov)
    y = _fill(x.shape)
    torch.cuda.synchronize()
    rc = L.lib.kwy_gmm_convert_frames_dev(ctx.handle, _p(dx, null, 'x'), n, D, M, _p(dw, null, 'w'), _p(dmu, null, 'mu'),
                                          _p(dcov, null, 'cov'), diff, _p(y, null, 'y'))
    return _finish(ctx, rc, {'y': y})


# ---- the cases ------------------------------------------------------------------------------------------------------
def _opt(em, gv):
    return f'em{"none" if em < 0 else em}_gv{"none" if gv < 0 else gv}'


def _dev_case(n, d, M, s, tag, diff=0, **kw):
    return lambda ctx: convert_dev(ctx, mcep(n, d, M, tag), (d, M, s, tag, diff), M, **kw)


def _batch_case(lengths, d, M, s, tag, diff=0, **kw):
    return lambda ctx: convert_batch(ctx, [mcep(n, d, M, tag) for n in lengths], (d, M, s, tag, diff), M, **kw)


def _host_case(n, d, M, s, tag, **kw):
    return lambda ctx: mlpg_host(ctx, static(n, d, M, tag), *mixture(d, M, s, tag), **kw)


def _mlpg_dev_case(n, d, M, s, tag, **kw):
    return lambda ctx: mlpg_dev(ctx, static(n, d, M, tag), *mixture(d, M, s, tag), **kw)


def _mlpg_model_dev_case(n, d, M, s, tag, **kw):
    return lambda ctx: mlpg_model_dev(ctx, static(n, d, M, tag), (d, M, s, tag, 0), M, **kw)


def _frames_case(**kw):
    def call(ctx):
        w, mu, cov, X = cc.frames_case(FRAMES_D, 3)
        return frames(ctx, np.ascontiguousarray(X[:17]), w, mu, cov, **kw)
    return call


def _cases():
    out = []
    for d, M, s, tag in SHAPES:
        g = f'single_d{d}'
        for T in TS:
            for em in EMS:
                for gv in GVS:
                    out.append((f'dev_d{d}_T{T}_{_opt(em, gv)}', g, _dev_case(T, d, M, s, tag, em=em, gv=gv)))
            out.append((f'mlpg_dev_d{d}_T{T}', g, _mlpg_dev_case(T, d, M, s, tag)))
            out.append((f'mlpg_model_dev_d{d}_T{T}', g, _mlpg_model_dev_case(T, d, M, s, tag)))
    # null loglik / objective / status; a diff = 1 model with the source as the ascent's offset and a weight of 2
    small = SHAPES[0]
    for em, gv in ((2, -1), (2, 4), (-1, 4)):
        out.append((f'dev_nulls_{_opt(em, gv)}', 'single_d2', _dev_case(17, *small, em=em, gv=gv, outputs=False)))
        if gv != -1:
            out.append((f'dev_offset_{_opt(em, gv)}', 'single_d2',
                        _dev_case(17, *small, diff=1, em=em, gv=gv, offset=1, weight=2.0)))
    for em in EMS:
        for gv in GVS:
            out.append((f'batch_{_opt(em, gv)}', 'batch', _batch_case(BATCH_TS, *small, diff=1, em=em, gv=gv, offset=1)))
    out.append(('batch_realign', 'batch', _batch_case(BATCH_TS, *small, realign=True)))
    for d, M, s, tag, T in HOST:
        for diff in (0, 1):
            for em in EMS:          # kwy_gmm_mlpg (none, none), kwy_gmm_mlpg_em (em, none), kwy_gmm_mlpg_gv (any, gv)
                for gv in GVS:
                    out.append((f'host_d{d}_diff{diff}_{_opt(em, gv)}', 'host',
                                _host_case(T, d, M, s, tag, diff=diff, em=em, gv=gv, offset=diff)))
    for diff in (0, 1):
        for host in (True, False):
            out.append((f'frames_{"host" if host else "dev"}_diff{diff}', 'frames', _frames_case(diff=diff, host=host)))
    return out


# ---- the refusals ------------------------------------------------------------------------------------------------------
# what is wrong -> keyword arguments of the calls above; `d` stands for inputs made at that static dimension
_BAD = (
    ('null_x', dict(null=('x',))),
    ('null_y', dict(null=('y',))),
    ('null_model', dict(null=('model',))),
    ('T0', dict(T=0)),
    ('d65', dict(d=65)),
    ('d48', dict(d=48)),
    ('em17', dict(em=17)),
    ('em_below', dict(em=-2)),
    ('gv257', dict(gv=257)),
    ('gv_below', dict(gv=-2)),
    ('weight0', dict(weight=0.0)),
    ('weight_negative', dict(weight=-1.0)),
    ('weight_nan', dict(weight=float('nan'))),
    ('null_gv_mean', dict(null=('gv_mean',))),
    # several at once: which one the message names
    ('T0_em17', dict(T=0, em=17)),
    ('em17_d48', dict(em=17, d=48)),
    ('em17_gv257', dict(em=17, gv=257)),
    ('d48_gv257', dict(d=48, gv=257)),
    ('weight0_gv257', dict(weight=0.0, gv=257)),
    ('null_gv_mean_weight0', dict(null=('gv_mean',), weight=0.0)),
)
_BASE = {'plain': (-1, -1), 'em': (2, -1), 'gv': (2, 4), 'gv_argmax': (-1, 4)}       # (em, gv) of an entry's good call


def _refusal(kind, options, kw):
    """the call of one refusal, or None where the entry has no such argument"""
    kw = dict(kw)
    d = kw.pop('d', 2)
    M, s, tag, T = 3, 1.0, 7, 17
    em, gv = _BASE[options]
    null = kw.pop('null', ())
    if ('em' in kw and em == -1) or (('gv' in kw or 'weight' in kw or 'gv_mean' in null) and gv == -1):
        return None
    kw.setdefault('em', em)
    kw.setdefault('gv', gv)
    if kind == 'host':
        return _host_case(T, d, M, s, tag, null=tuple('cov' if n == 'model' else n for n in null), **kw)
    if kind == 'dev':
        return _dev_case(T, d, M, s, tag, null=null, **kw)
    # a batch of 17 whose last job (the only one of the second pass) carries what is wrong
    if 'T' in kw:
        kw['Ts'] = list(BATCH_TS[:-1]) + [kw.pop('T')]
    for name, field in (('x', 'mc'), ('y', 'out')):
        if name in null:
            kw['null_job'] = (len(BATCH_TS) - 1, field)
    return _batch_case(BATCH_TS, d, M, s, tag, null=tuple(n for n in null if n not in ('x', 'y')), **kw)


def _refusals():
    out = []
    for kind in ('dev', 'batch', 'host'):
        for options in _BASE:
            for what, kw in _BAD:
                call = _refusal(kind, options, kw)
                if call is not None:
                    out.append((f'refuse_{kind}_{options}_{what}', call))
    small = SHAPES[0]
    for name, o in (('plain', {}), ('realign', dict(realign=True)), ('em', dict(em=2)), ('gv', dict(em=2, gv=4))):
        for what, kw in (('null_jobs', dict(null=('jobs',))), ('count_negative', dict(count=-1))):
            out.append((f'refuse_batch_{name}_{what}', _batch_case(BATCH_TS[:3], *small, **o, **kw)))
    out.append(('refuse_batch_realign_T0', _batch_case(BATCH_TS[:3], *small, realign=True, Ts=[1, 2, 0])))
    out.append(('refuse_batch_realign_null_feat', _batch_case(BATCH_TS[:3], *small, realign=True, null_job=(1, 'out'))))
    for what, kw in (('null_x', dict(null=('x',))), ('null_w', dict(null=('w',))), ('null_y', dict(null=('y',))),
                     ('T0', dict(T=0))):
        out.append((f'refuse_mlpg_dev_{what}', _mlpg_dev_case(17, *small, **kw)))
        if what != 'null_w':
            out.append((f'refuse_mlpg_model_dev_{what}', _mlpg_model_dev_case(17, *small, **kw)))
        for host in (True, False):
            out.append((f'refuse_frames_{"host" if host else "dev"}_{what}', _frames_case(host=host, **kw)))
    out.append(('refuse_mlpg_model_dev_null_model', _mlpg_model_dev_case(17, *small, null=('model',))))
    for d in (65, 48):
        out.append((f'refuse_mlpg_dev_d{d}', _mlpg_dev_case(17, d, *small[1:])))
        out.append((f'refuse_mlpg_model_dev_d{d}', _mlpg_model_dev_case(17, d, *small[1:])))
    return out


CASES = _cases()
REFUSALS = _refusals()
GROUPS = tuple(dict.fromkeys(g for _, g, _ in CASES))


# ---- the fixture -----------------------------------------------------------------------------------------------------
# Every output of every case is kept, as doubles (the status words are small integers).  Many outputs repeat another's
# bits -- no ascent steps leave the conversion's rows as they were, kwy_gmm_mlpg_dev and kwy_gmm_mlpg_model_dev run the
# same kernels -- so the values live once in one vector and an index names, per output, where its copy starts.
def pack(results):
    """{case key: {output name: array}} -> the arrays of the fixture: `data`, and per output `index_names`
    ('key.name' joined by newlines), `index_offset` and `index_size` into data"""
    data, seen, names, offsets, sizes, end = [], {}, [], [], [], 0
    for key, outs in results.items():
        for name in sorted(outs):
            v = np.ascontiguousarray(outs[name], dtype=np.float64).ravel()
            at = seen.get(v.tobytes())
            if at is None:
                at = seen[v.tobytes()] = end
                data.append(v)
                end += v.size
            names.append(f'{key}.{name}')
            offsets.append(at)
            sizes.append(v.size)
    return dict(data=np.concatenate(data), index_names=np.array('\n'.join(names).encode()),
                index_offset=np.array(offsets, dtype=np.int32), index_size=np.array(sizes, dtype=np.int32))


def unpack(golden):
    """the fixture's arrays -> {case key: {output name: vector}}"""
    data, out = golden['data'], {}
    names = bytes(golden['index_names']).decode().split('\n')
    for full, at, size in zip(names, golden['index_offset'], golden['index_size']):
        key, name = full.rsplit('.', 1)
        out.setdefault(key, {})[name] = data[at:at + size]
    return out


def refusal_digest():
    """a digest of the refusals' names in their order: the fixture keeps their results by position"""
    import hashlib
    return hashlib.sha1('\n'.join(k for k, _ in REFUSALS).encode()).hexdigest()


def run_case(ctx, call):
    rc, outs = call(ctx)
    assert rc == 0, (rc, ctx.error())
    return outs


def run_refusal(ctx, call):
    """(return code, the message, whether every output buffer still holds what it was filled with)"""
    rc, outs = call(ctx)
    clean = all((v == (FILL if v.dtype == np.float64 else -1)).all() for v in outs.values())
    return rc, (ctx.error() if rc != 0 else ''), clean
