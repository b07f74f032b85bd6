"""The work a `corpus.ConvertWave` enqueues, call by call, against a recording of the commit before the conversion
drivers were rewritten around `ConvertOptions` (tests/data/convert_wave_calls.json), and the memory the lockstep driver
holds on to while the MLSA recursions of a batch wait for its last wave.

A call is recorded as [name, 'main' | 'side' (the context whose handle it was given), argument, ...]: an int or float
argument as its value, a pointer argument as 'null' or 'ptr' (include/kwy.h's types, from _lib.SIGNATURES).  Calls
without a context -- the size queries of the constructor -- enqueue nothing and are not recorded.
`python tests/test_convert_trace_gpu.py` rewrites the recording from the code as it stands."""
import ctypes
import gc
import json
import os
import weakref

import numpy as np
import pytest

import convert_cases as cc

pytestmark = pytest.mark.gpu

FS, ORDER, MS_LENGTH = 16000, 24, 512          # (the shortest transform there is; 0.4 s are 81 frames)
RECORDING = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'convert_wave_calls.json')


def _waveforms(n=2):
    from kwiiyatta_amd.synthetic import make_utterance
    return [make_utterance(seed=60 + i, fs=FS, seconds=(0.25, 0.4)[i % 2], f0_base=(140.0, 190.0)[i % 2])[0]
            for i in range(n)]


def _mixture():
    from types import SimpleNamespace
    w, mu, cov = cc.mixture(3 * ORDER, 2, 5)
    return SimpleNamespace(weights_=w, means_=mu, covariances_=cov)


def _statistics():
    rng = np.random.default_rng(17)
    gv = dict(gv_stats=rng.uniform(0.05, 0.5, ORDER + 1), gv_var=rng.uniform(0.001, 0.01, ORDER + 1))
    triples = np.zeros((2, ORDER + 1, MS_LENGTH // 2 + 1, 3))
    triples[..., 0], triples[..., 1], triples[..., 2] = 10.0, rng.standard_normal(triples.shape[:-1]), 10.0
    return gv, dict(ms_stats=(triples[0], triples[1]), ms_length=MS_LENGTH)


def _cases():
    gv, ms = _statistics()
    gmm, diff = dict(gmm=True), dict(gmm=True, diff=True)
    return {
        'no gmm': {},
        'no gmm, formant_ratio': dict(formant_ratio=1.2),
        'gmm': gmm,
        'diff': diff,
        'diff, gv': dict(diff, gv_stats=gv['gv_stats'], gv_strength=1.0),
        'diff, ms': dict(diff, ms_strength=0.5, **ms),
        'diff, ms, gv': dict(diff, ms_strength=0.5, gv_stats=gv['gv_stats'], gv_strength=0.75, **ms),
        'diff, mlpg_em': dict(diff, mlpg_em=2),
        'diff, mlpg_gv, mlpg_em': dict(diff, mlpg_gv=3, mlpg_em=1, gv_weight=2.0, **gv),
        'diff, postfilter_beta, keep_power': dict(diff, postfilter_beta=0.25, keep_power=True),
        'diff, gv, keep_power, fft': dict(diff, gv_stats=gv['gv_stats'], gv_strength=1.0, keep_power=True,
                                          diff_filter='fft'),
        'f0_stats, transpose_key': dict(gmm, f0_stats=(5.0, 0.2, 5.3, 0.25), transpose_key=2.0),
        'pcm, diff, defer_mlsa': dict(diff, pcm=True, defer_mlsa=True),
    }


class _Recorder:
    """stands in for `corpus.lib`: every kwy_* call that is given one of the lockstep contexts is noted, then made"""

    def __init__(self, lib, ls, calls):
        self._lib, self._calls = lib, calls
        self._contexts = {ls.ctx.handle.value: 'main', ls.side_ctx.handle.value: 'side'}

    def __getattr__(self, name):
        from kwiiyatta_amd import _lib
        fn = getattr(self._lib, name)
        if not name.startswith('kwy_') or name not in _lib.SIGNATURES:
            return fn
        argtypes = _lib.SIGNATURES[name][1]

        def call(*args):
            where = self._contexts.get(getattr(args[0], 'value', args[0])) if args else None
            if where is not None:
                assert len(args) == len(argtypes), name
                self._calls.append([name, where] + [_noted(a, t) for a, t in zip(args[1:], argtypes[1:])])
            return fn(*args)
        return call


def _noted(arg, argtype):
    if argtype is ctypes.c_double:
        return float(arg)
    if argtype in (ctypes.c_int, ctypes.c_int64):
        return int(arg)
    if isinstance(arg, ctypes.c_void_p):
        arg = arg.value
    return 'null' if arg is None or (isinstance(arg, int) and arg == 0) else 'ptr'


def record_wave(monkeypatch, waves, mixture, gmm=False, **options):
    """the calls one ConvertWave(waves, ...) enqueues from its construction to the end of run()"""
    import torch
    from kwiiyatta_amd import corpus
    ls = corpus._Lockstep(0)
    dg = corpus.DeviceGMM(mixture.weights_, mixture.means_, mixture.covariances_, torch.device('cuda', 0)) if gmm else None
    calls = []
    with monkeypatch.context() as m:
        m.setattr(corpus, 'lib', _Recorder(corpus.lib, ls, calls))
        corpus.ConvertWave(ls, FS, waves, gmm=dg, order=ORDER, **options).run()
    ls.sync()
    return json.loads(json.dumps(calls))


def test_a_wave_enqueues_the_calls_it_did_before_the_options_record(monkeypatch):
    with open(RECORDING) as f:
        recorded = json.load(f)
    cases = _cases()
    assert sorted(recorded) == sorted(cases)
    waves, mixture = _waveforms(), _mixture()
    for name, options in cases.items():
        got = record_wave(monkeypatch, waves, mixture, **options)
        assert len(got) >= 5, name
        for i, (a, b) in enumerate(zip(got, recorded[name])):
            assert a == b, (name, i)
        assert len(got) == len(recorded[name]), name


def test_a_deferred_mlsa_pass_does_not_keep_the_waves(monkeypatch):
    """diff=True with the MLSA filter: the recursions of all files wait for the last wave, and all that waits with them
    is each wave's `_DeferredMlsa` record.  (Before the record the driver kept every whole wave until then -- on that
    code the first wave's aperiodicities are still alive in the fourth wave's callback and this test fails.)  The
    outputs do not depend on how the files are cut into waves."""
    import torch
    from kwiiyatta_amd import corpus
    from kwiiyatta_amd._convert_options import ConvertOptions
    waves, mixture = _waveforms(4), _mixture()
    dg = corpus.DeviceGMM(mixture.weights_, mixture.means_, mixture.covariances_, torch.device('cuda', 0))
    alive, built = [], corpus.ConvertWave.__init__

    def init(self, *args, **kwargs):
        built(self, *args, **kwargs)
        alive.append(weakref.ref(self.ap_all))
    monkeypatch.setattr(corpus.ConvertWave, '__init__', init)

    def run(wave_size, seen):
        out = [None] * len(waves)

        def keep(i, wave, pcm, wave_diff, pcm_diff):
            out[i] = wave_diff
            if i == 3 and seen is not None:
                gc.collect()
                seen.append(alive[0]() is None)
        corpus._lockstep_batch(waves, FS, 0, dg, ORDER, 5.0, None, keep, ConvertOptions().check(ORDER),
                               wave_size=wave_size, diff=True)
        return [w.cpu().numpy().tobytes() for w in out]
    seen = []
    one_by_one = run(1, seen)
    assert len(alive) == 4 and seen == [True]
    assert one_by_one == run(16, None)


if __name__ == '__main__':
    with pytest.MonkeyPatch.context() as patch:
        out = {name: record_wave(patch, _waveforms(), _mixture(), **options) for name, options in _cases().items()}
    with open(RECORDING, 'w') as f:
        f.write('{\n' + ',\n'.join(f' {json.dumps(k)}: [\n' + ',\n'.join('  ' + json.dumps(c) for c in v) + '\n ]'
                                   for k, v in out.items()) + '\n}\n')
    print({k: len(v) for k, v in out.items()})
