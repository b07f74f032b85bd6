"""Corpus-level path (BASELINE config 5): a parallel corpus -> joint training matrix in HBM -> converter
fit -> batch conversion, without the features ever visiting the host.

What the reference does for `kwiiyatta --source A --target B files...`
(/root/reference/kwiiyatta/config.py:83-104, convert_voice.py:6-46):

  per pair    analyse both sides; TrimmedDataset; align_even (pad 100 silent frames, DTW features with
              vuv='voiced' and a binarised power term, FastDTW radius 32, strict path filter, cut to the
              un-padded stretch); mel-cepstra of the aligned frames without c0; delta features;
              np.hstack + remove_zeros_frames; rows appended to one array (make_dataset_to_array)
  fit         GaussianMixture(n_components, covariance_type='full', max_iter=100, random_state=seed)
  per file    analyse; convert the mel-cepstrum (delta + GMM posterior + MLPG, c0 kept); synthesise

Here waves of up to 16 pairs run in lockstep through the batched entries on two HIP streams (`TrainWave`; the
pair-per-stream driver `TrainPair` remains as driver='streams'), ranks take contiguous blocks of pairs (the global
row order is the pair order whatever the number of ranks), the rows land in one device tensor that
`GaussianMixtureHIP.fit` uses as its shard, and the fitted model converts utterances wave by wave (`ConvertWave`;
stream-parallel with `ConvertPipeline`).  The only collectives are those of the fit.  Training, re-alignment and
evaluation share the lockstep pair path: a wave hands its `_AlignInputs` to an `_Alignment` (FastDTW, the rows of the
kept path, its index lists, its monitor), the rows go into a `_RowSink`, and an `_Ahead` thread prepares what the host
would otherwise wait for.

The silence padding of `align_even` draws from numpy's GLOBAL legacy generator in the reference
(kwiiyatta/vocoder/world.py:158-161, quirk kept): the draws are made on the host, in the reference's order
(source head, source tail, target head, target tail, pair after pair), and uploaded once per pair -- so this path
and the Python API path produce the same matrix under `np.random.seed`.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._blocks import Ragged, p as _p, to_device
from ._convert_options import ConvertOptions, takes_options
from ._lib import lib
from .pipeline import (PAD_LEN, PIECE_CEILING, POWER_THRESHOLD, POWER_WEIGHT, SAFE_GUARD_MINIMUM, VUV_WEIGHT, DeviceGMM,
                       _Graphed, _Side, check_f0_estimator, check_f0_status, coarse_f0_batch_dev, draw_silence, f0_jobs)

TRIM_EPS = 1e-7       # nnmnkwii trim_zeros_frames / remove_zeros_frames


class TrainPair:
    """One parallel pair -> its rows of the training matrix, on one stream.

        p.analyse()   enqueue CheapTrick + D4C of both sides and the trim lengths
        p.align()     (reads the two trim lengths: one 16-byte D2H) enqueue everything else
        p.rows()      (synchronises) the pair's joint rows, an (n, 2*3*order) device tensor
    """

    def __init__(self, device_index, fs, source, target, order=24, radius=32, frame_period=5.0, stream=None,
                 silence=None, ctx=None, silence_ready=None):
        """silence: the four (100, K) pad spectra (source head, source tail, target head, target tail) as numpy arrays
        or device tensors (then `silence_ready`: an event after which they are valid); default: drawn here from
        numpy's global generator in that order"""
        self.dev = torch.device('cuda', device_index)
        self.fs, self.order, self.radius, self.frame_period = int(fs), int(order), int(radius), float(frame_period)
        self.stream = stream if stream is not None else torch.cuda.Stream(device=self.dev)
        self.ctx = ctx if ctx is not None else _lib.Context(device_index, stream=self.stream.cuda_stream)
        self.fft = lib.kwy_cheaptrick_fft_size(self.fs, 71.0)
        self.K = self.fft // 2 + 1
        from .backend import sptk
        self.alpha = sptk.mcepalpha(self.fs)
        if silence is None:        # the reference's order of draws: source head, source tail, target head, tail
            silence = [draw_silence(self.fs, self.K) for _ in range(4)]
        with torch.cuda.stream(self.stream):
            # (align() writes all rows of the padded envelope it reads, and fills f0_pad's middle at the trimmed length)
            self.src, self.tgt = (_Side(*u, self.K, self.dev, sp_alloc=torch.empty) for u in (source, target))
            for s in (self.src, self.tgt):
                s.n_keep_dev = torch.zeros(1, dtype=torch.int64, device=self.dev)
                s.n = None          # frames kept by TrimmedDataset (host int, after analyse + sync)
            if silence_ready is not None:
                self.stream.wait_event(silence_ready)
            self.silence = [to_device(s, self.dev) for s in silence]
            # tensors made on other streams (the upload helper's, the generator's) are used on this one: the allocator
            # must not hand their memory out again while this stream's work on them is still queued
            for t_ in (self.src.x, self.src.f0, self.src.t, self.tgt.x, self.tgt.f0, self.tgt.t, *self.silence):
                t_.record_stream(self.stream)
        self.frames = self.src.T
        self.n_rows = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.joint = None

    def _chk(self, rc):
        _lib.check(self.ctx, rc)

    def analyse(self):
        h, fs, fft, K = self.ctx.handle, self.fs, self.fft, self.K
        with torch.cuda.stream(self.stream):
            for s in (self.src, self.tgt):
                self._chk(lib.kwy_cheaptrick_dev(h, _p(s.x), s.N, fs, _p(s.t), _p(s.f0), s.T, -0.15, 71.0, fft,
                                                 float(fs), _p(s.sp)))
                self._chk(lib.kwy_d4c_dev(h, _p(s.x), s.N, fs, _p(s.t), _p(s.f0), s.T, 0.85, fft, _p(s.ap)))
                self._chk(lib.kwy_trim_length_dev(h, _p(s.sp), s.T, K, TRIM_EPS, _p(s.n_keep_dev)))

    def align(self):
        h, fs, K, order, P = self.ctx.handle, self.fs, self.K, self.order, PAD_LEN
        f64 = dict(dtype=torch.float64, device=self.dev)
        i32 = dict(dtype=torch.int32, device=self.dev)
        with torch.cuda.stream(self.stream):
            keep = torch.cat((self.src.n_keep_dev, self.tgt.n_keep_dev)).cpu().tolist()   # waits for the analysis
            for s, n, sil in ((self.src, keep[0], self.silence[:2]), (self.tgt, keep[1], self.silence[2:])):
                s.n = int(n)
                s.feature_rows(s.n + 2 * P, order)       # (the side's Tp is the trimmed one from here on)
                # pad_silence on the first n frames (TrimmedDataset keeps feature[:n])
                s.sp_pad[:P].copy_(sil[0])
                s.sp_pad[P + s.n:s.Tp].copy_(sil[1])
                s.ap_pad[P + s.n:s.Tp].fill_(1 - SAFE_GUARD_MINIMUM)
                s.f0_pad[P:P + s.n].copy_(s.f0[:s.n])
                s.voiced = torch.empty(s.Tp, **f64)
                self._chk(lib.kwy_is_voiced_dev(h, _p(s.f0_pad), _p(s.ap_pad), s.Tp, K, fs, _p(s.voiced)))
                self._chk(lib.kwy_sp2mc_dev(h, _p(s.sp_pad), s.Tp, K, order, self.alpha, _p(s.mc_pad)))
                # make_feature(vuv='voiced', power='binalize', power_pivot='max')
                self._chk(lib.kwy_align_features_dev(h, _p(s.mc_pad), s.Tp, order + 1, _p(s.voiced), POWER_WEIGHT,
                                                     POWER_THRESHOLD, VUV_WEIGHT, _p(s.feat)))
            a, b = self.src, self.tgt
            cap = a.Tp + b.Tp + 2
            self.cap = cap
            self.path = torch.zeros((cap, 2), **i32)
            self.path_len = torch.zeros(1, dtype=torch.int64, device=self.dev)
            self.dist = torch.zeros(1, **f64)
            self.idx_x, self.idx_y = torch.zeros(cap, **i32), torch.zeros(cap, **i32)
            self.n_sel = torch.zeros(1, dtype=torch.int64, device=self.dev)
            self._chk(lib.kwy_fastdtw_dev(h, _p(a.feat), a.Tp, _p(b.feat), b.Tp, order + 2, self.radius, _p(self.dist),
                                          _p(self.path), _p(self.path_len)))
            # dtw_feature(strict=True) + align_even's cut
            self._chk(lib.kwy_align_even_dev(h, _p(self.path), _p(self.path_len), _p(a.feat), _p(b.feat), order + 2,
                                             1, 1, 1, a.Tp, b.Tp, P, _p(self.idx_x), _p(self.idx_y), cap,
                                             _p(self.n_sel)))
            halves = []
            for s, idx in ((a, self.idx_x), (b, self.idx_y)):
                mc_sel = torch.empty((cap, order + 1), **f64)
                self._chk(lib.kwy_gather_rows_dev(h, _p(s.mc_pad), s.Tp, order + 1, _p(idx), cap, _p(mc_sel)))
                static = mc_sel[:, 1:].contiguous()                        # drop the power coefficient
                delta = torch.empty((cap, 3 * order), **f64)
                self._chk(lib.kwy_delta_features_dev(h, _p(static), _p(self.n_sel), cap, order, _p(delta)))
                halves.append(delta)
            self.joint = torch.empty((cap, 6 * order), **f64)
            self._chk(lib.kwy_joint_rows_dev(h, _p(halves[0]), _p(halves[1]), _p(self.n_sel), cap, 3 * order, TRIM_EPS,
                                             _p(self.joint), _p(self.n_rows)))
            self._halves = halves        # alive until the stream is done with them

    def rows(self):
        with torch.cuda.stream(self.stream):
            n = int(self.n_rows.item())
            return self.joint[:n]


class _Lockstep:
    """Two streams with a library context each, shared by all waves of a lockstep driver (the default four hardware
    queues of the HIP runtime are enough: no GPU_MAX_HW_QUEUES)."""

    def __init__(self, device_index):
        self.dev = torch.device('cuda', device_index)
        self.main, self.side = torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)
        self.ctx = _lib.Context(device_index, stream=self.main.cuda_stream)
        self.side_ctx = _lib.Context(device_index, stream=self.side.cuda_stream)

    def sync(self):
        self.main.synchronize()
        self.side.synchronize()


class TrainWave:
    """<= 16 parallel pairs -> their rows of the training matrix, in lockstep through the batched entries of
    include/kwy.h (what TrainPair does pair by pair on a stream each):

        w.analyse()   enqueue CheapTrick + D4C of all utterances and their trim lengths; the lengths start their way
                      to the host (ONE read-back per wave)
        w.finish(sink, pads)   (waits for the lengths) enqueue padding, voicing, sp2mc, DTW features, FastDTW
                      (`align`, which `EvalWave` shares), strict filter + cut, deltas and the append of the joint rows
                      behind the sink's device-side cursor
    `frame_period` is accepted and ignored: the frames come with the f0 tracks."""

    def __init__(self, ls, fs, pairs, order=24, radius=32, frame_period=5.0, bands=False):
        self.ls, self.fs, self.order, self.radius = ls, int(fs), int(order), int(radius)
        dev = ls.dev
        self.bands = 0
        if bands:                    # the band tracks of the padded items as well (`align`): B + 1 doubles per frame
            from .backend import bap
            self.bands = bap.check_rate(self.fs)
        self.fft = lib.kwy_cheaptrick_fft_size(self.fs, 71.0)
        self.K = K = self.fft // 2 + 1
        from .backend import sptk
        self.alpha = sptk.mcepalpha(self.fs)
        self.n = len(pairs)
        f64 = dict(dtype=torch.float64, device=dev)
        P = PAD_LEN
        with torch.cuda.stream(ls.main):
            # (x, f0, t) of every side: both streams may use them after the caller has dropped them
            sides = [[to_device(a, dev, (ls.main, ls.side)) for a in s] for pair in pairs for s in pair]
            self.x, self.f0, self.t = ([s[k] for s in sides] for k in range(3))
            self.T = [len(v) for v in self.f0]
            self.layout = layout = Ragged([t + 2 * P for t in self.T])
            self.reg = layout.view          # reg(block, i): the padded rows of side i in one of the blocks below
            self.rows = rows = layout.total
            self.sp_pad = torch.empty((rows, K), **f64)
            self.ap_pad = torch.full((rows, K), 1 - SAFE_GUARD_MINIMUM, **f64)
            self.f0_pad = torch.empty(rows, **f64)
            self.voiced = torch.empty(rows, **f64)
            self.mc_pad = torch.empty((rows, order + 1), **f64)
            self.feat = torch.empty((rows, order + 2), **f64)
            self.track = torch.empty((rows, self.bands + 1), **f64) if self.bands else None
            ns = len(sides)
            self.keep_dev = torch.zeros(ns, dtype=torch.int64, device=dev)
            self.keep_host = torch.zeros(ns, dtype=torch.int64).pin_memory()
            self.sp, self.ap = layout.views(self.sp_pad, P, P), layout.views(self.ap_pad, P, P)
            self.j_env = _lib.utterance_array([(self.x[i], self.t[i], self.f0[i], self.sp[i]) for i in range(ns)])
            self.j_ap = _lib.utterance_array([(self.x[i], self.t[i], self.f0[i], self.ap[i]) for i in range(ns)])
            self.j_trim = _lib.job_array(_lib.TrimJob, [(self.sp[i], self.T[i], self.keep_dev[i:i + 1]) for i in range(ns)])
        self.frames = sum(self.T[0::2])

    def analyse(self):
        ls, fs, fft, K, ns = self.ls, self.fs, self.fft, self.K, 2 * self.n
        ls.side.wait_stream(ls.main)                # (the buffers were made on the main stream)
        with torch.cuda.stream(ls.side):
            _lib.check(ls.side_ctx, lib.kwy_d4c_batch_dev(ls.side_ctx.handle, self.j_ap, ns, fs, 0.85, fft))
            self.ap_done = torch.cuda.Event()
            self.ap_done.record(ls.side)
        with torch.cuda.stream(ls.main):
            h = ls.ctx.handle
            _lib.check(ls.ctx, lib.kwy_cheaptrick_batch_dev(h, self.j_env, ns, fs, -0.15, 71.0, fft, float(fs)))
            _lib.check(ls.ctx, lib.kwy_trim_length_batch_dev(h, self.j_trim, ns, K, TRIM_EPS))
            self.keep_host.copy_(self.keep_dev, non_blocking=True)
            self.keep_ready = torch.cuda.Event()
            self.keep_ready.record(ls.main)

    def finish(self, sink, pads, cache=None, band_sink=None):
        """pads(rows): fills the wave's pad rows -- a list of 4 n device views (source head, source tail, target
        head, target tail, pair after pair) -- on the main stream.  cache: a TrainCache that takes over the wave's
        alignment inputs (and its share of the monitor of this first alignment), or None.  band_sink: the `_RowSink` of
        the band matrix (a wave made with bands=True), or None"""
        a = self.align(pads)
        a.rows_into(sink, band_sink)
        if cache is not None:
            cache.add(a)

    def align(self, pads):
        """(waits for the trim lengths) enqueue padding, voicing, sp2mc, the DTW features and FastDTW of every pair;
        sets `keep` and `alignment` and returns that `_Alignment`"""
        ls, fs, K, order, P, ns = self.ls, self.fs, self.K, self.order, PAD_LEN, 2 * self.n
        self.keep_ready.synchronize()
        self.keep = keep = [int(v) for v in self.keep_host.tolist()]
        Tp = [k + 2 * P for k in keep]
        reg = self.reg
        with torch.cuda.stream(ls.main):
            h = ls.ctx.handle
            chk = lambda rc: _lib.check(ls.ctx, rc)  # noqa: E731
            sp_r = [reg(self.sp_pad, i) for i in range(ns)]
            pads([blk for i in range(ns) for blk in (sp_r[i][:P], sp_r[i][P + keep[i]:Tp[i]])])
            ls.main.wait_event(self.ap_done)
            J = _lib.job_array
            chk(lib.kwy_train_pad_batch_dev(h, J(_lib.PadJob, [(self.f0[i], keep[i], reg(self.f0_pad, i), reg(self.ap_pad, i),
                                                               reg(self.voiced, i)) for i in range(ns)]), ns, K, fs, P))
            if self.bands:       # every padded item is one job: its pad rows (1 - 1e-12) come out unvoiced by themselves
                chk(lib.kwy_bap_track_batch_dev(h, J(_lib.BapTrackJob, [(reg(self.ap_pad, i), Tp[i], reg(self.track, i))
                                                                        for i in range(ns)]), ns, fs, self.fft))
            chk(lib.kwy_sp2mc_dev(h, _p(self.sp_pad), self.rows, K, order, self.alpha, _p(self.mc_pad)))
            # make_feature(vuv='voiced', power='binalize', power_pivot='max')
            chk(lib.kwy_align_features_batch_dev(h, J(_lib.AlignJob, [(reg(self.mc_pad, i), reg(self.voiced, i), Tp[i],
                                                                       reg(self.feat, i)) for i in range(ns)]),
                                                 ns, order + 1, POWER_WEIGHT, POWER_THRESHOLD, VUV_WEIGHT))
        inputs = _AlignInputs(self.n, self.layout, Tp, keep, self.mc_pad, self.feat, self.voiced, order, self.track)
        self.alignment = _Alignment(ls, inputs, self.radius)
        return self.alignment


class _AlignInputs(namedtuple('_AlignInputs', 'n layout Tp keep mc_pad feat voiced order track', defaults=(None,))):
    """What a wave of `n` pairs hands to an alignment, and all a TrainCache keeps of it: the padded mel-cepstra, the DTW
    features and the voicing -- blocks in the wave's ragged `layout`, item 2 k the source, 2 k + 1 the target of pair
    k --, the padded lengths `Tp` in use and the frames `keep` that TrimmedDataset kept; `track`: the band tracks of the
    padded items in the same layout ((B + 1) * 8 bytes per padded frame), or None for a wave made without bands"""
    __slots__ = ()


class _Alignment:
    """One FastDTW alignment of a wave's `_AlignInputs`, enqueued on the main stream (the only place the DtwJob array is
    built): pair k's source features are item 2 k of `feat`, its target's item 2 k + 1 -- the inputs' own features, or
    the rewritten copy of a re-alignment -- and the mel-cepstra are both items of the inputs' `mc_pad`."""

    def __init__(self, ls, inputs, radius, feat=None):
        self.ls, self.inputs = ls, inputs
        self.feat = feat = inputs.feat if feat is None else feat
        n, off, Tp, reg, dev = inputs.n, inputs.layout.off, inputs.Tp, inputs.layout.view, ls.dev
        with torch.cuda.stream(ls.main):
            # (a path's capacity: the cells of both padded items at their untrimmed lengths, + 2)
            self.path = [torch.zeros((off[2 * k + 2] - off[2 * k] + 2, 2), dtype=torch.int32, device=dev) for k in range(n)]
            self.path_len = torch.zeros(n, dtype=torch.int64, device=dev)
            self.dist = torch.zeros(n, dtype=torch.float64, device=dev)
            _lib.check(ls.ctx, lib.kwy_fastdtw_batch_dev(
                ls.ctx.handle,
                _lib.job_array(_lib.DtwJob, [(reg(feat, 2 * k), Tp[2 * k], reg(feat, 2 * k + 1), Tp[2 * k + 1],
                                             self.dist[k:k + 1], self.path[k], self.path_len[k:k + 1]) for k in range(n)]),
                n, inputs.order + 2, radius))

    def rows_into(self, sink, band_sink=None):
        """enqueue dtw_feature(strict=True) + align_even's cut, deltas, hstack + remove_zeros_frames and the append
        behind the cursor of the `_RowSink` for every pair; `n_rows`: the pairs' row counts, device words.
        band_sink: the `_RowSink` of the band matrix: the band rows of the same kept cells (`index_lists`) that are
        voiced on both sides go behind its cursor (kwy_bap_rows_batch_dev), `n_band_rows` their counts; the inputs must
        carry the band tracks (ValueError otherwise)"""
        ls, inp, feat = self.ls, self.inputs, self.feat
        Tp, reg = inp.Tp, inp.layout.view
        with torch.cuda.stream(ls.main):
            self.n_rows = torch.zeros(inp.n, dtype=torch.int64, device=ls.dev)
            _lib.check(ls.ctx, lib.kwy_train_rows_batch_dev(
                ls.ctx.handle,
                _lib.job_array(_lib.TrainJob, [(self.path[k], self.path_len[k:k + 1], reg(feat, 2 * k), reg(feat, 2 * k + 1),
                                                reg(inp.mc_pad, 2 * k), reg(inp.mc_pad, 2 * k + 1), Tp[2 * k], Tp[2 * k + 1],
                                                self.n_rows[k:k + 1]) for k in range(inp.n)]),
                inp.n, inp.order, 1, 1, 1, PAD_LEN, TRIM_EPS, _p(sink.X), sink.X.shape[0], _p(sink.cursor)))
            if band_sink is not None:
                from .backend import bap
                if inp.track is None:
                    raise ValueError('band rows: this alignment\'s inputs carry no band tracks (the wave, or the cache '
                                     'it came from, was made without bands=True)')
                idx_x, idx_y, cap, n_sel = self.index_lists()
                self.n_band_rows = torch.zeros(inp.n, dtype=torch.int64, device=ls.dev)
                bap.rows_batch_dev(ls.ctx, [bap.rows_job(reg(inp.track, 2 * k)[:Tp[2 * k]], reg(inp.track, 2 * k + 1)[:Tp[2 * k + 1]],
                                                         idx_x[k], idx_y[k], self.n_band_rows[k:k + 1], n_dev=n_sel[k:k + 1],
                                                         capacity=cap[k]) for k in range(inp.n)],
                                   band_sink.X.shape[1] // 6, band_sink.X, band_sink.cursor)
                band_sink.take(self.n_band_rows)

    def index_lists(self, n_sel=None):
        """enqueue dtw_feature(strict=True) + align_even's cut of every pair: -> (idx_x, idx_y, cap, n_sel), per pair the
        kept path's index lists into the two padded items, their capacity and their length (device words: `n_sel`)"""
        ls, inp, feat = self.ls, self.inputs, self.feat
        n, Tp, reg, dev = inp.n, inp.Tp, inp.layout.view, ls.dev
        with torch.cuda.stream(ls.main):
            cap = [p.shape[0] for p in self.path]
            idx_x = [torch.zeros(c, dtype=torch.int32, device=dev) for c in cap]
            idx_y = [torch.zeros(c, dtype=torch.int32, device=dev) for c in cap]
            if n_sel is None:
                n_sel = torch.zeros(n, dtype=torch.int64, device=dev)
            for k in range(n):
                _lib.check(ls.ctx, lib.kwy_align_even_dev(
                    ls.ctx.handle, _p(self.path[k]), _p(self.path_len[k:k + 1]), _p(reg(feat, 2 * k)), _p(reg(feat, 2 * k + 1)),
                    inp.order + 2, 1, 1, 1, Tp[2 * k], Tp[2 * k + 1], PAD_LEN, _p(idx_x[k]), _p(idx_y[k]), cap[k],
                    _p(n_sel[k:k + 1])))
        return idx_x, idx_y, cap, n_sel

    def monitor(self, acc):
        """enqueue the monitor of this alignment: along the kept path of every pair (`index_lists`: the cells that
        `rows_into` turns into rows) the distortion in dB over c1..cN between columns 2.. of the source's DTW features
        -- the coefficients the path was found with -- and the target's mel-cepstrum (kwy_mcd_batch_dev, one workgroup
        per pair); the cells' sum and count are added to the two device words `acc` (kwy_moments_accumulate_dev)"""
        from .backend import distortion as dist
        ls, inp = self.ls, self.inputs
        n, Tp, reg = inp.n, inp.Tp, inp.layout.view
        with torch.cuda.stream(ls.main):
            idx_x, idx_y, cap, n_sel = self.index_lists()
            moments = torch.zeros((n, 3), dtype=torch.float64, device=ls.dev)
            # (column 1 of the features, the voicing term, stands where c0 stands in a mel-cepstrum: first_col = 1)
            jobs = [dist.mcd_job(reg(self.feat, 2 * k)[:Tp[2 * k], 1:], reg(inp.mc_pad, 2 * k + 1)[:Tp[2 * k + 1]],
                                 idx_a=idx_x[k], idx_b=idx_y[k], rows=cap[k], n_dev=n_sel[k:k + 1]) for k in range(n)]
            dist.mcd_batch_dev(ls.ctx, jobs, inp.order + 1, moments)
            _lib.check(ls.ctx, lib.kwy_moments_accumulate_dev(ls.ctx.handle, _p(moments), n, _p(acc)))


class _RowSink:
    """A training matrix being filled on the main stream: the capacity block `X`, the device-side `cursor` that
    kwy_train_rows_batch_dev appends behind, and `worst`, the minimum over all pairs' row counts (k_tr_rows_place marks
    a pair that did not fit behind the cursor with -1 - rows and drops it)."""

    def __init__(self, ls, cap_rows, order):
        self.ls, self.cap_rows = ls, cap_rows
        with torch.cuda.stream(ls.main):
            self.X = torch.empty((cap_rows, 6 * order), dtype=torch.float64, device=ls.dev)
            self.cursor = torch.zeros(1, dtype=torch.int64, device=ls.dev)
            self.worst = torch.zeros(1, dtype=torch.int64, device=ls.dev)

    def take(self, n_rows):
        """enqueue the fold of a wave's row counts into `worst`"""
        with torch.cuda.stream(self.ls.main):
            torch.minimum(self.worst, n_rows.min().reshape(1), out=self.worst)

    def close(self, extra=()):
        """the ONE read-back of a matrix: -> (the rows written, the `extra` int64 device words as host ints)"""
        cap_rows = self.cap_rows
        with torch.cuda.stream(self.ls.main):
            words = torch.cat((self.cursor, self.worst, *extra)).tolist()
        self.ls.sync()
        n_rows, dropped = int(words[0]), int(words[1])
        if dropped < 0:
            # (the capacity, a row per frame of both sides, bounds every pair's rows: a bug, never a data property)
            raise RuntimeError(f'training matrix: a pair of {-1 - dropped} rows did not fit the capacity of {cap_rows}')
        torch.cuda.current_stream(self.ls.dev).synchronize()
        # (a view would keep the whole capacity block alive: twice the rows actually used, or more)
        return (self.X[:n_rows].clone() if n_rows * 4 < cap_rows * 3 else self.X[:n_rows]), words[2:]


class TrainCache:
    """What a second alignment of the training set needs of the first, kept in HBM: per wave of pairs the padded
    mel-cepstra `mc_pad`, the DTW features `feat` of the first alignment, the voicing `voiced`, the padded lengths and
    the kept frames -- the waves' `_AlignInputs`: ragged blocks in `_blocks.Ragged` layout, the waves' own buffers taken
    over as they are.  The padded envelopes and aperiodicities (sp_pad, ap_pad: 2 x 1025 doubles per frame at 48 kHz)
    are NOT kept; without the cache a second pass would have to analyse every pair again.
    Size: (order + 1) + (order + 2) + 1 doubles per padded frame of both sides -- 416 bytes (0.41 KiB) at order 24;
    bench_corpus.py's 503 pairs of 5 s (1001 + 200 padded frames a side) take 2 x 1201 x 416 B = 1.0 MB a pair,
    0.50 GB in all.
    `monitor`: two device words, sum and count of the first alignment's monitor (see `_Alignment.monitor`);
    `path_len`: per wave the cells of the first alignment's FastDTW paths (n device words)."""

    def __init__(self, ls, fs, order, radius):
        self.ls, self.fs, self.order, self.radius = ls, int(fs), int(order), int(radius)
        self.waves, self.path_len = [], []
        self.monitor = torch.zeros(2, dtype=torch.float64, device=ls.dev)

    pairs = property(lambda self: sum(w.n for w in self.waves))
    frames = property(lambda self: sum(sum(w.Tp) for w in self.waves))
    nbytes = property(lambda self: sum(t.numel() * 8 for w in self.waves for t in (w.mc_pad, w.feat, w.voiced, w.track)
                                       if t is not None))

    def add(self, alignment):
        self.waves.append(alignment.inputs)
        self.path_len.append(alignment.path_len)
        # (its scratch is made and dropped on the main stream: reused there only behind the queued work)
        alignment.monitor(self.monitor)


def realign_training_matrix(cache, gmm, paths=None, bands=False):
    """One re-alignment pass over a cached training set with the fitted mixture `gmm`: -> (X, mcd_mean).
    The mixture is prepared once (kwy_gmm_prepare_dev); then, wave by wave (<= 16 pairs), the sources' padded
    mel-cepstra are converted -- deltas, mixture, MLPG: `MelCepstrumFeatureConverter.convert(..., diff=False)` -- straight
    into columns 2.. of a COPY of their DTW features (kwy_realign_features_batch_dev; the cache's first-alignment
    features stay as they are, power and voicing terms are the source's own), FastDTW runs on them against the targets'
    unchanged features, and the joint rows of the ORIGINAL mel-cepstra along the new paths go behind a device-side
    cursor (kwy_train_rows_batch_dev).  mcd_mean: the monitor of this alignment (`_Alignment.monitor`).  One read-back.
    paths: a list that receives, pair after pair, the (FastDTW path, its length) device tensors of this pass.
    bands=True: -> (X, mcd_mean, band matrix): the band rows along this pass's alignment as well; the cache must hold the
    band tracks (`build_training_matrix(keep=True, bands=True)`), ValueError otherwise, before anything is enqueued."""
    import struct
    if bands and any(w.track is None for w in cache.waves):
        raise ValueError('realign_training_matrix(bands=True): the cache holds no band tracks, so the band rows cannot '
                         'follow this alignment (build it with build_training_matrix(keep=True, bands=True))')
    ls, order, dev = cache.ls, cache.order, cache.ls.dev
    dg = DeviceGMM(gmm.weights_, gmm.means_, gmm.covariances_, dev)
    if dg.D2 != 6 * order:
        raise ValueError(f'realign_training_matrix: the mixture has {dg.D2} joint dimensions, the cache order {order}')
    sink = _RowSink(ls, cache.frames, order)      # a pair yields at most one row per cell of its path
    band_sink = _RowSink(ls, cache.frames, cache.waves[0].track.shape[1] - 1) if bands and cache.waves else None
    with torch.cuda.stream(ls.main):
        model = dg.model(diff=False)
        acc = torch.zeros(2, dtype=torch.float64, device=dev)
        for w in cache.waves:
            reg = w.layout.view
            feat = w.feat.clone()                  # the sources' items are rewritten below, the targets' only read
            _lib.check(ls.ctx, lib.kwy_realign_features_batch_dev(
                ls.ctx.handle, _lib.job_array(_lib.RealignJob, [(reg(w.mc_pad, 2 * k), w.Tp[2 * k], reg(feat, 2 * k))
                                                                for k in range(w.n)]), w.n, order, dg.M, _p(model)))
            a = _Alignment(ls, w, cache.radius, feat=feat)
            a.rows_into(sink, band_sink)
            a.monitor(acc)
            sink.take(a.n_rows)
            # (the wave's scratch -- feat, path, ... -- was made on the main stream: freed here, reused there in order)
            if paths is not None:
                paths.extend((a.path[k], a.path_len[k:k + 1]) for k in range(w.n))
    X, words = sink.close(extra=(acc.view(torch.int64),))
    total, cells = struct.unpack('<2d', struct.pack('<2q', *words))
    mcd = total / cells if cells > 0 else float('nan')
    return (X, mcd, band_sink.close()[0]) if band_sink is not None else (X, mcd)


def train_converter_realigned(pairs, fs, components=64, seed=None, align_iterations=0, max_iter=100, device_index=0,
                              order=24, radius=32, frame_period=5.0, silence_for=None, rng=None, pairs_before=0,
                              driver=None, lockstep=None, wave_pairs=16, f0_moments=False, gv_moments=False, verbose=0,
                              keep_matrices=False, covariance='full', ap_components=None):
    """Training with iterative re-alignment on the device: `build_training_matrix(keep=True)` and `fit_converter`, then
    `align_iterations` times `realign_training_matrix` with the mixture fitted last and `fit_converter` on its rows,
    from scratch (same components, seed, stopping rule, `covariance` structure).  The pads are drawn once -- numpy's global generator or the
    device-drawn stream (`rng`, `pairs_before`) advance as they do for align_iterations = 0 -- and the f0 / global
    variance moments are the first pass's.  Returns (mixture, history[, f0 moments][, gv statistic]): history holds a
    dict per fit -- rows, mcd (the alignment's monitor, `_Alignment.monitor`), em_iterations -- and with keep_matrices=True
    its matrix X.  Lockstep driver only.
    ap_components=N: also the band-aperiodicity mixture of N components (same seed, stopping rule, structure), fitted as
    it is on the band rows of the LAST alignment (`build_training_matrix(bands=True)` / `realign_training_matrix(bands=
    True)`); it is the last result.  Those rows exist only once the last pass has run: a pass whose cache holds no band
    tracks raises the ValueError of `realign_training_matrix`, which says so."""
    n_more = int(align_iterations)
    if n_more < 0:
        raise ValueError(f'align_iterations {align_iterations!r} is negative')
    if n_more > 0 and driver not in (None, 'lockstep'):
        raise ValueError(f"align_iterations > 0 needs the lockstep driver, not driver={driver!r}")
    out = build_training_matrix(pairs, fs, device_index=device_index, order=order, radius=radius, frame_period=frame_period,
                                silence_for=silence_for, rng=rng, pairs_before=pairs_before, driver=driver,
                                lockstep=lockstep, wave_pairs=wave_pairs, f0_moments=f0_moments, gv_moments=gv_moments,
                                keep=n_more > 0, bands=ap_components is not None)
    X, rest = out[0], list(out[2:])
    cache = rest.pop(0) if n_more > 0 else None
    Xb = rest.pop(0) if ap_components is not None else None
    history = []

    def fit(X, mcd):
        g = fit_converter(X, components=components, seed=seed, max_iter=max_iter, device_index=device_index,
                          verbose=verbose, covariance=covariance)
        history.append(dict(rows=int(X.shape[0]), mcd=mcd, em_iterations=int(g.n_iter_),
                            **(dict(X=X) if keep_matrices else {})))
        return g
    first = None
    if cache is not None:
        total, cells = cache.monitor.tolist()
        first = total / cells if cells > 0 else float('nan')
    g = fit(X, first)
    for _ in range(n_more):
        X, mcd, *band = realign_training_matrix(cache, g, bands=ap_components is not None)
        Xb = band[0] if band else Xb
        g = fit(X, mcd)
    if ap_components is not None:
        rest.append(fit_converter(Xb, components=ap_components, seed=seed, max_iter=max_iter, device_index=device_index,
                                  verbose=verbose, covariance=covariance))
    return (g, history, *rest)


class _NonparallelSide:
    """One side of a non-parallel training set in HBM: the utterances analysed in waves of <= 16 through the batched
    entries (CheapTrick, D4C, sp2mc, voicing, the DTW feature rows whose power and voicing terms pick and mark the speech
    frames: what `Analyzer` and `make_feature` do file by file), then per utterance the mel-cepstrum `mc` (T x
    (order + 1)), the int32 list `speech` of its speech frames and the f0 track, and over all its speech frames in
    utterance order `delta` (rows x 3 order: delta features of c1..cN over ALL frames, rows selected afterwards) and
    `voicing` (rows).  The envelopes and aperiodicities of a wave go when the wave is done."""

    def __init__(self, ls, utterances, fs, order, wave=16):
        self.ls, self.order = ls, int(order)
        dev, fs = ls.dev, int(fs)
        f64 = dict(dtype=torch.float64, device=dev)
        fft = lib.kwy_cheaptrick_fft_size(fs, 71.0)
        K = fft // 2 + 1
        from .backend import sptk
        alpha = sptk.mcepalpha(fs)
        h, J = ls.ctx.handle, _lib.job_array
        chk = lambda rc: _lib.check(ls.ctx, rc)  # noqa: E731
        self.mc, self.speech, self.f0, deltas, voicing = [], [], [], [], []
        with torch.cuda.stream(ls.main):
            for w0 in range(0, len(utterances), wave):
                items = [[to_device(a, dev, (ls.main,)) for a in u] for u in utterances[w0:w0 + wave]]
                x, f0, t = ([s[k] for s in items] for k in range(3))
                n, layout = len(items), Ragged([len(v) for v in f0])
                sp, ap = torch.empty((layout.total, K), **f64), torch.empty((layout.total, K), **f64)
                mc = torch.empty((layout.total, order + 1), **f64)
                feat = torch.empty((layout.total, order + 2), **f64)
                voiced = torch.empty(layout.total, **f64)
                sp_v, ap_v = layout.views(sp), layout.views(ap)
                chk(lib.kwy_cheaptrick_batch_dev(h, _lib.utterance_array([(x[i], t[i], f0[i], sp_v[i]) for i in range(n)]),
                                                 n, fs, -0.15, 71.0, fft, float(fs)))
                chk(lib.kwy_d4c_batch_dev(h, _lib.utterance_array([(x[i], t[i], f0[i], ap_v[i]) for i in range(n)]), n, fs,
                                          0.85, fft))
                chk(lib.kwy_sp2mc_dev(h, _p(sp), layout.total, K, order, alpha, _p(mc)))
                for i in range(n):
                    chk(lib.kwy_is_voiced_dev(h, _p(f0[i]), _p(ap_v[i]), len(f0[i]), K, fs, _p(layout.view(voiced, i))))
                # make_feature(vuv='voiced', power='binalize', power_pivot='max')
                chk(lib.kwy_align_features_batch_dev(h, J(_lib.AlignJob, [(layout.view(mc, i), layout.view(voiced, i),
                                                                           len(f0[i]), layout.view(feat, i))
                                                                          for i in range(n)]),
                                                     n, order + 1, POWER_WEIGHT, POWER_THRESHOLD, VUV_WEIGHT))
                for i in range(n):
                    rows = layout.view(feat, i)
                    speech = torch.nonzero(rows[:, 0] > 0).flatten().to(torch.int32)
                    self.mc.append(layout.view(mc, i))
                    self.speech.append(speech)
                    self.f0.append(f0[i])
                    voicing.append(rows[:, 1][speech.long()])
                    deltas.append(self.delta_rows(layout.view(mc, i), speech))
            self.delta = torch.cat(deltas) if deltas else torch.empty((0, 3 * order), **f64)
            self.voicing = torch.cat(voicing) if voicing else torch.empty(0, **f64)
        self.rows = int(self.delta.shape[0])

    def delta_rows(self, mc, speech):
        """delta_features(c1..cN of `mc`, DELTA_WINDOWS)[speech] on the device (enqueued on the main stream)"""
        ls, order, T = self.ls, self.order, int(mc.shape[0])
        out = torch.empty((len(speech), 3 * order), dtype=torch.float64, device=ls.dev)
        if T == 0 or len(speech) == 0:
            return out
        static = mc[:, 1:].contiguous()
        count = torch.full((1,), T, dtype=torch.int64, device=ls.dev)
        full = torch.empty((T, 3 * order), dtype=torch.float64, device=ls.dev)
        _lib.check(ls.ctx, lib.kwy_delta_features_dev(ls.ctx.handle, _p(static), _p(count), T, order, _p(full)))
        _lib.check(ls.ctx, lib.kwy_gather_rows_dev(ls.ctx.handle, _p(full), T, 3 * order, _p(speech), len(speech), _p(out)))
        return out


def train_converter_nonparallel(source, target, fs, components=64, seed=None, iterations=None, max_iter=100,
                                device_index=0, order=24, lockstep=None, f0_moments=False, gv_moments=False, verbose=0,
                                keep_matrices=False, covariance='full', splits=0):
    """Non-parallel training (INCA) on the device: `MelCepstrumFeatureConverter.train_nonparallel` with the features in
    HBM across the iterations.  source, target: lists of (x, f0, t) utterances that need not correspond.  Both sides are
    analysed once (`_NonparallelSide`); mel-cepstra, delta features, search rows [voicing term | c1..cN | delta c1..cN]
    and speech-frame index lists stay on the device.  Fit i = 0 .. iterations: kwy_convert_mcep_batch_dev on the source
    utterances with the mixture fitted last (fit 0: their own mel-cepstra), kwy_delta_features_dev, two
    kwy_nn_search_dev, kwy_gather_rows_dev into the joint matrix [x_k | y_p(k)] ; [x_q(j) | y_j], `fit_converter` from
    scratch, and ONE read-back: the monitor (mean distortion over c1..cN across the joint rows between the static columns
    the search used) with the searches' status words.
    Returns (mixture, history[, f0 moments][, gv statistic]): history holds a dict per fit -- rows, mcd, em_iterations,
    seconds (wall clock of the whole iteration, the fit included) and with keep_matrices=True its matrix X; the moments are the merged voiced log-f0 triples of (source, target), the
    statistic the target's global variance."""
    from .backend import distortion as dist, nn
    from .converter.mcep import MelCepstrumFeatureConverter as _M
    if iterations is None:
        iterations = _M.NONPARALLEL_DEFAULT
    lo, hi = _M.NONPARALLEL_RANGE
    if isinstance(iterations, bool) or int(iterations) != iterations or not lo <= iterations <= hi:
        raise ValueError(f'iterations must be an integer within [{lo}, {hi}], not {iterations!r}')
    if not len(source) or not len(target):
        raise ValueError(f'nonparallel: no {"source" if not len(source) else "target"} files')
    ls = lockstep if lockstep is not None else _Lockstep(device_index)
    dev, ctx, h = ls.dev, ls.ctx, ls.ctx.handle
    f64 = dict(dtype=torch.float64, device=dev)
    src, tgt = (_NonparallelSide(ls, side, fs, order) for side in (source, target))
    ns, nt = src.rows, tgt.rows
    if not ns or not nt:
        raise ValueError(f'nonparallel: no speech frames ({ns} on the source side, {nt} on the target side)')
    history, g = [], None
    with torch.cuda.stream(ls.main):
        T = torch.cat((tgt.voicing[:, None], tgt.delta[:, :2 * order]), dim=1).contiguous()
        p, q = (torch.empty(n, dtype=torch.int32, device=dev) for n in (ns, nt))
        d2 = torch.empty(max(ns, nt), **f64)
        own = torch.arange(max(ns, nt), dtype=torch.int32, device=dev)
        words = torch.zeros(5, **f64)            # the monitor's (n, mean, M2), then the two searches' status words
        status = torch.zeros(3, dtype=torch.int32, device=dev)
        _lib.check(ctx, lib.kwy_ctx_reserve(h, nn.scratch_bytes(max(ns, nt), splits)))
    import time
    for it in range(int(iterations) + 1):
        started = time.perf_counter()
        with torch.cuda.stream(ls.main):
            if g is None:
                mapped = src.delta[:, :2 * order]
            else:
                dg = DeviceGMM(g.weights_, g.means_, g.covariances_, dev)
                outs = [torch.empty_like(mc) for mc in src.mc]
                _lib.check(ctx, lib.kwy_convert_mcep_batch_dev(
                    h, _lib.job_array(_lib.ConvertJob, [(mc, mc.shape[0], out) for mc, out in zip(src.mc, outs)]),
                    len(outs), order, dg.M, _p(dg.model(diff=False))))
                mapped = torch.cat([src.delta_rows(out, sp) for out, sp in zip(outs, src.speech)])[:, :2 * order]
            S = torch.cat((src.voicing[:, None], mapped), dim=1).contiguous()
            nn.nearest_dev(ctx, S, T, p, d2, status[0:1], splits=splits)
            nn.nearest_dev(ctx, T, S, q, d2, status[1:2], splits=splits)
            X = torch.empty((ns + nt, 6 * order), **f64)
            half = torch.empty((max(ns, nt), 3 * order), **f64)
            X[:ns, :3 * order] = src.delta
            X[ns:, 3 * order:] = tgt.delta
            _lib.check(ctx, lib.kwy_gather_rows_dev(h, _p(tgt.delta), nt, 3 * order, _p(p), ns, _p(half)))
            X[:ns, 3 * order:] = half[:ns]
            _lib.check(ctx, lib.kwy_gather_rows_dev(h, _p(src.delta), ns, 3 * order, _p(q), nt, _p(half)))
            X[ns:, :3 * order] = half[:nt]
            idx_a, idx_b = torch.cat((own[:ns], q)), torch.cat((p, own[:nt]))
            dist.mcd_batch_dev(ctx, [dist.mcd_job(S[:, 1:order + 1], T[:, 1:order + 1], idx_a, idx_b)], order,
                               words[:3].view(1, 3), status[2:3], first_col=0)
            words[3:] = status[:2]
            n, mean, _, bad_p, bad_q = words.cpu().tolist()          # (the one read-back of the iteration; it synchronises)
        if bad_p or bad_q:
            nn.check_status([int(bad_p) + int(bad_q)], 'nonparallel')
        ls.sync()
        g = fit_converter(X, components=components, seed=seed, max_iter=max_iter, device_index=device_index,
                          verbose=verbose, covariance=covariance)
        history.append(dict(rows=int(X.shape[0]), mcd=float(mean) if n > 0 else float('nan'),
                            em_iterations=int(g.n_iter_), seconds=time.perf_counter() - started,
                            **(dict(X=X) if keep_matrices else {})))
    rest = []
    if f0_moments:
        from .backend import f0 as f0map
        with torch.cuda.stream(ls.main):
            merged = torch.empty((2, 3), **f64)
            for k, side in enumerate((src, tgt)):
                rows = torch.empty((len(side.f0), 3), **f64)
                f0map.logf0_moments_batch_dev(ctx, side.f0, rows)
                f0map.merge_moments_dev(ctx, rows, merged[k])
            rest.append(merged.cpu().numpy())
    if gv_moments:
        gv = _PairGV(len(tgt.mc), order, device_index)
        with torch.cuda.stream(ls.main):
            gv.add(ctx, 0, tgt.mc)
        ls.sync()
        rest.append(gv.statistic())
    return (g, history, *rest)


class EvalWave(TrainWave):
    """<= 16 parallel pairs -> their evaluation figures (kwiiyatta_amd.evaluate_voice), in lockstep: analysed, trimmed,
    padded and aligned exactly as TrainWave does it (`analyse`, `align`: the same pad rows in the same order), the
    source's trimmed mel-cepstra converted on their own time axis as ConvertWave converts (the batched GMM + MLPG
    entry, then the global-variance postfilter when asked for), and measured along the index lists that
    kwy_align_even_dev leaves on the device (kwy_mcd_batch_dev, kwy_f0_error_batch_dev: no gathered copies, the row
    counts stay device words).  Nothing is read back here: `measure` writes pair k's figures into row first + k of the
    caller's tensors.  `frame_period` is accepted and ignored, as in TrainWave."""

    def measure(self, pads, gmm, model, tot, first, opts, frames='speech', per_frame=False, ap_gmm=None):
        """tot: the _EvalTotals of the corpus; opts: the resolved options (`ConvertOptions.upload`) -- of them the f0
        map, the global-variance postfilter (`_GvFilter`), mlpg_em and the GV ascent, whose status words go where the
        postfilter's would (the two exclude each other).  ap_gmm (a DeviceGMM; the wave made with bands=True): also the
        band error of the source's band track, converted (clamped as the rendering clamps it) and unconverted, against
        the target's along the same index lists, into tot.bap (kwy_bap_error_batch_dev)"""
        mlpg_em, gvgen = opts.mlpg_em, opts.gvgen
        from .backend import distortion as dist
        a = self.align(pads)
        Tp = a.inputs.Tp
        ls, fs, order, P, n, reg, keep = self.ls, self.fs, self.order, PAD_LEN, self.n, self.reg, self.keep
        dev, cols = ls.dev, self.order + 1
        f64 = dict(dtype=torch.float64, device=dev)
        with torch.cuda.stream(ls.main):
            h = ls.ctx.handle
            chk = lambda rc: _lib.check(ls.ctx, rc)  # noqa: E731
            J = _lib.job_array
            # dtw_feature(strict=True) + align_even's cut: the index lists and their count stay on the device
            self.idx_x, self.idx_y, cap, n_sel = a.index_lists(tot.aligned[first:first + n])
            # the trimmed utterances inside their padded blocks
            src_mc = [reg(self.mc_pad, 2 * k)[P:P + keep[2 * k]] for k in range(n)]
            tgt_mc = [reg(self.mc_pad, 2 * k + 1)[P:P + keep[2 * k + 1]] for k in range(n)]
            src_f0 = [self.f0[2 * k][:keep[2 * k]] for k in range(n)]
            tgt_f0 = [self.f0[2 * k + 1][:keep[2 * k + 1]] for k in range(n)]
            own = Ragged(keep[0::2])                    # the sources' own time axes, end to end
            self.mc_conv = torch.empty((own.total, cols), **f64)
            conv = own.views(self.mc_conv)
            chk(_convert_mcep_batch(h, _convert_jobs([(src_mc[k], keep[2 * k], conv[k]) for k in range(n)], mlpg_em, gvgen),
                                    n, order, gmm.M, model, mlpg_em, gvgen, 0,
                                    tot.gv_status[first:first + n] if gvgen is not None else None))
            if opts.gv is not None:
                self.gv_filter = _GvFilter(opts.gv, opts.gv_strength, conv, keep[0::2], None, dev,
                                           status=tot.gv_status[first:first + n])
                self.gv_filter.prepare(chk, h)
                self.gv_filter.launch(chk, h)
            if opts.f0_map:
                from .backend.f0 import key_ratio
                self.f0_mapped = torch.empty(own.total, **f64)
                mapped = own.views(self.f0_mapped)
                chk(lib.kwy_f0_map_batch_dev(h, J(_lib.F0MapJob, [(src_f0[k], keep[2 * k], mapped[k]) for k in range(n)]),
                                             n, fs, None if opts.f0_stats is None else opts.f0_stats.data_ptr(),
                                             key_ratio(opts.transpose_key), _p(tot.f0_map_status[first:first + n])))
                src_f0 = mapped
            self.mcd_frames = [torch.empty(c, **f64) for c in cap] if per_frame else [None] * n
            jobs = []
            for k in range(n):
                along = dict(idx_a=self.idx_x[k], idx_b=self.idx_y[k], off_a=P, off_b=P, rows=cap[k], n_dev=n_sel[k:k + 1],
                             mask=reg(self.feat, 2 * k + 1)[:Tp[2 * k + 1], 0] if frames == 'speech' else None)
                jobs.append(dist.mcd_job(conv[k], tgt_mc[k], per_row=self.mcd_frames[k], **along))
                jobs.append(dist.mcd_job(src_mc[k], tgt_mc[k], **along))
            dist.mcd_batch_dev(ls.ctx, jobs, cols, tot.mcd[first:first + n].view(-1, 3),
                               tot.mcd_status[first:first + n].view(-1))
            dist.f0_error_batch_dev(ls.ctx, [dist.f0_error_job(src_f0[k], tgt_f0[k], self.idx_x[k], self.idx_y[k], P, P,
                                                               rows=cap[k], n_dev=n_sel[k:k + 1]) for k in range(n)],
                                    tot.counts[first:first + n], tot.f0[first:first + n], tot.f0_status[first:first + n])
            if ap_gmm is not None:
                from .backend import bap
                B = self.bands
                src_tr = [reg(self.track, 2 * k)[P:P + keep[2 * k]] for k in range(n)]
                tgt_tr = [reg(self.track, 2 * k + 1)[P:P + keep[2 * k + 1]] for k in range(n)]
                self.track_conv = torch.empty((own.total, B + 1), **f64)
                mapped = own.views(self.track_conv)
                chk(lib.kwy_convert_mcep_batch_dev(h, J(_lib.ConvertJob, [(src_tr[k], keep[2 * k], mapped[k]) for k in range(n)]),
                                                   n, B, ap_gmm.M, _p(ap_gmm.model(diff=False))))
                self.track_conv[:, 1:].clamp_(bap.FLOOR, bap.CEILING)
                jobs = []
                for k in range(n):
                    along = dict(idx_a=self.idx_x[k], idx_b=self.idx_y[k], off_a=P, off_b=P, rows=cap[k], n_dev=n_sel[k:k + 1])
                    jobs.append(bap.error_job(mapped[k], tgt_tr[k], **along))
                    jobs.append(bap.error_job(src_tr[k], tgt_tr[k], **along))
                bap.error_batch_dev(ls.ctx, jobs, B, tot.bap[first:first + n].view(-1, 3))


class _EvalTotals:
    """the figures of a corpus's pairs in HBM, a row per pair: the (n, mean, M2) triples of the distortion (converted,
    unconverted source) and of the f0 error, the voicing counts, the aligned frames and the status words"""

    def __init__(self, n_pairs, dev, bands=False):
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.mcd = torch.zeros((n_pairs, 2, 3), **f64)
        self.bap = torch.zeros((n_pairs, 2, 3), **f64) if bands else None     # band error: converted, unconverted source
        self.f0 = torch.zeros((n_pairs, 3), **f64)
        self.counts = torch.zeros((n_pairs, 4), dtype=torch.int64, device=dev)
        self.aligned = torch.zeros(n_pairs, dtype=torch.int64, device=dev)
        self.mcd_status, self.f0_status = torch.zeros((n_pairs, 2), **i32), torch.zeros(n_pairs, **i32)
        self.gv_status, self.f0_map_status = torch.zeros(n_pairs, **i32), torch.zeros(n_pairs, **i32)

    def read(self, ctx):
        """(enqueued behind the waves on ctx's stream) the pooled triples from the merge kernel, then everything to the
        host: (triples (n_pairs + 1, 3, 3) with the totals last -- (n_pairs + 1, 5, 3) with the band error's two behind
        them --, counts, aligned, status words (n_pairs, 5))"""
        from .backend import distortion as dist
        triples = torch.cat((self.mcd, self.f0[:, None]) + (() if self.bap is None else (self.bap,)), dim=1).contiguous()
        both = torch.cat((triples, torch.zeros_like(triples[:1])))
        dist.merge_moments_dev(ctx, triples, both[-1])
        status = torch.cat((self.mcd_status, self.f0_status[:, None], self.gv_status[:, None],
                            self.f0_map_status[:, None]), dim=1)
        whole = torch.cat((self.counts, self.aligned[:, None]), dim=1)
        return both.cpu().numpy(), whole[:, :4].cpu().numpy(), whole[:, 4].cpu().numpy(), status.cpu().numpy()


class ConvertPipeline(_Graphed):
    """convert_voice.convert(diffvc=False) of one utterance, HBM-resident: analyse -> mel-cepstrum -> GMM/MLPG
    conversion (c0 kept) -> spectrum -> synthesis with the utterance's own f0 and aperiodicity.

    mcep_fs: the sampling rate the converter was trained at, when it differs from the utterance's
    (`--mcep-fs`; MelCepstrumFeatureConverter.convert and the `feature.mel_cepstrum = ...` that follows it,
    /root/reference/kwiiyatta/converter/mcep.py:47-61, vocoder/mcep.py:31-45, vocoder/abc/feature.py): the
    mel-cepstrum travels to the converter's rate and back through its spectrum -- mc2sp on the vocoder's grid of
    the old rate, the bins cut at the new Nyquist frequency or extended by "silent" bins |N(0, EPS / old_fs)|, sp2mc
    with the new rate's alpha (any bin count: the dense form).  The silent bins are one numpy draw of (T, missing)
    values per call; `rng` (a backend.nprandom.DeviceRandomState) draws them on the device in the reference's
    order, so a seeded run equals the Python API path."""

    def __init__(self, device_index, fs, utterance, gmm, order=24, frame_period=5.0, stream=None, ctx=None,
                 mcep_fs=None, rng=None):
        self.dev = torch.device('cuda', device_index)
        self.fs, self.order, self.frame_period = int(fs), int(order), float(frame_period)
        self.stream = stream if stream is not None else torch.cuda.Stream(device=self.dev)
        self.ctx = ctx if ctx is not None else _lib.Context(device_index, stream=self.stream.cuda_stream)
        self.fft = lib.kwy_cheaptrick_fft_size(self.fs, 71.0)
        self.K = self.fft // 2 + 1
        from .backend import sptk
        self.alpha = sptk.mcepalpha(self.fs)
        self.gmm = gmm
        assert gmm.D2 == 6 * order
        with torch.cuda.stream(self.stream):
            self.gmm_model = gmm.model(diff=False)
        x, f0, t = utterance
        self.N, self.T = len(x), len(f0)
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.mcep_fs = int(mcep_fs) if mcep_fs is not None and int(mcep_fs) != self.fs else None
        self.rng = rng
        with torch.cuda.stream(self.stream):
            # (a caller's tensor is cloned on this stream, and recorded: the caller may drop it while the clone is queued)
            self.x, self.f0, self.t = (to_device(a, self.dev, (self.stream,)).clone() if torch.is_tensor(a) else
                                       to_device(a, self.dev) for a in (x, f0, t))
            self.sp = torch.empty((self.T, self.K), **f64)
            self.ap = torch.empty((self.T, self.K), **f64)
            self.mc = torch.empty((self.T, order + 1), **f64)
            self.mc_x = torch.empty((self.T, order), **f64)
            self.mc_y = torch.empty((self.T, order), **f64)
            self.mc_conv = torch.empty((self.T, order + 1), **f64)
            self.sp_conv = torch.empty((self.T, self.K), **f64)
            self.ylen = lib.kwy_synth_length(self.T, self.frame_period, self.fs)
            self.wave = torch.empty(self.ylen, **f64)
            if self.mcep_fs is not None:
                if rng is None:
                    raise ValueError('ConvertPipeline(mcep_fs=...) needs rng: the silent bins of the wider spectrum '
                                     'are random draws')
                fc = self.mcep_fs
                self.alpha_c = sptk.mcepalpha(fc)
                self.Kc = lib.kwy_cheaptrick_fft_size(fc, 71.0) // 2 + 1         # the vocoder's grid at the other rate
                self.n_there = self.K * fc // self.fs                            # our grid carried to the converter's rate
                self.n_back = self.Kc * self.fs // fc                            # its grid carried back to ours
                self.spec_u = torch.empty((self.T, self.K), **f64)
                self.there = torch.empty((self.T, self.n_there), **f64)
                self.mc_c = torch.empty((self.T, order + 1), **f64)
                self.mc_c2 = torch.empty((self.T, order + 1), **f64)
                self.spec_c = torch.empty((self.T, self.Kc), **f64)
                self.back = torch.empty((self.T, self.n_back), **f64)
                # the one "up" direction of the round trip appends random silent bins (drawn per run)
                miss = self.n_there - self.K if fc > self.fs else self.n_back - self.Kc
                self.silent = torch.empty((self.T, miss), **f64)
        self.stream.synchronize()
        self.frames = self.T

    def load(self, utterance):
        """another utterance of the same shape into the existing buffers (numpy arrays or device tensors;
        asynchronous on the pipeline's stream)"""
        x, f0, t = utterance
        if len(x) != self.N or len(f0) != self.T:
            raise ValueError('ConvertPipeline.load: shape differs from the pipeline\'s')
        with torch.cuda.stream(self.stream):
            for dst, src in ((self.x, x), (self.f0, f0), (self.t, t)):
                # (a caller's tensor is recorded: it may be dropped while the copy is still queued)
                dst.copy_(to_device(src, None, (self.stream,)), non_blocking=True)

    def _convert_across_rates(self, chk, h):
        """self.mc (utterance rate) -> self.mc_conv (utterance rate) through the converter's rate"""
        T, order, fs, fc = self.T, self.order, self.fs, self.mcep_fs
        EPS = 2.220446049250313e-16
        up_first = fc > fs
        # (one block: the order below IS the order of the reference's calls)
        # MelCepstrum.resample_data(fc): spectrum on our grid, cut / extended, coefficients with the new alpha
        chk(lib.kwy_mc2sp_dev(h, _p(self.mc), T, order, self.alpha, self.fft, _p(self.spec_u)))
        if up_first:
            self.rng.stream.wait_stream(self.stream)
            self.rng.abs_normal(EPS / fs, out=self.silent)
            self.stream.wait_event(self.rng.record_event())
            self.there[:, :self.K].copy_(self.spec_u)
            self.there[:, self.K:].copy_(self.silent)
        else:
            self.there.copy_(self.spec_u[:, :self.n_there])
        chk(lib.kwy_sp2mc_dev(h, _p(self.there), T, self.n_there, order, self.alpha_c, _p(self.mc_c)))
        # the conversion itself, at the converter's rate (c0 kept)
        chk(lib.kwy_convert_mcep_dev(h, _p(self.mc_c), T, order, self.gmm.M, _p(self.gmm_model), _p(self.mc_c2)))
        # `feature.mel_cepstrum = converted` -> resample_data(fs): back through the converter rate's grid
        chk(lib.kwy_mc2sp_dev(h, _p(self.mc_c2), T, order, self.alpha_c, 2 * (self.Kc - 1), _p(self.spec_c)))
        if not up_first:
            self.rng.stream.wait_stream(self.stream)
            self.rng.abs_normal(EPS / fc, out=self.silent)
            self.stream.wait_event(self.rng.record_event())
            self.back[:, :self.Kc].copy_(self.spec_c)
            self.back[:, self.Kc:].copy_(self.silent)
        else:
            self.back.copy_(self.spec_c[:, :self.n_back])
        chk(lib.kwy_sp2mc_dev(h, _p(self.back), T, self.n_back, order, self.alpha, _p(self.mc_conv)))

    def run(self):
        h, fs, fft, K, order, T = self.ctx.handle, self.fs, self.fft, self.K, self.order, self.T
        chk = lambda rc: _lib.check(self.ctx, rc)  # noqa: E731
        with torch.cuda.stream(self.stream):
            chk(lib.kwy_cheaptrick_dev(h, _p(self.x), self.N, fs, _p(self.t), _p(self.f0), T, -0.15, 71.0, fft,
                                       float(fs), _p(self.sp)))
            chk(lib.kwy_d4c_dev(h, _p(self.x), self.N, fs, _p(self.t), _p(self.f0), T, 0.85, fft, _p(self.ap)))
            chk(lib.kwy_sp2mc_dev(h, _p(self.sp), T, K, order, self.alpha, _p(self.mc)))
            if self.mcep_fs is None:
                chk(lib.kwy_convert_mcep_dev(h, _p(self.mc), T, order, self.gmm.M, _p(self.gmm_model), _p(self.mc_conv)))
            else:
                self._convert_across_rates(chk, h)
            chk(lib.kwy_mc2sp_dev(h, _p(self.mc_conv), T, order, self.alpha, fft, _p(self.sp_conv)))
            chk(lib.kwy_synthesize_dev(h, _p(self.f0), T, _p(self.sp_conv), _p(self.ap), fft, self.frame_period, fs,
                                       float(fs), self.ylen, _p(self.wave)))

    def sync(self):
        self.ctx.sync()

    def contexts(self):
        """(a captured pass also holds addresses of the generator's scratch arena)"""
        cs = [self.ctx]
        if self.mcep_fs is not None and self.rng is not None and self.rng.ctx is not self.ctx:
            cs.append(self.rng.ctx)
        return cs


def _mlpg_em(mlpg_em):
    """the option of the EM trajectory conversion as `ConvertOptions.check` leaves it: None or an int within [0, 16]"""
    return ConvertOptions(mlpg_em=mlpg_em).check(0).mlpg_em


def _postfilter_beta(beta):
    """the strength of the formant emphasis as `ConvertOptions.check` leaves it: a float within [0, 1]"""
    return ConvertOptions(postfilter_beta=beta).check(0).postfilter_beta


def _convert_jobs(rows, mlpg_em=None, gvgen=None):
    """the jobs of a batched conversion from (mc, T, mc_out) rows: kwy_convert_job, or with mlpg_em set
    kwy_convert_em_job (no log-likelihoods asked for), or with gvgen set kwy_convert_gv_job (no objective either)"""
    if gvgen is not None:
        return _lib.job_array(_lib.ConvertGvJob, [tuple(row) + (None, None) for row in rows])
    if mlpg_em is None:
        return _lib.job_array(_lib.ConvertJob, rows)
    return _lib.job_array(_lib.ConvertEmJob, [tuple(row) + (None,) for row in rows])


def _convert_mcep_batch(handle, jobs, n, order, M, model, mlpg_em=None, gvgen=None, offset=0, status=None):
    """kwy_convert_mcep_batch_dev over `_convert_jobs(rows, mlpg_em, gvgen)`, kwy_convert_mcep_em_batch_dev when mlpg_em
    is set, kwy_convert_mcep_gv_batch_dev when gvgen (`ConvertOptions.upload`) is: -> the return code.  offset: 1 for a
    model prepared with diff = 1 (the variance is that of trajectory + source); status: n int32 words on the device"""
    if gvgen is not None:
        return lib.kwy_convert_mcep_gv_batch_dev(handle, jobs, n, order, M, _p(model), -1 if mlpg_em is None else mlpg_em,
                                                 int(offset), _p(gvgen['mean']), _p(gvgen['var']), gvgen['weight'],
                                                 gvgen['iterations'], None if status is None else _p(status))
    if mlpg_em is None:
        return lib.kwy_convert_mcep_batch_dev(handle, jobs, n, order, M, _p(model))
    return lib.kwy_convert_mcep_em_batch_dev(handle, jobs, n, order, M, _p(model), mlpg_em)


def _check_gvgen_status(status):
    bad = [i for i, v in enumerate(status.tolist() if hasattr(status, 'tolist') else status) if v]
    if bad:
        raise ValueError(f'GV ascent: coefficients of utterance(s) {bad} were left at the maximum-likelihood track: their '
                         f'variance is not finite, or a statistic is not finite or not positive there')


class _McFilter:
    """A filter of a wave's converted mel-cepstra `conv` as one unit: its buffers, its jobs over the plain rows and --
    with `diff_rows`, the rows of the differential conversion -- over those, `words` status words per utterance (the
    plain conversion's, then the differential one's), `prepare` and `launch` on the main stream.  early: the filter
    changes the plain rows in place and the differential rows take that change (the jobs' base is `conv`), so they are
    filtered right before the plain ones; otherwise after the rendering."""

    def prepare(self, chk, h):
        pass


class _MsFilter(_McFilter):
    """The modulation-spectrum postfilter (kwy_ms_postfilter_batch_dev on c1..cN, in place)"""
    kind, early, words = 'ms', True, 1

    def __init__(self, pair, strength, conv, T, diff_rows, dev):
        from .backend import ms as msfilter
        self.pair, self.strength, self.n, self.cols = pair, strength, len(T), pair[0].shape[0]
        self.length = 2 * (pair[0].shape[1] - 1)
        msfilter._fits(T, self.length)
        self.status = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.jobs, self.jobs_diff = (None if out is None else _lib.job_array(
            _lib.MsJob, [(conv[i], T[i], out[i], out[i]) for i in range(self.n)]) for out in (conv, diff_rows))

    def launch(self, chk, h, differential=False):
        chk(lib.kwy_ms_postfilter_batch_dev(h, self.jobs_diff if differential else self.jobs, self.n, self.cols, 1,
                                            self.length, _p(self.pair[0]), _p(self.pair[1]), self.strength,
                                            None if differential else _p(self.status)))


class _GvFilter(_McFilter):
    """The global-variance postfilter (kwy_column_moments_batch_dev, then kwy_gv_postfilter_batch_dev on c1..cN, in
    place).  status: the caller's words instead of its own"""
    kind, early, words = 'gv', True, 1

    def __init__(self, gv, strength, conv, T, diff_rows, dev, status=None):
        self.gv, self.strength, self.n, self.cols = gv, strength, len(T), gv.numel()
        self.moments = torch.empty((self.n, self.cols, 3), dtype=torch.float64, device=dev)
        self.status = status if status is not None else torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.j_mom = _lib.job_array(_lib.GvMatrix, [(conv[i], T[i]) for i in range(self.n)])
        self.jobs, self.jobs_diff = (None if out is None else _lib.job_array(
            _lib.GvJob, [(conv[i], T[i], self.moments[i], out[i], out[i]) for i in range(self.n)])
            for out in (conv, diff_rows))

    def prepare(self, chk, h):
        chk(lib.kwy_column_moments_batch_dev(h, self.j_mom, self.n, self.cols, _p(self.moments)))

    def launch(self, chk, h, differential=False):
        chk(lib.kwy_gv_postfilter_batch_dev(h, self.jobs_diff if differential else self.jobs, self.n, self.cols, 1,
                                            _p(self.gv), self.strength, None if differential else _p(self.status)))


class _PowerFilter(_McFilter):
    """The formant emphasis / the power-preserving c0 on the ABSOLUTE converted rows, last of the filters
    (kwy_mcep_postfilter_batch_dev).  The plain conversion in place; the differential
    one as the base of source + differential (`mc` + `mc_diff` into a block of its own, column 0 of `mc_diff` zeroed
    first: it then carries the difference of c0, and the differential filter reads it).  env: the source's rows, whose
    frame energies keep_power restores"""
    kind, early = 'power', False

    def __init__(self, beta, keep_power, conv, env, T, diff_rows, rows, mc, mc_diff, scalars, dev):
        self.beta, self.n, self.scalars, self.mc, self.mc_diff = beta, len(T), scalars, mc, mc_diff      # scalars: order, alpha, fft
        self.words = 1 if diff_rows is None else 2
        self.status = torch.zeros(self.words * self.n, dtype=torch.int32, device=dev)
        ref = env if keep_power else [None] * self.n
        self.jobs = _lib.job_array(_lib.McPowerJob, [(conv[i], ref[i], None, conv[i], T[i]) for i in range(self.n)])
        if diff_rows is not None:
            self.mc_abs = torch.empty_like(mc)
            absolute = rows.views(self.mc_abs)
            self.jobs_diff = _lib.job_array(_lib.McPowerJob, [(absolute[i], ref[i], diff_rows[i], diff_rows[i], T[i])
                                                              for i in range(self.n)])

    def launch(self, chk, h, differential=False):
        if differential:
            self.mc_diff[:, 0] = 0.0
            torch.add(self.mc, self.mc_diff, out=self.mc_abs)
        words = self.status[self.n:] if differential else self.status[:self.n]
        chk(lib.kwy_mcep_postfilter_batch_dev(h, self.jobs_diff if differential else self.jobs, self.n, *self.scalars,
                                              self.beta, _p(words)))


# All that the MLSA pass behind the last wave of a batch reads of a wave: its MlsaJob rows (inputs, differential
# mel-cepstra, outputs), `finish` -- None, or (the FinishJob array of the outputs, their count, the block of 16-bit samples
# it points into) -- and the filter's scalars
_DeferredMlsa = namedtuple('_DeferredMlsa', 'rows finish alpha hop ignore_c0')


def _finish_diff(ctx, jobs, n, fs):
    """Wavdata.save's normalisation of `n` filtered waveforms (a filtered waveform has no synthesis post-step)"""
    _lib.check(ctx, lib.kwy_finish_pcm16_batch_dev(ctx.handle, jobs, n, fs, 0, PIECE_CEILING, 1, PIECE_CEILING))


class ConvertWave:
    """<= 16 utterances analysed and rendered in lockstep (the batched entries of include/kwy.h on two streams): with a
    prepared GMM model the mel-cepstra are converted in between (convert_voice.convert(diffvc=False) of every file,
    /root/reference/kwiiyatta/convert_voice.py:35-46), without one the features are resynthesised as they are
    (resynthesize_voice.py:46-79, BASELINE config 4).  Utterances of any lengths; `wave[i]` are views of one block.

    An utterance is an (x, f0, t) triple, or a bare waveform (numpy array / device tensor): then its f0 track is
    extracted inside the wave -- DIO + StoneMask on the device (kwy_dio_batch_dev, kwy_stonemask_batch_dev:
    Analyzer.extract_f0, /root/reference/kwiiyatta/vocoder/world.py:33-41) -- and `f0_status` holds one word per
    utterance to read back (non-zero: DIO's zero-crossing buffer overflowed).  pcm=True: the post-step and the 16-bit
    samples on the device as well (kwy_finish_pcm16_batch_dev: vocoder/abc/synthesizer.py:11-20, wavfile.py:8-29):
    `pcm[i]` int16 views, 2 bytes per sample to download.  diff=True (with a GMM): also the DIFFERENTIAL output of
    every file -- the input waveform through the MLSA filter of the differential conversion, convert(diffvc=True),
    /root/reference/kwiiyatta/convert_voice.py:19,39-40, filter/mlsa.py:9-30 -- as `wave_diff[i]` (and `pcm_diff[i]`:
    Wavdata.save's normalisation only).  defer_mlsa=True: the caller launches the MLSA recursions of several waves
    together, from their `deferred()` records.

    **options: the keywords of `ConvertOptions`, which describes each; resolved: `ConvertOptions.upload`'s result instead,
    as a driver hands it to all its waves.  What the wave adds to them:
    the mapped f0 is `f0_synth`; the status words to read back -- all None when their option is off -- are
    `f0_map_status`, `gv_status`, `ms_status` (a word per utterance), `formant_status` (one word for the wave),
    `gvgen_status` and with diff=True `power_status` (two words per utterance: the plain conversion's, then the
    differential one's); `status_words()` lists them.
    The filters of the converted mel-cepstra run in the order MS, GV, power / emphasis (`filters`: a unit each, see
    `_McFilter`).  The differential conversion has ONE place: right before the first filter that changes the plain
    conversion in place (MS or GV; it then has no GV ascent and offset 0, and takes those filters' changes of the plain
    conversion before the plain rows are overwritten), and without such a filter after the rendering (with the ascent
    options, offset 1).  With formant_ratio = 1, and with the power filter's options both neutral, no kernel is launched
    and no buffer added.
    ap_gmm (a DeviceGMM over 6 B dimensions, B the aperiodicity bands of fs; None: off, no call, buffer or status word
    is added): the aperiodicity the rendering reads is converted too -- band track, prepared-model MLPG at d = B and the
    in-place apply (kwy_bap_track / kwy_convert_mcep / kwy_bap_apply _batch_dev) on the SIDE stream right behind D4C,
    beside the mel-cepstrum conversion on the main stream; `ap_all` then holds the converted rows.  Independent of
    `gmm`; the differential outputs do not read the aperiodicity."""

    @takes_options()
    def __init__(self, ls, fs, utterances, gmm=None, order=24, frame_period=5.0, pcm=False, diff=False, defer_mlsa=False,
                 resolved=None, ap_gmm=None, f0_estimator='dio', **options):
        converting = gmm is not None
        self.f0_estimator = check_f0_estimator(f0_estimator)     # of bare waveforms: 'dio' or 'pyin' in front of StoneMask
        self.ap_gmm = ap_gmm
        opts = resolved or ConvertOptions(**options).check(order, converting).upload(ls.dev, converting)
        self.opts, self.mlpg_em, self.gvgen, self.gvgen_status = opts, opts.mlpg_em, opts.gvgen, None
        self.ls, self.fs, self.order, self.frame_period = ls, int(fs), int(order), float(frame_period)
        self.diff, self.defer_mlsa, self.formant_status = bool(diff) and converting, bool(defer_mlsa), None
        self.wav_in = len(utterances) > 0 and not isinstance(utterances[0], (tuple, list))
        dev = ls.dev
        self.fft = lib.kwy_cheaptrick_fft_size(self.fs, 71.0)
        self.K = K = self.fft // 2 + 1
        from .backend import sptk
        self.alpha = sptk.mcepalpha(self.fs)
        self.gmm = gmm
        self.n = n = len(utterances)
        f64 = dict(dtype=torch.float64, device=dev)
        with torch.cuda.stream(ls.main):
            self.model = gmm.model(diff=False) if converting else None
            both = (ls.main, ls.side)           # the inputs: both streams may use them after the caller has dropped them
            if self.wav_in:
                self.x = [to_device(u, dev, both) for u in utterances]
                self.T = [int(lib.kwy_dio_frames(self.fs, v.numel(), self.frame_period)) for v in self.x]
                rows = Ragged(self.T)           # the layout of every per-frame block: the utterances' frames end to end
                self.t, self.f0_dio, self.f0 = (rows.views(torch.empty(rows.total, **f64)) for _ in range(3))
                self.f0_status = torch.zeros(n, dtype=torch.int32, device=dev)
                self.j_dio, self.j_sm = f0_jobs(self.x, self.t, self.f0_dio, self.f0, self.f0_status)
            else:
                us = [[to_device(a, dev, both) for a in u] for u in utterances]
                self.x, self.f0, self.t = ([u[k] for u in us] for k in range(3))
                self.T = [len(v) for v in self.f0]
                rows = Ragged(self.T)
                self.f0_status = None
            self.rows = rows.total
            # (with a GMM nothing reads the analysed envelopes but sp2mc: CheapTrick hands over mel-cepstra instead,
            # kwy_cheaptrick_mcep_batch_dev)
            self.sp_all = torch.empty((self.rows, K), **f64) if not converting else None
            self.ap_all = torch.empty((self.rows, K), **f64)
            self.ylen = [int(lib.kwy_synth_length(t, self.frame_period, self.fs)) for t in self.T]
            out = Ragged(self.ylen)
            self.wave_all = torch.empty(out.total, **f64)
            self.wave = out.views(self.wave_all)
            self.pcm = None
            if pcm:
                self.pcm_all = torch.zeros(out.total, dtype=torch.int16, device=dev)
                self.pcm = out.views(self.pcm_all)
                self.j_fin = _lib.job_array(_lib.FinishJob, [(self.wave[i], self.ylen[i], self.T[i], self.pcm[i])
                                                             for i in range(n)])
            self.plan = [torch.empty(int(lib.kwy_synth_plan_bytes(y)), dtype=torch.uint8, device=dev) for y in self.ylen]
            self.f0_synth, self.f0_map_status = self.f0, None
            if opts.f0_map:
                self.f0_synth_all = torch.empty(self.rows, **f64)
                self.f0_synth = rows.views(self.f0_synth_all)
                self.f0_map_status = torch.zeros(n, dtype=torch.int32, device=dev)
                self.j_map = _lib.job_array(_lib.F0MapJob, [(self.f0[i], self.T[i], self.f0_synth[i]) for i in range(n)])
            if converting:
                assert gmm.D2 == 6 * order
                self.mc = torch.empty((self.rows, order + 1), **f64)
            # CheapTrick's rows (envelopes, or mel-cepstra for the conversion) and the rows the rendering reads
            env, ap = rows.views(self.mc if converting else self.sp_all), rows.views(self.ap_all)
            spec = env
            self.j_env = _lib.utterance_array([(self.x[i], self.t[i], self.f0[i], env[i]) for i in range(n)])
            self.j_ap = _lib.utterance_array([(self.x[i], self.t[i], self.f0[i], ap[i]) for i in range(n)])
            self.j_plan = _lib.job_array(_lib.SynthPlanJob, [(self.f0_synth[i], self.T[i], self.ylen[i], self.plan[i])
                                                             for i in range(n)])
            if ap_gmm is not None:
                from .backend import bap
                self.bands = B = bap.check_rate(self.fs)
                if ap_gmm.D2 != 6 * B:
                    raise ValueError(f'ap_gmm has {ap_gmm.D2} joint dimensions, {self.fs} Hz has {B} band(s): {6 * B}')
                self.ap_model = ap_gmm.model(diff=False)
                self.ap_src, self.ap_conv = (torch.empty((self.rows, B + 1), **f64) for _ in range(2))
                src, mapped = rows.views(self.ap_src), rows.views(self.ap_conv)
                self.j_bap = (_lib.job_array(_lib.BapTrackJob, [(ap[i], self.T[i], src[i]) for i in range(n)]),
                              _lib.job_array(_lib.ConvertJob, [(src[i], self.T[i], mapped[i]) for i in range(n)]),
                              _lib.job_array(_lib.BapApplyJob, [(src[i], mapped[i], self.T[i], ap[i]) for i in range(n)]))
            if converting:
                self.mc_conv = torch.empty((self.rows, order + 1), **f64)
                self.sp_conv = torch.empty((self.rows, K), **f64)
                conv, spec = rows.views(self.mc_conv), rows.views(self.sp_conv)
                self.j_conv = _convert_jobs([(env[i], self.T[i], conv[i]) for i in range(n)], self.mlpg_em, self.gvgen)
                if self.gvgen is not None:
                    self.gvgen_status = torch.zeros(2 * n, dtype=torch.int32, device=dev)
            self.mc_diff = self.mc_diff_rows = None
            if self.diff:
                self.model_diff = gmm.model(diff=True)
                self.mc_diff = torch.empty((self.rows, order + 1), **f64)
                self.mc_diff_rows = rows.views(self.mc_diff)
                self.j_conv_diff = _convert_jobs([(env[i], self.T[i], self.mc_diff_rows[i]) for i in range(n)], self.mlpg_em,
                                                 self.gvgen)
                samples = Ragged([v.numel() for v in self.x])         # the filtered inputs: as long as the inputs
                self.wave_diff_all = torch.empty(samples.total, **f64)
                self.wave_diff = samples.views(self.wave_diff_all)
                # (as rows too, for ONE launch over the utterances of several waves: a recursion occupies one wavefront
                # for 0.6 us per sample whatever else runs, so all files of a batch should recurse side by side)
                self.mlsa = [(self.x[i], self.x[i].numel(), self.mc_diff_rows[i], self.T[i], self.wave_diff[i]) for i in range(n)]
                self.j_mlsa = _lib.job_array(_lib.MlsaJob, self.mlsa)
                self.hop = int(self.fs * (self.frame_period * 0.001))
                if opts.diff_filter == 'fft':
                    from .backend import fftfilt
                    self.diff_fft = fftfilt.fft_filter_size(self.fs, self.hop)
                self.pcm_diff = None
                if pcm:
                    self.pcm_diff_all = torch.zeros(samples.total, dtype=torch.int16, device=dev)
                    self.pcm_diff = samples.views(self.pcm_diff_all)
                    self.j_fin_diff = _lib.job_array(_lib.FinishJob, [(self.wave_diff[i], self.x[i].numel(), 0, self.pcm_diff[i])
                                                                      for i in range(n)])
            self.filters = []
            if converting:
                if opts.ms is not None:
                    self.filters.append(_MsFilter(opts.ms, opts.ms_strength, conv, self.T, self.mc_diff_rows, dev))
                if opts.gv is not None:
                    self.filters.append(_GvFilter(opts.gv, opts.gv_strength, conv, self.T, self.mc_diff_rows, dev))
                if opts.power:
                    self.filters.append(_PowerFilter(opts.postfilter_beta, opts.keep_power, conv, env, self.T,
                                                     self.mc_diff_rows, rows, self.mc, self.mc_diff,
                                                     (order, self.alpha, self.fft), dev))
            status = {f.kind: f.status for f in self.filters}
            self.ms_status, self.gv_status, self.power_status = (status.get(kind) for kind in ('ms', 'gv', 'power'))
            # the ONE place of the differential conversion: in front of this filter, or (None) after the rendering
            self.diff_before = next((f for f in self.filters if f.early), None) if self.diff else None
            self.ignore_c0 = 0 if self.power_status is not None else 1
            self.j_render = _lib.synth_job_array([(self.plan[i], spec[i], ap[i], self.wave[i]) for i in range(n)])
            if opts.formant_ratio != 1:
                self.formant_status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.frames = int(sum(self.T))

    def status_words(self):
        """(kind, device words, words per utterance) of every status the wave's options write"""
        own = [(self.f0_estimator, self.f0_status, 1), ('f0_map', self.f0_map_status, 1), ('formant', self.formant_status, 1),
               ('gvgen', self.gvgen_status, 2)] + [(f.kind, f.status, f.words) for f in self.filters]
        return [item for item in own if item[1] is not None]

    def run(self):
        ls, fs, fft, K, order, n, opts = self.ls, self.fs, self.fft, self.K, self.order, self.n, self.opts
        if self.wav_in:
            with torch.cuda.stream(ls.main):
                coarse_f0_batch_dev(ls.ctx, self.f0_estimator, self.j_dio, n, fs, self.frame_period, lib=lib)
                _lib.check(ls.ctx, lib.kwy_stonemask_batch_dev(ls.ctx.handle, self.j_sm, n, fs))
        ls.side.wait_stream(ls.main)
        with torch.cuda.stream(ls.side):
            hs = ls.side_ctx.handle
            _lib.check(ls.side_ctx, lib.kwy_d4c_batch_dev(hs, self.j_ap, n, fs, 0.85, fft))
            if self.ap_gmm is not None:
                track, convert, apply = self.j_bap
                _lib.check(ls.side_ctx, lib.kwy_bap_track_batch_dev(hs, track, n, fs, fft))
                _lib.check(ls.side_ctx, lib.kwy_convert_mcep_batch_dev(hs, convert, n, self.bands, self.ap_gmm.M,
                                                                       _p(self.ap_model)))
                _lib.check(ls.side_ctx, lib.kwy_bap_apply_batch_dev(hs, apply, n, fs, fft))
            if self.f0_map_status is not None:
                from .backend.f0 import key_ratio
                _lib.check(ls.side_ctx, lib.kwy_f0_map_batch_dev(
                    hs, self.j_map, n, fs, None if opts.f0_stats is None else opts.f0_stats.data_ptr(),
                    key_ratio(opts.transpose_key), self.f0_map_status.data_ptr()))
            _lib.check(ls.side_ctx, lib.kwy_synth_plan_batch_dev(hs, self.j_plan, n, fft, self.frame_period, fs))
        with torch.cuda.stream(ls.main):
            h = ls.ctx.handle
            chk = lambda rc: _lib.check(ls.ctx, rc)  # noqa: E731
            if self.gmm is None:
                chk(lib.kwy_cheaptrick_batch_dev(h, self.j_env, n, fs, -0.15, 71.0, fft, float(fs)))
            else:
                chk(lib.kwy_cheaptrick_mcep_batch_dev(h, self.j_env, n, fs, -0.15, 71.0, fft, float(fs), order, self.alpha))
                chk(_convert_mcep_batch(h, self.j_conv, n, order, self.gmm.M, self.model, self.mlpg_em, self.gvgen, 0,
                                        None if self.gvgen is None else self.gvgen_status[:n]))
                for f in self.filters:
                    f.prepare(chk, h)
                    if self.diff and f.early:
                        if f is self.diff_before:
                            self._convert_diff(chk, h, late=False)
                        f.launch(chk, h, differential=True)
                    f.launch(chk, h)
                chk(lib.kwy_mc2sp_dev(h, _p(self.mc_conv), self.rows, order, self.alpha, fft, _p(self.sp_conv)))
            if self.formant_status is not None:     # the rows the rendering reads, warped in place
                rendered = self.sp_all if self.gmm is None else self.sp_conv
                chk(lib.kwy_formant_shift_dev(h, _p(rendered), self.rows, K, opts.formant_ratio, _p(rendered),
                                              _p(self.formant_status)))
            ls.main.wait_stream(ls.side)
            chk(lib.kwy_synth_render_batch_dev(h, self.j_render, n, fft, self.frame_period, fs, float(fs)))
            if self.pcm is not None:
                chk(lib.kwy_finish_pcm16_batch_dev(h, self.j_fin, n, fs, 1, PIECE_CEILING, 1, PIECE_CEILING))
            if self.diff:
                # the differential conversion of the same mel-cepstra, its filter over the INPUT waveforms: all
                # utterances' recursions side by side (one wavefront each)
                if self.diff_before is None:
                    self._convert_diff(chk, h, late=True)
                for f in self.filters:
                    if not f.early:
                        f.launch(chk, h, differential=True)
                if opts.diff_filter == 'fft' or not self.defer_mlsa:
                    self.filter_diff(ls.ctx)

    def _convert_diff(self, chk, h, late):
        """the differential conversion; late (behind the rendering): with the GV ascent, on the variance of
        differential + source (offset 1)"""
        gvgen = self.gvgen if late else None
        chk(_convert_mcep_batch(h, self.j_conv_diff, self.n, self.order, self.gmm.M, self.model_diff, self.mlpg_em, gvgen,
                                int(late), None if gvgen is None else self.gvgen_status[self.n:]))

    def deferred(self):
        """what a deferred MLSA pass needs of the wave, and nothing else of it"""
        return _DeferredMlsa(self.mlsa, None if self.pcm_diff is None else (self.j_fin_diff, self.n, self.pcm_diff_all),
                             self.alpha, self.hop, self.ignore_c0)

    def filter_diff(self, ctx):
        """the wave's differential outputs: the MLSA recursions, or the frame-parallel FFT filter over the same jobs
        (every frame of every file in one grid: nothing to defer), and their post-step"""
        if self.opts.diff_filter == 'fft':
            _lib.check(ctx, lib.kwy_mcep_filter_fft_batch_dev(ctx.handle, self.j_mlsa, self.n, self.order, self.alpha,
                                                              self.hop, self.diff_fft, self.ignore_c0))
        else:
            _lib.check(ctx, lib.kwy_mlsa_filter_batch_dev(ctx.handle, self.j_mlsa, self.n, self.order, self.alpha, 4,
                                                          self.hop, self.ignore_c0))
        if self.pcm_diff is not None:
            _finish_diff(ctx, self.j_fin_diff, self.n, self.fs)


_STATUS_KINDS = ('dio', 'pyin', 'f0_map', 'gv', 'ms', 'formant', 'gvgen', 'power')


def _check_dio_status(status):
    if bool(status.any()):
        bad = torch.nonzero(status).flatten().tolist()
        raise RuntimeError(f'dio: zero-crossing buffer overflow in utterance(s) {bad} (signal too noisy for the band filters)')


def _check_status_words(items, fs):
    """The status words of a batch's waves, read back ONCE: items are the waves' (kind, device words, words per
    utterance) in the order they ran; one concatenation, one copy to the host, then the kinds' checks in the order of
    `_STATUS_KINDS` (several words per utterance: the plain conversion's of a whole wave, then the differential one's,
    folded into one)."""
    if not items:
        return
    from .backend import f0, formant, gv, ms, power
    items = sorted(items, key=lambda item: _STATUS_KINDS.index(item[0]))        # (stable: a kind's waves stay in order)
    host = torch.cat([w for _, w, _ in items]).cpu().split([w.numel() for _, w, _ in items])
    folded = {}
    for (kind, w, per), words in zip(items, host):
        folded.setdefault(kind, []).append(words.reshape(per, w.numel() // per).sum(0))
    checks = dict(dio=_check_dio_status, pyin=lambda w: check_f0_status('pyin', w), f0_map=lambda w: f0.check_status(w, fs), gv=gv.check_status, ms=ms.check_status,
                  formant=lambda w: formant.check_status(w, what='wave(s)'), gvgen=_check_gvgen_status,
                  power=power.check_status)
    for kind, parts in folded.items():
        checks[kind](torch.cat(parts))


def _lockstep_batch(utterances, fs, device_index, gmm, order, frame_period, ls, keep, opts, wave_size=16, pcm=False,
                    diff=False, ap_gmm=None, f0_estimator='dio'):
    """utterances in waves of `wave_size` through ConvertWave; keep(i, waveform view, pcm view, differential waveform
    view, its pcm view) on the main stream, None for what was not asked for.  opts: a checked `ConvertOptions`, uploaded
    here once for all waves.
    Bare waveforms get their f0 on the device; the status words of all waves are read back ONCE at the end
    (`_check_status_words`).  ap_gmm: a DeviceGMM for every wave's aperiodicity conversion (`ConvertWave`), or None."""
    if gmm is not None and opts.ms_strength > 0:
        # an utterance longer than the transform is a ValueError BEFORE the batch (`ConvertOptions`): every frame count is
        # known here, and the per-wave check of `_MsFilter` would fire with the earlier waves already enqueued
        from .backend import ms as msfilter
        bare = len(utterances) > 0 and not isinstance(utterances[0], (tuple, list))
        msfilter._fits([int(lib.kwy_dio_frames(int(fs), len(u), float(frame_period))) if bare else len(u[1])
                        for u in utterances], 2 * (np.shape(opts.ms_stats[0])[1] - 1))
    ls = ls if ls is not None else _Lockstep(device_index)
    resolved = opts.upload(ls.dev, converting=gmm is not None)
    defer = bool(diff) and gmm is not None and resolved.diff_filter == 'mlsa'
    held, deferred, status = [], [], []
    for w0 in range(0, len(utterances), wave_size):
        wv = ConvertWave(ls, fs, utterances[w0:w0 + wave_size], gmm=gmm, order=order, frame_period=frame_period, pcm=pcm,
                         diff=diff, defer_mlsa=defer, resolved=resolved, ap_gmm=ap_gmm, f0_estimator=f0_estimator)
        wv.run()
        with torch.cuda.stream(ls.main):
            for i in range(wv.n):
                keep(w0 + i, wv.wave[i], wv.pcm[i] if pcm else None, wv.wave_diff[i] if wv.diff else None,
                     wv.pcm_diff[i] if wv.diff and pcm else None)
        status += wv.status_words()
        if defer:
            deferred.append(wv.deferred())            # (the wave itself goes when it leaves `held`)
        held.append(wv)
        while len(held) > 2:
            held.pop(0)
    if deferred:
        # the differential outputs of ALL files: one pass of launches over every recursion (64 per launch; two contexts
        # alternate so that consecutive launches overlap), then their post-step
        rows = [r for d in deferred for r in d.rows]
        d0 = deferred[0]
        ls.side.wait_stream(ls.main)
        for k, c0 in enumerate(range(0, len(rows), 64)):
            ctx = (ls.ctx, ls.side_ctx)[k % 2]
            with torch.cuda.stream((ls.main, ls.side)[k % 2]):
                chunk = rows[c0:c0 + 64]
                _lib.check(ctx, lib.kwy_mlsa_filter_batch_dev(ctx.handle, _lib.job_array(_lib.MlsaJob, chunk), len(chunk), order,
                                                              d0.alpha, 4, d0.hop, d0.ignore_c0))
        ls.main.wait_stream(ls.side)
        with torch.cuda.stream(ls.main):
            for jobs, n, _ in (d.finish for d in deferred if d.finish is not None):
                _finish_diff(ls.ctx, jobs, n, int(fs))
    ls.sync()
    _check_status_words(status, fs)
    return ls


class StreamPool:
    """`n` HIP streams with one library context each (a context owns constant tables and a scratch arena: built
    once per stream, not once per utterance).

    Streams only overlap when they land on different hardware queues; the HIP runtime creates 4 unless the
    application exports GPU_MAX_HW_QUEUES before HIP starts (bench.py and bench_corpus.py set 32, the chip's
    hardware queues, see bench.py).  The package does
    not touch the environment: with fewer queues than streams the pool still works, the streams just share."""

    def __init__(self, device_index, n):
        self.dev = torch.device('cuda', device_index)
        import os
        import warnings
        queues = os.environ.get('GPU_MAX_HW_QUEUES')
        if n > 4 and queues is None:
            warnings.warn(f'{n} streams, but GPU_MAX_HW_QUEUES is not set: the HIP runtime maps all streams onto 4 '
                          f'hardware queues and most of the overlap between utterances is lost; export it before the '
                          f'first HIP call', RuntimeWarning, stacklevel=2)
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(max(1, n))]
        self.contexts = [_lib.Context(device_index, stream=s.cuda_stream) for s in self.streams]

    def __len__(self):
        return len(self.streams)


def shard_block(n_items, rank, world_size):
    """Contiguous block of items for `rank`: the concatenation over ranks is the original order."""
    if not (0 <= rank < world_size):
        raise ValueError(f'rank {rank} outside world of size {world_size}')
    lo = n_items * rank // world_size
    hi = n_items * (rank + 1) // world_size
    return list(range(lo, hi))


class _Ahead:
    """The items of an iterable, evaluated on a helper thread at most `depth` ahead of the consumer, while the caller
    enqueues GPU work.  An exception of the producer is handed over: `get()` raises it where the item would have been.
    `stop()` (the drivers always call it, also when a pair raises) ends the thread: none is left behind producing."""

    def __init__(self, items, depth):
        import queue
        import threading
        self.q = queue.Queue(maxsize=max(1, depth))
        self.halt = threading.Event()

        def hand(item):
            while not self.halt.is_set():
                try:
                    self.q.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    continue
            return False

        def work():
            try:
                for item in items:
                    if not hand(item):
                        return
            except Exception as exc:
                hand(exc)
        self.thread = threading.Thread(target=work, daemon=True)
        self.thread.start()

    def get(self):
        item = self.q.get()
        if isinstance(item, Exception):
            raise item
        return item

    def stop(self):
        self.halt.set()
        self.thread.join(timeout=5.0)


def _pair_silences(n_pairs, fs):
    """the pad spectra of consecutive pairs, drawn from numpy's global legacy generator (the reference's source,
    `draw_silence`).  On an `_Ahead` thread: the generator is serial (4.6 ms per pair at 48 kHz) and numpy releases the
    GIL inside it.  The caller must not use `np.random` until `stop()`, after which no global draws are consumed."""
    K = lib.kwy_cheaptrick_fft_size(int(fs), 71.0) // 2 + 1
    for _ in range(n_pairs):
        yield [draw_silence(fs, K) for _ in range(4)]


def _pair_uploads(pairs, dev):
    """the waveforms, f0 tracks and frame times of consecutive pairs as device tensors, each copy complete when handed
    over.  On an `_Ahead` thread: a copy from pageable host memory blocks its caller (0.2 ms per 5 s waveform at 48 kHz,
    six copies per pair: 0.5 ms of the ~1.3 ms of host time a pair costs) and releases the interpreter lock meanwhile."""
    for pair in pairs:
        yield tuple(tuple(to_device(a, dev) for a in side) for side in pair)


def build_training_matrix(pairs, fs, device_index=0, order=24, radius=32, frame_period=5.0, streams=16,
                          silence_for=None, pool=None, rng=None, pairs_before=0, driver=None, lockstep=None,
                          wave_pairs=16, f0_moments=False, gv_moments=False, keep=False, gv_variance=False, bands=False):
    """driver='lockstep' (default): waves of `wave_pairs` pairs through the batched entries on two streams
    (`TrainWave`; `lockstep`: a _Lockstep to reuse), rows appended behind a device-side cursor, one read-back per wave;
    driver='streams': the pair-per-stream driver (`TrainPair`, below).  Same matrix either way.
    f0_moments=True: a third result, the (2, 3) numpy array of the merged voiced log-f0 moments (n, mean, M2) of the
    source and of the target side -- each side's trimmed f0 tracks, merged in pair order on the device
    (MelCepstrumFeatureConverter.train(f0_stats=True)'s statistics; backend.f0.stats_from_moments).
    gv_moments=True: a further result (after the f0 moments when both are asked for), the numpy vector of order + 1
    values of the target side's global variance -- the column moments of every pair's trimmed target mel-cepstra as
    the matrix path computes them, folded in pair order on the device (train(gv_stats=True)'s statistic).
    gv_variance=True (with gv_moments=True): one more result behind it, the order + 1 values of the variance over the
    pairs of the same per-utterance variance (train(gv_stats=True)'s `gv_var`, for mlpg_gv).
    keep=True (lockstep driver): a third result right behind (X, frames), the `TrainCache` with the alignment inputs of
    every pair for `realign_training_matrix`; the default keeps nothing, the waves' buffers go as they went before.
    bands=True (lockstep driver; fs of 12 kHz or more, ValueError otherwise before anything is read): one more result
    right behind (X, frames[, cache]), the band matrix (rows, 6 B) of the aperiodicity conversion -- the band rows of
    the same kept cells that both sides voice (include/kwy.h, "aperiodicity conversion"), appended behind a cursor of
    their own; with keep=True the cache holds the band tracks too."""
    driver = driver or ('streams' if pool is not None else 'lockstep')
    if bands:
        from .backend import bap
        if driver != 'lockstep':
            raise ValueError(f"build_training_matrix(bands=True) needs the lockstep driver, not driver={driver!r}")
        bap.check_rate(fs)
    if keep and driver != 'lockstep':
        raise ValueError(f"build_training_matrix(keep=True) needs the lockstep driver, not driver={driver!r}")
    if gv_variance and not gv_moments:
        raise ValueError('build_training_matrix(gv_variance=True) goes with gv_moments=True')
    moments = _PairMoments(len(pairs), device_index) if f0_moments else None
    gv = _PairGV(len(pairs), order, device_index) if gv_moments else None
    if driver == 'lockstep':
        out = _build_training_matrix_lockstep(pairs, fs, device_index, order, radius, frame_period, silence_for, rng,
                                              pairs_before, lockstep, wave_pairs, moments, gv, keep, bands)
    else:
        out = _build_training_matrix_streams(pairs, fs, device_index, order, radius, frame_period, streams, silence_for,
                                             pool, rng, pairs_before, moments, gv)
    if moments is not None:
        out = out + (moments.merged(),)
    if gv is None:
        return out
    return out + (gv.statistic(),) + ((gv.statistic(variance=True),) if gv_variance else ())


class _PairMoments:
    """per-track voiced log-f0 moments of a corpus's pairs in HBM: row 2 i the source, 2 i + 1 the target of pair i"""

    def __init__(self, n_pairs, device_index):
        self.dev = torch.device('cuda', device_index)
        self.rows = torch.empty((2 * n_pairs, 3), dtype=torch.float64, device=self.dev)     # every row is written

    def add(self, ctx, first_pair, tracks):
        """enqueue (on ctx's stream) the moments of `tracks`: the trimmed source and target f0 of consecutive pairs"""
        from .backend import f0 as f0map
        f0map.logf0_moments_batch_dev(ctx, tracks, self.rows[2 * first_pair:2 * first_pair + len(tracks)])

    def merged(self):
        """(after the streams that ran `add` are synchronised) the merged (source, target) triples"""
        if len(self.rows) == 0:
            return np.zeros((2, 3))
        from .backend import f0 as f0map
        ctx = _lib.Context(self.dev.index, stream=torch.cuda.current_stream(self.dev).cuda_stream)
        with torch.cuda.device(self.dev):
            out = torch.empty((2, 3), dtype=torch.float64, device=self.dev)
            # for the null stream the context runs a stream of its own: torch's copies are finished before it starts, and
            # it is finished before torch reads the result
            sides = [self.rows[side::2].contiguous() for side in (0, 1)]
            torch.cuda.current_stream(self.dev).synchronize()
            for side in (0, 1):
                f0map.merge_moments_dev(ctx, sides[side], out[side])
            ctx.sync()
            return out.cpu().numpy()


class _PairGV:
    """column moments of the trimmed target mel-cepstra of a corpus's pairs in HBM, one (order + 1, 3) block per pair"""

    def __init__(self, n_pairs, order, device_index):
        self.dev = torch.device('cuda', device_index)
        self.rows = torch.empty((n_pairs, order + 1, 3), dtype=torch.float64, device=self.dev)      # every block is written

    def add(self, ctx, first_pair, mats):
        """enqueue (on ctx's stream) the moments of `mats`: the trimmed target mel-cepstra of consecutive pairs"""
        from .backend import gv as gvfilter
        gvfilter.column_moments_batch_dev(ctx, mats, self.rows[first_pair:first_pair + len(mats)])

    def statistic(self, variance=False):
        """(after the streams that ran `add` are synchronised) the global variance, order + 1 values; variance=True: the
        variance over the pairs of the per-utterance variance instead (kwy_gv_stats_from_moments_dev)"""
        if len(self.rows) == 0:
            return np.zeros(self.rows.shape[1])
        from .backend import gv as gvfilter
        ctx = _lib.Context(self.dev.index, stream=torch.cuda.current_stream(self.dev).cuda_stream)
        with torch.cuda.device(self.dev):
            out = torch.empty(self.rows.shape[1], dtype=torch.float64, device=self.dev)
            if variance:
                mean = torch.empty_like(out)
                torch.cuda.current_stream(self.dev).synchronize()
                gvfilter.gv_statistics_dev(ctx, self.rows, mean, out)
            else:
                gvfilter.gv_from_moments_dev(ctx, self.rows, out)
            ctx.sync()            # (for the null stream the context runs a stream of its own, which .cpu() does not wait for)
            return out.cpu().numpy()


def _build_training_matrix_lockstep(pairs, fs, device_index, order, radius, frame_period, silence_for, rng, pairs_before,
                                    ls, wave_pairs, moments=None, gv=None, keep=False, bands=False):
    dev = torch.device('cuda', device_index)
    ls = ls if ls is not None else _Lockstep(device_index)
    cache = TrainCache(ls, fs, order, radius) if keep else None
    K = lib.kwy_cheaptrick_fft_size(int(fs), 71.0) // 2 + 1
    scale = 2.220446049250313e-16 / fs
    wave_pairs = max(1, min(16, int(wave_pairs)))
    B = lib.kwy_aperiodicity_bands(int(fs)) if bands else 0
    if not pairs:
        empty = lambda d: torch.empty((0, 6 * d), dtype=torch.float64, device=dev)  # noqa: E731
        return (empty(order), 0) + ((cache,) if keep else ()) + ((empty(B),) if bands else ())
    if rng is not None and pairs_before:
        with torch.cuda.stream(ls.main):
            sink = [torch.empty((PAD_LEN, K), dtype=torch.float64, device=dev) for _ in range(4 * 16)]
            left = pairs_before
            while left > 0:
                take = min(16, left)
                rng.abs_normal_blocks(scale, sink[:4 * take], ctx=ls.ctx)
                left -= take
    ahead = _Ahead(_pair_silences(len(pairs), fs), 2 * wave_pairs) if silence_for is None and rng is None else None
    uploads = _Ahead(_pair_uploads(pairs, dev), 3 * wave_pairs)
    # capacity of the matrix: a pair yields at most one row per path cell of its un-padded stretch
    cap_rows = sum(len(p[0][1]) + len(p[1][1]) for p in pairs)
    frames = 0
    done = [0]                # pairs whose pads have been handed out

    def pads(rows):
        n_pairs = len(rows) // 4
        if silence_for is not None or ahead is not None:
            for k in range(n_pairs):
                sil = silence_for(done[0] + k) if silence_for is not None else ahead.get()
                for dst, a in zip(rows[4 * k:4 * k + 4], sil):
                    dst.copy_(to_device(a, None), non_blocking=True)
        else:
            rng.abs_normal_blocks(scale, rows, ctx=ls.ctx)
        done[0] += n_pairs

    try:
        matrix = _RowSink(ls, cap_rows, order)
        band_matrix = _RowSink(ls, cap_rows, B) if bands else None
        prev, held = None, []           # prev: the wave that waits for its trim lengths, and its first pair

        def close(wave, first_pair):
            wave.finish(matrix, pads, cache, band_matrix)
            matrix.take(wave.alignment.n_rows)
            with torch.cuda.stream(ls.main):
                if moments is not None:
                    moments.add(ls.ctx, first_pair, [f[:k] for f, k in zip(wave.f0, wave.keep)])
                if gv is not None:
                    gv.add(ls.ctx, first_pair, [wave.reg(wave.mc_pad, 2 * k + 1)[PAD_LEN:PAD_LEN + wave.keep[2 * k + 1]]
                                                for k in range(wave.n)])
        for w0 in range(0, len(pairs), wave_pairs):
            chunk = [uploads.get() for _ in range(len(pairs[w0:w0 + wave_pairs]))]
            wave = TrainWave(ls, fs, chunk, order=order, radius=radius, frame_period=frame_period, bands=bands)
            wave.analyse()                     # enqueued BEFORE the host waits for the previous wave's lengths
            if prev is not None:
                close(*prev)
                held.append(prev[0])
            frames += wave.frames
            prev = (wave, w0)
            while len(held) > 2:
                held.pop(0)                    # (its buffers: all uses are ordered on the main stream before reuse)
        close(*prev)
        X, _ = matrix.close()
        Xb = band_matrix.close()[0] if bands else None
    finally:
        if ahead is not None:
            ahead.stop()
        uploads.stop()
    return (X, frames) + ((cache,) if keep else ()) + ((Xb,) if bands else ())


def _build_training_matrix_streams(pairs, fs, device_index=0, order=24, radius=32, frame_period=5.0, streams=16,
                                   silence_for=None, pool=None, rng=None, pairs_before=0, moments=None, gv=None):
    """pairs: list of ((x, f0, t), (x, f0, t)) numpy triples of THIS rank, in corpus order.  Returns the
    (n, 2*3*order) float64 device tensor of make_dataset_to_array and the number of source frames analysed.
    Pairs are processed `streams` at a time, each on its own stream (`pool`: a StreamPool to use instead of a new one).
    The pad spectra of pair i come from
      silence_for(i)   if given (four host arrays), else from
      rng              a DeviceRandomState: drawn on the GPU, in the reference's order, from numpy's legacy stream;
                       `pairs_before` pairs (those of the ranks before this one) are drawn and discarded first, so
                       that every pair gets the pads it would get on one rank, whatever the number of ranks; else from
      np.random        the global generator on the host, as the reference draws them, one wave of pairs ahead of the
                       GPU on a helper thread (bit-equal to the Python API path under np.random.seed)."""
    dev = torch.device('cuda', device_index)
    if pool is None:
        pool = StreamPool(device_index, streams)
    K = lib.kwy_cheaptrick_fft_size(int(fs), 71.0) // 2 + 1
    scale = 2.220446049250313e-16 / fs
    if rng is not None and pairs_before:
        with torch.cuda.stream(rng.stream):
            sink = [torch.empty((PAD_LEN, K), dtype=torch.float64, device=dev) for _ in range(4)]
            for _ in range(pairs_before):
                rng.abs_normal_blocks(scale, sink)
    ahead = _Ahead(_pair_silences(len(pairs), fs), 2 * len(pool)) if silence_for is None and rng is None and pairs else None
    uploads = _Ahead(_pair_uploads(pairs, dev), 2 * len(pool)) if pairs else None
    blocks, frames = [], 0

    def finish(wave, first_pair):
        """the host-dependent half of a wave: trim lengths back, alignment and row extraction enqueued, rows collected"""
        nonlocal frames
        for k, p in enumerate(wave):
            p.align()
            if moments is not None:
                with torch.cuda.stream(p.stream):
                    moments.add(p.ctx, first_pair + k, [p.src.f0[:p.src.n], p.tgt.f0[:p.tgt.n]])
            if gv is not None:
                with torch.cuda.stream(p.stream):
                    gv.add(p.ctx, first_pair + k, [p.tgt.mc_pad[PAD_LEN:PAD_LEN + p.tgt.n]])
        for p in wave:
            blocks.append(p.rows().clone())  # enqueued on the default stream after rows() has synchronised
            frames += p.frames
        torch.cuda.current_stream(dev).synchronize()     # the copies are done before the wave's buffers are released

    try:
        # Waves of len(pool) pairs, software-pipelined: the analysis of wave w + 1 is enqueued (same streams, behind
        # wave w's analysis) BEFORE the host turns to wave w's alignment, whose two read-backs per pair (trim lengths,
        # row count) would otherwise leave the GPU idle.
        prev = None
        for w0 in range(0, len(pairs), len(pool)):
            wave = []
            for k in range(len(pairs[w0:w0 + len(pool)])):
                src, tgt = uploads.get()        # (the pair's arrays, on the device already)
                ready = None
                if silence_for is not None:
                    sil = silence_for(w0 + k)
                elif rng is not None:
                    with torch.cuda.stream(rng.stream):
                        sil = rng.abs_normal_blocks(scale, [torch.empty((PAD_LEN, K), dtype=torch.float64, device=dev)
                                                            for _ in range(4)])
                    ready = rng.record_event()
                else:
                    sil = ahead.get()
                wave.append(TrainPair(device_index, fs, src, tgt, order=order, radius=radius,
                                      frame_period=frame_period, stream=pool.streams[k], ctx=pool.contexts[k],
                                      silence=sil, silence_ready=ready))
            for p in wave:
                p.analyse()
            if prev is not None:
                finish(prev, w0 - len(pool))
            prev = wave
        if prev is not None:
            finish(prev, (len(pairs) - 1) // len(pool) * len(pool))
        torch.cuda.synchronize(dev)
    finally:
        if ahead is not None:
            ahead.stop()
        if uploads is not None:
            uploads.stop()
    if not blocks:
        return torch.empty((0, 6 * order), dtype=torch.float64, device=dev), 0
    X = torch.cat(blocks).contiguous()
    torch.cuda.current_stream(dev).synchronize()      # the fit reads X on its own stream
    return X, frames


def fit_converter(X, components=64, seed=None, max_iter=100, device_index=0, verbose=0, covariance='full'):
    """GMMFeatureConverter._train on the device-resident matrix (this rank's shard).  covariance: 'full' or
    'block_diag' (GaussianMixtureHIP's covariance_structure)."""
    from .converter.gmm_fit import GaussianMixtureHIP
    return GaussianMixtureHIP(n_components=components, max_iter=max_iter, random_state=seed, verbose=verbose,
                              device_index=device_index, covariance_structure=covariance).fit(X)


def _stream_batch(make_pipeline, utterances, pool, shapes_per_stream, keep):
    """Utterance i on stream i % len(pool); a stream keeps the pipelines (buffers) of its `shapes_per_stream` most
    recently used utterance shapes.  A shape seen for the first time just runs kernel by kernel; from its SECOND
    appearance on the stream its pass is a captured HIP graph -- a corpus of files of all different lengths pays
    neither the extra passes of a capture nor the memory of a graph per file.  All pipelines of a stream share the
    stream's context and its scratch arena, which moves when a longer utterance needs more room: a graph captured
    before such a move is discarded and captured again (`_Graphed.graph_valid`) instead of being replayed against
    freed memory.  keep(i, pipeline): called with the pipeline's stream current right after utterance i was enqueued.
    The streams run independently of each other and the host waits once, at the end."""
    from collections import OrderedDict
    cache = [OrderedDict() for _ in range(len(pool))]
    for i, u in enumerate(utterances):
        k = i % len(pool)
        shape = (len(u[0]), len(u[1]))
        p = cache[k].get(shape)
        if p is None:
            while len(cache[k]) >= max(1, shapes_per_stream):
                _, old = cache[k].popitem(last=False)
                old.sync()                  # its buffers go back to the allocator: nothing of it may still be queued
            p = make_pipeline(u, pool.streams[k], pool.contexts[k])
            cache[k][shape] = p
            p.run()
        else:
            cache[k].move_to_end(shape)
            p.load(u)
            if not p.graph_valid():
                p.capture()                 # a plain pass (sizes the arena for this shape), then the capture
            p.replay()
        with torch.cuda.stream(p.stream):
            keep(i, p)
    for s_ in pool.streams:
        s_.synchronize()


@takes_options()
def convert_batch(utterances, fs, gmm, device_index=0, order=24, frame_period=5.0, streams=16, pool=None,
                  shapes_per_stream=4, driver=None, lockstep=None, pcm=False, diff=False, ap_gmm=None, f0_estimator='dio',
                  **options):
    """Convert this rank's utterances with the fitted mixture: list of waveforms (device tensors).
    Lockstep driver only: an utterance may be a bare waveform (its f0 is then extracted on the device), and pcm=True
    returns (waveforms, int16 tensors of the post-processed samples) -- wav in, 16-bit PCM out without the host;
    diff=True appends the differential outputs (the inputs through the MLSA filter of the differential conversion,
    convert_voice.py's .diff.wav): (waveforms, pcm or None, diff waveforms, diff pcm or None).
    driver='lockstep' (default): waves of 16 utterances through the batched entries on two streams (`ConvertWave`);
    'streams': the utterance-per-stream driver, see `_stream_batch` for its scheduling.
    **options: the keywords of `ConvertOptions`, which describes each (lockstep driver; every value is checked before
    anything is put on the device).
    ap_gmm (lockstep driver): the fitted band-aperiodicity mixture (weights_, means_, covariances_ over 6 B dimensions):
    the synthesised outputs are rendered on the converted aperiodicity (`ConvertWave`); None: on the analysed one.
    f0_estimator (lockstep driver): 'dio' or 'pyin', the coarse f0 track of bare waveforms in front of StoneMask
    (kwy_dio_batch_dev / kwy_pyin_batch_dev); with 'pyin' a sample that is not finite is a ValueError after the batch."""
    opts = ConvertOptions(**options).check(order)
    if check_f0_estimator(f0_estimator) != 'dio' and (driver or ('streams' if pool is not None else 'lockstep')) != 'lockstep':
        raise ValueError("convert_batch: f0_estimator='pyin' needs the lockstep driver")
    driver = driver or ('streams' if pool is not None else 'lockstep')     # (a caller's pool asks for the stream driver)
    if driver != 'lockstep' and opts.need_lockstep():
        raise ValueError(f'convert_batch: {opts.need_lockstep()[0]} the lockstep driver')
    if driver != 'lockstep' and ap_gmm is not None:
        raise ValueError('convert_batch: ap_gmm needs the lockstep driver')
    dev = torch.device('cuda', device_index)
    dg = DeviceGMM(gmm.weights_, gmm.means_, gmm.covariances_, dev)
    if ap_gmm is not None:
        from .backend import bap
        bap.check_rate(fs)
        ap_gmm = DeviceGMM(ap_gmm.weights_, ap_gmm.means_, ap_gmm.covariances_, dev)
    out = [None] * len(utterances)
    if driver == 'lockstep':
        pcms, dwav, dpcm = ([None] * len(utterances) for _ in range(3))

        def keep_view(i, w, p, wd, pd):
            out[i], pcms[i], dwav[i], dpcm[i] = w, p, wd, pd      # (views of their wave's blocks, which live as long as the views)
        _lockstep_batch(utterances, fs, device_index, dg, order, frame_period, lockstep, keep_view, opts, pcm=pcm, diff=diff,
                        ap_gmm=ap_gmm, f0_estimator=f0_estimator)
        if diff:
            return out, (pcms if pcm else None), dwav, (dpcm if pcm else None)
        return (out, pcms) if pcm else out
    if pcm or diff or (len(utterances) and not isinstance(utterances[0], (tuple, list))):
        raise ValueError('convert_batch: wav-in utterances and pcm=True need the lockstep driver')
    if pool is None:
        pool = StreamPool(device_index, streams)

    def keep(i, p):
        out[i] = p.wave.clone()
    _stream_batch(lambda u, st, ctx: ConvertPipeline(device_index, fs, u, dg, order=order, frame_period=frame_period,
                                                     stream=st, ctx=ctx), utterances, pool, shapes_per_stream, keep)
    return out


@takes_options(dict(formant_ratio=1.0))
def resynthesize_batch(utterances, fs, device_index=0, frame_period=5.0, streams=16, pool=None, shapes_per_stream=4,
                       out=None, driver=None, lockstep=None, **options):
    """BASELINE config 4 on one rank: analyse + resynthesise every utterance ((x, f0, t) triples: numpy arrays or
    device tensors), more utterances than the driver has in flight.  Returns the list of waveforms (device tensors;
    written into `out[i]` instead when a list of preallocated tensors is given) and the number of frames analysed.
    driver='lockstep' (default): waves of 16 through the batched entries; 'streams': a fixed pool of streams.
    formant_ratio (lockstep driver): a ratio other than 1 warps the analysed envelopes along frequency before the
    synthesis (ConvertWave); ValueError for a row it cannot warp after the batch, for a ratio outside [0.5, 2] before."""
    opts = ConvertOptions(only=dict(formant_ratio=1.0), **options).check(24, converting=False)
    driver = driver or ('streams' if pool is not None else 'lockstep')
    if driver != 'lockstep' and opts.need_lockstep():
        raise ValueError(f'resynthesize_batch: {opts.need_lockstep()[0]} the lockstep driver')
    res = [None] * len(utterances)
    frames = 0
    for u in utterances:
        frames += len(u[1])
    if driver == 'lockstep':
        def keep_view(i, w, *_):
            if out is not None:
                out[i].copy_(w)
                res[i] = out[i]
            else:
                res[i] = w
        _lockstep_batch(utterances, fs, device_index, None, 24, frame_period, lockstep, keep_view, opts)
        return res, frames
    from .pipeline import UtterancePipeline
    if pool is None:
        pool = StreamPool(device_index, streams)

    def keep(i, p):
        if out is not None:
            out[i].copy_(p.wave)
            res[i] = out[i]
        else:
            res[i] = p.wave.clone()
    _stream_batch(lambda u, st, ctx: UtterancePipeline(device_index, fs, u, frame_period=frame_period, stream=st,
                                                       ctx=ctx), utterances, pool, shapes_per_stream, keep)
    return res, frames


_EVALUATED = {name: ConvertOptions.DEFAULTS[name] for name in ('f0_stats', 'transpose_key', 'gv_stats', 'gv_strength',
                                                               'mlpg_em', 'mlpg_gv', 'gv_var', 'gv_weight')}


@takes_options(_EVALUATED)
def evaluate_batch(pairs, fs, gmm, device_index=0, order=24, radius=32, frame_period=5.0, frames='speech', per_frame=False,
                   converter_fs=None, lockstep=None, wave_pairs=16, ap_gmm=None, **options):
    """Objective evaluation of the fitted mixture on parallel pairs, HBM-resident (what
    kwiiyatta_amd.evaluate_voice.evaluate does pair by pair through the Python API): waves of `wave_pairs` pairs
    through `EvalWave`.  pairs: ((x, f0, t), (x, f0, t)) triples as `build_training_matrix` takes them, all at the
    sampling rate `fs` -- which must be the converter's: converter_fs (when given) != fs raises ValueError, such pairs
    go through evaluate_voice.evaluate_pair, which resamples.  The silence pads are drawn from numpy's global
    generator in training's order, so under np.random.seed a pair's alignment is the one training would use.
    frames='speech': the distortion over the aligned frames whose target-side binarised power term is set; 'all': over
    every aligned frame inside both utterances.  **options: gv_stats / gv_strength, f0_stats / transpose_key, mlpg_em,
    mlpg_gv / gv_var / gv_weight of `ConvertOptions`, as in `convert_batch`.  Returns (records, total): a dict per pair and one of the pooled figures -- the triples
    mcd_moments, source_moments, f0_moments ((n, mean, M2); merged by kwy_moments_merge_dev for the total), counts
    (VV, VU, UV, UU), aligned (frames of the alignment) and outside (those beyond either utterance) -- read back once,
    after the last wave.  per_frame=True: a record also holds idx_x, idx_y (frame indices into the trimmed utterances)
    and mcd_frames (per aligned frame, nan where not selected).  A value that is not finite raises ValueError.
    ap_gmm: the fitted band-aperiodicity mixture (fs of 12 kHz or more, ValueError otherwise before anything is read):
    records and total also hold bap_moments and bap_source_moments, the band error of the converted and of the
    unconverted source's band track against the target's over the aligned frames both sides voice."""
    if ap_gmm is not None:
        from .backend import bap
        bap.check_rate(fs)
    if frames not in ('speech', 'all'):
        raise ValueError(f"frames must be 'speech' or 'all', not {frames!r}")
    if converter_fs is not None and int(converter_fs) != int(fs):
        raise ValueError(f'evaluate_batch: the pairs are at {fs} Hz, the converter at {converter_fs} Hz; pairs of another '
                         f'sampling rate go through evaluate_voice.evaluate_pair')
    dev = torch.device('cuda', device_index)
    opts = ConvertOptions(only=_EVALUATED, **options).check(order).upload(dev)
    zero = dict(mcd_moments=(0.0, 0.0, 0.0), source_moments=(0.0, 0.0, 0.0), f0_moments=(0.0, 0.0, 0.0),
                counts=(0, 0, 0, 0), aligned=0, outside=0)
    if not pairs:
        return [], zero
    ls = lockstep if lockstep is not None else _Lockstep(device_index)
    dg = DeviceGMM(gmm.weights_, gmm.means_, gmm.covariances_, dev)
    assert dg.D2 == 6 * order
    wave_pairs = max(1, min(16, int(wave_pairs)))
    K = lib.kwy_cheaptrick_fft_size(int(fs), 71.0) // 2 + 1
    with torch.cuda.stream(ls.main):
        model = dg.model(diff=False)
        tot = _EvalTotals(len(pairs), dev, bands=ap_gmm is not None)
        if ap_gmm is not None:
            ap_gmm = DeviceGMM(ap_gmm.weights_, ap_gmm.means_, ap_gmm.covariances_, dev)
            ap_gmm.model(diff=False)

    def pads(rows):          # the reference's order of draws: source head, source tail, target head, target tail
        for dst in rows:
            dst.copy_(to_device(draw_silence(fs, K), None), non_blocking=True)
    waves = []
    for w0 in range(0, len(pairs), wave_pairs):
        wave = EvalWave(ls, fs, pairs[w0:w0 + wave_pairs], order=order, radius=radius, frame_period=frame_period,
                        bands=ap_gmm is not None)
        wave.analyse()
        wave.measure(pads, dg, model, tot, w0, opts, frames=frames, per_frame=per_frame, ap_gmm=ap_gmm)
        waves.append(wave)
        if not per_frame:
            while len(waves) > 2:
                waves.pop(0)            # (its buffers: all uses are ordered on the main stream before reuse)
    with torch.cuda.stream(ls.main):
        triples, counts, aligned, status = tot.read(ls.ctx)
    ls.sync()
    if status[:, :3].any():
        from .backend import distortion as dist
        dist.check_status(status[:, :3].sum(axis=1), 'evaluation')
    if opts.gv is not None:
        from .backend import gv as gvfilter
        gvfilter.check_status(status[:, 3])
    if opts.gvgen is not None:
        _check_gvgen_status(status[:, 3])
    if opts.f0_map:
        from .backend.f0 import check_status
        check_status(status[:, 4], fs)

    def record(m, c, n_aligned):
        c = tuple(int(v) for v in c)
        band = dict(bap_moments=tuple(m[3].tolist()), bap_source_moments=tuple(m[4].tolist())) if len(m) > 3 else {}
        return dict(mcd_moments=tuple(m[0].tolist()), source_moments=tuple(m[1].tolist()), f0_moments=tuple(m[2].tolist()),
                    counts=c,
                    aligned=int(n_aligned), outside=int(n_aligned) - sum(c), **band)
    records = [record(triples[i], counts[i], aligned[i]) for i in range(len(pairs))]
    if per_frame:
        i = 0
        for wave in waves:
            for k in range(wave.n):
                n = records[i]['aligned']
                records[i].update(idx_x=wave.idx_x[k][:n].cpu().numpy() - PAD_LEN, idx_y=wave.idx_y[k][:n].cpu().numpy() - PAD_LEN,
                                  mcd_frames=wave.mcd_frames[k][:n].cpu().numpy())
                i += 1
    return records, record(triples[-1], counts.sum(axis=0), aligned.sum())
