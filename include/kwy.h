/*
 * include/kwy.h -- C ABI of libkwy.so, the MI355X (gfx950) implementation of
 * kwiiyatta's per-utterance conversion hot path.
 *
 * The reference (Iselix/kwiiyatta) has no native code: its replaceable seam is
 * the set of third-party calls it makes.  Every entry
 * point below replaces one of those calls; the comment on each names the
 * reference call site.  Conventions:
 *
 *   - all arrays are float64, C-contiguous, caller-allocated; the library never
 *     retains or frees a caller pointer
 *   - `kwy_<op>`      takes HOST pointers (what a ctypes/numpy binding passes);
 *                     it stages through HBM, runs the HIP kernels and copies
 *                     the result back (synchronous on return).  Every such entry
 *                     can return KWY_ENOMEM with "<op>: scratch arena too small"
 *                     (a staged buffer did not fit the arena the call had sized)
 *   - `kwy_<op>_dev`  takes DEVICE pointers; work is enqueued on the context's
 *                     HIP stream and NOT synchronised (call kwy_ctx_sync)
 *   - return value: 0 on success, a negative KWY_E* code otherwise;
 *     kwy_last_error(ctx) gives a message.  No C++ exception crosses the ABI.
 *   - a kwy_ctx owns one HIP stream plus its device scratch; calls on one
 *     context are serialised, different contexts run concurrently
 *     (one context per utterance stream / per Python thread).
 *   - There is NO CPU fallback: without a HIP device kwy_ctx_create fails.
 */
#ifndef KWY_H_
#define KWY_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KWY_OK 0
#define KWY_EINVAL (-1)   /* bad argument                               -> ValueError   */
#define KWY_EHIP (-2)     /* HIP runtime / launch failure               -> RuntimeError */
#define KWY_ENOMEM (-3)   /* device allocation failed                   -> MemoryError  */
#define KWY_ENODEV (-4)   /* no usable HIP device                       -> RuntimeError */
#define KWY_ENUMERIC (-5) /* numerical failure (e.g. covariance not PD) -> ValueError   */

typedef struct kwy_ctx kwy_ctx;

/* ---- context --------------------------------------------------------------- */
int kwy_version(void);
/* device: HIP device ordinal.  stream: an existing hipStream_t to enqueue on
 * (e.g. torch's current stream), or NULL to let the context create its own. */
int kwy_ctx_create(int device, void *stream, kwy_ctx **out);
void kwy_ctx_destroy(kwy_ctx *ctx);
int kwy_ctx_sync(kwy_ctx *ctx);
void *kwy_ctx_stream(kwy_ctx *ctx);
/* The context's scratch arena grows on demand, and growing RELOCATES it (the stream is synchronised first).  A HIP
 * graph captured from calls on this context holds arena addresses: it is valid only while
 * kwy_ctx_arena_generation() returns the value it had at capture time.  kwy_ctx_reserve() grows the arena to at
 * least `bytes` ahead of time (e.g. for the longest utterance of a batch) so that later calls do not move it. */
int64_t kwy_ctx_arena_generation(kwy_ctx *ctx);
int kwy_ctx_reserve(kwy_ctx *ctx, int64_t bytes);
/* dst[0 .. bytes) <- src[0 .. bytes), device to device, as a KERNEL on the context's stream (bytes a multiple of 8;
 * the buffers must not overlap).  For drivers that move a step's inputs and results between staging blocks and the
 * buffers a captured graph reads (Wavdata -> Analyzer's copy, kwiiyatta/vocoder/world.py:14-17): a copy-engine
 * transfer per stream and direction does not scale over many streams here, a kernel does. */
int kwy_copy_dev(kwy_ctx *ctx, void *dst, const void *src, int64_t bytes);
/* WORLD's analysis / synthesis noise is ONE fixed pseudo-random sequence (the generator is reseeded at the entry of
 * every pyworld call); the library keeps its first 2^KWY_RANDN_LOG2 draws (environment, default 25 = 128 MB, 0 = none)
 * in a table per device and computes draws beyond it by jump-ahead -- the same numbers either way.  This call lowers
 * the number of table draws THIS context uses (draws < 0: all of them); returns the length now in use.  For tests of
 * the jump-ahead path. */
int64_t kwy_ctx_set_randn_limit(kwy_ctx *ctx, int64_t draws);
/* draws [first, first + count) of that sequence as WORLD's randn() returns them (host array), read from the table */
int kwy_randn_stream(kwy_ctx *ctx, int64_t first, int64_t count, double *out);
/* Per-kernel timing: when enabled, the main kernels are bracketed by HIP events
 * on the context's stream.  kwy_ctx_profile_read synchronises the stream and
 * returns the summed duration [ms] and launch count of `kernel` since the last
 * read (kernel names as in rocprofv3, without template arguments, e.g.
 * "k_d4c_body"). */
int kwy_ctx_profile(kwy_ctx *ctx, int enable);
int kwy_ctx_profile_read(kwy_ctx *ctx, const char *kernel, double *total_ms, int64_t *count);
const char *kwy_last_error(kwy_ctx *ctx);
/* error text when kwy_ctx_create itself failed (no context to ask) */
const char *kwy_create_error(void);

/* ---- sizes (pure host arithmetic, no device needed) -------------------------- */
/* pyworld.get_cheaptrick_fft_size(fs, f0_floor)      kwiiyatta/vocoder/world.py:96 */
int kwy_cheaptrick_fft_size(int fs, double f0_floor);
/* number of frames pyworld.dio returns               kwiiyatta/vocoder/world.py:35 */
int64_t kwy_dio_frames(int fs, int64_t x_length, double frame_period_ms);
/* output length of pyworld.synthesize                kwiiyatta/vocoder/world.py:86 */
int64_t kwy_synth_length(int64_t f0_length, double frame_period_ms, int fs);

/* ---- WORLD analysis ----------------------------------------------------------- */
/* pyworld.cheaptrick(x, f0, t, fs, q1, f0_floor, fft_size)
 *                                                    kwiiyatta/vocoder/world.py:45
 * fft_size <= 0: derive from (fs, f0_floor).  out: T x (fft_size/2+1).
 * out_div: the result is divided by this value (pass fs to fold the
 * `spectrum_envelope /= fs` of world.py:50 into the kernel; 1.0 = pyworld). */
int kwy_cheaptrick(kwy_ctx *ctx, const double *x, int64_t x_length, int fs,
                   const double *temporal_positions, const double *f0, int64_t f0_length,
                   double q1, double f0_floor, int fft_size, double out_div, double *out);
int kwy_cheaptrick_dev(kwy_ctx *ctx, const double *x, int64_t x_length, int fs,
                       const double *temporal_positions, const double *f0, int64_t f0_length,
                       double q1, double f0_floor, int fft_size, double out_div, double *out);

/* The same call for a batch of utterances of one sampling rate (device pointers), one grid over all their frames:
 * what Analyzer.extract_spectrum_envelope does file after file (kwiiyatta/vocoder/world.py:43-52) for both sides of a
 * pair, or for every file of a corpus.  A lone utterance's ~2 000 workgroups are 2.2 rounds of what the chip holds. */
typedef struct kwy_utterance {
  const double *x;                   /* waveform, x_length samples */
  int64_t x_length;
  const double *temporal_positions;  /* f0_length frame times [s] */
  const double *f0;                  /* f0_length */
  int64_t f0_length;
  double *out;                       /* f0_length x (fft_size/2+1) */
} kwy_utterance;
int kwy_cheaptrick_batch_dev(kwy_ctx *ctx, const kwy_utterance *utterances, int count, int fs, double q1,
                             double f0_floor, int fft_size, double out_div);
/* CheapTrick and sp2mc in one, for consumers that only need the mel-cepstrum (the alignment, the conversion):
 *   Analyzer.extract_spectrum_envelope + MelCepstrum of it        kwiiyatta/vocoder/world.py:43-52, mcep.py:68-71
 * CheapTrick's last steps are: lifter the cepstrum, transform back, exp; sp2mc's first: log, transform to the
 * cepstrum.  The fused form keeps the liftered cepstrum and applies pysptk's frequency transform to it directly (an
 * f64 matrix product): no K-bin envelope row is written or read.  utterances[i].out: f0_length x (order + 1)
 * mel-cepstral coefficients, equal to kwy_sp2mc_dev(kwy_cheaptrick_dev(...)) up to the rounding of the skipped
 * exp / log round trip (1e-12 relative in the tests).  order <= 63. */
int kwy_cheaptrick_mcep_batch_dev(kwy_ctx *ctx, const kwy_utterance *utterances, int count, int fs, double q1,
                                  double f0_floor, int fft_size, double out_div, int order, double alpha);

/* pyworld.d4c(x, f0, t, fs, threshold, fft_size)     kwiiyatta/vocoder/world.py:55
 * out: T x (fft_size/2+1). */
int kwy_d4c(kwy_ctx *ctx, const double *x, int64_t x_length, int fs,
            const double *temporal_positions, const double *f0, int64_t f0_length,
            double threshold, int fft_size, double *out);
int kwy_d4c_dev(kwy_ctx *ctx, const double *x, int64_t x_length, int fs,
                const double *temporal_positions, const double *f0, int64_t f0_length,
                double threshold, int fft_size, double *out);
/* ... for a batch of utterances (see kwy_cheaptrick_batch_dev) */
int kwy_d4c_batch_dev(kwy_ctx *ctx, const kwy_utterance *utterances, int count, int fs, double threshold,
                      int fft_size);

/* pyworld.dio(x, fs, f0_floor, f0_ceil, channels_in_octave, frame_period, speed,
 *             allowed_range) -> (f0, t)              kwiiyatta/vocoder/world.py:35
 * only speed == 1 (pyworld's default, the only value kwiiyatta uses). */
int kwy_dio(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor,
            double f0_ceil, double channels_in_octave, double frame_period_ms, int speed,
            double allowed_range, double *temporal_positions, double *f0);
/* pyworld.stonemask(x, f0, t, fs)                    kwiiyatta/vocoder/world.py:39 */
int kwy_stonemask(kwy_ctx *ctx, const double *x, int64_t x_length, int fs,
                  const double *temporal_positions, const double *f0, int64_t f0_length,
                  double *refined_f0);
/* The f0 track without the host (round 5): what Analyzer.extract_f0 does in front of every analysis,
 * kwiiyatta/vocoder/world.py:33-41, on DEVICE pointers, enqueued on the context's stream and not synchronised; the
 * batch forms take the utterances of a wave in one pass of launches (DIO <= 32 per pass: the two sides of a wave of 16
 * pairs share the single-wavefront contour repair; StoneMask <= 16), as kwy_cheaptrick_batch_dev does.  Every job's result equals the host entry's bit for bit (the host entries run the same pass on staged copies).
 * status (one int32 on the device per utterance, or NULL): cleared by the call, set to 1 when an engine's
 * zero-crossing buffer overflowed (kwy_dio reports that as KWY_EHIP); a driver reads the words back once per wave. */
typedef struct kwy_f0_job {
  const double *x;               /* waveform, x_length samples */
  int64_t x_length;
  double *temporal_positions;    /* kwy_dio_frames(fs, x_length, frame_period_ms) frame times [s], written */
  double *f0;                    /* as many f0 values, written */
  int32_t *status;               /* see above; may be NULL */
} kwy_f0_job;
int kwy_dio_dev(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor, double f0_ceil,
                double channels_in_octave, double frame_period_ms, int speed, double allowed_range,
                double *temporal_positions, double *f0, int32_t *status);
int kwy_dio_batch_dev(kwy_ctx *ctx, const kwy_f0_job *jobs, int count, int fs, double f0_floor, double f0_ceil,
                      double channels_in_octave, double frame_period_ms, int speed, double allowed_range);
int kwy_stonemask_dev(kwy_ctx *ctx, const double *x, int64_t x_length, int fs,
                      const double *temporal_positions, const double *f0, int64_t f0_length,
                      double *refined_f0);
/* utterances[i].out: the refined f0 (f0_length values); .f0: the initial track */
int kwy_stonemask_batch_dev(kwy_ctx *ctx, const kwy_utterance *utterances, int count, int fs);

/* ---- probabilistic YIN: the second f0 estimator (Mauch & Dixon 2014) --------------------------------------
 * A coarse f0 track on DIO's frame grid (kwy_dio_frames frames, t_i = i frame_period), refined by StoneMask like
 * DIO's.  Voicing and pitch are decided jointly by a Viterbi pass over the utterance.  The reference has no
 * counterpart.  Parameters (the defaults of the Python front-end): f0_floor 71, f0_ceil 800, p_a 0.01, switch
 * probability 0.01, maximal pitch rate 35.92 octaves / s; KWY_PYIN_BINS_PER_OCTAVE pitch bins an octave (10 cents).
 *   tau_min = floor(fs / f0_ceil), tau_max = ceil(fs / f0_floor), W = tau_max + 1
 *   nb = kwy_pyin_bins     = ceil(120 log2(f0_ceil / f0_floor))                      (420 at the defaults)
 *   R  = kwy_pyin_radius   = ceil(max_rate 120 frame_period / 1000)                  (22 at 5 ms)
 *   N  = kwy_pyin_fft_size = the smallest power of two >= 2 W and >= 1024            (1024 at 16 kHz, 2048 at 48 kHz)
 * 1 frame        c = floor(t_i fs + 0.5); the frame is x[c - W .. c + W), zeros outside the signal.
 * 2 difference   d(tau) = sum_{j < W} (x_j - x_{j + tau})^2 for tau <= tau_max + 1, formed as e(0) + e(tau) - 2 r(tau):
 *                r the correlation of the first W samples with the whole frame (two real transforms of length N, a
 *                product, one inverse), e the sliding energy from a prefix sum.  A value below
 *                2^-40 (e(0) + e(tau)) counts as 0: a constant or silent frame has no candidates.
 * 3 normalise    d'(0) = 1; d'(tau) = d(tau) tau / sum_{j = 1 .. tau} d(j), and 1 where that sum is 0.
 * 4 candidates   every tau in [max(tau_min, 1), tau_max] with d'(tau) < d'(tau - 1) and d'(tau) <= d'(tau + 1); with
 *                a = d'(tau - 1), b = d'(tau), c = d'(tau + 1) and a - 2 b + c > 0 the parabola gives the offset
 *                (a - c) / (2 (a - 2 b + c)) and the trough value v = max(b - (a - c) offset / 4, 0); else 0 and b.
 * 5 prior        Beta(2, 18) over a CONTINUOUS threshold, F(v) = 1 - (1 - v)^18 (1 + 18 v) on [0, 1] (no probability
 *                jumps with a rounding error of v; the paper has 100 discrete thresholds).  The candidates are walked
 *                in ascending tau with a running minimum m = 1: one with v < m receives F(m) - F(v) and sets m = v;
 *                the last one that set m also receives p_a F(m).
 * 6 observation  a candidate of frequency f = fs / (tau + offset) falls into bin floor(120 log2(f / f0_floor));
 *                outside [0, nb) it is dropped.  p_b: the masses of bin b, added in ascending tau.  The stage writes
 *                L (T x (nb + 1) doubles): L[t][b] = log max(p_b, 1e-300), L[t][nb] = log max((1 - sum p_b) / nb,
 *                1e-300), the value of every unvoiced state.
 * 7 decoding     2 nb states (voiced bin b, unvoiced bin b), uniform start.  A step from bin s to bin s + k, |k| <= R,
 *                weighs (R + 1 - |k|) / (R + 1)^2 (NOT renormalised at the ends of the bin range), times 1 - switch
 *                where the voicing stays and times switch where it changes.  trans: the 2 (2 R + 1) logarithms of
 *                those, [kept | changed][k + R], formed on the host; the device adds and compares only
 *                (delta' = max(delta + trans) + L, nothing contracted).  Of equal predecessors the one of the same
 *                voicing wins, within each voicing the lowest bin; at the end the lowest state.  freq[b]: the track's
 *                value for voiced bin b, f0_floor 2^((b + 1/2) / 120); an unvoiced state gives 0.
 * 8 status       a non-finite sample sets the utterance's status word (cleared by the call otherwise) and makes its
 *                track all zero; the entries on host pointers return KWY_EINVAL.  No other utterance of a batch is
 *                touched by it.
 * KWY_EINVAL, nothing written: N > 4096 (the frame no longer fits one workgroup's transform: 96 kHz is the highest
 * rate at f0_floor 71), 2 nb > 1024 (one thread per state), R > 8191, p_a outside [0, 1], switch outside (0, 1), and
 * what kwy_dio refuses.
 * Scratch: L and the 16-bit back-pointers (T x 2 nb) live in the context's arena; the _dev entries do not allocate
 * once it holds kwy_pyin_scratch_bytes(frames of the longest utterance, nb, count) bytes (kwy_ctx_reserve), and all
 * launches of a call are enqueued without a host round trip.  The batch form takes <= 32 utterances per pass of
 * launches and is a drop-in for kwy_dio_batch_dev; every job's result equals the single entries' bit for bit. */
#define KWY_PYIN_BINS_PER_OCTAVE 120
/* pure host arithmetic, no device needed; 0 (kwy_pyin_radius: -1) for an argument out of range */
int kwy_pyin_fft_size(int fs, double f0_floor);
int kwy_pyin_bins(double f0_floor, double f0_ceil);
int kwy_pyin_radius(double frame_period_ms, double max_rate);
size_t kwy_pyin_scratch_bytes(int64_t frames, int nb, int count);
int kwy_pyin(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor, double f0_ceil,
             double frame_period_ms, double p_a, double switch_prob, double max_rate, double *temporal_positions,
             double *f0);
int kwy_pyin_dev(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor, double f0_ceil,
                 double frame_period_ms, double p_a, double switch_prob, double max_rate, double *temporal_positions,
                 double *f0, int32_t *status);
int kwy_pyin_batch_dev(kwy_ctx *ctx, const kwy_f0_job *jobs, int count, int fs, double f0_floor, double f0_ceil,
                       double frame_period_ms, double p_a, double switch_prob, double max_rate);
/* steps 1 - 6 alone: L, kwy_dio_frames(...) x (kwy_pyin_bins(...) + 1).  status (may be NULL): set for a non-finite
 * sample that one of the FRAMES reads (it counts as 0 there); unlike the whole estimator, which looks through the whole
 * waveform in front of the decoding, this entry does not see a sample between the frames of a window narrower than
 * the frame period (2 W < frame_period fs / 1000: an f0_floor above 400 Hz at 5 ms). */
int kwy_pyin_observe(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor, double f0_ceil,
                     double frame_period_ms, double p_a, double *L);
int kwy_pyin_observe_dev(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor, double f0_ceil,
                         double frame_period_ms, double p_a, double *L, int32_t *status);
/* step 7 alone on the caller's L (T x (nb + 1)), trans (2 (2 R + 1)) and freq (nb): f0, T values */
int kwy_pyin_decode(kwy_ctx *ctx, const double *L, int64_t T, int nb, const double *trans, int R, const double *freq,
                    double *f0);
int kwy_pyin_decode_dev(kwy_ctx *ctx, const double *L, int64_t T, int nb, const double *trans, int R,
                        const double *freq, double *f0);

/* ---- WORLD synthesis ------------------------------------------------------------ */
/* pyworld.synthesize(f0, sp, ap, fs, frame_period)   kwiiyatta/vocoder/world.py:86-92
 * sp_mul: every spectrogram value is multiplied by this before use (pass fs to
 * fold `spectrum_envelope * fs` of world.py:88; 1.0 = pyworld).
 * y: kwy_synth_length(...) samples. */
int kwy_synthesize(kwy_ctx *ctx, const double *f0, int64_t f0_length, const double *sp,
                   const double *ap, int fft_size, double frame_period_ms, int fs,
                   double sp_mul, int64_t y_length, double *y);
int kwy_synthesize_dev(kwy_ctx *ctx, const double *f0, int64_t f0_length, const double *sp,
                       const double *ap, int fft_size, double frame_period_ms, int fs,
                       double sp_mul, int64_t y_length, double *y);
/* The same call in two steps, for pipelines: the pulse placement depends on f0 alone (WORLD's phase accumulation and
 * zero-crossing search, synthesis.cpp GetTimeBase [RECALL]), so it can run on another context / stream while the
 * spectral features are still being computed.  plan: kwy_synth_plan_bytes(y_length) bytes of device memory, written
 * by kwy_synth_plan_dev and read by kwy_synth_render_dev (same f0-derived arguments in both calls). */
int64_t kwy_synth_plan_bytes(int64_t y_length);
int kwy_synth_plan_dev(kwy_ctx *ctx, const double *f0, int64_t f0_length, int fft_size, double frame_period_ms,
                       int fs, int64_t y_length, void *plan);
int kwy_synth_render_dev(kwy_ctx *ctx, const void *plan, int64_t f0_length, const double *sp, const double *ap,
                         int fft_size, double frame_period_ms, int fs, double sp_mul, int64_t y_length, double *y);
/* The pulse placement of several utterances in one pass of launches: the serial phase chain of an utterance is one
 * workgroup, so N utterances occupy N compute units side by side (Synthesizer.synthesize runs file after file,
 * kwiiyatta/vocoder/world.py:80-92).  Every plan equals kwy_synth_plan_dev's bit for bit. */
typedef struct kwy_synth_plan_job {
  const double *f0;      /* f0_length */
  int64_t f0_length;
  int64_t y_length;
  void *plan;            /* kwy_synth_plan_bytes(y_length) bytes */
} kwy_synth_plan_job;
int kwy_synth_plan_batch_dev(kwy_ctx *ctx, const kwy_synth_plan_job *jobs, int count, int fft_size,
                             double frame_period_ms, int fs);
/* ... for a batch of utterances: a pass of launches renders the pulses of up to KWY_BATCH_MAX = 16 of them (dealt to
 * the workgroups from one queue; the passes of a call share one pool of response slots, 116 MB per 10 s utterance at
 * 48 kHz), as kwy_cheaptrick_batch_dev / kwy_d4c_batch_dev analyse them.  What Synthesizer.synthesize does file
 * after file (kwiiyatta/vocoder/world.py:63-80, resynthesize_voice.py:46-79).  Every job's waveform equals
 * kwy_synth_render_dev's bit for bit.
 * ap_rows (optional): the aperiodicity through a row index, as an alignment leaves it.  `aperiodicity` is then a
 * matrix of ap_src_rows rows and frame t reads its row clamp(ap_rows[t], 0, ap_src_rows - 1) -- kwy_gather_rows_dev's
 * clamp, so the waveform equals, bit for bit, the one rendered from the rows gathered beforehand, without the copy.
 * NULL: row t is row t (ap_src_rows is ignored). */
typedef struct kwy_synth_job {
  const void *plan;             /* kwy_synth_plan_dev's output for this utterance */
  const double *spectrogram;    /* f0_length x (fft_size/2+1) */
  const double *aperiodicity;   /* f0_length (with ap_rows: ap_src_rows) x (fft_size/2+1) */
  int64_t f0_length;
  int64_t y_length;
  double *y;                    /* y_length samples */
  const int32_t *ap_rows;       /* f0_length row numbers into `aperiodicity`, or NULL */
  int64_t ap_src_rows;          /* rows of `aperiodicity` when ap_rows is set (> 0) */
} kwy_synth_job;
int kwy_synth_render_batch_dev(kwy_ctx *ctx, const kwy_synth_job *jobs, int count, int fft_size,
                               double frame_period_ms, int fs, double sp_mul);

/* The post-step of a synthesised waveform and its 16-bit PCM, for a batch of waveforms in device memory:
 *   Synthesizer.synthesize(normalize=True): wavdata.normalize(None); normalize_data() on the first `frame_len`
 *     1 ms pieces                                     kwiiyatta/vocoder/abc/synthesizer.py:11-20
 *   Wavdata.save(normalize=True): data -= mean; normalize_data(data, peak_lv); (data * 2**15).astype(np.int16)
 *                                                     kwiiyatta/wavfile.py:8-29
 * normalize_synth / normalize_save: the two `normalize` flags; piece_ceiling / save_ceiling: 10 ** (peak_lv / 10) of
 * the two calls (save_ceiling NaN: peak_lv=None, mean removal only).  The samples equal the host path's exactly
 * (numpy's chunked pairwise mean is reproduced).  y is not modified; a wave downloads 2 bytes per sample.  Enqueued on
 * the context's stream, not synchronised.  KWY_EINVAL where the reference's loop would fail (a piece beyond the end). */
typedef struct kwy_finish_job {
  const double *y;      /* y_length samples (kwy_synthesize's output) */
  int64_t y_length;
  int64_t frame_len;    /* frames of the feature the waveform was rendered from */
  int16_t *pcm;         /* y_length samples, written */
} kwy_finish_job;
int kwy_finish_pcm16_batch_dev(kwy_ctx *ctx, const kwy_finish_job *jobs, int count, int fs, int normalize_synth,
                               double piece_ceiling, int normalize_save, double save_ceiling);
/* bytes of the context's scratch arena one waveform of that length needs in the call above (kwy_ctx_reserve) */
int64_t kwy_finish_scratch_bytes(int64_t y_length);

/* ---- f0 conversion ---------------------------------------------------------------- */
/* The reference synthesises a converted voice on the source's own f0 track (kwiiyatta/convert_voice.py:35-46); its
 * dialog transposes the key with feature.f0 = feature.f0 * (2.0 ** (transposeKey / 12))
 * (kwiiyatta/view/qt/kwiieiya.py:152-155).  These entries add the log-Gaussian normalised f0 transform
 *   log f0' = (log f0 - mu_src) * sigma_tgt / sigma_src + mu_tgt            on voiced frames (f0 > 0)
 * and the key ratio on top of it.  Moments are (n, mean, M2) of log f0 over the voiced frames of a track, M2 the
 * sum of squared deviations from the mean; an all-unvoiced track gives (0, 0, 0).  Every reduction has a fixed order:
 * a track's triple does not depend on the run nor on the other tracks of the call.  The _dev forms allocate nothing
 * and do not synchronise (legal inside a stream capture); the host forms stage through HBM and synchronise. */
typedef struct kwy_f0_track {
  const double *f0;     /* length values */
  int64_t length;
} kwy_f0_track;
/* moments: count x 3 doubles, written */
int kwy_logf0_moments(kwy_ctx *ctx, const kwy_f0_track *tracks, int count, double *moments);
int kwy_logf0_moments_batch_dev(kwy_ctx *ctx, const kwy_f0_track *tracks, int count, double *moments);
/* count triples -> one (Chan's pairwise combination, a left fold in index order): the statistics of a corpus,
 * bit-equal however its tracks were grouped into calls */
int kwy_logf0_moments_merge(kwy_ctx *ctx, const double *moments, int count, double *out);
int kwy_logf0_moments_merge_dev(kwy_ctx *ctx, const double *moments, int count, double *out);
/* f0_out[i] = exp((log f0 - stats[0]) * stats[3] / stats[1] + stats[2]) * ratio on voiced frames, 0 stays 0.
 * stats: (mu_src, sigma_src, mu_tgt, sigma_tgt) -- device memory in the _dev form -- or NULL: f0 * ratio on every
 * frame (the dialog's product, bit for bit).  ratio = 2 ** (key / 12), formed by the caller.  f0_out may equal f0_in.
 * status: count int32 (or NULL), each set to the number of the track's frames whose input is negative or not finite
 * or whose output is >= fs / 8: the synthesis plan holds y_length / 8 + 16 pulses (kwy_synth_plan_bytes), which a
 * track below fs / 8 always fits. */
typedef struct kwy_f0_map_job {
  const double *f0_in;  /* length values */
  int64_t length;
  double *f0_out;       /* length values, written */
} kwy_f0_map_job;
int kwy_f0_map(kwy_ctx *ctx, const kwy_f0_map_job *jobs, int count, int fs, const double *stats, double ratio,
               int32_t *status);
int kwy_f0_map_batch_dev(kwy_ctx *ctx, const kwy_f0_map_job *jobs, int count, int fs, const double *stats,
                         double ratio, int32_t *status);

/* ---- global variance ---------------------------------------------------------------- */
/* The reference has no counterpart (kwiiyatta/convert_voice.py:35-46 synthesises the converter's output as it is):
 * these entries add the global-variance postfilter of Toda et al. (2007) for the over-smoothed trajectories of a
 * GMM / MLPG conversion.  For a row-major (rows, cols) matrix x, per column d >= first_col
 *   m_d = mean of x[:, d],   v_d = M2_d / rows (variance, ddof 0),   r_d = sqrt(gv_d / v_d)
 *   out[t, d] = base[t, d] + strength * (r_d - 1) * (x[t, d] - m_d)
 * evaluated operation by operation as written; columns below first_col are copied from base.  base == x is the plain
 * filter (variance gv_d at strength 1), base == the differential conversion the differential one.  A column with
 * v_d == 0 (a constant column, rows <= 1) or strength * (r_d - 1) == 0 is copied from base; so is a column whose v_d
 * is not finite or whose gv_d is not finite or <= 0, and those are counted in the matrix's status word.
 * Column moments are (n, mean, M2) per column, cols x 3 doubles per matrix: n = rows, M2 the sum of squared deviations
 * from the mean, in two passes; a column whose values all equal its first one has that value as its mean and M2 == 0
 * exactly.  Every reduction has a fixed order: a matrix's moments depend on the matrix alone, not on the run nor on
 * the other matrices of the call.  cols <= 64.  The _dev forms allocate nothing and do not synchronise (legal inside
 * a stream capture); the host forms stage through HBM and synchronise. */
typedef struct kwy_gv_matrix {
  const double *x;      /* rows x cols values */
  int64_t rows;
} kwy_gv_matrix;
/* moments: count x cols x 3 doubles, written */
int kwy_column_moments(kwy_ctx *ctx, const kwy_gv_matrix *mats, int count, int cols, double *moments);
int kwy_column_moments_dev(kwy_ctx *ctx, const double *x, int64_t rows, int cols, double *moments);
int kwy_column_moments_batch_dev(kwy_ctx *ctx, const kwy_gv_matrix *mats, int count, int cols, double *moments);
/* gv[d] = the mean over the matrices with n > 0 of M2 / n (a left fold in index order, then one division): the
 * statistic of a corpus, bit-equal however its matrices were grouped into calls; 0 when no matrix has rows.
 * moments: count x cols x 3; gv: cols doubles, written */
int kwy_gv_from_moments(kwy_ctx *ctx, const double *moments, int count, int cols, double *gv);
int kwy_gv_from_moments_dev(kwy_ctx *ctx, const double *moments, int count, int cols, double *gv);
typedef struct kwy_gv_job {
  const double *x;        /* rows x cols: the matrix the moments were taken from */
  int64_t rows;
  const double *moments;  /* cols x 3, of x (the host form computes them itself and ignores this field) */
  const double *base;     /* rows x cols (may equal x) */
  double *out;            /* rows x cols, written (may equal base) */
} kwy_gv_job;
/* gv: cols doubles -- device memory in the _dev forms; strength in [0, 1]; status: one int32 per matrix (or NULL),
 * set to the number of columns >= first_col that were copied because v_d or gv_d is unusable */
int kwy_gv_postfilter(kwy_ctx *ctx, const kwy_gv_job *jobs, int count, int cols, int first_col, const double *gv,
                      double strength, int32_t *status);
int kwy_gv_postfilter_dev(kwy_ctx *ctx, const double *x, int64_t rows, int cols, int first_col, const double *moments,
                          const double *gv, double strength, const double *base, double *out, int32_t *status);
int kwy_gv_postfilter_batch_dev(kwy_ctx *ctx, const kwy_gv_job *jobs, int count, int cols, int first_col,
                                const double *gv, double strength, int32_t *status);

/* ---- modulation spectrum -------------------------------------------------------------- */
/* The reference has no counterpart.  These entries add the utterance-level modulation-spectrum postfilter of Takamichi
 * et al. (2016): the global-variance filter above fixes one number per trajectory, this one every modulation-frequency
 * bin of it.  For column d of a row-major (T, cols) matrix x and a transform length L in {512, 1024, 2048, 4096, 8192},
 * T <= L (KWY_EINVAL otherwise, nothing is written):
 *   m = mean of x[:, d] (as kwy_column_moments defines it),  z[t] = x[t, d] - m for t < T, 0 for T <= t < L
 *   Z = the real transform of z, bins f = 0 .. L/2,   s[f] = log(max(|Z[f]|^2, DBL_MIN) / T)
 * s is the log modulation spectrum.  Statistics are (n, mean, M2) per (column, bin), cols x (L/2 + 1) x 3 doubles,
 * sigma = sqrt(M2 / n); bin 0 carries none (after the mean removal it holds rounding noise) and stays (0, 0, 0).
 * The filter at strength k in [0, 1], with the statistics G of converted and N of natural speech, for f >= 1:
 *   s'[f] = (1 - k) s[f] + k (sigmaN[f] / sigmaG[f] (s[f] - muG[f]) + muN[f]),   g[f] = exp((s'[f] - s[f]) / 2),  g[0] = 1
 *   out[t, d] = base[t, d] + (z'[t] - z[t]),   z' = the inverse transform of g Z, t < T
 * base == x is the plain filter, base == the differential conversion the differential one.  A bin whose statistics
 * are unusable (nG < 2, nN < 2, a mean that is not finite, sigmaG not finite or <= 0, sigmaN not finite or < 0) or
 * whose gain is not finite keeps g = 1 and is counted in the matrix's status word.  Columns below first_col, columns
 * with T < 2 or M2 == 0, and everything at k == 0 are copied from base bit for bit.
 * Every reduction has a fixed order: a matrix's result depends on the matrix, the statistics and the shape alone.
 * cols <= 64.  The _dev forms allocate nothing and do not synchronise once the context holds the tables of the
 * length (its first call makes them); the host forms stage through HBM and synchronise. */
/* spectra: count x cols x (L/2 + 1) doubles, written; valid: count x cols int32, written: 1, or 0 for a column with
 * T < 2 or M2 == 0, whose row of spectra is then zero */
int kwy_ms_logspectra(kwy_ctx *ctx, const kwy_gv_matrix *mats, int count, int cols, int L, double *spectra,
                      int32_t *valid);
int kwy_ms_logspectra_batch_dev(kwy_ctx *ctx, const kwy_gv_matrix *mats, int count, int cols, int L, double *spectra,
                                int32_t *valid);
/* acc: cols x (L/2 + 1) x 3, updated in place by Welford's step over the count matrices in index order, the invalid
 * columns skipped: bit-equal however a corpus was grouped into calls.  A new accumulator is all zero. */
int kwy_ms_stats_update(kwy_ctx *ctx, double *acc, const double *spectra, const int32_t *valid, int count, int cols,
                        int L);
int kwy_ms_stats_update_dev(kwy_ctx *ctx, double *acc, const double *spectra, const int32_t *valid, int count, int cols,
                            int L);
typedef struct kwy_ms_job {
  const double *x;        /* rows x cols: the matrix whose modulation spectrum is modified */
  int64_t rows;
  const double *base;     /* rows x cols (may equal x) */
  double *out;            /* rows x cols, written (may equal base or x) */
} kwy_ms_job;
/* statsG, statsN: cols x (L/2 + 1) x 3 -- device memory in the _dev forms; status: one int32 per matrix (or NULL),
 * set to the number of bins that kept g = 1 because their statistics or their gain are unusable */
int kwy_ms_postfilter(kwy_ctx *ctx, const kwy_ms_job *jobs, int count, int cols, int first_col, int L,
                      const double *statsG, const double *statsN, double strength, int32_t *status);
int kwy_ms_postfilter_dev(kwy_ctx *ctx, const double *x, int64_t rows, int cols, int first_col, int L,
                          const double *statsG, const double *statsN, double strength, const double *base, double *out,
                          int32_t *status);
int kwy_ms_postfilter_batch_dev(kwy_ctx *ctx, const kwy_ms_job *jobs, int count, int cols, int first_col, int L,
                                const double *statsG, const double *statsN, double strength, int32_t *status);

/* ---- waveform pitch shift -------------------------------------------------------------- */
/* The reference has no counterpart: its differential output (kwiiyatta/convert_voice.py:19,39-40) keeps the source's
 * pitch.  These entries add the waveform pitch shifter GMM voice-conversion recipes run on the source recordings: a
 * WSOLA time stretch by `rate` followed by resampling back to the input's length, which multiplies every frequency by
 * `rate`.  x: n samples, xb: x extended with zeros on both sides; rate within [0.5, 2.0]; int64 index arithmetic.
 *   constants   H = (int)(fs * 0.010), L = 2 H, S = H;  M = floor(n * rate + 0.5);  K = ceil(M / H) frames (0 for M = 0)
 *   positions   p_0 = 0;  for k = 1 .. K-1:  a_k = (k H n + M / 2) / M  (integer divisions),
 *               candidates q in [lo, hi], lo = min(max(a_k - S, 0), n - 1), hi = min(a_k + S, n - 1),
 *               template t[i] = xb[p_{k-1} + H + i], i < L;  d(q) = sum_{i < L} (xb[q + i] - t[i])^2 (any order);
 *               p_k = the q of the smallest d, ties to the smallest |q - a_k|, then to the smaller q
 *   stretch     for m < M, k = m / H, i = m % H:  s[m] = xb[i] for k = 0, otherwise a + w_i (b - a) with
 *               a = xb[p_{k-1} + H + i], b = xb[p_k + i], w_i = 0.5 - 0.5 cos(2 pi i / L)
 *   resample    M == n: y = s.  Otherwise c = min(1, n / M), W = 32 / c and for every j < n
 *               base = (j M) / n, frac = ((j M) % n) / n,
 *               y[j] = sum_i s[base + i] g(frac - i) over the i with 0 <= base + i < M and |frac - i| < W,
 *               g(t) = c sinc(c t) bh(t / W), sinc(u) = sin(pi u) / (pi u), sinc(0) = 1,
 *               bh(u) = 0.35875 + 0.48829 cos(pi u) + 0.14128 cos(2 pi u) + 0.01168 cos(3 pi u)
 * rate == 1 gives p_k = k H and y == x bit for bit.  fs within [100, 128000] (the search window and the template of a
 * step, 6 H doubles, stay in LDS).  The chain of positions of an utterance is one workgroup; a batch runs all its
 * utterances side by side in one grid, and every job's result equals the single call's bit for bit. */
/* M and K of the above; -1 for a bad argument (n < 0, fs or rate out of range or not finite).  No device needed. */
int64_t kwy_pitch_stretched_length(int64_t n, double rate);
int64_t kwy_pitch_frames(int64_t n, int fs, double rate);
/* x, y: n samples (host); positions: kwy_pitch_frames(n, fs, rate) int32 values, written, or NULL */
int kwy_pitch_shift(kwy_ctx *ctx, const double *x, int64_t n, int fs, double rate, double *y, int32_t *positions);
typedef struct kwy_pitch_job {
  const double *x;      /* n samples */
  int64_t n;
  double *y;            /* n samples, written (must not overlap x) */
  int32_t *pos;         /* kwy_pitch_frames(n, fs, rate) positions, written, or NULL */
} kwy_pitch_job;
/* device pointers; enqueued on the context's stream, not synchronised (uses the context's scratch arena) */
int kwy_pitch_shift_batch_dev(kwy_ctx *ctx, const kwy_pitch_job *jobs, int count, int fs, double rate);

/* ---- formant shift --------------------------------------------------------------------- */
/* The reference has no counterpart: its dialog transposes the key and keeps the source's formants.  These entries add
 * the second knob of an analysis / synthesis voice changer, a frequency-axis warp of the spectral envelope, which sets
 * the apparent vocal-tract length.  For a row-major (rows, K) matrix sp of positive envelope values and a ratio rho
 * (rho > 1 moves formants up, rho < 1 down), with l = log(sp[t]):
 *   u_k = k / rho  (one IEEE division, k = 0 .. K-1),   j = floor(u_k),   a = u_k - j
 *   out[t, k] = sp[t, K-1]                          if j >= K-1  (the band nothing maps to holds the edge value)
 *             = sp[t, j]                            if a == 0    (bit for bit: k = 0, every bin at rho = 0.5, ...)
 *             = exp(l[j] + a * (l[j+1] - l[j]))     otherwise    (linear in the log domain, evaluated as written)
 * j, a and the choice between the three depend on (k, rho) only.  rho must be finite and within [0.5, 2]: KWY_EINVAL
 * otherwise, and nothing is written.  At rho == 1 out is sp bit for bit, nothing is examined and every status is 0.
 * A row that holds a value that is not finite or is <= 0 is copied unchanged and counted in its job's status word.
 * 2 <= K <= KWY_FORMANT_MAX_K, the envelope width of the longest transform CheapTrick accepts.  out may equal sp: a
 * row is stored only after all of it has been read.  The aperiodicity is deliberately not warped: it describes the
 * excitation per absolute frequency band.  Every job's result equals the single call's bit for bit: it depends on the
 * job alone.  The _dev forms allocate nothing and do not synchronise (legal inside a stream capture); the host form
 * stages through HBM and synchronises. */
#define KWY_FORMANT_MAX_K 2049
typedef struct kwy_formant_job {
  const double *sp;     /* rows x K envelope values */
  int64_t rows;
  double *out;          /* rows x K, written (may equal sp) */
} kwy_formant_job;
/* status: one int32 per job (or NULL), set to the number of the job's rows that were copied unchanged */
int kwy_formant_shift(kwy_ctx *ctx, const kwy_formant_job *jobs, int count, int K, double rho, int32_t *status);
int kwy_formant_shift_dev(kwy_ctx *ctx, const double *sp, int64_t rows, int K, double rho, double *out,
                          int32_t *status);
int kwy_formant_shift_batch_dev(kwy_ctx *ctx, const kwy_formant_job *jobs, int count, int K, double rho,
                                int32_t *status);

/* ---- objective evaluation ------------------------------------------------------------- */
/* The reference has no counterpart: it compares features only in its tests (tests/feature.py: calc_feature_diffs).
 * These entries add the measures voice-conversion work reports on held-out parallel utterances, taken along an
 * alignment (the index lists of kwy_align_even_dev, or any other):
 *   mel-cepstral distortion (Kubichek 1993), per selected row t
 *     mcd[t] = (10 / ln 10) * sqrt(2 * sum_{d = first_col .. cols-1} (a[ia[t], d] - b[ib[t], d])^2)      dB
 *   f0 error: 1200 * log2(fa / fb) cents over the rows where both tracks are voiced (f0 > 0); its root mean square is
 *     sqrt(M2 / n + mean^2)
 *   voicing error: the confusion counts VV, VU, UV, UU (a voiced / b voiced, a voiced / b unvoiced, ...)
 * Row t of a job reads row idx_a[t] - off_a of a and row idx_b[t] - off_b of b (a NULL list is the identity), so that
 * indices into a padded block can address an unpadded one; a row that falls outside either side this way is not a
 * row of the measure and is passed over.  No gathered copies are made.  The row count is `rows`, or
 * -- _dev forms only -- the device word n_dev[0] clamped to [0, rows] (kwy_align_even_dev's n_out; rows is then the
 * capacity of the lists).  Moments are (n, mean, M2) over the rows that count, M2 the sum of squared deviations from
 * the mean in a second pass; no such row gives (0, 0, 0).  Every reduction has a fixed order: a job's result depends
 * on the job alone, not on the run nor on the other jobs of the call.  The _dev forms allocate nothing and do not
 * synchronise (legal inside a stream capture); the host forms stage through HBM and synchronise. */
typedef struct kwy_mcd_job {
  const double *a;        /* a_rows rows of cols values, a_stride doubles apart (>= cols when there are rows to step over) */
  int64_t a_rows, a_stride;
  const double *b;        /* b_rows rows, b_stride doubles apart */
  int64_t b_rows, b_stride;
  const int32_t *idx_a;   /* rows indices, or NULL: t */
  const int32_t *idx_b;
  int64_t off_a, off_b;
  int64_t rows;
  const int64_t *n_dev;   /* device word with the row count, or NULL (always NULL in the host form) */
  const double *mask;     /* or NULL.  Row t counts when mask[idx_b[t] * mask_stride] > 0: the UNSHIFTED b-side index */
  int64_t mask_stride, mask_rows;
  double *per_row;        /* rows values, written (or NULL): mcd[t], NaN for a row that does not count */
} kwy_mcd_job;
/* cols <= 64; first_col = 1 leaves the power coefficient out.  moments: count x 3 doubles, written.  status: one int32
 * per job (or NULL): the rows left out because one of the coefficients first_col .. cols-1 is not finite on either
 * side; rows whose mask is clear (or whose index lies outside the mask) are not examined. */
int kwy_mcd(kwy_ctx *ctx, const kwy_mcd_job *jobs, int count, int cols, int first_col, double *moments,
            int32_t *status);
int kwy_mcd_batch_dev(kwy_ctx *ctx, const kwy_mcd_job *jobs, int count, int cols, int first_col, double *moments,
                      int32_t *status);
typedef struct kwy_f0_error_job {
  const double *f0_a;     /* a_length values: the track under test */
  int64_t a_length;
  const double *f0_b;     /* b_length values: the track it is measured against */
  int64_t b_length;
  const int32_t *idx_a;   /* as in kwy_mcd_job */
  const int32_t *idx_b;
  int64_t off_a, off_b;
  int64_t rows;
  const int64_t *n_dev;
} kwy_f0_error_job;
/* counts: count x 4 int64 (VV, VU, UV, UU), written; moments: count x 3 doubles, written: the cents over the VV rows.
 * status: one int32 per job (or NULL): the rows left out of every figure because an f0 value is negative or not
 * finite.  The four counts and the status add up to the rows that lie inside both tracks. */
int kwy_f0_error(kwy_ctx *ctx, const kwy_f0_error_job *jobs, int count, int64_t *counts, double *moments,
                 int32_t *status);
int kwy_f0_error_batch_dev(kwy_ctx *ctx, const kwy_f0_error_job *jobs, int count, int64_t *counts, double *moments,
                           int32_t *status);
/* count rows of width triples -> width triples (width <= 64): per column Chan's pairwise combination, a left fold in
 * row order that skips n == 0 (kwy_logf0_moments_merge is this with width 1) -- the totals of a corpus, bit-equal
 * however its utterances were grouped into calls */
int kwy_moments_merge(kwy_ctx *ctx, const double *moments, int count, int width, double *out);
int kwy_moments_merge_dev(kwy_ctx *ctx, const double *moments, int count, int width, double *out);
/* The monitor of a re-alignment pass: acc[0] += sum_i n_i * mean_i, acc[1] += sum_i n_i over count (n, mean, M2)
 * triples in row order (kwy_mcd_batch_dev's output for the pairs of a wave): the distortion summed over the cells of
 * the wave and their number, accumulated across waves in one device block.  No host synchronisation. */
int kwy_moments_accumulate_dev(kwy_ctx *ctx, const double *moments, int count, double *acc);

/* ---- mel-cepstrum ---------------------------------------------------------------- */
/* pysptk.sp2mc(spec, order, alpha) row-wise          kwiiyatta/vocoder/mcep.py:71
 * sp: T x K (K = fftlen/2+1), mc: T x (order+1).  Accepted: T >= 1, 2 <= K <= 4097 (any even fftlen),
 * 1 <= order <= min(63, fftlen/2) and |alpha| < 1, every combination of them; anything else is KWY_EINVAL. */
int kwy_sp2mc(kwy_ctx *ctx, const double *sp, int64_t T, int K, int order, double alpha,
              double *mc);
int kwy_sp2mc_dev(kwy_ctx *ctx, const double *sp, int64_t T, int K, int order, double alpha,
                  double *mc);
/* pysptk.mc2sp(mc, alpha, fftlen) row-wise           kwiiyatta/vocoder/mcep.py:65 */
int kwy_mc2sp(kwy_ctx *ctx, const double *mc, int64_t T, int order, double alpha, int fftlen,
              double *sp);
int kwy_mc2sp_dev(kwy_ctx *ctx, const double *mc, int64_t T, int order, double alpha,
                  int fftlen, double *sp);

/* ---- alignment -------------------------------------------------------------------- */
/* fastdtw.fastdtw(x, y, radius, dist=2) -> (dist, path)
 *                                                    kwiiyatta/vocoder/align.py:71
 * x: Tx x dim, y: Ty x dim; path: capacity (Tx+Ty) x 2 int32, *path_len pairs written.
 * radius >= 1 (KWY_EINVAL otherwise: fastdtw 0.3.2 raises a KeyError for radius 0). */
int kwy_fastdtw(kwy_ctx *ctx, const double *x, int64_t Tx, const double *y, int64_t Ty,
                int dim, int radius, double *dist, int32_t *path, int64_t *path_len);
int kwy_fastdtw_dev(kwy_ctx *ctx, const double *x, int64_t Tx, const double *y, int64_t Ty,
                    int dim, int radius, double *dist, int32_t *path, int64_t *path_len);
/* ... for a batch of pairs (device pointers): every kernel of the level recursion runs all pairs in one grid -- the
 * serial recurrence of a pair is one workgroup, so N pairs occupy N compute units instead of one after the other --
 * what align does pair after pair over a corpus (kwiiyatta/vocoder/align.py:61-96,123-131, convert_voice.py:35-46).
 * Every job's distance and path equal kwy_fastdtw_dev's bit for bit.  The scratch capacities are bounds for any
 * pair of lengths (no overflow, whatever the length ratio). */
typedef struct kwy_dtw_job {
  const double *x;       /* x_length x dim */
  int64_t x_length;
  const double *y;       /* y_length x dim */
  int64_t y_length;
  double *dist;          /* 1 */
  int32_t *path;         /* capacity (x_length + y_length) x 2 */
  int64_t *path_len;     /* 1 */
} kwy_dtw_job;
int kwy_fastdtw_batch_dev(kwy_ctx *ctx, const kwy_dtw_job *jobs, int count, int dim, int radius);

/* Device-side glue that keeps a source/target pair resident in HBM between the
 * stages (used by the batched pipeline; the host API does these in numpy):
 * DTW feature rows [power, voicing, mc1..mcN] -- make_feature(power='binalize',
 * power_pivot='max', vuv='f0')                      kwiiyatta/vocoder/align.py:20-58
 * mc: T x ncoef, out: T x (ncoef+1).  The power coefficients mc[:, 0] must be finite: with a NaN among them the
 * pivot differs from numpy's max (the kernel's fmax skips a NaN, numpy's max returns it); such input is outside the
 * contract. */
int kwy_align_features_dev(kwy_ctx *ctx, const double *mc, int64_t T, int ncoef, const double *f0,
                           double power_weight, double power_threshold, double vuv_weight,
                           double *out);
typedef struct kwy_align_job {
  const double *mc;      /* T x ncoef */
  const double *f0;      /* T (or any per-frame voicing value: > 0 = voiced) */
  int64_t T;
  double *out;           /* T x (ncoef + 1) */
} kwy_align_job;
int kwy_align_features_batch_dev(kwy_ctx *ctx, const kwy_align_job *jobs, int count, int ncoef, double power_weight,
                                 double power_threshold, double vuv_weight);
/* project_path_iter(path, trim, trim_len): one x index per y frame
 *                                                    kwiiyatta/vocoder/align.py:99-120
 * path / path_len as produced by kwy_fastdtw_dev (device); trim_len = 0: no trimming.  A jump in y of any length is
 * filled as the generator fills it.  n_out[0] <- the number of indices the generator yields, whatever the capacity:
 * when it exceeds idx_capacity, idx holds the first idx_capacity of them and nothing is written behind. */
int kwy_align_project_dev(kwy_ctx *ctx, const int32_t *path, const int64_t *path_len, int trim_len,
                          int32_t *idx, int64_t idx_capacity, int64_t *n_out);
typedef struct kwy_project_job {
  const int32_t *path;
  const int64_t *path_len;
  int32_t *idx;
  int64_t idx_capacity;
  int64_t *n_out;
} kwy_project_job;
int kwy_align_project_batch_dev(kwy_ctx *ctx, const kwy_project_job *jobs, int count, int trim_len);
/* Feature.__getitem__(list): dst[i] = src[idx[i]]    kwiiyatta/vocoder/abc/feature.py:170-194
 * An index outside [0, src_rows) does not fail and does not wrap: it is clamped, below 0 to the first row, at or above
 * src_rows to the last one (callers gather a fixed capacity of rows from index lists whose tail is stale). */
int kwy_gather_rows_dev(kwy_ctx *ctx, const double *src, int64_t src_rows, int width,
                        const int32_t *idx, int64_t n, double *dst);
typedef struct kwy_gather_job {
  const double *src;     /* src_rows x width */
  int64_t src_rows;
  const int32_t *idx;    /* n */
  int64_t n;
  double *dst;           /* n x width */
} kwy_gather_job;
int kwy_gather_rows_batch_dev(kwy_ctx *ctx, const kwy_gather_job *jobs, int count, int width);

/* ---- converter apply ---------------------------------------------------------------- */
/* delta_features(X, DELTA_WINDOWS) + MLPG(gmm, windows, diff).transform(X)[:, :d]
 *                         kwiiyatta/converter/delta.py:39-50, gmm.py:28-34
 * x: T x d static features.  GMM: M components over the joint (2*3d)-dim
 * static+delta+delta2 space (source | target), full covariances.
 * y: T x d converted static features. */
int kwy_gmm_mlpg(kwy_ctx *ctx, const double *x, int64_t T, int d, int M,
                 const double *weights, const double *means, const double *covs, int diff,
                 double *y);
int kwy_gmm_mlpg_dev(kwy_ctx *ctx, const double *x, int64_t T, int d, int M,
                     const double *weights, const double *means, const double *covs, int diff,
                     double *y);
/* MLPG(gmm, windows=DELTA_WINDOWS[0:1], diff).transform(X): GMMFeatureConverter.convert(feature, mlpg=False)
 *                                                    kwiiyatta/converter/gmm.py:28-34
 * frame-wise conversion without trajectory smoothing: y_t = sum_m p(m | x_t) E[y | x_t, m] (nnmnkwii MLPGBase).
 * x, y: T x D rows of whatever the mixture was trained on (D <= 128); the mixture is over 2 D joint dimensions. */
int kwy_gmm_convert_frames(kwy_ctx *ctx, const double *x, int64_t T, int D, int M, const double *weights,
                           const double *means, const double *covs, int diff, double *y);
int kwy_gmm_convert_frames_dev(kwy_ctx *ctx, const double *x, int64_t T, int D, int M, const double *weights,
                               const double *means, const double *covs, int diff, double *y);
/* The part of MLPG(gmm, windows, diff).__init__ that depends on the GMM only
 * (nnmnkwii computes it in the constructor, kwiiyatta/converter/gmm.py:32 builds one MLPG per
 * convert call): per mixture the Cholesky factor of Sxx, A = Syx Sxx^-1, b = mu_y - A mu_x, the
 * conditional variances and the log-density constants.  model: kwy_gmm_model_doubles(d, M)
 * doubles of device memory, filled once and reused by kwy_gmm_mlpg_model_dev for every utterance.
 * kwy_gmm_prepare_dev synchronises the stream (it reports a non-positive-definite Sxx). */
int64_t kwy_gmm_model_doubles(int d, int M);
int kwy_gmm_prepare_dev(kwy_ctx *ctx, const double *weights, const double *means, const double *covs,
                        int d, int M, int diff, double *model);
int kwy_gmm_mlpg_model_dev(kwy_ctx *ctx, const double *x, int64_t T, int d, int M, const double *model,
                           double *y);
/* MelCepstrumFeatureConverter.convert(mel_cepstrum) at the converter's sampling rate
 *                                                    kwiiyatta/converter/mcep.py:47-61
 * mc, mc_out: T x (d+1); column 0 (the power coefficient) is kept, columns 1..d are converted (delta features,
 * GMM, MLPG) with a prepared model (diff = 0 or 1 as given to kwy_gmm_prepare_dev). */
int kwy_convert_mcep_dev(kwy_ctx *ctx, const double *mc, int64_t T, int d, int M, const double *model,
                         double *mc_out);
/* ... for a batch of utterances: the frame-parallel kernels (deltas, mixture log-densities on the matrix cores,
 * conditional means) run over the frames of all of them, the trajectory solves of all of them share two launches
 * (convert_voice.py:35-46 converts file after file).  Every job's result equals kwy_convert_mcep_dev's bit for bit. */
typedef struct kwy_convert_job {
  const double *mc;      /* T x (d + 1) */
  int64_t T;
  double *mc_out;        /* T x (d + 1) */
} kwy_convert_job;
int kwy_convert_mcep_batch_dev(kwy_ctx *ctx, const kwy_convert_job *jobs, int count, int d, int M,
                               const double *model);
/* EM trajectory conversion over soft mixture posteriors (an addition: nnmnkwii, like the entries above, picks one arg-max
 * mixture per frame, the "sub-optimal mixture sequence" of Toda, Black and Tokuda 2007; this is that paper's method).
 * With the prepared model's mux_m, muy_m, A_m, v_m (the diagonal conditional variance, `diff` folded in), the source's
 * delta features X (T x D, D = 3 d) and logp[t,m] = log w_m + log N(X_t; mux_m, Sxx_m):
 *     E[m,t]   = muy_m + A_m (X_t - mux_m)
 *     g[t,m]   = softmax over m of logp[t,:]
 *     for k = 0 .. em_iterations:
 *         pbar[t,c] = sum_m g[t,m] / v_m[c]
 *         r[t,c]    = sum_m g[t,m] E[m,t][c] / v_m[c]                               (m ascending)
 *         y_k       = per static dimension the solution of W' diag(pbar) W y = W' r   (the MLPG solver above)
 *         Y_k       = [y_k | 0.5 (y_k[t+1] - y_k[t-1]) | y_k[t+1] - 2 y_k[t] + y_k[t-1]], zeros outside the utterance
 *         l[t,m]    = logp[t,m] - 0.5 sum_c (log(2 pi v_m[c]) + (Y_k[t,c] - E[m,t][c])^2 / v_m[c])
 *         L_k       = sum_t logsumexp_m l[t,:]
 *         g[t,m]    = softmax over m of l[t,:]
 * The result is y_em_iterations; loglik (em_iterations + 1 doubles, or NULL) receives L_0 .. L_em_iterations.  The
 * posteriors are taken under the diagonal conditional model that the solve maximises, so this is exact EM:
 * L_k never decreases.  em_iterations is a fixed count in [0, KWY_MLPG_EM_MAX]: no convergence test, and the _dev forms
 * do not synchronise (legal inside a stream capture).  0 is the single solve under the source-only posteriors; the
 * arg-max entries above are this scheme with g replaced by a one-hot and em_iterations = 0.  Without loglik the closing
 * E-step that only yields the last L is skipped; y does not depend on whether loglik is given.  An em_iterations out of
 * range, or an argument the entries above refuse, returns KWY_EINVAL with nothing written; count == 0 is KWY_OK.
 * Every job of a batch equals the single call's bits.  kwy_gmm_mlpg_em: host pointers, as kwy_gmm_mlpg;
 * kwy_convert_mcep_em_dev: device pointers (loglik too), column 0 kept, as kwy_convert_mcep_dev. */
#define KWY_MLPG_EM_MAX 16
int kwy_gmm_mlpg_em(kwy_ctx *ctx, const double *x, int64_t T, int d, int M, const double *weights,
                    const double *means, const double *covs, int diff, int em_iterations, double *y,
                    double *loglik);
int kwy_convert_mcep_em_dev(kwy_ctx *ctx, const double *mc, int64_t T, int d, int M, const double *model,
                            int em_iterations, double *mc_out, double *loglik);
typedef struct kwy_convert_em_job {
  const double *mc;      /* T x (d + 1) */
  int64_t T;
  double *mc_out;        /* T x (d + 1) */
  double *loglik;        /* em_iterations + 1 doubles on the device, or NULL */
} kwy_convert_em_job;
int kwy_convert_mcep_em_batch_dev(kwy_ctx *ctx, const kwy_convert_em_job *jobs, int count, int d, int M,
                                  const double *model, int em_iterations);
/* Parameter generation considering the global variance (an addition: section IV of the same paper).  The postfilter
 * kwy_gv_postfilter scales a converted track linearly about its mean; this maximises the trajectory likelihood and
 * the likelihood of the trajectory's global variance jointly, starting from that scaled track.  Per utterance of T
 * frames and per static dimension c (the dimensions are independent), with
 *     P, b     the pentadiagonal W' diag(pbar) W and W' r, as records {P[t][t], P[t][t-1], P[t][t-2], b[t]} per (t, c)
 *              (P[0][-1], P[0][-2], P[1][-1] are not read)
 *     y_ML     the solution of P y = b
 *     s        an offset track (zero when NULL): z = y + s is the track whose variance counts
 *     mu, s2   gv_mean[c], gv_var[c]: mean and variance over the training utterances of the target's per-utterance
 *              variance of this coefficient;    weight > 0;    w = 1 / (3 T)
 *     zbar = mean of z,   v(y) = (1/T) sum_t (z_t - zbar)^2
 *     Q(y) = w (-1/2 y'P y + b'y) - 1/2 weight (v(y) - mu)^2 / s2
 *     g(y) = w (b - P y) - weight (v(y) - mu) / s2 * (2/T) (z - zbar)
 * Start: y_0 = sqrt(mu / v(y_ML)) (z - zbar) + zbar - s (z, zbar of y_ML), taken if Q(y_0) >= Q(y_ML), else y_0 = y_ML.
 * Iterations k = 1 .. N, nonlinear conjugate gradients (Polak-Ribiere+) with an exact line search:
 *     p = g_1 for k = 1;  else beta = max(0, g_k.(g_k - g_k-1) / (g_k-1.g_k-1)), p = g_k + beta p, p = g_k if g_k.p <= 0
 *     v(y + a p) = v(y) + 2 a cov(z, p) + a^2 var(p) (ddof 0), so with A = p'P p, B = p.(b - P y), e = v(y) - mu,
 *     k = weight / s2 the derivative of a -> Q(y + a p) is the cubic
 *         (w B - 2 k e cov) - (w A + k (4 cov^2 + 2 e var)) a - 6 k cov var a^2 - 2 k var^2 a^3
 *     a = its smallest positive real root; y <- y + a p if Q, evaluated at the new point, is not smaller.
 *     Without such a root, with g.p not positive and finite, or with the step refused, the column is frozen: it keeps y
 *     for the remaining iterations.
 * N is a fixed count in [0, KWY_MLPG_GV_MAX]: no convergence test.  objective (N + 1 doubles, or NULL) receives
 * Q_0 .. Q_N of the utterance: the sum over its processed columns in ascending c; the sequence never decreases.
 * A column with v(y_ML) == 0 (a constant track, T == 1) is returned unchanged and adds nothing to the objective.  So
 * does a column whose mu or s2 is not finite or not positive, or whose v(y_ML) is not finite; those are counted in
 * the utterance's status word (one int32 per job, or NULL).  Every reduction has a fixed order and no job depends on
 * another: every job of a batch equals the single call's bits.  The _dev forms take scratch from the context's arena
 * and do not synchronise (legal inside a stream capture once the arena has its size).  d <= 64.  Counts out of range, a
 * weight that is not positive and finite, or a null matrix return KWY_EINVAL with nothing written; count == 0 is
 * KWY_OK.
 * kwy_gv_ascent (host pointers) / kwy_gv_ascent_batch_dev (device pointers: jobs' arrays, gv_mean, gv_var, status):
 * the ascent on the caller's records. */
#define KWY_MLPG_GV_MAX 256
typedef struct kwy_gv_ascent_job {
  const double *band;    /* T x d records of four doubles */
  const double *offset;  /* T x d, or NULL */
  double *y;             /* T x d: in y_ML, out y_N */
  int64_t T;
  double *objective;     /* iterations + 1 doubles, or NULL */
} kwy_gv_ascent_job;
int kwy_gv_ascent(kwy_ctx *ctx, const kwy_gv_ascent_job *jobs, int count, int d, const double *gv_mean,
                  const double *gv_var, double weight, int iterations, int32_t *status);
int kwy_gv_ascent_batch_dev(kwy_ctx *ctx, const kwy_gv_ascent_job *jobs, int count, int d, const double *gv_mean,
                            const double *gv_var, double weight, int iterations, int32_t *status);
/* gv_mean[c], gv_var[c] from (count, cols, 3) column moments: mean and variance (ddof 0, two passes, left folds in
 * index order) of M2 / n over the matrices with n > 0.  gv_mean equals kwy_gv_from_moments' value bit for bit; with
 * fewer than two such matrices gv_var is 0. */
int kwy_gv_stats_from_moments(kwy_ctx *ctx, const double *moments, int count, int cols, double *gv_mean,
                              double *gv_var);
int kwy_gv_stats_from_moments_dev(kwy_ctx *ctx, const double *moments, int count, int cols, double *gv_mean,
                                  double *gv_var);
/* The conversion with the ascent behind it.  The posteriors are fixed first: em_iterations == -1 picks one arg-max
 * mixture per frame (kwy_gmm_mlpg / kwy_convert_mcep_dev), em_iterations in [0, KWY_MLPG_EM_MAX] runs the EM scheme
 * above; the ascent then runs on the P, b of the last solve and on its y.  gv_offset == 1: s = the source's static
 * coefficients (for a model prepared with diff = 1: the trajectory is the differential y - x and the variance that
 * matters is that of the converted spectrum); 0: s = 0.  gv_mean, gv_var: d values for c1..cd.  loglik
 * (em_iterations + 1 doubles, or NULL; ignored with em_iterations == -1), objective (gv_iterations + 1 doubles, or
 * NULL), status (one int32 per job, or NULL).  kwy_gmm_mlpg_gv: host pointers, as kwy_gmm_mlpg_em;
 * kwy_convert_mcep_gv_dev / _batch_dev: device pointers (gv_mean, gv_var, loglik, objective and status too), column 0
 * kept.  Refusals as above and as the EM entries'. */
int kwy_gmm_mlpg_gv(kwy_ctx *ctx, const double *x, int64_t T, int d, int M, const double *weights,
                    const double *means, const double *covs, int diff, int em_iterations, int gv_offset,
                    const double *gv_mean, const double *gv_var, double weight, int gv_iterations, double *y,
                    double *loglik, double *objective, int32_t *status);
int kwy_convert_mcep_gv_dev(kwy_ctx *ctx, const double *mc, int64_t T, int d, int M, const double *model,
                            int em_iterations, int gv_offset, const double *gv_mean, const double *gv_var,
                            double weight, int gv_iterations, double *mc_out, double *loglik, double *objective,
                            int32_t *status);
typedef struct kwy_convert_gv_job {
  const double *mc;      /* T x (d + 1) */
  int64_t T;
  double *mc_out;        /* T x (d + 1) */
  double *loglik;        /* em_iterations + 1 doubles on the device, or NULL */
  double *objective;     /* gv_iterations + 1 doubles on the device, or NULL */
} kwy_convert_gv_job;
int kwy_convert_mcep_gv_batch_dev(kwy_ctx *ctx, const kwy_convert_gv_job *jobs, int count, int d, int M,
                                  const double *model, int em_iterations, int gv_offset, const double *gv_mean,
                                  const double *gv_var, double weight, int gv_iterations, int32_t *status);
/* Re-alignment of the training set (an addition: the reference aligns once): the same batched conversion, with the
 * converted c1..cd of every job stored straight into columns 2.. of its DTW feature rows (kwy_align_features_dev's
 * layout, rows d + 2 doubles apart) -- columns 0 and 1, the source's own power and voicing terms, are not touched, and no
 * T x (d + 1) intermediate is made.  Columns 2.. equal columns 1.. of kwy_convert_mcep_dev's output for the same mc and
 * model bit for bit.  Any count (KWY_BATCH_MAX = 16 utterances share a pass of launches); no host synchronisation. */
typedef struct kwy_realign_job {
  const double *mc;      /* T x (d + 1): the padded source mel-cepstrum */
  int64_t T;
  double *feat;          /* T x (d + 2) DTW features, columns 2.. written */
} kwy_realign_job;
int kwy_realign_features_batch_dev(kwy_ctx *ctx, const kwy_realign_job *jobs, int count, int d, int M,
                                   const double *model);

/* ---- cross-rate aperiodicity codec ------------------------------------------------------
 * pyworld.code_aperiodicity(ap, fs) / pyworld.decode_aperiodicity(coded, fs, fft_size)
 *                                        kwiiyatta/vocoder/world.py:98-145
 * ap: T x (fft_size/2+1); coded: T x kwy_aperiodicity_bands(fs) on the coding side.  The
 * decoder takes the number of coded columns explicitly (the reference truncates or extends the
 * coded array when it changes the sampling rate, world.py:121-143), at most kwy_aperiodicity_bands(fs) of them:
 * with more, the band centres would reach fs/2 and the interpolation grid would not increase (KWY_EINVAL). */
int kwy_aperiodicity_bands(int fs);
int kwy_code_aperiodicity(kwy_ctx *ctx, const double *ap, int64_t T, int fs, int fft_size, double *coded);
int kwy_code_aperiodicity_dev(kwy_ctx *ctx, const double *ap, int64_t T, int fs, int fft_size, double *coded);
int kwy_decode_aperiodicity(kwy_ctx *ctx, const double *coded, int64_t T, int fs, int fft_size, int bands,
                            double *ap);
int kwy_decode_aperiodicity_dev(kwy_ctx *ctx, const double *coded, int64_t T, int fs, int fft_size, int bands,
                                double *ap);

/* ---- aperiodicity conversion (an addition: the reference renders a converted voice with the source's aperiodicity) ----
 * The aperiodic component as one more stream of the joint-density GMM conversion (Ohtani et al. 2006: a mixture on band
 * aperiodicity; sprocket's `codeap` mixture).  B = kwy_aperiodicity_bands(fs) must be >= 1 (fs >= 12 kHz): with B == 0
 * every entry below returns KWY_EINVAL.
 *
 * BAND TRACK of an utterance with aperiodicity ap (T x K, K = fft_size / 2 + 1): S, T x (B + 1).
 *   c[t, b]    the coded value in dB, k_code_aperiodicity's arithmetic: bit-equal to kwy_code_aperiodicity_dev.
 *   S[t, 0]    v[t] = 1.0 when (sum_b c[t, b]) / B <= -0.5, else 0.0 -- the sum a left fold, b ascending, compared with
 *              > -0.5 exactly as k_decode_aperiodicity does: v[t] == 0 exactly for the frames the decoder flattens to
 *              1 - 1e-12.  D4C writes that row for f0 = 0, so no f0 track is needed; the pad rows of a training item
 *              (1 - 1e-12) come out unvoiced by themselves.
 *   S[t, 1..B] c[t, :] for a voiced frame; for an unvoiced one the row of the nearest voiced frame before it, and
 *              without one that of the nearest voiced frame after it ("hold fill": the delta windows see no 0 dB spike
 *              at a voicing boundary, in training and in conversion alike).  A track without any voiced frame keeps c.
 *
 * TRAINING ROWS of an aligned pair with tracks X, Y and the kept cells (ix[k], iy[k]), k < n -- the lists the
 * mel-cepstrum rows use (dtw_feature(strict) + align_even's cut): gx[k] = X[ix[k], 1:], gy[k] = Y[iy[k], 1:]; the delta
 * features of both gathered sequences as kwy_delta_features_dev takes them; row k = [gx, dgx, ddgx | gy, dgy, ddgy][k],
 * 6 B wide, kept only if X[ix[k], 0] == 1 and Y[iy[k], 0] == 1.  Kept rows go, in order, behind the device cursor
 * as kwy_train_rows_batch_dev's do; a pair that does not fit is dropped whole with n_rows = -1 - rows.  An index
 * outside its track reads the track's nearest row.
 *
 * CONVERSION: Y^ = kwy_convert_mcep(_batch)_dev(S, d = B, M, model(diff = 0)): arg-max MLPG, column 0 travels through.
 * Then, IN PLACE over ap: row t with v[t] == 1 becomes the decode of clamp(Y^[t, 1:], -60, -1e-12) with
 * k_decode_aperiodicity's arithmetic, its flat-row rule included (bit-equal to kwy_decode_aperiodicity_dev on the
 * clamped row); a row with v[t] == 0 is not written, so an utterance without a voiced frame is left as it is.
 *
 * BAND ERROR along an alignment: over the cells voiced on both sides, sqrt(sum_b (a - b)^2 / B) in dB, as the
 * (n, mean, M2) triples of kwy_mcd_batch_dev (rows, index lists, offsets and n_dev as in kwy_mcd_job; fixed reduction
 * order).
 *
 * The _dev forms allocate nothing and do not synchronise (kwy_bap_rows_batch_dev takes 8 bytes per pair from the
 * context's scratch arena); the host forms stage through HBM and synchronise. */
typedef struct kwy_bap_track_job {
  const double *ap;          /* T x K; a padded training item is one job */
  int64_t T;
  double *track;             /* T x (B + 1), written */
} kwy_bap_track_job;
int kwy_bap_track(kwy_ctx *ctx, const kwy_bap_track_job *jobs, int count, int fs, int fft_size);
int kwy_bap_track_dev(kwy_ctx *ctx, const double *ap, int64_t T, int fs, int fft_size, double *track);
int kwy_bap_track_batch_dev(kwy_ctx *ctx, const kwy_bap_track_job *jobs, int count, int fs, int fft_size);
typedef struct kwy_bap_rows_job {
  const double *track_x;     /* x_rows x (B + 1) */
  int64_t x_rows;
  const double *track_y;     /* y_rows x (B + 1) */
  int64_t y_rows;
  const int32_t *idx_x;      /* capacity cells */
  const int32_t *idx_y;
  const int64_t *n_dev;      /* device word with the cell count, clamped to [0, capacity]; NULL: capacity cells (always
                                NULL in the host form) */
  int64_t capacity;
  int64_t *n_rows;           /* 1, written: the rows kept, or -1 - rows for a pair that did not fit */
} kwy_bap_rows_job;
/* joint: capacity_rows x 6 B doubles; cursor[0]: rows written so far, read and advanced in job order */
int kwy_bap_rows(kwy_ctx *ctx, const kwy_bap_rows_job *jobs, int count, int bands, double *joint,
                 int64_t capacity_rows, int64_t *cursor);
int kwy_bap_rows_batch_dev(kwy_ctx *ctx, const kwy_bap_rows_job *jobs, int count, int bands, double *joint,
                           int64_t capacity_rows, int64_t *cursor);
typedef struct kwy_bap_apply_job {
  const double *track_src;   /* T x (B + 1): the band track of ap as analysed (its column 0 decides) */
  const double *track_conv;  /* T x (B + 1): the converted track */
  int64_t T;
  double *ap;                /* T x K, voiced rows rewritten in place */
} kwy_bap_apply_job;
int kwy_bap_apply(kwy_ctx *ctx, const kwy_bap_apply_job *jobs, int count, int fs, int fft_size);
int kwy_bap_apply_dev(kwy_ctx *ctx, const double *track_src, const double *track_conv, int64_t T, int fs,
                      int fft_size, double *ap);
int kwy_bap_apply_batch_dev(kwy_ctx *ctx, const kwy_bap_apply_job *jobs, int count, int fs, int fft_size);
typedef struct kwy_bap_error_job {
  const double *a;           /* a_rows x (B + 1): the track under test */
  int64_t a_rows;
  const double *b;           /* b_rows x (B + 1): the track it is measured against */
  int64_t b_rows;
  const int32_t *idx_a;      /* as in kwy_mcd_job */
  const int32_t *idx_b;
  int64_t off_a, off_b;
  int64_t rows;
  const int64_t *n_dev;
  double *per_row;           /* rows values, written (or NULL): the cell's error, NaN for a cell that does not count */
} kwy_bap_error_job;
/* moments: count x 3 doubles, written */
int kwy_bap_error(kwy_ctx *ctx, const kwy_bap_error_job *jobs, int count, int bands, double *moments);
int kwy_bap_error_batch_dev(kwy_ctx *ctx, const kwy_bap_error_job *jobs, int count, int bands, double *moments);

/* ---- spectral-axis stretch (another number of bins at the same sampling rate) ------------------------
 * Synthesizer._reshape_feature on log values, as reshape_spectrum_envelope / reshape_aperiodicity call it:
 *   np.exp(scipy.signal.resample_poly(np.hstack((edge x pad, np.log(rows), edge x pad)), new_K, K, axis=1)[:, trim:-trim])
 *                                        kwiiyatta/vocoder/abc/synthesizer.py:31-54
 * rows: T x K (positive), out: T x new_K.  The FIR (scipy's firwin, Kaiser beta 5, 20 max(up, down) + 1 taps) is
 * designed by the library per (K, new_K) and cached in the context. */
int kwy_stretch_log(kwy_ctx *ctx, const double *rows, int64_t T, int K, int new_K, double *out);
int kwy_stretch_log_dev(kwy_ctx *ctx, const double *rows, int64_t T, int K, int new_K, double *out);

/* ---- numpy's legacy normal generator (the source of pad_silence's spectra) --------------------------------------
 * np.abs(np.random.normal(0, EPS / fs, (frame_len, spectrum_len)))
 *        WorldSynthesizer._silence_spectrum_envelope, kwiiyatta/vocoder/world.py:158-161 (via pad_silence,
 *        vocoder/abc/feature.py:19-41, for both sides of every aligned pair)
 * out[i] = loc + scale * g_i (its absolute value when take_abs), i < n, where g continues numpy's RandomState stream
 * from `state`: MT19937 + polar Box-Muller with the same accept / reject decisions and the same use of the cached
 * second value; `state` is advanced exactly as numpy advances it.  state: kwy_np_state_bytes() bytes laid out as
 * { uint32 key[624]; int32 pos; int32 has_gauss; double cached_gaussian } = numpy's get_state() tuple.  Values agree
 * with numpy's up to the rounding of log() (<= 1 ulp). */
int64_t kwy_np_state_bytes(void);
int kwy_np_normal(kwy_ctx *ctx, void *state, double loc, double scale, int take_abs, int64_t n, double *out);
int kwy_np_normal_dev(kwy_ctx *ctx, void *state, double loc, double scale, int take_abs, int64_t n, double *out);
/* `count` consecutive requests of n_each values each in one call -- the four pad blocks of one aligned pair (source
 * head, source tail, target head, target tail), or those of all pairs of a batch in pair order; outs: HOST array of
 * `count` device pointers */
int kwy_np_normal_blocks_dev(kwy_ctx *ctx, void *state, double loc, double scale, int take_abs, int count,
                             int64_t n_each, double *const *outs);

/* ---- MLSA differential-spectrum filter ---------------------------------------------------
 * pysptk.mc2b(mc, alpha)                                     kwiiyatta/filter/mlsa.py:28
 * pysptk.synthesis.Synthesizer(MLSADF(order, alpha, pd), hopsize).synthesis(x, b)     :24-29
 * mc, b: T x (order+1).  Frame i filters samples [i hopsize, (i+1) hopsize) with coefficients
 * interpolated linearly from frame i-1's to frame i's (frame 0 from its own); the input is
 * scaled by exp(b[0]); frames that reach the end of x are left unprocessed (output 0 there;
 * upstream leaves them uninitialised).  pd: Pade order, 4 (pysptk default) or 5.  x, y: n samples. */
int kwy_mc2b(kwy_ctx *ctx, const double *mc, int64_t T, int order, double alpha, double *b);
int kwy_mc2b_dev(kwy_ctx *ctx, const double *mc, int64_t T, int order, double alpha, double *b);
int kwy_mlsa_synthesis(kwy_ctx *ctx, const double *x, int64_t n, const double *b, int64_t T, int order,
                       double alpha, int pd, int hopsize, double *y);
int kwy_mlsa_synthesis_dev(kwy_ctx *ctx, const double *x, int64_t n, const double *b, int64_t T, int order,
                           double alpha, int pd, int hopsize, double *y);
/* kwiiyatta.apply_mlsa_filter for a batch of signals (device pointers, not synchronised): what convert_voice.py writes
 * as <name>.diff.wav for every file (kwiiyatta/convert_voice.py:19,39-40; filter/mlsa.py:9-30) -- pysptk.mc2b of the
 * job's mel-cepstra (ignore_c0 != 0: with c0 taken as zero, filter/mlsa.py's `mcep.data[:, 0] = 0`), then the MLSA
 * filter over the waveform, one wavefront per signal and all signals of the batch side by side in one launch (the
 * recursion is serial in the sample: N signals occupy N compute units).  Every job's output equals kwy_mc2b_dev +
 * kwy_mlsa_synthesis_dev bit for bit. */
typedef struct kwy_mlsa_job {
  const double *x;      /* x_length samples in */
  int64_t x_length;
  const double *mc;     /* T x (order + 1) mel-cepstra */
  int64_t T;
  double *y;            /* x_length samples out */
} kwy_mlsa_job;
int kwy_mlsa_filter_batch_dev(kwy_ctx *ctx, const kwy_mlsa_job *jobs, int count, int order, double alpha, int pd,
                              int hopsize, int ignore_c0);

/* ---- frame-parallel FFT form of the differential filter -------------------------------------
 * The filter the MLSA filter approximates, H(z) = exp sum_m c_m z~^-m, applied frame by frame through its closed
 * frequency response (overlap-save), all frames of all signals side by side.  An option beside the MLSA filter, not a
 * replacement: the MLSA filter interpolates the coefficients across a frame, this one crossfades the outputs of the
 * two fixed filters over the same samples with the same weights.
 *   x: n samples, mc: T x (order+1) mel-cepstra, N = fft_size, hop = hopsize, m0 = ignore_c0 ? 1 : 0
 *   w_k = 2 pi k / N,  w~_k = w_k + 2 atan2(alpha sin w_k, 1 - alpha cos w_k)
 *   H_i[k] = exp( sum_{m = m0 .. order} mc[i][m] e^{-j m w~_k} ),  k = 0 .. N/2   (real at k = 0 and k = N/2)
 *   nproc = min(T, (n - 1) / hop) (integer division: the MLSA filter's rule); y[nproc hop ..] = 0.0 exactly, so
 *   n <= hop gives an all-zero output.  For frame i < nproc:
 *     X = rfft of the N samples x[(i+1) hop - N .. (i+1) hop), samples before index 0 counting as zero
 *     a = irfft(X H_{max(i-1, 0)}), b = irfft(X H_i), the last hop samples of each
 *     y[i hop + j] = (1 - j/hop) a_j + (j/hop) b_j,  j = 0 .. hop-1
 * Every output sample is written by exactly one workgroup, without atomics or accumulation in memory: the result is
 * bit-reproducible from run to run and does not depend on the batch a signal is part of.
 * KWY_EINVAL, nothing written: fft_size outside {1024, 2048, 4096, 8192} or <= hopsize, hopsize < 1, an order
 * kwy_mlsa_synthesis does not accept (2 .. 62), a null pointer, an empty input, y overlapping x (a frame reads the
 * input of the frames before it).
 * kwy_mcep_filter_fft_size: max(1024, smallest power of two >= hopsize + ceil(0.025 fs)), 0 if that exceeds 8192 (the
 * transforms the LDS FFTs provide): 1024 at 16 / 22.05 kHz, 2048 at 44.1 / 48 kHz, 4096 at 96 kHz with 5 ms frames.
 * With fft_size - hopsize >= 25 ms the impulse response behind the kept samples is at rounding level for
 * |log H| <= 3.6, so the N-point filter is the exact LTI filter to working precision.  Needs no device.
 * _dev: device pointers, not synchronised, legal inside a stream capture once the tables of (fft_size, alpha) exist
 * (the first call makes them).  _batch_dev: every job equals the single call bit for bit; more jobs than one launch
 * holds are split; count == 0 is KWY_OK. */
int kwy_mcep_filter_fft_size(int fs, int hopsize);
int kwy_mcep_filter_fft(kwy_ctx *ctx, const double *x, int64_t n, const double *mc, int64_t T, int order, double alpha,
                        int hopsize, int fft_size, int ignore_c0, double *y);
int kwy_mcep_filter_fft_dev(kwy_ctx *ctx, const double *x, int64_t n, const double *mc, int64_t T, int order,
                            double alpha, int hopsize, int fft_size, int ignore_c0, double *y);
int kwy_mcep_filter_fft_batch_dev(kwy_ctx *ctx, const kwy_mlsa_job *jobs, int count, int order, double alpha,
                                  int hopsize, int fft_size, int ignore_c0);

/* ---- mel-cepstral energy: power-preserving c0 and the formant-emphasis postfilter --------------
 * The reference has no counterpart (kwiiyatta/convert_voice.py:35-46 synthesises the converter's output as it is).
 * c0 of a mel-cepstrum is not its power: the energy of a frame is the mean of |H|^2 with log |H| = sum c_m cos(m w~),
 * so changing c1.. at a fixed c0 moves it.  For a row c of order + 1 coefficients, alpha and N = fft_size:
 *   w_k = 2 pi k / N,   w~_k = w_k + 2 atan2(alpha sin w_k, 1 - alpha cos w_k)             (as kwy_mcep_filter_fft)
 *   L_k = sum_{m = 0 .. order} c[m] cos(m w~_k),   m ascending
 *   E(c) = ( exp(2 L_0) + exp(2 L_{N/2}) + 2 sum_{k = 1 .. N/2 - 1} exp(2 L_k) ) / N
 * E(c) is the energy of the filter's N-periodic impulse response.  SPTK's mc2e truncates that response at irleng
 * samples; this takes all of it, so no parity with SPTK is claimed.  No spectrum is stored: the kernel reads a table
 * of cos(m w~_k), (order + 1) x (N/2 + 1) doubles per (N, alpha, order), kept with the context.
 * The filter of a row x with strength beta in [0, 1] (the mel-cepstral formant emphasis of the HTS vocoder and SPTK's
 * mcpf, renormalised by E instead of a truncated response) and a reference row r (absent: r = x):
 *   b[order] = x[order];  b[m] = x[m] - alpha b[m+1],  m = order-1 .. 0                      (kwy_mc2b)
 *   if order >= 2:  b[1] = b[1] - (beta alpha) b[2];   b[m] = b[m] (1 + beta),  m = 2 .. order
 *   y[order] = b[order];  y[m] = b[m] + alpha b[m+1],  m = order-1 .. 0
 *   y[0] = y[0] + log(E(r) / E(y)) / 2                                (E(y) of y before this line)
 * evaluated operation by operation as written.  beta == 0: y = x before the last line and no b is formed, so with a
 * reference the row keeps x[1..] and gets the c0 at which its energy is the reference's (the power-preserving shift);
 * beta == 0 without a reference copies the row and forms no energy.  out = y, or with a base matrix
 * out = base + (y - x) element by element (the differential form, as the GV and MS filters have it).  A row where E(r)
 * or E(y) is not finite or not > 0, or whose correction is not finite, takes y = x: it is copied bit for bit from base
 * (from x without one) and counted in the matrix's status word; so is every row at beta == 0 without a reference,
 * uncounted.  The reductions over k have a fixed order: a row's result depends on the row, alpha, N, beta and its
 * reference alone -- not on the run, nor on the batch, nor on the launch it ran in.  No atomics, nothing accumulated in
 * memory.
 * KWY_EINVAL, nothing written: order outside [1, 63], fft_size not a power of two within [512, 8192], |alpha| >= 1,
 * beta outside [0, 1], a null jobs / x / out pointer (with rows > 0), negative rows or count.  count == 0 is KWY_OK.
 * out may equal x or base (a workgroup reads its rows before it writes them).  _dev: device pointers, not
 * synchronised, nothing allocated: legal inside a stream capture once the context holds the table of (fft_size,
 * alpha, order) and, for a non-NULL status, its count slots (256 KB) -- the first call makes them.  A workgroup writes
 * the number of rows it copied into a slot of its own and a second kernel adds a matrix's slots up.  _batch_dev: every job equals the single call bit for bit; more jobs than
 * one launch holds are split.  The host forms stage through HBM and synchronise. */
typedef struct kwy_energy_job {
  const double *mc;       /* rows x (order + 1) mel-cepstra */
  int64_t rows;
  double *energy;         /* rows doubles, written */
} kwy_energy_job;
int kwy_mcep_energy(kwy_ctx *ctx, const double *mc, int64_t T, int order, double alpha, int fft_size, double *energy);
int kwy_mcep_energy_dev(kwy_ctx *ctx, const double *mc, int64_t T, int order, double alpha, int fft_size,
                        double *energy);
int kwy_mcep_energy_batch_dev(kwy_ctx *ctx, const kwy_energy_job *jobs, int count, int order, double alpha,
                              int fft_size);
typedef struct kwy_mcpower_job {
  const double *x;        /* rows x (order + 1): the rows that are filtered */
  const double *ref;      /* rows x (order + 1): the rows whose energy the output takes, or NULL (x itself) */
  const double *base;     /* rows x (order + 1), or NULL: out = base + (y - x) */
  double *out;            /* rows x (order + 1), written (may equal x or base) */
  int64_t rows;
} kwy_mcpower_job;
/* status: one int32 per matrix (or NULL), set to the number of rows that were copied because an energy or the
 * correction is unusable */
int kwy_mcep_postfilter(kwy_ctx *ctx, const kwy_mcpower_job *jobs, int count, int order, double alpha, int fft_size,
                        double beta, int32_t *status);
int kwy_mcep_postfilter_dev(kwy_ctx *ctx, const double *x, int64_t rows, int order, double alpha, int fft_size,
                            double beta, const double *ref, const double *base, double *out, int32_t *status);
int kwy_mcep_postfilter_batch_dev(kwy_ctx *ctx, const kwy_mcpower_job *jobs, int count, int order, double alpha,
                                  int fft_size, double beta, int32_t *status);


/* ---- converter fit: EM building blocks --------------------------------------------------------
 * sklearn.mixture.GaussianMixture(covariance_type='full').fit as used at
 *                                                    kwiiyatta/converter/gmm.py:14-26
 * The data are sharded by frames; each call works on the local shard X (n x D, device).
 * A driver (kwiiyatta_amd/converter/gmm_fit.py) runs, per EM iteration,
 *   estep -> sums -> [all-reduce stats] -> means -> cov -> [all-reduce sxx] -> finalize
 * and all-reduces the statistics over RCCL when several GPUs hold shards.
 * M <= 256, D <= 160 (and (D+1) / (256 / 2^ceil(log2 M)) <= 40). */
int kwy_gmm_em_estep_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, int M, const double *weights,
                         const double *means, const double *covs, double *resp /* n x M */,
                         double *loglik_parts /* ceil(n/256) */, int *status_out);
int kwy_gmm_em_sums_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, int M, const double *resp,
                        double *stats /* M x (D+1): [sum r, sum r x] */);
int kwy_gmm_em_means_dev(kwy_ctx *ctx, const double *stats, int D, int M, double *means);
int kwy_gmm_em_cov_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, int M, const double *resp,
                       const double *means, double *sxx /* M x D x D */);
/* the same with the (globally reduced) sums of kwy_gmm_em_sums_dev at hand (stats; NULL = kwy_gmm_em_cov_dev): a
 * frame whose responsibility for a mixture is below 2^-70 of that mixture's mass nk is left out of its covariance
 * sum -- all such frames together weigh less than n 2^-70 of the mixture, below the rounding of nk itself for
 * n <= 2^25 -- which lets the kernel skip the matrix products of the (many) frames that do not belong to a
 * component.  kwy_gmm_em_cov_dev skips below 2^-200 only. */
int kwy_gmm_em_cov_stats_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, int M, const double *resp,
                             const double *means, const double *stats, double *sxx);
int kwy_gmm_em_finalize_dev(kwy_ctx *ctx, const double *stats, const double *sxx, int D, int M,
                            double reg_covar, double *weights, double *covs);
int kwy_gmm_em_scratch_bytes(int64_t n, int D, int M, int64_t *bytes);

/* ---- converter fit: block-diagonal covariances ------------------------------------------------
 * The same EM for a joint-density mixture over z = [x | y] (D = 2 h) whose covariance blocks Sxx, Syy and Sxy = Syx
 * are diagonal (Toda, Black and Tokuda 2007; sprocket's covtype 'block_diag'): pairing x_i with y_i leaves h
 * independent 2 x 2 blocks [[a_i, c_i], [c_i, b_i]] per mixture.  covs_bd and sbd are M x 3 x h doubles, laid out
 * [a | b | c] per mixture.  Per EM iteration a driver runs
 *   estep_bd -> sums -> [all-reduce stats] -> means -> cov_bd -> [all-reduce sbd] -> finalize_bd
 * with kwy_gmm_em_sums_dev and kwy_gmm_em_means_dev from above; EM in this family is exact (the M-step's maximum is
 * the empirical covariance restricted to the pattern).  All pointers are device pointers, nothing
 * synchronises, the stream is the context's.  1 <= M <= 256, D even with 2 <= D <= 160, n >= 1; anything else, a NULL
 * pointer included, is KWY_EINVAL with a message in kwy_last_error.
 *
 * estep_bd: resp (n x M) and loglik_parts (ceil(n/256) doubles, summed in a fixed order: bit-reproducible) as
 *   kwy_gmm_em_estep_dev writes them, from log N(z; mu, S) = -1/2 (D log 2pi + sum_i log(a_i b_i - c_i^2)
 *   + sum_i [b_i dx_i^2 - 2 c_i dx_i dy_i + a_i dy_i^2] / (a_i b_i - c_i^2)).  status_out[0] is set to non-zero when
 *   some block has a <= 0 or a b - c^2 <= 0 (the block is then evaluated as the unit block: the outputs stay finite
 *   and mean nothing), and to zero otherwise.
 * cov_bd: sbd = [sum_t r (x - mux)^2 | sum_t r (y - muy)^2 | sum_t r (x - mux)(y - muy)] over the local shard, summed
 *   in a fixed order without atomics.  stats (the reduced sums, or NULL) is accepted for symmetry with
 *   kwy_gmm_em_cov_stats_dev; every frame is summed either way.
 * finalize_bd: weights as kwy_gmm_em_finalize_dev; a = sa / nk + reg_covar, b = sb / nk + reg_covar, c = sc / nk.
 * expand_bd: the M x D x D matrices -- the three diagonals copied exactly, +0.0 everywhere else -- which the
 *   conversion entries (kwy_gmm_prepare_dev, ...) take as they take any full mixture. */
int kwy_gmm_em_estep_bd_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, int M, const double *weights,
                            const double *means, const double *covs_bd /* M x 3 x D/2 */, double *resp /* n x M */,
                            double *loglik_parts /* ceil(n/256) */, int *status_out);
int kwy_gmm_em_cov_bd_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, int M, const double *resp,
                          const double *means, const double *stats_or_null, double *sbd /* M x 3 x D/2 */);
int kwy_gmm_em_finalize_bd_dev(kwy_ctx *ctx, const double *stats, const double *sbd, int D, int M, double reg_covar,
                               double *weights, double *covs_bd);
int kwy_gmm_expand_bd_dev(kwy_ctx *ctx, const double *covs_bd, int D, int M, double *covs /* M x D x D */);

/* The one-call fits below are full-covariance only: a block-diagonal fit is driven through the building blocks above.
 *
 * The whole fit of ONE rank's rows as one call: GaussianMixture(n_components=M, covariance_type='full', max_iter, tol,
 * reg_covar, random_state=seed).fit(X)                kwiiyatta/converter/gmm.py:14-26
 * -- the k-means initialisation below (numpy's RandomState(seed) draws, scikit-learn's seeding and Lloyd loop) and the
 * EM loop above, run by the library.  X: n x D on the device; weights (M), means (M x D), covs (M x D x D): HOST outputs;
 * n_iter / lower_bound / converged / kmeans_iter: scikit-learn's n_iter_, lower_bound_, converged_ and the number of
 * Lloyd iterations (may be NULL).  Synchronous. */
int kwy_gmm_fit_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, int M, int max_iter, double tol, double reg_covar,
                    uint32_t seed, double *weights, double *means, double *covs, int *n_iter, double *lower_bound,
                    int *converged, int *kmeans_iter);
/* The same fit over the rows of SEVERAL ranks (fit row: "multi-GPU variant takes an RCCL communicator
 * handle"): every rank calls with its own shard X (global row order: rank 0's rows, then rank 1's, ...) and a
 * communicator given as an in-place SUM all-reduce of device doubles on a HIP stream --
 *     int reduce(void *user, double *buf, int64_t count, void *stream) {
 *       return ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, (ncclComm_t)user, (hipStream_t)stream) != ncclSuccess; }
 * -- and all ranks return the same model (that of a one-rank fit of the concatenated rows, up to the rounding of the
 * sums).  What is exchanged: per k-means++ centre the shard totals, <= 8 candidate rows and potentials; per Lloyd
 * iteration M (D + 1) + 1 doubles; per EM iteration M (D + 1) and M D D doubles and the log-likelihood.  comm == NULL:
 * kwy_gmm_fit_dev.  The library does not link RCCL: the callback is the caller's.
 * Errors: what can go wrong on ONE rank -- its arguments (every rank needs n >= 1 rows: an empty shard is an error),
 * its allocations -- is the first quantity the ranks exchange, so either every rank fits or every rank returns an
 * error (the failing ones their own code, the others KWY_EINVAL "another rank failed its set-up"); nobody is left
 * waiting in a collective.  A failure of the callback itself (non-zero return, e.g. an exception in a Python
 * binder) cannot be agreed on and is fatal for the whole group: the caller must tear the group down. */
typedef struct kwy_comm {
  int rank, world;
  int (*all_reduce_sum)(void *user, double *device_buffer, int64_t count, void *stream);   /* 0 = success */
  void *user;
} kwy_comm;
int kwy_gmm_fit_comm_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, int M, int max_iter, double tol,
                         double reg_covar, uint32_t seed, const kwy_comm *comm, double *weights, double *means,
                         double *covs, int *n_iter, double *lower_bound, int *converged, int *kmeans_iter);

/* ---- converter fit: k-means initialisation ------------------------------------------------------
 * The `init_params='kmeans'` step of the same GaussianMixture.fit (kwiiyatta/converter/gmm.py:14-23):
 * sklearn.cluster.KMeans(n_clusters=M, n_init=1) -- centred input, k-means++ seeding with 2 + ln M
 * candidates per centre, Lloyd iterations until the labels stop changing or the summed squared centre
 * shift falls below 1e-4 mean(var(X)) -- whose labels become the one-hot responsibilities of the first
 * M-step.  Sharded by rows like the EM blocks; the driver all-reduces / all-gathers shard totals,
 * candidate rows, potentials and the centroid statistics ("k-means init likewise").
 * All pointers are device pointers; D <= 160, M <= 256, at most 8 candidates per step. */
/* out[0..D) = sum_t (X[t] - shift), out[D..2D) = sum_t (X[t] - shift)^2; shift may be NULL */
int kwy_km_colstats_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, const double *shift, double *out);
/* Xc = X - mean, xsq[t] = |Xc[t]|^2 */
int kwy_km_center_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, const double *mean, double *Xc,
                      double *xsq);
/* k-means++: newd[c][t] = min(closest[t], max(0, |Xc[t] - cand[c]|^2)) for c < L (closest NULL: no min),
 * pots[c] = sum_t newd[c][t] over this shard.  newd: L x n, pots: 8 doubles. */
int kwy_km_pp_dist_dev(kwy_ctx *ctx, const double *Xc, const double *xsq, int64_t n, int D, const double *cand,
                       int L, const double *closest, double *newd, double *pots);
/* np.searchsorted(np.cumsum(closest), vals) over the global row order, shard by shard:
 * kwy_km_pp_total_dev fills csums (kwy_km_chunks(n) chunk totals) and total[0]; with lo / hi = the cumulated totals
 * of the shards before this one / including this one (the same cumulative sums of the all-gathered totals on every
 * rank, so that a value on a shard boundary has exactly one owner; NULL: 0 / lo + this shard's total),
 * kwy_km_pp_pick_dev returns for each vals[c] the local row index of the hit, or -1 if it lies in another shard
 * (first / last: position of this shard; beyond the end -> last row). */
int64_t kwy_km_chunks(int64_t n);
int kwy_km_pp_total_dev(kwy_ctx *ctx, const double *v, int64_t n, double *csums, double *total);
int kwy_km_pp_pick_dev(kwy_ctx *ctx, const double *v, int64_t n, const double *csums, const double *lo,
                       const double *hi, const double *vals, int L, int first, int last, int64_t *idx);
/* Lloyd: labels[t] = argmin_j |c_j|^2 - 2 <Xc[t], c_j> (int32; in: previous labels), resp = one-hot rows
 * (n x M, may be NULL), changed[0] = number of rows whose label changed (uint64).  The centroid sums are
 * kwy_gmm_em_sums_dev(Xc, resp); kwy_km_update_dev turns the reduced [count, sums] into the new centres
 * and the squared shift of every centre. */
int kwy_km_assign_dev(kwy_ctx *ctx, const double *Xc, int64_t n, int D, const double *centers, int M,
                      int32_t *labels, double *resp, unsigned long long *changed);
int kwy_km_update_dev(kwy_ctx *ctx, const double *stats, const double *centers_old, int M, int D,
                      double *centers_new, double *shift2);
/* Up to `iterations` Lloyd iterations back to back WITHOUT the host (one shard: no reduction between the ranks' sums):
 * each is kwy_km_assign_dev + kwy_gmm_em_sums_dev + kwy_km_update_dev followed by the decision sklearn's
 * _kmeans_single_lloyd takes after an iteration, taken on the device; the kernels of the iterations enqueued behind
 * the one that ended the loop return at once.  centers2: 2 x M x D, the centres of iteration i in buffer i & 1.
 * state (int64[4], zeroed by the caller before the first batch): [0] 0 = running, 1 = labels unchanged (strict
 * convergence), 2 = squared centre shift <= abs_tol (summed in numpy's order), 3 = a cluster is empty -- the
 * iteration is left after its sums (labels, resp, stats are its own, the centres not updated) for the caller to
 * relocate and finish (resp is NOT up to date: kwy_km_onehot_dev), 4 = max_iter iterations done; [1] finished iterations; [2] changed labels of the last
 * assignment.  log: 2 doubles per finished iteration (changed labels, centre shift), max_iter rows.
 * Replaces the per-iteration host round trip of sklearn/cluster/_kmeans.py:_kmeans_single_lloyd. */
int kwy_km_lloyd_dev(kwy_ctx *ctx, const double *Xc, int64_t n, int D, double *centers2, int M, int32_t *labels,
                     double *resp, unsigned long long *changed, double *stats, double *shift2, double abs_tol,
                     int iterations, int64_t max_iter, long long *state, double *log);
/* resp[t][:] = the one-hot row of labels[t] (n x M): kwy_km_lloyd_dev sums the centroids from the labels and leaves
 * `resp` alone (4 bytes per frame and iteration instead of M doubles written and read); the caller that wants
 * scikit-learn's `resp` of the k-means initialisation (sklearn/mixture/_base.py:_initialize_parameters) asks for it
 * once, after the loop. */
int kwy_km_onehot_dev(kwy_ctx *ctx, const int32_t *labels, int64_t n, int M, double *resp);

/* ---- non-parallel training: all-pairs nearest-neighbour search ---------------------------------------
 * The search of INCA (Erro, Moreno, Bonafonte 2010: every source frame paired with its nearest target frame and the
 * other way round, the mixture fitted on those pairs, the source converted, the search repeated).  The reference
 * trains on parallel data only and has no counterpart.
 * Q: nq x D queries, C: nc x D candidates, row-major doubles; 1 <= D <= 160 (the k-means limit), nc <= 2^31 - 1.
 *   score     s(t, j) = |c_j|^2 - 2 <q_t, c_j>: |c_j|^2 summed over the columns in ascending order, the product on
 *             v_mfma_f64_16x16x4_f64 with the k-steps ascending (kwy_km_assign_dev's arithmetic).  The score of a pair
 *             is the same bits in whatever tile, slice or launch the pair lands.
 *   idx[t]    the j of the lexicographic minimum of (s(t, j), j): of equal scores the lower index
 *   dist2[t]  sum_k (q_tk - c_jk)^2 for that j, recomputed directly, k ascending, no contraction (NOT s + |q|^2)
 *   A comparison with a score that is not finite is never "less": a query without any finite score gets idx = -1 and
 *   dist2 = NaN and is counted in status[0] (set, not accumulated; status may be NULL).
 *   splits    0: the entry chooses (enough slices to fill the chip when the queries are few); 1 .. KWY_NN_MAX_SPLITS:
 *             that many slices of the candidate range, slice s = [s L, min(nc, (s + 1) L)) with
 *             L = kwy_nn_slice(nc, splits) = ceil(nc / splits) rounded up to a multiple of 64.  A slice without
 *             candidates contributes (+inf, INT_MAX).  The results are bit for bit independent of `splits`.
 *   Rows beyond nc and columns beyond D are padding inside the kernel and cannot win (a padded row scores +inf).
 * KWY_EINVAL, nothing written: D outside [1, 160], nq < 0, splits outside [0, KWY_NN_MAX_SPLITS], and with nq > 0:
 * nc < 1 or beyond the limit, a null Q, C, idx or dist2.  nq = 0 is KWY_OK and writes nothing.
 * The _dev form does not synchronise and does not allocate once the context's scratch holds
 * kwy_nn_scratch_bytes(nq, splits) bytes (kwy_ctx_reserve; splits = 0: the bound for every choice of the entry) --
 * the slices' partial results ([splits][nq] scores and indices) live there -- so it is legal in a stream capture.
 * It uses no atomics. */
#define KWY_NN_MAX_SPLITS 64
int kwy_nn_search(kwy_ctx *ctx, const double *Q, int64_t nq, const double *C, int64_t nc, int D, int splits,
                  int32_t *idx, double *dist2, int32_t *status);
int kwy_nn_search_dev(kwy_ctx *ctx, const double *Q, int64_t nq, const double *C, int64_t nc, int D, int splits,
                      int32_t *idx, double *dist2, int32_t *status);
/* pure host arithmetic, no device needed; 0 for nq <= 0, and for kwy_nn_slice with an argument out of range */
size_t kwy_nn_scratch_bytes(int64_t nq, int splits);
int64_t kwy_nn_slice(int64_t nc, int splits);

/* ---- exemplar-based conversion: KL-NMF activations over coupled dictionaries --------------------------
 * The exemplar converter (Takashima et al. 2012; Wu, Virtanen, Chng, Li 2014): the aligned training frames are the
 * model, a source frame is explained as a sparse non-negative combination of source exemplars, and the same
 * activations applied to the paired target exemplars are the converted frame.  The reference has no counterpart.
 * Row-major doubles:  S: A x B source atoms, Tg: A x B target atoms, X: T x B frames.  Every entry is finite and > 0,
 * and every atom of S and Tg and every frame of X has unit sum over its B bins (the caller's preparation: the
 * entry does not scale and does not check the sums).
 *   H (T x A) starts at all ones, or at h0 (T x A, entries finite and >= 0) when h0 is not NULL.  For n = 1 .. N:
 *       R = H S                      (T x B)
 *       Q = X / max(R, DBL_MIN)      element by element
 *       G = Q S^T                    (T x A)
 *       H <- (H * G) / (1 + lambda)  element by element; atom sums are 1, so the usual denominator S^T 1 + lambda
 *                                    is this constant
 *   Y = H Tg (T x B); H itself (T x A); objective[t] = sum_b (x log(x / max(r, DBL_MIN)) - x + r) + lambda sum_a h
 *   with r = H S of the final H.  Each of Y, H, objective may be NULL; Tg and Y are given together or both NULL.
 *   Frames never interact: a frame's outputs depend on its own row of X (and of h0) only, not on T nor on the other
 *   rows.  The result after n updates does not depend on N: N updates are the first N of any longer run.
 *   Every element of every product is one v_mfma_f64_16x16x4_f64 accumulator chain over its k (atoms for R and Y,
 *   bins for G) in ascending order starting from zero, four k per step; nothing is contracted.  The order is fixed
 *   within one build: a call is bit-reproducible from run to run, and H after n updates is the same bits whether
 *   one call ran n updates or n calls of one update were chained through h0.  It uses no atomics.
 *   status[0] (may be NULL; set, not accumulated): the number of entries of S, Tg and X that are not finite and > 0
 *   plus those of h0 that are not finite and >= 0.  The outputs are written all the same, from the values as given,
 *   and mean nothing when the status is not zero; nothing aborts on the device.
 * KWY_EINVAL, nothing written and nothing launched: A outside [1, 8192], B outside [2, 2049], T < 0 or above
 * 2^31 - 1, N outside [0, 1000], lambda negative or not finite, and with T > 0: a null S or X, Tg without Y or Y
 * without Tg, no output asked for, and for the _dev form a scratch buffer that is NULL or smaller than
 * kwy_nmf_scratch_bytes(A, B, T).  T = 0 is KWY_OK and writes nothing.
 * The _dev form takes device pointers, runs on the context's stream, does not synchronise and allocates nothing:
 * its scratch (zero-padded copies of S, Tg, X, and Q and H) is the caller's buffer.  A ragged batch of utterances
 * is one call with T the sum of their frames. */
int kwy_nmf_convert(kwy_ctx *ctx, const double *S, const double *Tg, const double *X, int A, int B, int64_t T,
                    int iterations, double sparsity, const double *h0, double *Y, double *H, double *objective,
                    int32_t *status);
int kwy_nmf_convert_dev(kwy_ctx *ctx, const double *S, const double *Tg, const double *X, int A, int B, int64_t T,
                        int iterations, double sparsity, const double *h0, double *Y, double *H, double *objective,
                        int32_t *status, void *scratch, size_t scratch_bytes);
/* pure host arithmetic, no device needed; 0 for T <= 0 and for sizes outside the limits */
size_t kwy_nmf_scratch_bytes(int A, int B, int64_t T);

/* ---- training-set path (device-resident) ---------------------------------------------------------
 * What the reference does per parallel pair before the converter fit (Config.load_dataset ->
 * align_dataset -> MelCepstrumDataset -> DeltaFeatureDataset -> make_dataset_to_array,
 * kwiiyatta/config.py:83-104, converter/__init__.py:17-18, converter/dataset.py:49-77), as device
 * calls so that the joint feature rows are produced in HBM.  Counts that depend on the data
 * (path length, kept rows) are device scalars; buffers are sized by their capacities. */
/* TrimmedDataset (dataset.py:49-52): n_out[0] = len(trim_zeros_frames(sp)), rows with L1 norm < eps
 * (nnmnkwii: 1e-7) counting as zero (a row with a NaN is not below eps: it counts as a frame, as np.trim_zeros has
 * it); the caller keeps the FIRST n_out frames, as the reference does */
int kwy_trim_length_dev(kwy_ctx *ctx, const double *sp, int64_t T, int K, double eps, int64_t *n_out);
typedef struct kwy_trim_job {
  const double *sp;      /* T x K */
  int64_t T;
  int64_t *n_out;        /* 1 */
} kwy_trim_job;
int kwy_trim_length_batch_dev(kwy_ctx *ctx, const kwy_trim_job *jobs, int count, int K, double eps);
/* pad_silence's cheap parts (kwiiyatta/vocoder/feature.py:19-41) on the first n frames of analysed utterances that are
 * stored with pad_len frames of room on both ends -- f0_pad (n + 2 pad_len): the f0 track between zeros; ap_pad
 * ((n + 2 pad_len) x K): the rows behind the kept frames = 1 - 1e-12 (the rows in front are the caller's
 * initialisation) -- and, when `voiced` is not NULL, WorldSynthesizer.extract_is_voiced of the padded feature
 * (world.py:147-151).  The pad SPECTRA come from kwy_np_normal_blocks_dev.  A job with n = 0 is allowed; with
 * pad_len = 0 as well it has nothing to write, which is no error. */
typedef struct kwy_pad_job {
  const double *f0;      /* >= n */
  int64_t n;             /* frames kept (kwy_trim_length_dev) */
  double *f0_pad;        /* n + 2 pad_len */
  double *ap_pad;        /* (n + 2 pad_len) x K, rows [pad_len, pad_len + n) analysed */
  double *voiced;        /* n + 2 pad_len, or NULL */
} kwy_pad_job;
int kwy_train_pad_batch_dev(kwy_ctx *ctx, const kwy_pad_job *jobs, int count, int K, int fs, int pad_len);
/* WorldSynthesizer.extract_is_voiced (world.py:147-151): voiced[t] = 1.0 / 0.0 */
int kwy_is_voiced_dev(kwy_ctx *ctx, const double *f0, const double *ap, int64_t T, int K, int fs,
                      double *voiced);
/* dtw_feature's strict filter (align.py:73-92) and align_even's cut to [pad_len, T - pad_len)
 * (align.py:134-146) on a FastDTW path over the DTW features feat_x (Tx x width) / feat_y:
 * idx_x / idx_y <- the x and y of the surviving cells, n_out[0] their number (<= capacity): with more survivors than
 * `capacity`, the first `capacity` of them are stored, nothing is written behind, and n_out[0] = capacity.
 * pad_len = 0: no cut (the reference's pad_silence=False).  A one-cell path comes out twice under `strict` (the
 * reference's chain(path[0], ..., path[-1])) and once without it (its np.array(path)).
 * The path has at most Tx + Ty + 4 cells (any FastDTW path has fewer than Tx + Ty). */
int kwy_align_even_dev(kwy_ctx *ctx, const int32_t *path, const int64_t *path_len, const double *feat_x,
                       const double *feat_y, int width, int strict, int use_power, int use_vuv, int64_t Tx,
                       int64_t Ty, int pad_len, int32_t *idx_x, int32_t *idx_y, int64_t capacity,
                       int64_t *n_out);
/* nnmnkwii delta_features(x, DELTA_WINDOWS) (delta.py:8-12,30): x: n[0] x d (device count, <= capacity
 * rows allocated) -> out: n x 3d = [static | delta | delta-delta], zero-padded at both ends */
int kwy_delta_features_dev(kwy_ctx *ctx, const double *x, const int64_t *n, int64_t capacity, int d,
                           double *out);
/* make_dataset_to_array's np.hstack + remove_zeros_frames (dataset.py:61-77): joint <- [xd[t] | yd[t]]
 * for the rows t < n[0] (n[0] above `capacity` counts as `capacity`) whose L1 norm is not below eps, in order;
 * n_out[0] = rows written.  A row with a NaN is not below eps and is written; nnmnkwii's `s > 0` would leave it
 * out, but the analysis produces no NaN features, so the training path never meets that difference. */
int kwy_joint_rows_dev(kwy_ctx *ctx, const double *xd, const double *yd, const int64_t *n, int64_t capacity,
                       int width, double eps, double *joint, int64_t *n_out);
/* Everything between FastDTW and the training matrix for a batch of aligned pairs, counts staying on the device:
 * dtw_feature's strict filter + align_even's cut (kwy_align_even_dev), the mel-cepstra of the surviving cells without
 * c0, their delta features, np.hstack + remove_zeros_frames, and the APPEND to the matrix
 *   (kwiiyatta/vocoder/align.py:73-92,134-146, converter/mcep.py:10-33, delta.py:15-30, dataset.py:61-77)
 * joint: capacity_rows x (2 * 3 d) doubles; cursor[0]: rows written so far (device; read and advanced in pair order,
 * so the matrix holds the pairs' rows in job order behind whatever was there).  n_rows[0] <- the pair's rows (a pair
 * that does not fit the capacity is dropped whole: n_rows = -1 - rows).  No host synchronisation. */
typedef struct kwy_train_job {
  const int32_t *path;       /* FastDTW path over the padded DTW features */
  const int64_t *path_len;
  const double *feat_x;      /* x_length x (d + 2) DTW features */
  const double *feat_y;      /* y_length x (d + 2) */
  const double *mc_x;        /* x_length x (d + 1) padded mel-cepstra */
  const double *mc_y;        /* y_length x (d + 1) */
  int64_t x_length, y_length;
  int64_t *n_rows;           /* 1 */
} kwy_train_job;
int kwy_train_rows_batch_dev(kwy_ctx *ctx, const kwy_train_job *jobs, int count, int d, int strict, int use_power,
                             int use_vuv, int pad_len, double eps, double *joint, int64_t capacity_rows,
                             int64_t *cursor);

#ifdef __cplusplus
}
#endif
#endif /* KWY_H_ */
