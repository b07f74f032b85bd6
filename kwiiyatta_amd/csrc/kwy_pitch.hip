// kwy_pitch.hip -- waveform pitch shift: a WSOLA time stretch by `rate`, resampled back to the input's length
//
//   positions   p_0 = 0;  p_k = argmin_q sum_{i < L} (xb[q + i] - xb[p_{k-1} + H + i])^2 over q in [a_k - S, a_k + S]
//   stretch     s[m] = a + w_i (b - a),  a = xb[p_{k-1} + H + i],  b = xb[p_k + i]              (k = m / H, i = m % H)
//   resample    y[j] = sum_i s[base + i] g(frac - i),  g = windowed sinc (Blackman-Harris, 32 zero crossings)
//
// (include/kwy.h, "waveform pitch shift", states the operation in full.)  There is no reference call to cite: the
// reference's differential output keeps the source's pitch (kwiiyatta/convert_voice.py:19,39-40).
//
// k_pitch_positions: the chain.  Step k needs p_{k-1}, so an utterance is ONE workgroup that walks k; the utterances
// of a batch are the grid.  Per step the search window xb[lo .. lo + 2S + L) and the template go to LDS, a thread
// takes FOUR consecutive candidates and slides over i in blocks of four: per block it reads four new window values and
// four template values (a broadcast) for sixteen squared differences, each one subtraction and one fused multiply-add.
// The window is stored de-interleaved by four (w[4 j + r] at row r, column j), so that the lanes of a wavefront --
// whose candidates are four samples apart -- read consecutive LDS words.  The argmin with the tie rule is a shuffle
// reduction per wavefront and one LDS exchange between the four wavefronts.  Every thread then knows p_k; two barriers
// per step.
//
// k_pitch_resample: a thread per output sample.  The stretched signal is never stored: a tap forms s[m] from x, the
// two positions of its frame and a table of the cross-fade weights.  No scatter, no atomics.
//
// Results do not depend on the batch: a workgroup reads its own utterance only, and a sample its own taps in order.
#include <math.h>

#include "kwy_internal.hpp"

#define PITCH_GROUP 64         // job records per launch of the table kernel
#define PITCH_MIN_FS 100
#define PITCH_MAX_FS 128000    // H <= 1280: 6 H doubles of window and template fit 64 KB of LDS
#define PITCH_MAX_N (1ll << 30)
#define PITCH_ZEROS 32         // zero crossings of the resampling kernel on each side
#define PITCH_X_BLOCKS 2048

struct pitch_rec {
  const double *x;
  int64_t n;
  double *y;
  int32_t *pos;                // K positions (the caller's, or scratch)
  int64_t M, K;
};
typedef kwy_group<pitch_rec, PITCH_GROUP> pitch_recs;
static_assert(sizeof(pitch_recs) + 8 <= KWY_KERNARG_MAX, "k_pitch_table: the table and one pointer");

__global__ void k_pitch_table(pitch_recs B, pitch_rec *__restrict__ table) {
  const int i = threadIdx.x;
  if (i < B.n) table[i] = B.u[i];
}

// w[i] = 0.5 - 0.5 cos(2 pi i / L), i < H: the rising half of the Hann window, the weight of the new frame
__global__ void k_pitch_window(int H, double *__restrict__ w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < H) w[i] = 0.5 - 0.5 * cos(2.0 * KWY_PI * (double)i / (double)(2 * H));
}

__device__ __forceinline__ double pitch_xb(const double *__restrict__ x, int64_t n, int64_t i) {
  return i >= 0 && i < n ? x[i] : 0.0;
}

// (d, q) beats (bd, bq): smaller distance, then nearer to a, then the smaller q; bq < 0: nothing chosen yet
__device__ __forceinline__ bool pitch_better(double d, int q, double bd, int bq, int a) {
  if (!(d == d) || q < 0) return false;
  if (bq < 0 || d < bd) return true;
  if (d > bd) return false;
  const int e = q > a ? q - a : a - q, be = bq > a ? bq - a : a - bq;
  return e < be || (e == be && q < bq);
}

__global__ __launch_bounds__(KWY_THREADS) void k_pitch_positions(const pitch_rec *__restrict__ table, int H) {
  extern __shared__ double pitch_lds[];
  __shared__ double red_d[KWY_WAVES];
  __shared__ int red_q[KWY_WAVES];
  const pitch_rec U = table[blockIdx.x];
  const int tid = threadIdx.x;
  const int64_t n = U.n, M = U.M;
  const int K = (int)U.K;
  if (K < 1) return;
  if (tid == 0) U.pos[0] = 0;
  const int L = 2 * H, S = H, L4 = L & ~3;
  const int rowlen = H + 3;                 // 4 rowlen >= (2 S + 1 + 3) + L: the candidates padded to fours, plus L
  double *wq = pitch_lds;                   // [4][rowlen]: window sample m at row m & 3, column m >> 2
  double *tpl = pitch_lds + 4 * rowlen;     // [L]
  const double *__restrict__ x = U.x;
  int p_prev = 0;
  for (int k = 1; k < K; ++k) {
    const int64_t a64 = ((int64_t)k * H * n + M / 2) / M;
    const int a = (int)a64;
    int lo = a - S < 0 ? 0 : a - S;
    lo = lo < (int)(n - 1) ? lo : (int)(n - 1);
    const int hi = a64 + S < n - 1 ? a + S : (int)(n - 1);
    const int ncand = hi - lo + 1;
    for (int m = tid; m < 4 * rowlen; m += KWY_THREADS) wq[(m & 3) * rowlen + (m >> 2)] = pitch_xb(x, n, (int64_t)lo + m);
    const int64_t tbase = (int64_t)p_prev + H;
    for (int i = tid; i < L; i += KWY_THREADS) tpl[i] = pitch_xb(x, n, tbase + i);
    __syncthreads();
    double bd = 0.0;
    int bq = -1;
    const int groups = (ncand + 3) >> 2;
    for (int g = tid; g < groups; g += KWY_THREADS) {
      const double *r0 = wq + g, *r1 = r0 + rowlen, *r2 = r1 + rowlen, *r3 = r2 + rowlen;
      double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
      double w0 = r0[0], w1 = r1[0], w2 = r2[0];
#pragma unroll 2
      for (int ib = 0; ib < L4 / 4; ++ib) {
        const double w3 = r3[ib], w4 = r0[ib + 1], w5 = r1[ib + 1], w6 = r2[ib + 1];
        const double t0 = tpl[4 * ib], t1 = tpl[4 * ib + 1], t2 = tpl[4 * ib + 2], t3 = tpl[4 * ib + 3];
        double e;
        e = w0 - t0; d0 = __builtin_fma(e, e, d0);
        e = w1 - t1; d0 = __builtin_fma(e, e, d0);
        e = w2 - t2; d0 = __builtin_fma(e, e, d0);
        e = w3 - t3; d0 = __builtin_fma(e, e, d0);
        e = w1 - t0; d1 = __builtin_fma(e, e, d1);
        e = w2 - t1; d1 = __builtin_fma(e, e, d1);
        e = w3 - t2; d1 = __builtin_fma(e, e, d1);
        e = w4 - t3; d1 = __builtin_fma(e, e, d1);
        e = w2 - t0; d2 = __builtin_fma(e, e, d2);
        e = w3 - t1; d2 = __builtin_fma(e, e, d2);
        e = w4 - t2; d2 = __builtin_fma(e, e, d2);
        e = w5 - t3; d2 = __builtin_fma(e, e, d2);
        e = w3 - t0; d3 = __builtin_fma(e, e, d3);
        e = w4 - t1; d3 = __builtin_fma(e, e, d3);
        e = w5 - t2; d3 = __builtin_fma(e, e, d3);
        e = w6 - t3; d3 = __builtin_fma(e, e, d3);
        w0 = w4; w1 = w5; w2 = w6;
      }
      for (int i = L4; i < L; ++i) {          // (L = 2 H is not a multiple of four when H is odd)
        const double t = tpl[i];
        double e;
        e = wq[((i + 0) & 3) * rowlen + g + ((i + 0) >> 2)] - t; d0 = __builtin_fma(e, e, d0);
        e = wq[((i + 1) & 3) * rowlen + g + ((i + 1) >> 2)] - t; d1 = __builtin_fma(e, e, d1);
        e = wq[((i + 2) & 3) * rowlen + g + ((i + 2) >> 2)] - t; d2 = __builtin_fma(e, e, d2);
        e = wq[((i + 3) & 3) * rowlen + g + ((i + 3) >> 2)] - t; d3 = __builtin_fma(e, e, d3);
      }
      const int c = 4 * g, q = lo + c;
      if (pitch_better(d0, q, bd, bq, a)) { bd = d0; bq = q; }
      if (c + 1 < ncand && pitch_better(d1, q + 1, bd, bq, a)) { bd = d1; bq = q + 1; }
      if (c + 2 < ncand && pitch_better(d2, q + 2, bd, bq, a)) { bd = d2; bq = q + 2; }
      if (c + 3 < ncand && pitch_better(d3, q + 3, bd, bq, a)) { bd = d3; bq = q + 3; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double od = __shfl_xor(bd, off);
      const int oq = __shfl_xor(bq, off);
      if (pitch_better(od, oq, bd, bq, a)) { bd = od; bq = oq; }
    }
    if ((tid & 63) == 0) { red_d[tid >> 6] = bd; red_q[tid >> 6] = bq; }
    __syncthreads();                         // (also: every thread is done with this step's window)
    bd = red_d[0];
    bq = red_q[0];
#pragma unroll
    for (int w = 1; w < KWY_WAVES; ++w)
      if (pitch_better(red_d[w], red_q[w], bd, bq, a)) { bd = red_d[w]; bq = red_q[w]; }
    if (bq < 0) bq = a < lo ? lo : (a > hi ? hi : a);      // (every distance is NaN: the ideal position)
    p_prev = bq;
    if (tid == 0) U.pos[k] = bq;
  }
}

// the resampling kernel: c sinc(c t) bh(t / W)
__device__ __forceinline__ double pitch_tap(double t, double c, double W) {
  const double u = c * t;
  const double pu = KWY_PI * u;
  const double sinc = u == 0.0 ? 1.0 : sin(pu) / pu;
  const double cv = cos(KWY_PI * (t / W));
  const double cc = cv * cv;
  const double bh = 0.35875 + 0.48829 * cv + 0.14128 * (2.0 * cc - 1.0) + 0.01168 * ((4.0 * cc - 3.0) * cv);
  return c * sinc * bh;
}

// blockIdx.y: the utterance; its workgroups stride over the output samples
__global__ __launch_bounds__(KWY_THREADS) void k_pitch_resample(const pitch_rec *__restrict__ table, int H,
                                                                 const double *__restrict__ win) {
  const pitch_rec U = table[blockIdx.y];
  const int64_t n = U.n, M = U.M;
  if (n < 1) return;
  const double c = n < M ? (double)n / (double)M : 1.0, W = (double)PITCH_ZEROS / c;     // (per job: M is rounded)
  const int64_t reach = (int64_t)ceil(W);
  const double *__restrict__ x = U.x;
  const int32_t *__restrict__ pos = U.pos;
  for (int64_t j = (int64_t)blockIdx.x * KWY_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * KWY_THREADS) {
    const int64_t jm = j * M, base = M == n ? j : jm / n;
    const double frac = M == n ? 0.0 : (double)(jm - base * n) / (double)n;
    int64_t m = M == n ? base : (base - reach < 0 ? 0 : base - reach);
    const int64_t m_end = M == n ? base : (base + reach > M - 1 ? M - 1 : base + reach);
    int k = (int)(m / H), i = (int)(m - (int64_t)k * H);
    int64_t pa = k > 0 ? (int64_t)pos[k - 1] + H : 0, pb = k > 0 ? pos[k] : 0;
    double acc = 0.0;
    for (; m <= m_end; ++m) {
      double s;
      if (k == 0) s = pitch_xb(x, n, i);
      else {
        const double a = pitch_xb(x, n, pa + i), b = pitch_xb(x, n, pb + i);
        s = a + win[i] * (b - a);
      }
      if (M == n) acc = s;
      else {
        const double t = frac - (double)(m - base);
        if (fabs(t) < W) acc += s * pitch_tap(t, c, W);
      }
      if (++i == H) {
        i = 0;
        ++k;
        if (m < m_end) { pa = (int64_t)pos[k - 1] + H; pb = pos[k]; }
      }
    }
    U.y[j] = acc;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static bool pitch_rate_ok(double rate) { return rate >= 0.5 && rate <= 2.0; }     // (false for NaN)
static bool pitch_fs_ok(int fs) { return fs >= PITCH_MIN_FS && fs <= PITCH_MAX_FS; }

extern "C" int64_t kwy_pitch_stretched_length(int64_t n, double rate) {
  if (n < 0 || n > PITCH_MAX_N || !pitch_rate_ok(rate)) return -1;
  return (int64_t)floor((double)n * rate + 0.5);
}

extern "C" int64_t kwy_pitch_frames(int64_t n, int fs, double rate) {
  const int64_t M = kwy_pitch_stretched_length(n, rate);
  if (M < 0 || !pitch_fs_ok(fs)) return -1;
  const int64_t H = (int64_t)((double)fs * 0.010);
  return (M + H - 1) / H;
}

static int pitch_check(kwy_ctx *ctx, const kwy_pitch_job *jobs, int count, int fs, double rate) {
  if (!pitch_rate_ok(rate)) { ctx->err = "pitch_shift: rate must be within [0.5, 2.0]"; return KWY_EINVAL; }
  if (!pitch_fs_ok(fs)) { ctx->err = "pitch_shift: fs must be within [100, 128000]"; return KWY_EINVAL; }
  if (!jobs || count < 1) { ctx->err = "pitch_shift: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i)
    if (jobs[i].n < 0 || jobs[i].n > PITCH_MAX_N || (jobs[i].n > 0 && (!jobs[i].x || !jobs[i].y))) {
      ctx->err = "pitch_shift: bad argument";
      return KWY_EINVAL;
    }
  return KWY_OK;
}

// arena bytes of pitch_run: the job table, the cross-fade weights, the positions of the jobs that keep none
static size_t pitch_bytes(const kwy_pitch_job *jobs, int count, int fs, double rate) {
  size_t bytes = kwy_pad(sizeof(pitch_rec) * (size_t)count) + kwy_pad(sizeof(double) * (size_t)(fs / 100 + 1));
  for (int i = 0; i < count; ++i)
    if (!jobs[i].pos) bytes += kwy_pad(sizeof(int32_t) * (size_t)kwy_pitch_frames(jobs[i].n, fs, rate));
  return bytes;
}

// jobs: device pointers; the arena has been begun with pitch_bytes() to spare
static int pitch_run(kwy_ctx *ctx, const kwy_pitch_job *jobs, int count, int fs, double rate) {
  const int H = (int)((double)fs * 0.010);
  pitch_rec *table = kwy_arena<pitch_rec>(ctx, (size_t)count);
  double *win = kwy_arena<double>(ctx, (size_t)(fs / 100 + 1));
  if (!table || !win) { ctx->err = "pitch_shift: scratch arena too small"; return KWY_EHIP; }
  int64_t longest = 0;
  bool starved = false;                // a job's positions did not fit the arena
  KWY_TRY(kwy_for_tables<pitch_recs>(
      count,
      [&](int i) {
        const kwy_pitch_job &j = jobs[i];
        const int64_t M = kwy_pitch_stretched_length(j.n, rate), K = kwy_pitch_frames(j.n, fs, rate);
        int32_t *pos = j.pos ? j.pos : kwy_arena<int32_t>(ctx, (size_t)K);
        starved = starved || !pos;
        if (j.n > longest) longest = j.n;
        return pitch_rec{j.x, j.n, j.y, pos, M, K};
      },
      [&](const pitch_recs &B, int i0) {
        if (starved) { ctx->err = "pitch_shift: scratch arena too small"; return KWY_EHIP; }
        hipLaunchKernelGGL(k_pitch_table, dim3(1), dim3(PITCH_GROUP), 0, ctx->stream, B, table + i0);
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      }));
  if (longest == 0) return KWY_OK;
  hipLaunchKernelGGL(k_pitch_window, dim3((H + KWY_THREADS - 1) / KWY_THREADS), dim3(KWY_THREADS), 0, ctx->stream, H, win);
  KWY_HIP(hipGetLastError());
  const size_t lds = sizeof(double) * (size_t)(4 * (H + 3) + 2 * H);
  KWY_PROF(ctx, "k_pitch_positions",
           hipLaunchKernelGGL(k_pitch_positions, dim3(count), dim3(KWY_THREADS), lds, ctx->stream, table, H));
  KWY_HIP(hipGetLastError());
  int64_t blocks = (longest + KWY_THREADS - 1) / KWY_THREADS;
  blocks = blocks > PITCH_X_BLOCKS ? PITCH_X_BLOCKS : blocks;
  KWY_PROF(ctx, "k_pitch_resample", hipLaunchKernelGGL(k_pitch_resample, dim3((unsigned)blocks, count), dim3(KWY_THREADS),
                                                       0, ctx->stream, table, H, win));
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

extern "C" int kwy_pitch_shift_batch_dev(kwy_ctx *ctx, const kwy_pitch_job *jobs, int count, int fs, double rate) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(pitch_check(ctx, jobs, count, fs, rate));
  KWY_HIP(hipSetDevice(ctx->device));
  KWY_TRY(kwy_arena_begin(ctx, pitch_bytes(jobs, count, fs, rate)));
  return pitch_run(ctx, jobs, count, fs, rate);
}

extern "C" int kwy_pitch_shift(kwy_ctx *ctx, const double *x, int64_t n, int fs, double rate, double *y,
                               int32_t *positions) {
  if (!ctx) return KWY_EINVAL;
  const kwy_pitch_job host = {x, n, y, positions};
  KWY_TRY(pitch_check(ctx, &host, 1, fs, rate));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "pitch_shift");
  kwy_pitch_job staged = host;
  st.in(staged.x, x, (size_t)n);
  st.out(staged.y, y, (size_t)n);
  st.out(staged.pos, positions, (size_t)kwy_pitch_frames(n, fs, rate));
  KWY_TRY(st.begin(pitch_bytes(&host, 1, fs, rate)));
  KWY_TRY(pitch_run(ctx, &staged, 1, fs, rate));
  return st.finish();
}
