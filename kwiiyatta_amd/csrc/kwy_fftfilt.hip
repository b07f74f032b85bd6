// kwy_fftfilt.hip -- frame-parallel FFT form of the differential mel-cepstral filter on gfx950.
//
// The MLSA filter of kwy_mlsa.hip is a time-varying IIR, serial in the sample: one wavefront per signal, however
// large the chip.  The filter it approximates, H(z) = exp sum_m c_m z~^-m (z~: the all-pass of alpha), has a closed
// frequency response, so a frame can be filtered by a transform of its own (overlap-save) and all frames of all
// signals run side by side.  Contract (include/kwy.h has it in full):
//   w~_k   = w_k + 2 atan2(alpha sin w_k, 1 - alpha cos w_k),  w_k = 2 pi k / N
//   H_i[k] = exp( sum_{m = m0 .. order} mc[i][m] e^{-j m w~_k} ),  k = 0 .. N/2
//   frame i < nproc = min(T, (n - 1) / hop):  X = rfft(x[(i+1) hop - N .. (i+1) hop)),  zeros before sample 0
//     a = irfft(X H_{max(i-1, 0)}), b = irfft(X H_i), the last hop samples of each
//     y[i hop + j] = (1 - j/hop) a_j + (j/hop) b_j
//   y[nproc hop ..] = 0
// One workgroup per (signal, frame) -- or per FF_TAIL samples of a signal's zero tail: every output sample has one
// writer, nothing is accumulated, the result does not depend on the launch it ran in.
//   * cos / sin of w~_k: one table per (N, alpha), kept with the context (built on the host on first use)
//   * e^{-j m w~_k}: the rotation recurrence from m = 0 upwards, the two frames' sums side by side on one rotation;
//     separate multiplications and additions in a fixed order (the library is built with -ffp-contract=off)
//   * one real transform in, two spectral products, two real transforms out: the LDS FFTs of kwy_fft.hpp, in two
//     buffers of N/2 + 1 complex
#include <math.h>
#include <stdio.h>

#include "kwy_internal.hpp"

#define FF_MAX_ORDER 62          // what kwy_mlsa_synthesis accepts
#define FF_JOBS_MAX 64           // signals per launch
#define FF_TAIL 16384            // samples of a zero tail per workgroup
#define FF_BLOCKS_MAX (1 << 30)  // workgroups per launch

struct ff_job {
  const double *x;    // n samples in
  const double *mc;   // T x (m + 1) mel-cepstra
  double *y;          // n samples out
  int64_t n, T;
};
typedef kwy_batch<ff_job, FF_JOBS_MAX> ff_jobs;
static_assert(sizeof(ff_jobs) + 48 <= KWY_KERNARG_MAX, "k_fft_filter: the table and seven scalar arguments");

static inline int64_t ff_nproc(int64_t n, int64_t T, int hop) {
  const int64_t f = (n - 1) / hop;
  return f < T ? f : T;
}
// workgroups of one signal: its processed frames, then its zero tail in pieces of FF_TAIL
static inline int64_t ff_blocks(int64_t n, int64_t T, int hop) {
  const int64_t np = ff_nproc(n, T, hop);
  return np + (n - np * hop + FF_TAIL - 1) / FF_TAIL;
}

template <int LOG2N>
__global__ __launch_bounds__(KWY_THREADS) void k_fft_filter(ff_jobs J, int m, int m0, int hop,
                                                           const kwy_c *__restrict__ warp,
                                                           const kwy_c *__restrict__ twH,
                                                           const kwy_c *__restrict__ twP,
                                                           const kwy_c *__restrict__ twN) {
  constexpr int N = 1 << LOG2N, H = N / 2, TWL = H / 8;
  extern __shared__ double smem[];
  kwy_c *bufA = (kwy_c *)smem;                // H + 1 complex: X H_prev -> a
  kwy_c *bufX = bufA + (H + 1);               // H + 1 complex: the frame -> X -> X H_cur -> b
  kwy_c *twl = bufX + (H + 1);                // exp(-2 pi i k / H), k < H/8
  double *smc = (double *)(twl + TWL);        // 2 x 64: the mel-cepstra of the frame before and of this frame
  const int tid = threadIdx.x;
  const int g = blockIdx.x;
  int u = 0;
  while (u + 1 < J.n && g >= J.start[u + 1]) ++u;   // uniform: a scalar loop
  const double *__restrict__ x = J.u[u].x;
  const double *__restrict__ mc = J.u[u].mc;
  double *__restrict__ y = J.u[u].y;
  const int64_t n = J.u[u].n, T = J.u[u].T;
  const int64_t i = g - J.start[u];
  int64_t nproc = (n - 1) / hop;
  if (nproc > T) nproc = T;
  if (i >= nproc) {                           // a piece of the zero tail
    const int64_t base = nproc * hop + (i - nproc) * FF_TAIL;
    for (int j = tid; j < FF_TAIL; j += KWY_THREADS)
      if (base + j < n) y[base + j] = 0.0;
    return;
  }
  // the N samples that end at (i + 1) hop  (< n: the frame is a processed one)
  const int64_t s = (i + 1) * hop - N;
  double *L = (double *)bufX;
  for (int j = tid; j < N; j += KWY_THREADS) {
    const int64_t p = s + j;
    L[j] = p >= 0 ? x[p] : 0.0;
  }
  for (int k = tid; k < TWL; k += KWY_THREADS) twl[k] = twH[k];
  if (tid < 128) {
    const int t = tid & 63;
    const int64_t fr = tid < 64 ? (i > 0 ? i - 1 : 0) : i;
    smc[tid] = (t <= m && t >= m0) ? mc[fr * (m + 1) + t] : 0.0;
  }
  const kwy_c twb = twN[tid];
  __syncthreads();
  kwy_rfft_inplace<LOG2N - 1, KWY_THREADS>(bufX, twl, twP, twb, twN);
  // the two responses of bin k and the two products
  for (int k = tid; k <= H; k += KWY_THREADS) {
    const kwy_c wd = warp[k];
    double c = 1.0, sn = 0.0;
    double re0 = 0.0, im0 = 0.0, re1 = 0.0, im1 = 0.0;
    for (int q = 0; q <= m; ++q) {
      const double c0 = smc[q], c1 = smc[64 + q];
      re0 += c0 * c; im0 -= c0 * sn;
      re1 += c1 * c; im1 -= c1 * sn;
      kwy_rotate(c, sn, wd.x, wd.y);
    }
    double s0, k0, s1, k1;
    kwy_sincos_medium(im0, &s0, &k0);
    kwy_sincos_medium(im1, &s1, &k1);
    const double g0 = exp(re0), g1 = exp(re1);
    const kwy_c X = bufX[k];
    bufA[k] = cmul(X, kwy_c{g0 * k0, g0 * s0});
    bufX[k] = cmul(X, kwy_c{g1 * k1, g1 * s1});
  }
  kwy_irfft_inplace<LOG2N - 1, KWY_THREADS>(bufA, twl, twP, twb, twN);
  kwy_irfft_inplace<LOG2N - 1, KWY_THREADS>(bufX, twl, twP, twb, twN);
  const double *A = (const double *)bufA + (N - hop), *B = (const double *)bufX + (N - hop);
  const double inv = 1.0 / N;
  double *yo = y + i * hop;
  for (int j = tid; j < hop; j += KWY_THREADS) {
    const double w = (double)j / (double)hop;
    yo[j] = (1.0 - w) * (A[j] * inv) + w * (B[j] * inv);
  }
}

// cos / sin of the warped frequencies w~_k, k <= N/2, per (N, alpha); exactly (+-1, 0) at k = 0 and N/2
static int ff_warp_table(kwy_ctx *ctx, int N, double alpha, const kwy_c **out) {
  char key[96];
  snprintf(key, sizeof(key), "fftfilt_warp:%d:%.17g", N, alpha);
  return kwy_cached_table<kwy_c>(ctx, key, [&] {
    const int H = N / 2;
    std::vector<kwy_c> h(H + 1);
    for (int k = 0; k <= H; ++k) {
      const double w = 2.0 * M_PI * (double)k / (double)N;
      const double wt = w + 2.0 * atan2(alpha * sin(w), 1.0 - alpha * cos(w));
      h[k].x = cos(wt);
      h[k].y = sin(wt);
    }
    h[0] = {1.0, 0.0};
    h[H] = {-1.0, 0.0};
    return h;
  }, out);
}

static bool ff_overlap(const double *a, const double *b, int64_t n) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b, len = (uintptr_t)n * sizeof(double);
  return pa < pb + len && pb < pa + len;
}

static int ff_check_common(kwy_ctx *ctx, int order, double alpha, int hop, int N) {
  if (!ctx) return KWY_EINVAL;
  if (order < 2 || order > FF_MAX_ORDER || !(fabs(alpha) < 1.0) || hop < 1 ||
      (N != 1024 && N != 2048 && N != 4096 && N != 8192) || N <= hop) {
    ctx->err = "mcep_filter_fft: bad argument (order 2..62, hopsize >= 1, fft_size 1024 | 2048 | 4096 | 8192 and > hopsize)";
    return KWY_EINVAL;
  }
  return KWY_OK;
}

static int ff_check_job(kwy_ctx *ctx, const double *x, int64_t n, const double *mc, int64_t T, int hop, const double *y) {
  if (!x || !mc || !y || n <= 0 || T <= 0) { ctx->err = "mcep_filter_fft: bad argument (null pointer or empty input)"; return KWY_EINVAL; }
  if (ff_overlap(x, y, n)) { ctx->err = "mcep_filter_fft: y must not alias x (a frame reads the input of the frames before it)"; return KWY_EINVAL; }
  if (ff_blocks(n, T, hop) > FF_BLOCKS_MAX) { ctx->err = "mcep_filter_fft: signal too long"; return KWY_EINVAL; }
  return KWY_OK;
}

template <int LOG2N>
static int ff_launch(kwy_ctx *ctx, const ff_jobs &J, int m, int m0, int hop, const kwy_c *warp) {
  constexpr int N = 1 << LOG2N, H = N / 2;
  const kwy_c *twH, *twN, *twP;
  KWY_TRY(kwy_get_twiddles(ctx, LOG2N - 1, &twH));
  KWY_TRY(kwy_get_twiddle_powers(ctx, LOG2N - 1, &twP));
  KWY_TRY(kwy_get_twiddles(ctx, LOG2N, &twN));
  const size_t lds = sizeof(kwy_c) * (2 * (H + 1) + H / 8) + sizeof(double) * 128;
  KWY_HIP(hipFuncSetAttribute((const void *)k_fft_filter<LOG2N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  KWY_PROF(ctx, "k_fft_filter", hipLaunchKernelGGL(k_fft_filter<LOG2N>, dim3((unsigned)J.start[J.n]), dim3(KWY_THREADS), lds,
                                                   ctx->stream, J, m, m0, hop, warp, twH, twP, twN));
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

static int ff_core(kwy_ctx *ctx, const ff_jobs &J, int m, int m0, int hop, int N, const kwy_c *warp) {
  if (J.start[J.n] == 0) return KWY_OK;
  switch (N) {
    case 1024: return ff_launch<10>(ctx, J, m, m0, hop, warp);
    case 2048: return ff_launch<11>(ctx, J, m, m0, hop, warp);
    case 4096: return ff_launch<12>(ctx, J, m, m0, hop, warp);
    default: return ff_launch<13>(ctx, J, m, m0, hop, warp);
  }
}

// the jobs in launches of <= FF_JOBS_MAX signals and <= FF_BLOCKS_MAX workgroups (all of them checked already): the
// second limit also ends a table, so this walk is its own and not kwy_for_tables
static int ff_run(kwy_ctx *ctx, const kwy_mlsa_job *jobs, int count, int order, double alpha, int hop, int N, int ignore_c0) {
  KWY_HIP(hipSetDevice(ctx->device));
  const kwy_c *warp;
  KWY_TRY(ff_warp_table(ctx, N, alpha, &warp));
  ff_jobs J{};
  for (int i = 0; i < count; ++i) {
    const kwy_mlsa_job &q = jobs[i];
    const int64_t nb = ff_blocks(q.x_length, q.T, hop);
    if (J.n == FF_JOBS_MAX || (int64_t)J.start[J.n] + nb > FF_BLOCKS_MAX) {
      KWY_TRY(ff_core(ctx, J, order, ignore_c0 ? 1 : 0, hop, N, warp));
      J = ff_jobs{};
    }
    J.u[J.n] = ff_job{q.x, q.mc, q.y, q.x_length, q.T};
    J.start[J.n + 1] = J.start[J.n] + (int)nb;
    ++J.n;
  }
  if (J.n) KWY_TRY(ff_core(ctx, J, order, ignore_c0 ? 1 : 0, hop, N, warp));
  return KWY_OK;
}

extern "C" int kwy_mcep_filter_fft_size(int fs, int hopsize) {
  if (fs < 1 || hopsize < 1) return 0;
  const int64_t need = (int64_t)hopsize + ((int64_t)fs + 39) / 40;   // hopsize + ceil(0.025 fs)
  int64_t p = 1024;
  while (p < need && p <= 8192) p *= 2;
  return p > 8192 ? 0 : (int)p;
}

extern "C" int kwy_mcep_filter_fft_batch_dev(kwy_ctx *ctx, const kwy_mlsa_job *jobs, int count, int order, double alpha,
                                             int hopsize, int fft_size, int ignore_c0) {
  KWY_TRY(ff_check_common(ctx, order, alpha, hopsize, fft_size));
  if (count == 0) return KWY_OK;
  if (!jobs || count < 0) { ctx->err = "mcep_filter_fft_batch: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i)
    KWY_TRY(ff_check_job(ctx, jobs[i].x, jobs[i].x_length, jobs[i].mc, jobs[i].T, hopsize, jobs[i].y));
  return ff_run(ctx, jobs, count, order, alpha, hopsize, fft_size, ignore_c0);
}

extern "C" int kwy_mcep_filter_fft_dev(kwy_ctx *ctx, const double *x, int64_t n, const double *mc, int64_t T, int order,
                                       double alpha, int hopsize, int fft_size, int ignore_c0, double *y) {
  KWY_TRY(ff_check_common(ctx, order, alpha, hopsize, fft_size));
  KWY_TRY(ff_check_job(ctx, x, n, mc, T, hopsize, y));
  const kwy_mlsa_job q = {x, n, mc, T, y};
  return ff_run(ctx, &q, 1, order, alpha, hopsize, fft_size, ignore_c0);
}

extern "C" int kwy_mcep_filter_fft(kwy_ctx *ctx, const double *x, int64_t n, const double *mc, int64_t T, int order,
                                   double alpha, int hopsize, int fft_size, int ignore_c0, double *y) {
  KWY_TRY(ff_check_common(ctx, order, alpha, hopsize, fft_size));
  KWY_TRY(ff_check_job(ctx, x, n, mc, T, hopsize, y));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "mcep_filter_fft");
  kwy_mlsa_job q = {x, n, mc, T, y};
  st.in(q.x, x, (size_t)n);
  st.out(q.y, y, (size_t)n);
  st.in(q.mc, mc, (size_t)T * (order + 1));
  KWY_TRY(st.begin());
  KWY_TRY(ff_run(ctx, &q, 1, order, alpha, hopsize, fft_size, ignore_c0));
  return st.finish();
}
