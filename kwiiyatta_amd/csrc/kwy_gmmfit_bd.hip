// kwy_gmmfit_bd.hip -- EM building blocks for a joint-density mixture whose covariances are block-diagonal in
// the sense of Toda, Black and Tokuda (2007): with z = [x | y], D = 2 h, the blocks Sxx, Syy, Sxy = Syx are
// diagonal, so pairing x_i with y_i leaves h independent 2 x 2 blocks [[a_i, c_i], [c_i, b_i]] per mixture
// (3 h numbers instead of D (D + 1) / 2).  covs_bd and sbd are M x 3 x h, laid out [a | b | c].
//
//   E:  k_bd_prec       per (mixture, pair): the 2 x 2 inverse [b, a, -c] / det and the means, the mixture's
//                       log-normaliser; flags a <= 0 or det <= 0                       (replicated, once per call)
//       k_bd_logprob    per 64-frame tile: the frames' rows staged in LDS once, the mixtures' precision forms
//                       passed through LDS 16 at a time; a lane owns a frame, a wavefront two mixtures of the
//                       chunk: log w + log N(z; mu_m, S_m) in the CENTRED form
//                       sum_i  P dx^2 + 2 R dx dy + Q dy^2,   dx = x_i - mux_i, dy = y_i - muy_i
//       k_fit_resp      (kwy_gmmfit.hip) log-sum-exp over the mixtures, responsibilities, log-likelihood parts
//   M:  k_bd_cov        per (row chunk, 8 mixtures, pair): sum_t r dx^2, sum_t r dy^2, sum_t r dx dy, then a
//                       reduction over the chunks in a fixed order (no atomics: bit-reproducible)
//       k_bd_finalize   weights, a = sa / nk + reg, b = sb / nk + reg, c = sc / nk
//       k_bd_expand     the M x D x D matrices the conversion reads
//   Sums and means are those of the full fit (kwy_gmm_em_sums_dev, kwy_gmm_em_means_dev).
//
// FP64 throughout; the products that feed a sum are written as fma() (the build runs with -ffp-contract=off).
// The centred form was taken over the expansion into one MFMA product over [x^2, xy, y^2, x, y]: it needs no
// second pass over X for a global mean, loses nothing to cancellation whatever the spread of the means, and at
// 8 operations per (frame, mixture, pair) it is 1.8e10 f64 operations for 5e5 x 144, M = 64: half a millisecond of
// the vector pipe, a twentieth of the full fit's E-step.
#include <math.h>

#include "kwy_internal.hpp"

#define BD_PREC 6          // doubles per (mixture, pair) of the precision form: P, Q, R, mux, muy, pad (16-byte rows)
#define BD_MC 16           // mixtures per LDS chunk in k_bd_logprob
#define BD_NT 512          // threads of k_bd_logprob: eight wavefronts
#define BD_MQ 2            // mixtures of the chunk per wavefront: w and w + 8
#define BD_TILE 64         // frames per tile: one per lane
#define BD_CQ 8            // mixtures per thread in k_bd_cov
static_assert(BD_MQ * (BD_NT / 64) == BD_MC, "the wavefronts of k_bd_logprob cover a chunk");

// prec[m][i] = {b/det, a/det, -c/det, mux, muy, 0}, cst[m] = log w - 0.5 (D log 2pi + sum_i log det_i).
// An unusable block (a <= 0 or det <= 0, NaN included) sets *status and is replaced by the unit block: what the
// later kernels compute from it is finite and is thrown away by the driver.
__global__ __launch_bounds__(KWY_THREADS) void k_bd_prec(const double *__restrict__ weights,
                                                        const double *__restrict__ means,
                                                        const double *__restrict__ covs_bd, int D,
                                                        double *__restrict__ prec, double *__restrict__ cst,
                                                        int *__restrict__ status) {
  __shared__ double ld[KWY_THREADS];
  const int h = D / 2, m = blockIdx.x, i = threadIdx.x;
  if (i < h) {
    const double *cb = covs_bd + (size_t)m * 3 * h;
    double a = cb[i], b = cb[h + i], c = cb[2 * h + i];
    double det = a * b - c * c;
    if (!(a > 0.0) || !(det > 0.0) || !(det < INFINITY)) {
      atomicExch(status, 1);
      a = 1.0; b = 1.0; c = 0.0; det = 1.0;
    }
    double *p = prec + ((size_t)m * h + i) * BD_PREC;
    p[0] = b / det;
    p[1] = a / det;
    p[2] = -c / det;
    p[3] = means[(size_t)m * D + i];
    p[4] = means[(size_t)m * D + h + i];
    p[5] = 0.0;
    ld[i] = log(det);
  }
  __syncthreads();
  if (i == 0) {
    double s = 0.0;
    for (int k = 0; k < h; ++k) s += ld[k];
    cst[m] = log(weights[m]) - 0.5 * (D * log(2.0 * KWY_PI) + s);
  }
}

// wlp[t][m] = cst[m] - 0.5 sum_i (P dx^2 + 2 R dx dy + Q dy^2).  Workgroups walk over the 64-frame tiles; a tile's
// rows go into LDS once (row stride D + 1 doubles: odd, so the lanes' 8-byte reads of one column fall on distinct
// banks) and serve all mixtures; the precision forms come through LDS in chunks of 16 mixtures (linear copies of
// `prec`, which the chip's L2 holds) and are read as broadcasts: two 16-byte and one 8-byte read per (mixture, pair)
// against eight f64 operations on 64 frames.  Eight wavefronts, two per SIMD (the LDS of one workgroup fills the CU):
// one computes while the other waits for its reads.
__global__ __launch_bounds__(BD_NT) void k_bd_logprob(const double *__restrict__ X, int64_t n, int D, int M,
                                                      const double *__restrict__ prec,
                                                      const double *__restrict__ cst, double *__restrict__ wlp) {
  extern __shared__ __align__(16) double bd_sm[];
  const int h = D / 2, S = D + 1;
  double *pr = bd_sm;                        // BD_MC x h x BD_PREC
  double *xs = pr + BD_MC * h * BD_PREC;     // BD_TILE x S
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t ntiles = (n + BD_TILE - 1) / BD_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t t0 = tile * BD_TILE;
    __syncthreads();                         // the previous tile's rows have been read
    for (int f = wv; f < BD_TILE; f += BD_NT / 64) {
      const double *row = X + min(t0 + f, n - 1) * D;       // rows behind the last one repeat it; never stored
      for (int c = lane; c < D; c += 64) xs[f * S + c] = row[c];
    }
    const double *xl = xs + lane * S;
    const int64_t t = t0 + lane;
    for (int c0 = 0; c0 < M; c0 += BD_MC) {
      const int cnt = min(BD_MC, M - c0);
      __syncthreads();                       // rows staged; the previous chunk has been read
      const double *src = prec + (size_t)c0 * h * BD_PREC;
      for (int e = tid; e < cnt * h * BD_PREC; e += BD_NT) pr[e] = src[e];
      __syncthreads();
      int ml[BD_MQ];
      const double *pm[BD_MQ];
      double q[BD_MQ];
#pragma unroll
      for (int j = 0; j < BD_MQ; ++j) {
        ml[j] = wv + (BD_NT / 64) * j;
        pm[j] = pr + (size_t)min(ml[j], cnt - 1) * h * BD_PREC;   // beyond the chunk: a copy of its last, not stored
        q[j] = 0.0;
      }
#pragma unroll 2
      for (int i = 0; i < h; ++i) {
        const double x = xl[i], y = xl[h + i];
#pragma unroll
        for (int j = 0; j < BD_MQ; ++j) {
          const double2 *p = (const double2 *)(pm[j] + i * BD_PREC);
          const double2 pq = p[0], rm = p[1];
          const double muy = pm[j][i * BD_PREC + 4];
          const double dx = x - rm.y, dy = y - muy;
          const double u = fma(pq.x, dx, rm.x * dy);      // P dx + R dy
          const double v = fma(pq.y, dy, rm.x * dx);      // Q dy + R dx
          q[j] = fma(dx, u, q[j]);
          q[j] = fma(dy, v, q[j]);
        }
      }
      if (t < n) {
#pragma unroll
        for (int j = 0; j < BD_MQ; ++j)
          if (ml[j] < cnt) wlp[t * M + c0 + ml[j]] = cst[c0 + ml[j]] - 0.5 * q[j];
      }
    }
  }
}

// part[chunk][m][k][i], k = 0, 1, 2: sum over the chunk's rows of r dx^2, r dy^2, r dx dy around `means`.
// Thread e of a chunk owns pair i = e % h and the mixtures 8 (e / h) .. + 7: per frame two coalesced loads of X,
// the eight responsibilities (one address per group of mixtures: a broadcast) and 64 f64 operations.  No barrier.
// (Staging the rows and the responsibilities through LDS, 32 frames at a time, was measured and is no faster: 1.76 ms
// against 1.60 ms at 5e5 x 144, M = 64.)
__global__ __launch_bounds__(KWY_THREADS) void k_bd_cov(const double *__restrict__ X, const double *__restrict__ resp,
                                                       int64_t n, int D, int M, int rows_per_chunk,
                                                       const double *__restrict__ means, double *__restrict__ part) {
  const int h = D / 2;
  const int e = blockIdx.y * blockDim.x + threadIdx.x;
  const int ng = (M + BD_CQ - 1) / BD_CQ;
  if (e >= ng * h) return;
  const int g = e / h, i = e % h, m0 = BD_CQ * g;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk, r1 = min(n, r0 + rows_per_chunk);
  int mj[BD_CQ];
  double mux[BD_CQ], muy[BD_CQ], sa[BD_CQ], sb[BD_CQ], sc[BD_CQ];
#pragma unroll
  for (int j = 0; j < BD_CQ; ++j) {
    mj[j] = min(m0 + j, M - 1);              // beyond M: a copy of the last mixture, not stored
    mux[j] = means[(size_t)mj[j] * D + i];
    muy[j] = means[(size_t)mj[j] * D + h + i];
    sa[j] = sb[j] = sc[j] = 0.0;
  }
  const bool vec = (M % BD_CQ) == 0 && ((uintptr_t)resp & 15) == 0;     // rows of resp in 64-byte steps: 16-byte loads
#pragma unroll 2
  for (int64_t t = r0; t < r1; ++t) {
    const double x = X[t * D + i], y = X[t * D + h + i];
    double r[BD_CQ];
    if (vec) {
      const double2 *rp = (const double2 *)(resp + t * M + m0);
#pragma unroll
      for (int j = 0; j < BD_CQ / 2; ++j) {
        const double2 v = rp[j];
        r[2 * j] = v.x;
        r[2 * j + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < BD_CQ; ++j) r[j] = resp[t * M + mj[j]];
    }
#pragma unroll
    for (int j = 0; j < BD_CQ; ++j) {
      const double dx = x - mux[j], dy = y - muy[j];
      const double rx = r[j] * dx;
      sa[j] = fma(rx, dx, sa[j]);
      sc[j] = fma(rx, dy, sc[j]);
      sb[j] = fma(r[j] * dy, dy, sb[j]);
    }
  }
  double *out = part + (size_t)blockIdx.x * M * 3 * h;
#pragma unroll
  for (int j = 0; j < BD_CQ; ++j)
    if (m0 + j < M) {
      double *o = out + (size_t)(m0 + j) * 3 * h + i;
      o[0] = sa[j];
      o[h] = sb[j];
      o[2 * h] = sc[j];
    }
}

// out[e] = sum_c part[c][e], chunks in ascending order
__global__ void k_bd_reduce(const double *__restrict__ part, int nchunks, int64_t len, double *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= len) return;
  double s = 0.0;
  for (int c = 0; c < nchunks; ++c) s += part[(size_t)c * len + e];
  out[e] = s;
}

// weights = nk / sum nk (as k_fit_finalize); covs_bd = sbd / nk, reg on a and b
__global__ void k_bd_finalize(const double *__restrict__ stats, const double *__restrict__ sbd, int D, int M,
                              double reg, double *__restrict__ weights, double *__restrict__ covs_bd) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int h = D / 2;
  if (e < M) {
    double tot = 0.0;
    for (int k = 0; k < M; ++k) tot += stats[(size_t)k * (D + 1)] + 10 * 2.220446049250313e-16;
    weights[e] = (stats[(size_t)e * (D + 1)] + 10 * 2.220446049250313e-16) / tot;
  }
  if (e >= M * 3 * h) return;
  const int m = e / (3 * h), k = (e % (3 * h)) / h;
  const double nk = stats[(size_t)m * (D + 1)] + 10 * 2.220446049250313e-16;
  double v = sbd[e] / nk;
  if (k < 2) v += reg;
  covs_bd[e] = v;
}

// covs[m][r][c]: a on the diagonal of the xx block, b on that of the yy block, c on those of xy and yx, +0.0 elsewhere
__global__ void k_bd_expand(const double *__restrict__ covs_bd, int D, int M, double *__restrict__ covs) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)M * D * D) return;
  const int h = D / 2;
  const int m = (int)(e / ((int64_t)D * D));
  const int rem = (int)(e % ((int64_t)D * D));
  const int r = rem / D, c = rem % D;
  const double *cb = covs_bd + (size_t)m * 3 * h;
  double v = 0.0;
  if (r == c) v = r < h ? cb[r] : cb[h + (r - h)];
  else if (c == r + h) v = cb[2 * h + r];
  else if (r == c + h) v = cb[2 * h + c];
  covs[e] = v;
}

// ---- C ABI ------------------------------------------------------------------------------------------
static int bd_check(kwy_ctx *ctx, int64_t n, int D, int M) {
  if (!ctx) return KWY_EINVAL;
  if (n < 1 || D < 2 || D > 160 || (D & 1) || M < 1 || M > 256) {
    ctx->err = "gmm_em_bd: need n >= 1, an even D with 2 <= D <= 160 and 1 <= M <= 256";
    return KWY_EINVAL;
  }
  return KWY_OK;
}

// frames per workgroup of k_bd_cov: about 1024 chunks, at least 256 frames each
static int bd_cov_rows(int64_t n) {
  const int64_t r = (n + 1023) / 1024;
  return (int)(r < 256 ? 256 : r);
}

extern "C" int kwy_gmm_em_estep_bd_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, int M, const double *weights,
                                       const double *means, const double *covs_bd, double *resp, double *loglik_parts,
                                       int *status_out) {
  KWY_TRY(bd_check(ctx, n, D, M));
  if (!X || !weights || !means || !covs_bd || !resp || !loglik_parts || !status_out) {
    ctx->err = "gmm_em_estep_bd: null pointer";
    return KWY_EINVAL;
  }
  KWY_HIP(hipSetDevice(ctx->device));
  const int h = D / 2;
  const size_t nprec = (size_t)M * h * BD_PREC;
  KWY_TRY(kwy_arena_begin(ctx, kwy_pad(sizeof(double) * nprec) + kwy_pad(sizeof(double) * M)));
  double *prec = kwy_arena<double>(ctx, nprec);
  double *cst = kwy_arena<double>(ctx, M);
  if (!prec || !cst) { ctx->err = "gmm_em_estep_bd: scratch"; return KWY_ENOMEM; }
  KWY_HIP(hipMemsetAsync(status_out, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_bd_prec, dim3(M), dim3(KWY_THREADS), 0, ctx->stream, weights, means, covs_bd, D, prec, cst,
                     status_out);
  const size_t lds = sizeof(double) * ((size_t)BD_MC * h * BD_PREC + (size_t)BD_TILE * (D + 1));
  KWY_HIP(hipFuncSetAttribute((const void *)k_bd_logprob, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t ntiles = (n + BD_TILE - 1) / BD_TILE;
  const unsigned grid = (unsigned)(ntiles < 2048 ? ntiles : 2048);
  KWY_PROF(ctx, "k_bd_logprob", hipLaunchKernelGGL(k_bd_logprob, dim3(grid), dim3(BD_NT), lds, ctx->stream, X, n, D, M, prec, cst, resp));
  KWY_HIP(hipGetLastError());
  return kwy_fit_resp(ctx, resp, n, M, loglik_parts);
}

extern "C" int kwy_gmm_em_cov_bd_dev(kwy_ctx *ctx, const double *X, int64_t n, int D, int M, const double *resp,
                                     const double *means, const double *stats, double *sbd) {
  KWY_TRY(bd_check(ctx, n, D, M));
  if (!X || !resp || !means || !sbd) { ctx->err = "gmm_em_cov_bd: null pointer"; return KWY_EINVAL; }
  (void)stats;      // every frame is summed: the sums cost what the test for skipping them would
  KWY_HIP(hipSetDevice(ctx->device));
  const int h = D / 2;
  const int rows = bd_cov_rows(n);
  const int nchunks = (int)((n + rows - 1) / rows);
  const int64_t len = (int64_t)M * 3 * h;
  KWY_TRY(kwy_arena_begin(ctx, kwy_pad(sizeof(double) * (size_t)nchunks * len)));
  double *part = kwy_arena<double>(ctx, (size_t)nchunks * len);
  if (!part) { ctx->err = "gmm_em_cov_bd: scratch"; return KWY_ENOMEM; }
  // wavefronts over the (mixture group, pair) items of a chunk, three or four to a workgroup, whichever leaves
  // fewer idle (D = 144, M = 64: 576 items = 9 wavefronts = 3 workgroups of 3)
  const int items = ((M + BD_CQ - 1) / BD_CQ) * h;
  const int nw = (items + 63) / 64;
  const int wpb = nw < 4 ? nw : ((nw % 4) && !(nw % 3)) ? 3 : 4;
  KWY_PROF(ctx, "k_bd_cov", hipLaunchKernelGGL(k_bd_cov, dim3(nchunks, (nw + wpb - 1) / wpb), dim3(64 * wpb), 0, ctx->stream, X, resp, n, D, M, rows, means, part));
  hipLaunchKernelGGL(k_bd_reduce, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, ctx->stream, part, nchunks, len,
                     sbd);
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

extern "C" int kwy_gmm_em_finalize_bd_dev(kwy_ctx *ctx, const double *stats, const double *sbd, int D, int M,
                                          double reg_covar, double *weights, double *covs_bd) {
  KWY_TRY(bd_check(ctx, 1, D, M));
  if (!stats || !sbd || !weights || !covs_bd) { ctx->err = "gmm_em_finalize_bd: null pointer"; return KWY_EINVAL; }
  KWY_HIP(hipSetDevice(ctx->device));
  const int len = M * 3 * (D / 2);
  hipLaunchKernelGGL(k_bd_finalize, dim3((unsigned)(((len > M ? len : M) + 255) / 256)), dim3(256), 0, ctx->stream,
                     stats, sbd, D, M, reg_covar, weights, covs_bd);
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

extern "C" int kwy_gmm_expand_bd_dev(kwy_ctx *ctx, const double *covs_bd, int D, int M, double *covs) {
  KWY_TRY(bd_check(ctx, 1, D, M));
  if (!covs_bd || !covs) { ctx->err = "gmm_expand_bd: null pointer"; return KWY_EINVAL; }
  KWY_HIP(hipSetDevice(ctx->device));
  const int64_t len = (int64_t)M * D * D;
  hipLaunchKernelGGL(k_bd_expand, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, ctx->stream, covs_bd, D, M, covs);
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}
