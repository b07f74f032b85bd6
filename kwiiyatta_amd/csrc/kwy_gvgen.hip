// kwy_gvgen.hip -- parameter generation considering the global variance (Toda, Black and Tokuda 2007, section IV) on gfx950.
//
// The arithmetic is the contract of kwy_gv_ascent in include/kwy.h: per (utterance, static dimension) a fixed number
// of nonlinear conjugate-gradient steps (Polak-Ribiere+, exact line search) on
//     Q(y) = w (-1/2 y'P y + b'y) - 1/2 weight (v(y) - mu)^2 / sigma^2,     w = 1 / (3 T)
// from the linearly scaled maximum-likelihood track.  There is no reference call to cite: the reference synthesises the
// converter's output as it is (kwiiyatta/convert_voice.py:35-46).
//
// Kernels:
//   k_gv_ascent   one workgroup of GVA_NT threads per (utterance, dimension), all iterations inside.  Thread i owns the
//                 rows i, i + GVA_NT, ...: consecutive lanes consecutive rows, so the tracks' LDS accesses are free of
//                 bank conflicts and the records of a row are two 16-byte loads.  Three tracks (y, the direction p, the
//                 previous gradient) live in LDS with two zero rows before and after, so the band product needs no edge
//                 case.  Up to GVA_REG_ROWS rows per thread keep their six band values and the offset in registers
//                 (T <= 2048); longer tracks stream the records from L2 in every pass; tracks beyond GVA_LDS_ROWS rows
//                 live in global scratch.  The three forms run the same arithmetic in the same order.
//                 Reductions: a thread adds its rows in ascending order, a wavefront folds by a butterfly (every lane
//                 ends with the same bits), the four wavefronts' sums are added in wavefront order by every thread.
//                 All scalars of the iteration are therefore uniform without a broadcast, and so is the control flow.
//   k_gv_fold     per utterance: Q_k summed over the dimensions in ascending order, the status word
//   k_gv_stats    mean and variance over the utterances of the per-utterance variance, one lane per column
//
// No grid-wide synchronisation, no atomics: the columns are independent.  The _dev entries take their scratch from
// the context's arena and do not synchronise.
#include <math.h>

#include <algorithm>
#include <vector>

#include "kwy_internal.hpp"

#define GVA_NT 256
#define GVA_REG_ROWS 8       // rows per thread whose records stay in registers: T <= GVA_NT * GVA_REG_ROWS
#define GVA_LDS_ROWS 6800    // 3 tracks of T + 4 doubles + GVA_RED doubles of reduction scratch <= 160 KB
#define GVA_NS 5             // sums of the widest reduction
#define GVA_RED (2 * (GVA_NT / 64) * GVA_NS + 8)   // two buffers, used in turn: one barrier per reduction
#define GVA_MAX_COLS 64

struct gva_job {
  const double *band;
  const double *off;
  double *y;
  int64_t T;
  int ldy, ldo;
  double *work;            // d x (iterations + 2): Q_0 .. Q_N of the column, then 1.0 if the column is unusable
  double *tracks;          // d x 3 x (T + 4) doubles where T > GVA_LDS_ROWS, else null
  double *objective;
  int32_t *status;
};
typedef kwy_group<gva_job, KWY_BATCH_MAX> gva_jobs;

// the butterfly leaves the same bits in every lane (a + b == b + a)
__device__ __forceinline__ double gva_wave_sum(double s) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

template <int NS>
__device__ __forceinline__ void gva_reduce(double (&s)[NS], double *red, int &phase) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double *buf = red + phase * (GVA_NT / 64) * GVA_NS;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const double w = gva_wave_sum(s[i]);
    if (lane == 0) buf[wave * GVA_NS + i] = w;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    double a = buf[i];
#pragma unroll
    for (int w = 1; w < GVA_NT / 64; ++w) a += buf[w * GVA_NS + i];
    s[i] = a;
  }
  phase ^= 1;
}

// the smallest positive root of c3 a^3 + c2 a^2 + c1 a + c0 with c0 > 0 and c3 <= 0, or -1: the stationary points cut
// the half line into monotone pieces, the first piece with a sign change is narrowed by Newton steps kept inside a
// bisection bracket
__device__ double gva_root(double c0, double c1, double c2, double c3) {
  if (!(c0 > 0.0)) return -1.0;
  if (c3 == 0.0 && c2 == 0.0) return c1 < 0.0 ? -c0 / c1 : -1.0;
  if (!(c3 < 0.0)) return -1.0;
  auto f = [&](double a) { return ((c3 * a + c2) * a + c1) * a + c0; };
  auto df = [&](double a) { return (3.0 * c3 * a + 2.0 * c2) * a + c1; };
  double e[2];
  int ne = 0;
  const double disc = c2 * c2 - 3.0 * c3 * c1;
  if (disc > 0.0) {
    const double sq = sqrt(disc);
    const double qq = -(c2 + (c2 < 0.0 ? -sq : sq));
    const double e1 = qq / (3.0 * c3);
    const double e2 = qq != 0.0 ? c1 / qq : e1;
    const double lo_ = e1 < e2 ? e1 : e2, hi_ = e1 < e2 ? e2 : e1;
    if (lo_ > 0.0) e[ne++] = lo_;
    if (hi_ > 0.0 && hi_ != lo_) e[ne++] = hi_;
  }
  double lo = 0.0, hi = -1.0;
  for (int i = 0; i < ne; ++i) {
    if (f(e[i]) <= 0.0) { hi = e[i]; break; }
    lo = e[i];
  }
  if (hi < 0.0) {   // beyond the last stationary point the cubic falls monotonically: widen until it is <= 0
    double h = lo > 0.0 ? lo : (c1 < 0.0 ? -c0 / c1 : 1.0);
    hi = lo + h;
    int it = 0;
    while (f(hi) > 0.0) {
      if (++it > 2100 || !(hi <= KWY_DBL_MAX)) return -1.0;
      lo = hi;
      h *= 2.0;
      hi = lo + h;
    }
  }
  double x = 0.5 * (lo + hi);
  for (int it = 0; it < 200; ++it) {
    const double fx = f(x);
    if (fx > 0.0) lo = x; else hi = x;
    double xn = x - fx / df(x);
    if (!(xn > lo && xn < hi)) {
      xn = 0.5 * (lo + hi);
      if (!(xn > lo && xn < hi)) break;
    }
    if (xn == x) break;
    x = xn;
  }
  return x;
}

template <bool REG, bool LDSTRK>
__global__ __launch_bounds__(GVA_NT) void k_gv_ascent(gva_jobs J, int d, const double *__restrict__ gv_mean,
                                                       const double *__restrict__ gv_var, double weight, int N) {
  extern __shared__ __attribute__((aligned(16))) char gva_smem[];
  const gva_job &U = J.u[blockIdx.y];
  // a launch holds the jobs of one form; the others' workgroups leave at once
  const bool reg = U.T <= GVA_NT * GVA_REG_ROWS, ldstrk = U.T <= GVA_LDS_ROWS;
  if (reg != REG || ldstrk != LDSTRK) return;
  const int c = blockIdx.x, tid = threadIdx.x, T = (int)U.T;
  double *qo = U.work + (size_t)c * (N + 2);
  const double mu = gv_mean[c], var = gv_var[c];
  auto leave = [&](double flag) {
    for (int k = tid; k <= N; k += GVA_NT) qo[k] = 0.0;
    if (tid == 0) qo[N + 1] = flag;
  };
  if (!(mu > 0.0 && mu <= KWY_DBL_MAX && var > 0.0 && var <= KWY_DBL_MAX)) { leave(1.0); return; }

  double *red = (double *)gva_smem;
  double *trk = LDSTRK ? red + GVA_RED : U.tracks + (size_t)c * 3 * ((size_t)T + 4);
  double *yt = trk + 2, *pt = trk + (T + 4) + 2, *gt = trk + 2 * (T + 4) + 2;
  const double *band = U.band;
  const double *off = U.off;
  int phase = 0;

  // the values of row t: P[t][t], P[t][t-1], P[t][t-2], b[t], P[t+1][t], P[t+2][t], s[t]
  auto fetch = [&](int t, double &p0, double &p1, double &p2, double &b, double &u1, double &u2, double &s) {
    const double2 *r = (const double2 *)band + ((int64_t)t * d + c) * 2;
    const double2 a = r[0], bb = r[1];
    p0 = a.x;
    p1 = t >= 1 ? a.y : 0.0;
    p2 = t >= 2 ? bb.x : 0.0;
    b = bb.y;
    u1 = t + 1 < T ? ((const double *)band)[((int64_t)(t + 1) * d + c) * 4 + 1] : 0.0;
    u2 = t + 2 < T ? ((const double *)band)[((int64_t)(t + 2) * d + c) * 4 + 2] : 0.0;
    s = off ? off[(int64_t)t * U.ldo + c] : 0.0;
  };
  double q0[GVA_REG_ROWS], q1[GVA_REG_ROWS], q2[GVA_REG_ROWS], qb[GVA_REG_ROWS], qu1[GVA_REG_ROWS],
      qu2[GVA_REG_ROWS], qs[GVA_REG_ROWS];
  if (REG) {
#pragma unroll
    for (int k = 0; k < GVA_REG_ROWS; ++k) {
      const int t = tid + k * GVA_NT;
      q0[k] = q1[k] = q2[k] = qb[k] = qu1[k] = qu2[k] = qs[k] = 0.0;
      if (t < T) fetch(t, q0[k], q1[k], q2[k], qb[k], qu1[k], qu2[k], qs[k]);
    }
  }
  // body(t, p0, p1, p2, b, u1, u2, s) for the thread's rows in ascending order
  auto rows = [&](auto body) {
    if (REG) {
#pragma unroll
      for (int k = 0; k < GVA_REG_ROWS; ++k) {
        const int t = tid + k * GVA_NT;
        if (t < T) body(t, q0[k], q1[k], q2[k], qb[k], qu1[k], qu2[k], qs[k]);
      }
    } else {
      for (int t = tid; t < T; t += GVA_NT) {
        double p0, p1, p2, b, u1, u2, s;
        fetch(t, p0, p1, p2, b, u1, u2, s);
        body(t, p0, p1, p2, b, u1, u2, s);
      }
    }
  };

  if (tid < 2) {
    yt[-2 + tid] = 0.0; yt[T + tid] = 0.0;
    pt[-2 + tid] = 0.0; pt[T + tid] = 0.0;
  }
  for (int t = tid; t < T; t += GVA_NT) yt[t] = U.y[(int64_t)t * U.ldy + c];
  __syncthreads();

  const double omega = 1.0 / (3.0 * (double)T), dT = (double)T;
  // Q and its parts at x (+ alpha p): the quadratic form, the linear term, the mean and the variance of x + s
  auto evaluate = [&](const double *x, bool step, double alpha, double &zbar, double &v) {
    double s3[3] = {0.0, 0.0, 0.0};
    rows([&](int t, double p0, double p1, double p2, double b, double u1, double u2, double s) {
      double xm2 = x[t - 2], xm1 = x[t - 1], x0 = x[t], xp1 = x[t + 1], xp2 = x[t + 2];
      if (step) {
        xm2 = xm2 + alpha * pt[t - 2]; xm1 = xm1 + alpha * pt[t - 1]; x0 = x0 + alpha * pt[t];
        xp1 = xp1 + alpha * pt[t + 1]; xp2 = xp2 + alpha * pt[t + 2];
      }
      const double px = p0 * x0 + p1 * xm1 + p2 * xm2 + u1 * xp1 + u2 * xp2;
      s3[0] += x0 * px;
      s3[1] += b * x0;
      s3[2] += x0 + s;
    });
    gva_reduce(s3, red, phase);
    zbar = s3[2] / dT;
    double s1[1] = {0.0};
    rows([&](int t, double, double, double, double, double, double, double s) {
      const double x0 = step ? x[t] + alpha * pt[t] : x[t];
      const double zc = x0 + s - zbar;
      s1[0] += zc * zc;
    });
    gva_reduce(s1, red, phase);
    v = s1[0] / dT;
    return omega * (-0.5 * s3[0] + s3[1]) - 0.5 * weight * ((v - mu) * (v - mu)) / var;
  };

  double zbar, v;
  double Q = evaluate(yt, false, 0.0, zbar, v);
  if (!kwy_finite_nonneg(v)) { leave(1.0); return; }
  if (v == 0.0) { leave(0.0); return; }
  {
    const double a = sqrt(mu / v);
    rows([&](int t, double, double, double, double, double, double, double s) {
      pt[t] = a * (yt[t] + s - zbar) + zbar - s;
    });
    __syncthreads();
    double zbar0, v0;
    const double Q0 = evaluate(pt, false, 0.0, zbar0, v0);
    if (Q0 >= Q) {
      rows([&](int t, double, double, double, double, double, double, double) { yt[t] = pt[t]; });
      Q = Q0; zbar = zbar0; v = v0;
    }
    __syncthreads();
  }
  if (tid == 0) qo[0] = Q;

  double gg_prev = 0.0;
  bool frozen = false;
  for (int k = 1; k <= N; ++k) {
    if (!frozen) {
      const bool first = k == 1;
      const double cg = weight * (v - mu) / var * (2.0 / dT);
      double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};    // g.g, g.(g - g_prev), g.r, p_prev.r, g.p_prev
      rows([&](int t, double p0, double p1, double p2, double b, double u1, double u2, double s) {
        const double y0 = yt[t];
        const double py = p0 * y0 + p1 * yt[t - 1] + p2 * yt[t - 2] + u1 * yt[t + 1] + u2 * yt[t + 2];
        const double r = b - py;
        const double g = omega * r - cg * (y0 + s - zbar);
        const double go = first ? 0.0 : gt[t], po = first ? 0.0 : pt[t];
        s5[0] += g * g;
        s5[1] += g * (g - go);
        s5[2] += g * r;
        s5[3] += po * r;
        s5[4] += g * po;
        gt[t] = g;
      });
      gva_reduce(s5, red, phase);
      const double gg = s5[0];
      double beta = 0.0;
      if (!first && gg_prev > 0.0) {
        const double pr = s5[1] / gg_prev;
        beta = pr > 0.0 ? pr : 0.0;
      }
      double gp = gg + beta * s5[4];
      if (!(gp > 0.0)) { beta = 0.0; gp = gg; }
      if (!kwy_finite_pos(gp)) {
        frozen = true;
      } else {
        const double pr = s5[2] + beta * s5[3];      // p.(b - P y)
        double s1[1] = {0.0};
        rows([&](int t, double, double, double, double, double, double, double) {
          const double g = gt[t];
          const double p = beta == 0.0 ? g : g + beta * pt[t];
          pt[t] = p;
          s1[0] += p;
        });
        gva_reduce(s1, red, phase);
        const double pbar = s1[0] / dT;
        double s3[3] = {0.0, 0.0, 0.0};              // p'P p, sum (z - zbar)(p - pbar), sum (p - pbar)^2
        rows([&](int t, double p0, double p1, double p2, double, double u1, double u2, double s) {
          const double x0 = pt[t];
          const double pp = p0 * x0 + p1 * pt[t - 1] + p2 * pt[t - 2] + u1 * pt[t + 1] + u2 * pt[t + 2];
          const double pc = x0 - pbar;
          s3[0] += x0 * pp;
          s3[1] += (yt[t] + s - zbar) * pc;
          s3[2] += pc * pc;
        });
        gva_reduce(s3, red, phase);
        const double cov = s3[1] / dT, vp = s3[2] / dT, kap = weight / var, e = v - mu;
        const double c0 = omega * pr - 2.0 * kap * e * cov;
        const double c1 = -omega * s3[0] - kap * (4.0 * cov * cov + 2.0 * e * vp);
        const double c2 = -6.0 * kap * cov * vp;
        const double c3 = -2.0 * kap * vp * vp;
        const double alpha = gva_root(c0, c1, c2, c3);
        if (!kwy_finite_pos(alpha)) {
          frozen = true;
        } else {
          double zbar1, v1;
          const double Q1 = evaluate(yt, true, alpha, zbar1, v1);
          if (Q1 >= Q) {
            rows([&](int t, double, double, double, double, double, double, double) {
              yt[t] = yt[t] + alpha * pt[t];
            });
            Q = Q1; zbar = zbar1; v = v1; gg_prev = gg;
            __syncthreads();
          } else {
            frozen = true;
          }
        }
      }
    }
    if (tid == 0) qo[k] = Q;
  }
  if (tid == 0) qo[N + 1] = 0.0;
  for (int t = tid; t < T; t += GVA_NT) U.y[(int64_t)t * U.ldy + c] = yt[t];
}

__global__ __launch_bounds__(GVA_NT) void k_gv_fold(gva_jobs J, int d, int N) {
  const gva_job &U = J.u[blockIdx.x];
  for (int k = threadIdx.x; k <= N; k += GVA_NT) {
    if (!U.objective) break;
    double s = 0.0;
    for (int c = 0; c < d; ++c) s += U.work[(size_t)c * (N + 2) + k];
    U.objective[k] = s;
  }
  if (threadIdx.x == 0 && U.status) {
    int bad = 0;
    for (int c = 0; c < d; ++c) bad += U.work[(size_t)c * (N + 2) + N + 1] != 0.0 ? 1 : 0;
    *U.status = bad;
  }
}

// mean[c], var[c] of M2 / n over the matrices with n > 0: two passes, left folds in index order
__global__ __launch_bounds__(GVA_MAX_COLS) void k_gv_stats(const double *__restrict__ m, int count, int cols,
                                                           double *__restrict__ mean, double *__restrict__ var) {
  const int c = threadIdx.x;
  if (c >= cols) return;
  double sum = 0.0, used = 0.0;
  for (int i = 0; i < count; ++i) {
    const double *t = m + 3 * ((int64_t)i * cols + c);
    if (t[0] > 0.0) {
      sum += t[2] / t[0];
      used += 1.0;
    }
  }
  const double mn = used > 0.0 ? sum / used : 0.0;
  double s2 = 0.0;
  for (int i = 0; i < count; ++i) {
    const double *t = m + 3 * ((int64_t)i * cols + c);
    if (t[0] > 0.0) {
      const double dv = t[2] / t[0] - mn;
      s2 += dv * dv;
    }
  }
  mean[c] = mn;
  var[c] = used > 1.0 ? s2 / used : 0.0;
}

// ---- host side ------------------------------------------------------------------------------------------
static size_t gva_lds_bytes(int64_t T) { return sizeof(double) * (GVA_RED + 3 * ((size_t)T + 4)); }

size_t kwy_gva_scratch_bytes(const int64_t *T, int n, int d, int iterations) {
  size_t bytes = 0;
  for (int j = 0; j < n; ++j) {
    bytes += kwy_pad(sizeof(double) * (size_t)d * (iterations + 2));
    if (T[j] > GVA_LDS_ROWS) bytes += kwy_pad(sizeof(double) * (size_t)d * 3 * ((size_t)T[j] + 4));
  }
  return bytes;
}

template <bool REG, bool LDSTRK>
static int gva_launch_form(kwy_ctx *ctx, const gva_jobs &J, int d, const double *gv_mean, const double *gv_var,
                           double weight, int N, int64_t Tmax) {
  const size_t lds = LDSTRK ? gva_lds_bytes(Tmax) : sizeof(double) * GVA_RED;
  KWY_HIP(hipFuncSetAttribute((const void *)k_gv_ascent<REG, LDSTRK>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds));
  KWY_PROF(ctx, "k_gv_ascent", hipLaunchKernelGGL((k_gv_ascent<REG, LDSTRK>), dim3(d, J.n), dim3(GVA_NT), lds,
                                                 ctx->stream, J, d, gv_mean, gv_var, weight, N));
  return KWY_OK;
}

int kwy_gva_launch(kwy_ctx *ctx, const kwy_gva_view *v, int n, int d, const double *gv_mean, const double *gv_var,
                   double weight, int iterations) {
  const auto form = [](int64_t T) { return T <= GVA_NT * GVA_REG_ROWS ? 0 : (T <= GVA_LDS_ROWS ? 1 : 2); };
  return kwy_for_tables<gva_jobs>(
      n,
      [&](int j) {
        gva_job q{v[j].band, v[j].offset, v[j].y, v[j].T, v[j].ldy, v[j].ldo, nullptr, nullptr, v[j].objective,
                  v[j].status};
        q.work = kwy_arena<double>(ctx, (size_t)d * (iterations + 2));
        if (form(q.T) == 2) q.tracks = kwy_arena<double>(ctx, (size_t)d * 3 * ((size_t)q.T + 4));
        return q;
      },
      [&](const gva_jobs &J, int) {
        int64_t tmax[3] = {0, 0, 0};
        for (int j = 0; j < J.n; ++j) {
          const gva_job &q = J.u[j];
          if (!q.work || (form(q.T) == 2 && !q.tracks)) { ctx->err = "gv_ascent: scratch arena too small"; return KWY_ENOMEM; }
          tmax[form(q.T)] = std::max(tmax[form(q.T)], q.T);
        }
        if (tmax[0] > 0) KWY_TRY((gva_launch_form<true, true>(ctx, J, d, gv_mean, gv_var, weight, iterations, tmax[0])));
        if (tmax[1] > 0) KWY_TRY((gva_launch_form<false, true>(ctx, J, d, gv_mean, gv_var, weight, iterations, tmax[1])));
        if (tmax[2] > 0) KWY_TRY((gva_launch_form<false, false>(ctx, J, d, gv_mean, gv_var, weight, iterations, tmax[2])));
        hipLaunchKernelGGL(k_gv_fold, dim3(J.n), dim3(GVA_NT), 0, ctx->stream, J, d, iterations);
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

static int gva_check(kwy_ctx *ctx, const kwy_gv_ascent_job *jobs, int count, int d, const double *gv_mean,
                     const double *gv_var, double weight, int iterations) {
  if (d < 1 || d > GVA_MAX_COLS || !gv_mean || !gv_var) {
    ctx->err = "gv_ascent: bad argument";
    return KWY_EINVAL;
  }
  if (!kwy_finite_pos(weight)) {
    ctx->err = "gv_ascent: weight must be positive and finite";
    return KWY_EINVAL;
  }
  if (iterations < 0 || iterations > KWY_MLPG_GV_MAX) {
    ctx->err = "gv_ascent: iterations outside [0, KWY_MLPG_GV_MAX]";
    return KWY_EINVAL;
  }
  for (int j = 0; j < count; ++j)
    if (jobs[j].T < 1 || jobs[j].T > 0x7ffffff0 || !jobs[j].band || !jobs[j].y) {
      ctx->err = "gv_ascent: bad argument";
      return KWY_EINVAL;
    }
  return KWY_OK;
}

static int gva_run(kwy_ctx *ctx, const kwy_gv_ascent_job *jobs, int count, int d, const double *gv_mean,
                   const double *gv_var, double weight, int iterations, int32_t *status) {
  std::vector<kwy_gva_view> v((size_t)count);
  for (int j = 0; j < count; ++j) {
    const kwy_gv_ascent_job &q = jobs[j];
    v[j] = kwy_gva_view{q.band, q.offset, q.y, q.T, d, d, q.objective, status ? status + j : nullptr};
  }
  return kwy_gva_launch(ctx, v.data(), count, d, gv_mean, gv_var, weight, iterations);
}

static size_t gva_jobs_scratch(const kwy_gv_ascent_job *jobs, int count, int d, int iterations) {
  size_t bytes = 0;
  for (int j = 0; j < count; ++j) bytes += kwy_gva_scratch_bytes(&jobs[j].T, 1, d, iterations);
  return bytes;
}

extern "C" int kwy_gv_ascent_batch_dev(kwy_ctx *ctx, const kwy_gv_ascent_job *jobs, int count, int d,
                                       const double *gv_mean, const double *gv_var, double weight, int iterations,
                                       int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  if (!jobs || count < 0) { ctx->err = "gv_ascent: bad argument"; return KWY_EINVAL; }
  if (count == 0) return KWY_OK;
  KWY_TRY(gva_check(ctx, jobs, count, d, gv_mean, gv_var, weight, iterations));
  KWY_HIP(hipSetDevice(ctx->device));
  KWY_TRY(kwy_arena_begin(ctx, gva_jobs_scratch(jobs, count, d, iterations)));
  return gva_run(ctx, jobs, count, d, gv_mean, gv_var, weight, iterations, status);
}

extern "C" int kwy_gv_ascent(kwy_ctx *ctx, const kwy_gv_ascent_job *jobs, int count, int d, const double *gv_mean,
                             const double *gv_var, double weight, int iterations, int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  if (!jobs || count < 0) { ctx->err = "gv_ascent: bad argument"; return KWY_EINVAL; }
  if (count == 0) return KWY_OK;
  KWY_TRY(gva_check(ctx, jobs, count, d, gv_mean, gv_var, weight, iterations));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "gv_ascent");
  double *dmean, *dvar;
  int32_t *dstatus;
  st.in(dmean, gv_mean, (size_t)d);
  st.in(dvar, gv_var, (size_t)d);
  st.out(dstatus, status, (size_t)count);
  std::vector<kwy_gv_ascent_job> staged(jobs, jobs + count);
  for (int j = 0; j < count; ++j) {
    const size_t n = (size_t)jobs[j].T * d;
    st.in(staged[j].band, jobs[j].band, n * 4);
    st.inout(staged[j].y, jobs[j].y, n);
    if (jobs[j].offset) st.in(staged[j].offset, jobs[j].offset, n);
    if (jobs[j].objective) st.out(staged[j].objective, jobs[j].objective, (size_t)iterations + 1);
  }
  KWY_TRY(st.begin(gva_jobs_scratch(jobs, count, d, iterations)));
  KWY_TRY(gva_run(ctx, staged.data(), count, d, dmean, dvar, weight, iterations, dstatus));
  return st.finish();
}

static int gvs_check(kwy_ctx *ctx, const double *moments, int count, int cols, const double *mean, const double *var) {
  if (cols < 1 || cols > GVA_MAX_COLS) { ctx->err = "gv_stats_from_moments: cols must be within [1, 64]"; return KWY_EINVAL; }
  if (!moments || count < 1 || !mean || !var) { ctx->err = "gv_stats_from_moments: bad argument"; return KWY_EINVAL; }
  return KWY_OK;
}

extern "C" int kwy_gv_stats_from_moments_dev(kwy_ctx *ctx, const double *moments, int count, int cols, double *gv_mean,
                                             double *gv_var) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(gvs_check(ctx, moments, count, cols, gv_mean, gv_var));
  KWY_HIP(hipSetDevice(ctx->device));
  KWY_PROF(ctx, "k_gv_stats", hipLaunchKernelGGL(k_gv_stats, dim3(1), dim3(GVA_MAX_COLS), 0, ctx->stream, moments, count,
                                                cols, gv_mean, gv_var));
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

extern "C" int kwy_gv_stats_from_moments(kwy_ctx *ctx, const double *moments, int count, int cols, double *gv_mean,
                                         double *gv_var) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(gvs_check(ctx, moments, count, cols, gv_mean, gv_var));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "gv_stats_from_moments");
  double *dm, *dmean, *dvar;
  st.in(dm, moments, 3 * (size_t)cols * (size_t)count);
  st.out(dmean, gv_mean, (size_t)cols);
  st.out(dvar, gv_var, (size_t)cols);
  KWY_TRY(st.begin());
  KWY_TRY(kwy_gv_stats_from_moments_dev(ctx, dm, count, cols, dmean, dvar));
  return st.finish();
}
