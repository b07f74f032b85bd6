// kwy_eval.hip -- objective evaluation of a conversion along an alignment: mel-cepstral distortion, f0 and voicing
// error, and the merge of per-utterance moments into corpus totals
//
//   mcd[t] = (10 / ln 10) * sqrt(2 * sum_{d = first_col .. cols-1} (a[ia[t], d] - b[ib[t], d])^2)          dB
//   cents  = 1200 * log2(fa[ia[t]] / fb[ib[t]])        on the frames where both tracks are voiced (f0 > 0)
//
// There is no reference call to cite: the reference measures a conversion only in its tests
// (tests/feature.py: calc_feature_diffs).  These are the measures voice-conversion work reports on held-out parallel
// utterances (Kubichek 1993 for the distortion; Toda, Black and Tokuda 2007 report it beside the unconverted source).
//
// The kernels gather through the alignment's index lists themselves: no gathered copies are made, and the row count
// may stay a device word (kwy_align_even_dev's n_out).  Reductions are deterministic: one workgroup per utterance;
// the lanes of a row's slot group add its squared differences through DPP, a slot group adds its rows in index order
// and the groups' partial sums are combined in group order through LDS (the f0 kernel: a thread's frames in index
// order, then kwy_block_sum).  An utterance's result therefore depends on that utterance alone -- not on the run, nor
// on the other utterances of the launch.  M2 is taken in a second pass about the mean of the first, as the column
// moments of kwy_gv.hip are.  Nothing is written but the triples, the counts, a status word and (when asked for) the
// per-row values.
//
// No kernel here allocates, synchronises or uses the context's arena: the _dev entries are legal inside a stream
// capture.  The host entries stage through the arena and synchronise, as kwy_gv_postfilter does.
#include <math.h>

#include "kwy_internal.hpp"

#define EV_GROUP 16        // utterances per launch
#define EV_MAX_COLS 64
#define EV_DB (10.0 / 2.302585092994045684)      // 10 / ln 10

struct ev_mcd {
  const double *a, *b;
  const int32_t *ia, *ib;
  const int64_t *n_dev;
  const double *mask;
  double *per_row;
  double *moments;         // (n, mean, M2)
  int32_t *status;         // rows with a coefficient that is not finite (may be NULL)
  int64_t a_rows, a_stride, b_rows, b_stride, off_a, off_b, rows, mask_stride, mask_rows;
};
typedef kwy_group<ev_mcd, EV_GROUP> ev_mcds;

struct ev_f0 {
  const double *fa, *fb;
  const int32_t *ia, *ib;
  const int64_t *n_dev;
  int64_t *counts;         // VV, VU, UV, UU
  double *moments;         // (n, mean, M2) of the cents over the VV frames
  int32_t *status;         // frames with an f0 that is negative or not finite (may be NULL)
  int64_t a_len, b_len, off_a, off_b, rows;
};
typedef kwy_group<ev_f0, EV_GROUP> ev_f0s;

// sum over the SLOTS lanes that share a row (a whole wavefront, or one of its halves); each of them gets the result
template <int SLOTS>
__device__ __forceinline__ double ev_slot_sum(double v) {
  if (SLOTS == 64) return kwy_wave_sum(v);
  v += kwy_dpp_f64<0x101>(v);
  v += kwy_dpp_f64<0x102>(v);
  v += kwy_dpp_f64<0x104>(v);
  v += kwy_dpp_f64<0x108>(v);  // lane 0 of every row of 16 lanes now holds its row's sum
  const double lo = kwy_readlane_f64(v, 0) + kwy_readlane_f64(v, 16);
  const double hi = kwy_readlane_f64(v, 32) + kwy_readlane_f64(v, 48);
  return (threadIdx.x & 32) ? hi : lo;
}

#define EV_AHEAD 4         // rows a slot group has in flight: the index, mask and row loads of a step are dependent

// One pass over the selected rows of a job.  Slot group g takes the rows t = g, g + G, ... in that order, EV_AHEAD of
// them per step -- first their indices, then their mask words, then their coefficients, so that a step waits for three
// loads and not for twelve -- and every thread runs every step, so that the lane exchanges are uniform.  SECOND: the
// squared deviations from `mean` instead of the values (the per-row values and the left-out count are the first
// pass's).
template <int SLOTS, bool SECOND>
__device__ __forceinline__ void ev_mcd_pass(const ev_mcd &U, int64_t n, int cols, int first_col, double mean, double &acc,
                                            double &cnt, int &left_out) {
  constexpr int G = KWY_THREADS / SLOTS;
  const int c = threadIdx.x % SLOTS, g = threadIdx.x / SLOTS;
  const bool live = c >= first_col && c < cols;
  for (int64_t t0 = 0; t0 < n; t0 += G * EV_AHEAD) {
    int64_t ra[EV_AHEAD], rb[EV_AHEAD], jm[EV_AHEAD];
    bool chosen[EV_AHEAD];
    double x[EV_AHEAD], y[EV_AHEAD];
#pragma unroll
    for (int q = 0; q < EV_AHEAD; ++q) {
      const int64_t t = t0 + q * G + g;
      const bool valid = t < n;
      const int64_t ja = valid && U.ia ? (int64_t)U.ia[t] : t, jb = valid && U.ib ? (int64_t)U.ib[t] : t;
      ra[q] = ja - U.off_a;
      rb[q] = jb - U.off_b;
      jm[q] = jb;
      chosen[q] = valid && ra[q] >= 0 && ra[q] < U.a_rows && rb[q] >= 0 && rb[q] < U.b_rows &&
                  (!U.mask || (jb >= 0 && jb < U.mask_rows));      // (beyond either side or the mask: passed over)
    }
    if (U.mask) {
#pragma unroll
      for (int q = 0; q < EV_AHEAD; ++q) chosen[q] = chosen[q] && U.mask[jm[q] * U.mask_stride] > 0.0;
    }
#pragma unroll
    for (int q = 0; q < EV_AHEAD; ++q) {
      const bool read = chosen[q] && live;
      x[q] = read ? U.a[ra[q] * U.a_stride + c] : 0.0;
      y[q] = read ? U.b[rb[q] * U.b_stride + c] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < EV_AHEAD; ++q) {
      const int64_t t = t0 + q * G + g;
      const bool odd = !(kwy_finite(x[q]) && kwy_finite(y[q]));      // a coefficient that is not finite
      const double d = x[q] - y[q];
      const double s = ev_slot_sum<SLOTS>(odd ? 0.0 : d * d);
      const unsigned long long odd_lanes = __ballot(odd);
      const bool row_odd = SLOTS == 64 ? odd_lanes != 0 : ((odd_lanes >> (threadIdx.x & 32)) & 0xffffffffull) != 0;
      const bool use = chosen[q] && !row_odd;
      const double v = EV_DB * sqrt(2.0 * s);
      if (SECOND) {
        if (use) {
          const double dv = v - mean;
          acc += dv * dv;
        }
      } else {
        if (use) {
          acc += v;
          cnt += 1.0;
        }
        if (chosen[q] && row_odd) ++left_out;
        if (U.per_row && t < n && c == 0) U.per_row[t] = use ? v : __builtin_nan("");
      }
    }
  }
}

// the slot groups' partials (part[g]) added in group order; every thread gets the result
template <int G>
__device__ __forceinline__ double ev_group_fold(double v, int c, int g, double *part) {
  __syncthreads();
  if (c == 0) part[g] = v;
  __syncthreads();
  double s = part[0];
#pragma unroll
  for (int i = 1; i < G; ++i) s += part[i];
  return s;
}

template <int SLOTS>
__device__ __forceinline__ void ev_mcd_job(const ev_mcd &U, int cols, int first_col, double *part) {
  constexpr int G = KWY_THREADS / SLOTS;
  const int c = threadIdx.x % SLOTS, g = threadIdx.x / SLOTS;
  const int64_t n = kwy_device_count(U.rows, U.n_dev);
  double sum = 0.0, cnt = 0.0, m2 = 0.0, none = 0.0;
  int left_out = 0, unused = 0;
  ev_mcd_pass<SLOTS, false>(U, n, cols, first_col, 0.0, sum, cnt, left_out);
  sum = ev_group_fold<G>(sum, c, g, part);
  cnt = ev_group_fold<G>(cnt, c, g, part);
  const double bad = ev_group_fold<G>((double)left_out, c, g, part);
  const double mean = cnt > 0.0 ? sum / cnt : 0.0;
  ev_mcd_pass<SLOTS, true>(U, n, cols, first_col, mean, m2, none, unused);
  m2 = ev_group_fold<G>(m2, c, g, part);
  if (threadIdx.x == 0) {
    U.moments[0] = cnt;
    U.moments[1] = mean;
    U.moments[2] = m2;
    if (U.status) *U.status = (int32_t)fmin(bad, 2147483647.0);
  }
}

// one workgroup per utterance: 32 slots x 8 rows a step for cols <= 32, 64 x 4 above (a wavefront reads whole
// consecutive rows of the index list)
__global__ __launch_bounds__(KWY_THREADS) void k_eval_mcd(ev_mcds B, int cols, int first_col) {
  __shared__ double part[KWY_THREADS / 32];
  const ev_mcd &U = B.u[blockIdx.x];
  if (cols <= 32) ev_mcd_job<32>(U, cols, first_col, part);
  else ev_mcd_job<64>(U, cols, first_col, part);
}

// one workgroup per utterance: the voicing confusion counts, and (n, mean, M2) of the cents over the VV frames
__global__ __launch_bounds__(KWY_THREADS) void k_eval_f0(ev_f0s B) {
  __shared__ double red[KWY_WAVES];
  const ev_f0 &U = B.u[blockIdx.x];
  const int tid = threadIdx.x;
  const int64_t n = kwy_device_count(U.rows, U.n_dev);
  double vv = 0.0, vu = 0.0, uv = 0.0, uu = 0.0, bad = 0.0, sum = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    const double mean = vv > 0.0 ? sum / vv : 0.0;        // (second pass: of the first pass's totals)
    double c_vv = 0.0, c_vu = 0.0, c_uv = 0.0, c_uu = 0.0, c_bad = 0.0, acc = 0.0;
    for (int64_t t = tid; t < n; t += KWY_THREADS) {
      const int64_t ra = (U.ia ? (int64_t)U.ia[t] : t) - U.off_a, rb = (U.ib ? (int64_t)U.ib[t] : t) - U.off_b;
      if (!(ra >= 0 && ra < U.a_len && rb >= 0 && rb < U.b_len)) continue;      // beyond either track: not a frame
      const double fa = U.fa[ra], fb = U.fb[rb];
      if (!(fa >= 0.0 && fa <= KWY_DBL_MAX && fb >= 0.0 && fb <= KWY_DBL_MAX)) { c_bad += 1.0; continue; }
      const bool va = fa > 0.0, vb = fb > 0.0;
      if (va && vb) {
        const double cents = 1200.0 * log2(fa / fb);
        if (pass == 0) acc += cents;
        else acc += (cents - mean) * (cents - mean);
        c_vv += 1.0;
      } else if (va) c_vu += 1.0;
      else if (vb) c_uv += 1.0;
      else c_uu += 1.0;
    }
    if (pass == 0) {
      vv = kwy_block_sum(c_vv, red);
      vu = kwy_block_sum(c_vu, red);
      uv = kwy_block_sum(c_uv, red);
      uu = kwy_block_sum(c_uu, red);
      bad = kwy_block_sum(c_bad, red);
      sum = kwy_block_sum(acc, red);
    } else {
      const double m2 = kwy_block_sum(acc, red);
      if (tid == 0) {
        U.counts[0] = (int64_t)vv;
        U.counts[1] = (int64_t)vu;
        U.counts[2] = (int64_t)uv;
        U.counts[3] = (int64_t)uu;
        U.moments[0] = vv;
        U.moments[1] = mean;
        U.moments[2] = m2;
        if (U.status) *U.status = (int32_t)fmin(bad, 2147483647.0);
      }
    }
  }
}

// Chan et al.'s pairwise combination, a left fold over `count` rows of `width` triples in row order: one lane per
// column of triples, rows with n == 0 skipped
__global__ __launch_bounds__(EV_MAX_COLS) void k_moments_merge(const double *__restrict__ m, int count, int width,
                                                                double *__restrict__ out) {
  const int c = threadIdx.x;
  if (c >= width) return;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int i = 0; i < count; ++i) {
    const double *t = m + 3 * ((int64_t)i * width + c);
    const double nb = t[0], mb = t[1], m2b = t[2];
    if (nb == 0.0) continue;
    if (n == 0.0) {
      n = nb; mean = mb; m2 = m2b;
      continue;
    }
    const double nn = n + nb, delta = mb - mean;
    mean = mean + delta * (nb / nn);
    m2 = (m2 + m2b) + delta * delta * (n * nb / nn);
    n = nn;
  }
  out[3 * c] = n;
  out[3 * c + 1] = mean;
  out[3 * c + 2] = m2;
}

// sum and count behind `count` triples, added to acc[0..1] in row order by one lane: the running totals of a
// re-alignment pass stay on the device from wave to wave
__global__ void k_eval_accumulate(const double *__restrict__ m, int count, double *__restrict__ acc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sum = acc[0], n = acc[1];
  for (int i = 0; i < count; ++i) {
    const double ni = m[3 * (int64_t)i];
    if (ni == 0.0) continue;
    sum += ni * m[3 * (int64_t)i + 1];
    n += ni;
  }
  acc[0] = sum;
  acc[1] = n;
}

// ---- mel-cepstral distortion ------------------------------------------------------------------------------------------
static int ev_check_mcd(kwy_ctx *ctx, const kwy_mcd_job *jobs, int count, int cols, int first_col, const double *moments,
                        bool host) {
  if (cols < 1 || cols > EV_MAX_COLS) { ctx->err = "mcd: cols must be within [1, 64]"; return KWY_EINVAL; }
  if (!jobs || count < 1 || !moments || first_col < 0 || first_col > cols) {
    ctx->err = "mcd: bad argument";
    return KWY_EINVAL;
  }
  for (int i = 0; i < count; ++i) {
    const kwy_mcd_job &j = jobs[i];
    const bool bad = j.rows < 0 || j.a_rows < 0 || j.b_rows < 0 || (j.a_rows > 1 && j.a_stride < cols) ||
                     (j.b_rows > 1 && j.b_stride < cols) ||
                     (j.a_rows > 0 && !j.a) || (j.b_rows > 0 && !j.b) ||
                     (j.mask && (j.mask_rows < 0 || (j.mask_rows > 1 && j.mask_stride < 1))) || (host && j.n_dev);
    if (bad) {
      ctx->err = host && j.n_dev ? "mcd: the host form takes its row count by value" : "mcd: bad argument";
      return KWY_EINVAL;
    }
  }
  return KWY_OK;
}

static int ev_launch_mcd(kwy_ctx *ctx, const kwy_mcd_job *jobs, int count, int cols, int first_col, double *moments,
                         int32_t *status) {
  return kwy_for_tables<ev_mcds>(
      count,
      [&](int i) {
        const kwy_mcd_job &j = jobs[i];
        return ev_mcd{j.a, j.b, j.idx_a, j.idx_b, j.n_dev, j.mask, j.per_row, moments + 3 * (int64_t)i,
                      status ? status + i : nullptr, j.a_rows, j.a_stride, j.b_rows, j.b_stride, j.off_a, j.off_b,
                      j.rows, j.mask_stride, j.mask_rows};
      },
      [&](const ev_mcds &B, int) {
        KWY_PROF(ctx, "k_eval_mcd",
                 hipLaunchKernelGGL(k_eval_mcd, dim3(B.n), dim3(KWY_THREADS), 0, ctx->stream, B, cols, first_col));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

extern "C" int kwy_mcd_batch_dev(kwy_ctx *ctx, const kwy_mcd_job *jobs, int count, int cols, int first_col,
                                 double *moments, int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(ev_check_mcd(ctx, jobs, count, cols, first_col, moments, false));
  KWY_HIP(hipSetDevice(ctx->device));
  return ev_launch_mcd(ctx, jobs, count, cols, first_col, moments, status);
}

// doubles of a strided block of `rows` rows whose last row holds `last` values
static inline size_t ev_span(int64_t rows, int64_t stride, int64_t last) {
  return rows > 0 ? (size_t)((rows - 1) * stride + last) : 0;
}

extern "C" int kwy_mcd(kwy_ctx *ctx, const kwy_mcd_job *jobs, int count, int cols, int first_col, double *moments,
                       int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(ev_check_mcd(ctx, jobs, count, cols, first_col, moments, true));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "mcd");
  double *dm;
  int32_t *dstatus;
  st.out(dm, moments, 3 * (size_t)count);
  st.out(dstatus, status, (size_t)count);
  std::vector<kwy_mcd_job> staged(jobs, jobs + count);
  for (int i = 0; i < count; ++i) {
    const kwy_mcd_job &j = jobs[i];
    kwy_mcd_job &s = staged[i];
    st.in(s.a, j.a, ev_span(j.a_rows, j.a_stride, cols));
    st.in(s.b, j.b, ev_span(j.b_rows, j.b_stride, cols));
    if (j.idx_a) st.in(s.idx_a, j.idx_a, (size_t)j.rows);
    if (j.idx_b) st.in(s.idx_b, j.idx_b, (size_t)j.rows);
    if (j.mask) st.in(s.mask, j.mask, ev_span(j.mask_rows, j.mask_stride, 1));
    if (j.per_row) st.out(s.per_row, j.per_row, (size_t)j.rows);
  }
  KWY_TRY(st.begin());
  KWY_TRY(ev_launch_mcd(ctx, staged.data(), count, cols, first_col, dm, dstatus));
  return st.finish();
}

// ---- f0 and voicing error ----------------------------------------------------------------------------------------------
static int ev_check_f0(kwy_ctx *ctx, const kwy_f0_error_job *jobs, int count, const int64_t *counts,
                       const double *moments, bool host) {
  if (!jobs || count < 1 || !counts || !moments) { ctx->err = "f0_error: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i) {
    const kwy_f0_error_job &j = jobs[i];
    if (j.rows < 0 || j.a_length < 0 || j.b_length < 0 || (j.a_length > 0 && !j.f0_a) || (j.b_length > 0 && !j.f0_b) ||
        (host && j.n_dev)) {
      ctx->err = host && j.n_dev ? "f0_error: the host form takes its row count by value" : "f0_error: bad argument";
      return KWY_EINVAL;
    }
  }
  return KWY_OK;
}

static int ev_launch_f0(kwy_ctx *ctx, const kwy_f0_error_job *jobs, int count, int64_t *counts, double *moments,
                        int32_t *status) {
  return kwy_for_tables<ev_f0s>(
      count,
      [&](int i) {
        const kwy_f0_error_job &j = jobs[i];
        return ev_f0{j.f0_a, j.f0_b, j.idx_a, j.idx_b, j.n_dev, counts + 4 * (int64_t)i, moments + 3 * (int64_t)i,
                     status ? status + i : nullptr, j.a_length, j.b_length, j.off_a, j.off_b, j.rows};
      },
      [&](const ev_f0s &B, int) {
        KWY_PROF(ctx, "k_eval_f0", hipLaunchKernelGGL(k_eval_f0, dim3(B.n), dim3(KWY_THREADS), 0, ctx->stream, B));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

extern "C" int kwy_f0_error_batch_dev(kwy_ctx *ctx, const kwy_f0_error_job *jobs, int count, int64_t *counts,
                                      double *moments, int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(ev_check_f0(ctx, jobs, count, counts, moments, false));
  KWY_HIP(hipSetDevice(ctx->device));
  return ev_launch_f0(ctx, jobs, count, counts, moments, status);
}

extern "C" int kwy_f0_error(kwy_ctx *ctx, const kwy_f0_error_job *jobs, int count, int64_t *counts, double *moments,
                            int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(ev_check_f0(ctx, jobs, count, counts, moments, true));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "f0_error");
  double *dm;
  int64_t *dc;
  int32_t *dstatus;
  st.out(dm, moments, 3 * (size_t)count);
  st.out(dc, counts, 4 * (size_t)count);
  st.out(dstatus, status, (size_t)count);
  std::vector<kwy_f0_error_job> staged(jobs, jobs + count);
  for (int i = 0; i < count; ++i) {
    const kwy_f0_error_job &j = jobs[i];
    kwy_f0_error_job &s = staged[i];
    st.in(s.f0_a, j.f0_a, (size_t)j.a_length);
    st.in(s.f0_b, j.f0_b, (size_t)j.b_length);
    if (j.idx_a) st.in(s.idx_a, j.idx_a, (size_t)j.rows);
    if (j.idx_b) st.in(s.idx_b, j.idx_b, (size_t)j.rows);
  }
  KWY_TRY(st.begin());
  KWY_TRY(ev_launch_f0(ctx, staged.data(), count, dc, dm, dstatus));
  return st.finish();
}

// ---- merging -------------------------------------------------------------------------------------------------------------
static int ev_check_merge(kwy_ctx *ctx, const double *moments, int count, int width, const double *out) {
  if (!moments || count < 1 || width < 1 || width > EV_MAX_COLS || !out) {
    ctx->err = "moments_merge: bad argument (width within [1, 64])";
    return KWY_EINVAL;
  }
  return KWY_OK;
}

extern "C" int kwy_moments_merge_dev(kwy_ctx *ctx, const double *moments, int count, int width, double *out) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(ev_check_merge(ctx, moments, count, width, out));
  KWY_HIP(hipSetDevice(ctx->device));
  KWY_PROF(ctx, "k_moments_merge", hipLaunchKernelGGL(k_moments_merge, dim3(1), dim3(EV_MAX_COLS), 0, ctx->stream,
                                                       moments, count, width, out));
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

extern "C" int kwy_moments_merge(kwy_ctx *ctx, const double *moments, int count, int width, double *out) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(ev_check_merge(ctx, moments, count, width, out));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "moments_merge");
  double *dm, *dout;
  st.in(dm, moments, 3 * (size_t)width * (size_t)count);
  st.out(dout, out, 3 * (size_t)width);
  KWY_TRY(st.begin());
  KWY_TRY(kwy_moments_merge_dev(ctx, dm, count, width, dout));
  return st.finish();
}

extern "C" int kwy_moments_accumulate_dev(kwy_ctx *ctx, const double *moments, int count, double *acc) {
  if (!ctx) return KWY_EINVAL;
  if (!moments || !acc || count < 0) { ctx->err = "moments_accumulate: bad argument"; return KWY_EINVAL; }
  if (count == 0) return KWY_OK;
  KWY_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_eval_accumulate, dim3(1), dim3(64), 0, ctx->stream, moments, count, acc);
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}
