// kwy_gv.hip -- global-variance postfilter: the column moments of a batch of matrices, the corpus statistic, the filter
//
//   m_d = mean of x[:, d],  v_d = M2_d / rows,  r_d = sqrt(gv_d / v_d)
//   out[t, d] = base[t, d] + strength * (r_d - 1) * (x[t, d] - m_d)          (d >= first_col)
//
// There is no reference call to cite: the reference synthesises the converter's output as it is
// (kwiiyatta/convert_voice.py:35-46).  This is the postfilter of Toda, Black and Tokuda (2007) in the form
// s (r (x - m) + m) + (1 - s) x, written so that s = 0 leaves base as it is.
//
// Reductions are deterministic: one workgroup per matrix; a thread owns ONE column slot and ONE residue class of rows
// (32 slots x 8 row lanes for cols <= 32, 64 x 4 above: a wavefront then reads whole consecutive rows and no thread
// changes column between steps), adds its rows in index order, and the row lanes' partial sums are combined in lane
// order through LDS.  A matrix's moments therefore depend on its own values and shape only -- not on the run, nor on the
// other matrices of the launch.  The statistic is a left fold over the matrices in index order, one lane per column.
//
// No kernel here allocates, synchronises or uses the context's arena: the _dev entries are legal inside a stream
// capture.  The host entries stage through the arena and synchronise, as kwy_f0_map does.
#include <math.h>

#include "kwy_internal.hpp"

#define GV_GROUP 32        // matrices per launch
#define GV_MAX_COLS 64
#define GV_CHUNK 2048      // elements a workgroup of the filter takes per step
#define GV_MAX_BLOCKS 64   // workgroups per matrix in the filter

struct gv_mat {
  const double *x;
  int64_t rows;
  double *out;             // cols x (n, mean, M2)
};
typedef kwy_group<gv_mat, GV_GROUP> gv_mats;

struct gv_apply {
  const double *x;
  int64_t rows;
  const double *moments;
  const double *base;
  double *out;
  int32_t *status;         // columns copied for an unusable v or gv (may be NULL)
};
typedef kwy_group<gv_apply, GV_GROUP> gv_applies;

// the row lanes' partials of column slot c (part[lane * slots + c]) added in lane order
__device__ __forceinline__ double gv_lane_fold(const double *part, int slots, int lanes, int c) {
  double s = part[c];
  for (int l = 1; l < lanes; ++l) s += part[l * slots + c];
  return s;
}

// one workgroup per matrix: (n, mean, M2) of every column in two passes
__global__ __launch_bounds__(KWY_THREADS) void k_gv_moments(gv_mats B, int cols) {
  __shared__ double part[KWY_THREADS];
  __shared__ double same[KWY_THREADS];
  __shared__ double mean_s[GV_MAX_COLS];
  const gv_mat &U = B.u[blockIdx.x];
  const int slots = cols <= 32 ? 32 : 64, lanes = KWY_THREADS / slots;
  const int tid = threadIdx.x, c = tid % slots, lane = tid / slots;
  const bool live = c < cols;
  const int64_t rows = U.rows;
  const double *col = U.x + c;
  const double first = live && rows > 0 ? col[0] : 0.0;
  double sum = 0.0, eq = 1.0;
  if (live) {
#pragma unroll 4
    for (int64_t r = lane; r < rows; r += lanes) {
      const double v = col[r * cols];
      sum += v;
      eq = v == first ? eq : 0.0;
    }
  }
  part[tid] = sum;
  same[tid] = eq;
  __syncthreads();
  if (tid < cols) {
    const double s = gv_lane_fold(part, slots, lanes, tid);
    double all = same[tid];
    for (int l = 1; l < lanes; ++l) all = same[l * slots + tid] != 0.0 ? all : 0.0;
    // a column of one repeated value: that value, whatever rows copies of it add up to (its M2 is then 0 exactly)
    mean_s[tid] = rows > 0 ? (all != 0.0 ? first : s / (double)rows) : 0.0;
  }
  __syncthreads();
  double m2 = 0.0;
  if (live) {
    const double mean = mean_s[c];
#pragma unroll 4
    for (int64_t r = lane; r < rows; r += lanes) {
      const double d = col[r * cols] - mean;
      m2 += d * d;
    }
  }
  part[tid] = m2;
  __syncthreads();
  if (tid < cols) {
    double *o = U.out + 3 * tid;
    o[0] = (double)rows;
    o[1] = mean_s[tid];
    o[2] = gv_lane_fold(part, slots, lanes, tid);
  }
}

// gv[c] = mean over the matrices with n > 0 of M2 / n: a left fold in index order, one lane per column
__global__ __launch_bounds__(GV_MAX_COLS) void k_gv_statistic(const double *__restrict__ m, int count, int cols,
                                                              double *__restrict__ gv) {
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
  gv[c] = used > 0.0 ? sum / used : 0.0;
}

// blockIdx.y: the matrix; its workgroups stride over the flattened matrix in steps of GV_CHUNK elements
__global__ __launch_bounds__(KWY_THREADS) void k_gv_apply(gv_applies B, int cols, int first_col,
                                                           const double *__restrict__ gv, double strength) {
  __shared__ double coef[GV_MAX_COLS];     // strength * (r - 1); 0: the column is copied
  __shared__ double mean_s[GV_MAX_COLS];
  __shared__ int bad_s[GV_MAX_COLS];
  const gv_apply &U = B.u[blockIdx.y];
  const int tid = threadIdx.x;
  if (tid < cols) {
    double k = 0.0;
    int bad = 0;
    const double n = U.moments[3 * tid], g = gv[tid];
    if (tid >= first_col) {
      const double v = n > 0.0 ? U.moments[3 * tid + 2] / n : 0.0;       // (no rows: nothing to stretch)
      const bool v_ok = v >= 0.0 && v <= KWY_DBL_MAX;
      const bool g_ok = g > 0.0 && g <= KWY_DBL_MAX;
      if (!v_ok || !g_ok) bad = 1;
      else if (v > 0.0) k = strength * (sqrt(g / v) - 1.0);
    }
    coef[tid] = k;
    mean_s[tid] = U.moments[3 * tid + 1];
    bad_s[tid] = bad;
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0 && U.status) {
    int bad = 0;
    for (int c = 0; c < cols; ++c) bad += bad_s[c];
    *U.status = bad;
  }
  const int64_t total = U.rows * cols;
  for (int64_t i0 = (int64_t)blockIdx.x * GV_CHUNK; i0 < total; i0 += (int64_t)gridDim.x * GV_CHUNK) {
    const int c0 = (int)(i0 % cols);         // (uniform; the lanes' columns follow in 32-bit arithmetic)
#pragma unroll
    for (int q = 0; q < GV_CHUNK / KWY_THREADS; ++q) {
      const int64_t i = i0 + q * KWY_THREADS + tid;
      if (i < total) {
        const int c = (c0 + q * KWY_THREADS + tid) % cols;
        const double k = coef[c], b = U.base[i];
        U.out[i] = k != 0.0 ? b + k * (U.x[i] - mean_s[c]) : b;
      }
    }
  }
}

static int gv_check_cols(kwy_ctx *ctx, int cols, const char *what) {
  if (cols < 1 || cols > GV_MAX_COLS) {
    ctx->err = std::string(what) + ": cols must be within [1, 64]";
    return KWY_EINVAL;
  }
  return KWY_OK;
}

static int gv_check_mats(kwy_ctx *ctx, const kwy_gv_matrix *mats, int count, int cols, const double *moments) {
  KWY_TRY(gv_check_cols(ctx, cols, "column_moments"));
  if (!mats || count < 1 || !moments) { ctx->err = "column_moments: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i)
    if (mats[i].rows < 0 || (mats[i].rows > 0 && !mats[i].x)) {
      ctx->err = "column_moments: bad argument";
      return KWY_EINVAL;
    }
  return KWY_OK;
}

static int gv_launch_moments(kwy_ctx *ctx, const kwy_gv_matrix *mats, int count, int cols, double *moments) {
  return kwy_for_tables<gv_mats>(
      count, [&](int i) { return gv_mat{mats[i].x, mats[i].rows, moments + 3 * (int64_t)cols * i}; },
      [&](const gv_mats &B, int) {
        KWY_PROF(ctx, "k_gv_moments",
                 hipLaunchKernelGGL(k_gv_moments, dim3(B.n), dim3(KWY_THREADS), 0, ctx->stream, B, cols));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

extern "C" int kwy_column_moments_batch_dev(kwy_ctx *ctx, const kwy_gv_matrix *mats, int count, int cols,
                                            double *moments) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(gv_check_mats(ctx, mats, count, cols, moments));
  KWY_HIP(hipSetDevice(ctx->device));
  return gv_launch_moments(ctx, mats, count, cols, moments);
}

extern "C" int kwy_column_moments_dev(kwy_ctx *ctx, const double *x, int64_t rows, int cols, double *moments) {
  const kwy_gv_matrix one = {x, rows};
  return kwy_column_moments_batch_dev(ctx, &one, 1, cols, moments);
}

extern "C" int kwy_column_moments(kwy_ctx *ctx, const kwy_gv_matrix *mats, int count, int cols, double *moments) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(gv_check_mats(ctx, mats, count, cols, moments));
  KWY_HIP(hipSetDevice(ctx->device));
  const size_t nm = 3 * (size_t)cols * (size_t)count;
  kwy_staging st(ctx, "column_moments");
  double *dm;
  st.out(dm, moments, nm);
  std::vector<kwy_gv_matrix> staged(mats, mats + count);
  for (int i = 0; i < count; ++i) st.in(staged[i].x, mats[i].x, (size_t)mats[i].rows * cols);
  KWY_TRY(st.begin());
  KWY_TRY(gv_launch_moments(ctx, staged.data(), count, cols, dm));
  return st.finish();
}

static int gv_check_statistic(kwy_ctx *ctx, const double *moments, int count, int cols, const double *gv) {
  KWY_TRY(gv_check_cols(ctx, cols, "gv_from_moments"));
  if (!moments || count < 1 || !gv) { ctx->err = "gv_from_moments: bad argument"; return KWY_EINVAL; }
  return KWY_OK;
}

extern "C" int kwy_gv_from_moments_dev(kwy_ctx *ctx, const double *moments, int count, int cols, double *gv) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(gv_check_statistic(ctx, moments, count, cols, gv));
  KWY_HIP(hipSetDevice(ctx->device));
  KWY_PROF(ctx, "k_gv_statistic",
           hipLaunchKernelGGL(k_gv_statistic, dim3(1), dim3(GV_MAX_COLS), 0, ctx->stream, moments, count, cols, gv));
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

extern "C" int kwy_gv_from_moments(kwy_ctx *ctx, const double *moments, int count, int cols, double *gv) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(gv_check_statistic(ctx, moments, count, cols, gv));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "gv_from_moments");
  double *dm, *dgv;
  st.in(dm, moments, 3 * (size_t)cols * (size_t)count);
  st.out(dgv, gv, (size_t)cols);
  KWY_TRY(st.begin());
  KWY_TRY(kwy_gv_from_moments_dev(ctx, dm, count, cols, dgv));
  return st.finish();
}

static int gv_check_jobs(kwy_ctx *ctx, const kwy_gv_job *jobs, int count, int cols, int first_col, const double *gv,
                         double strength, bool need_moments) {
  KWY_TRY(gv_check_cols(ctx, cols, "gv_postfilter"));
  if (!(strength >= 0.0 && strength <= 1.0)) {
    ctx->err = "gv_postfilter: strength must be within [0, 1]";
    return KWY_EINVAL;
  }
  if (!jobs || count < 1 || !gv || first_col < 0 || first_col > cols) {
    ctx->err = "gv_postfilter: bad argument";
    return KWY_EINVAL;
  }
  for (int i = 0; i < count; ++i)
    if (jobs[i].rows < 0 || (need_moments && !jobs[i].moments) ||
        (jobs[i].rows > 0 && (!jobs[i].x || !jobs[i].base || !jobs[i].out))) {
      ctx->err = "gv_postfilter: bad argument";
      return KWY_EINVAL;
    }
  return KWY_OK;
}

static int gv_launch_apply(kwy_ctx *ctx, const kwy_gv_job *jobs, int count, int cols, int first_col, const double *gv,
                           double strength, int32_t *status) {
  return kwy_for_tables<gv_applies>(
      count,
      [&](int i) {
        const kwy_gv_job &j = jobs[i];
        return gv_apply{j.x, j.rows, j.moments, j.base, j.out, status ? status + i : nullptr};
      },
      [&](const gv_applies &B, int) {
        int64_t longest = 0;
        for (int u = 0; u < B.n; ++u) longest = B.u[u].rows > longest ? B.u[u].rows : longest;
        int64_t blocks = (longest * cols + GV_CHUNK - 1) / GV_CHUNK;
        blocks = blocks < 1 ? 1 : (blocks > GV_MAX_BLOCKS ? GV_MAX_BLOCKS : blocks);      // (block 0 writes the status)
        KWY_PROF(ctx, "k_gv_apply", hipLaunchKernelGGL(k_gv_apply, dim3((unsigned)blocks, B.n), dim3(KWY_THREADS), 0,
                                                       ctx->stream, B, cols, first_col, gv, strength));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

extern "C" int kwy_gv_postfilter_batch_dev(kwy_ctx *ctx, const kwy_gv_job *jobs, int count, int cols, int first_col,
                                           const double *gv, double strength, int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(gv_check_jobs(ctx, jobs, count, cols, first_col, gv, strength, true));
  KWY_HIP(hipSetDevice(ctx->device));
  return gv_launch_apply(ctx, jobs, count, cols, first_col, gv, strength, status);
}

extern "C" int kwy_gv_postfilter_dev(kwy_ctx *ctx, const double *x, int64_t rows, int cols, int first_col,
                                     const double *moments, const double *gv, double strength, const double *base,
                                     double *out, int32_t *status) {
  const kwy_gv_job one = {x, rows, moments, base, out};
  return kwy_gv_postfilter_batch_dev(ctx, &one, 1, cols, first_col, gv, strength, status);
}

extern "C" int kwy_gv_postfilter(kwy_ctx *ctx, const kwy_gv_job *jobs, int count, int cols, int first_col,
                                 const double *gv, double strength, int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(gv_check_jobs(ctx, jobs, count, cols, first_col, gv, strength, false));
  KWY_HIP(hipSetDevice(ctx->device));
  const size_t nm = 3 * (size_t)cols;
  kwy_staging st(ctx, "gv_postfilter");
  double *dgv, *dm;
  int32_t *dstatus;
  st.in(dgv, gv, (size_t)cols);
  st.out(dstatus, status, (size_t)count);
  st.tmp(dm, nm * (size_t)count);
  std::vector<kwy_gv_job> staged(jobs, jobs + count);
  std::vector<kwy_gv_matrix> mats((size_t)count);
  for (int i = 0; i < count; ++i) {
    const size_t n = (size_t)jobs[i].rows * cols;
    st.in(staged[i].x, jobs[i].x, n);
    if (jobs[i].base != jobs[i].x) st.in(staged[i].base, jobs[i].base, n);
    st.out(staged[i].out, jobs[i].out, n);
  }
  KWY_TRY(st.begin());
  for (int i = 0; i < count; ++i) {
    if (jobs[i].base == jobs[i].x) staged[i].base = staged[i].x;
    staged[i].moments = dm + nm * (size_t)i;
    mats[i] = kwy_gv_matrix{staged[i].x, jobs[i].rows};
  }
  KWY_TRY(gv_launch_moments(ctx, mats.data(), count, cols, dm));
  KWY_TRY(gv_launch_apply(ctx, staged.data(), count, cols, first_col, dgv, strength, dstatus));
  return st.finish();
}
