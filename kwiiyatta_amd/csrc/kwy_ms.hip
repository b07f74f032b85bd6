// kwy_ms.hip -- modulation-spectrum postfilter: the log modulation spectra of a batch of matrices, their running
// statistics, the filter
//
//   m = mean of x[:, d],  z[t] = x[t, d] - m (t < T), 0 (T <= t < L),  Z = rfft(z)
//   s[f]  = log(max(|Z[f]|^2, DBL_MIN) / T)                                        f = 0 .. L/2
//   s'[f] = (1 - k) s[f] + k (sigmaN[f] / sigmaG[f] (s[f] - muG[f]) + muN[f]),   g[f] = exp((s'[f] - s[f]) / 2),  g[0] = 1
//   out[t, d] = base[t, d] + (irfft(g Z)[t] - z[t])                               (d >= first_col)
//
// There is no reference call to cite: the reference synthesises the converter's output as it is
// (kwiiyatta/convert_voice.py:35-46).  This is the utterance-level postfilter of Takamichi et al. (2016); the
// global-variance filter of kwy_gv.hip is its one-bin case.
//
// One workgroup per (matrix, column) does everything in one pass over LDS: the column's mean as kwy_column_moments
// defines it, the zero-padded trajectory, the forward real transform, the per-bin log / gain, the inverse transform,
// and the T samples.  blockIdx.x is the column, so the workgroups that share a matrix's cache lines (a column is read
// with a stride of cols doubles) are launched next to each other.  L = 2H reals are H packed points: 16 (H + 1 + H/8)
// bytes of LDS, 74 KB at L = 8192 -- two workgroups per CU; 256 threads up to L = 4096 (H/8 <= 256: one butterfly per
// thread and pass), 512 at L = 8192.
//
// Every reduction has a fixed order (thread-strided partials, kwy_block_sum): a matrix's result depends on its own
// values, the statistics and the shape only.  The status word of a matrix is a count of integers added with atomicAdd
// (order-free) onto a word the entry zeroes first.  The statistics update is a Welford fold per (column, bin), one
// thread each, over the block's matrices in index order.
//
// No kernel here allocates or synchronises: the _dev entries are legal inside a stream capture once the context holds
// the twiddle tables of the length (the first call of a length makes them).  The host entries stage through the arena
// and synchronise.
#include <float.h>
#include <math.h>

#include "kwy_internal.hpp"

#define MS_GROUP 64        // matrices per launch
#define MS_MAX_COLS 64

struct ms_view {
  const double *x;
  int64_t rows;
  const double *base;      // filter only
  double *out;             // filter: rows x cols; log-spectra: cols x (L/2 + 1)
  int32_t *status;         // filter: the matrix's word (may be NULL); log-spectra: cols validity words
};
typedef kwy_group<ms_view, MS_GROUP> ms_views;
static_assert(sizeof(ms_views) + 64 <= KWY_KERNARG_MAX, "k_ms: the table and eight scalar arguments");

template <int LOG2H>
struct ms_cfg {
  static constexpr int NT = LOG2H == 12 ? 512 : 256;
};


template <int LOG2H, bool FILTER>
__global__ __launch_bounds__(ms_cfg<LOG2H>::NT) void k_ms(ms_views B, int cols, int first_col,
                                                          const double *__restrict__ statsG,
                                                          const double *__restrict__ statsN, double strength,
                                                          const kwy_c *__restrict__ twH, const kwy_c *__restrict__ twP,
                                                          const kwy_c *__restrict__ twN) {
  constexpr int NT = ms_cfg<LOG2H>::NT, H = 1 << LOG2H, N = 2 * H, TWL = H / 8, E = N / NT, K = H + 1;
  extern __shared__ double smem[];
  kwy_c *z = (kwy_c *)smem;              // H + 1 complex
  kwy_c *twl = z + (H + 1);              // exp(-2 pi i k / H), k < H/8
  double *red = (double *)(twl + TWL);   // NT / 64
  const int tid = threadIdx.x, c = blockIdx.x;
  const ms_view &U = B.u[blockIdx.y];
  const int T = (int)U.rows;             // (the entry has checked rows <= L)
  const int64_t stride = cols;

  bool plain = T < 2;                    // (uniform) nothing to transform: base as it is / an invalid row
  if (FILTER) plain = plain || c < first_col || strength == 0.0;
  double zr[E];
  double mean = 0.0;
  if (!plain) {
    for (int i = tid; i < TWL; i += NT) twl[i] = twH[i];
    const double *col = U.x + c;
    const double first = col[0];
    double sum = 0.0, differ = 0.0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const int t = tid + NT * j;
      const double v = t < T ? col[t * stride] : first;
      zr[j] = v;
      sum += t < T ? v : 0.0;
      differ = v != first ? 1.0 : differ;
    }
    const double total = kwy_block_sum<NT>(sum, red);
    const double any = kwy_block_sum<NT>(differ, red);
    // a column of one repeated value: that value (kwy_gv.hip), and then M2 == 0 exactly
    mean = any == 0.0 ? first : total / (double)T;
    double m2 = 0.0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const int t = tid + NT * j;
      zr[j] = t < T ? zr[j] - mean : 0.0;
      m2 += zr[j] * zr[j];
    }
    plain = kwy_block_sum<NT>(m2, red) == 0.0;
  }
  if (plain) {
    if (FILTER) {
      if (U.out != U.base)
        for (int t = tid; t < T; t += NT) U.out[t * stride + c] = U.base[t * stride + c];
    } else {
      double *row = U.out + (int64_t)c * K;
      for (int f = tid; f < K; f += NT) row[f] = 0.0;
      if (tid == 0) U.status[c] = 0;
    }
    return;
  }

  double *A = (double *)z;
#pragma unroll
  for (int j = 0; j < E; ++j) A[tid + NT * j] = zr[j];
  __syncthreads();
  const kwy_c twb = twN[tid];
  kwy_rfft_inplace<LOG2H, NT>(z, twl, twP, twb, twN);

  if (!FILTER) {
    double *row = U.out + (int64_t)c * K;
    for (int f = tid; f < K; f += NT) {
      const kwy_c Z = z[f];
      row[f] = log(fmax(Z.x * Z.x + Z.y * Z.y, DBL_MIN) / (double)T);
    }
    if (tid == 0) U.status[c] = 1;
    return;
  }

  // ---- per-bin gain (bin 0 stays: after the mean removal it holds rounding noise only)
  double bad = 0.0;
  for (int f = 1 + tid; f < K; f += NT) {
    const kwy_c Z = z[f];
    const double s = log(fmax(Z.x * Z.x + Z.y * Z.y, DBL_MIN) / (double)T);
    const double *__restrict__ g3 = statsG + 3 * ((int64_t)c * K + f), *__restrict__ n3 = statsN + 3 * ((int64_t)c * K + f);
    const double nG = g3[0], muG = g3[1], nN = n3[0], muN = n3[1];
    double g = 1.0;
    bool ok = nG >= 2.0 && nN >= 2.0 && kwy_finite(muG) && kwy_finite(muN);
    if (ok) {
      const double sG = sqrt(g3[2] / nG), sN = sqrt(n3[2] / nN);
      ok = kwy_finite(sG) && sG > 0.0 && kwy_finite(sN) && sN >= 0.0;
      if (ok) {
        const double sp = (1.0 - strength) * s + strength * (sN / sG * (s - muG) + muN);
        g = exp((sp - s) / 2.0);
        ok = kwy_finite(g);
      }
    }
    if (!ok) {
      g = 1.0;
      bad += 1.0;
    }
    z[f] = {Z.x * g, Z.y * g};
  }
  const double nbad = kwy_block_sum<NT>(bad, red);
  if (tid == 0 && U.status && nbad > 0.0) atomicAdd(U.status, (int)nbad);

  kwy_irfft_inplace<LOG2H, NT>(z, twl, twP, twb, twN);      // (opens with a barrier) N times the signal
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int t = tid + NT * j;
    if (t < T) U.out[t * stride + c] = U.base[t * stride + c] + (A[t] / (double)N - zr[j]);
  }
}

// Welford's update of (n, mean, M2) per (column, bin >= 1) over the block's valid rows, in index order
__global__ __launch_bounds__(KWY_THREADS) void k_ms_stats(double *__restrict__ acc, const double *__restrict__ spectra,
                                                          const int32_t *__restrict__ valid, int count, int cols, int K) {
  const int i = blockIdx.x * KWY_THREADS + threadIdx.x;
  if (i >= cols * K) return;
  const int c = i / K, f = i - c * K;
  if (f == 0) return;
  double n = acc[3 * i], m = acc[3 * i + 1], m2 = acc[3 * i + 2];
  for (int u = 0; u < count; ++u) {
    if (!valid[(int64_t)u * cols + c]) continue;
    const double s = spectra[((int64_t)u * cols + c) * K + f];
    n += 1.0;
    const double d = s - m;
    m += d / n;
    m2 += d * (s - m);
  }
  acc[3 * i] = n;
  acc[3 * i + 1] = m;
  acc[3 * i + 2] = m2;
}

// ---------------------------------------------------------------------------------------------------- launches
static int ms_check_shape(kwy_ctx *ctx, int cols, int L, const char *what, int *log2h) {
  if (cols < 1 || cols > MS_MAX_COLS) {
    ctx->err = std::string(what) + ": cols must be within [1, 64]";
    return KWY_EINVAL;
  }
  const int l = kwy_ilog2(L > 0 ? L : 1);
  if (L < 512 || L > 8192 || (1 << l) != L) {
    ctx->err = std::string(what) + ": L must be a power of two in [512, 8192]";
    return KWY_EINVAL;
  }
  *log2h = l - 1;
  return KWY_OK;
}

static int ms_check_rows(kwy_ctx *ctx, int64_t rows, int L, const char *what) {
  if (rows > L) {
    ctx->err = std::string(what) + ": a matrix of T = " + std::to_string((long long)rows) +
               " rows is longer than the transform length L = " + std::to_string(L);
    return KWY_EINVAL;
  }
  return KWY_OK;
}

template <int LOG2H, bool FILTER>
static int ms_launch_as(kwy_ctx *ctx, const ms_views &B, int cols, int first_col, const double *statsG,
                        const double *statsN, double strength) {
  constexpr int NT = ms_cfg<LOG2H>::NT, H = 1 << LOG2H;
  const kwy_c *twH, *twN, *twP;
  KWY_TRY(kwy_get_twiddles(ctx, LOG2H, &twH));
  KWY_TRY(kwy_get_twiddle_powers(ctx, LOG2H, &twP));
  KWY_TRY(kwy_get_twiddles(ctx, LOG2H + 1, &twN));
  const size_t lds = sizeof(kwy_c) * ((H + 1) + H / 8) + sizeof(double) * 16;
  int64_t &raised = ctx->i_vals[std::string("ms_lds_") + std::to_string(2 * LOG2H + FILTER)];
  if (lds > 65536 && !raised) {          // (only L = 8192 asks for more than a launch gets by default: once per context)
    KWY_HIP(hipFuncSetAttribute((const void *)k_ms<LOG2H, FILTER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = 1;
  }
  KWY_PROF(ctx, FILTER ? "k_ms_filter" : "k_ms_logspectra",
           hipLaunchKernelGGL((k_ms<LOG2H, FILTER>), dim3((unsigned)cols, (unsigned)B.n), dim3(NT), lds, ctx->stream, B,
                              cols, first_col, statsG, statsN, strength, twH, twP, twN));
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

template <bool FILTER>
static int ms_launch(kwy_ctx *ctx, int log2h, const ms_views &B, int cols, int first_col, const double *statsG,
                     const double *statsN, double strength) {
  switch (log2h) {
    case 8: return ms_launch_as<8, FILTER>(ctx, B, cols, first_col, statsG, statsN, strength);
    case 9: return ms_launch_as<9, FILTER>(ctx, B, cols, first_col, statsG, statsN, strength);
    case 10: return ms_launch_as<10, FILTER>(ctx, B, cols, first_col, statsG, statsN, strength);
    case 11: return ms_launch_as<11, FILTER>(ctx, B, cols, first_col, statsG, statsN, strength);
    default: return ms_launch_as<12, FILTER>(ctx, B, cols, first_col, statsG, statsN, strength);
  }
}

// ------------------------------------------------------------------------------------------------ log-spectra
static int ms_check_mats(kwy_ctx *ctx, const kwy_gv_matrix *mats, int count, int cols, int L, const double *spectra,
                         const int32_t *valid, int *log2h) {
  KWY_TRY(ms_check_shape(ctx, cols, L, "ms_logspectra", log2h));
  if (!mats || count < 1 || !spectra || !valid) { ctx->err = "ms_logspectra: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i) {
    if (mats[i].rows < 0 || (mats[i].rows > 0 && !mats[i].x)) { ctx->err = "ms_logspectra: bad argument"; return KWY_EINVAL; }
    KWY_TRY(ms_check_rows(ctx, mats[i].rows, L, "ms_logspectra"));
  }
  return KWY_OK;
}

static int ms_launch_logspectra(kwy_ctx *ctx, int log2h, const kwy_gv_matrix *mats, int count, int cols, double *spectra,
                                int32_t *valid) {
  const int64_t K = (1 << log2h) + 1;
  return kwy_for_tables<ms_views>(
      count,
      [&](int i) {
        return ms_view{mats[i].x, mats[i].rows, nullptr, spectra + (int64_t)i * cols * K, valid + (int64_t)i * cols};
      },
      [&](const ms_views &B, int) { return ms_launch<false>(ctx, log2h, B, cols, 0, nullptr, nullptr, 0.0); });
}

extern "C" int kwy_ms_logspectra_batch_dev(kwy_ctx *ctx, const kwy_gv_matrix *mats, int count, int cols, int L,
                                           double *spectra, int32_t *valid) {
  if (!ctx) return KWY_EINVAL;
  int log2h;
  KWY_TRY(ms_check_mats(ctx, mats, count, cols, L, spectra, valid, &log2h));
  KWY_HIP(hipSetDevice(ctx->device));
  return ms_launch_logspectra(ctx, log2h, mats, count, cols, spectra, valid);
}

extern "C" int kwy_ms_logspectra(kwy_ctx *ctx, const kwy_gv_matrix *mats, int count, int cols, int L, double *spectra,
                                 int32_t *valid) {
  if (!ctx) return KWY_EINVAL;
  int log2h;
  KWY_TRY(ms_check_mats(ctx, mats, count, cols, L, spectra, valid, &log2h));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "ms_logspectra");
  double *ds;
  int32_t *dv;
  st.out(ds, spectra, (size_t)count * cols * (L / 2 + 1));
  st.out(dv, valid, (size_t)count * cols);
  std::vector<kwy_gv_matrix> staged(mats, mats + count);
  for (int i = 0; i < count; ++i) st.in(staged[i].x, mats[i].x, (size_t)mats[i].rows * cols);
  KWY_TRY(st.begin());
  KWY_TRY(ms_launch_logspectra(ctx, log2h, staged.data(), count, cols, ds, dv));
  return st.finish();
}

// ------------------------------------------------------------------------------------------------- statistics
static int ms_check_stats(kwy_ctx *ctx, const double *acc, const double *spectra, const int32_t *valid, int count,
                          int cols, int L, int *log2h) {
  KWY_TRY(ms_check_shape(ctx, cols, L, "ms_stats_update", log2h));
  if (!acc || !spectra || !valid || count < 1) { ctx->err = "ms_stats_update: bad argument"; return KWY_EINVAL; }
  return KWY_OK;
}

static int ms_launch_stats(kwy_ctx *ctx, double *acc, const double *spectra, const int32_t *valid, int count, int cols,
                           int L) {
  const int K = L / 2 + 1, blocks = (cols * K + KWY_THREADS - 1) / KWY_THREADS;
  KWY_PROF(ctx, "k_ms_stats", hipLaunchKernelGGL(k_ms_stats, dim3((unsigned)blocks), dim3(KWY_THREADS), 0, ctx->stream,
                                                 acc, spectra, valid, count, cols, K));
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

extern "C" int kwy_ms_stats_update_dev(kwy_ctx *ctx, double *acc, const double *spectra, const int32_t *valid, int count,
                                       int cols, int L) {
  if (!ctx) return KWY_EINVAL;
  int log2h;
  KWY_TRY(ms_check_stats(ctx, acc, spectra, valid, count, cols, L, &log2h));
  KWY_HIP(hipSetDevice(ctx->device));
  return ms_launch_stats(ctx, acc, spectra, valid, count, cols, L);
}

extern "C" int kwy_ms_stats_update(kwy_ctx *ctx, double *acc, const double *spectra, const int32_t *valid, int count,
                                   int cols, int L) {
  if (!ctx) return KWY_EINVAL;
  int log2h;
  KWY_TRY(ms_check_stats(ctx, acc, spectra, valid, count, cols, L, &log2h));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "ms_stats_update");
  double *da, *ds;
  int32_t *dv;
  st.inout(da, acc, 3 * (size_t)cols * (L / 2 + 1));
  st.in(ds, spectra, (size_t)count * cols * (L / 2 + 1));
  st.in(dv, valid, (size_t)count * cols);
  KWY_TRY(st.begin());
  KWY_TRY(ms_launch_stats(ctx, da, ds, dv, count, cols, L));
  return st.finish();
}

// ----------------------------------------------------------------------------------------------------- filter
static int ms_check_jobs(kwy_ctx *ctx, const kwy_ms_job *jobs, int count, int cols, int first_col, int L,
                         const double *statsG, const double *statsN, double strength, int *log2h) {
  KWY_TRY(ms_check_shape(ctx, cols, L, "ms_postfilter", log2h));
  if (!(strength >= 0.0 && strength <= 1.0)) {
    ctx->err = "ms_postfilter: strength must be within [0, 1]";
    return KWY_EINVAL;
  }
  if (!jobs || count < 1 || !statsG || !statsN || first_col < 0 || first_col > cols) {
    ctx->err = "ms_postfilter: bad argument";
    return KWY_EINVAL;
  }
  for (int i = 0; i < count; ++i) {
    if (jobs[i].rows < 0 || (jobs[i].rows > 0 && (!jobs[i].x || !jobs[i].base || !jobs[i].out))) {
      ctx->err = "ms_postfilter: bad argument";
      return KWY_EINVAL;
    }
    KWY_TRY(ms_check_rows(ctx, jobs[i].rows, L, "ms_postfilter"));
  }
  return KWY_OK;
}

static int ms_launch_filter(kwy_ctx *ctx, int log2h, const kwy_ms_job *jobs, int count, int cols, int first_col,
                            const double *statsG, const double *statsN, double strength, int32_t *status) {
  if (status) KWY_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)count, ctx->stream));
  return kwy_for_tables<ms_views>(
      count,
      [&](int i) {
        const kwy_ms_job &j = jobs[i];
        return ms_view{j.x, j.rows, j.base, j.out, status ? status + i : nullptr};
      },
      [&](const ms_views &B, int) { return ms_launch<true>(ctx, log2h, B, cols, first_col, statsG, statsN, strength); });
}

extern "C" int kwy_ms_postfilter_batch_dev(kwy_ctx *ctx, const kwy_ms_job *jobs, int count, int cols, int first_col,
                                           int L, const double *statsG, const double *statsN, double strength,
                                           int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  int log2h;
  KWY_TRY(ms_check_jobs(ctx, jobs, count, cols, first_col, L, statsG, statsN, strength, &log2h));
  KWY_HIP(hipSetDevice(ctx->device));
  return ms_launch_filter(ctx, log2h, jobs, count, cols, first_col, statsG, statsN, strength, status);
}

extern "C" int kwy_ms_postfilter_dev(kwy_ctx *ctx, const double *x, int64_t rows, int cols, int first_col, int L,
                                     const double *statsG, const double *statsN, double strength, const double *base,
                                     double *out, int32_t *status) {
  const kwy_ms_job one = {x, rows, base, out};
  return kwy_ms_postfilter_batch_dev(ctx, &one, 1, cols, first_col, L, statsG, statsN, strength, status);
}

extern "C" int kwy_ms_postfilter(kwy_ctx *ctx, const kwy_ms_job *jobs, int count, int cols, int first_col, int L,
                                 const double *statsG, const double *statsN, double strength, int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  int log2h;
  KWY_TRY(ms_check_jobs(ctx, jobs, count, cols, first_col, L, statsG, statsN, strength, &log2h));
  KWY_HIP(hipSetDevice(ctx->device));
  const size_t na = 3 * (size_t)cols * (L / 2 + 1);
  kwy_staging st(ctx, "ms_postfilter");
  double *dG, *dN;
  int32_t *dstatus;
  st.in(dG, statsG, na);
  st.in(dN, statsN, na);
  st.out(dstatus, status, (size_t)count);
  std::vector<kwy_ms_job> staged(jobs, jobs + count);
  for (int i = 0; i < count; ++i) {
    const size_t n = (size_t)jobs[i].rows * cols;
    st.in(staged[i].x, jobs[i].x, n);
    if (jobs[i].base != jobs[i].x) st.in(staged[i].base, jobs[i].base, n);
    st.out(staged[i].out, jobs[i].out, n);
  }
  KWY_TRY(st.begin());
  for (int i = 0; i < count; ++i)
    if (jobs[i].base == jobs[i].x) staged[i].base = staged[i].x;
  KWY_TRY(ms_launch_filter(ctx, log2h, staged.data(), count, cols, first_col, dG, dN, strength, dstatus));
  return st.finish();
}
