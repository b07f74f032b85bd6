// kwy_mcpower.hip -- the energy of a mel-cepstrum without its spectrum, and the two repairs that need it: the
// formant-emphasis postfilter (beta) and the power-preserving shift of c0.
//
//   w~_k = w_k + 2 atan2(alpha sin w_k, 1 - alpha cos w_k),  w_k = 2 pi k / N            (as kwy_fftfilt.hip)
//   L_k  = sum_{m = 0 .. order} c[m] cos(m w~_k),  m ascending
//   E(c) = ( exp(2 L_0) + exp(2 L_{N/2}) + 2 sum_{k = 1 .. N/2 - 1} exp(2 L_k) ) / N
//   y    = x through mc2b, b[1] -= beta alpha b[2], b[2..] *= 1 + beta, and back;  y[0] += log(E(ref) / E(y)) / 2
// include/kwy.h ("mel-cepstral energy") has the contract in full.  There is no reference call to cite: the reference
// synthesises the converter's output as it is (kwiiyatta/convert_voice.py:35-46).
//
// One workgroup takes MP_ROWS rows of one matrix at a time: their reference rows and their filtered rows are MP_NV
// coefficient vectors in LDS, read at wave-uniform addresses, and every element of the cosine table a lane loads
// serves all MP_NV of them from a register.  A lane takes up to four bins at a time, so that a coefficient read from
// LDS serves four products: with one bin per read the LDS port, not the f64 pipe, sets the time.  The bins run across the lanes; a lane adds its bins in index order, the
// lanes are summed by kwy_wave_sum and the wavefronts in index order, so a row's energy depends on its coefficients,
// alpha, N and order alone -- not on the run, on its neighbours in the workgroup, or on the batch.  Nothing is
// accumulated in memory: a workgroup writes the number of rows it left unfiltered into a slot of its own, and a second
// small kernel adds a matrix's slots into its status word.
//
// The _dev entries allocate nothing and do not synchronise once the context holds the table of (N, alpha, order) and the
// count slots (the first call makes them): they are legal inside a stream capture from then on.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "kwy_internal.hpp"

#define MP_ROWS 4                // rows of a matrix per workgroup and step (KWY_THREADS / MP_LD)
#define MP_NV 8                  // coefficient vectors per step: (reference, filtered) of MP_ROWS rows, or MP_NV rows
#define MP_LD 64                 // doubles between two vectors in LDS (order <= 63)
#define MP_JOBS_MAX 64           // matrices per launch
#define MP_JOB_BLOCKS 1024       // workgroups per matrix; they stride over its rows
#define MP_SLOTS (MP_JOBS_MAX * MP_JOB_BLOCKS)

static_assert(MP_ROWS * MP_LD == KWY_THREADS, "one thread per (row, coefficient) of a step");

struct mp_job {
  const double *x;
  const double *ref;     // or null
  const double *base;    // or null
  double *out;
  int64_t rows;
};
typedef kwy_batch<mp_job, MP_JOBS_MAX> mp_jobs;
static_assert(sizeof(mp_jobs) + 48 <= KWY_KERNARG_MAX, "k_mcpower_filter: the table and six scalar arguments");
// the table's start[] alone for k_mcpower_status: a kernel that took the whole mp_jobs would find start[] four bytes
// further on and get 2.8 KB of arguments for 260 bytes it reads
struct mp_starts {
  int start[MP_JOBS_MAX + 1];
};

// the energies of the MP_NV vectors in coef (coefficient m of vector v at coef[m * MP_NV + v]) into Es; red:
// MP_NV (KWY_WAVES + 1) doubles.  A thread takes BPT bins at a time (H is a multiple of KWY_THREADS * BPT), so that a
// coefficient read from LDS serves BPT products; its bins are added in index order whatever BPT is.  Bin N/2 is left
// to the MP_NV threads that fold the wavefronts' sums, one vector each.  Ends on a barrier; every thread may read Es
// afterwards.
template <int BPT>
__device__ __forceinline__ void mp_energies(const double *coef, int order, int H, const double *__restrict__ tab,
                                            double *red, double *Es) {
  const int tid = threadIdx.x;
  const size_t ld = (size_t)(H + 1);
  double s[MP_NV], first[MP_NV];
#pragma unroll
  for (int v = 0; v < MP_NV; ++v) s[v] = first[v] = 0.0;
  for (int k0 = tid; k0 < H; k0 += KWY_THREADS * BPT) {
    double L[BPT][MP_NV];
#pragma unroll
    for (int j = 0; j < BPT; ++j)
#pragma unroll
      for (int v = 0; v < MP_NV; ++v) L[j][v] = 0.0;
    const double *t = tab + k0;
    for (int m = 0; m <= order; ++m) {
      double c[BPT];
#pragma unroll
      for (int j = 0; j < BPT; ++j) c[j] = t[m * ld + j * KWY_THREADS];
#pragma unroll
      for (int v = 0; v < MP_NV; ++v) {
        const double a = coef[m * MP_NV + v];
#pragma unroll
        for (int j = 0; j < BPT; ++j) L[j][v] += a * c[j];
      }
    }
#pragma unroll
    for (int j = 0; j < BPT; ++j)
#pragma unroll
      for (int v = 0; v < MP_NV; ++v) {
        const double p = exp(2.0 * L[j][v]);
        if (k0 + j == 0) first[v] = p;       // bin 0: thread 0's first
        else s[v] += p;
      }
  }
#pragma unroll
  for (int v = 0; v < MP_NV; ++v) s[v] = kwy_wave_sum(s[v]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int v = 0; v < MP_NV; ++v) {
      red[v * KWY_WAVES + (tid >> 6)] = s[v];
      if (tid == 0) red[MP_NV * KWY_WAVES + v] = first[v];
    }
  }
  __syncthreads();
  if (tid < MP_NV) {
    double last = 0.0;
    for (int m = 0; m <= order; ++m) last += coef[m * MP_NV + tid] * tab[m * ld + H];
    const double *a = red + tid * KWY_WAVES;
    double S = a[0];
#pragma unroll
    for (int w = 1; w < KWY_WAVES; ++w) S += a[w];
    Es[tid] = ((red[MP_NV * KWY_WAVES + tid] + exp(2.0 * last)) + 2.0 * S) / (double)(2 * H);
  }
  __syncthreads();
}


template <int BPT>
__global__ __launch_bounds__(KWY_THREADS) void k_mcpower_filter(mp_jobs J, int order, double alpha, double beta, int H,
                                                                 const double *__restrict__ tab, int32_t *counts) {
  __shared__ double coef[MP_NV * MP_LD];      // vector 2 r: the reference of row r, 2 r + 1: its filtered row
  __shared__ double red[MP_NV * (KWY_WAVES + 1)];
  __shared__ double Es[MP_NV];
  const int tid = threadIdx.x, r = tid / MP_LD, m = tid % MP_LD;
  int u = 0;
  while (u + 1 < J.n && (int)blockIdx.x >= J.start[u + 1]) ++u;   // uniform: a scalar loop
  const mp_job &U = J.u[u];
  const int64_t rows = U.rows;
  const int cols = order + 1;
  const int64_t g = (int)blockIdx.x - J.start[u], G = J.start[u + 1] - J.start[u];
  const bool copy = beta == 0.0 && !U.ref;
  int bad = 0;
  for (int64_t r0 = g * MP_ROWS; r0 < rows; r0 += G * MP_ROWS) {
    const bool row_live = r0 + r < rows, live = row_live && m < cols;
    const int64_t at = (r0 + r) * cols + m;
    const double xv = live ? U.x[at] : 0.0;
    const double bv = live && U.base ? U.base[at] : 0.0;
    double ov = U.base ? bv : xv;
    bool failed = false;
    if (!copy) {       // (uniform)
      coef[m * MP_NV + 2 * r] = live && U.ref ? U.ref[at] : xv;
      coef[m * MP_NV + 2 * r + 1] = xv;
      __syncthreads();
      if (beta != 0.0 && tid < MP_ROWS) {
        double *c = coef + 2 * tid + 1;        // (its coefficients MP_NV apart)
        double nx = c[order * MP_NV];          // b[m + 1]
        for (int q = order - 1; q >= 0; --q) {
          nx = c[q * MP_NV] - alpha * nx;
          c[q * MP_NV] = nx;
        }
        if (order >= 2) {
          c[MP_NV] = c[MP_NV] - (beta * alpha) * c[2 * MP_NV];
          for (int q = 2; q <= order; ++q) c[q * MP_NV] = c[q * MP_NV] * (1.0 + beta);
        }
        for (int q = 0; q < order; ++q) c[q * MP_NV] = c[q * MP_NV] + alpha * c[(q + 1) * MP_NV];
      }
      __syncthreads();
      mp_energies<BPT>(coef, order, H, tab, red, Es);
      const double corr = log(Es[2 * r] / Es[2 * r + 1]) / 2.0;
      failed = !(kwy_finite_pos(Es[2 * r]) && kwy_finite_pos(Es[2 * r + 1]) && kwy_finite(corr));
      if (!failed) {
        double yv = coef[m * MP_NV + 2 * r + 1];
        if (m == 0) yv = yv + corr;
        ov = U.base ? bv + (yv - xv) : yv;
      }
    }
    if (live) U.out[at] = ov;
    bad += __syncthreads_count(failed && row_live && m == 0);     // (and the barrier before coef is written again)
  }
  if (counts && tid == 0) counts[blockIdx.x] = bad;
}

// block u: status[u] = the sum of the count slots of job u's workgroups
__global__ __launch_bounds__(KWY_THREADS) void k_mcpower_status(mp_starts S, const int32_t *__restrict__ counts,
                                                                 int32_t *__restrict__ status) {
  __shared__ int part[KWY_THREADS];
  const int tid = threadIdx.x, u = blockIdx.x;
  int s = 0;
  for (int i = S.start[u] + tid; i < S.start[u + 1]; i += KWY_THREADS) s += counts[i];
  part[tid] = s;
  __syncthreads();
  for (int h = KWY_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) part[tid] += part[tid + h];
    __syncthreads();
  }
  if (tid == 0) status[u] = part[0];
}

// MP_NV rows per step; job.out: one double per row
template <int BPT>
__global__ __launch_bounds__(KWY_THREADS) void k_mcpower_energy(mp_jobs J, int order, int H,
                                                                 const double *__restrict__ tab) {
  __shared__ double coef[MP_NV * MP_LD];
  __shared__ double red[MP_NV * (KWY_WAVES + 1)];
  __shared__ double Es[MP_NV];
  const int tid = threadIdx.x;
  int u = 0;
  while (u + 1 < J.n && (int)blockIdx.x >= J.start[u + 1]) ++u;
  const mp_job &U = J.u[u];
  const int64_t rows = U.rows;
  const int cols = order + 1;
  const int64_t g = (int)blockIdx.x - J.start[u], G = J.start[u + 1] - J.start[u];
  for (int64_t r0 = g * MP_NV; r0 < rows; r0 += G * MP_NV) {
    for (int i = tid; i < MP_NV * MP_LD; i += KWY_THREADS) {
      const int r = i / MP_LD, m = i % MP_LD;
      coef[m * MP_NV + r] = (r0 + r < rows && m < cols) ? U.x[(r0 + r) * cols + m] : 0.0;
    }
    __syncthreads();
    mp_energies<BPT>(coef, order, H, tab, red, Es);
    if (tid < MP_NV && r0 + tid < rows) U.out[r0 + tid] = Es[tid];
    __syncthreads();
  }
}

// cos(m w~_k), m <= order, k <= N/2, row m contiguous in k: one table per (N, alpha, order)
static int mp_table(kwy_ctx *ctx, int N, double alpha, int order, const double **out) {
  char key[112];
  snprintf(key, sizeof(key), "mcpower_cos:%d:%.17g:%d", N, alpha, order);
  return kwy_cached_table<double>(ctx, key, [&] {
    const int H = N / 2;
    std::vector<double> h((size_t)(order + 1) * (H + 1));
    for (int k = 0; k <= H; ++k) {
      const double w = 2.0 * M_PI * (double)k / (double)N;
      const double wt = w + 2.0 * atan2(alpha * sin(w), 1.0 - alpha * cos(w));
      for (int m = 0; m <= order; ++m) h[(size_t)m * (H + 1) + k] = cos((double)m * wt);
    }
    return h;
  }, out);
}

// one slot per workgroup of a launch (every launch writes the slots it reads: the initial values are never used)
static int mp_slots(kwy_ctx *ctx, int32_t **out) {
  const int32_t *p;
  KWY_TRY(kwy_cached_table<int32_t>(ctx, "mcpower_slots", [] { return std::vector<int32_t>(MP_SLOTS, 0); }, &p));
  *out = (int32_t *)p;
  return KWY_OK;
}

static int mp_check_common(kwy_ctx *ctx, int order, double alpha, int N, const char *what) {
  if (!ctx) return KWY_EINVAL;
  if (order < 1 || order > MP_LD - 1 || !(fabs(alpha) < 1.0) || N < 512 || N > 8192 || (N & (N - 1)) != 0) {
    ctx->err = std::string(what) + ": bad argument (order 1..63, |alpha| < 1, fft_size a power of two within [512, 8192])";
    return KWY_EINVAL;
  }
  return KWY_OK;
}

static int mp_check_filter(kwy_ctx *ctx, const kwy_mcpower_job *jobs, int count, double beta) {
  if (!(beta >= 0.0 && beta <= 1.0)) { ctx->err = "mcep_postfilter: beta must be within [0, 1]"; return KWY_EINVAL; }
  if (count < 0 || (count > 0 && !jobs)) { ctx->err = "mcep_postfilter: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i)
    if (jobs[i].rows < 0 || (jobs[i].rows > 0 && (!jobs[i].x || !jobs[i].out))) {
      ctx->err = "mcep_postfilter: bad argument (negative rows or a null pointer)";
      return KWY_EINVAL;
    }
  return KWY_OK;
}

static int mp_check_energy(kwy_ctx *ctx, const kwy_energy_job *jobs, int count) {
  if (count < 0 || (count > 0 && !jobs)) { ctx->err = "mcep_energy: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i)
    if (jobs[i].rows < 0 || (jobs[i].rows > 0 && (!jobs[i].mc || !jobs[i].energy))) {
      ctx->err = "mcep_energy: bad argument (negative rows or a null pointer)";
      return KWY_EINVAL;
    }
  return KWY_OK;
}

static inline int mp_blocks(int64_t rows, int per) {
  const int64_t b = (rows + per - 1) / per;
  return (int)(b < MP_JOB_BLOCKS ? b : MP_JOB_BLOCKS);
}

// the jobs (all of them checked already) in launches of <= MP_JOBS_MAX matrices
static int mp_run_filter(kwy_ctx *ctx, const kwy_mcpower_job *jobs, int count, int order, double alpha, int N,
                         double beta, int32_t *status) {
  KWY_HIP(hipSetDevice(ctx->device));
  const double *tab;
  int32_t *slots = nullptr;
  KWY_TRY(mp_table(ctx, N, alpha, order, &tab));
  if (status) KWY_TRY(mp_slots(ctx, &slots));
  return kwy_for_tables<mp_jobs>(
      count,
      [&](int i, int &blocks) {
        const kwy_mcpower_job &q = jobs[i];
        blocks = mp_blocks(q.rows, MP_ROWS);
        return mp_job{q.x, q.ref, q.base, q.out, q.rows};
      },
      [&](const mp_jobs &J, int i0) {
        if (J.start[J.n] > 0) {
          auto k = N >= 2048 ? k_mcpower_filter<4> : N == 1024 ? k_mcpower_filter<2> : k_mcpower_filter<1>;
          KWY_PROF(ctx, "k_mcpower_filter", hipLaunchKernelGGL(k, dim3((unsigned)J.start[J.n]), dim3(KWY_THREADS), 0,
                                                               ctx->stream, J, order, alpha, beta, N / 2, tab, slots));
          KWY_HIP(hipGetLastError());
        }
        if (status) {
          mp_starts S;
          memcpy(S.start, J.start, sizeof(S.start));
          KWY_PROF(ctx, "k_mcpower_status", hipLaunchKernelGGL(k_mcpower_status, dim3(J.n), dim3(KWY_THREADS), 0,
                                                               ctx->stream, S, slots, status + i0));
          KWY_HIP(hipGetLastError());
        }
        return KWY_OK;
      });
}

static int mp_run_energy(kwy_ctx *ctx, const kwy_energy_job *jobs, int count, int order, double alpha, int N) {
  KWY_HIP(hipSetDevice(ctx->device));
  const double *tab;
  KWY_TRY(mp_table(ctx, N, alpha, order, &tab));
  return kwy_for_tables<mp_jobs>(
      count,
      [&](int i, int &blocks) {
        const kwy_energy_job &q = jobs[i];
        blocks = mp_blocks(q.rows, MP_NV);
        return mp_job{q.mc, nullptr, nullptr, q.energy, q.rows};
      },
      [&](const mp_jobs &J, int) {
        if (J.start[J.n] == 0) return KWY_OK;
        auto k = N >= 2048 ? k_mcpower_energy<4> : N == 1024 ? k_mcpower_energy<2> : k_mcpower_energy<1>;
        KWY_PROF(ctx, "k_mcpower_energy", hipLaunchKernelGGL(k, dim3((unsigned)J.start[J.n]), dim3(KWY_THREADS), 0,
                                                             ctx->stream, J, order, N / 2, tab));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

extern "C" int kwy_mcep_energy_batch_dev(kwy_ctx *ctx, const kwy_energy_job *jobs, int count, int order, double alpha,
                                         int fft_size) {
  KWY_TRY(mp_check_common(ctx, order, alpha, fft_size, "mcep_energy"));
  KWY_TRY(mp_check_energy(ctx, jobs, count));
  if (count == 0) return KWY_OK;
  return mp_run_energy(ctx, jobs, count, order, alpha, fft_size);
}

extern "C" int kwy_mcep_energy_dev(kwy_ctx *ctx, const double *mc, int64_t T, int order, double alpha, int fft_size,
                                   double *energy) {
  const kwy_energy_job one = {mc, T, energy};
  return kwy_mcep_energy_batch_dev(ctx, &one, 1, order, alpha, fft_size);
}

extern "C" int kwy_mcep_energy(kwy_ctx *ctx, const double *mc, int64_t T, int order, double alpha, int fft_size,
                               double *energy) {
  KWY_TRY(mp_check_common(ctx, order, alpha, fft_size, "mcep_energy"));
  kwy_energy_job q = {mc, T, energy};
  KWY_TRY(mp_check_energy(ctx, &q, 1));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "mcep_energy");
  st.in(q.mc, mc, (size_t)T * (order + 1));
  st.out(q.energy, energy, (size_t)T);
  KWY_TRY(st.begin());
  KWY_TRY(mp_run_energy(ctx, &q, 1, order, alpha, fft_size));
  return st.finish();
}

extern "C" int kwy_mcep_postfilter_batch_dev(kwy_ctx *ctx, const kwy_mcpower_job *jobs, int count, int order,
                                             double alpha, int fft_size, double beta, int32_t *status) {
  KWY_TRY(mp_check_common(ctx, order, alpha, fft_size, "mcep_postfilter"));
  KWY_TRY(mp_check_filter(ctx, jobs, count, beta));
  if (count == 0) return KWY_OK;
  return mp_run_filter(ctx, jobs, count, order, alpha, fft_size, beta, status);
}

extern "C" int kwy_mcep_postfilter_dev(kwy_ctx *ctx, const double *x, int64_t rows, int order, double alpha,
                                       int fft_size, double beta, const double *ref, const double *base, double *out,
                                       int32_t *status) {
  const kwy_mcpower_job one = {x, ref, base, out, rows};
  return kwy_mcep_postfilter_batch_dev(ctx, &one, 1, order, alpha, fft_size, beta, status);
}

extern "C" int kwy_mcep_postfilter(kwy_ctx *ctx, const kwy_mcpower_job *jobs, int count, int order, double alpha,
                                   int fft_size, double beta, int32_t *status) {
  KWY_TRY(mp_check_common(ctx, order, alpha, fft_size, "mcep_postfilter"));
  KWY_TRY(mp_check_filter(ctx, jobs, count, beta));
  if (count == 0) return KWY_OK;
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "mcep_postfilter");
  int32_t *dstatus;
  st.out(dstatus, status, (size_t)count);
  std::vector<kwy_mcpower_job> staged(jobs, jobs + count);
  for (int i = 0; i < count; ++i) {
    const size_t n = (size_t)jobs[i].rows * (order + 1);
    st.in(staged[i].x, jobs[i].x, n);
    if (jobs[i].ref) st.in(staged[i].ref, jobs[i].ref, n);
    if (jobs[i].base && jobs[i].base != jobs[i].x) st.in(staged[i].base, jobs[i].base, n);
    st.out(staged[i].out, jobs[i].out, n);
  }
  KWY_TRY(st.begin());
  for (int i = 0; i < count; ++i)
    if (jobs[i].base == jobs[i].x) staged[i].base = staged[i].x;
  KWY_TRY(mp_run_filter(ctx, staged.data(), count, order, alpha, fft_size, beta, status ? dstatus : nullptr));
  return st.finish();
}
