// kwy_internal.hpp -- host-side internals of libkwy.so (context, scratch arena,
// constant tables).  Not part of the ABI (see include/kwy.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/kwy.h"
#include "kwy_fft.hpp"      // (and kwy_device.hpp through it: kwy_c is the element type of the twiddle tables)

struct kwy_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;

  // scratch arena (grow-only bump allocator, reset at the start of every call)
  char *arena = nullptr;
  size_t arena_cap = 0, arena_off = 0;
  int64_t arena_generation = 0;            // counts (re)allocations: a captured HIP graph holds arena addresses

  // constant tables
  uint4 *d_pow2 = nullptr;                 // [64][128] columns of T^(2^k)
  const uint32_t *d_randn = nullptr;       // the device's table of WORLD's randn stream (shared by all contexts)
  uint64_t randn_n = 0;                    // draws of it this context uses (kwy_ctx_set_randn_limit lowers it)
  kwy_c *d_tw[20] = {nullptr};             // d_tw[l]: exp(-2 pi i k / 2^l), k < 2^l
  kwy_c *d_twp[20] = {nullptr};            // d_twp[l]: powers of the stride-64 pass factors of a 2^l-point transform
  std::map<uint64_t, uint4 *> d_poly;      // stride(steps) -> x^(stride*t) mod P, t < 256
  std::map<std::string, void *> d_mats;    // cached host-built tables (kwy_cached_table)
  std::map<std::string, int64_t> i_vals;   // small cached integers that go with them

  // optional per-kernel timing with HIP events on this context's stream
  void *dbg = nullptr;  // optional device buffer for in-kernel cycle stamps (diagnostic builds)
  bool prof = false;
  std::map<std::string, std::vector<std::pair<hipEvent_t, hipEvent_t>>> prof_events;
};

#define KWY_HIP(call)                                                              \
  do {                                                                             \
    hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess) {                                                        \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                \
      return e_ == hipErrorOutOfMemory ? KWY_ENOMEM : KWY_EHIP;                    \
    }                                                                              \
  } while (0)

#define KWY_TRY(call)              \
  do {                             \
    int rc_ = (call);              \
    if (rc_ != KWY_OK) return rc_; \
  } while (0)

// --- profiling ---------------------------------------------------------------
// KWY_PROF(ctx, "kernel", launch-statement): brackets the launch with two HIP
// events when profiling is on (kwy_ctx_profile); otherwise just launches.
struct kwy_prof_scope {
  kwy_ctx *ctx;
  hipEvent_t a = nullptr, b = nullptr;
  const char *name;
  kwy_prof_scope(kwy_ctx *c, const char *n) : ctx(c), name(n) {
    if (ctx->prof) {
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
      (void)hipEventRecord(a, ctx->stream);
    }
  }
  ~kwy_prof_scope() {
    if (a && b) {
      (void)hipEventRecord(b, ctx->stream);
      ctx->prof_events[name].push_back({a, b});
    }
  }
};
#define KWY_PROF(ctx, name, stmt) do { kwy_prof_scope ps_(ctx, name); stmt; } while (0)

// --- arena ------------------------------------------------------------------
// Reserve `bytes` of scratch for the current call (must be called once, before
// any kwy_arena_alloc of the call); grows the arena if needed.
int kwy_arena_begin(kwy_ctx *ctx, size_t bytes);
void *kwy_arena_alloc(kwy_ctx *ctx, size_t bytes);
template <typename T>
static inline T *kwy_arena(kwy_ctx *ctx, size_t n) {
  return (T *)kwy_arena_alloc(ctx, n * sizeof(T));
}
static inline size_t kwy_pad(size_t b) { return (b + 255) & ~(size_t)255; }

// --- staging of the entries on host pointers ------------------------------------------
// A host entry names every buffer it stages once: in() is uploaded, out() is downloaded, inout() both (worked on in
// place on the device), tmp() is device scratch that keeps its place among them.  begin() sizes the arena for all of
// them (kwy_pad(sizeof(T) * n) each) plus `scratch` bytes the entry's core takes afterwards, takes the device pointers
// in the order of the statements, stores them where the statements said, and enqueues the uploads; finish() enqueues
// the downloads and synchronises.  A buffer of no elements is allocated (zero bytes) and never copied; neither is one
// whose host pointer is null (an optional output).  The device pointers are valid from begin() on: an alias
// (base == x) is filled in after it.
struct kwy_staging {
  kwy_ctx *ctx;
  const char *entry;   // for "<entry>: scratch arena too small"
  struct buffer { void **dev; const void *src; void *dst; size_t bytes; };
  std::vector<buffer> buffers;
  kwy_staging(kwy_ctx *c, const char *e) : ctx(c), entry(e) {}
  template <class D, class T> void in(D *&d, const T *h, size_t n) { add(d, h, nullptr, sizeof(T) * n); }
  template <class D, class T> void out(D *&d, T *h, size_t n) { add(d, nullptr, h, sizeof(T) * n); }
  template <class D, class T> void inout(D *&d, T *h, size_t n) { inout(d, h, h, n); }
  template <class D, class T> void inout(D *&d, const T *src, T *dst, size_t n) { add(d, src, dst, sizeof(T) * n); }
  template <class D> void tmp(D *&d, size_t n) { add(d, nullptr, nullptr, sizeof(D) * n); }
  // after begin(): n values of a buffer that was not staged as an output (a status word in the core's scratch or in a
  // tmp() block), downloaded by finish() with the others
  template <class D, class T> void fetch(D *&d, T *h, size_t n) { add(d, nullptr, h, sizeof(T) * n); }
  int begin(size_t scratch = 0);
  int finish();
 private:
  template <class D> void add(D *&d, const void *src, void *dst, size_t bytes) {
    buffers.push_back({(void **)&d, src, dst, bytes});
  }
};

// --- tables -----------------------------------------------------------------
// The device copy of a host-built table, made on first use (never inside a captured region) and kept in ctx->d_mats
// until the context goes: `build` returns the table as a std::vector (or a reference to one that outlives the call).
int kwy_table_upload(kwy_ctx *ctx, const std::string &key, const void *host, size_t bytes, void **out);
template <class T, class BUILD>
static inline int kwy_cached_table(kwy_ctx *ctx, const std::string &key, BUILD build, const T **out) {
  auto it = ctx->d_mats.find(key);
  if (it != ctx->d_mats.end()) { *out = (const T *)it->second; return KWY_OK; }
  const std::vector<T> &h = build();
  return kwy_table_upload(ctx, key, h.data(), sizeof(T) * h.size(), (void **)out);
}

int kwy_get_twiddles(kwy_ctx *ctx, int log2n, const kwy_c **out);
// w^1 .. w^7 of every factor w the stride-64 radix-8 pass of a 2^log2h-point LDS transform uses (kwy_fft.hpp:
// kwy_tw_powers), KWY_TWP_ENTRY complex per factor; made together with the twiddles of that length.  Transforms below
// 1024 points have no such pass: *out = NULL.
int kwy_get_twiddle_powers(kwy_ctx *ctx, int log2h, const kwy_c **out);
int kwy_get_poly(kwy_ctx *ctx, uint64_t stride_steps, const uint4 **out);
// pysptk.sp2mc's frequency transform for transform length N as a matrix [ncut][64] (kwy_mcep.hip): mc[j] = sum_n F[n][j] c[n]
int kwy_get_sp2mc_matrix(kwy_ctx *ctx, int N, int order, double alpha, const double **out, int *ncut);
// kwy_gmm_em_sums_dev whose kernels return at once when gate[0] != 0 (gate may be NULL); with `labels` the weights are
// the one-hot rows of the labels (resp is not read): kwy_gmmfit.hip
int kwy_fit_sums_gated(kwy_ctx *ctx, const double *X, int64_t n, int D, int M, const double *resp, double *stats,
                       const long long *gate, const int *labels);
// the log-sum-exp step of the E-step (k_fit_resp, kwy_gmmfit.hip): wlp (n x M) becomes the responsibilities in place,
// ll_part[ceil(n/256)] the partial sums of the frames' log-likelihoods; shared by the full and the block-diagonal E-step
int kwy_fit_resp(kwy_ctx *ctx, double *wlp, int64_t n, int M, double *ll_part);
// [max_c][nthreads] table: row c-1 holds x^(12*c*t) mod P, t < nthreads (chunk of c draws per thread)
int kwy_get_poly_multi(kwy_ctx *ctx, int max_c, int nthreads, const uint4 **out);

// the context's view of the randn stream: table, usable length, jump matrices
static inline kwy_randn_src kwy_randn(const kwy_ctx *ctx) {
  return kwy_randn_src{ctx->d_randn, ctx->randn_n, ctx->d_pow2};
}

// --- job tables ---------------------------------------------------------------------
// A batched kernel takes the views of up to N jobs (utterances, matrices, signals) per launch, and the views travel BY
// VALUE in the kernel arguments: scalar loads, no descriptor table in device memory, nothing to upload, capturable in
// HIP graphs.  A launch's whole argument block must stay under the 4 KB kernel-argument limit: an instantiation near it
// carries a static_assert on its sizeof where it is declared.
//   kwy_group<VIEW, N>: the kernel finds its job from the block index alone (u[blockIdx.x], u[blockIdx.y]).
//   kwy_batch<VIEW, N>: the jobs share one grid dimension: workgroup g belongs to the job u with
//     start[u] <= g < start[u + 1] and handles its frame (or slice) g - start[u].  One launch over both utterances of a
//     pair -- or over all pairs of a step -- fills the chip where a single utterance's 2 000 frames are 2.2 rounds of
//     resident workgroups.
#define KWY_BATCH_MAX 16
#define KWY_KERNARG_MAX 4096
template <class VIEW, int N>
struct kwy_group {
  int n;
  VIEW u[N];
};
template <class VIEW, int N = KWY_BATCH_MAX>
struct kwy_batch {
  int n;
  int start[N + 1];
  VIEW u[N];
  // job of workgroup g (uniform: scalar loop)
  __device__ __forceinline__ int find(int g) const {
    int k = 0;
    while (k + 1 < n && g >= start[k + 1]) ++k;
    return k;
  }
};

// slot u of a table from job i: view(i) for a group; view(i, blocks) for a batch, which also says how many workgroups
// the job takes (blocks comes in as 0)
template <class VIEW, int N, class FILL>
static inline void kwy_table_fill(kwy_group<VIEW, N> &t, int u, int i, FILL &fill) { t.u[u] = fill(i); }
template <class VIEW, int N, class FILL>
static inline void kwy_table_fill(kwy_batch<VIEW, N> &t, int u, int i, FILL &fill) {
  int blocks = 0;
  t.u[u] = fill(i, blocks);
  t.start[u + 1] = t.start[u] + blocks;
}

// `count` jobs in launches of at most N: every table starts out value-initialised (the slots from n on are zero and
// null, whatever the kernel), slot u is filled from job i0 + u, and launch(table, i0) -- table.n jobs, the first of them
// job i0 of the call -- enqueues the kernels; its first return other than KWY_OK ends the walk.
template <class TABLE, class FILL, class LAUNCH>
static inline int kwy_for_tables(int count, FILL fill, LAUNCH launch) {
  constexpr int N = (int)(sizeof(TABLE::u) / sizeof(TABLE::u[0]));
  for (int i0 = 0; i0 < count; i0 += N) {
    TABLE t{};
    t.n = count - i0 < N ? count - i0 : N;
    for (int u = 0; u < t.n; ++u) kwy_table_fill(t, u, i0 + u, fill);
    KWY_TRY(launch(t, i0));
  }
  return KWY_OK;
}

// --- GV-considering trajectory generation (kwy_gvgen.hip) ---------------------------------
// One utterance of the ascent for the conversion entries of kwy_mlpg.hip: the band records of its last solve (a copy:
// k_mlpg_chunks consumes its own in place), the trajectory (rows ldy doubles apart) and the offset track (rows ldo
// apart, or null).  kwy_gva_launch takes its scratch (kwy_gva_scratch_bytes) from the arena of the call in progress.
struct kwy_gva_view {
  const double *band;
  const double *offset;
  double *y;
  int64_t T;
  int ldy, ldo;
  double *objective;       // iterations + 1 doubles on the device, or null
  int32_t *status;         // one word on the device, or null
};
size_t kwy_gva_scratch_bytes(const int64_t *T, int n, int d, int iterations);
int kwy_gva_launch(kwy_ctx *ctx, const kwy_gva_view *v, int n, int d, const double *gv_mean, const double *gv_var,
                   double weight, int iterations);

static inline int kwy_ilog2(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return l;
}
