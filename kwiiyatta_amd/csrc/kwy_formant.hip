// kwy_formant.hip -- formant shift: a frequency-axis warp of spectral envelopes (include/kwy.h, "formant shift")
//
//   u_k = k / rho,  j = floor(u_k),  a = u_k - j,  l = log(sp[t])
//   out[t, k] = sp[t, K-1]                        j >= K-1
//             = sp[t, j]                          a == 0
//             = exp(l[j] + a * (l[j+1] - l[j]))   otherwise
//
// There is no reference call to cite: the reference's dialog (kwiiyatta/resynthesize_voice.py) transposes the key only.
//
// Traffic: rows x K x 8 bytes in and as many out.  A workgroup takes chunks of whole rows -- R = min(64,
// 2048 / K) rows, contiguous in memory (one row of 2049 bins in a buffer twice as large) -- and stages a chunk as its
// logarithms in LDS: one kwy_log per input bin.
// Every output is then two LDS reads and one exp, or a read of the input where the definition copies.  The outputs of a
// chunk wait in registers until every lane has passed the barrier behind the last read of the chunk: out may equal sp.
// Lane `tid` owns the elements tid + 512 q of a chunk, so loads and stores are coalesced along k; its (j, a) per q depend
// on (k, rho) alone and the chunk stride is a multiple of K: they are formed once, in front of the chunk loop.
// Unusable rows are flagged per chunk in LDS and counted with an integer atomic (the order of an integer sum is free).
//
// The kernel neither allocates nor synchronises nor uses the context's arena: the _dev entries are legal inside a stream
// capture.  The host entry stages through the arena and synchronises, as kwy_gv_postfilter does.
#include <math.h>

#include "kwy_internal.hpp"

#define FS_GROUP 32                         // jobs per launch
#define FS_THREADS 512                      // lanes of a workgroup
#define FS_CHUNK 2048                       // doubles of staged logarithms; twice that where a row is longer
#define FS_MAX_ROWS 64                      // rows per chunk at most
#define FS_BLOCKS 2048                      // workgroups per launch, about

static_assert(KWY_FORMANT_MAX_K <= 2 * FS_CHUNK, "a row must fit the staging buffer");
static_assert(2 * FS_MAX_ROWS <= FS_THREADS, "the flags are cleared by one lane each");

struct fs_view {
  const double *sp;
  int64_t rows;
  double *out;
  int32_t *status;         // rows copied unchanged (may be NULL); zero before the launch
};
typedef kwy_group<fs_view, FS_GROUP> fs_views;

static inline int fs_chunk_rows(int K, int cap) {
  const int r = cap / K;
  return r < FS_MAX_ROWS ? r : FS_MAX_ROWS;
}

// blockIdx.y: the job; its workgroups stride over the job's chunks of R rows, R K <= FS_THREADS Q.  W: the wavefronts
// per SIMD the registers are to leave room for (Q = 4: 80 VGPRs, three workgroups per CU; Q = 8: 119, two)
template <int Q, int W>
__global__ __launch_bounds__(FS_THREADS, W) void k_formant_shift(fs_views B, int K, int R, double rho) {
  constexpr int NT = FS_THREADS;
  __shared__ double lg[NT * Q];
  __shared__ int bad[2][FS_MAX_ROWS];
  const fs_view &U = B.u[blockIdx.y];
  const int tid = threadIdx.x;
  const int64_t chunks = (U.rows + R - 1) / R;
  if ((int64_t)blockIdx.x >= chunks) return;                  // (uniform)
  // element tid + 512 q of any chunk: its row within the chunk (high half) and the chunk index of its lower tap
  int tap[Q];
  double frac[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = tid + q * NT;
    const int r = i / K, k = i - r * K;
    const double u = (double)k / rho;
    const double fj = floor(u);
    int j = (int)fj;                                          // (u <= 2 (K - 1))
    double a = u - fj;
    if (j >= K - 1) {
      j = K - 1;
      a = 0.0;
    }
    tap[q] = (r << 16) | ((r * K + j) & 0xffff);              // (beyond R K: never used)
    frac[q] = a;
  }
  if (tid < 2 * FS_MAX_ROWS) (&bad[0][0])[tid] = 0;
  __syncthreads();
  const double *in = U.sp;
  double *out = U.out;
  int par = 0;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x, par ^= 1) {
    const int64_t r0 = c * R;
    const int nr = U.rows - r0 < R ? (int)(U.rows - r0) : R;
    const int count = nr * K;
    const int64_t base = r0 * K;
    double v[Q];                                              // (all loads of the chunk in flight before the first log)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = tid + q * NT;
      v[q] = i < count ? in[base + i] : 1.0;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = tid + q * NT;
      if (i < count) {
        lg[i] = kwy_log(v[q]);
        if (!kwy_finite_pos(v[q])) bad[par][tap[q] >> 16] = 1;
      }
    }
    __syncthreads();
    if (tid < FS_MAX_ROWS) {
      bad[par ^ 1][tid] = 0;                                  // (last read before the previous barrier, set after the next)
      if (tid < nr && bad[par][tid] && U.status) atomicAdd(U.status, 1);
    }
    double o[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = tid + q * NT;
      o[q] = 0.0;
      if (i < count) {
        const int s = tap[q] & 0xffff;
        const double a = frac[q];
        if (bad[par][tap[q] >> 16]) o[q] = in[base + i];
        else if (a == 0.0) o[q] = in[base + s];
        else {
          const double l0 = lg[s], l1 = lg[s + 1];
          o[q] = exp(l0 + a * (l1 - l0));
        }
      }
    }
    __syncthreads();                                          // every read of the chunk is done: out may be sp
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = tid + q * NT;
      if (i < count) out[base + i] = o[q];
    }
  }
}

static int fs_check(kwy_ctx *ctx, const kwy_formant_job *jobs, int count, int K, double rho) {
  if (!(rho >= 0.5 && rho <= 2.0)) {                          // (a NaN fails both)
    ctx->err = "formant_shift: the ratio must be finite and within [0.5, 2]";
    return KWY_EINVAL;
  }
  if (K < 2 || K > KWY_FORMANT_MAX_K) {
    ctx->err = "formant_shift: K must be within [2, 2049]";
    return KWY_EINVAL;
  }
  if (!jobs || count < 1) { ctx->err = "formant_shift: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i)
    if (jobs[i].rows < 0 || (jobs[i].rows > 0 && (!jobs[i].sp || !jobs[i].out))) {
      ctx->err = "formant_shift: bad argument";
      return KWY_EINVAL;
    }
  return KWY_OK;
}

// device pointers throughout
static int fs_launch(kwy_ctx *ctx, const kwy_formant_job *jobs, int count, int K, double rho, int32_t *status) {
  if (status) KWY_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)count, ctx->stream));
  if (rho == 1.0) {                                           // nothing is examined
    for (int i = 0; i < count; ++i)
      if (jobs[i].rows > 0 && jobs[i].out != jobs[i].sp)
        KWY_HIP(hipMemcpyAsync(jobs[i].out, jobs[i].sp, sizeof(double) * (size_t)jobs[i].rows * K,
                               hipMemcpyDeviceToDevice, ctx->stream));
    return KWY_OK;
  }
  const int cap = K > FS_CHUNK ? 2 * FS_CHUNK : FS_CHUNK;
  const int R = fs_chunk_rows(K, cap);
  return kwy_for_tables<fs_views>(
      count,
      [&](int i) { return fs_view{jobs[i].sp, jobs[i].rows, jobs[i].out, status ? status + i : nullptr}; },
      [&](const fs_views &B, int) {
        int64_t longest = 0;
        for (int u = 0; u < B.n; ++u) longest = B.u[u].rows > longest ? B.u[u].rows : longest;
        if (longest == 0) return KWY_OK;
        int64_t blocks = (longest + R - 1) / R;
        const int64_t share = FS_BLOCKS / B.n;
        blocks = blocks > share ? share : blocks;
        const dim3 grid((unsigned)blocks, B.n), block(FS_THREADS);
        if (cap == FS_CHUNK)
          KWY_PROF(ctx, "k_formant_shift", hipLaunchKernelGGL((k_formant_shift<FS_CHUNK / FS_THREADS, 6>), grid, block,
                                                              0, ctx->stream, B, K, R, rho));
        else      // (only K = 2049, a 4096-point transform: a row needs the larger buffer)
          KWY_PROF(ctx, "k_formant_shift", hipLaunchKernelGGL((k_formant_shift<2 * FS_CHUNK / FS_THREADS, 4>), grid,
                                                              block, 0, ctx->stream, B, K, R, rho));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

extern "C" int kwy_formant_shift_batch_dev(kwy_ctx *ctx, const kwy_formant_job *jobs, int count, int K, double rho,
                                           int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(fs_check(ctx, jobs, count, K, rho));
  KWY_HIP(hipSetDevice(ctx->device));
  return fs_launch(ctx, jobs, count, K, rho, status);
}

extern "C" int kwy_formant_shift_dev(kwy_ctx *ctx, const double *sp, int64_t rows, int K, double rho, double *out,
                                     int32_t *status) {
  const kwy_formant_job one = {sp, rows, out};
  return kwy_formant_shift_batch_dev(ctx, &one, 1, K, rho, status);
}

extern "C" int kwy_formant_shift(kwy_ctx *ctx, const kwy_formant_job *jobs, int count, int K, double rho,
                                 int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(fs_check(ctx, jobs, count, K, rho));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "formant_shift");
  int32_t *dstatus;
  st.out(dstatus, status, (size_t)count);
  std::vector<kwy_formant_job> staged(jobs, jobs + count);
  for (int i = 0; i < count; ++i)                             // warped in place on the device
    st.inout(staged[i].out, jobs[i].sp, jobs[i].out, (size_t)jobs[i].rows * K);
  KWY_TRY(st.begin());
  for (int i = 0; i < count; ++i) staged[i].sp = staged[i].out;
  KWY_TRY(fs_launch(ctx, staged.data(), count, K, rho, dstatus));
  return st.finish();
}
