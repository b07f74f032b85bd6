// libkwy_selftest.so -- NOT part of the product: entry points that let tests drive device-side building blocks of
// kwy_device.hpp on caller data.  Built beside libkwy.so by build.sh, loaded only by tests (test_select_gpu.py,
// test_devmath_gpu.py, test_fft_regs_gpu.py).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../kwy_device.hpp"
#include "../kwy_selftest.h"

#define D4C_NT 256   // the 256-thread select of the 16..48 kHz band kernel

// ---- diagnostic: the "sum of the m smallest" routine of kwy_device.hpp on caller-supplied data -------------
// (one 256-thread workgroup per problem; out[p] = {sum of the m smallest, sum of all})
__global__ __launch_bounds__(D4C_NT) void k_select_selftest(const double *__restrict__ v, int n, int m,
                                                           double *__restrict__ out) {
  constexpr int RK = 9;
  __shared__ __attribute__((aligned(16))) uint32_t hist[KWY_SELECT_WORDS(D4C_NT)];
  __shared__ double red[2 * D4C_NT / 64];
  const int tid = threadIdx.x;
  const double *x = v + (size_t)blockIdx.x * n;
  unsigned long long key[RK];
#pragma unroll
  for (int r = 0; r < RK; ++r) {
    const int k = tid + D4C_NT * r;
    key[r] = k < n ? (unsigned long long)__double_as_longlong(x[k]) : ~0ull;
  }
  double s_small, s_all;
  kwy_block_smallest_sum<RK, D4C_NT>(key, n, m, hist, red, &s_small, &s_all);
  if (tid == 0) { out[2 * blockIdx.x] = s_small; out[2 * blockIdx.x + 1] = s_all; }
}

extern "C" int kwy_debug_smallest_sum_dev(void *stream, const double *values, int problems, int n, int m,
                                          double *out) {
  if (!values || !out || problems <= 0 || n <= 0 || n > 9 * D4C_NT || m <= 0 || m > n) return -1;
  hipLaunchKernelGGL(k_select_selftest, dim3(problems), dim3(D4C_NT), 0, (hipStream_t)stream, values, n, m, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- diagnostic: kwy_log / kwy_sincos_medium of kwy_device.hpp element by element ----------------------------
__global__ void k_devmath_selftest(const double *__restrict__ x, int n, double *__restrict__ lg, double *__restrict__ sn,
                                   double *__restrict__ cs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  lg[i] = kwy_log(x[i]);
  kwy_sincos_medium(x[i], &sn[i], &cs[i]);
}

extern "C" int kwy_debug_devmath_dev(void *stream, const double *x, int n, double *log_out, double *sin_out,
                                     double *cos_out) {
  if (!x || !log_out || !sin_out || !cos_out || n <= 0) return -1;
  hipLaunchKernelGGL(k_devmath_selftest, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, n, log_out,
                     sin_out, cos_out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- diagnostic: the real transform of N = 4096 samples through the stored and the drained closing pass ----------
// (one 256-thread workgroup per row; both paths return TWICE the bins 0 .. H, (H + 1) x {re, im} per row, formed by
// kwy_rfft_bin2_w resp. its register form with the same twiddle expressions the D4C kernels use: W^k of a bin below
// H/2 from the thread's base factor, the others from the table)
template <int LOG2N, int NT>
__global__ __launch_bounds__(NT) void k_rfft_paths_selftest(const double *__restrict__ x, const kwy_c *__restrict__ twH,
                                                            const kwy_c *__restrict__ twN, kwy_c *__restrict__ out_old,
                                                            kwy_c *__restrict__ out_new) {
  constexpr int N = 1 << LOG2N, H = N / 2, HEX = 16 * NT / N;
  extern __shared__ double smem[];
  kwy_c *B = (kwy_c *)smem;          // H + 1 complex
  double *Bd = smem;
  const int tid = threadIdx.x;
  const double *row = x + (size_t)blockIdx.x * N;
  kwy_c *oo = out_old + (size_t)blockIdx.x * (H + 1), *on = out_new + (size_t)blockIdx.x * (H + 1);
  kwy_c tw4[4];
  kwy_fft_thread_twiddles<LOG2N - 1, NT>(twH, tw4);
  // stored form
  for (int i = tid; i < N; i += NT) Bd[i] = row[i];
  __syncthreads();
  kwy_fft_inplace_w<LOG2N - 1, NT, false>(B, tw4);
  for (int r = 0; tid + NT * r <= H; ++r) {
    const int k = tid + NT * r;
    const kwy_c w = r < 4 ? kwy_tw_hex(twN[tid], HEX * r) : twN[k];
    oo[k] = kwy_rfft_bin2_w<LOG2N - 1>(B, k, w);
  }
  __syncthreads();
  // drained form
  for (int i = tid; i < N; i += NT) Bd[i] = row[i];
  __syncthreads();
  kwy_fft_inplace_w<LOG2N - 1, NT, false, false>(B, tw4);
  kwy_c lo[4], hi[4], md;
  kwy_fft_tail4_drain<LOG2N - 1, NT, false>(B, lo, hi, md);
  const kwy_c twa = twN[tid], twc = twN[(NT - tid) & (NT - 1)];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = kwy_drain_bin<LOG2N - 1>(s, tid);
    if (k == 0) {
      on[0] = {2.0 * (lo[0].x + lo[0].y), 0.0};
      on[H] = {2.0 * (lo[0].x - lo[0].y), 0.0};
    } else {
      on[k] = kwy_rfft_bin2_v(lo[s], hi[s], kwy_drain_tw<LOG2N - 1, NT>(s, twa, twc));
      on[H - k] = kwy_rfft_bin2_v(hi[s], lo[s], twN[H - k]);
    }
  }
  if (tid == 0) on[H / 2] = kwy_rfft_bin2_v(md, md, twN[H / 2]);
}

extern "C" int kwy_debug_rfft_paths_dev(void *stream, const double *x, int problems, int log2n, double *out_old,
                                        double *out_new) {
  if (!x || !out_old || !out_new || problems <= 0) return -1;
  if (log2n != 12) return -1;        // the one size with a drained closing pass
  constexpr int LOG2N = 12, NT = 256, N = 1 << LOG2N, H = N / 2;
  std::vector<kwy_c> h(H / 8 + N);
  for (int k = 0; k < H / 8; ++k) { const double a = -2.0 * KWY_PI * k / H; h[k] = {cos(a), sin(a)}; }
  for (int k = 0; k < N; ++k) { const double a = -2.0 * KWY_PI * k / N; h[H / 8 + k] = {cos(a), sin(a)}; }
  kwy_c *tw = nullptr;
  if (hipMalloc((void **)&tw, sizeof(kwy_c) * h.size()) != hipSuccess) return -2;
  int rc = 0;
  if (hipMemcpy(tw, h.data(), sizeof(kwy_c) * h.size(), hipMemcpyHostToDevice) != hipSuccess) rc = -2;
  if (rc == 0) {
    const size_t lds = sizeof(kwy_c) * (H + 1);
    auto kern = k_rfft_paths_selftest<LOG2N, NT>;
    if (hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) rc = -2;
    if (rc == 0) {
      hipLaunchKernelGGL(kern, dim3(problems), dim3(NT), lds, (hipStream_t)stream, x, tw, tw + H / 8, (kwy_c *)out_old,
                         (kwy_c *)out_new);
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = -2;
    }
  }
  hipFree(tw);
  return rc;
}
