// libkwy_selftest.so -- NOT part of the product: entry points that let tests drive device-side building blocks of
// kwy_device.hpp and kwy_fft.hpp on caller data.  Built beside libkwy.so by build.sh, loaded only by tests (test_select_gpu.py,
// test_select_paths_gpu.py, test_devmath_gpu.py, test_fft_regs_gpu.py).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../kwy_fft.hpp"
#include "../kwy_selftest.h"

#define D4C_NT 256   // the 256-thread select of the 16..48 kHz band kernel

// ---- diagnostic: the "sum of the m smallest" routine of kwy_device.hpp on caller-supplied data -------------
// (one 256-thread workgroup per problem; out[p] = {sum of the m smallest, sum of all})
__global__ __launch_bounds__(D4C_NT) void k_select_selftest(const double *__restrict__ v, int n, int m,
                                                           double *__restrict__ out) {
  constexpr int RK = 9;
  __shared__ __attribute__((aligned(16))) uint32_t hist[KWY_SELECT_WORDS(D4C_NT) + KWY_SELECT_WIDE_WORDS];
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
  kwy_block_smallest_sum<RK, D4C_NT>(key, n, m, hist, hist + KWY_SELECT_WORDS(D4C_NT), red, &s_small, &s_all);
  if (tid == 0) { out[2 * blockIdx.x] = s_small; out[2 * blockIdx.x + 1] = s_all; }
}

extern "C" int kwy_debug_smallest_sum_dev(void *stream, const double *values, int problems, int n, int m,
                                          double *out) {
  if (!values || !out || problems <= 0 || n <= 0 || n > 9 * D4C_NT || m <= 0 || m > n) return -1;
  hipLaunchKernelGGL(k_select_selftest, dim3(problems), dim3(D4C_NT), 0, (hipStream_t)stream, values, n, m, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- diagnostic: the select as it was before its from-the-top path got private histogram copies and fewer
// barriers -- ONE histogram counted with same-address atomics, both sums formed behind the selection and exchanged by
// kwy_block_sum2 -- kept here as the reference the current one is held to, bit for bit
// (its scratch: 2 * KWY_SELECT_BINS + 32 words)
#define REF_SELECT_WORDS (2 * KWY_SELECT_BINS + 32)
template <int RMAX, int NT = KWY_THREADS>
__device__ inline void ref_block_smallest_sum(unsigned long long (&key)[RMAX], int n, int m,
                                              uint32_t *hist, double *red, double *sum_small,
                                              double *sum_all) {
  constexpr int BITS = KWY_SELECT_BITS, BINS = 1 << BITS;
  constexpr int TOP_SHIFT = 18;                           // high word: 20 mantissa bits -> quarter binades
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t *ctlb = hist + 2 * BINS;  // 2 x {digit, rank, population, before}; [8..9] one 64-bit key; [10] list
                                     // length; [11..12] two counts; [16 ..] one word per wavefront
  unsigned long long *k64 = (unsigned long long *)(ctlb + 8);
  unsigned long long *list = (unsigned long long *)(hist + BINS);
  unsigned long long vkey;           // bit pattern of v*
  int copies;                        // how many keys equal to v* belong to the m smallest

  // ---- (1) from the top
  uint32_t hmax = 0;
#pragma unroll
  for (int r = 0; r < RMAX; ++r)
    if (tid + NT * r < n) hmax = max(hmax, (uint32_t)(key[r] >> 32));
  hmax = kwy_wave_max_u32(hmax);
  if (lane == 0) ctlb[16 + wv] = hmax;
  for (int i = tid; i < BINS; i += NT) hist[i] = 0;
  if (tid == 0) ctlb[10] = 0;
  __syncthreads();
  hmax = ctlb[16];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) hmax = max(hmax, ctlb[16 + i]);
  uint32_t dg[RMAX];
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    dg[r] = BINS;                                         // (no bin: slot beyond n)
    if (NT * r + (tid & ~63) >= n) continue;              // nothing in this slot for the whole wavefront
    if (tid + NT * r < n) {
      dg[r] = min((hmax - (uint32_t)(key[r] >> 32)) >> TOP_SHIFT, (uint32_t)(BINS - 1));
      atomicAdd(&hist[dg[r]], 1u);
    }
  }
  __syncthreads();
  if (wv == 0) kwy_select_scan(hist, n - m + 1, ctlb, lane);
  __syncthreads();
  const uint32_t chosen = ctlb[0], pop = ctlb[2];
  if (chosen < (uint32_t)(BINS - 1) && pop <= (uint32_t)KWY_SELECT_LIST) {
    const int rank = (int)ctlb[1], above = (int)ctlb[3];
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
      if (dg[r] == chosen) list[atomicAdd(&ctlb[10], 1u)] = key[r];
    __syncthreads();
    kwy_select_rank<true>(list, (int)pop, rank, tid, k64, &ctlb[11]);
    __syncthreads();
    vkey = *k64;
    copies = m - (n - above - (int)ctlb[11] - (int)ctlb[12]);   // keys >= v*: above + listed in front + ties
  } else {
    // ---- (2) general: the block's smallest and largest key, relative keys, radix rounds
    double lo = INFINITY, hi = 0.0;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      if (tid + NT * r < n) {
        const double x = __longlong_as_double((long long)key[r]);
        lo = fmin(lo, x); hi = fmax(hi, x);
      }
    }
    lo = kwy_wave_min_f64(lo);
    hi = kwy_wave_max_f64(hi);
    if (lane == 0) { red[wv] = lo; red[NT / 64 + wv] = hi; }
    for (int i = tid; i < BINS; i += NT) hist[i] = 0;
    if (tid == 0) ctlb[10] = 0;
    __syncthreads();
    lo = red[0]; hi = red[NT / 64];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) { lo = fmin(lo, red[i]); hi = fmax(hi, red[NT / 64 + i]); }
    const unsigned long long kmin = (unsigned long long)__double_as_longlong(lo);
    const unsigned long long range = (unsigned long long)__double_as_longlong(hi) - kmin;
    const int top0 = range ? 64 - __clzll((long long)range) : 0;     // one past the highest differing bit
    const int rounds = (top0 + BITS - 1) / BITS;                    // 0: all keys equal
#pragma unroll
    for (int r = 0; r < RMAX; ++r) key[r] -= kmin;                  // (slots beyond n are never looked at)
    unsigned long long prefix = 0ull;
    int kk = m;  // 1-based rank of the wanted element among the still-matching keys
    bool alive[RMAX];  // key still carries the prefix found so far
#pragma unroll
    for (int r = 0; r < RMAX; ++r) alive[r] = tid + NT * r < n;
    for (int round = 0; round < rounds; ++round) {
      // digits are taken from bit top0 - 1 downwards; the last one may be narrower
      const int top = top0 - BITS * round;                  // one past the digit's highest bit
      const int shift = top - BITS > 0 ? top - BITS : 0;
      const unsigned long long mask = (1ull << (top - shift)) - 1ull;
      uint32_t *h = hist + (round & 1) * BINS, *hn = hist + ((round + 1) & 1) * BINS;
      uint32_t *ctl = ctlb + (round & 1) * 4;
      for (int i = tid; i < BINS; i += NT) hn[i] = 0;
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        if (NT * r + (tid & ~63) >= n) continue;  // nothing in this slot for the whole wavefront
        const int d = (int)((key[r] >> shift) & mask);
#if KWY_SELECT_AGG
        const unsigned long long mm = __ballot(alive[r]);
        if (mm != 0ull) {
          const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)mm) - 1);
          const int d0 = __builtin_amdgcn_readlane(d, leader);
          const bool same = alive[r] && d == d0;
          const unsigned long long ms = __ballot(same);
          if (lane == leader) atomicAdd(&h[d0], (uint32_t)__popcll(ms));
          if (alive[r] && !same) atomicAdd(&h[d], 1u);
        }
#else
        if (alive[r]) atomicAdd(&h[d], 1u);
#endif
      }
      __syncthreads();
      if (wv == 0) kwy_select_scan(h, kk, ctl, lane);
      __syncthreads();
      const int chosen_d = (int)ctl[0];
      prefix |= (unsigned long long)chosen_d << shift;
      kk = (int)ctl[1];
#pragma unroll
      for (int r = 0; r < RMAX; ++r) alive[r] = alive[r] && (int)((key[r] >> shift) & mask) == chosen_d;
      const uint32_t left = ctl[2];
      if (left == 1u && round < rounds - 1) {
        // exactly one key carries this prefix: it IS the wanted element, skip the remaining rounds
#pragma unroll
        for (int r = 0; r < RMAX; ++r)
          if (alive[r]) *k64 = key[r];
        __syncthreads();
        prefix = *k64;
        kk = 1;
        break;
      }
      if (left <= (uint32_t)KWY_SELECT_LIST && round < rounds - 1) {
        // a handful of keys carry this prefix: listed in the other histogram's words and ranked against each other
        unsigned long long *lst = (unsigned long long *)hn;
#pragma unroll
        for (int r = 0; r < RMAX; ++r)
          if (alive[r]) lst[atomicAdd(&ctlb[10], 1u)] = key[r];
        __syncthreads();
        kwy_select_rank<false>(lst, (int)left, kk, tid, k64, &ctlb[11]);
        __syncthreads();
        prefix = *k64;
        kk -= (int)ctlb[11];                                // copies of v* among the m smallest
        break;
      }
    }
    // (all keys equal: no round ran, prefix = 0 = every relative key, kk = m of them)
    vkey = prefix + kmin;
    copies = kk;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) key[r] += kmin;
  }
  const double vstar = __longlong_as_double((long long)vkey);
  double s_less = 0.0, s_all = 0.0;
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    if (tid + NT * r < n) {
      const double x = __longlong_as_double((long long)key[r]);
      s_all += x;
      if (key[r] < vkey) s_less += x;
    }
  }
  double t_less, t_all;
  kwy_block_sum2<NT>(s_less, s_all, red, &t_less, &t_all);
  *sum_small = t_less + (double)copies * vstar;
  *sum_all = t_all;
}

// both on the same keys, NT threads per problem: out_ref[p], out_new[p] = {sum of the m smallest, sum of all}; the
// current one in the form the band kernel calls (results in thread 0 only)
template <int NT>
__global__ __launch_bounds__(NT) void k_select_paths_selftest(const double *__restrict__ v, int n, int m,
                                                              double *__restrict__ out_ref, double *__restrict__ out_new) {
  constexpr int RK = 9;
  __shared__ __attribute__((aligned(16))) uint32_t hist[KWY_SELECT_WORDS(NT) + KWY_SELECT_WIDE_WORDS];
  __shared__ double red[2 * NT / 64];
  static_assert(REF_SELECT_WORDS <= KWY_SELECT_WORDS(NT), "the reference's scratch fits the current one's");
  const int tid = threadIdx.x;
  const double *x = v + (size_t)blockIdx.x * n;
  unsigned long long key[RK];
#pragma unroll
  for (int r = 0; r < RK; ++r) {
    const int k = tid + NT * r;
    key[r] = k < n ? (unsigned long long)__double_as_longlong(x[k]) : ~0ull;
  }
  double s_small, s_all;
  ref_block_smallest_sum<RK, NT>(key, n, m, hist, red, &s_small, &s_all);
  if (tid == 0) { out_ref[2 * blockIdx.x] = s_small; out_ref[2 * blockIdx.x + 1] = s_all; }
  __syncthreads();
  kwy_block_smallest_sum<RK, NT, false>(key, n, m, hist, hist + KWY_SELECT_WORDS(NT), red, &s_small, &s_all);
  if (tid == 0) { out_new[2 * blockIdx.x] = s_small; out_new[2 * blockIdx.x + 1] = s_all; }
}

extern "C" int kwy_debug_select_paths_dev(void *stream, const double *values, int problems, int n, int m,
                                          double *out_ref, double *out_new) {
  if (!values || !out_ref || !out_new || problems <= 0 || n <= 0 || n > 9 * 256 || m <= 0 || m > n) return -1;
  hipLaunchKernelGGL(k_select_paths_selftest<256>, dim3(problems), dim3(256), 0, (hipStream_t)stream, values, n, m,
                     out_ref, out_new);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int kwy_debug_select_paths512_dev(void *stream, const double *values, int problems, int n, int m,
                                             double *out_ref, double *out_new) {
  if (!values || !out_ref || !out_new || problems <= 0 || n <= 0 || n > 9 * 512 || m <= 0 || m > n) return -1;
  hipLaunchKernelGGL(k_select_paths_selftest<512>, dim3(problems), dim3(512), 0, (hipStream_t)stream, values, n, m,
                     out_ref, out_new);
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

// ---- diagnostic: kwy_block_exscan, one workgroup of 256 threads per problem ------------------------------------
__global__ __launch_bounds__(KWY_THREADS) void k_block_exscan_selftest(const int *__restrict__ v,
                                                                      int *__restrict__ offsets, int *__restrict__ totals) {
  __shared__ int sh[KWY_WAVES];
  const int i = blockIdx.x * KWY_THREADS + threadIdx.x;
  int tot;
  offsets[i] = kwy_block_exscan(v[i], sh, &tot);
  if (threadIdx.x == KWY_THREADS - 1) totals[blockIdx.x] = tot;
}

extern "C" int kwy_debug_block_exscan_dev(void *stream, const int *values, int problems, int *offsets, int *totals) {
  if (!values || !offsets || !totals || problems <= 0) return -1;
  hipLaunchKernelGGL(k_block_exscan_selftest, dim3(problems), dim3(KWY_THREADS), 0, (hipStream_t)stream, values,
                     offsets, totals);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- the twiddle tables of the FFT diagnostics below, on the device for the lifetime of the object -------------------
// twH: exp(-2 pi i k / H), k < nh; twN (where asked): exp(-2 pi i k / N), k < N = 2H; twP: the powers table of an H-point
// transform's stride-64 pass, filled on `s` by the library's own fill kernel from twH (which reads twH[64 u], u < H/512:
// inside the H/8 factors every caller asks for) -- behind the tables, or in `powers_out` where the caller wants to see it.
struct fft_tables {
  kwy_c *buf = nullptr;
  const kwy_c *twH = nullptr, *twN = nullptr, *twP = nullptr;
  int rc = 0;
  fft_tables(hipStream_t s, int log2h, int nh, bool with_n, kwy_c *powers_out = nullptr) {
    const int H = 1 << log2h, N = 2 * H, nn = with_n ? N : 0, entries = H / 512;
    std::vector<kwy_c> h(nh + nn);
    for (int k = 0; k < nh; ++k) { const double a = -2.0 * KWY_PI * k / H; h[k] = {cos(a), sin(a)}; }
    for (int k = 0; k < nn; ++k) { const double a = -2.0 * KWY_PI * k / N; h[nh + k] = {cos(a), sin(a)}; }
    if (hipMalloc((void **)&buf, sizeof(kwy_c) * (h.size() + KWY_TWP_ENTRY * entries)) != hipSuccess ||
        hipMemcpy(buf, h.data(), sizeof(kwy_c) * h.size(), hipMemcpyHostToDevice) != hipSuccess) { rc = -2; return; }
    kwy_c *pw = powers_out ? powers_out : buf + h.size();
    twH = buf; twN = with_n ? buf + nh : nullptr; twP = pw;
    hipLaunchKernelGGL(k_twiddle_powers_fill<0>, dim3(1), dim3(64), 0, s, twH, pw, entries);
    if (hipGetLastError() != hipSuccess) rc = -2;
  }
  ~fft_tables() { (void)hipFree(buf); }
  fft_tables(const fft_tables &) = delete;
  fft_tables &operator=(const fft_tables &) = delete;
};

// ---- diagnostic: the real transform of N = 4096 samples through the stored and the drained closing pass ----------
// (one 256-thread workgroup per row; both paths return TWICE the bins 0 .. H, (H + 1) x {re, im} per row, formed by
// kwy_rfft_bin2_w resp. its register form with the same twiddle expressions the D4C kernels use: W^k of a bin below
// H/2 from the thread's base factor, the others from the table)
template <int LOG2N, int NT>
__global__ __launch_bounds__(NT) void k_rfft_paths_selftest(const double *__restrict__ x, const kwy_c *__restrict__ twH,
                                                            const kwy_c *__restrict__ twP,
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
  kwy_fft_inplace_w<LOG2N - 1, NT, false>(B, tw4, twP);
  for (int r = 0; tid + NT * r <= H; ++r) {
    const int k = tid + NT * r;
    const kwy_c w = r < 4 ? kwy_tw_hex(twN[tid], HEX * r) : twN[k];
    oo[k] = kwy_rfft_bin2_w<LOG2N - 1>(B, k, w);
  }
  __syncthreads();
  // drained form
  for (int i = tid; i < N; i += NT) Bd[i] = row[i];
  __syncthreads();
  kwy_fft_inplace_w<LOG2N - 1, NT, false, false>(B, tw4, twP);
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
  hipStream_t s = (hipStream_t)stream;
  fft_tables t(s, LOG2N - 1, H / 8, true);
  int rc = t.rc;
  const size_t lds = sizeof(kwy_c) * (H + 1);
  auto kern = k_rfft_paths_selftest<LOG2N, NT>;
  if (rc == 0 && hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) rc = -2;
  if (rc == 0) {
    hipLaunchKernelGGL(kern, dim3(problems), dim3(NT), lds, s, x, t.twH, t.twP, t.twN, (kwy_c *)out_old, (kwy_c *)out_new);
    if (hipGetLastError() != hipSuccess) rc = -2;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = -2;
  return rc;
}

// ---- diagnostic: the stride-64 radix-8 pass with per-lane powers and with the powers table ----------------------------
// (one NT-thread workgroup per row of H complex; both paths return the H bins of the complex transform.  The passes
// around the stride-64 one are the same calls in both paths.)
template <int LOG2H, int NT, bool INV>
__global__ __launch_bounds__(NT) void k_fft_powers_selftest(const kwy_c *__restrict__ x, const kwy_c *__restrict__ twH,
                                                            const kwy_c *__restrict__ twP, kwy_c *__restrict__ out_lane,
                                                            kwy_c *__restrict__ out_table) {
  constexpr int H = 1 << LOG2H;
  extern __shared__ double smem[];
  kwy_c *B = (kwy_c *)smem;          // H complex
  const int tid = threadIdx.x;
  const kwy_c *row = x + (size_t)blockIdx.x * H;
#pragma nounroll
  for (int path = 0; path < 2; ++path) {
    kwy_c *o = (path == 0 ? out_lane : out_table) + (size_t)blockIdx.x * H;
    for (int i = tid; i < H; i += NT) B[i] = row[i];
    __syncthreads();
    kwy_fft_pass8<LOG2H, 0, NT, INV>(B, twH);
    kwy_fft_pass8<LOG2H, 3, NT, INV>(B, twH);
    if (path == 0) kwy_fft_pass8<LOG2H, 6, NT, INV>(B, twH);
    else kwy_fft_pass8_s64<LOG2H, NT, INV>(B, twP);
    if constexpr (LOG2H == 12) kwy_fft_pass8<LOG2H, 9, NT, INV>(B, twH);
    if constexpr (LOG2H % 3 != 0) kwy_fft_tail<LOG2H, LOG2H % 3, NT, INV>(B);
    for (int i = tid; i < H; i += NT) o[i] = B[i];
    __syncthreads();
  }
}

// the table's entries once more, by one thread, from w^1 and from its conjugate (the inverse direction's factor)
__global__ void k_twiddle_powers_ref(const kwy_c *__restrict__ twH, int entries, kwy_c *__restrict__ ref,
                                     kwy_c *__restrict__ ref_conj) {
  for (int u = 0; u < entries; ++u) {
    for (int c = 0; c < 2; ++c) {
      kwy_c w1 = twH[64 * u];
      if (c) w1.y = -w1.y;
      const kwy_c w2 = cmulf(w1, w1), w4 = cmulf(w2, w2);
      const kwy_c w3 = cmulf(w1, w2), w5 = cmulf(w4, w1), w6 = cmulf(w4, w2);
      const kwy_c w7 = cmulf(w4, w3);
      kwy_c *o = (c ? ref_conj : ref) + KWY_TWP_ENTRY * u;
      o[0] = {1.0, 0.0}; o[1] = w1; o[2] = w2; o[3] = w3; o[4] = w4; o[5] = w5; o[6] = w6; o[7] = w7;
    }
  }
}

template <int LOG2H, int NT>
static int fft_powers_launch(hipStream_t stream, const kwy_c *x, int problems, bool inverse, const kwy_c *twH,
                             const kwy_c *twP, kwy_c *out_lane, kwy_c *out_table) {
  const size_t lds = sizeof(kwy_c) * (1 << LOG2H);
  if (hipFuncSetAttribute((const void *)k_fft_powers_selftest<LOG2H, NT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
      hipFuncSetAttribute((const void *)k_fft_powers_selftest<LOG2H, NT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -2;
  if (inverse) hipLaunchKernelGGL((k_fft_powers_selftest<LOG2H, NT, true>), dim3(problems), dim3(NT), lds, stream, x, twH, twP, out_lane, out_table);
  else hipLaunchKernelGGL((k_fft_powers_selftest<LOG2H, NT, false>), dim3(problems), dim3(NT), lds, stream, x, twH, twP, out_lane, out_table);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// x: problems rows of 2^log2h complex; out_lane / out_table: the same shape; tab, tab_ref, tab_ref_conj:
// KWY_TWP_ENTRY * 2^log2h / 512 complex each (the table as the library fills it, and the one-thread recomputations)
extern "C" int kwy_debug_fft_powers_dev(void *stream, const double *x, int problems, int log2h, int nt, int inverse,
                                        double *out_lane, double *out_table, double *tab, double *tab_ref,
                                        double *tab_ref_conj) {
  if (!x || !out_lane || !out_table || !tab || !tab_ref || !tab_ref_conj || problems <= 0) return -1;
  if (!((log2h == 10 && (nt == 128 || nt == 256)) || (log2h == 11 && nt == 256) || (log2h == 12 && nt == 512))) return -1;
  const int H = 1 << log2h, entries = H / 512;
  hipStream_t s = (hipStream_t)stream;
  fft_tables t(s, log2h, H, false, (kwy_c *)tab);    // (the per-lane stride-64 pass reads the whole table)
  int rc = t.rc;
  if (rc == 0) {
    hipLaunchKernelGGL(k_twiddle_powers_ref, dim3(1), dim3(1), 0, s, t.twH, entries, (kwy_c *)tab_ref, (kwy_c *)tab_ref_conj);
    if (hipGetLastError() != hipSuccess) rc = -2;
  }
  if (rc == 0) {
    const kwy_c *cx = (const kwy_c *)x, *tw = t.twH, *tp = t.twP;
    kwy_c *ol = (kwy_c *)out_lane, *ot = (kwy_c *)out_table;
    if (log2h == 10 && nt == 128) rc = fft_powers_launch<10, 128>(s, cx, problems, inverse != 0, tw, tp, ol, ot);
    else if (log2h == 10) rc = fft_powers_launch<10, 256>(s, cx, problems, inverse != 0, tw, tp, ol, ot);
    else if (log2h == 11) rc = fft_powers_launch<11, 256>(s, cx, problems, inverse != 0, tw, tp, ol, ot);
    else rc = fft_powers_launch<12, 512>(s, cx, problems, inverse != 0, tw, tp, ol, ot);
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = -2;
  return rc;
}

// ---- diagnostic: the first passes and the real split of the 2048-point synthesis kernel, every form on the same rows ----
// (one 128-thread workgroup per row of 1024 complex; the passes behind the first one and the transform in front of the
// split are the same calls in every path.  The half pass gets NaNs where it must not read.)
template <int = 0>
__global__ __launch_bounds__(128) void k_syn_first_passes_selftest(const kwy_c *__restrict__ x, const kwy_c *__restrict__ twH,
                                                                   const kwy_c *__restrict__ twP, const kwy_c *__restrict__ twN,
                                                                   kwy_c *__restrict__ out_dense, kwy_c *__restrict__ out_sparse,
                                                                   kwy_c *__restrict__ out_half, double *__restrict__ fold_ref,
                                                                   double *__restrict__ fold_new) {
  constexpr int LOG2H = 10, NT = 128, V = 2, H = 1 << LOG2H, Q = H / 8;
  extern __shared__ double smem[];
  kwy_c *B = (kwy_c *)smem;          // H + 1 complex
  const double *L = smem;
  const int tid = threadIdx.x;
  const kwy_c *row = x + (size_t)blockIdx.x * H;
  kwy_c twb[V];
#pragma unroll
  for (int g = 0; g < V; ++g) twb[g] = twN[tid + NT * g];
#pragma nounroll
  for (int path = 0; path < 5; ++path) {
    if (path == 1) {
      const kwy_c a0 = row[tid], a1 = tid == 0 ? row[Q] : kwy_c{0.0, 0.0};
      kwy_fft_pass8_first_sparse_core<LOG2H, NT, false>(B, kwy_tw_table{twH}, a0, a1);
    } else if (path == 2) {
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      for (int i = tid; i <= H; i += NT) B[i] = i <= H / 2 ? row[i] : kwy_c{nan, nan};
      __syncthreads();
      kwy_fft_pass8_first_half_core<LOG2H, NT, false>(B, kwy_tw_table{twH});
    } else {
      for (int i = tid; i < H; i += NT) B[i] = row[i];
      __syncthreads();
      kwy_fft_pass8<LOG2H, 0, NT, false>(B, twH);
    }
    kwy_fft_inplace_rest<LOG2H, NT, false>(B, twH, twP);
    if (path < 3) {
      kwy_c *o = (path == 0 ? out_dense : (path == 1 ? out_sparse : out_half)) + (size_t)blockIdx.x * H;
      for (int i = tid; i < H; i += NT) o[i] = B[i];
    } else {
      if (path == 3) {
        kwy_syn_rsplit<LOG2H, NT, V>(B, twb, twN);
        kwy_syn_fold<LOG2H, NT, true>(B);
      } else {
        kwy_syn_rsplit_fold<LOG2H, NT, V, true>(B, twb, twN);
      }
      double *o = (path == 3 ? fold_ref : fold_new) + (size_t)blockIdx.x * (H + 1);
      for (int i = tid; i <= H; i += NT) o[i] = L[i];
    }
    __syncthreads();
  }
}

extern "C" int kwy_debug_syn_first_passes_dev(void *stream, const double *x, int problems, double *out_dense,
                                              double *out_sparse, double *out_half, double *fold_ref, double *fold_new) {
  if (!x || !out_dense || !out_sparse || !out_half || !fold_ref || !fold_new || problems <= 0) return -1;
  constexpr int LOG2H = 10, H = 1 << LOG2H;
  hipStream_t s = (hipStream_t)stream;
  fft_tables t(s, LOG2H, H / 8, true);
  int rc = t.rc;
  if (rc == 0) {
    const size_t lds = sizeof(kwy_c) * (H + 1);
    hipLaunchKernelGGL(k_syn_first_passes_selftest<0>, dim3(problems), dim3(128), lds, s, (const kwy_c *)x, t.twH, t.twP, t.twN,
                       (kwy_c *)out_dense, (kwy_c *)out_sparse, (kwy_c *)out_half, fold_ref, fold_new);
    if (hipGetLastError() != hipSuccess) rc = -2;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = -2;
  return rc;
}

// ---- diagnostic: the transform on thread-held factors, dense and with the half-input first pass -----------------------
// (one NT-thread workgroup per row of H complex, the shapes of k_d4c_body: H = 1024 and 2048 with 256 threads, 4096 with
// 512.  The half path copies points 0 .. H/2 of the row and puts `stale` -- whatever the caller likes, NaNs included --
// where the dense path has the row's upper points, which the half transform must not read.  TAIL = false stops both
// paths in front of the closing radix-4 / radix-2 pass.)
template <int LOG2H, int NT, bool INV, bool TAIL>
__global__ __launch_bounds__(NT) void k_fft_half_w_selftest(const kwy_c *__restrict__ x, const kwy_c *__restrict__ stale,
                                                            const kwy_c *__restrict__ twH, const kwy_c *__restrict__ twP,
                                                            kwy_c *__restrict__ out_dense, kwy_c *__restrict__ out_half) {
  constexpr int H = 1 << LOG2H;
  extern __shared__ double smem[];
  kwy_c *B = (kwy_c *)smem;          // H complex
  const int tid = threadIdx.x;
  const kwy_c *row = x + (size_t)blockIdx.x * H, *old = stale + (size_t)blockIdx.x * H;
  kwy_c tw4[4];
  kwy_fft_thread_twiddles<LOG2H, NT>(twH, tw4);
#pragma nounroll
  for (int path = 0; path < 2; ++path) {
    kwy_c *o = (path == 0 ? out_dense : out_half) + (size_t)blockIdx.x * H;
    for (int i = tid; i < H; i += NT) B[i] = (path == 0 || i <= H / 2) ? row[i] : old[i];
    __syncthreads();
    if (path == 0) kwy_fft_inplace_w<LOG2H, NT, INV, TAIL>(B, tw4, twP);
    else kwy_fft_inplace_sel_w<LOG2H, NT, INV, TAIL>(B, tw4, twP, true);
    for (int i = tid; i < H; i += NT) o[i] = B[i];
    __syncthreads();
  }
}

template <int LOG2H, int NT, bool INV, bool TAIL>
static int fft_half_w_launch(hipStream_t stream, const kwy_c *x, const kwy_c *stale, int problems, const kwy_c *twH,
                             const kwy_c *twP, kwy_c *out_dense, kwy_c *out_half) {
  const size_t lds = sizeof(kwy_c) * (1 << LOG2H);
  auto kern = k_fft_half_w_selftest<LOG2H, NT, INV, TAIL>;
  if (hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -2;
  hipLaunchKernelGGL(kern, dim3(problems), dim3(NT), lds, stream, x, stale, twH, twP, out_dense, out_half);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template <int LOG2H, int NT>
static int fft_half_w_pick(hipStream_t s, bool inv, bool tail, const kwy_c *x, const kwy_c *stale, int problems,
                           const kwy_c *twH, const kwy_c *twP, kwy_c *od, kwy_c *oh) {
  if (inv) return tail ? fft_half_w_launch<LOG2H, NT, true, true>(s, x, stale, problems, twH, twP, od, oh)
                       : fft_half_w_launch<LOG2H, NT, true, false>(s, x, stale, problems, twH, twP, od, oh);
  return tail ? fft_half_w_launch<LOG2H, NT, false, true>(s, x, stale, problems, twH, twP, od, oh)
              : fft_half_w_launch<LOG2H, NT, false, false>(s, x, stale, problems, twH, twP, od, oh);
}

extern "C" int kwy_debug_fft_half_w_dev(void *stream, const double *x, const double *stale, int problems, int log2h,
                                        int inverse, int tail, double *out_dense, double *out_half) {
  if (!x || !stale || !out_dense || !out_half || problems <= 0) return -1;
  if (log2h < 10 || log2h > 12) return -1;
  const int H = 1 << log2h;
  hipStream_t s = (hipStream_t)stream;
  fft_tables t(s, log2h, H / 8, false);
  int rc = t.rc;
  if (rc == 0) {
    const kwy_c *cx = (const kwy_c *)x, *cs = (const kwy_c *)stale;
    kwy_c *od = (kwy_c *)out_dense, *oh = (kwy_c *)out_half;
    if (log2h == 10) rc = fft_half_w_pick<10, 256>(s, inverse != 0, tail != 0, cx, cs, problems, t.twH, t.twP, od, oh);
    else if (log2h == 11) rc = fft_half_w_pick<11, 256>(s, inverse != 0, tail != 0, cx, cs, problems, t.twH, t.twP, od, oh);
    else rc = fft_half_w_pick<12, 512>(s, inverse != 0, tail != 0, cx, cs, problems, t.twH, t.twP, od, oh);
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = -2;
  return rc;
}

// ---- diagnostic: the 2048-point transform up to the drained pairs, Stockham chain against the wave-local form --------
// (one 256-thread workgroup per row, the shape of k_d4c_body<12> / k_d4c_bands<12>.  Both paths start from a buffer that
// holds the row of `stale` in all H + 1 points -- what the previous transform, the smoothing or the select left there --
// and fill what their kind of input fills: see kwy_selftest.h.)
template <bool SPARSE>
__global__ __launch_bounds__(256) void k_fft_wave_local_selftest(const kwy_c *__restrict__ x, const kwy_c *__restrict__ stale,
                                                                 const kwy_c *__restrict__ twH, const kwy_c *__restrict__ twP,
                                                                 int kind, kwy_c *__restrict__ out_old,
                                                                 kwy_c *__restrict__ out_new) {
  constexpr int LOG2H = 11, H = 1 << LOG2H, NT = 256;
  extern __shared__ double smem[];
  kwy_c *B = (kwy_c *)smem;          // H + 1 complex
  const int tid = threadIdx.x;
  const kwy_c *row = x + (size_t)blockIdx.x * H, *old = stale + (size_t)blockIdx.x * (H + 1);
  const bool half = kind == 1 || kind == 2;
#pragma nounroll
  for (int path = 0; path < 2; ++path) {
    kwy_c *o = (path == 0 ? out_old : out_new) + ((size_t)blockIdx.x * NT + tid) * 9;
    for (int i = tid; i <= H; i += NT) B[i] = old[i];
    __syncthreads();
    if (!SPARSE) {
      const int n = half ? H / 2 + 1 : H;
      for (int i = tid; i < n; i += NT) B[i] = (kind == 2 && i == H / 2) ? kwy_c{0.0, 0.0} : row[i];
      __syncthreads();
    }
    kwy_c tw4[4], lo[4], hi[4], md;
    if (path == 0) {
      kwy_fft_thread_twiddles<LOG2H, NT>(twH, tw4);
      if constexpr (SPARSE) {
        kwy_fft_pass8_first_sparse_core<LOG2H, NT, false>(B, kwy_tw_reg{tw4[0]}, row[tid], tid == 0 ? row[H / 8] : kwy_c{0.0, 0.0});
        kwy_fft_inplace_rest_w<LOG2H, NT, false, false>(B, tw4, twP);
      } else {
        kwy_fft_inplace_sel_w<LOG2H, NT, false, false>(B, tw4, twP, half);
      }
      kwy_fft_tail4_drain<LOG2H, NT, false>(B, lo, hi, md);
    } else {
      kwy_fftwl_thread_twiddles(twH, tid, tw4);
      if constexpr (SPARSE) kwy_fftwl_first_sparse<false>(B, kwy_tw_reg{tw4[0]}, row[tid], tid == 0 ? row[H / 8] : kwy_c{0.0, 0.0});
      else kwy_fftwl_first_sel<false>(B, kwy_tw_reg{tw4[0]}, half);
      kwy_fftwl_rest<false>(B, kwy_tw_reg{tw4[1]}, twP);
      kwy_fftwl_tail4_drain<false>(B, lo, hi, md);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) { o[s] = lo[s]; o[4 + s] = hi[s]; }
    o[8] = md;
    __syncthreads();
  }
}

extern "C" int kwy_debug_fft_wave_local_dev(void *stream, const double *x, const double *stale, int problems, int kind,
                                            double *out_old, double *out_new) {
  if (!x || !stale || !out_old || !out_new || problems <= 0 || kind < 0 || kind > 3) return -1;
  constexpr int LOG2H = 11, H = 1 << LOG2H;
  hipStream_t s = (hipStream_t)stream;
  fft_tables t(s, LOG2H, H / 8, false);
  int rc = t.rc;
  const size_t lds = sizeof(kwy_c) * (H + 1);
  auto kern = kind == 3 ? k_fft_wave_local_selftest<true> : k_fft_wave_local_selftest<false>;
  if (rc == 0 && hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) rc = -2;
  if (rc == 0) {
    hipLaunchKernelGGL(kern, dim3(problems), dim3(256), lds, s, (const kwy_c *)x, (const kwy_c *)stale, t.twH, t.twP, kind,
                       (kwy_c *)out_old, (kwy_c *)out_new);
    if (hipGetLastError() != hipSuccess) rc = -2;
  }
  if (hipStreamSynchronize(s) != hipSuccess) rc = -2;
  return rc;
}
