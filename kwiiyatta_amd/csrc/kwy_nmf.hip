// kwy_nmf.hip -- exemplar-based (NMF) spectral conversion on gfx950: include/kwy.h, "exemplar-based conversion".
//
// A frame is explained as a sparse non-negative combination of source exemplars (KL-NMF activations, Takashima et al.
// 2012; Wu, Virtanen, Chng, Li 2014), and the same activations applied to the paired target exemplars are the converted
// frame.  The reference has no counterpart.  Per multiplicative update, all on v_mfma_f64_16x16x4_f64:
//
//   k_nmf_gemm<RATIO>    R = H S     (T x B, K = A), epilogue Q = X / max(R, DBL_MIN)
//   k_nmf_gemm<UPDATE>   G = Q S^T   (T x A, K = B), epilogue H <- H G / (1 + lambda)
// and to close
//   k_nmf_gemm<APPLY>    Y = H Tg    (T x B, K = A)
//   k_nmf_gemm<MODEL>    R = H S stored as it is, for k_nmf_objective: KL(X || R) + lambda sum H per frame
//   k_nmf_pad            the caller's matrices into the padded scratch, counting the entries outside the contract
//   k_nmf_unpad          H back out;   k_nmf_status   the counts into the status word
//
// One tile shape for all products: a workgroup of four wavefronts owns 128 rows x 64 columns, a wavefront the 32-row
// pair tile of k_km_assign / k_nn_search against four column blocks (eight accumulator chains).  BOTH operands stream
// through LDS here -- K is the number of atoms, up to 8192, so the rows cannot stay in registers as the queries of
// k_nn_search do -- in tiles of 16 k (four k-steps), in fragment order (kwy_mfma.hpp), two tiles in LDS: the loads of
// the next tile are issued before the MFMAs of the current one and are stored behind them, one barrier per tile.
// Fragments are NMF_FS = 80 doubles apart, not 64: a wavefront still reads one with a conflict-free 512-byte load,
// and the staging stores of neighbouring fragments fall into different halves of the banks.
//
// Bits.  Every element of every product is one accumulator chain over its k-steps in ascending order from zero; the
// padding (atoms beyond A, bins beyond B, frames beyond T) is zeros, which add +0.  Nothing depends on T, on the
// number of updates asked for or on the launch: a frame's result after n updates is the same bits in any call.
#include <float.h>
#include <math.h>

#include "kwy_internal.hpp"
#include "kwy_mfma.hpp"
#include "kwy_nmf_args.hpp"

#define NMF_NT 256
#define NMF_FS 80                             // doubles from one LDS fragment to the next
#define NMF_AFR (NMF_ROWS / 16 * 4)           // fragments of a tile of the row operand: 8 row blocks x 4 k-steps
#define NMF_BFR (NMF_COLS / 16 * 4)           // of the column operand: 4 column blocks x 4 k-steps
#define NMF_TILE ((NMF_AFR + NMF_BFR) * NMF_FS)

enum { NMF_RATIO = 0, NMF_UPDATE = 1, NMF_APPLY = 2, NMF_MODEL = 3 };

// P: the row operand, rows x lda with k contiguous (H or Q, padded: rows a multiple of 128, lda of 64).
// W: the column operand.  WK false: K x ldw with the columns contiguous (S or Tg as they are stored, atoms the k);
//    WK true: columns x ldw with k contiguous (S again, atoms the columns: the product with S^T).
// K (a multiple of 16) k are summed; ncb column blocks of 16 exist, the tile of blockIdx.y starts at block 4 blockIdx.y.
// out / aux by MODE: RATIO out = Q, aux = X (both ldo); UPDATE out = H in place (ldo); MODEL out = R (ldo);
// APPLY out = Y, T x B exactly as the caller has it (rows < T and columns < B are written).
// The tile of one workgroup with NB of its four column blocks in existence (the last tile of a row of tiles may have
// fewer: B = 257 is 17 blocks).  A template over NB, not a test inside the loop: the accumulator chains of the
// blocks that exist are then plain straight-line code.
template <int MODE, bool WK, int NB>
__device__ __forceinline__ void nmf_tile(double *sm, const double *__restrict__ P, int lda, const double *__restrict__ W,
                                         int ldw, int K, double *out, const double *aux, int ldo, int64_t T, int B,
                                         double scale) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ar = lane & 15, ak = lane >> 4;
  const int64_t t0 = (int64_t)blockIdx.x * NMF_ROWS;
  const int n0 = blockIdx.y * NMF_COLS;

  // staging.  Row operand: thread (row = idx >> 2, ks = idx & 3), idx = tid + 256 i, takes the four k of that k-step:
  // four lanes read 128 contiguous bytes of a row.  They go to fragment (row >> 4, ks), lanes 16 ak + (row & 15).
  double pa[2][4], pw[4];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + NMF_NT * i;
      const double *p = P + (t0 + (idx >> 2)) * lda + k0 + 4 * (idx & 3);
#pragma unroll
      for (int j = 0; j < 4; ++j) pa[i][j] = p[j];
    }
    if constexpr (WK) {                                   // 64 columns x 4 k-steps: one (column, k-step) per thread
      const double *p = W + (int64_t)(n0 + (tid >> 2)) * ldw + k0 + 4 * (tid & 3);
#pragma unroll
      for (int j = 0; j < 4; ++j) pw[j] = p[j];
    } else {                                              // k = 4 i + wv, column = lane: 512 contiguous bytes
#pragma unroll
      for (int i = 0; i < 4; ++i) pw[i] = W[(int64_t)(k0 + 4 * i + wv) * ldw + n0 + lane];
    }
  };
  auto store = [&](double *buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + NMF_NT * i, row = idx >> 2, ks = idx & 3;
      double *d = buf + ((row >> 4) * 4 + ks) * NMF_FS + (row & 15);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[16 * j] = pa[i][j];
    }
    double *wb = buf + NMF_AFR * NMF_FS;
    if constexpr (WK) {
      const int col = tid >> 2, ks = tid & 3;
      double *d = wb + ((col >> 4) * 4 + ks) * NMF_FS + (col & 15);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[16 * j] = pw[j];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) wb[((lane >> 4) * 4 + i) * NMF_FS + 16 * wv + ar] = pw[i];
    }
  };

  kwy_v4f64 acc0[NB], acc1[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc0[nb] = acc1[nb] = kwy_v4f64{0.0, 0.0, 0.0, 0.0};

  const int ntiles = K / 16;
  load(0);
  store(sm);
  __syncthreads();
  for (int it = 0; it < ntiles; ++it) {
    const double *cur = sm + (it & 1) * NMF_TILE;
    const bool more = it + 1 < ntiles;                    // (uniform)
    if (more) load(16 * (it + 1));
    const double *fa = cur + (2 * wv) * 4 * NMF_FS + lane;
    const double *fw = cur + NMF_AFR * NMF_FS + lane;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const double a0 = fa[ks * NMF_FS], a1 = fa[(4 + ks) * NMF_FS];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const double b = fw[(nb * 4 + ks) * NMF_FS];
        acc0[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc0[nb], 0, 0, 0);
        acc1[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc1[nb], 0, 0, 0);
      }
    }
    if (more) store(sm + ((it & 1) ^ 1) * NMF_TILE);
    __syncthreads();
  }

  // D[row ak + 4 r][column ar] of every accumulator
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int c = n0 + 16 * nb + ar;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t t = t0 + 32 * wv + 16 * h + ak + 4 * r;
        const double v = h ? acc1[nb][r] : acc0[nb][r];
        if constexpr (MODE == NMF_RATIO) {
          out[t * ldo + c] = aux[t * ldo + c] / fmax(v, DBL_MIN);
        } else if constexpr (MODE == NMF_UPDATE) {
          out[t * ldo + c] = out[t * ldo + c] * v / scale;
        } else if constexpr (MODE == NMF_MODEL) {
          out[t * ldo + c] = v;
        } else {
          if (t < T && c < B) out[t * B + c] = v;
        }
      }
  }
}

template <int MODE, bool WK>
__global__ __launch_bounds__(NMF_NT) void k_nmf_gemm(const double *__restrict__ P, int lda, const double *__restrict__ W,
                                                    int ldw, int K, int ncb, double *out, const double *aux, int ldo,
                                                    int64_t T, int B, double scale) {
  __shared__ double sm[2 * NMF_TILE];
  const int nblk = ncb - 4 * (int)blockIdx.y;             // (uniform) column blocks of this tile that exist
  if (nblk >= 4) nmf_tile<MODE, WK, 4>(sm, P, lda, W, ldw, K, out, aux, ldo, T, B, scale);
  else if (nblk == 3) nmf_tile<MODE, WK, 3>(sm, P, lda, W, ldw, K, out, aux, ldo, T, B, scale);
  else if (nblk == 2) nmf_tile<MODE, WK, 2>(sm, P, lda, W, ldw, K, out, aux, ldo, T, B, scale);
  else nmf_tile<MODE, WK, 1>(sm, P, lda, W, ldw, K, out, aux, ldo, T, B, scale);
}

// dst (prows x ld) <- src (rows x cols, or `fill` everywhere when src is null), zeros beyond.  CHECK 1: an entry of
// src that is not finite and > 0 is counted; CHECK 2: one that is not finite and >= 0; into bad[blockIdx.x].
template <int CHECK>
__global__ __launch_bounds__(KWY_THREADS) void k_nmf_pad(const double *__restrict__ src, int64_t rows, int cols,
                                                        double fill, double *__restrict__ dst, int64_t prows, int ld,
                                                        int *__restrict__ bad) {
  __shared__ int red[KWY_THREADS];
  const int64_t total = prows * ld;
  int n = 0;
  for (int64_t base = (int64_t)blockIdx.x * KWY_THREADS; base < total; base += (int64_t)gridDim.x * KWY_THREADS) {
    const int64_t idx = base + threadIdx.x;
    if (idx < total) {
      const int64_t r = idx / ld;
      const int c = (int)(idx - r * ld);
      double v = 0.0;
      if (r < rows && c < cols) {
        v = src ? src[r * cols + c] : fill;
        if (CHECK == 1) n += !(v > 0.0 && v < INFINITY);
        if (CHECK == 2) n += !(v >= 0.0 && v < INFINITY);
      }
      dst[idx] = v;
    }
  }
  if (CHECK) {
    red[threadIdx.x] = n;
    __syncthreads();
    for (int w = KWY_THREADS / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) bad[blockIdx.x] = red[0];
  }
}

// dst (rows x cols) <- the first columns of src (rows of ld)
__global__ __launch_bounds__(KWY_THREADS) void k_nmf_unpad(const double *__restrict__ src, int ld,
                                                          double *__restrict__ dst, int64_t rows, int cols) {
  const int64_t total = rows * cols;
  for (int64_t idx = (int64_t)blockIdx.x * KWY_THREADS + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * KWY_THREADS) {
    const int64_t r = idx / cols;
    dst[idx] = src[r * ld + (idx - r * cols)];
  }
}

// objective[t] = sum_b (x log(x / max(r, DBL_MIN)) - x + r) + lambda sum_a h: one wavefront per frame, lane l takes
// the bins (atoms) l, l + 64, .. in ascending order, then the lanes are summed in a fixed tree
__global__ __launch_bounds__(64) void k_nmf_objective(const double *__restrict__ X, const double *__restrict__ R, int ldb,
                                                     int B, const double *__restrict__ H, int lda, int A, double lambda,
                                                     double *__restrict__ objective) {
  __shared__ double red[64];
  const int64_t t = blockIdx.x;
  const double *x = X + t * ldb, *r = R + t * ldb, *h = H + t * lda;
  double kl = 0.0, hs = 0.0;
  for (int b = threadIdx.x; b < B; b += 64) kl += x[b] * log(x[b] / fmax(r[b], DBL_MIN)) - x[b] + r[b];
  for (int a = threadIdx.x; a < A; a += 64) hs += h[a];
  red[threadIdx.x] = kl + lambda * hs;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) objective[t] = red[0];
}

// status[0] = sum of bad[0 .. n) (one workgroup; integers, so the order does not matter)
__global__ __launch_bounds__(KWY_THREADS) void k_nmf_status(const int *__restrict__ bad, int n,
                                                           int32_t *__restrict__ status) {
  __shared__ long long red[KWY_THREADS];
  long long s = 0;
  for (int i = threadIdx.x; i < n; i += KWY_THREADS) s += bad[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = KWY_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) status[0] = (int32_t)min(red[0], (long long)0x7fffffff);
}

// ---- C ABI ------------------------------------------------------------------------------------------
extern "C" size_t kwy_nmf_scratch_bytes(int A, int B, int64_t T) { return nmf_scratch_bytes(A, B, T); }

static int nmf_check(kwy_ctx *ctx, const double *S, const double *Tg, const double *X, int A, int B, int64_t T,
                     int iterations, double sparsity, const double *Y, const double *H, const double *objective) {
  if (!ctx) return KWY_EINVAL;
  if (const char *e = nmf_sizes_error(A, B, T, iterations, sparsity)) { ctx->err = e; return KWY_EINVAL; }
  if (T == 0) return KWY_OK;
  if (const char *e = nmf_pointers_error(S, Tg, X, Y, H, objective)) { ctx->err = e; return KWY_EINVAL; }
  return KWY_OK;
}

static unsigned nmf_pad_grid(int64_t elements) {
  const int64_t blocks = (elements + KWY_THREADS - 1) / KWY_THREADS;
  return (unsigned)(blocks < NMF_PAD_BLOCKS ? (blocks < 1 ? 1 : blocks) : NMF_PAD_BLOCKS);
}

template <int MODE, bool WK>
static void nmf_gemm(kwy_ctx *ctx, const char *name, const nmf_layout &L, const double *P, int lda, const double *W,
                     int ldw, int K, int ncb, double *out, const double *aux, int ldo, int64_t T, int B, double scale) {
  const dim3 grid((unsigned)(L.Tp / NMF_ROWS), (unsigned)((ncb + 3) / 4));
  KWY_PROF(ctx, name, hipLaunchKernelGGL((k_nmf_gemm<MODE, WK>), grid, dim3(NMF_NT), 0, ctx->stream, P, lda, W, ldw, K, ncb, out, aux, ldo, T, B, scale));
}

// all device pointers; `scratch` holds nmf_scratch_bytes(A, B, T) bytes
static int nmf_core(kwy_ctx *ctx, const double *S, const double *Tg, const double *X, int A, int B, int64_t T,
                    int iterations, double sparsity, const double *h0, double *Y, double *H, double *objective,
                    int32_t *status, void *scratch) {
  const nmf_layout L = nmf_make_layout(A, B, T);
  char *base = (char *)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
  double *dS = (double *)(base + L.off_S), *dT = (double *)(base + L.off_Tg), *dX = (double *)(base + L.off_X);
  double *dQ = (double *)(base + L.off_Q), *dH = (double *)(base + L.off_H);
  int *bad = (int *)(base + L.off_bad);
  const dim3 nt(KWY_THREADS);
  if (status) KWY_HIP(hipMemsetAsync(bad, 0, sizeof(int) * 5 * NMF_PAD_BLOCKS, ctx->stream));
  hipLaunchKernelGGL(k_nmf_pad<1>, dim3(nmf_pad_grid((int64_t)L.Ap * L.Bp)), nt, 0, ctx->stream, S, (int64_t)A, B, 0.0, dS,
                     (int64_t)L.Ap, L.Bp, bad);
  if (Tg)
    hipLaunchKernelGGL(k_nmf_pad<1>, dim3(nmf_pad_grid((int64_t)L.Ap * L.Bp)), nt, 0, ctx->stream, Tg, (int64_t)A, B, 0.0,
                       dT, (int64_t)L.Ap, L.Bp, bad + NMF_PAD_BLOCKS);
  hipLaunchKernelGGL(k_nmf_pad<1>, dim3(nmf_pad_grid(L.Tp * L.Bp)), nt, 0, ctx->stream, X, T, B, 0.0, dX, L.Tp, L.Bp,
                     bad + 2 * NMF_PAD_BLOCKS);
  hipLaunchKernelGGL(k_nmf_pad<2>, dim3(nmf_pad_grid(L.Tp * L.Ap)), nt, 0, ctx->stream, h0, T, A, 1.0, dH, L.Tp, L.Ap,
                     bad + 3 * NMF_PAD_BLOCKS);
  if (status) hipLaunchKernelGGL(k_nmf_status, dim3(1), nt, 0, ctx->stream, bad, 5 * NMF_PAD_BLOCKS, status);
  const double scale = 1.0 + sparsity;
  for (int n = 0; n < iterations; ++n) {
    nmf_gemm<NMF_RATIO, false>(ctx, "k_nmf_ratio", L, dH, L.Ap, dS, L.Bp, L.A16, L.B16 / 16, dQ, dX, L.Bp, T, B, 0.0);
    nmf_gemm<NMF_UPDATE, true>(ctx, "k_nmf_update", L, dQ, L.Bp, dS, L.Bp, L.B16, L.A16 / 16, dH, nullptr, L.Ap, T, B, scale);
  }
  if (Y) nmf_gemm<NMF_APPLY, false>(ctx, "k_nmf_apply", L, dH, L.Ap, dT, L.Bp, L.A16, L.B16 / 16, Y, nullptr, 0, T, B, 0.0);
  if (H) hipLaunchKernelGGL(k_nmf_unpad, dim3(nmf_pad_grid(T * A)), nt, 0, ctx->stream, dH, L.Ap, H, T, A);
  if (objective) {
    nmf_gemm<NMF_MODEL, false>(ctx, "k_nmf_model", L, dH, L.Ap, dS, L.Bp, L.A16, L.B16 / 16, dQ, nullptr, L.Bp, T, B, 0.0);
    hipLaunchKernelGGL(k_nmf_objective, dim3((unsigned)T), dim3(64), 0, ctx->stream, dX, dQ, L.Bp, B, dH, L.Ap, A, sparsity,
                       objective);
  }
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

extern "C" int kwy_nmf_convert_dev(kwy_ctx *ctx, const double *S, const double *Tg, const double *X, int A, int B,
                                   int64_t T, int iterations, double sparsity, const double *h0, double *Y, double *H,
                                   double *objective, int32_t *status, void *scratch, size_t scratch_bytes) {
  KWY_TRY(nmf_check(ctx, S, Tg, X, A, B, T, iterations, sparsity, Y, H, objective));
  if (T == 0) return KWY_OK;
  if (!scratch || scratch_bytes < nmf_scratch_bytes(A, B, T)) {
    ctx->err = "nmf_convert: the scratch buffer holds fewer than kwy_nmf_scratch_bytes(A, B, T) bytes";
    return KWY_EINVAL;
  }
  KWY_HIP(hipSetDevice(ctx->device));
  return nmf_core(ctx, S, Tg, X, A, B, T, iterations, sparsity, h0, Y, H, objective, status, scratch);
}

extern "C" int kwy_nmf_convert(kwy_ctx *ctx, const double *S, const double *Tg, const double *X, int A, int B, int64_t T,
                               int iterations, double sparsity, const double *h0, double *Y, double *H,
                               double *objective, int32_t *status) {
  KWY_TRY(nmf_check(ctx, S, Tg, X, A, B, T, iterations, sparsity, Y, H, objective));
  if (T == 0) return KWY_OK;
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "nmf_convert");
  double *dS, *dT, *dX, *dh0, *dY, *dH, *dO;
  int32_t *ds;
  char *scratch;
  st.in(dS, S, (size_t)A * B);
  st.in(dT, Tg, Tg ? (size_t)A * B : (size_t)0);
  st.in(dX, X, (size_t)T * B);
  st.in(dh0, h0, h0 ? (size_t)T * A : (size_t)0);
  st.out(dY, Y, Y ? (size_t)T * B : (size_t)0);
  st.out(dH, H, H ? (size_t)T * A : (size_t)0);
  st.out(dO, objective, objective ? (size_t)T : (size_t)0);
  st.out(ds, status, status ? (size_t)1 : (size_t)0);
  st.tmp(scratch, nmf_scratch_bytes(A, B, T));
  KWY_TRY(st.begin());
  KWY_TRY(nmf_core(ctx, dS, Tg ? dT : nullptr, dX, A, B, T, iterations, sparsity, h0 ? dh0 : nullptr, Y ? dY : nullptr,
                   H ? dH : nullptr, objective ? dO : nullptr, status ? ds : nullptr, scratch));
  return st.finish();
}
