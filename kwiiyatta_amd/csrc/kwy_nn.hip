// kwy_nn.hip -- all-pairs nearest-neighbour search on gfx950: the hot path of non-parallel (INCA) training.
//
// INCA (Erro, Moreno, Bonafonte 2010) pairs every source frame with its nearest target frame and every target frame
// with its nearest source frame, fits the mixture on those pairs, converts, and searches again.  The search is
// 2 nq nc D flop per direction and has no counterpart in the reference, which trains on parallel data only.
//
//   k_nn_search   s(t, j) = |c_j|^2 - 2 <q_t, c_j> on v_mfma_f64_16x16x4_f64, arg-min in registers: k_km_assign's
//                 arithmetic with the B operand STREAMED -- k_km_assign keeps <= 256 centres in LDS for the whole
//                 kernel, here 10^5 .. 10^6 candidate rows pass through LDS in tiles of 64
//   k_nn_merge    the lexicographic (score, index) minimum over the slices of the candidate range, and the distance
//                 of the winner recomputed directly
//   k_nn_status   the number of queries without a finite score
//
// Bits.  The score of a pair is cn - 2 acc with cn = sum_k c_k^2 (k ascending, no contraction) and acc the chain of
// the pair's k-steps in ascending order starting from zero; columns beyond D are zeros on both sides, which add +0.
// Neither depends on the tile, the slice or the launch the pair falls into, so the result does not depend on `splits`.
#include <math.h>

#include <atomic>

#include "kwy_internal.hpp"
#include "kwy_mfma.hpp"

#define NN_NT 512          // eight wavefronts of 32 query rows: 256 queries per workgroup
#define NN_TILE 64         // candidate rows per LDS tile
#define NN_NONE 0x7fffffff // index of "no finite score"
#define NN_MAX_DEVICES 64  // devices whose raised LDS limits are remembered

// Slice s of the candidate range is [s L, min(nc, (s + 1) L)), L = kwy_nn_slice(nc, splits): whole tiles
static int64_t nn_slice(int64_t nc, int splits) {
  const int64_t per = (nc + splits - 1) / splits;
  return (per + NN_TILE - 1) / NN_TILE * NN_TILE;
}

// Grid: (query tiles of 256, slices).  pv / pi: [slices][nq] best score / candidate of the slice, (+inf, NN_NONE)
// where the slice has no candidate with a finite score.
// A wavefront holds its 32 query rows as A fragments (the pair tile of k_km_assign) for the whole kernel.  A tile is
// 64 candidates in fragment order (kwy_mfma.hpp, rectangular: fragment (mb, ks) at mb KS + ks) plus their 64 norms,
// +inf behind the end of the slice: a padded row scores +inf and cannot win, whatever the query.
// DB: two tiles in LDS; the loads of the next one are issued before the MFMAs of the current one and land in LDS
// after them, one barrier per tile.  Without it (KS > 16: a tile of D = 160 is 80 KB) one tile, two barriers.
template <int KS, bool DB>
__global__ __launch_bounds__(NN_NT) void k_nn_search(const double *__restrict__ Q, int64_t nq,
                                                    const double *__restrict__ C, int64_t nc, int D, int64_t slice,
                                                    double *__restrict__ pv, int *__restrict__ pi) {
  constexpr int TILE = 4 * KS * 64;                       // doubles of a tile
  constexpr int PER = (TILE + NN_NT - 1) / NN_NT;         // elements a thread stages
  extern __shared__ double sm[];                          // nn_lds_doubles(KS, DB)
  double *cf = sm;                                        // (DB ? 2 : 1) x TILE
  double *cn = sm + (DB ? 2 : 1) * TILE;                  // (DB ? 2 : 1) x 64
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ar = lane & 15, ak = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.y * slice, c1 = min(nc, c0 + slice);
  const int ntiles = c1 > c0 ? (int)((c1 - c0 + NN_TILE - 1) / NN_TILE) : 0;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + 32 * wv;
  const bool live = t0 < nq;                              // (uniform over the wavefront)

  double a0[KS], a1[KS];
  {
    const double *xa = Q + min(t0 + ar, nq - 1) * D, *xb = Q + min(t0 + 16 + ar, nq - 1) * D;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = 4 * ks + ak;
      a0[ks] = k < D ? xa[k] : 0.0;
      a1[ks] = k < D ? xb[k] : 0.0;
    }
  }
  double bv0[4], bv1[4];
  int bi0[4], bi1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { bv0[r] = bv1[r] = INFINITY; bi0[r] = bi1[r] = NN_NONE; }

  // element i of this thread in the tile that starts at candidate j0: fragment f = wv + 8 i, lane `lane`
  auto load = [&](int64_t j0, int i) -> double {
    const int f = wv + 8 * i;
    const int mb = f / KS, ks = f - mb * KS;
    const int64_t j = j0 + 16 * mb + ar;
    const int k = 4 * ks + ak;
    return (f < 4 * KS && j < c1 && k < D) ? C[j * D + k] : 0.0;
  };
  auto norm = [&](int64_t j0) -> double {                 // tid < 64: |c|^2 of candidate j0 + tid
    const int64_t j = j0 + tid;
    double s = INFINITY;
    if (j < c1) {
      const double *c = C + j * D;
      s = 0.0;
      for (int k = 0; k < D; ++k) s += c[k] * c[k];
    }
    return s;
  };
  auto compute = [&](const double *cfb, const double *cnb, int64_t j0) {
    const int nmb = (int)min((int64_t)4, (c1 - j0 + 15) / 16);
    for (int mb = 0; mb < nmb; ++mb) {
      kwy_v4f64 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
      const double *frag = cfb + (size_t)mb * KS * 64 + lane;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const double b = frag[ks * 64];
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[ks], b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[ks], b, acc1, 0, 0, 0);
      }
      const double c2 = cnb[16 * mb + ar];
      const int j = (int)(j0 + 16 * mb + ar);
#pragma unroll
      for (int r = 0; r < 4; ++r) {                       // a score that is not finite is never "less"
        const double d0 = c2 - 2.0 * acc0[r], d1 = c2 - 2.0 * acc1[r];
        if (d0 < bv0[r] && d0 > -INFINITY) { bv0[r] = d0; bi0[r] = j; }
        if (d1 < bv1[r] && d1 > -INFINITY) { bv1[r] = d1; bi1[r] = j; }
      }
    }
  };

  if constexpr (DB) {
    if (ntiles > 0) {
#pragma unroll
      for (int i = 0; i < PER; ++i)
        if (wv + 8 * i < 4 * KS) cf[(wv + 8 * i) * 64 + lane] = load(c0, i);
      if (tid < 64) cn[tid] = norm(c0);
    }
    __syncthreads();
    for (int it = 0; it < ntiles; ++it) {
      const int cur = it & 1;
      const int64_t j0 = c0 + (int64_t)it * NN_TILE;
      const bool more = it + 1 < ntiles;                  // (uniform)
      double nx[PER], nn = 0.0;
      if (more) {
#pragma unroll
        for (int i = 0; i < PER; ++i) nx[i] = load(j0 + NN_TILE, i);
        if (tid < 64) nn = norm(j0 + NN_TILE);
      }
      if (live) compute(cf + cur * TILE, cn + cur * 64, j0);
      if (more) {
        double *dst = cf + (cur ^ 1) * TILE;
#pragma unroll
        for (int i = 0; i < PER; ++i)
          if (wv + 8 * i < 4 * KS) dst[(wv + 8 * i) * 64 + lane] = nx[i];
        if (tid < 64) cn[(cur ^ 1) * 64 + tid] = nn;
      }
      __syncthreads();
    }
  } else {
    for (int it = 0; it < ntiles; ++it) {
      const int64_t j0 = c0 + (int64_t)it * NN_TILE;
      if (it) __syncthreads();
#pragma unroll
      for (int i = 0; i < PER; ++i)
        if (wv + 8 * i < 4 * KS) cf[(wv + 8 * i) * 64 + lane] = load(j0, i);
      if (tid < 64) cn[tid] = norm(j0);
      __syncthreads();
      if (live) compute(cf, cn, j0);
    }
  }
  if (!live) return;
  // over the 16 lanes of the row, once for the whole stream: (score, candidate) lexicographic minimum
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const kwy_val_idx b0 = kwy_row_allreduce(kwy_val_idx{bv0[r], bi0[r]}, kwy_lex_min);
    const kwy_val_idx b1 = kwy_row_allreduce(kwy_val_idx{bv1[r], bi1[r]}, kwy_lex_min);
    bv0[r] = b0.v; bi0[r] = b0.i;
    bv1[r] = b1.v; bi1[r] = b1.i;
  }
  if (ar == 0) {
    double *v = pv + (size_t)blockIdx.y * nq;
    int *ix = pi + (size_t)blockIdx.y * nq;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t t = t0 + ak + 4 * r;
      if (t < nq) { v[t] = bv0[r]; ix[t] = bi0[r]; }
      if (t + 16 < nq) { v[t + 16] = bv1[r]; ix[t + 16] = bi1[r]; }
    }
  }
}

// idx[t] = the candidate of the lexicographic minimum over the slices; dist2[t] = sum_k (q_k - c_k)^2 of that pair,
// k ascending.  Without a finite score: -1 and NaN, counted in bad[block] (bad may be NULL).
__global__ __launch_bounds__(KWY_THREADS) void k_nn_merge(const double *__restrict__ Q, int64_t nq,
                                                         const double *__restrict__ C, int D, int splits,
                                                         const double *__restrict__ pv, const int *__restrict__ pi,
                                                         int *__restrict__ idx, double *__restrict__ dist2,
                                                         int *__restrict__ bad) {
  const int64_t t = (int64_t)blockIdx.x * KWY_THREADS + threadIdx.x;
  int none = 0;
  if (t < nq) {
    kwy_val_idx best{INFINITY, NN_NONE};
    for (int s = 0; s < splits; ++s)
      best = kwy_lex_min(best, kwy_val_idx{pv[(size_t)s * nq + t], pi[(size_t)s * nq + t]});
    if (best.i == NN_NONE) {
      none = 1;
      idx[t] = -1;
      dist2[t] = NAN;
    } else {
      const double *q = Q + t * D, *c = C + (int64_t)best.i * D;
      double s = 0.0;
      for (int k = 0; k < D; ++k) {
        const double d = q[k] - c[k];
        s += d * d;
      }
      idx[t] = best.i;
      dist2[t] = s;
    }
  }
  const int cnt = __syncthreads_count(none);
  if (bad && threadIdx.x == 0) bad[blockIdx.x] = cnt;
}

// status[0] = sum of bad[0 .. n) (one workgroup; integers, so the order does not matter)
__global__ __launch_bounds__(KWY_THREADS) void k_nn_status(const int *__restrict__ bad, int64_t n,
                                                          int32_t *__restrict__ status) {
  __shared__ long long red[KWY_THREADS];
  long long s = 0;
  for (int64_t i = threadIdx.x; i < n; i += KWY_THREADS) s += bad[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = KWY_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) status[0] = (int32_t)min(red[0], (long long)0x7fffffff);
}

// ---- C ABI ------------------------------------------------------------------------------------------
static constexpr size_t nn_lds_doubles(int ks, bool db) { return (size_t)(db ? 2 : 1) * (4 * ks * 64 + 64); }

static int64_t nn_merge_blocks(int64_t nq) { return (nq + KWY_THREADS - 1) / KWY_THREADS; }

extern "C" size_t kwy_nn_scratch_bytes(int64_t nq, int splits) {
  if (nq <= 0) return 0;
  if (splits < 1 || splits > KWY_NN_MAX_SPLITS) splits = KWY_NN_MAX_SPLITS;
  return kwy_pad(sizeof(double) * (size_t)splits * nq) + kwy_pad(sizeof(int) * (size_t)splits * nq) +
         kwy_pad(sizeof(int) * (size_t)nn_merge_blocks(nq));
}

extern "C" int64_t kwy_nn_slice(int64_t nc, int splits) {
  if (nc < 1 || splits < 1 || splits > KWY_NN_MAX_SPLITS) return 0;
  return nn_slice(nc, splits);
}

// the slices for few queries: at least 512 workgroups in the grid, never more slices than tiles of candidates.  At the
// speech case's 162 registers one workgroup of eight wavefronts is resident per CU, so 512 are two rounds of the 256
// CUs (the second evens out slices of unequal length), not one resident fill
static int nn_auto_splits(int64_t nq, int64_t nc) {
  const int64_t qtiles = (nq + 255) / 256, ctiles = (nc + NN_TILE - 1) / NN_TILE;
  int64_t s = (512 + qtiles - 1) / qtiles;
  if (s > ctiles) s = ctiles;
  if (s > KWY_NN_MAX_SPLITS) s = KWY_NN_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

template <int KS, bool DB>
static int nn_launch(kwy_ctx *ctx, const double *Q, int64_t nq, const double *C, int64_t nc, int D, int splits,
                     double *pv, int *pi) {
  const size_t lds = sizeof(double) * nn_lds_doubles(KS, DB);
  // the LDS limit of an instantiation is raised once per device, on its first launch there: later launches (a stream
  // capture among them) are plain launches
  static std::atomic<bool> raised[NN_MAX_DEVICES];
  const bool known = ctx->device >= 0 && ctx->device < NN_MAX_DEVICES;
  if (!known || !raised[ctx->device].load()) {
    KWY_HIP(hipFuncSetAttribute((const void *)k_nn_search<KS, DB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (known) raised[ctx->device].store(true);
  }
  const dim3 grid((unsigned)((nq + 255) / 256), (unsigned)splits);
  KWY_PROF(ctx, "k_nn_search", hipLaunchKernelGGL((k_nn_search<KS, DB>), grid, dim3(NN_NT), lds, ctx->stream, Q, nq, C, nc, D, nn_slice(nc, splits), pv, pi));
  return KWY_OK;
}

// one instantiation per number of k-steps up to 16 (D <= 64, two tiles in LDS), per four of them above (one tile)
template <int KS = 1>
static int nn_dispatch(int ks, kwy_ctx *ctx, const double *Q, int64_t nq, const double *C, int64_t nc, int D,
                       int splits, double *pv, int *pi) {
  if constexpr (KS > 40) {
    return KWY_EINVAL;
  } else {
    if (ks <= KS) return nn_launch<KS, (KS <= 16)>(ctx, Q, nq, C, nc, D, splits, pv, pi);
    return nn_dispatch<(KS < 16 ? KS + 1 : KS + 4)>(ks, ctx, Q, nq, C, nc, D, splits, pv, pi);
  }
}

static int nn_check(kwy_ctx *ctx, const double *Q, int64_t nq, const double *C, int64_t nc, int D, int splits,
                    const int32_t *idx, const double *dist2) {
  if (!ctx) return KWY_EINVAL;
  if (D < 1 || D > 160) { ctx->err = "nn_search: need 1 <= D <= 160"; return KWY_EINVAL; }
  if (nq < 0) { ctx->err = "nn_search: negative number of queries"; return KWY_EINVAL; }
  if (splits < 0 || splits > KWY_NN_MAX_SPLITS) { ctx->err = "nn_search: splits outside 0 .. KWY_NN_MAX_SPLITS"; return KWY_EINVAL; }
  if (nq == 0) return KWY_OK;
  if (nc < 1 || nc > 0x7fffffffLL) { ctx->err = "nn_search: need 1 <= nc <= 2^31 - 1 candidates"; return KWY_EINVAL; }
  if (!Q || !C || !idx || !dist2) { ctx->err = "nn_search: null pointer"; return KWY_EINVAL; }
  return KWY_OK;
}

// the arena of the call in progress holds the partial results (nn_core takes them; the caller has sized it)
static int nn_core(kwy_ctx *ctx, const double *Q, int64_t nq, const double *C, int64_t nc, int D, int splits,
                   int32_t *idx, double *dist2, int32_t *status) {
  const int64_t blocks = nn_merge_blocks(nq);
  double *pv = kwy_arena<double>(ctx, (size_t)splits * nq);
  int *pi = kwy_arena<int>(ctx, (size_t)splits * nq);
  int *bad = kwy_arena<int>(ctx, (size_t)blocks);
  if (!pv || !pi || !bad) { ctx->err = "nn_search: scratch"; return KWY_ENOMEM; }
  KWY_TRY(nn_dispatch((D + 3) / 4, ctx, Q, nq, C, nc, D, splits, pv, pi));
  hipLaunchKernelGGL(k_nn_merge, dim3((unsigned)blocks), dim3(KWY_THREADS), 0, ctx->stream, Q, nq, C, D, splits, pv, pi,
                     idx, dist2, status ? bad : nullptr);
  if (status) hipLaunchKernelGGL(k_nn_status, dim3(1), dim3(KWY_THREADS), 0, ctx->stream, bad, blocks, status);
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

extern "C" int kwy_nn_search_dev(kwy_ctx *ctx, const double *Q, int64_t nq, const double *C, int64_t nc, int D,
                                 int splits, int32_t *idx, double *dist2, int32_t *status) {
  KWY_TRY(nn_check(ctx, Q, nq, C, nc, D, splits, idx, dist2));
  if (nq == 0) return KWY_OK;
  KWY_HIP(hipSetDevice(ctx->device));
  if (splits == 0) splits = nn_auto_splits(nq, nc);
  KWY_TRY(kwy_arena_begin(ctx, kwy_nn_scratch_bytes(nq, splits)));
  return nn_core(ctx, Q, nq, C, nc, D, splits, idx, dist2, status);
}

extern "C" int kwy_nn_search(kwy_ctx *ctx, const double *Q, int64_t nq, const double *C, int64_t nc, int D, int splits,
                             int32_t *idx, double *dist2, int32_t *status) {
  KWY_TRY(nn_check(ctx, Q, nq, C, nc, D, splits, idx, dist2));
  if (nq == 0) return KWY_OK;
  KWY_HIP(hipSetDevice(ctx->device));
  if (splits == 0) splits = nn_auto_splits(nq, nc);
  kwy_staging st(ctx, "nn_search");
  double *dq, *dc, *dd;
  int32_t *di, *ds;
  st.in(dq, Q, (size_t)nq * D);
  st.in(dc, C, (size_t)nc * D);
  st.out(di, idx, (size_t)nq);
  st.out(dd, dist2, (size_t)nq);
  st.out(ds, status, status ? (size_t)1 : (size_t)0);
  KWY_TRY(st.begin(kwy_nn_scratch_bytes(nq, splits)));
  KWY_TRY(nn_core(ctx, dq, nq, dc, nc, D, splits, di, dd, status ? ds : nullptr));
  return st.finish();
}
