// kwy_mlpg.hip -- GMM-based spectral mapping with MLPG on gfx950.
//
// Replaces, for the converter-apply step of the reference
// (kwiiyatta/converter/delta.py:39-50 and gmm.py:28-34):
//     X  = nnmnkwii.preprocessing.delta_features(x, DELTA_WINDOWS)
//     y  = nnmnkwii.baseline.gmm.MLPG(gmm, windows=DELTA_WINDOWS, diff).transform(X)[:, :d]
//
// Kernels:
//   k_gmm_prep   one workgroup per mixture: Cholesky of S_xx in LDS, its inverse,
//                A = S_yx S_xx^-1 and its transpose, diagonal conditional variance, log-normaliser
//   k_delta      static + delta + delta-delta features (3-tap correlations)
//   k_gmm_logp_frag  (frame tile x mixture) workgroups: ||L^-1 (x - mu)||^2 on the f64 MFMA, L^-1 in fragment order in
//                LDS, the frames in registers (profiled as "k_gmm_logp")
//   k_gmm_cond   four frames per wavefront: arg-max mixture, conditional mean E (from A transposed) and variance D
//   k_mlpg_build per (frame, dim): the pentadiagonal normal equations W'PW, W'P mu
//   k_mlpg_chunks / k_mlpg_finish  per static dim: banded Cholesky, partitioned into chunks (nested dissection)
//   k_em_prep / k_em_estep / k_em_loglik  EM trajectory conversion over soft mixture posteriors (below the others):
//                all M conditional means of a frame tile on the f64 MFMA, online softmax, precision-weighted sums
// Host side, behind the kernels: one core (ml_convert_core) for arg-max, EM and the GV ascent, one driver for the device
// entries (ml_convert_jobs), one staging path for the host-pointer entries (ml_convert_host).
//
// Algorithmic HBM bytes per frame: d*8 in, d*8 out (+ the GMM once per call).
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "kwy_internal.hpp"
#include "kwy_mfma.hpp"

struct ml_dims { int d, D, M; int64_t T; };

// A conversion call handles a batch of up to KWY_BATCH_MAX utterances (a single call is a batch of one).  The frames of
// all of them form ONE matrix for the frame-parallel kernels (log-densities, conditional means: dm.T = all frames);
// the kernels that look at neighbouring frames (deltas, normal equations) and the trajectory solves find their
// utterance u by start[u] <= frame < start[u + 1].  Descriptors travel by value in the kernel arguments.
struct ml_part { int P, base, extra; };
struct ml_seg {
  const double *x;          // T x d static features, rows ldx doubles apart
  double *y;                // T x d converted, rows ldy apart
  const double *keep_in;    // (may be null) one more column copied through, ldx / ldy apart
  double *keep_out;
  ml_part pt;               // chunks of the partitioned trajectory solve
};
struct ml_batch {
  int n, ldx, ldy;
  int64_t start[KWY_BATCH_MAX + 1];
  ml_seg u[KWY_BATCH_MAX];
  __device__ __forceinline__ int find(int64_t t) const {
    int k = 0;
    while (k + 1 < n && t >= start[k + 1]) ++k;
    return k;
  }
};

// ---- per-mixture preparation -----------------------------------------------------
// layout of the prepared model (doubles), per mixture m:
//   Z   [D*D]  lower-triangular inverse of chol(S_xx)   (row j: Z[j][0..j])
//   A   [D*D]  S_yx S_xx^-1
//   mux [D], muy [D], dvar [D], cst [1] (+ padding to 8)
//   AT  [D*D]  A transposed (AT[k][i] = A[i][k]): what k_gmm_cond reads, consecutive lanes consecutive doubles
__host__ __device__ static inline size_t ml_model_stride(int D) { return (size_t)3 * D * D + 3 * D + 8; }
__host__ __device__ static inline size_t ml_model_at(int D) { return (size_t)2 * D * D + 3 * D + 8; }

__global__ __launch_bounds__(KWY_THREADS) void k_gmm_prep(const double *__restrict__ weights,
                                                         const double *__restrict__ means,
                                                         const double *__restrict__ covs, int D, int diff,
                                                         double *__restrict__ model, int *__restrict__ status) {
  extern __shared__ double smem[];
  double *L = smem;          // D x D
  double *Z = L + D * D;     // D x D
  double *W = Z + D * D;     // D x D
  const int tid = threadIdx.x, m = blockIdx.x, D2 = 2 * D;
  const double *C = covs + (size_t)m * D2 * D2;
  double *out = model + (size_t)m * ml_model_stride(D);
  double *oZ = out, *oA = oZ + D * D, *omux = oA + D * D, *omuy = omux + D, *odv = omuy + D, *ocst = odv + D;
  double *oAT = out + ml_model_at(D);

  auto Sxx = [&](int i, int j) { return C[(size_t)i * D2 + j]; };
  auto Sxy = [&](int i, int j) { return diff ? C[(size_t)i * D2 + D + j] - C[(size_t)i * D2 + j] : C[(size_t)i * D2 + D + j]; };
  auto Syx = [&](int i, int j) { return diff ? Sxy(j, i) : C[(size_t)(D + i) * D2 + j]; };
  auto Syy = [&](int i, int j) {
    double v = C[(size_t)(D + i) * D2 + D + j];
    if (diff) v = C[(size_t)i * D2 + j] + v - C[(size_t)i * D2 + D + j] - C[(size_t)(D + i) * D2 + j];
    return v;
  };

  for (int e = tid; e < D * D; e += KWY_THREADS) L[e] = Sxx(e / D, e % D);
  __syncthreads();
  // right-looking Cholesky (same subtraction order per entry as the textbook left-looking form)
  for (int j = 0; j < D; ++j) {
    const double piv = L[j * D + j];
    if (!(piv > 0.0)) { if (tid == 0) atomicExch(status, 1); return; }
    const double dj = sqrt(piv);
    __syncthreads();
    if (tid == 0) L[j * D + j] = dj;
    for (int i = j + 1 + tid; i < D; i += KWY_THREADS) L[i * D + j] = L[i * D + j] / dj;
    __syncthreads();
    const int rem = D - j - 1;
    for (int e = tid; e < rem * rem; e += KWY_THREADS) {
      int i = j + 1 + e / rem, k = j + 1 + e % rem;
      if (k <= i) L[i * D + k] -= L[i * D + j] * L[k * D + j];
    }
    __syncthreads();
  }
  // Z = L^-1 (lower): column c by thread c
  for (int c = tid; c < D; c += KWY_THREADS) {
    for (int i = 0; i < D; ++i) {
      double v = (i == c) ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) v -= L[i * D + k] * Z[k * D + c];
      Z[i * D + c] = (i < c) ? 0.0 : v / L[i * D + i];
    }
  }
  __syncthreads();
  // W = S_yx Z'   (W[r][j] = sum_i Syx[r][i] Z[j][i])
  for (int e = tid; e < D * D; e += KWY_THREADS) {
    int r = e / D, j = e % D;
    double v = 0.0;
    for (int i = 0; i <= j; ++i) v += Syx(r, i) * Z[j * D + i];
    W[e] = v;
  }
  __syncthreads();
  // A = W Z       (A[r][c] = sum_j W[r][j] Z[j][c])
  for (int e = tid; e < D * D; e += KWY_THREADS) {
    int r = e / D, c = e % D;
    double v = 0.0;
    for (int j = c; j < D; ++j) v += W[r * D + j] * Z[j * D + c];
    oA[e] = v;
    oAT[c * D + r] = v;
    oZ[e] = Z[e];
  }
  for (int i = tid; i < D; i += KWY_THREADS) {
    double mx = means[(size_t)m * D2 + i], my = means[(size_t)m * D2 + D + i];
    omux[i] = mx;
    omuy[i] = diff ? my - mx : my;
    odv[i] = Syy(i, i) - Syx(i, i) / Sxx(i, i) * Sxy(i, i);
  }
  if (tid == 0) {
    double ld = 0.0;
    for (int i = 0; i < D; ++i) ld -= log(L[i * D + i]);
    ocst[0] = -0.5 * (D * log(2.0 * KWY_PI)) + ld + log(weights[m]);
  }
}

// ---- delta features -----------------------------------------------------------------
// DELTA_WINDOWS (kwiiyatta/converter/delta.py:8-12): [1], [-0.5, 0, 0.5], [1, -2, 1]
// x rows are ldx doubles apart.  keep_in / keep_out (may be null): one more column that is copied through
// unchanged (the power coefficient c0 of a mel-cepstrum, kwiiyatta/converter/mcep.py:57-59), ldx / ldy apart.
// NOT kwy_delta_windows: this sums from 0.0 and skips outside taps, which signs some zeros differently (recorded bits).
__global__ void k_delta(ml_batch b, ml_dims dm, double *__restrict__ X) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= dm.T * dm.d) return;
  const int64_t tg = e / dm.d;              // frame of the batch
  const int c = (int)(e % dm.d);
  const int u = b.find(tg);
  const int64_t t = tg - b.start[u], T = b.start[u + 1] - b.start[u];
  const double *__restrict__ x = b.u[u].x;
  const int ldx = b.ldx, ldy = b.ldy;
  if (b.u[u].keep_out && c == 0) b.u[u].keep_out[t * ldy] = b.u[u].keep_in[t * ldx];
  const double xm = t > 0 ? x[(t - 1) * ldx + c] : 0.0;
  const double x0 = x[t * ldx + c];
  const double xp = t + 1 < T ? x[(t + 1) * ldx + c] : 0.0;
  double *o = X + tg * dm.D;
  o[c] = 0.0 + x0 * 1.0;
  double s = 0.0;
  if (t > 0) s += xm * -0.5;
  s += x0 * 0.0;
  if (t + 1 < T) s += xp * 0.5;
  o[dm.d + c] = s;
  s = 0.0;
  if (t > 0) s += xm * 1.0;
  s += x0 * -2.0;
  if (t + 1 < T) s += xp * 1.0;
  o[2 * dm.d + c] = s;
}

// ---- log p(x_t | m) up to the shared constant -------------------------------------------
// || Z_m (x_t - mu_m) ||^2 for a tile of frames and one mixture is a frames x D times D x D (lower-triangular) product:
// the one MFMA-shaped piece of the arg-max conversion path, with the frame operand in registers (the form of
// k_fit_logprob, kwy_gmmfit.hip; fed from LDS alone the MFMA is LDS-bound).  Z_m (zero above the diagonal) is expanded
// once per workgroup into MFMA-fragment order (kwy_mfma.hpp: one conflict-free 512-byte read per operand, 29 KB for
// D = 72).  A wavefront takes 32 frames: x - mu_x of two 16-frame sub-tiles goes straight from global memory into the A
// registers (2 x Kp/4 doubles per lane), and every B fragment feeds two independent accumulator chains.  Per
// logp[t][m]: per 16-column block nb the k-steps min(Kp/4, 4 (nb + 1)) that reach the block's diagonal, from a zero
// accumulator (58 instead of 90 MFMAs per 16 frames for D = 72), the squares summed in ascending nb, then the row sum.
// NBLK = column blocks (D <= 16 NBLK), NW = wavefronts per workgroup.
__host__ __device__ constexpr int ml_kp(int D) { return (D + 3) & ~3; }
__host__ __device__ constexpr int ml_np(int D) { return (D + 15) & ~15; }

#define ML_FRAG_MAXBLK 6    // D <= 96.  The fragments would fit the LDS up to nine blocks (D = 144, 92 KB), but k_gmm_prep
                            // holds three D x D matrices in LDS and admits D <= 82 (checked where ml_prep_lds is defined)
template <int NBLK, int NW>
__global__ __launch_bounds__(64 * NW) void k_gmm_logp_frag(const double *__restrict__ X, ml_dims dm,
                                                          const double *__restrict__ model,
                                                          double *__restrict__ logp) {
  constexpr int KS = 4 * NBLK, TILE = 32 * NW;
  extern __shared__ double smem[];              // kwy_tri_lds_doubles(NBLK)
  double *zf = smem;                            // the fragments of Z_m
  double *mus = zf + kwy_tri_frags(NBLK) * 64;  // 16 NBLK: mu_x, zero beyond D
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = blockIdx.y;
  const int ar = lane & 15, ak = lane >> 4;
  const int D = dm.D, kp4 = ml_kp(D) / 4;      // 4 (NBLK - 1) < kp4 <= 4 NBLK
  const double *mod = model + (size_t)m * ml_model_stride(D);
  const double *mZ = mod, *mux = mod + 2 * D * D;
  const double cst = mod[2 * D * D + 3 * D];
  kwy_tri_fill<NBLK, 64 * NW>(zf, D, tid, [&](int j, int i) { return mZ[j * D + i]; });
  for (int c = tid; c < 16 * NBLK; c += 64 * NW) mus[c] = c < D ? mux[c] : 0.0;
  __syncthreads();
  const int64_t ntiles = (dm.T + TILE - 1) / TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // (no barrier in this loop)
    const int64_t t0 = tile * TILE + 32 * wv;
    if (t0 >= dm.T) break;
    // rows behind the last frame repeat it (their results are not stored); columns beyond D are zero
    const double *xa = X + min(t0 + ar, dm.T - 1) * D, *xb = X + min(t0 + 16 + ar, dm.T - 1) * D;
    double a0[KS], a1[KS];
#pragma unroll
    for (int ks = 0; ks < KS - 4; ++ks) {
      const double mu = mus[4 * ks + ak];
      a0[ks] = xa[4 * ks + ak] - mu;
      a1[ks] = xb[4 * ks + ak] - mu;
    }
#pragma unroll
    for (int ks = KS - 4; ks < KS; ++ks) {
      const int c = 4 * ks + ak, cc = min(c, D - 1);
      const double mu = mus[cc];
      const double v0 = xa[cc] - mu, v1 = xb[cc] - mu;
      a0[ks] = c < D ? v0 : 0.0;
      a1[ks] = c < D ? v1 : 0.0;
    }
    double q0[4] = {0.0, 0.0, 0.0, 0.0}, q1[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int nb = 0; nb < NBLK; ++nb) {
      kwy_v4f64 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
      const double *frag = zf + (2 * nb * (nb + 1)) * 64 + lane;
#pragma unroll
      for (int ks = 0; ks < 4 * nb + 4; ++ks) {
        // only the last block can end before its diagonal (Kp/4 k-steps), and never before its first k-step
        if (nb < NBLK - 1 || ks <= 4 * (NBLK - 1) || ks < kp4) {
          const double b = frag[ks * 64];
          acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[ks], b, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[ks], b, acc1, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        q0[r] += acc0[r] * acc0[r];
        q1[r] += acc1[r] * acc1[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) kwy_row_sum15(q0[r], q1[r]);
    if (ar == 15) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t t = t0 + ak + 4 * r;
        if (t < dm.T) logp[t * dm.M + m] = cst - 0.5 * q0[r];
        if (t + 16 < dm.T) logp[(t + 16) * dm.M + m] = cst - 0.5 * q1[r];
      }
    }
  }
}

// ---- arg-max mixture, conditional mean / variance --------------------------------------------
// A wavefront takes ML_COND_F consecutive frames, a workgroup ML_COND_W wavefronts.  The arg-max is the lowest index
// among equal maxima (what a serial `lp > best` walk from -inf returns; a frame without any lp > -inf gets mixture 0).
// Lane i then forms output i as muy[i] + sum_k AT[k][i] (x - mux)[k], k ascending: a load instruction reads one row
// of AT, consecutive doubles, where a row-major A puts every lane on a cache line of its own.  The kernel is bound by
// the D x D doubles of A that a frame pulls through L2 (41 KB at D = 72), so where the frames of a wavefront agree on
// the mixture -- neighbouring frames of speech mostly do -- one load of AT serves all of them; the sums of a frame are
// the same operations in the same order either way.
#define ML_COND_F 4
#define ML_COND_W 4
__global__ __launch_bounds__(64 * ML_COND_W) void k_gmm_cond(const double *__restrict__ X, ml_dims dm,
                                                            const double *__restrict__ model,
                                                            const double *__restrict__ logp,
                                                            double *__restrict__ E, double *__restrict__ Dv,
                                                            int *__restrict__ mix) {
  __shared__ double dsh_all[ML_COND_W][ML_COND_F][192];     // (x - mux) of every frame: D <= 192
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, D = dm.D;
  const int64_t tb = ((int64_t)blockIdx.x * ML_COND_W + wv) * ML_COND_F;
  double (*dsh)[192] = dsh_all[wv];
  const int none = 0x7fffffff;
  int bms[ML_COND_F];
#pragma unroll
  for (int f = 0; f < ML_COND_F; ++f) {
    const int64_t t = min(tb + f, dm.T - 1);      // frames behind the last one repeat it and store nothing
    int bm = none;
    double best = -INFINITY;
    for (int m = lane; m < dm.M; m += 64) {
      const double lp = logp[t * dm.M + m];
      if (lp > best) { best = lp; bm = m; }
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const double ob = __shfl_xor(best, s);
      const int om = __shfl_xor(bm, s);
      if (ob > best || (ob == best && om < bm)) { best = ob; bm = om; }
    }
    if (bm == none) bm = 0;
    bm = __builtin_amdgcn_readfirstlane(bm);
    bms[f] = bm;
    const double *mux = model + (size_t)bm * ml_model_stride(D) + 2 * D * D;
    for (int i = lane; i < D; i += 64) dsh[f][i] = X[t * D + i] - mux[i];
    if (lane == 0 && tb + f < dm.T) mix[t] = bm;
  }
  __syncthreads();
  bool same = true;                      // (wave-uniform: the mixtures sit in scalar registers)
#pragma unroll
  for (int f = 1; f < ML_COND_F; ++f) same = same && bms[f] == bms[0];
  if (same) {
    const double *mod = model + (size_t)bms[0] * ml_model_stride(D);
    const double *muy = mod + 2 * D * D + D, *dvar = muy + D, *AT = mod + ml_model_at(D);
    for (int i = lane; i < D; i += 64) {
      double v[ML_COND_F];
#pragma unroll
      for (int f = 0; f < ML_COND_F; ++f) v[f] = muy[i];
      const double *at = AT + i;
#pragma unroll 4
      for (int k = 0; k < D; ++k) {
        const double a = at[(size_t)k * D];
#pragma unroll
        for (int f = 0; f < ML_COND_F; ++f) v[f] += a * dsh[f][k];
      }
      const double dv = dvar[i];
#pragma unroll
      for (int f = 0; f < ML_COND_F; ++f)
        if (tb + f < dm.T) { E[(tb + f) * D + i] = v[f]; Dv[(tb + f) * D + i] = dv; }
    }
  } else {
    for (int f = 0; f < ML_COND_F; ++f) {
      if (tb + f >= dm.T) break;
      const double *mod = model + (size_t)bms[f] * ml_model_stride(D);
      const double *muy = mod + 2 * D * D + D, *dvar = muy + D, *AT = mod + ml_model_at(D);
      for (int i = lane; i < D; i += 64) {
        double v = muy[i];
        const double *at = AT + i;
#pragma unroll 8
        for (int k = 0; k < D; ++k) v += at[(size_t)k * D] * dsh[f][k];
        E[(tb + f) * D + i] = v;
        Dv[(tb + f) * D + i] = dvar[i];
      }
    }
  }
}

// ---- frame-wise conversion (MLPG switched off): posterior-weighted conditional mean ------------------------
// nnmnkwii MLPGBase.transform, what GMMFeatureConverter.convert(mlpg=False) runs (kwiiyatta/converter/gmm.py:28-34
// with windows[0:1]): y_t = sum_m p(m | x_t) (mu_y,m + A_m (x_t - mu_x,m)), the posterior being the softmax of the
// weighted log-densities (sklearn predict_proba).  One workgroup per frame.
__global__ __launch_bounds__(128) void k_gmm_soft(const double *__restrict__ X, ml_dims dm,
                                                 const double *__restrict__ model,
                                                 const double *__restrict__ logp, double *__restrict__ Y) {
  __shared__ double post[256];
  __shared__ double xs[192];
  __shared__ double red[4];
  const int64_t t = blockIdx.x;
  const int tid = threadIdx.x, D = dm.D, M = dm.M;
  double mx = -INFINITY;
  for (int m = tid; m < M; m += 128) mx = fmax(mx, logp[t * M + m]);
  mx = kwy_wave_max_f64(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  for (int i = tid; i < D; i += 128) xs[i] = X[t * D + i];
  __syncthreads();
  mx = fmax(red[0], red[1]);
  double se = 0.0;
  for (int m = tid; m < M; m += 128) { const double e = exp(logp[t * M + m] - mx); post[m] = e; se += e; }
  se = kwy_wave_sum(se);
  __syncthreads();
  if ((tid & 63) == 0) red[2 + (tid >> 6)] = se;
  __syncthreads();
  const double inv = 1.0 / (red[2] + red[3]);
  for (int i = tid; i < D; i += 128) {
    double y = 0.0;
    for (int m = 0; m < M; ++m) {
      const double pm = post[m] * inv;
      if (pm == 0.0) continue;
      const double *mod = model + (size_t)m * ml_model_stride(D);
      const double *ar = mod + D * D + (size_t)i * D, *mux = mod + 2 * D * D, *muy = mux + D;
      double v = muy[i];
      for (int k = 0; k < D; ++k) v += ar[k] * (xs[k] - mux[k]);
      y += pm * v;
    }
    Y[t * D + i] = y;
  }
}

// ---- MLPG: normal equations ---------------------------------------------------------------------
// rec[t][c][0..3] = P[t][t], P[t][t-1], P[t][t-2], rhs[t]: one 32-byte record per (row, dimension), so that the
// solver moves it with two 16-byte accesses per lane (its sweeps are bound by the vector-memory instruction rate of
// the one CU they run on)
__device__ __forceinline__ double ml_wcoef(int w, int k) {  // window w at offset k in [-1, 1]
  if (w == 0) return k == 0 ? 1.0 : 0.0;
  if (w == 1) return k == -1 ? -0.5 : (k == 0 ? 0.0 : 0.5);
  return k == 0 ? -2.0 : 1.0;
}

__global__ void k_mlpg_build(const double *__restrict__ E, const double *__restrict__ Dv, ml_batch bt, ml_dims dm,
                             double *__restrict__ rec) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= dm.T * dm.d) return;
  const int64_t ag = e / dm.d;
  const int c = (int)(e % dm.d);
  const int u = bt.find(ag);
  const int64_t t0 = bt.start[u], a = ag - t0, T = bt.start[u + 1] - t0;    // row a of utterance u's system
  E += t0 * dm.D;
  Dv += t0 * dm.D;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0, b = 0.0;
  for (int w = 0; w < 3; ++w) {
    const int l = w == 0 ? 0 : 1;
    for (int64_t t = a - l; t <= a + l; ++t) {  // frames whose window touches row a (ascending t)
      if (t < 0 || t >= T) continue;
      const int k1 = (int)(a - t);
      const double prec = 1 / Dv[t * dm.D + w * dm.d + c];
      const double bm = prec * E[t * dm.D + w * dm.d + c];
      const double ca = ml_wcoef(w, k1);
      b += ca * bm;
      for (int k2 = -l; k2 <= k1; ++k2) {
        const int64_t cc = t + k2;
        if (cc < 0 || cc >= T) continue;
        const double v = ca * prec * ml_wcoef(w, k2);
        const int off = (int)(a - cc);
        if (off == 0) p0 += v; else if (off == 1) p1 += v; else p2 += v;
      }
    }
  }
  double2 *o = (double2 *)rec + e * 2;
  o[0] = make_double2(p0, p1);
  o[1] = make_double2(p2, b);
}

// ---- MLPG: the T x T pentadiagonal SPD systems (one per static dimension), partitioned --------------------
// Round 1 walked the T rows serially, one lane per dimension: 2 x 2201 dependent steps of ~170 ns (0.76 ms, the
// longest kernel on the latency path of a pair).  Now the rows are cut into P chunks with a separator of two rows
// between neighbours (bandwidth 2: removing two rows decouples the chunks), and the elimination runs in
// nested-dissection order:
//   1. every (chunk, dimension) lane -- 64/d chunks per wavefront -- factors its chunk (banded Cholesky) and solves
//      it for five right-hand sides: the chunk's part of b, and the two columns that couple it to the separator
//      above and below.  The reciprocal square root on the serial chain is v_rsq_f64 + two Newton steps instead of
//      an IEEE square root and division (chain of ~9 instead of ~25 dependent operations per row).
//   2. one lane per dimension assembles the Schur complement on the 2 (P-1) separator unknowns from the chunks'
//      first and last two solution rows (it is SPD, block tridiagonal with 2 x 2 blocks = bandwidth 3) and solves it.
//   3. all threads: x = g - Y_top x_sep_above - Y_bottom x_sep_below, written straight to the (strided) output.
// Same arithmetic as a Cholesky solve in another elimination order: differences to the serial CPU order are rounding
// (tests: <= 1e-10 relative).  Rows stream from and to global memory as 32-byte records (two 16-byte accesses per
// lane) through register double buffers.
// Two launches: k_mlpg_chunks does step 1 with ONE wavefront per workgroup (ML_CHUNK_WGS of them at most), so the
// chunks spread over that many CUs -- as a single workgroup the sweeps were bound by one CU's memory concurrency
// (8.9 MB written by other XCDs just before, every line over the fabric: ~30 B/clk, 0.13 ms of a 0.18 ms kernel);
// k_mlpg_finish does steps 2 and 3 on a small grid, every workgroup solving the (tiny) separator system for itself
// and recovering its share of the rows.
#define ML_CHUNK_WGS 16
#define ML_MAX_CHUNKS 64      // bounds the serial separator solve (2 (P-1) rows of bandwidth 3 per dimension)
#define ML_FIN_NT 256
#define ML_FIN_WGS 8
#define ML_U 8    // rows per register buffer, forward sweep (4 values per row)
#define ML_UB 4   // backward sweep (6 values per row, 10 running values)
#define ML_G 16   // the unguarded middle section is a multiple of this many rows (2 ML_U, 4 ML_UB)
#define ML_BD 24   // doubles kept per (chunk, dimension) for step 2 (global scratch bnd[P][d][ML_BD])

__device__ __forceinline__ double ml_rsqrt(double v) {
  double r = __builtin_amdgcn_rsq(v);
  double e = fma(-v * r, r, 1.0);
  r = fma(0.5 * r, e, r);
  e = fma(-v * r, r, 1.0);
  r = fma(0.5 * r, e, r);
  return r;
}

__device__ __forceinline__ int ml_chunk_rows(const ml_part &q, int j) { return q.base + (j < q.extra ? 1 : 0); }
__device__ __forceinline__ int64_t ml_chunk_start(const ml_part &q, int j) {
  return (int64_t)j * q.base + (j < q.extra ? j : q.extra) + 2 * j;
}

__global__ __launch_bounds__(64) void k_mlpg_chunks(double *__restrict__ rec, double *__restrict__ zz,
                                                    double *__restrict__ Y, double *__restrict__ bnd, ml_dims dm,
                                                    ml_batch bt, int *__restrict__ status, long long *__restrict__ dbg) {
  // utterance blockIdx.y: its rows start at start[u] in the batch's arrays; its boundary records have their own block
  const ml_part pt = bt.u[blockIdx.y].pt;
  {
    const int64_t r0 = bt.start[blockIdx.y] * dm.d;
    rec += r0 * 4; zz += r0 * 2; Y += r0 * 4;
    bnd += (size_t)blockIdx.y * ML_CHUNK_WGS * 64 * ML_BD;
  }
  const int lane = threadIdx.x, d = dm.d, P = pt.P;
#define ML_STAMP(n) do { if (dbg && lane == 0 && blockIdx.x == 0) dbg[n] = clock64(); } while (0)
  ML_STAMP(0);
  const int cpw = 64 / d;
  const int slot = lane / d, c = lane - slot * d;
  const int j = blockIdx.x * cpw + slot;
  if (slot < cpw && j < P) {
    const int nj = ml_chunk_rows(pt, j);
    const int64_t st = ml_chunk_start(pt, j);
    const bool has_top = j > 0, has_bot = j < P - 1;
    // row i of this lane: records rq[i * 2 d] = {1/diag | P0, L1 | P1}, rq[i * 2 d + 1] = {L2 | P2, z or y of b | b};
    // zq[i * d] = z of the two top columns; yq[i * 2 d], yq[i * 2 d + 1] = y of the top and the bottom columns
    double2 *rq = (double2 *)rec + (st * d + c) * 2;
    double2 *zq = (double2 *)zz + st * d + c;
    double2 *yq = (double2 *)Y + (st * d + c) * 2;
    const int s2 = d * 2;
    // ---------------- forward: L L' = A_jj, z = L^-1 [b, top columns]; stored per row: 1/L[t][t], L[t][t-1], L[t][t-2]
    // Rows 0, 1 (which carry the top columns' right-hand sides) and the last rows (at least two: the bottom columns
    // start there) go through a guarded path; the rows between -- the same count, a multiple of ML_G, in every lane --
    // run without any divergent branch, two register buffers taking turns: while one is consumed the other one's
    // loads are in flight.  (With guards in that loop the compiler's wait counts degrade to "everything issued".)
    const int nmain = pt.base > 4 ? ((pt.base - 4) / ML_G) * ML_G : 0;      // rows [2, 2 + nmain)
    double r1 = 0, r2 = 0, l11 = 0;
    double zg1 = 0, zg2 = 0, za1 = 0, za2 = 0, zb1 = 0, zb2 = 0;
    double p2f = 0, p1f = 0, p2f1 = 0;
    bool bad = false;
    auto fwd_row = [&](int i, double p0, double p1, double p2, double b, double ra, double rb) {
      const double L2 = p2 * r2;
      const double L1 = (p1 - L2 * l11) * r1;
      double v = p0 - L2 * L2;
      v -= L1 * L1;
      if (!(v > 0.0)) { bad = true; v = 1.0; }
      const double r0 = ml_rsqrt(v);
      const double zg = ((b - L1 * zg1) - L2 * zg2) * r0;
      const double za = ((ra - L1 * za1) - L2 * za2) * r0;
      const double zb = ((rb - L1 * zb1) - L2 * zb2) * r0;
      rq[i * s2] = make_double2(r0, L1);
      rq[i * s2 + 1] = make_double2(L2, zg);
      zq[i * d] = make_double2(za, zb);
      r2 = r1; r1 = r0; l11 = L1;
      zg2 = zg1; zg1 = zg; za2 = za1; za1 = za; zb2 = zb1; zb1 = zb;
    };
    auto fwd_guarded = [&](int lo, int hi) {      // rows [lo, hi), a few at a time, not pipelined
      for (int i0 = lo; i0 < hi; i0 += ML_U) {
        double2 A[ML_U], B[ML_U];
#pragma unroll
        for (int u = 0; u < ML_U; ++u) {
          const int i = i0 + u < hi ? i0 + u : hi - 1;
          A[u] = rq[i * s2]; B[u] = rq[i * s2 + 1];
        }
#pragma unroll
        for (int u = 0; u < ML_U; ++u) {
          const int i = i0 + u;
          if (i < hi) {
            double ra = 0.0, rb = 0.0;       // the columns of the separator above: x[u], x[u+1]
            if (i == 0) { p2f = B[u].x; p1f = A[u].y; if (has_top) { ra = B[u].x; rb = A[u].y; } }
            if (i == 1) { p2f1 = B[u].x; if (has_top) rb = B[u].x; }
            fwd_row(i, A[u].x, A[u].y, B[u].x, B[u].y, ra, rb);
          }
        }
      }
    };
    auto fwd_load = [&](double2 (&A)[ML_U], double2 (&B)[ML_U], int i0, int last) {   // rows clamped to <= last
#pragma unroll
      for (int u = 0; u < ML_U; ++u) {
        const int i = i0 + u < last ? i0 + u : last;
        A[u] = rq[i * s2]; B[u] = rq[i * s2 + 1];
      }
    };
    auto fwd_rows = [&](const double2 (&A)[ML_U], const double2 (&B)[ML_U], int i0) {
#pragma unroll
      for (int u = 0; u < ML_U; ++u) fwd_row(i0 + u, A[u].x, A[u].y, B[u].x, B[u].y, 0.0, 0.0);
    };
    fwd_guarded(0, nj < 2 ? nj : 2);
    if (nmain > 0) {
      double2 A0[ML_U], B0[ML_U], A1[ML_U], B1[ML_U];
      const int last = 1 + nmain;
      fwd_load(A0, B0, 2, last);
      for (int i0 = 2; i0 < 2 + nmain; i0 += 2 * ML_U) {
        fwd_load(A1, B1, i0 + ML_U, last);
        fwd_rows(A0, B0, i0);
        fwd_load(A0, B0, i0 + 2 * ML_U, last);
        fwd_rows(A1, B1, i0 + ML_U);
      }
    }
    fwd_guarded(2 + nmain, nj);
    if (bad) atomicExch(status, 2);
    ML_STAMP(1);
    // the columns of the separator below are zero until the last two rows of the chunk
    double zc0 = 0, zc1 = 0, zd1 = 0;     // z of column x[s] at rows n-2, n-1; of column x[s+1] at row n-1
    if (has_bot) {
      const double *sq = rec + ((st + nj) * d + c) * 4;
      const double p1s = sq[1], p2s = sq[2], p2s1 = sq[4 * d + 2];
      zc0 = p2s * r2;
      zc1 = (p1s - l11 * zc0) * r1;
      zd1 = p2s1 * r1;
    }
    // ---------------- backward: y = L^-T z, five columns; the same three sections in reverse
    double *bo = bnd + ((size_t)j * d + c) * ML_BD;
    bo[20] = p2f; bo[21] = p1f; bo[22] = p2f1;
    double n11 = 0, n22 = 0, n12 = 0;
    double yg1 = 0, yg2 = 0, ya1 = 0, ya2 = 0, yb1 = 0, yb2 = 0, yc1 = 0, yc2 = 0, yd1 = 0, yd2 = 0;
    double yg, ya, yb, yc, yd;
    auto bwd_row = [&](int i, double2 A, double2 B, double2 Z, double zc, double zd) {
      const double r0 = A.x;
      yg = ((B.y - n11 * yg1) - n22 * yg2) * r0;
      ya = ((Z.x - n11 * ya1) - n22 * ya2) * r0;
      yb = ((Z.y - n11 * yb1) - n22 * yb2) * r0;
      yc = ((zc - n11 * yc1) - n22 * yc2) * r0;
      yd = ((zd - n11 * yd1) - n22 * yd2) * r0;
      ((double *)(rq + i * s2 + 1))[1] = yg;
      yq[i * s2] = make_double2(ya, yb);
      yq[i * s2 + 1] = make_double2(yc, yd);
      n22 = n12; n11 = A.y; n12 = B.x;
      yg2 = yg1; yg1 = yg; ya2 = ya1; ya1 = ya; yb2 = yb1; yb1 = yb; yc2 = yc1; yc1 = yc; yd2 = yd1; yd1 = yd;
    };
    auto bwd_guarded = [&](int lo, int hi) {      // rows hi-1 down to lo
      for (int i0 = hi - 1; i0 >= lo; i0 -= ML_UB) {
        double2 A[ML_UB], B[ML_UB], Z[ML_UB];
#pragma unroll
        for (int u = 0; u < ML_UB; ++u) {
          const int i = i0 - u >= lo ? i0 - u : lo;
          A[u] = rq[i * s2]; B[u] = rq[i * s2 + 1]; Z[u] = zq[i * d];
        }
#pragma unroll
        for (int u = 0; u < ML_UB; ++u) {
          const int i = i0 - u;
          if (i >= lo) {
            bwd_row(i, A[u], B[u], Z[u], i == nj - 1 ? zc1 : (i == nj - 2 ? zc0 : 0.0), i == nj - 1 ? zd1 : 0.0);
            if (i >= nj - 2) { double *o = bo + 15 - 5 * (nj - 1 - i); o[0] = yg; o[1] = ya; o[2] = yb; o[3] = yc; o[4] = yd; }
            if (i <= 1) { double *o = bo + 5 * i; o[0] = yg; o[1] = ya; o[2] = yb; o[3] = yc; o[4] = yd; }
          }
        }
      }
    };
    auto bwd_load = [&](double2 (&A)[ML_UB], double2 (&B)[ML_UB], double2 (&Z)[ML_UB], int i0) {   // rows i0, i0-1, ..., >= 2
#pragma unroll
      for (int u = 0; u < ML_UB; ++u) {
        const int i = i0 - u >= 2 ? i0 - u : 2;
        A[u] = rq[i * s2]; B[u] = rq[i * s2 + 1]; Z[u] = zq[i * d];
      }
    };
    auto bwd_rows = [&](const double2 (&A)[ML_UB], const double2 (&B)[ML_UB], const double2 (&Z)[ML_UB], int i0) {
#pragma unroll
      for (int u = 0; u < ML_UB; ++u) bwd_row(i0 - u, A[u], B[u], Z[u], 0.0, 0.0);
    };
    bwd_guarded(2 + nmain, nj);
    if (nmain > 0) {
      double2 A0[ML_UB], B0[ML_UB], Z0[ML_UB], A1[ML_UB], B1[ML_UB], Z1[ML_UB];
      bwd_load(A0, B0, Z0, 1 + nmain);
      for (int i0 = 1 + nmain; i0 >= 2; i0 -= 2 * ML_UB) {
        bwd_load(A1, B1, Z1, i0 - ML_UB);
        bwd_rows(A0, B0, Z0, i0);
        bwd_load(A0, B0, Z0, i0 - 2 * ML_UB);
        bwd_rows(A1, B1, Z1, i0 - ML_UB);
      }
    }
    bwd_guarded(0, nj < 2 ? nj : 2);
  }
  ML_STAMP(2);
#undef ML_STAMP
}

__global__ __launch_bounds__(ML_FIN_NT) void k_mlpg_finish(const double *__restrict__ rec, const double *__restrict__ Y,
                                                          const double *__restrict__ bnd, ml_dims dm, ml_batch bt,
                                                          int *__restrict__ status, long long *__restrict__ dbg) {
  extern __shared__ double sm[];
  const ml_part pt = bt.u[blockIdx.y].pt;
  double *__restrict__ y = bt.u[blockIdx.y].y;
  const int ldy = bt.ldy;
  {
    const int64_t r0 = bt.start[blockIdx.y] * dm.d;
    rec += r0 * 4; Y += r0 * 4;
    bnd += (size_t)blockIdx.y * ML_CHUNK_WGS * 64 * ML_BD;
  }
  const int tid = threadIdx.x, d = dm.d, P = pt.P;
#define ML_STAMP(n) do { if (dbg && tid == 0 && blockIdx.x == 0) dbg[n] = clock64(); } while (0)
  ML_STAMP(3);
  const int64_t T = bt.start[blockIdx.y + 1] - bt.start[blockIdx.y];
  const int m = 2 * (P - 1);
  double *red = sm;                    // [d][m][5]: lower band (diag, 3 sub-diagonals) and right-hand side

  // ---------------- the separators: Schur complement (bandwidth 3) on 2 (P-1) unknowns per dimension
  // assembly: one thread per (separator, dimension); R[r][q] = S[r][r-q], R[r][4] = right-hand side
  for (int e = tid; e < (P - 1) * d; e += ML_FIN_NT) {
    const int k = e / d, cc = e - k * d;
    const int na = ml_chunk_rows(pt, k);
    const int64_t s = ml_chunk_start(pt, k) + na;
    const double *A = bnd + ((size_t)k * d + cc) * ML_BD, *B = bnd + ((size_t)(k + 1) * d + cc) * ML_BD;
    const double *q0 = rec + (s * d + cc) * 4, *q1 = q0 + d * 4;   // separator rows: untouched by the chunks
    const double p0s = q0[0], p1s = q0[1], p2s = q0[2], p0s1 = q1[0], p1s1 = q1[1], p2s1 = q1[2];
    // cb(col) = C_bottom' (column of the chunk above); ct(col) = C_top' (column of the chunk below);
    // at(col) = C_top' of the chunk above applied to its own columns: the coupling to the previous separator
    auto cb0 = [&](int col) { return p2s * A[10 + col] + p1s * A[15 + col]; };
    auto cb1 = [&](int col) { return p2s1 * A[15 + col]; };
    auto ct0 = [&](int col) { return B[20] * B[col]; };
    auto ct1 = [&](int col) { return B[21] * B[col] + B[22] * B[5 + col]; };
    auto at0 = [&](int col) { return A[20] * A[col]; };
    auto at1 = [&](int col) { return A[21] * A[col] + A[22] * A[5 + col]; };
    double *R0 = red + ((size_t)cc * m + 2 * k) * 5, *R1 = R0 + 5;
    R0[0] = (p0s - cb0(3)) - ct0(1);
    R0[1] = k > 0 ? -at1(3) : 0.0;
    R0[2] = k > 0 ? -at0(3) : 0.0;
    R0[3] = 0.0;
    R0[4] = (q0[3] - cb0(0)) - ct0(0);
    R1[0] = (p0s1 - cb1(4)) - ct1(2);
    R1[1] = (p1s1 - cb1(3)) - ct1(1);
    R1[2] = k > 0 ? -at1(4) : 0.0;
    R1[3] = k > 0 ? -at0(4) : 0.0;
    R1[4] = (q1[3] - cb1(0)) - ct1(0);
  }
  __syncthreads();
  // banded Cholesky and the two sweeps, one lane per dimension; the last three rows stay in registers.
  // In place: R[r][0] = 1 / L[r][r], R[r][q] = L[r][r-q], R[r][4] = solution.
  if (m > 0 && tid < d) {
    double *R = red + (size_t)tid * m * 5;
    double ri1 = 0, ri2 = 0, ri3 = 0, a1 = 0, a2 = 0, b1 = 0, z1 = 0, z2 = 0, z3 = 0;   // a: row r-1, b: row r-2
    for (int r = 0; r < m; ++r) {
      double *Rr = R + (size_t)r * 5;
      const double s0 = Rr[0], s1 = Rr[1], s2 = Rr[2], s3 = Rr[3], bb = Rr[4];
      const double l3 = s3 * ri3;
      const double l2 = (s2 - l3 * b1) * ri2;
      const double l1 = ((s1 - l3 * a2) - l2 * a1) * ri1;
      double dd = ((s0 - l3 * l3) - l2 * l2) - l1 * l1;
      if (!(dd > 0.0)) { atomicExch(status, 2); dd = 1.0; }
      const double ri = ml_rsqrt(dd);
      const double z = (((bb - l1 * z1) - l2 * z2) - l3 * z3) * ri;
      Rr[0] = ri; Rr[1] = l1; Rr[2] = l2; Rr[3] = l3; Rr[4] = z;
      ri3 = ri2; ri2 = ri1; ri1 = ri;
      b1 = a1; a1 = l1; a2 = l2;
      z3 = z2; z2 = z1; z1 = z;
    }
    double x1 = 0, x2 = 0, x3 = 0, u1 = 0, v2 = 0, w3 = 0, v1n = 0, w1n = 0, w2n = 0;
    // u1 = L[r+1][r], v2 = L[r+2][r], w3 = L[r+3][r]
    for (int r = m - 1; r >= 0; --r) {
      double *Rr = R + (size_t)r * 5;
      const double x = (((Rr[4] - u1 * x1) - v2 * x2) - w3 * x3) * Rr[0];
      Rr[4] = x;
      // row r's sub-diagonals become: L[r][r-1] -> u1 of row r-1; L[r][r-2] -> v2 of row r-2; L[r][r-3] -> w3 of row r-3
      w3 = w2n; w2n = w1n; w1n = Rr[3];
      v2 = v1n; v1n = Rr[2];
      u1 = Rr[1];
      x3 = x2; x2 = x1; x1 = x;
    }
  }
  __syncthreads();
  ML_STAMP(4);

  // ---------------- every row: x = g - Y_top x_above - Y_bottom x_below; separator rows take the reduced solution.
  // Four elements per thread and pass, all loads issued before the first use; the multipliers of a missing
  // separator are the zero columns computed above, so the index is merely clamped.
  const int big = pt.base + 3, small_ = pt.base + 2;
  const int total = (int)(T * d);
  const int share = (total + gridDim.x - 1) / gridDim.x;
  const int e_lo = blockIdx.x * share, e_hi = min(total, e_lo + share);
  if (P == 1) {
    for (int e = e_lo + tid; e < e_hi; e += ML_FIN_NT) { const int t = e / d; y[(int64_t)t * ldy + (e - t * d)] = rec[(size_t)e * 4 + 3]; }
  } else {
    for (int e0 = e_lo + tid; e0 < e_hi; e0 += 4 * ML_FIN_NT) {
      double g[4];
      double2 ya[4], yb[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = e0 + q * ML_FIN_NT < e_hi ? e0 + q * ML_FIN_NT : e_lo;
        g[q] = rec[(size_t)e * 4 + 3];
        ya[q] = ((const double2 *)Y)[(size_t)e * 2];
        yb[q] = ((const double2 *)Y)[(size_t)e * 2 + 1];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = e0 + q * ML_FIN_NT;
        if (e < e_hi) {
          const int t = e / d;
          const int cc = e - t * d;
          int jj, off, nrows;
          if (t < pt.extra * big) { jj = t / big; off = t - jj * big; nrows = pt.base + 1; }
          else {
            const int t2 = t - pt.extra * big;
            jj = pt.extra + t2 / small_;
            off = t2 - (jj - pt.extra) * small_;
            nrows = pt.base;
          }
          const double *R = red + (size_t)cc * m * 5;
          const int ka = jj > 0 ? jj - 1 : 0, kb = jj < P - 1 ? jj : P - 2;
          double v = ((g[q] - ya[q].x * R[(2 * ka) * 5 + 4]) - ya[q].y * R[(2 * ka + 1) * 5 + 4]);
          v = (v - yb[q].x * R[(2 * kb) * 5 + 4]) - yb[q].y * R[(2 * kb + 1) * 5 + 4];
          if (off >= nrows) v = R[(2 * jj + (off - nrows)) * 5 + 4];
          y[(int64_t)t * ldy + cc] = v;
        }
      }
    }
  }
  ML_STAMP(5);
#undef ML_STAMP
}

// ---- host side: launch geometry ---------------------------------------------------------------------------------------
#define ML_LDS_MAX (160 * 1024)   // bytes of LDS a workgroup can have

// k_gmm_prep keeps three D x D matrices in LDS: that bounds the feature dimension of every conversion entry (D <= 82),
// and with it the column blocks of the kernels that are templates over them
static constexpr size_t ml_prep_lds(int D) { return sizeof(double) * 3 * D * D; }
static constexpr bool ml_lds_fits(int D) { return ml_prep_lds(D) <= ML_LDS_MAX; }
static constexpr int ml_widest_d() {
  int D = 1;
  while (ml_lds_fits(D + 1)) ++D;
  return D;
}
static constexpr int ml_frag_blocks(int D) { return ml_np(D) / 16; }
static_assert(ml_frag_blocks(ml_widest_d()) <= ML_FRAG_MAXBLK, "a D that k_gmm_prep admits has no k_gmm_logp_frag instance");
static_assert(sizeof(double) * kwy_tri_lds_doubles(ML_FRAG_MAXBLK) <= ML_LDS_MAX, "k_gmm_logp_frag: fragments beyond the LDS");

// log-densities: eight wavefronts, 256 frames per tile; frame-tile walkers per mixture, not more than tiles
#define ML_FRAG_NW 8
#define ML_FRAG_WGS 1024  // workgroups of a launch: measured 0.341 / 0.306 / 0.296 ms with 256 / 512 / 1024 (D = 72, 35 216 frames)
static int ml_frag_splits(int64_t T, int M) {
  const int64_t ntiles = (T + 32 * ML_FRAG_NW - 1) / (32 * ML_FRAG_NW);
  int64_t s = (ML_FRAG_WGS + M - 1) / M;
  if (s > ntiles) s = ntiles;
  return (int)(s < 1 ? 1 : s);
}

// (the callers have checked ml_lds_fits(dm.D))
static int ml_launch_logp(kwy_ctx *ctx, const double *X, const ml_dims &dm, const double *model, double *logp) {
  return kwy_with_blocks<ML_FRAG_MAXBLK>(ml_frag_blocks(dm.D), [&](auto nb) -> int {
    constexpr int NBLK = decltype(nb)::value;
    const size_t lds = sizeof(double) * kwy_tri_lds_doubles(NBLK);
    const dim3 grid((unsigned)ml_frag_splits(dm.T, dm.M), dm.M);
    KWY_HIP(hipFuncSetAttribute((const void *)k_gmm_logp_frag<NBLK, ML_FRAG_NW>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    KWY_PROF(ctx, "k_gmm_logp", hipLaunchKernelGGL((k_gmm_logp_frag<NBLK, ML_FRAG_NW>), grid, dim3(64 * ML_FRAG_NW), lds,
                                                   ctx->stream, X, dm, model, logp));
    return KWY_OK;
  });
}

// chunks of the partitioned solve of a T-row system: 64/d per wavefront, at least 16 rows each
static ml_part ml_partition(int64_t T, int d) {
  ml_part pt;
  const int cpw = 64 / d;
  pt.P = ML_CHUNK_WGS * cpw;
  if (pt.P > ML_MAX_CHUNKS) pt.P = ML_MAX_CHUNKS;
  if ((int64_t)pt.P > T / 16) pt.P = (int)(T / 16);
  if (pt.P < 1) pt.P = 1;
  pt.base = (int)((T - 2 * (pt.P - 1)) / pt.P);
  pt.extra = (int)((T - 2 * (pt.P - 1)) % pt.P);
  return pt;
}

// ---- EM trajectory conversion over soft mixture posteriors (Toda et al. 2007, section IV) -----------------------
// The arithmetic is the contract of kwy_gmm_mlpg_em in include/kwy.h.  Instead of one arg-max mixture per frame every
// mixture weighs in with its posterior, and the posteriors are re-estimated from the source frame AND the trajectory
// of the previous solve (with its deltas) a fixed number of times.  Per iteration that takes all M conditional means of
// every frame: k_em_estep, the E-step, on the f64 MFMA.
//   k_em_prep    per mixture: 1 / v_m[c] and sum_c log(2 pi v_m[c]) (c ascending), once per call
//   k_em_estep   a workgroup owns 64 frames, a wavefront 16 of them, and walks the mixtures in ascending order.  AT_m goes
//                through registers into LDS in MFMA-fragment order (fragment (nb, ks) = the 64 lane values of the B
//                operand of column block nb and k-step ks; the loads of mixture m + 1 are in flight while m is
//                multiplied); E[m] = muy_m + A_m (x - mux_m) is accumulated from muy_m in ascending k, as k_gmm_cond
//                does, the column blocks' accumulators as independent chains under every k-step.  In the accumulator layout (col = lane & 15, row = (lane >> 4) + 4 reg) a lane holds, for four
//                frames and every column block, the trajectory's delta features, pbar and r; the quadratic term of a
//                frame is a butterfly sum over the 16 lanes of its row group (every lane ends with the same bits), and
//                the mixture is folded into pbar and r by an online softmax (running maximum, rescaling).  It stores
//                Ebar = r / pbar and Dbar = 1 / pbar, which k_mlpg_build takes as they are, and logsumexp_m per frame.
//   k_em_loglik  one workgroup per utterance: the sum of the frames' logsumexp in a fixed order
// A frame's results depend on its own row of X, its neighbours' trajectory rows inside its utterance and the model
// only: not on the tile it falls into, nor on what else is in the batch.
#define ML_EM_NW 4
#define ML_EM_TILE (16 * ML_EM_NW)
#define ML_EM_MAXBLK ML_FRAG_MAXBLK      // D <= 96: beyond what k_gmm_prep admits (D <= 82)

struct ml_em_out { double *loglik[KWY_BATCH_MAX]; };     // per utterance: em_iterations + 1 doubles, or null

__global__ void k_em_prep(const double *__restrict__ model, int D, int M, double *__restrict__ iv,
                          double *__restrict__ lc) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const double *dv = model + (size_t)m * ml_model_stride(D) + 2 * D * D + 2 * D;
  double s = 0.0;
  for (int c = 0; c < D; ++c) {
    iv[(size_t)m * D + c] = 1.0 / dv[c];
    s += log(2.0 * KWY_PI * dv[c]);
  }
  lc[m] = s;
}

template <int NBLK>
__global__ __launch_bounds__(64 * ML_EM_NW) void k_em_estep(const double *__restrict__ X, ml_dims dm, ml_batch bt,
                                                            const double *__restrict__ model,
                                                            const double *__restrict__ logp,
                                                            const double *__restrict__ iv, const double *__restrict__ lc,
                                                            int first, double *__restrict__ E, double *__restrict__ Dv,
                                                            double *__restrict__ lse) {
  constexpr int KS = 4 * NBLK, NP = 16 * NBLK, NFRAG = NBLK * KS, NT = 64 * ML_EM_NW;
  constexpr int PER = NFRAG * 64 / NT, PERV = (3 * NP + NT - 1) / NT;
  extern __shared__ double smem[];
  double *af = smem;                // NFRAG x 64: AT_m in fragment order (beyond D: copies of row / column D - 1)
  double *vec = af + NFRAG * 64;    // mux_m | muy_m | 1 / v_m, NP each, zero beyond D
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ar = lane & 15, ak = lane >> 4;
  const int D = dm.D, M = dm.M, kp4 = ml_kp(D) / 4;      // 4 (NBLK - 1) < kp4 <= 4 NBLK
  const int64_t t0 = (int64_t)blockIdx.x * ML_EM_TILE + 16 * wv;
  // rows behind the last frame repeat it and store nothing (a wavefront without frames still keeps the barriers)
  const double *xrow = X + min(t0 + ar, dm.T - 1) * D;
  double xa[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int c = 4 * ks + ak;
    const double v = xrow[min(c, D - 1)];
    xa[ks] = c < D ? v : 0.0;
  }
  int64_t tc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) tc[r] = min(t0 + ak + 4 * r, dm.T - 1);
  // delta features of the current trajectory at [frame (lane >> 4) + 4 r][column 16 nb + (lane & 15)]
  double Yd[NBLK][4];
#pragma unroll
  for (int nb = 0; nb < NBLK; ++nb)
#pragma unroll
    for (int r = 0; r < 4; ++r) Yd[nb][r] = 0.0;
  if (!first) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int u = bt.find(tc[r]);
      const int64_t t = tc[r] - bt.start[u], Tu = bt.start[u + 1] - bt.start[u];
      const double *y = bt.u[u].y + t * bt.ldy;
#pragma unroll
      for (int nb = 0; nb < NBLK; ++nb) {
        const int col = 16 * nb + ar;
        if (col < D) {
          const int w = col / dm.d, c = col - w * dm.d;
          const double y0 = y[c];
          const double ym = t > 0 ? y[c - bt.ldy] : 0.0;
          const double yp = t + 1 < Tu ? y[c + bt.ldy] : 0.0;
          Yd[nb][r] = w == 0 ? y0 : (w == 1 ? 0.5 * (yp - ym) : (yp - 2.0 * y0) + ym);
        }
      }
    }
  }
  double pb[NBLK][4], ra[NBLK][4], mx[4], sm[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mx[r] = -INFINITY;
    sm[r] = 0.0;
#pragma unroll
    for (int nb = 0; nb < NBLK; ++nb) { pb[nb][r] = 0.0; ra[nb][r] = 0.0; }
  }
  double pre[PER], prv[PERV];
  auto fetch = [&](int m) {
    const double *mod = model + (size_t)m * ml_model_stride(D);
    const double *AT = mod + ml_model_at(D), *mux = mod + 2 * D * D, *muy = mux + D, *ivm = iv + (size_t)m * D;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int idx = tid + i * NT, f = idx >> 6, l = idx & 63;
      const int nb = f / KS, ks = f - nb * KS;
      const int col = 16 * nb + (l & 15), k = 4 * ks + (l >> 4);
      // no zero padding needed (and no select next to the load: the compiler turns one into a branch around the load
      // with a wait inside, 25 load latencies in a row per mixture): a row k >= D meets the A operand 0 - 0, and a
      // column >= D is weighed by the zero behind 1 / v_m and never stored; the clamped loads keep both finite
      pre[i] = AT[(size_t)min(k, D - 1) * D + min(col, D - 1)];
    }
#pragma unroll
    for (int i = 0; i < PERV; ++i) {
      const int j = tid + i * NT, which = j / NP, c = j - which * NP;
      const double *src = which == 0 ? mux : (which == 1 ? muy : ivm);
      prv[i] = src[min(c, D - 1)];       // (zeroed beyond D where it is stored: a mask there, not a select here)
    }
  };
  fetch(0);
  for (int m = 0; m < M; ++m) {
    __syncthreads();      // mixture m - 1 has been consumed
#pragma unroll
    for (int i = 0; i < PER; ++i) af[tid + i * NT] = pre[i];
#pragma unroll
    for (int i = 0; i < PERV; ++i) {
      const int j = tid + i * NT;
      const long long keep = -(long long)(j % NP < D);
      if (j < 3 * NP) vec[j] = __longlong_as_double(__double_as_longlong(prv[i]) & keep);
    }
    __syncthreads();
    if (m + 1 < M) fetch(m + 1);
    double lpm[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) lpm[r] = logp[tc[r] * M + m];
    const double lcm = lc[m];
    // NBLK independent accumulator chains (one per column block) under every k-step: a chain alone leaves the matrix
    // core waiting for its own result
    kwy_v4f64 acc[NBLK];
    double ivc[NBLK], q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int nb = 0; nb < NBLK; ++nb) {
      const double my = vec[NP + 16 * nb + ar];
      ivc[nb] = vec[2 * NP + 16 * nb + ar];
      acc[nb] = kwy_v4f64{my, my, my, my};
    }
    // the operands of k-step ks + 1 are read from LDS before the products of k-step ks are issued (one wavefront per
    // SIMD: nothing else hides the LDS latency in front of every product)
    double bc[NBLK], bn[NBLK], mc = vec[ak], mn = 0.0;
#pragma unroll
    for (int nb = 0; nb < NBLK; ++nb) { bc[nb] = af[nb * KS * 64 + lane]; bn[nb] = 0.0; }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + 1 < KS) {
        mn = vec[4 * (ks + 1) + ak];
#pragma unroll
        for (int nb = 0; nb < NBLK; ++nb) bn[nb] = af[(nb * KS + ks + 1) * 64 + lane];
      }
      __builtin_amdgcn_sched_barrier(0);
      if (ks <= KS - 4 || ks < kp4) {
        const double a = xa[ks] - mc;
#pragma unroll
        for (int nb = 0; nb < NBLK; ++nb)
          acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bc[nb], acc[nb], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      mc = mn;
#pragma unroll
      for (int nb = 0; nb < NBLK; ++nb) bc[nb] = bn[nb];
    }
#pragma unroll
    for (int nb = 0; nb < NBLK; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double dl = Yd[nb][r] - acc[nb][r];
        q[r] += (dl * dl) * ivc[nb];
      }
    if (!first) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {     // butterfly over the row group: commutative sums, the same bits in every lane
        double v = q[r];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 8);
        q[r] = v;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double l = first ? lpm[r] : lpm[r] - 0.5 * (lcm + q[r]);
      const double mn = fmax(mx[r], l);
      double sc = 1.0, w = 0.0;
      if (mn != -INFINITY) { sc = exp(mx[r] - mn); w = exp(l - mn); }
      sm[r] = sm[r] * sc + w;
      mx[r] = mn;
#pragma unroll
      for (int nb = 0; nb < NBLK; ++nb) {
        const double wi = w * ivc[nb];
        pb[nb][r] = pb[nb][r] * sc + wi;
        ra[nb][r] = ra[nb][r] * sc + wi * acc[nb][r];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t t = t0 + ak + 4 * r;
    if (t < dm.T) {
#pragma unroll
      for (int nb = 0; nb < NBLK; ++nb) {
        const int col = 16 * nb + ar;
        if (col < D) {
          E[t * D + col] = ra[nb][r] / pb[nb][r];
          Dv[t * D + col] = sm[r] / pb[nb][r];
        }
      }
      if (ar == 0) lse[t] = mx[r] + log(sm[r]);
    }
  }
}

__global__ __launch_bounds__(256) void k_em_loglik(const double *__restrict__ lse, ml_batch bt, ml_em_out out, int k) {
  __shared__ double red[256];
  const int u = blockIdx.x, tid = threadIdx.x;
  double *dst = out.loglik[u];
  if (!dst) return;
  const int64_t t0 = bt.start[u], t1 = bt.start[u + 1];
  double s = 0.0;
  for (int64_t t = t0 + tid; t < t1; t += 256) s += lse[t];
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) dst[k] = red[0];
}

// ---- host side: the conversion ----------------------------------------------------------------------------------------
static size_t ml_em_lds(int nblk) { return sizeof(double) * ((size_t)4 * nblk * nblk * 64 + 48 * nblk); }

// The mixture of a call: the joint mixture's parameters on the device, or a model made by kwy_gmm_prepare_dev (then
// weights / means / covs only stand in for it where the arguments are checked).
struct ml_mixture {
  const double *weights, *means, *covs;
  int diff;
  const double *prepared;
};
static ml_mixture ml_prepared(const double *model) { return ml_mixture{model, model, model, 0, model}; }

// The ascent of kwy_gvgen.hip behind a conversion (kwy_gmm_mlpg_gv, include/kwy.h): null means none.  The band records
// are copied after the build of the last solve, because k_mlpg_chunks consumes its own in place (and, with EM, the
// closing E-step overwrites E / Dv).
struct ml_gv_opts {
  const double *mean, *var;       // d values each
  double weight;
  int iterations, offset;
  int32_t *status;                // one word per utterance of the call on the device, or null
};
struct ml_opts {
  int em;                         // EM re-estimations of the posteriors; -1: one arg-max mixture per frame
  bool em_only;                   // set by the kwy_*_em entries: they have no arg-max form, so em = -1 is refused
  const ml_gv_opts *gv;
};
// one utterance: T x d static features and their trajectory (row strides: the call's), one more column copied through
// (k_delta; or null), em + 1 log-likelihoods and gv->iterations + 1 objective values on the device (or null)
struct ml_job {
  const double *x;
  double *y;
  const double *keep_in;
  double *keep_out;
  int64_t T;
  double *loglik, *objective;
};

static int ml_check(kwy_ctx *ctx, const ml_job &q, int d, int M, const ml_mixture &gm, const ml_opts &o) {
  if (!ctx) return KWY_EINVAL;
  if (!q.x || !gm.weights || !gm.means || !gm.covs || !q.y || q.T <= 0 || d <= 0 || d > 64 || M <= 0) {
    ctx->err = "gmm_mlpg: bad argument";
    return KWY_EINVAL;
  }
  // (the GV entries take em = -1 as "arg-max"; to the EM entries it is an iteration count out of range)
  if (o.em_only || o.em != -1) {
    if (o.em < 0 || o.em > KWY_MLPG_EM_MAX) {
      ctx->err = "gmm_mlpg_em: em_iterations outside [0, KWY_MLPG_EM_MAX]";
      return KWY_EINVAL;
    }
    // what kwy_gmm_prepare_dev refuses (three D x D matrices in LDS) cannot arrive here as a prepared model either
    if (sizeof(double) * 3 * (3 * d) * (3 * d) > ML_LDS_MAX || ml_frag_blocks(3 * d) > ML_EM_MAXBLK) {
      ctx->err = "gmm_mlpg_em: feature dimension too large";
      return KWY_EINVAL;
    }
  }
  if (o.gv) {
    if (!o.gv->mean || !o.gv->var) { ctx->err = "gmm_mlpg_gv: bad argument"; return KWY_EINVAL; }
    if (!kwy_finite_pos(o.gv->weight)) {
      ctx->err = "gmm_mlpg_gv: weight must be positive and finite";
      return KWY_EINVAL;
    }
    if (o.gv->iterations < 0 || o.gv->iterations > KWY_MLPG_GV_MAX) {
      ctx->err = "gmm_mlpg_gv: gv_iterations outside [0, KWY_MLPG_GV_MAX]";
      return KWY_EINVAL;
    }
  }
  return KWY_OK;
}

// The arena buffers of a call are described once, by a function that names each pointer with its element count: walked
// with ctx == null it sums the bytes kwy_arena_begin is asked for, walked with the context it takes them, in that order.
struct ml_arena {
  kwy_ctx *ctx;
  size_t bytes = 0;
  bool ok = true;
  template <class T>
  void take(T *&p, size_t n) {
    bytes += kwy_pad(sizeof(T) * n);
    if (ctx && !(p = kwy_arena<T>(ctx, n))) ok = false;
  }
};

// the work buffers of one pass of the core over n utterances with T frames in all
struct ml_work {
  double *model, *X, *E, *Dv, *logp;
  int *mix;
  double *band, *rhs, *Ysp, *bnd;
  double *iv, *lc, *lse;
  int *status;
  double *band2;
};
static void ml_work_buffers(ml_arena &a, ml_work &w, int64_t T, int n, int d, int M, const ml_mixture &gm, const ml_opts &o) {
  const int D = 3 * d;
  if (gm.prepared) w.model = const_cast<double *>(gm.prepared);
  else a.take(w.model, ml_model_stride(D) * M);
  a.take(w.X, (size_t)T * D);
  a.take(w.E, (size_t)T * D);
  a.take(w.Dv, (size_t)T * D);
  a.take(w.logp, (size_t)T * M);
  if (o.em < 0) a.take(w.mix, T);
  a.take(w.band, (size_t)T * d * 4);   // records {P0, P1, P2, rhs}
  a.take(w.rhs, (size_t)T * d * 2);    // forward solutions of the two top columns
  a.take(w.Ysp, (size_t)T * d * 4);
  a.take(w.bnd, (size_t)n * ML_CHUNK_WGS * 64 * ML_BD);
  if (o.em >= 0) {
    a.take(w.iv, (size_t)M * D);
    a.take(w.lc, M);
    a.take(w.lse, T);
  }
  a.take(w.status, 16);
  if (o.gv) a.take(w.band2, (size_t)T * d * 4);
  else w.band2 = w.band;
}
// what a pass asks of the arena: its work buffers and the ascent's scratch
static size_t ml_pass_bytes(const int64_t *Ts, int n, int d, int M, const ml_mixture &gm, const ml_opts &o) {
  int64_t T = 0;
  for (int k = 0; k < n; ++k) T += Ts[k];
  ml_arena a{nullptr};
  ml_work w = {};
  ml_work_buffers(a, w, T, n, d, M, gm, o);
  return a.bytes + (o.gv ? kwy_gva_scratch_bytes(Ts, n, d, o.gv->iterations) : 0);
}

// the preparation of the mixture over D dimensions per side: its LDS attribute, and the launch
static int ml_prep_attr(kwy_ctx *ctx, int D) {
  KWY_HIP(hipFuncSetAttribute((const void *)k_gmm_prep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ml_prep_lds(D)));
  return KWY_OK;
}
static void ml_launch_prep(kwy_ctx *ctx, const ml_mixture &gm, int D, int M, double *model, int *status) {
  hipLaunchKernelGGL(k_gmm_prep, dim3(M), dim3(KWY_THREADS), ml_prep_lds(D), ctx->stream, gm.weights, gm.means, gm.covs, D,
                     gm.diff, model, status);
}

// One conversion over a batch of utterances: bt.n, bt.ldx / ldy and every u[k].x / y / keep_* filled in by the caller,
// Ts[k] the utterances' frames.  o.em + 1 trajectory solves; with EM an E-step before each, and one more after the last
// where a log-likelihood is asked for (lik[k]: utterance k's o.em + 1 doubles on the device, or null).  objective[k]:
// the ascent's o.gv->iterations + 1 doubles of utterance k, or null.  who: the prefix of its messages.
static int ml_convert_core(kwy_ctx *ctx, const char *who, ml_batch &bt, const int64_t *Ts, int d, int M,
                           const ml_mixture &gm, const ml_opts &o, double *const *lik, double *const *objective,
                           int **status_out) {
  const int D = 3 * d, n = bt.n, nblk = ml_frag_blocks(D);
  const bool em = o.em >= 0;
  int64_t T = 0, Tmax = 0;
  int Pmax = 1;
  bool want_lik = false;
  ml_em_out out;
  for (int k = 0; k < n; ++k) {
    bt.start[k] = T;
    T += Ts[k];
    Tmax = std::max(Tmax, Ts[k]);
    bt.u[k].pt = ml_partition(Ts[k], d);
    Pmax = std::max(Pmax, bt.u[k].pt.P);
    out.loglik[k] = em ? lik[k] : nullptr;
    want_lik = want_lik || out.loglik[k];
  }
  for (int k = n; k <= KWY_BATCH_MAX; ++k) bt.start[k] = T;
  for (int k = n; k < KWY_BATCH_MAX; ++k) { bt.u[k] = bt.u[0]; out.loglik[k] = nullptr; }
  ml_dims dm = {d, D, M, T};
  ml_arena a{ctx};
  ml_work w = {};
  ml_work_buffers(a, w, T, n, d, M, gm, o);
  if (!a.ok) { ctx->err = std::string(who) + ": scratch arena too small"; return KWY_ENOMEM; }
  *status_out = w.status;
  KWY_HIP(hipMemsetAsync(w.status, 0, sizeof(int) * 16, ctx->stream));
  const int cpw = 64 / d;
  const size_t lds_solve = sizeof(double) * ((size_t)d * 2 * (Pmax - 1) * 5 + 8);
  if (!ml_lds_fits(D)) { ctx->err = std::string(who) + ": feature dimension too large"; return KWY_EINVAL; }
  if (lds_solve > ML_LDS_MAX) { ctx->err = std::string(who) + ": static dimension too large"; return KWY_EINVAL; }
  KWY_HIP(hipFuncSetAttribute((const void *)k_mlpg_finish, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_solve));
  if (em)
    KWY_TRY(kwy_with_blocks<ML_EM_MAXBLK>(nblk, [&](auto nb) -> int {
      KWY_HIP(hipFuncSetAttribute((const void *)k_em_estep<decltype(nb)::value>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)ml_em_lds(decltype(nb)::value)));
      return KWY_OK;
    }));
  auto estep = [&](int first) {
    kwy_with_blocks<ML_EM_MAXBLK>(nblk, [&](auto nb) -> int {
      constexpr int NBLK = decltype(nb)::value;
      KWY_PROF(ctx, "k_em_estep", hipLaunchKernelGGL(k_em_estep<NBLK>, dim3((unsigned)((T + ML_EM_TILE - 1) / ML_EM_TILE)),
                                                     dim3(64 * ML_EM_NW), ml_em_lds(NBLK), ctx->stream, w.X, dm, bt, w.model,
                                                     w.logp, w.iv, w.lc, first, w.E, w.Dv, w.lse));
      return 0;
    });
  };
  KWY_TRY(ml_prep_attr(ctx, D));
  if (!gm.prepared) ml_launch_prep(ctx, gm, D, M, w.model, w.status);
  const unsigned ge = (unsigned)((T * d + 255) / 256);
  hipLaunchKernelGGL(k_delta, dim3(ge), dim3(256), 0, ctx->stream, bt, dm, w.X);
  KWY_TRY(ml_launch_logp(ctx, w.X, dm, w.model, w.logp));
  if (em) {
    hipLaunchKernelGGL(k_em_prep, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, ctx->stream, w.model, D, M, w.iv, w.lc);
    estep(1);
  } else {
    hipLaunchKernelGGL(k_gmm_cond, dim3((unsigned)((T + ML_COND_F * ML_COND_W - 1) / (ML_COND_F * ML_COND_W))),
                       dim3(64 * ML_COND_W), 0, ctx->stream, w.X, dm, w.model, w.logp, w.E, w.Dv, w.mix);
  }
  int fin = (int)((Tmax * d + 4 * ML_FIN_NT - 1) / (4 * ML_FIN_NT));
  if (fin > ML_FIN_WGS) fin = ML_FIN_WGS;
  const int solves = std::max(o.em, 0) + 1;
  for (int k = 0; k < solves; ++k) {
    hipLaunchKernelGGL(k_mlpg_build, dim3(ge), dim3(256), 0, ctx->stream, w.E, w.Dv, bt, dm, w.band);
    if (o.gv && k == solves - 1)
      KWY_HIP(hipMemcpyAsync(w.band2, w.band, sizeof(double) * T * d * 4, hipMemcpyDeviceToDevice, ctx->stream));
    KWY_PROF(ctx, "k_mlpg_chunks", hipLaunchKernelGGL(k_mlpg_chunks, dim3((unsigned)((Pmax + cpw - 1) / cpw), n), dim3(64), 0,
                                                       ctx->stream, w.band, w.rhs, w.Ysp, w.bnd, dm, bt, w.status,
                                                       (long long *)ctx->dbg));
    KWY_PROF(ctx, "k_mlpg_finish", hipLaunchKernelGGL(k_mlpg_finish, dim3((unsigned)fin, n), dim3(ML_FIN_NT), lds_solve,
                                                       ctx->stream, w.band, w.Ysp, w.bnd, dm, bt, w.status,
                                                       (long long *)ctx->dbg));
    if (em && (k < o.em || want_lik)) {
      estep(0);
      if (want_lik) hipLaunchKernelGGL(k_em_loglik, dim3(n), dim3(256), 0, ctx->stream, w.lse, bt, out, k);
    }
  }
  KWY_HIP(hipGetLastError());
  if (!o.gv) return KWY_OK;
  kwy_gva_view v[KWY_BATCH_MAX];
  for (int k = 0; k < n; ++k)
    v[k] = kwy_gva_view{w.band2 + bt.start[k] * d * 4, o.gv->offset ? bt.u[k].x : nullptr, bt.u[k].y, Ts[k], bt.ldy, bt.ldx,
                        objective[k], o.gv->status ? o.gv->status + k : nullptr};
  return kwy_gva_launch(ctx, v, n, d, o.gv->mean, o.gv->var, o.gv->weight, o.gv->iterations);
}

// one pass of launches: jobs q[0 .. n), n <= KWY_BATCH_MAX, the first of them job `first` of the call.  Utterance j
// reads the d static coefficients of row t at x + t * ldx and gets its trajectory at y + t * ldy: the final store of
// k_mlpg_finish runs along the coefficient index whatever the row stride, so consecutive lanes write consecutive
// doubles of a row.
static int ml_convert_pass(kwy_ctx *ctx, const ml_job *q, int n, int first, int ldx, int ldy, int d, int M,
                           const ml_mixture &gm, ml_opts o, int **status_out) {
  ml_batch bt;
  int64_t Ts[KWY_BATCH_MAX];
  double *lik[KWY_BATCH_MAX], *obj[KWY_BATCH_MAX];
  bt.n = n;
  bt.ldx = ldx;
  bt.ldy = ldy;
  for (int k = 0; k < n; ++k) {
    bt.u[k].x = q[k].x; bt.u[k].y = q[k].y; bt.u[k].keep_in = q[k].keep_in; bt.u[k].keep_out = q[k].keep_out;
    Ts[k] = q[k].T;
    lik[k] = q[k].loglik;
    obj[k] = q[k].objective;
  }
  ml_gv_opts gv;
  if (o.gv) {
    gv = *o.gv;
    if (gv.status) gv.status += first;
    o.gv = &gv;
  }
  return ml_convert_core(ctx, o.em < 0 ? "gmm_mlpg" : "gmm_mlpg_em", bt, Ts, d, M, gm, o, lik, obj, status_out);
}

// A call on device pointers: `count` jobs, job j as read(j) gives it, KWY_BATCH_MAX of them per pass.  Every job is
// checked before anything is enqueued.  entry: the name of a batch entry for the check of its own arguments, or null.
template <class READ>
static int ml_convert_jobs(kwy_ctx *ctx, const char *entry, const void *jobs, int count, READ read, int ldx, int ldy, int d,
                           int M, const ml_mixture &gm, const ml_opts &o) {
  if (!ctx) return KWY_EINVAL;
  if (entry && (!jobs || count < 0)) { ctx->err = std::string(entry) + ": bad argument"; return KWY_EINVAL; }
  if (count == 0) return KWY_OK;
  ml_job one;                      // a single-utterance entry allocates nothing
  std::vector<ml_job> many(count > 1 ? count : 0);
  ml_job *q = count > 1 ? many.data() : &one;
  size_t bytes = 0;
  for (int j0 = 0; j0 < count; j0 += KWY_BATCH_MAX) {
    int64_t Ts[KWY_BATCH_MAX];
    const int n = std::min(KWY_BATCH_MAX, count - j0);
    for (int k = 0; k < n; ++k) {
      q[j0 + k] = read(j0 + k);
      KWY_TRY(ml_check(ctx, q[j0 + k], d, M, gm, o));
      Ts[k] = q[j0 + k].T;
    }
    bytes += ml_pass_bytes(Ts, n, d, M, gm, o);
  }
  KWY_HIP(hipSetDevice(ctx->device));
  KWY_TRY(kwy_arena_begin(ctx, bytes));
  for (int j0 = 0; j0 < count; j0 += KWY_BATCH_MAX) {
    int *status;
    KWY_TRY(ml_convert_pass(ctx, &q[j0], std::min(KWY_BATCH_MAX, count - j0), j0, ldx, ldy, d, M, gm, o, &status));
  }
  return KWY_OK;
}

// a T x (d + 1) mel-cepstrum matrix as a job: column 0 (power) is copied, columns 1 .. d are converted.  A null matrix
// stays null for ml_check: no pointer arithmetic on it.
static ml_job ml_mcep_job(const double *mc, int64_t T, double *mc_out, double *loglik = nullptr,
                          double *objective = nullptr) {
  return ml_job{mc ? mc + 1 : nullptr, mc_out ? mc_out + 1 : nullptr, mc, mc_out, T, loglik, objective};
}

static const ml_opts ML_ARGMAX = {-1, false, nullptr};

extern "C" int kwy_gmm_mlpg_dev(kwy_ctx *ctx, const double *x, int64_t T, int d, int M,
                                const double *weights, const double *means, const double *covs, int diff,
                                double *y) {
  const ml_job job = {x, y, nullptr, nullptr, T, nullptr, nullptr};
  return ml_convert_jobs(ctx, nullptr, nullptr, 1, [&](int) { return job; }, d, d, d, M,
                         ml_mixture{weights, means, covs, diff, nullptr}, ML_ARGMAX);
}

extern "C" int64_t kwy_gmm_model_doubles(int d, int M) {
  if (d <= 0 || d > 64 || M <= 0) return 0;
  return (int64_t)ml_model_stride(3 * d) * M;
}

extern "C" int kwy_gmm_prepare_dev(kwy_ctx *ctx, const double *weights, const double *means, const double *covs,
                                   int d, int M, int diff, double *model) {
  if (!ctx) return KWY_EINVAL;
  if (!weights || !means || !covs || !model || d <= 0 || d > 64 || M <= 0) {
    ctx->err = "gmm_prepare: bad argument";
    return KWY_EINVAL;
  }
  KWY_HIP(hipSetDevice(ctx->device));
  const int D = 3 * d;
  KWY_TRY(kwy_arena_begin(ctx, kwy_pad(64)));
  int *status = kwy_arena<int>(ctx, 16);
  if (!status) { ctx->err = "gmm_prepare: scratch arena too small"; return KWY_ENOMEM; }
  KWY_HIP(hipMemsetAsync(status, 0, sizeof(int) * 16, ctx->stream));
  if (ml_prep_lds(D) > ML_LDS_MAX) { ctx->err = "gmm_prepare: feature dimension too large"; return KWY_EINVAL; }
  KWY_TRY(ml_prep_attr(ctx, D));
  KWY_PROF(ctx, "k_gmm_prep", ml_launch_prep(ctx, ml_mixture{weights, means, covs, diff, nullptr}, D, M, model, status));
  KWY_HIP(hipGetLastError());
  int hstatus = 0;
  KWY_HIP(hipMemcpyAsync(&hstatus, status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  KWY_HIP(hipStreamSynchronize(ctx->stream));
  if (hstatus != 0) { ctx->err = "gmm_prepare: source covariance is not positive definite"; return KWY_ENUMERIC; }
  return KWY_OK;
}

extern "C" int kwy_gmm_mlpg_model_dev(kwy_ctx *ctx, const double *x, int64_t T, int d, int M, const double *model,
                                      double *y) {
  const ml_job job = {x, y, nullptr, nullptr, T, nullptr, nullptr};
  return ml_convert_jobs(ctx, nullptr, nullptr, 1, [&](int) { return job; }, d, d, d, M, ml_prepared(model), ML_ARGMAX);
}

// MelCepstrumFeatureConverter.convert at the converter's own sampling rate (kwiiyatta/converter/mcep.py:47-61):
// mc, mc_out: T x (d + 1) mel-cepstra; column 0 (power) is copied, columns 1..d go through delta + GMM + MLPG.
extern "C" int kwy_convert_mcep_dev(kwy_ctx *ctx, const double *mc, int64_t T, int d, int M, const double *model,
                                    double *mc_out) {
  return ml_convert_jobs(ctx, nullptr, nullptr, 1, [&](int) { return ml_mcep_job(mc, T, mc_out); }, d + 1, d + 1, d, M,
                         ml_prepared(model), ML_ARGMAX);
}

extern "C" int kwy_convert_mcep_batch_dev(kwy_ctx *ctx, const kwy_convert_job *jobs, int count, int d, int M,
                                          const double *model) {
  return ml_convert_jobs(ctx, "convert_mcep_batch", jobs, count,
                         [&](int j) { return ml_mcep_job(jobs[j].mc, jobs[j].T, jobs[j].mc_out); }, d + 1, d + 1, d, M,
                         ml_prepared(model), ML_ARGMAX);
}

// Re-alignment of a training pair (include/kwy.h): the conversion of kwy_convert_mcep_batch_dev, its trajectories
// stored straight into columns 2.. of the DTW feature rows (row stride d + 2); columns 0 and 1 (the source's own power
// and voicing terms) are not touched, and there is no T x (d + 1) intermediate.
extern "C" int kwy_realign_features_batch_dev(kwy_ctx *ctx, const kwy_realign_job *jobs, int count, int d, int M,
                                              const double *model) {
  return ml_convert_jobs(ctx, "realign_features_batch", jobs, count, [&](int j) {
    const kwy_realign_job &q = jobs[j];
    return ml_job{q.mc ? q.mc + 1 : nullptr, q.feat ? q.feat + 2 : nullptr, nullptr, nullptr, q.T, nullptr, nullptr};
  }, d + 1, d + 2, d, M, ml_prepared(model), ML_ARGMAX);
}

extern "C" int kwy_convert_mcep_em_batch_dev(kwy_ctx *ctx, const kwy_convert_em_job *jobs, int count, int d, int M,
                                             const double *model, int em_iterations) {
  return ml_convert_jobs(ctx, "convert_mcep_em_batch", jobs, count,
                         [&](int j) { return ml_mcep_job(jobs[j].mc, jobs[j].T, jobs[j].mc_out, jobs[j].loglik); }, d + 1,
                         d + 1, d, M, ml_prepared(model), ml_opts{em_iterations, true, nullptr});
}

extern "C" int kwy_convert_mcep_em_dev(kwy_ctx *ctx, const double *mc, int64_t T, int d, int M, const double *model,
                                       int em_iterations, double *mc_out, double *loglik) {
  const kwy_convert_em_job job = {mc, T, mc_out, loglik};
  return kwy_convert_mcep_em_batch_dev(ctx, &job, 1, d, M, model, em_iterations);
}

// the conversion with the GV ascent behind it (kwy_gvgen.hip; the contract is kwy_gv_ascent's in include/kwy.h)
extern "C" int kwy_convert_mcep_gv_batch_dev(kwy_ctx *ctx, const kwy_convert_gv_job *jobs, int count, int d, int M,
                                             const double *model, int em_iterations, int gv_offset,
                                             const double *gv_mean, const double *gv_var, double weight,
                                             int gv_iterations, int32_t *status) {
  const ml_gv_opts gv = {gv_mean, gv_var, weight, gv_iterations, gv_offset, status};
  return ml_convert_jobs(ctx, "convert_mcep_gv_batch", jobs, count, [&](int j) {
    return ml_mcep_job(jobs[j].mc, jobs[j].T, jobs[j].mc_out, jobs[j].loglik, jobs[j].objective);
  }, d + 1, d + 1, d, M, ml_prepared(model), ml_opts{em_iterations, false, &gv});
}

extern "C" int kwy_convert_mcep_gv_dev(kwy_ctx *ctx, const double *mc, int64_t T, int d, int M, const double *model,
                                       int em_iterations, int gv_offset, const double *gv_mean, const double *gv_var,
                                       double weight, int gv_iterations, double *mc_out, double *loglik,
                                       double *objective, int32_t *status) {
  const kwy_convert_gv_job job = {mc, T, mc_out, loglik, objective};
  return kwy_convert_mcep_gv_batch_dev(ctx, &job, 1, d, M, model, em_iterations, gv_offset, gv_mean, gv_var, weight,
                                       gv_iterations, status);
}

// ---- the entries on host pointers ---------------------------------------------------------------------------------
// what every such call brings and takes home: x and y (T rows of `width`) and the joint mixture over `joint` dimensions
struct ml_staged {
  double *x, *y, *w, *mu, *cv;
};
static void ml_stage(kwy_staging &st, ml_staged &s, const double *x, int64_t T, int width, int M, int joint,
                     const double *weights, const double *means, const double *covs, double *y) {
  st.in(s.x, x, (size_t)T * width);
  st.out(s.y, y, (size_t)T * width);
  st.in(s.w, weights, (size_t)M);
  st.in(s.mu, means, (size_t)M * joint);
  st.in(s.cv, covs, (size_t)M * joint * joint);
}
// the staged outputs and the core's status word in one synchronisation; word 1 or 2 becomes the entry's message
static int ml_finish(kwy_staging &st, int *core_status) {
  kwy_ctx *ctx = st.ctx;
  int hstatus = 0;
  st.fetch(core_status, &hstatus, 1);
  KWY_TRY(st.finish());
  if (hstatus != 0) {
    ctx->err = std::string(st.entry) + (hstatus == 1 ? ": source covariance is not positive definite"
                                                     : ": MLPG system is not positive definite");
    return KWY_ENUMERIC;
  }
  return KWY_OK;
}

// the three kwy_gmm_mlpg* entries: o.gv (if any) with the statistics on the host.  The optional series (nl
// log-likelihoods, no objective values) and the ascent's status word come home through host copies: on a status word of
// the core only y has been written.
static int ml_convert_host(kwy_ctx *ctx, const char *entry, const double *x, int64_t T, int d, int M,
                           const double *weights, const double *means, const double *covs, int diff, ml_opts o,
                           double *y, double *loglik, double *objective, int32_t *gv_status) {
  const ml_mixture host = {weights, means, covs, diff, nullptr};
  KWY_TRY(ml_check(ctx, ml_job{x, y, nullptr, nullptr, T, nullptr, nullptr}, d, M, host, o));
  KWY_HIP(hipSetDevice(ctx->device));
  const int nl = loglik && o.em >= 0 ? o.em + 1 : 0, no = o.gv ? o.gv->iterations + 1 : 0;
  const size_t scratch = ml_pass_bytes(&T, 1, d, M, host, o);
  kwy_staging st(ctx, entry);
  ml_staged s;
  double *dlik = nullptr, *dobj = nullptr;
  std::vector<double> hl(nl), ho(no);
  int32_t hgv = 0;
  ml_gv_opts gv;
  ml_stage(st, s, x, T, d, M, 6 * d, weights, means, covs, y);
  if (nl) st.out(dlik, hl.data(), (size_t)nl);
  if (o.gv) {
    gv = *o.gv;
    st.out(dobj, ho.data(), (size_t)no);
    st.in(gv.mean, o.gv->mean, (size_t)d);
    st.in(gv.var, o.gv->var, (size_t)d);
    st.out(gv.status, &hgv, 1);
    o.gv = &gv;
  }
  KWY_TRY(st.begin(scratch));
  const ml_job job = {s.x, s.y, nullptr, nullptr, T, dlik, dobj};
  int *status;
  KWY_TRY(ml_convert_pass(ctx, &job, 1, 0, d, d, d, M, ml_mixture{s.w, s.mu, s.cv, diff, nullptr}, o, &status));
  KWY_TRY(ml_finish(st, status));
  if (loglik) std::copy(hl.begin(), hl.end(), loglik);
  if (objective) std::copy(ho.begin(), ho.end(), objective);
  if (gv_status) *gv_status = hgv;
  return KWY_OK;
}

extern "C" int kwy_gmm_mlpg(kwy_ctx *ctx, const double *x, int64_t T, int d, int M, const double *weights,
                            const double *means, const double *covs, int diff, double *y) {
  return ml_convert_host(ctx, "gmm_mlpg", x, T, d, M, weights, means, covs, diff, ML_ARGMAX, y, nullptr, nullptr, nullptr);
}

extern "C" int kwy_gmm_mlpg_em(kwy_ctx *ctx, const double *x, int64_t T, int d, int M, const double *weights,
                               const double *means, const double *covs, int diff, int em_iterations, double *y,
                               double *loglik) {
  return ml_convert_host(ctx, "gmm_mlpg_em", x, T, d, M, weights, means, covs, diff, ml_opts{em_iterations, true, nullptr},
                         y, loglik, nullptr, nullptr);
}

extern "C" int kwy_gmm_mlpg_gv(kwy_ctx *ctx, const double *x, int64_t T, int d, int M, const double *weights,
                               const double *means, const double *covs, int diff, int em_iterations, int gv_offset,
                               const double *gv_mean, const double *gv_var, double weight, int gv_iterations, double *y,
                               double *loglik, double *objective, int32_t *status) {
  const ml_gv_opts gv = {gv_mean, gv_var, weight, gv_iterations, gv_offset, nullptr};
  return ml_convert_host(ctx, "gmm_mlpg_gv", x, T, d, M, weights, means, covs, diff, ml_opts{em_iterations, false, &gv}, y,
                         loglik, objective, status);
}

// ---- frame-wise conversion (MLPG switched off) ---------------------------------------------------------------------
struct soft_work {
  double *model, *logp;
  int *status;
};
static void soft_buffers(ml_arena &a, soft_work &w, int64_t T, int D, int M) {
  a.take(w.model, ml_model_stride(D) * M);
  a.take(w.logp, (size_t)T * M);
  a.take(w.status, 16);
}

// x, y: T x D device rows; gm: the joint mixture over 2 D dimensions, on the device
static int soft_core(kwy_ctx *ctx, const double *x, int64_t T, int D, int M, const ml_mixture &gm, double *y,
                     int **status_out) {
  ml_dims dm = {D, D, M, T};
  ml_arena a{ctx};
  soft_work w;
  soft_buffers(a, w, T, D, M);
  if (!a.ok) { ctx->err = "gmm_convert_frames: scratch arena too small"; return KWY_ENOMEM; }
  *status_out = w.status;
  KWY_HIP(hipMemsetAsync(w.status, 0, sizeof(int) * 16, ctx->stream));
  if (!ml_lds_fits(D) || D > 192 || M > 256) {
    // (3 D^2 doubles of LDS for the preparation: 160 KB hold D <= 82)
    ctx->err = "gmm_convert_frames: feature dimension (<= 82 per side) or mixture count (<= 256) too large";
    return KWY_EINVAL;
  }
  KWY_TRY(ml_prep_attr(ctx, D));
  if (!gm.prepared) ml_launch_prep(ctx, gm, D, M, w.model, w.status);
  KWY_TRY(ml_launch_logp(ctx, x, dm, w.model, w.logp));
  hipLaunchKernelGGL(k_gmm_soft, dim3((unsigned)T), dim3(128), 0, ctx->stream, x, dm, w.model, w.logp, y);
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

static int soft_check(kwy_ctx *ctx, const void *x, int64_t T, int D, int M, const void *w, const void *mu,
                      const void *cv, const void *y) {
  if (!ctx) return KWY_EINVAL;
  if (!x || !w || !mu || !cv || !y || T <= 0 || D <= 0 || M <= 0) {
    ctx->err = "gmm_convert_frames: bad argument";
    return KWY_EINVAL;
  }
  return KWY_OK;
}

static size_t soft_bytes(int64_t T, int D, int M) {
  ml_arena a{nullptr};
  soft_work w;
  soft_buffers(a, w, T, D, M);
  return a.bytes;
}

extern "C" int kwy_gmm_convert_frames_dev(kwy_ctx *ctx, const double *x, int64_t T, int D, int M,
                                          const double *weights, const double *means, const double *covs, int diff,
                                          double *y) {
  KWY_TRY(soft_check(ctx, x, T, D, M, weights, means, covs, y));
  KWY_HIP(hipSetDevice(ctx->device));
  KWY_TRY(kwy_arena_begin(ctx, soft_bytes(T, D, M)));
  int *status;
  return soft_core(ctx, x, T, D, M, ml_mixture{weights, means, covs, diff, nullptr}, y, &status);
}

extern "C" int kwy_gmm_convert_frames(kwy_ctx *ctx, const double *x, int64_t T, int D, int M, const double *weights,
                                      const double *means, const double *covs, int diff, double *y) {
  KWY_TRY(soft_check(ctx, x, T, D, M, weights, means, covs, y));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "gmm_convert_frames");
  ml_staged s;
  ml_stage(st, s, x, T, D, M, 2 * D, weights, means, covs, y);
  KWY_TRY(st.begin(soft_bytes(T, D, M)));
  int *status;
  KWY_TRY(soft_core(ctx, s.x, T, D, M, ml_mixture{s.w, s.mu, s.cv, diff, nullptr}, s.y, &status));
  return ml_finish(st, status);
}
