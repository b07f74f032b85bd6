// kwy_mfma.hpp -- the parts that the double-precision matrix-core kernels share: one copy of each.
// Included by the five files that issue v_mfma_f64_16x16x4_f64 (__builtin_amdgcn_mfma_f64_16x16x4f64): kwy_gmmfit.hip,
// kwy_kmeans.hip, kwy_mlpg.hip, kwy_mcep.hip, kwy_cheaptrick.hip.
//
// Lane map of the instruction (lane l of the wavefront, r = accumulator element 0 .. 3):
//   A[row l&15][k l>>4],  B[k l>>4][col l&15],  D[row (l>>4)+4r][col l&15].
// Throughout: ar = l & 15, ak = l >> 4.
//
// Fragment order.  A B operand kept in LDS is stored as FRAGMENTS: the 64 lane values of one (column block, k-step) in
// lane order, so that a wavefront reads an operand with one conflict-free 512-byte load at frag[ks * 64 + lane].
//   triangular (Z = L^-1, lower-triangular, NBLK blocks of 16 columns): fragment (nb, ks), ks < 4 nb + 4, sits at
//     2 nb (nb + 1) + ks and holds Z[16 nb + (l & 15)][4 ks + (l >> 4)], zero above the diagonal and beyond D:
//     kwy_tri_frags(NBLK) = 2 NBLK (NBLK + 1) fragments, then 16 NBLK doubles of per-column data (kwy_tri_lds_doubles);
//   rectangular (k_km_assign: 4 blocks of 16 centres, KS = 4 NBLK k-steps each): fragment (mb, ks) at mb KS + ks, then
//     64 doubles (kwy_km_lds_doubles).
//
// Who uses what:
//   kwy_v4f64                         every kernel that issues the instruction
//   kwy_static_for                    k_fit_cov (its blocks of the lower triangle, dealt to the wavefronts)
//   kwy_tri_fill                      k_fit_logprob (packed triangle), k_gmm_logp_frag (row-major)
//   kwy_row_sum15                     k_fit_logprob, k_gmm_logp_frag
//   kwy_row_allreduce                 k_fit_resp (max, sum), k_km_pp_dist (sum), k_km_assign ((value, index) minimum)
//   kwy_with_blocks, LDS formulas     the launches of the kernels that are templates over the column-block count:
//                                     k_fit_logprob, k_fit_sums, k_fit_cov, k_km_assign (ten and above go to <10>),
//                                     k_gmm_logp_frag, k_em_estep (one to six)
// The pair tile itself -- 32 rows per wavefront as two 16-row sub-tiles a0[KS], a1[KS] loaded straight from global
// memory, every B fragment read feeding two accumulator chains -- stays written out in k_fit_logprob, k_km_assign and
// k_gmm_logp_frag: as routines here its operand load and its chain changed those kernels' instruction streams
// (profiles/mfma_header_kernels.txt).
//
// The accumulators rely on the build flag -mllvm -amdgpu-mfma-vgpr-form=1 (csrc/build.sh): an accumulator chain then
// stays in architectural VGPRs across its loop instead of being copied to and from AGPRs around every instruction.
#pragma once

#include <type_traits>

#include "kwy_device.hpp"

typedef double kwy_v4f64 __attribute__((ext_vector_type(4)));

// compile-time loop: f(std::integral_constant<int, I>) for I in [I0, I1)
template <int I0, int I1, class F>
__device__ __forceinline__ void kwy_static_for(F &&f) {
  if constexpr (I0 < I1) {
    f(std::integral_constant<int, I0>{});
    kwy_static_for<I0 + 1, I1>(f);
  }
}

// ---- the lower-triangular factor in fragment order ---------------------------------------------------------------------
__host__ __device__ constexpr int kwy_tri_frags(int nblk) { return 2 * nblk * (nblk + 1); }
__host__ __device__ constexpr size_t kwy_tri_lds_doubles(int nblk) { return (size_t)kwy_tri_frags(nblk) * 64 + 16 * nblk; }
__host__ __device__ constexpr size_t kwy_km_lds_doubles(int nblk) { return (size_t)4 * 4 * nblk * 64 + 64; }

// zf[0 .. kwy_tri_frags(NBLK) * 64) by a block of NT threads; z(j, i) = element (row j, column i <= j) of the factor
template <int NBLK, int NT, class SRC>
__device__ __forceinline__ void kwy_tri_fill(double *zf, int D, int tid, SRC z) {
  for (int idx = tid; idx < kwy_tri_frags(NBLK) * 64; idx += NT) {
    const int f = idx >> 6, l = idx & 63;
    int nb = 0;
    while (2 * (nb + 1) * (nb + 2) <= f) ++nb;
    const int ks = f - 2 * nb * (nb + 1);
    const int j = 16 * nb + (l & 15), i = 4 * ks + (l >> 4);
    zf[idx] = (j < D && i <= j) ? z(j, i) : 0.0;
  }
}

// ---- reductions over the 16 lanes of a DPP row (the 16 columns of an accumulator row) ----------------------------------
// sum: lane 15 of the row ends up with the total (row_shr 1, 2, 4, 8)
__device__ __forceinline__ void kwy_row_sum15(double &v, double &w) {   // two values, their steps interleaved
  v += kwy_dpp_f64<0x111>(v); w += kwy_dpp_f64<0x111>(w);
  v += kwy_dpp_f64<0x112>(v); w += kwy_dpp_f64<0x112>(w);
  v += kwy_dpp_f64<0x114>(v); w += kwy_dpp_f64<0x114>(w);
  v += kwy_dpp_f64<0x118>(v); w += kwy_dpp_f64<0x118>(w);
}

// all-reduce by rotation (row_ror 1, 2, 4, 8): every lane ends up with op over the row, in the same order of operands
// relative to itself.  For doubles, and for a (value, index) pair.
struct kwy_val_idx { double v; int i; };
template <int CTRL>
__device__ __forceinline__ double kwy_row_rot(double v) { return kwy_dpp_f64<CTRL>(v); }
template <int CTRL>
__device__ __forceinline__ kwy_val_idx kwy_row_rot(kwy_val_idx a) {
  return kwy_val_idx{kwy_dpp_f64<CTRL>(a.v), (int)kwy_dpp_u32<CTRL>((uint32_t)a.i)};
}
template <class T, class OP>
__device__ __forceinline__ T kwy_row_allreduce(T v, OP op) {
  v = op(v, kwy_row_rot<0x121>(v));   // row_ror:1
  v = op(v, kwy_row_rot<0x122>(v));
  v = op(v, kwy_row_rot<0x124>(v));
  v = op(v, kwy_row_rot<0x128>(v));
  return v;
}
// the lexicographic (value, index) minimum: of equal values the lower index
__device__ __forceinline__ kwy_val_idx kwy_lex_min(kwy_val_idx a, kwy_val_idx o) {
  return (o.v < a.v || (o.v == a.v && o.i < a.i)) ? o : a;
}

// ---- host side: from the column-block count to a template instantiation ------------------------------------------------
// f(std::integral_constant<int, N>) for N = min(nblk, MAXBLK), nblk >= 1: the kernels with one code path per number of
// 16-column blocks are templates over it
template <int MAXBLK, int N = 1, class F>
static auto kwy_with_blocks(int nblk, F &&f) {
  if constexpr (N >= MAXBLK) {
    return f(std::integral_constant<int, MAXBLK>());
  } else {
    if (nblk <= N) return f(std::integral_constant<int, N>());
    return kwy_with_blocks<MAXBLK, N + 1>(nblk, f);
  }
}
