// kwy_nmf_args.hpp -- the host arithmetic of the exemplar (NMF) converter: its limits and its scratch layout.
// No HIP in here: kwy_nmf.hip includes it, and so can a plain host program that walks the argument checks under a
// sanitizer (selftest/nmf_args_main.cpp).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define NMF_MAX_ATOMS 8192
#define NMF_MAX_BINS 2049
#define NMF_MAX_ITERATIONS 1000
#define NMF_ROWS 128        // frames of a workgroup's tile
#define NMF_COLS 64         // columns of a workgroup's tile, and the unit every leading dimension is padded to
#define NMF_PAD_BLOCKS 1024 // workgroups of a padding pass at the most: one count of offending entries each

static inline size_t nmf_pad256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline int64_t nmf_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// NULL when the sizes are within the contract of kwy_nmf_convert (include/kwy.h), else what is wrong
static inline const char *nmf_sizes_error(int A, int B, int64_t T, int iterations, double sparsity) {
  if (A < 1 || A > NMF_MAX_ATOMS) return "nmf_convert: need 1 <= A <= 8192 atoms";
  if (B < 2 || B > NMF_MAX_BINS) return "nmf_convert: need 2 <= B <= 2049 bins";
  if (T < 0) return "nmf_convert: negative number of frames";
  if (T > 0x7fffffffLL) return "nmf_convert: more than 2^31 - 1 frames in one call";
  if (iterations < 0 || iterations > NMF_MAX_ITERATIONS) return "nmf_convert: need 0 <= iterations <= 1000";
  if (!(sparsity >= 0.0) || !(sparsity <= 1.7976931348623157e308)) return "nmf_convert: sparsity must be finite and >= 0";
  return NULL;
}

// NULL when the pointers fit together: Tg and Y go together (both or neither), and something must be asked for
static inline const char *nmf_pointers_error(const void *S, const void *Tg, const void *X, const void *Y, const void *H,
                                             const void *objective) {
  if (!S || !X) return "nmf_convert: null S or X";
  if ((Tg == NULL) != (Y == NULL)) return "nmf_convert: Tg and Y go together";
  if (!Y && !H && !objective) return "nmf_convert: no output asked for";
  return NULL;
}

// The scratch of a call, every part 256-byte aligned behind a base that is rounded up to 256 itself:
//   S, Tg  Ap x Bp   the atoms, zero beyond A and B
//   X, Q   Tp x Bp   the frames and the ratio X / R
//   H      Tp x Ap   the activations
//   bad    5 x NMF_PAD_BLOCKS counts of entries outside the contract (S, Tg, X, h0, spare)
struct nmf_layout {
  int Ap, Bp, A16, B16;
  int64_t Tp;
  size_t off_S, off_Tg, off_X, off_Q, off_H, off_bad, total;
};

static inline nmf_layout nmf_make_layout(int A, int B, int64_t T) {
  nmf_layout L;
  L.Ap = (int)nmf_round_up(A, NMF_COLS);
  L.Bp = (int)nmf_round_up(B, NMF_COLS);
  L.A16 = (int)nmf_round_up(A, 16);
  L.B16 = (int)nmf_round_up(B, 16);
  L.Tp = nmf_round_up(T, NMF_ROWS);
  size_t off = 0;
  const size_t atoms = nmf_pad256(sizeof(double) * (size_t)L.Ap * L.Bp);
  const size_t frames = nmf_pad256(sizeof(double) * (size_t)L.Tp * L.Bp);
  L.off_S = off; off += atoms;
  L.off_Tg = off; off += atoms;
  L.off_X = off; off += frames;
  L.off_Q = off; off += frames;
  L.off_H = off; off += nmf_pad256(sizeof(double) * (size_t)L.Tp * L.Ap);
  L.off_bad = off; off += nmf_pad256(sizeof(int) * 5 * NMF_PAD_BLOCKS);
  L.total = off + 256;   // room to round the caller's base up
  return L;
}

static inline size_t nmf_scratch_bytes(int A, int B, int64_t T) {
  if (T <= 0 || nmf_sizes_error(A, B, T, 0, 0.0)) return 0;
  return nmf_make_layout(A, B, T).total;
}
