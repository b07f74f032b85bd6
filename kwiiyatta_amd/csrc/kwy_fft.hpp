// kwy_fft.hpp -- the double-precision complex and real FFTs that the gfx950 kernels run inside one workgroup's LDS.
//
// All of them are radix-8 decimation-in-frequency transforms of H = 2^LOG2H complex points (512 .. 4096) that work in
// place in ONE buffer, close with a radix-4 or radix-2 pass where LOG2H is no multiple of 3, and are unnormalised in
// both directions.  A real transform of N = 2H samples is the complex one on the packed samples plus a "split" of the
// pairs (k, H - k).  The forms:
//
//   Stockham chain     kwy_fft_pass8_core per pass: loads, barrier, stores to the Stockham places of the same buffer,
//                      barrier; natural order in, natural order out.  Pass factors from
//                        kwy_tw_table   a table exp(-2 pi i k / H), global or LDS     (kwy_fft_inplace)
//                        kwy_tw_reg     the thread's own registers                    (kwy_fft_inplace_w, .._sel_w)
//                        kwy_tw_powers  the per-context table of ready-made powers, by scalar loads: the stride-64
//                                       pass of every form
//   first passes       dense (kwy_fft_pass8_core<.., 0, ..>); half input, zero from x[H/2 + 1] on, chosen at run time
//                      (kwy_fft_pass8_first_sel_core) or at compile time (.._first_half_core); sparse input, zero but
//                      for x[0 .. H/8], handed over in registers (.._first_sparse_core).  The loads, the butterfly and
//                      the factors of each kind of input are ONE routine that leaves the eight results in registers
//                      (kwy_first8_dense, kwy_first8_sparse); a form adds its guard, barriers and stores.
//   drained tail       kwy_fft_tail4_drain: the closing radix-4 pass leaves the pairs (k, H - k) in the registers of
//                      the thread that consumes them instead of storing the transform
//   wave-local form    kwy_fftwl_*: H = 2048 on 256 threads, the two middle passes local to a wavefront, two workgroup
//                      barriers in front of the drained tail instead of six; a layout of its own
//   real splits        kwy_rsplit_pair / kwy_irsplit_pair (whole bins, in place; the loops are kwy_rfft_inplace's,
//                      kwy_syn_rsplit's, ...), kwy_syn_rsplit_fold (real parts only, fused with the cepstrum fold),
//                      kwy_rfft_bin2_* / kwy_rfft_pair_power2_* (bins or powers of single pairs)
//
// Who runs what:
//   k_cheaptrick, k_dio_filter, k_ms, k_fft_filter, k_sp2mc   kwy_rfft_inplace / kwy_irfft_inplace: table chain + split
//   k_syn_pulse        table chain with the dense or the compile-time half first pass (kwy_fft_inplace_rest behind it),
//                      the splits with the pair twiddles of its "virtual" threads, kwy_syn_fold / kwy_syn_rsplit_fold
//   k_d4c_lovetrain    kwy_fft_inplace_w, bins by kwy_rfft_bin2_w
//   k_d4c_body         4096-sample frames: wave-local form (kwy_fftwl_first_sel, kwy_fftwl_rest, kwy_fftwl_tail4_drain);
//                      the other lengths: kwy_fft_inplace_sel_w, powers by kwy_rfft_pair_power2_w
//   k_d4c_bands        kwy_fft_pass8_first_sparse_core or kwy_fft_inplace_w, the thread-held chain behind it, and at
//                      4096 samples kwy_fft_tail4_drain
//
// What they share:
//   * Barriers.  Every routine that reads z expects a workgroup barrier between the caller's last store to z and the
//     call, and every routine that stores to z ENDS with one.  The exceptions say so at their definition: the sparse
//     first passes read nothing (the buffer must be free, no barrier needed in front), the inverse real transforms open
//     with a barrier of their own, the drains only read (the caller puts a barrier behind them before z is stored to), and the bin /
//     power routines neither store nor synchronise.
//   * "The same expressions, so the same bits."  The forms are interchangeable bit for bit (tests/test_fft_*_gpu.py hold
//     them to that), and the fixtures under tests/golden pin the kernels' outputs as bits.  That rests on every
//     butterfly being formed by the same source expressions on the same operands in the same order, whichever thread
//     runs it and wherever its points lie: kwy_dft8 / kwy_dft8_low5 / kwy_dft4 for the sums, kwy_twiddle_chain for
//     the factor's 2nd .. 7th powers (w2 = w1 w1, w4 = w2 w2, w3 = w1 w2, w5 = w4 w1, w6 = w4 w2, w7 = w4 w3),
//     cmulf(w_m, a_m) for the products, kwy_tw_octant / kwy_tw_hex for pair twiddles.  The powers table is filled
//     by kwy_twiddle_chain itself, under the same -ffp-contract=off.  A change to one of these expressions changes
//     every form at once -- and every fixture.
#pragma once

#include "kwy_device.hpp"

struct __attribute__((aligned(16))) kwy_c { double x, y; };  // complex double (16 B, LDS b128 accesses)

__device__ __forceinline__ kwy_c cadd(kwy_c a, kwy_c b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ kwy_c csub(kwy_c a, kwy_c b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ kwy_c cmul(kwy_c a, kwy_c b) {
  return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}
// The same product with explicit fused multiply-adds: 4 instructions instead of 6.  The library is compiled with
// -ffp-contract=off because several kernels reproduce serial CPU roundings exactly (phase accumulation, DTW costs,
// numpy's accept / reject); the FFT passes are not among them -- their results are compared at 1e-8 ... 1e-12 -- and
// the twiddle products are 40 % of a radix-8 pass.
__device__ __forceinline__ kwy_c cmulf(kwy_c a, kwy_c b) {
  return {__builtin_fma(a.x, b.x, -(a.y * b.y)), __builtin_fma(a.x, b.y, a.y * b.x)};
}

// exp(-2 pi i (t + r*NT) / N) from base = exp(-2 pi i t / N) when NT = N/8: base times an 8th root of unity
__device__ __forceinline__ kwy_c kwy_tw_octant(kwy_c b, int r) {
  const double h = 0.70710678118654752440;
  switch (r & 7) {
    case 0: return b;
    case 1: return {h * (b.x + b.y), h * (b.y - b.x)};
    case 2: return {b.y, -b.x};
    case 3: return {h * (b.y - b.x), h * (-b.x - b.y)};
    case 4: return {-b.x, -b.y};
    case 5: return {h * (-b.x - b.y), h * (b.x - b.y)};
    case 6: return {-b.y, b.x};
    default: return {h * (b.x - b.y), h * (b.x + b.y)};
  }
}

// ------------------------------------------------------------------- butterflies
template <bool INV>
__device__ __forceinline__ kwy_c kwy_rot90(kwy_c a) {  // a * (-i) forward, a * (+i) inverse
  return INV ? kwy_c{-a.y, a.x} : kwy_c{a.y, -a.x};
}

template <bool INV>
__device__ __forceinline__ void kwy_dft8(kwy_c (&a)[8]) {
  const double h = 0.70710678118654752440;
  kwy_c t0 = cadd(a[0], a[4]), t1 = csub(a[0], a[4]);
  kwy_c t2 = cadd(a[2], a[6]), t3 = kwy_rot90<INV>(csub(a[2], a[6]));
  kwy_c t4 = cadd(a[1], a[5]), t5 = csub(a[1], a[5]);
  kwy_c t6 = cadd(a[3], a[7]), t7 = csub(a[3], a[7]);
  kwy_c u0 = cadd(t0, t2), u1 = csub(t0, t2), u2 = cadd(t4, t6), u3 = kwy_rot90<INV>(csub(t4, t6));
  // c1 = t5 * w8, c3 = t7 * w8^3 with w8 = exp(-+ i pi/4)
  kwy_c c1 = INV ? kwy_c{h * (t5.x - t5.y), h * (t5.x + t5.y)} : kwy_c{h * (t5.x + t5.y), h * (t5.y - t5.x)};
  kwy_c c3 = INV ? kwy_c{h * (-t7.x - t7.y), h * (t7.x - t7.y)} : kwy_c{h * (t7.y - t7.x), h * (-t7.x - t7.y)};
  kwy_c v0 = cadd(t1, t3), v1 = csub(t1, t3), v2 = cadd(c1, c3), v3 = kwy_rot90<INV>(csub(c1, c3));
  a[0] = cadd(u0, u2); a[4] = csub(u0, u2); a[2] = cadd(u1, u3); a[6] = csub(u1, u3);
  a[1] = cadd(v0, v2); a[5] = csub(v0, v2); a[3] = cadd(v1, v3); a[7] = csub(v1, v3);
}

// kwy_dft8 of an input whose a[5], a[6], a[7] are zero: the sums and differences with those zeros are left out, every
// other operation keeps its operands and order, so the values are kwy_dft8's (a zero may come out with the other sign).
template <bool INV>
__device__ __forceinline__ void kwy_dft8_low5(kwy_c (&a)[8]) {
  const double h = 0.70710678118654752440;
  kwy_c t0 = cadd(a[0], a[4]), t1 = csub(a[0], a[4]);
  kwy_c t2 = a[2], t3 = kwy_rot90<INV>(a[2]);
  kwy_c t4 = a[1], t5 = a[1];
  kwy_c t6 = a[3], t7 = a[3];
  kwy_c u0 = cadd(t0, t2), u1 = csub(t0, t2), u2 = cadd(t4, t6), u3 = kwy_rot90<INV>(csub(t4, t6));
  kwy_c c1 = INV ? kwy_c{h * (t5.x - t5.y), h * (t5.x + t5.y)} : kwy_c{h * (t5.x + t5.y), h * (t5.y - t5.x)};
  kwy_c c3 = INV ? kwy_c{h * (-t7.x - t7.y), h * (t7.x - t7.y)} : kwy_c{h * (t7.y - t7.x), h * (-t7.x - t7.y)};
  kwy_c v0 = cadd(t1, t3), v1 = csub(t1, t3), v2 = cadd(c1, c3), v3 = kwy_rot90<INV>(csub(c1, c3));
  a[0] = cadd(u0, u2); a[4] = csub(u0, u2); a[2] = cadd(u1, u3); a[6] = csub(u1, u3);
  a[1] = cadd(v0, v2); a[5] = csub(v0, v2); a[3] = cadd(v1, v3); a[7] = csub(v1, v3);
}

// the radix-4 butterfly of the closing pass (no factors)
template <bool INV>
__device__ __forceinline__ void kwy_dft4(kwy_c (&a)[4]) {
  const kwy_c apc = cadd(a[0], a[2]), amc = csub(a[0], a[2]);
  const kwy_c bpd = cadd(a[1], a[3]), jb = kwy_rot90<INV>(csub(a[1], a[3]));
  a[0] = cadd(apc, bpd); a[1] = cadd(amc, jb); a[2] = csub(apc, bpd); a[3] = csub(amc, jb);
}

// w1^1 .. w1^7: THE expressions of a pass factor's powers.  The passes, the sparse first passes and the fill kernel of
// the powers table all come here; the self-test's k_twiddle_powers_ref spells them out once more, on purpose, as what
// the table is compared with.  (Named values, no arrays or loops: the compiler sees what it saw when every pass
// spelled the chain out itself.)
struct kwy_tw7 { kwy_c w1, w2, w3, w4, w5, w6, w7; };
__device__ __forceinline__ kwy_tw7 kwy_twiddle_chain(kwy_c w1) {
  const kwy_c w2 = cmulf(w1, w1), w4 = cmulf(w2, w2);
  const kwy_c w3 = cmulf(w1, w2), w5 = cmulf(w4, w1), w6 = cmulf(w4, w2);
  const kwy_c w7 = cmulf(w4, w3);
  return {w1, w2, w3, w4, w5, w6, w7};
}
// a[m] *= w1^m behind a radix-8 butterfly; w1 is the forward factor, the inverse direction conjugates it first
template <bool INV>
__device__ __forceinline__ void kwy_dft8_twiddle(kwy_c (&a)[8], kwy_c w1) {
  if (INV) w1.y = -w1.y;
  const kwy_tw7 w = kwy_twiddle_chain(w1);
  a[1] = cmulf(w.w1, a[1]); a[2] = cmulf(w.w2, a[2]); a[3] = cmulf(w.w3, a[3]);
  a[4] = cmulf(w.w4, a[4]); a[5] = cmulf(w.w5, a[5]); a[6] = cmulf(w.w6, a[6]);
  a[7] = cmulf(w.w7, a[7]);
}

// ------------------------------------------------- in-place radix-8 LDS FFT: the Stockham chain
// One buffer: every pass loads its operands into registers, all threads meet at a barrier, and the results go back to
// the same array (Stockham ordering, so the output is in natural order).  8 points per thread and pass: an H = 2048
// point transform is 8*8*8*4 = 4 LDS round trips.
//
// Radix-8 pass with sub-transform stride S = 2^LOG2S over H points, in place.
// The first pass (S = 1) would store each thread's 8 results 128 B apart -- an
// 8-way conflict on ds_write_b128 -- so it stores to i ^ ((i >> 3) & 7) instead,
// and the second pass (S = 8) reads through the same permutation.
// tw: exp(-2 pi i k / H) for k < H/8 at least (the factors of one radix-8 pass are tw[ps], ps < H/8,
// and its 2nd .. 7th powers, which are formed by multiplication); it may live in LDS.
struct kwy_tw_table {   // pass factor from a table exp(-2 pi i k / H) (global or LDS)
  const kwy_c *tw;
  __device__ __forceinline__ kwy_c operator()(int ps) const { return tw[ps]; }
};
// The pass with sub-transform stride 64 (LOG2S == 6): ps = (j >> 6) << 6 is ONE value per wavefront (NT is a multiple of
// 64), so its factor and the 2nd .. 7th powers come ready-made from the per-context table of kwy_get_twiddle_powers
// (kwy_ctx.hip): entry u = j >> 6 holds w^1 .. w^7 at [1] .. [7] of 8 complex, w = exp(-2 pi i 64 u / H), formed by
// kwy_twiddle_chain like the per-lane path's, so the bits are the same.  The index goes through readfirstlane and the
// table is const __restrict__: the factors arrive by scalar loads and feed the products as scalar operands -- no
// vector instruction forms them and no vector register holds them.  The inverse direction conjugates at use
// (cmulf of conjugates is exactly the conjugate of cmulf).
#define KWY_TWP_ENTRY 8                                   // complex per table entry ([0] unused)
#define KWY_TWP_ENTRIES(LOG2H) ((1 << (LOG2H)) / 512)     // distinct ps of the stride-64 pass of an H-point transform
struct kwy_tw_powers {
  const kwy_c *__restrict__ pw;
};
// one table entry from w^1 (the table's fill kernel and the self-test)
__device__ __forceinline__ void kwy_twiddle_powers(kwy_c w1, kwy_c *o) {
  const kwy_tw7 w = kwy_twiddle_chain(w1);
  o[0] = {1.0, 0.0}; o[1] = w.w1; o[2] = w.w2; o[3] = w.w3; o[4] = w.w4; o[5] = w.w5; o[6] = w.w6; o[7] = w.w7;
}
// fills the table from tw = exp(-2 pi i k / H): one thread per entry, ordinary vector stores (a template so that the
// library and the self-test library launch the same code)
template <int = 0>
__global__ __launch_bounds__(64) void k_twiddle_powers_fill(const kwy_c *__restrict__ tw, kwy_c *__restrict__ tab, int entries) {
  const int u = threadIdx.x;
  if (u < entries) kwy_twiddle_powers(tw[64 * u], tab + KWY_TWP_ENTRY * u);
}
template <class TW> struct kwy_tw_has_powers { static constexpr bool value = false; };
template <> struct kwy_tw_has_powers<kwy_tw_powers> { static constexpr bool value = true; };
struct kwy_tw_reg {     // pass factor held by the thread itself (one butterfly per thread and pass)
  kwy_c w;
  // behind an optimisation barrier: its 2nd..7th powers are formed again in every pass instead of
  // being computed once per kernel and carried (spilled) across all transforms
  __device__ __forceinline__ kwy_c operator()(int) const {
    kwy_c v = w;
    asm volatile("" : "+v"(v.x), "+v"(v.y));
    return v;
  }
};

template <int LOG2H, int LOG2S, int NT, bool INV, class TW>
__device__ __forceinline__ void kwy_fft_pass8_core(kwy_c *z, TW tw) {
  constexpr int H = 1 << LOG2H, Q = H / 8, S = 1 << LOG2S;
  constexpr int IT = (Q + NT - 1) / NT;
  constexpr bool LAST = (LOG2S + 3 == LOG2H);
  static_assert(Q >= 8, "transform too short for the radix-8 kernel");
  kwy_c a[IT][8];
  const int tid = kwy_tid_opaque();
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int j = tid + it * NT;
    if (j < Q) {
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int idx = j + m * Q;
        a[it][m] = z[(LOG2S == 3) ? (idx ^ ((idx >> 3) & 7)) : idx];
      }
      kwy_dft8<INV>(a[it]);
      if constexpr (kwy_tw_has_powers<TW>::value) {
        static_assert(LOG2S == 6 && !LAST && NT % 64 == 0 && Q % 64 == 0, "the wave-uniform pass");
        const kwy_c *__restrict__ pw = tw.pw + KWY_TWP_ENTRY * __builtin_amdgcn_readfirstlane(j >> 6);
#pragma unroll
        for (int m = 1; m < 8; ++m) {
          kwy_c w = pw[m];
          if (INV) w.y = -w.y;
          a[it][m] = cmulf(w, a[it][m]);
        }
      } else if (!LAST) {
        kwy_dft8_twiddle<INV>(a[it], tw((j >> LOG2S) << LOG2S));
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int j = tid + it * NT;
    if (j < Q) {
      const int q = j & (S - 1), p = j >> LOG2S;
      const int o = q + ((8 * p) << LOG2S);
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        if (LOG2S == 0) z[8 * j + (m ^ (j & 7))] = a[it][m];
        else z[o + (m << LOG2S)] = a[it][m];
      }
    }
  }
  __syncthreads();
}

template <int LOG2H, int LOG2S, int NT, bool INV>
__device__ __forceinline__ void kwy_fft_pass8(kwy_c *z, const kwy_c *__restrict__ tw) {
  kwy_fft_pass8_core<LOG2H, LOG2S, NT, INV>(z, kwy_tw_table{tw});
}
// the stride-64 pass: factors from the powers table where it is not the closing pass (which has none)
template <int LOG2H, int NT, bool INV>
__device__ __forceinline__ void kwy_fft_pass8_s64(kwy_c *z, const kwy_c *__restrict__ pw) {
  if constexpr (LOG2H == 9) kwy_fft_pass8_core<LOG2H, 6, NT, INV>(z, kwy_tw_table{nullptr});
  else kwy_fft_pass8_core<LOG2H, 6, NT, INV>(z, kwy_tw_powers{pw});
}

// ---- first passes (S = 1) that know their input, one butterfly per thread.  The two routines below are the pass up to
// its results in registers, for the Stockham chain here and the wave-local form further down.
// Input that is dense, or (`half`, block-uniform or a constant) zero from x[H/2 + 1] on -- a real sequence of 2H samples
// that ends at sample H, packed: inputs 4 .. 7 of every butterfly are then known zeros, except x[H/2], input 4 of
// thread 0; four (thread 0: five) loads instead of eight, and the caller does not have to write the zeros.  Only the
// loads and the butterfly branch: a kernel at its register budget carries one set of factors, powers and stores.
template <int LOG2H, bool INV, class TW>
__device__ __forceinline__ void kwy_first8_dense(const kwy_c *z, int j, TW tw, bool half, kwy_c (&a)[8]) {
  constexpr int H = 1 << LOG2H, Q = H / 8;
#pragma unroll
  for (int m = 0; m < 4; ++m) a[m] = z[j + m * Q];
  if (half) {
    a[4] = {0.0, 0.0};
    if (j == 0) a[4] = z[H / 2];
    kwy_dft8_low5<INV>(a);
  } else {
#pragma unroll
    for (int m = 4; m < 8; ++m) a[m] = z[j + m * Q];
    kwy_dft8<INV>(a);
  }
  kwy_dft8_twiddle<INV>(a, tw(j));
}
// Input that is zero except for x[0 .. H/8]: thread j supplies x[j] in a0, thread 0 also x[H/8] in a1.  The butterfly
// degenerates to a copy (every output of thread j is x[j] times its factor), so nothing is read from LDS.
template <bool INV, class TW>
__device__ __forceinline__ void kwy_first8_sparse(int j, TW tw, kwy_c a0, kwy_c a1, kwy_c (&a)[8]) {
  if (j == 0) {
    a[0] = a0; a[1] = a1;
#pragma unroll
    for (int m = 2; m < 8; ++m) a[m] = {0.0, 0.0};
    kwy_dft8<INV>(a);
  } else {
    const kwy_c w1 = tw(j);
    a[0] = a0; a[1] = a0; a[2] = a0; a[3] = a0; a[4] = a0; a[5] = a0; a[6] = a0; a[7] = a0;
    kwy_dft8_twiddle<INV>(a, w1);
  }
}

// The sparse first pass of the chain: no barrier is needed before the stores -- as long as the buffer itself is
// free.  Ends with a barrier.
template <int LOG2H, int NT, bool INV, class TW>
__device__ __forceinline__ void kwy_fft_pass8_first_sparse_core(kwy_c *z, TW tw, kwy_c a0, kwy_c a1) {
  constexpr int H = 1 << LOG2H, Q = H / 8;
  static_assert(Q <= NT, "one butterfly per thread");
  const int j = kwy_tid_opaque();
  if (j < Q) {
    kwy_c a[8];
    kwy_first8_sparse<INV>(j, tw, a0, a1, a);
#pragma unroll
    for (int m = 0; m < 8; ++m) z[8 * j + (m ^ (j & 7))] = a[m];
  }
  __syncthreads();
}

// The first pass of a kernel that meets both kinds of input (`half`, block-uniform).  The caller has a barrier between
// filling z (z[0 .. H/2] where half) and this call; ends with a barrier.
template <int LOG2H, int NT, bool INV, class TW>
__device__ __forceinline__ void kwy_fft_pass8_first_sel_core(kwy_c *z, TW tw, bool half) {
  constexpr int H = 1 << LOG2H, Q = H / 8;
  static_assert(Q <= NT && Q >= 8, "one butterfly per thread");
  const int j = kwy_tid_opaque();
  kwy_c a[8];
  if (j < Q) kwy_first8_dense<LOG2H, INV>(z, j, tw, half, a);
  __syncthreads();
  if (j < Q) {
#pragma unroll
    for (int m = 0; m < 8; ++m) z[8 * j + (m ^ (j & 7))] = a[m];
  }
  __syncthreads();
}
// ... and of one whose input is always the half kind
template <int LOG2H, int NT, bool INV, class TW>
__device__ __forceinline__ void kwy_fft_pass8_first_half_core(kwy_c *z, TW tw) {
  kwy_fft_pass8_first_sel_core<LOG2H, NT, INV>(z, tw, true);
}

// closing radix-4 (TAIL = 2) or radix-2 (TAIL = 1) pass: sub-transform stride H/4 resp. H/2, no twiddles
template <int LOG2H, int TAIL, int NT, bool INV>
__device__ __forceinline__ void kwy_fft_tail(kwy_c *z) {
  constexpr int H = 1 << LOG2H, R = 1 << TAIL, Q = H / R;
  constexpr int IT = (Q + NT - 1) / NT;
  kwy_c a[IT][R];
  const int tid = kwy_tid_opaque();
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int j = tid + it * NT;
    if (j < Q) {
#pragma unroll
      for (int m = 0; m < R; ++m) a[it][m] = z[j + m * Q];
      if constexpr (TAIL == 2) {
        kwy_dft4<INV>(a[it]);
      } else {
        kwy_c s0 = cadd(a[it][0], a[it][1]), s1 = csub(a[it][0], a[it][1]);
        a[it][0] = s0; a[it][1] = s1;
      }
      // the closing pass writes exactly the locations it read: no barrier in between
#pragma unroll
      for (int m = 0; m < R; ++m) z[j + m * Q] = a[it][m];
    }
  }
  __syncthreads();
}

// the remaining passes after a first pass of the table-driven chain
template <int LOG2H, int NT, bool INV>
__device__ inline void kwy_fft_inplace_rest(kwy_c *z, const kwy_c *__restrict__ tw, const kwy_c *__restrict__ pw) {
  kwy_fft_pass8<LOG2H, 3, NT, INV>(z, tw);
  kwy_fft_pass8_s64<LOG2H, NT, INV>(z, pw);
  if constexpr (LOG2H == 12) kwy_fft_pass8<LOG2H, 9, NT, INV>(z, tw);
  if constexpr (LOG2H == 11) kwy_fft_tail<LOG2H, 2, NT, INV>(z);
  if constexpr (LOG2H == 10) kwy_fft_tail<LOG2H, 1, NT, INV>(z);
}

// In-place complex FFT of H = 2^LOG2H (512 .. 4096) points in LDS.  The caller
// has a barrier between filling z and this call; ends with a barrier.
// tw: exp(-2 pi i k / H), k < H/8 (global or LDS); pw: the powers table of the stride-64 pass (global; unused below
// H = 1024).  Unnormalised in both directions.
template <int LOG2H, int NT, bool INV>
__device__ inline void kwy_fft_inplace(kwy_c *z, const kwy_c *__restrict__ tw, const kwy_c *__restrict__ pw) {
  static_assert(LOG2H >= 8 && LOG2H <= 12, "unsupported in-place FFT length");
  kwy_fft_pass8<LOG2H, 0, NT, INV>(z, tw);
  kwy_fft_pass8<LOG2H, 3, NT, INV>(z, tw);
  if constexpr (LOG2H >= 9) kwy_fft_pass8_s64<LOG2H, NT, INV>(z, pw);
  if constexpr (LOG2H == 12) kwy_fft_pass8<LOG2H, 9, NT, INV>(z, tw);
  if constexpr (LOG2H % 3 != 0) kwy_fft_tail<LOG2H, LOG2H % 3, NT, INV>(z);
}

// The same transform with the pass factors held by the threads: when a pass has one butterfly
// per thread (H/8 <= NT), the factor of pass p is the thread constant
// w[p] = exp(-2 pi i ((tid >> 3p) << 3p) / H)  -- no table at all (kwy_fft_thread_twiddles).  The stride-64 pass
// (p = 2) is the exception: its factors are wave-uniform and come from the powers table, w[2] is not fetched.
template <int LOG2H, int NT>
__device__ __forceinline__ void kwy_fft_thread_twiddles(const kwy_c *__restrict__ twH, kwy_c (&w)[4]) {
  static_assert((1 << LOG2H) / 8 <= NT, "one butterfly per thread and pass");
  const int j = threadIdx.x;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int ps = (j >> (3 * p)) << (3 * p);
    w[p] = (p != 2 && 3 * p + 3 < LOG2H + 0 && ps < (1 << LOG2H) / 8) ? twH[ps] : kwy_c{1.0, 0.0};
  }
}
// TAIL = false: stop in front of the closing radix-4 / radix-2 pass (the caller runs kwy_fft_tail4_drain instead)
template <int LOG2H, int NT, bool INV, bool TAIL = true>
__device__ inline void kwy_fft_inplace_rest_w(kwy_c *z, const kwy_c (&w)[4], const kwy_c *__restrict__ pw) {
  kwy_fft_pass8_core<LOG2H, 3, NT, INV>(z, kwy_tw_reg{w[1]});
  if constexpr (LOG2H >= 9) kwy_fft_pass8_s64<LOG2H, NT, INV>(z, pw);
  if constexpr (LOG2H == 12) kwy_fft_pass8_core<LOG2H, 9, NT, INV>(z, kwy_tw_reg{w[3]});
  if constexpr (TAIL && LOG2H % 3 != 0) kwy_fft_tail<LOG2H, LOG2H % 3, NT, INV>(z);
}
template <int LOG2H, int NT, bool INV, bool TAIL = true>
__device__ inline void kwy_fft_inplace_w(kwy_c *z, const kwy_c (&w)[4], const kwy_c *__restrict__ pw) {
  static_assert(LOG2H >= 8 && LOG2H <= 12, "unsupported in-place FFT length");
  kwy_fft_pass8_core<LOG2H, 0, NT, INV>(z, kwy_tw_reg{w[0]});
  kwy_fft_inplace_rest_w<LOG2H, NT, INV, TAIL>(z, w, pw);
}
// The same transform for a kernel whose input may be zero from z[H/2 + 1] on: where `half` (block-uniform) says so, the
// caller has filled z[0 .. H/2] -- point H/2 itself too, with its value or zero, whatever the buffer held before -- and
// nothing above is read; the first pass stores all H points, and the bins are those of kwy_fft_inplace_w on the
// zero-padded input (a zero may come out with the other sign).  Only the first pass's loads and butterfly branch;
// half = false is kwy_fft_inplace_w.
template <int LOG2H, int NT, bool INV, bool TAIL = true>
__device__ inline void kwy_fft_inplace_sel_w(kwy_c *z, const kwy_c (&w)[4], const kwy_c *__restrict__ pw, bool half) {
  static_assert(LOG2H >= 9 && LOG2H <= 12, "unsupported in-place FFT length");
  kwy_fft_pass8_first_sel_core<LOG2H, NT, INV>(z, kwy_tw_reg{w[0]}, half);
  kwy_fft_inplace_rest_w<LOG2H, NT, INV, TAIL>(z, w, pw);
}

// exp(-2 pi i (t + r*NT) / N) from base = exp(-2 pi i t / N): base times a 16th root of unity,
// idx16 = r * 16 NT / N.  Even indices go through the exact 8th-root form.
__device__ __forceinline__ kwy_c kwy_tw_hex(kwy_c b, int idx16) {
  if (!(idx16 & 1)) return kwy_tw_octant(b, idx16 >> 1);
  const double c1 = 0.92387953251128675613, s1 = 0.38268343236508977173;  // cos, sin of pi/8
  double wr, wi;  // exp(-i pi idx16 / 8)
  switch (idx16 & 15) {
    case 1: wr = c1; wi = -s1; break;
    case 3: wr = s1; wi = -c1; break;
    case 5: wr = -s1; wi = -c1; break;
    case 7: wr = -c1; wi = -s1; break;
    case 9: wr = -c1; wi = s1; break;
    case 11: wr = -s1; wi = c1; break;
    case 13: wr = s1; wi = c1; break;
    default: wr = c1; wi = s1; break;
  }
  return {__builtin_fma(b.x, wr, -(b.y * wi)), __builtin_fma(b.x, wi, b.y * wr)};
}

// ------------------------------------------------- real transforms around it, in place in a buffer of H+1 complex
// A thread combines "its" pairs (k, H - k), k = tid + NT r <= H/2 -- both results come from the same two packed values
// A = Z[k], Bc = Z[H - k] -- so no barrier separates a split's loads from its stores.  w = exp(-2 pi i k / N), N = 2H.
// The arithmetic of a pair stands here once per direction; the loops over a thread's pairs stay with their callers
// (kwy_rfft_inplace / kwy_syn_rsplit, kwy_irfft_inplace / syn_irfft_inplace of kwy_synth.hip): moved into one routine
// they compute the same, but the compiler lays the blocks of some thirty kernels out differently.
// forward: X[k] = E + O w,  X[H-k] = conj(E - O w)  with E = (A + conj B)/2, O = (A - conj B)/(2i)
__device__ __forceinline__ void kwy_rsplit_pair(kwy_c A, kwy_c Bc, kwy_c w, kwy_c &xk, kwy_c &xm) {
  const double er = 0.5 * (A.x + Bc.x), ei = 0.5 * (A.y - Bc.y);
  const double dr = 0.5 * (A.x - Bc.x), di = 0.5 * (A.y + Bc.y);
  const double orr = di, oi = -dr;
  const double pr = __builtin_fma(orr, w.x, -(oi * w.y)), pi = __builtin_fma(orr, w.y, oi * w.x);
  xk = {er + pr, ei + pi};
  xm = {er - pr, -(ei - pi)};
}
// inverse (w is conjugated here): b[k]: (a, conj b) = (A, conj Bc);  b[H-k]: (Bc, conj A), twiddle -conj(w)
__device__ __forceinline__ void kwy_irsplit_pair(kwy_c A, kwy_c Bc, kwy_c w, kwy_c &bk, kwy_c &bm) {
  const double er = A.x + Bc.x, ei = A.y - Bc.y;
  const double dr = A.x - Bc.x, di = A.y + Bc.y;
  const double wr = w.x, wi = -w.y;
  const double orr = __builtin_fma(dr, wr, -(di * wi)), oi = __builtin_fma(dr, wi, di * wr);
  bk = {er - oi, ei + orr};
  bm = {er + oi, -(ei - orr)};
}

// kwy_rfft_inplace: z holds N = 2H reals (viewed as H packed complex); on return z[0..H] are the
// bins X[0..H].  twb = exp(-2 pi i tid / N):
// for NT >= N/8 the pair twiddles are twb times 8th roots of unity, else they are read from twN[].
// Ends with a barrier.
template <int LOG2H, int NT>
__device__ inline void kwy_rfft_inplace(kwy_c *z, const kwy_c *__restrict__ tw, const kwy_c *__restrict__ pw, kwy_c twb,
                                   const kwy_c *__restrict__ twN = nullptr) {
  constexpr int H = 1 << LOG2H, N = 2 * H;
  constexpr int OCT = 8 * NT / N;  // 0: the workgroup is narrower than N/8, pair twiddles come from twN[]
  kwy_fft_inplace<LOG2H, NT, false>(z, tw, pw);
  const int tid = kwy_tid_opaque();
#pragma unroll
  for (int r = 0; r * NT <= H / 2; ++r) {
    const int k = tid + NT * r;
    if (k > H / 2) continue;
    if (k == 0) {
      const kwy_c z0 = z[0];
      z[0] = {z0.x + z0.y, 0.0};
      z[H] = {z0.x - z0.y, 0.0};
    } else {
      const kwy_c w = (OCT >= 1) ? kwy_tw_octant(twb, OCT * r) : twN[k];
      kwy_c xk, xm;
      kwy_rsplit_pair(z[k], z[H - k], w, xk, xm);
      z[k] = xk;
      if (k != H - k) z[H - k] = xm;
    }
  }
  __syncthreads();
}

// kwy_irfft_inplace: z[0..H] holds X; on return the first N doubles of z are the signal times N
// (unnormalised: N times the true inverse).  Opens with a barrier of its own, ends with a barrier.
template <int LOG2H, int NT>
__device__ inline void kwy_irfft_inplace(kwy_c *z, const kwy_c *__restrict__ tw, const kwy_c *__restrict__ pw, kwy_c twb,
                                   const kwy_c *__restrict__ twN = nullptr) {
  constexpr int H = 1 << LOG2H, N = 2 * H;
  constexpr int OCT = 8 * NT / N;  // 0: the workgroup is narrower than N/8, pair twiddles come from twN[]
  const int tid = kwy_tid_opaque();
  __syncthreads();
#pragma unroll
  for (int r = 0; r * NT <= H / 2; ++r) {
    const int k = tid + NT * r;
    if (k > H / 2) continue;
    if (k == 0) {
      // b[0] from a[0], a[H] (imaginary parts of the DC and Nyquist bins ignored)
      const double ar = z[0].x, br = z[H].x;
      z[0] = {ar + br, ar - br};
    } else {
      const kwy_c w = (OCT >= 1) ? kwy_tw_octant(twb, OCT * r) : twN[k];
      kwy_c bk, bm;
      kwy_irsplit_pair(z[k], z[H - k], w, bk, bm);
      z[k] = bk;
      if (k != H - k) z[H - k] = bm;
    }
  }
  __syncthreads();
  kwy_fft_inplace<LOG2H, NT, true>(z, tw, pw);
}

// ---- the real split of the synthesis pulse kernel (k_syn_pulse) and the cepstrum fold behind it
// The kernel runs NT threads that each stand for the V "virtual" threads t + NT g of a 256-thread workgroup.  Pair
// twiddles: exp(-2 pi i k / N) for k = t + NT r as base[r % V] times an 8th root of unity,
// base[g] = exp(-2 pi i (t + NT g) / N); the long transforms (NT V < N/8) read them from twN[k].
template <int LOG2H, int NT, int V>
__device__ __forceinline__ kwy_c syn_pair_twiddle(const kwy_c (&base)[V], const kwy_c *__restrict__ twN, int k, int r) {
  constexpr int N = 2 << LOG2H;
  constexpr int OCT = 8 * (NT * V) / N;
  if constexpr (OCT < 1) return twN[k];
  else return kwy_tw_octant(base[r % V], OCT * (r / V));
}

// the packed half-length transform in z -> the bins X[0 .. H] in z[0 .. H] (as kwy_rfft_inplace).  Ends with a barrier.
template <int LOG2H, int NT, int V>
__device__ __forceinline__ void kwy_syn_rsplit(kwy_c *z, const kwy_c (&base)[V], const kwy_c *__restrict__ twN) {
  constexpr int H = 1 << LOG2H;
  const int tid = kwy_tid_opaque();
#pragma unroll
  for (int r = 0; r * NT <= H / 2; ++r) {
    const int k = tid + NT * r;
    if (k > H / 2) continue;
    if (k == 0) {
      const kwy_c z0 = z[0];
      z[0] = {z0.x + z0.y, 0.0};
      z[H] = {z0.x - z0.y, 0.0};
    } else {
      const kwy_c w = syn_pair_twiddle<LOG2H, NT, V>(base, twN, k, r);
      kwy_c xk, xm;
      kwy_rsplit_pair(z[k], z[H - k], w, xk, xm);
      z[k] = xk;
      if (k != H - k) z[H - k] = xm;
    }
  }
  __syncthreads();
}

// The causal fold of the cepstrum whose bins kwy_syn_rsplit left in z (a real, even log-spectrum went in, so only the
// real parts count): c[0], 2 c[1 .. H-1], c[H] as packed reals over the complex bins they came from; ZEROS: and
// zeros up to sample N - 1, for a dense first pass behind it.  The caller has a barrier in front; ends with a barrier.
template <int LOG2H, int NT, bool ZEROS>
__device__ __forceinline__ void kwy_syn_fold(kwy_c *z) {
  constexpr int H = 1 << LOG2H, N = 2 * H, RK = (H + 1 + NT - 1) / NT;
  double *L = (double *)z;
  const int tid = kwy_tid_opaque();
  double cv[RK];
#pragma unroll
  for (int r = 0; r < RK; ++r) {
    const int n = tid + NT * r;
    double v = 0.0;
    if (n <= H) {
      v = z[n].x;
      if (n >= 1 && n < H) v *= 2.0;
    }
    cv[r] = v;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RK; ++r) {
    const int n = tid + NT * r;
    if (n <= H) L[n] = cv[r];
  }
  if constexpr (ZEROS) {
    for (int n = H + 1 + tid; n < N; n += NT) L[n] = 0.0;
  }
  __syncthreads();
}

// kwy_syn_rsplit and kwy_syn_fold<.., false> in one: the split forms only the real parts of its pairs (k, H - k), by
// the same expressions, keeps them in registers with the fold's factor 2, and writes the folded cepstrum behind ONE
// barrier -- no imaginary parts, no store of the bins and no second read.  (A computation of its own, not kwy_rsplit_pair:
// the imaginary parts are never formed.)  ZEROS as for kwy_syn_fold.  Ends with a barrier.
template <int LOG2H, int NT, int V, bool ZEROS>
__device__ __forceinline__ void kwy_syn_rsplit_fold(kwy_c *z, const kwy_c (&base)[V], const kwy_c *__restrict__ twN) {
  constexpr int H = 1 << LOG2H, N = 2 * H, R = H / 2 / NT + 1;
  double *L = (double *)z;
  const int tid = kwy_tid_opaque();
  double lo[R], hi[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = tid + NT * r;
    lo[r] = hi[r] = 0.0;
    if (k > H / 2) continue;
    if (k == 0) {
      const kwy_c z0 = z[0];
      lo[r] = z0.x + z0.y;
      hi[r] = z0.x - z0.y;
    } else {
      const kwy_c w = syn_pair_twiddle<LOG2H, NT, V>(base, twN, k, r);
      const kwy_c A = z[k], Bc = z[H - k];
      const double er = 0.5 * (A.x + Bc.x);
      const double dr = 0.5 * (A.x - Bc.x), di = 0.5 * (A.y + Bc.y);
      const double orr = di, oi = -dr;
      const double pr = __builtin_fma(orr, w.x, -(oi * w.y));
      double a = er + pr, b = er - pr;
      a *= 2.0;
      b *= 2.0;
      lo[r] = a;
      hi[r] = b;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = tid + NT * r;
    if (k > H / 2) continue;
    L[k] = lo[r];
    if (k != H - k) L[H - k] = hi[r];
  }
  if constexpr (ZEROS) {
    for (int n = H + 1 + tid; n < N; n += NT) L[n] = 0.0;
  }
  __syncthreads();
}

// ---- single bins and powers from the packed half-length transform Z of N = 2H reals, times TWO: the four halvings of
// the even / odd split are left out.  For consumers that only form ratios of quadratic expressions of the bins --
// D4C's centroid over power spectrum, band energy ratios, LoveTrain's cumulative power ratio -- the factor cancels
// exactly (a power of two), and every bin saves four multiplications.  The _v / _dc forms take the packed points
// A = Z[k], Bz = Z[H - k] themselves (from LDS or from a drained tail's registers), the _w forms load them from z
// (read-only).  w = exp(-2 pi i k / N).
// 2 X[k], k != 0, H: (er, ei) + (di, -dr) w, as two fused multiply-adds per component (see cmulf)
__device__ __forceinline__ kwy_c kwy_rfft_bin2_v(kwy_c A, kwy_c Bz, kwy_c w) {
  const kwy_c B = {Bz.x, -Bz.y};
  const double er = A.x + B.x, ei = A.y + B.y;
  const double dr = A.x - B.x, di = A.y - B.y;
  return {__builtin_fma(dr, w.y, __builtin_fma(di, w.x, er)), __builtin_fma(-dr, w.x, __builtin_fma(di, w.y, ei))};
}
// 2 X[k], 0 <= k <= H
template <int LOG2H>
__device__ __forceinline__ kwy_c kwy_rfft_bin2_w(const kwy_c *z, int k, kwy_c w) {
  constexpr int H = 1 << LOG2H;
  if (k == 0) return {2.0 * (z[0].x + z[0].y), 0.0};
  if (k == H) return {2.0 * (z[0].x - z[0].y), 0.0};
  return kwy_rfft_bin2_v(z[k], z[H - k], w);
}
// |2 X[k]|^2 and |2 X[H - k]|^2 together (k != 0): the two bins are E + O w and conj(E - O w) of the same two packed
// points -- one pair of operands, one twiddle and one complex product for two powers
__device__ __forceinline__ void kwy_rfft_pair_power2_v(kwy_c A, kwy_c Bz, kwy_c w, double *pk, double *pm) {
  const double er = A.x + Bz.x, ei = A.y - Bz.y;
  const double dr = A.x - Bz.x, di = A.y + Bz.y;
  const double pr = __builtin_fma(dr, w.y, di * w.x), pi = __builtin_fma(-dr, w.x, di * w.y);
  const double xr = er + pr, xi = ei + pi, yr = er - pr, yi = ei - pi;
  *pk = __builtin_fma(xr, xr, xi * xi);
  *pm = __builtin_fma(yr, yr, yi * yi);
}
// ... and its k = 0 case (DC and Nyquist) on Z[0]
__device__ __forceinline__ void kwy_rfft_pair_power2_dc(kwy_c Z0, double *pk, double *pm) {
  const double a = 2.0 * (Z0.x + Z0.y), b = 2.0 * (Z0.x - Z0.y);
  *pk = a * a; *pm = b * b;
}
// the pair of powers of bins k and H - k, 0 <= k <= H/2
template <int LOG2H>
__device__ __forceinline__ void kwy_rfft_pair_power2_w(const kwy_c *z, int k, kwy_c w, double *pk, double *pm) {
  constexpr int H = 1 << LOG2H;
  if (k == 0) kwy_rfft_pair_power2_dc(z[0], pk, pm);
  else kwy_rfft_pair_power2_v(z[k], z[H - k], w, pk, pm);
}

// ------------------------------------------------------- the closing radix-4 pass drained into registers
// kwy_fft_tail stores the whole transform only for the consumer to read bins k and H - k back: a whole-buffer store
// (the slow direction of the LDS), a whole-buffer read and a barrier per transform.  Here thread t runs the two
// radix-4 butterflies whose eight outputs ARE four such pairs, and hands them over in registers.  With Q = H/4
// butterflies and NT = Q/2 threads:
//   t >= 1: butterflies j = t and j = Q - t      -> pairs (k, H - k) for k = t, Q + t, Q - t, 2Q - t
//   t == 0: butterflies j = 0 and j = Q/2        -> k = 0 (X[0] twice: DC / Nyquist), Q, Q/2, 3Q/2, and the
//                                                    self-paired X[H/2] in `mid` (every thread gets its X[2Q + t])
// Slot s of thread t holds lo[s] = X[k], hi[s] = X[H - k] with k = kwy_drain_bin(s, t); every k in [0, H/2) belongs
// to exactly one (t, s).  W^k = exp(-2 pi i k / 2H) of a slot is kwy_drain_tw(): the expression kwy_tw_hex(twN[k mod
// NT], HEX (k div NT)) that the k = tid + NT q mapping forms, so that the bits of every bin stay what they were.
// Reads z only; the caller has a barrier in front (the last radix-8 pass ends with one) and puts one behind before
// anything is stored to z.
// (first the two butterflies and the hand-over on operands already in registers -- a: butterfly j = t, b: butterfly
// j = Q - t resp. Q/2 -- which the loads of the natural order and those of the wave-local layout below share)
template <bool INV>
__device__ __forceinline__ void kwy_tail4_drain_pairs(kwy_c (&a)[4], kwy_c (&b)[4], bool t0, kwy_c (&lo)[4],
                                                      kwy_c (&hi)[4], kwy_c &mid) {
  kwy_dft4<INV>(a);
  kwy_dft4<INV>(b);
  lo[0] = a[0]; hi[0] = t0 ? a[0] : b[3];
  lo[1] = a[1]; hi[1] = t0 ? a[3] : b[2];
  lo[2] = b[0]; hi[2] = t0 ? b[3] : a[3];
  lo[3] = b[1]; hi[3] = t0 ? b[2] : a[2];
  mid = a[2];
}
template <int LOG2H, int NT, bool INV>
__device__ __forceinline__ void kwy_fft_tail4_drain(const kwy_c *z, kwy_c (&lo)[4], kwy_c (&hi)[4], kwy_c &mid) {
  constexpr int H = 1 << LOG2H, Q = H / 4;
  static_assert(LOG2H % 3 == 2 && NT == Q / 2, "radix-4 tail, two butterflies per thread");
  const int t = kwy_tid_opaque();
  const int jb = t ? Q - t : Q / 2;
  kwy_c a[4], b[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) { a[m] = z[t + m * Q]; b[m] = z[jb + m * Q]; }
  kwy_tail4_drain_pairs<INV>(a, b, t == 0, lo, hi, mid);
}
// the bin k of slot s (see above); Q = H/4
template <int LOG2H>
__device__ __forceinline__ int kwy_drain_bin(int s, int t) {
  constexpr int Q = (1 << LOG2H) / 4;
  switch (s) {
    case 0: return t;
    case 1: return Q + t;
    case 2: return t ? Q - t : Q / 2;
    default: return t ? 2 * Q - t : Q + Q / 2;
  }
}
// exp(-2 pi i k / 2H) for k = kwy_drain_bin(s, t); twa = twN[t], twc = twN[(NT - t) & (NT - 1)] (twN: exp(-2 pi i k / 2H))
template <int LOG2H, int NT>
__device__ __forceinline__ kwy_c kwy_drain_tw(int s, kwy_c twa, kwy_c twc) {
  constexpr int HEX = 16 * NT / (2 << LOG2H);
  static_assert(HEX >= 1, "workgroup narrower than N/16");
  switch (s) {
    case 0: return kwy_tw_hex(twa, 0);
    case 1: return kwy_tw_hex(twa, 2 * HEX);
    case 2: return kwy_tw_hex(twc, HEX);
    default: return kwy_tw_hex(twc, 3 * HEX);
  }
}

// ------------------------------------------------------- the 2048-point transform with two wave-local passes
// (H = 2048 on 256 threads: the 4096-point D4C frames.)  The Stockham chain above permutes the buffer in every pass, so
// each pass has a workgroup barrier between its loads and its stores and one behind its stores: six per transform in
// front of the drained closing pass.  The data flow needs two.  Call a point of the transform after the first pass
// (s, n): s = 0..7 the sub-transform (the output residue mod 8), n = 0..255 the first-pass butterfly that made it, and
// let every later butterfly store its results to the eight places it read (decimation in frequency, in place):
//   first pass    thread j reads x[j + 256 m] (natural order, as the callers fill it), stores result m as (m, j)
//   stride 8      butterfly (s, j1), j1 = 0..31: points n = j1 + 32 m, m = 0..7; factor twH[8 j1]; result m1 back to
//                 (s, j1 + 32 m1), which is point s + 8 m1 + 64 j1 of the Stockham order
//   stride 64     butterfly (s, m1, j2), j2 = 0..3: points n = j2 + 4 m + 32 m1, m = 0..7; factors: entry j2 of the
//                 powers table; result m2 back to (s, j2 + 4 m2 + 32 m1): Stockham point s + 8 m1 + 64 m2 + 512 j2
//   radix-4 tail  butterfly j = s + 8 m1 + 64 m2: points n = j2 + 4 m2 + 32 m1, j2 = 0..3 -> X[j + 512 m3]
// Wavefront w runs the stride-8 butterflies with j1 mod 4 = w and the stride-64 butterflies with j2 = w: both touch
// exactly the points with n mod 4 = w, so the stride-64 pass reads what its own wavefront wrote, and between the two
// the wavefront only waits for its own stores (the LDS executes one wavefront's instructions in order; all 64 lanes
// are live).  Two exchanges cross wavefronts -- first pass to stride-8 pass, stride-64 pass to tail -- and those are
// the transform's two workgroup barriers.  Same butterflies on the same operands with the same factors as the chain
// above, formed by the same routines: only which thread runs a butterfly and where its points lie differ, so every
// bin keeps its bits.
// Layout: (s, n) lies at 256 s + (n ^ sw(s) ^ (((n >> 5) & 1) << 3)), sw(s) = s ^ ((s & 4) << 1).  A 16-byte load is
// served in four groups of 16 lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- over the sixteen
// 16-byte slots of a 256-byte row, a 16-byte store in eight groups of 8 consecutive lanes over eight slots.  A lane is
// (s, h) = (t & 7, (t >> 3) & 7), and the points of one access of either wave-local pass or of the tail differ in s and
// h only, n carrying h in its bits 2..4 (stride 8) or 5..7 (stride 64, tail): a load group holds the lanes with equal
// h2 and equal s2 ^ h0 ^ h1, so s has to reach slot bits 0..2 (which also spreads the eight s of a store group), s2 slot
// bit 3 as well, and n5 slot bit 3.  Counted over those groups, every load and store of the transform is free of
// conflicts except the tail's second butterfly (j = 512 - t), at 16 extra LDS cycles per transform.  The place differs
// from the natural one, n + 256 s, in bits 0..3 only: the first pass's stores land in the 64 columns its own wavefront
// read, so the write-after-read hazard stays inside the wavefront and that pass needs no barrier between its loads and
// its stores either.
// orders a wavefront's LDS loads behind its own LDS stores: kwy_lds_barrier() without the rendezvous
__device__ __forceinline__ void kwy_lds_wave_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// the thread's factors: w[0] = twH[t] for the first pass, w[1] = twH[8 j1] of its stride-8 butterfly (t: the thread
// index, opaque where the fetch is to stay at its use)
__device__ __forceinline__ void kwy_fftwl_thread_twiddles(const kwy_c *__restrict__ twH, int t, kwy_c (&w)[4]) {
  w[0] = twH[t];
  w[1] = twH[32 * ((t >> 3) & 7) + 8 * ((t >> 6) & 3)];
  w[2] = w[3] = kwy_c{1.0, 0.0};
}
// first-pass stores: result m of thread j to (m, j)
__device__ __forceinline__ void kwy_fftwl_store_first(kwy_c *z, int j, const kwy_c (&a)[8]) {
  const int c = j ^ (((j >> 5) & 1) << 3);
#pragma unroll
  for (int m = 0; m < 8; ++m) z[256 * m + (c ^ (m ^ ((m & 4) << 1)))] = a[m];
}
// First pass, dense or (block-uniform `half`) half input: kwy_first8_dense, stored in this layout with no barrier in
// between (see above).  The caller has a barrier between filling z and this call; ends with a barrier.
template <bool INV>
__device__ __forceinline__ void kwy_fftwl_first_sel(kwy_c *z, kwy_tw_reg tw, bool half) {
  const int j = kwy_tid_opaque();
  kwy_c a[8];
  kwy_first8_dense<11, INV>(z, j, tw, half, a);
  kwy_fftwl_store_first(z, j, a);
  __syncthreads();
}
// First pass of an input that is zero except for x[0 .. 256]: kwy_first8_sparse in this layout (nothing is read, the
// buffer itself must be free).  Ends with a barrier.
// (k_d4c_bands, the kernel with this kind of input, keeps the chain -- kwy_d4c.hip; the self-test holds this to its bits.)
template <bool INV>
__device__ __forceinline__ void kwy_fftwl_first_sparse(kwy_c *z, kwy_tw_reg tw, kwy_c a0, kwy_c a1) {
  const int j = kwy_tid_opaque();
  kwy_c a[8];
  kwy_first8_sparse<INV>(j, tw, a0, a1, a);
  kwy_fftwl_store_first(z, j, a);
  __syncthreads();
}
// The two wave-local passes behind a first pass; ends with a barrier, in front of the drained tail.
// w1: twH[8 j1] of this thread (kwy_fftwl_thread_twiddles); pw: the powers table.
template <bool INV>
__device__ __forceinline__ void kwy_fftwl_rest(kwy_c *z, kwy_tw_reg tw1, const kwy_c *__restrict__ pw) {
  const int t = kwy_tid_opaque();
  const int s = t & 7, hi3 = (t >> 3) & 7, wv = (t >> 6) & 3;
  const int sw = s ^ ((s & 4) << 1);
  kwy_c a[8];
  {   // stride 8: butterfly (s, j1 = 4 hi3 + wv), points n = j1 + 32 m at 256 s + 32 m + (j1 ^ sw ^ ((m & 1) << 3))
    const int c = 256 * s + ((4 * hi3 + wv) ^ sw);
    const int at[2] = {c, c ^ 8};
#pragma unroll
    for (int m = 0; m < 8; ++m) a[m] = z[at[m & 1] + 32 * m];
    kwy_dft8<INV>(a);
    kwy_dft8_twiddle<INV>(a, tw1(0));
#pragma unroll
    for (int m = 0; m < 8; ++m) z[at[m & 1] + 32 * m] = a[m];
  }
  kwy_lds_wave_fence();
  {   // stride 64: butterfly (s, m1 = hi3, j2 = wv), points n = wv + 4 m + 32 m1 at
      // 256 s + 32 m1 + ((wv + 4 m) ^ k), k = sw ^ ((m1 & 1) << 3)
    const int k = sw ^ ((hi3 & 1) << 3);
    const int c = 256 * s + 32 * hi3 + (wv ^ (k & 3));
    int at[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) at[q] = c + 4 * (q ^ (k >> 2));
#pragma unroll
    for (int m = 0; m < 8; ++m) a[m] = z[at[m & 3] + 4 * (m & 4)];
    kwy_dft8<INV>(a);
    const kwy_c *__restrict__ pe = pw + KWY_TWP_ENTRY * __builtin_amdgcn_readfirstlane(t >> 6);
#pragma unroll
    for (int m = 1; m < 8; ++m) {
      kwy_c w = pe[m];
      if (INV) w.y = -w.y;
      a[m] = cmulf(w, a[m]);
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) z[at[m & 3] + 4 * (m & 4)] = a[m];
  }
  __syncthreads();
}
// the place of operand j2 of the tail's butterfly j = s + 8 m1 + 64 m2, j < 512
__device__ __forceinline__ int kwy_fftwl_tail_at(int j, int j2) {
  const int s = j & 7, m1 = (j >> 3) & 7, m2 = (j >> 6) & 7;
  const int k = s ^ ((s & 4) << 1) ^ ((m1 & 1) << 3);
  return 256 * s + 32 * m1 + ((4 * m2) ^ (k & 12)) + (j2 ^ (k & 3));
}
// kwy_fft_tail4_drain<11, 256, INV> on this layout: the same butterflies, pairs and slots
template <bool INV>
__device__ __forceinline__ void kwy_fftwl_tail4_drain(const kwy_c *z, kwy_c (&lo)[4], kwy_c (&hi)[4], kwy_c &mid) {
  constexpr int Q = 512;
  const int t = kwy_tid_opaque();
  const int jb = t ? Q - t : Q / 2;
  kwy_c a[4], b[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) { a[m] = z[kwy_fftwl_tail_at(t, m)]; b[m] = z[kwy_fftwl_tail_at(jb, m)]; }
  kwy_tail4_drain_pairs<INV>(a, b, t == 0, lo, hi, mid);
}
