// kwy_device.hpp -- device-side building blocks shared by the gfx950 kernels:
//   * WORLD's xorshift128 "randn" stream with GF(2) jump-ahead, so that every
//     frame / pulse draws exactly the numbers the serial CPU algorithm would
//   * block-wide f64 reductions and scans (64-wide wavefronts)
//   * fdlibm forms of log and sincos, the block-wide "sum of the m smallest" select
//   * the small routines that several kernels must compute bit for bit alike (band codec, delta windows, row placement)
// The LDS-resident FFTs live in kwy_fft.hpp, which includes this file.
// Written for CDNA4 only (wave64, 160 KB LDS); no portability layer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define KWY_THREADS 256
#define KWY_WAVES (KWY_THREADS / 64)
#define KWY_PI 3.1415926535897932384
#define KWY_SAFE 0.000000000001                    // WORLD's safe guard (world/constantnumbers.h)
#define KWY_DBL_MAX 1.79769313486231570815e+308
static_assert(1.0 - KWY_SAFE == 1.0 - 1e-12, "the two spellings of the safe guard are one double");

// ---------------------------------------------------------------- xorshift128
struct kwy_rng {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ void kwy_rng_seed(kwy_rng &r) {
  r.x = 123456789u; r.y = 362436069u; r.z = 521288629u; r.w = 88675123u;
}

__device__ __forceinline__ uint32_t kwy_rng_step(kwy_rng &r) {
  uint32_t t = r.x ^ (r.x << 11);
  r.x = r.y; r.y = r.z; r.z = r.w;
  r.w = (r.w ^ (r.w >> 19)) ^ (t ^ (t >> 8));
  return r.w;
}

// one "randn" = 12 generator steps (sum of 12 uniforms, WORLD matlabfunctions);
// the raw integer sum keeps a draw in one register, randn = raw / 2^28 - 6
__device__ __forceinline__ uint32_t kwy_rng_randn_raw(kwy_rng &r) {
  uint32_t tmp = kwy_rng_step(r) >> 4;
#pragma unroll
  for (int i = 0; i < 11; ++i) tmp += kwy_rng_step(r) >> 4;
  return tmp;
}
__device__ __forceinline__ double kwy_rng_randn(kwy_rng &r) {
  return kwy_rng_randn_raw(r) / 268435456.0 - 6.0;
}

// XOR over the wavefront, result in every lane: row-local DPP shifts, then the four row totals
// through scalar registers (no LDS round trips).
__device__ __forceinline__ uint32_t kwy_wave_xor_u32(uint32_t v) {
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);  // row_shr:1
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
  v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);  // lane 15 of a row: the row's XOR
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 15) ^ (uint32_t)__builtin_amdgcn_readlane((int)v, 31) ^
         (uint32_t)__builtin_amdgcn_readlane((int)v, 47) ^ (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Wavefront-cooperative jump: all 64 lanes hold the same state s[4]; on return
// every lane holds T^steps s.  pow2: [64][128] columns of T^(2^k) (uint4 each).
__device__ inline void kwy_wave_jump(uint32_t (&s)[4], uint64_t steps, const uint4 *__restrict__ pow2) {
  // (behind an optimisation barrier: this is the cold path beyond the randn table, and the table address of the lane
  // is otherwise formed at the head of the calling kernel and carried -- in k_d4c_body, spilled -- across all of it)
  int lane = threadIdx.x & 63;
  asm volatile("" : "+v"(lane));
  for (int k = 0; steps != 0; ++k, steps >>= 1) {
    if (!(steps & 1)) continue;
    // lane l owns state bits l and l+64 (words l>>5 and 2+(l>>5))
    const uint32_t wlo = lane < 32 ? s[0] : s[1];
    const uint32_t whi = lane < 32 ? s[2] : s[3];
    uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
    uint32_t m = 0u - ((wlo >> (lane & 31)) & 1u);
    uint4 c = pow2[k * 128 + lane];
    o0 ^= c.x & m; o1 ^= c.y & m; o2 ^= c.z & m; o3 ^= c.w & m;
    m = 0u - ((whi >> (lane & 31)) & 1u);
    c = pow2[k * 128 + 64 + lane];
    o0 ^= c.x & m; o1 ^= c.y & m; o2 ^= c.z & m; o3 ^= c.w & m;
    s[0] = kwy_wave_xor_u32(o0); s[1] = kwy_wave_xor_u32(o1);
    s[2] = kwy_wave_xor_u32(o2); s[3] = kwy_wave_xor_u32(o3);
  }
}

// e[0..130]: the extended word sequence of a start state S0 (e0..e3 = x,y,z,w,
// e[4+i] = output of step i+1), so that T^i S0 = (e[i], e[i+1], e[i+2], e[i+3]).
#define KWY_EBASE_WORDS 132
__device__ inline void kwy_rng_ebase(kwy_rng s, uint32_t *e) {
  e[0] = s.x; e[1] = s.y; e[2] = s.z; e[3] = s.w;
  for (int i = 4; i < 131; ++i) e[i] = kwy_rng_step(s);
  e[131] = 0;
}

// state = sum_i c_i T^i S0 with c = coefficients of x^n mod P(x) (P = the
// characteristic polynomial of T); e[] lives in LDS.
__device__ __forceinline__ void kwy_rng_combine_word(kwy_rng &r, const uint32_t *e, uint32_t bits,
                                                      uint32_t &w0, uint32_t &w1, uint32_t &w2) {
#pragma unroll 8
  for (int b = 0; b < 32; ++b) {
    uint32_t w3 = e[b + 3];
    uint32_t m = 0u - ((bits >> b) & 1u);
    r.x ^= w0 & m; r.y ^= w1 & m; r.z ^= w2 & m; r.w ^= w3 & m;
    w0 = w1; w1 = w2; w2 = w3;
  }
}

__device__ __forceinline__ kwy_rng kwy_rng_combine(const uint32_t *e, uint4 c) {
  kwy_rng r = {0, 0, 0, 0};
  uint32_t w0 = e[0], w1 = e[1], w2 = e[2];
  kwy_rng_combine_word(r, e, c.x, w0, w1, w2);
  kwy_rng_combine_word(r, e + 32, c.y, w0, w1, w2);
  kwy_rng_combine_word(r, e + 64, c.z, w0, w1, w2);
  kwy_rng_combine_word(r, e + 96, c.w, w0, w1, w2);
  return r;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for the wave's outstanding GLOBAL stores
// (it is a workgroup-scope fence: s_waitcnt vmcnt(0) before s_barrier) -- a microsecond per barrier in a loop that
// streams results out while it exchanges through LDS.  Use where no thread reads global data another thread of the
// workgroup wrote.
__device__ __forceinline__ void kwy_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---------------------------------------------------------------- the randn stream as a table
// WORLD reseeds its generator at the entry of CheapTrick, D4C and Synthesis, so draw i of the stream is the same
// number in every call, for every utterance: the first `n` raw 12-step sums live in one process-wide table per
// device (kwy_ctx.hip), and a consumer that knows the stream position of its piece loads the draws -- coalesced
// dwords, shared by all streams through the 256 MiB Infinity Cache -- instead of jumping the generator and stepping
// it (which was a quarter of the D4C stage's instructions).  Pieces that reach beyond the table fall back to the
// GF(2) jump-ahead below, inside the consumer (kwy_rng_block_ebase + jump table + 12 steps per draw): same draws.
struct kwy_randn_src {
  const uint32_t *tab;   // raw sums of draws [0, n)
  uint64_t n;
  const uint4 *pow2;     // [64][128] columns of T^(2^k), for the positions beyond the table
};

__device__ __forceinline__ double kwy_randn_from_raw(uint32_t raw) {
  return __builtin_fma((double)raw, 3.7252902984619140625e-09, -6.0);   // raw / 2^28 - 6: the product is exact, so the
                                                                       // fused form rounds like the division
}

// threadIdx.x behind an optimisation barrier: address arithmetic derived from it is redone where it
// is used instead of being computed once per kernel and carried (spilled) across every phase.
__device__ __forceinline__ int kwy_tid_opaque() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// A value every lane holds identically, moved to scalar registers (so that everything
// derived from it is scalar too and stays out of the vector register budget).
__device__ __forceinline__ double kwy_uniform(double v) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The same combination four coefficient bits at a time: for every nibble position g (32 of
// them) and nibble value v the XOR of the <= 4 selected state vectors is tabulated once per
// stream position (512 entries of 16 B, built by the whole workgroup from e[]), after which a
// thread's jump is 32 table reads + XORs instead of 128 select-and-XOR steps.
template <int NT>
__device__ __forceinline__ void kwy_rng_build_table(const uint32_t *e, uint4 *tab) {
  for (int id = threadIdx.x; id < 512; id += NT) {
    const int g = id >> 4, v = id & 15;
    const uint32_t *q = e + 4 * g;
    uint32_t x = 0, y = 0, z = 0, w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t m = 0u - ((v >> b) & 1u);
      x ^= q[b] & m; y ^= q[b + 1] & m; z ^= q[b + 2] & m; w ^= q[b + 3] & m;
    }
    tab[id] = make_uint4(x, y, z, w);
  }
}

__device__ __forceinline__ kwy_rng kwy_rng_combine_table(const uint4 *tab, uint4 c) {
  kwy_rng r = {0, 0, 0, 0};
  const uint32_t cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const uint4 t = tab[(8 * k + n) * 16 + ((cw[k] >> (4 * n)) & 15u)];
      r.x ^= t.x; r.y ^= t.y; r.z ^= t.z; r.w ^= t.w;
    }
  }
  return r;
}

// Fallback beyond the randn table: the extended word sequence e[0..131] (LDS) of the stream position `pos` (in draws),
// made by the workgroup itself -- wavefront 0 jumps the seed state, its lane 0 runs the 127-step recurrence, the
// others wait.  Slow (about 3 k instruction times), which is why the table should cover the utterance.
// Ends with a barrier.
__device__ inline void kwy_rng_block_ebase(uint64_t pos, const uint4 *__restrict__ pow2, uint32_t *e) {
  if (threadIdx.x < 64) {
    uint32_t s[4] = {123456789u, 362436069u, 521288629u, 88675123u};
    kwy_wave_jump(s, 12ull * pos, pow2);
    if (threadIdx.x == 0) {
      kwy_rng r = {s[0], s[1], s[2], s[3]};
      kwy_rng_ebase(r, e);
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------ cos on [-pi, pi]
// (Its Horner steps as explicit fused multiply-adds were measured in round 3 and dropped: half the instructions of the
// polynomial, but the different schedule pushes k_d4c_body and k_syn_pulse, both at their register cap, from 12 / 96
// to 92 / 224 bytes of scratch per lane: k_d4c_body 0.315 -> 0.334 ms.)
// The analysis windows evaluate cos() a few thousand times per frame with arguments that never
// leave [-pi, pi] (up to rounding).  Two-constant Cody-Waite reduction by pi/2 and the fdlibm
// kernel polynomials: < 1 ulp, a quarter of the instructions of the general-range routine.
__device__ __forceinline__ double kwy_cos_pi_range(double x) {
  const double ax = fabs(x);
  const double kf = rint(ax * 6.36619772367581382433e-01);  // 0, 1 or 2 (3 if x is a hair beyond pi... )
  const int k = (int)kf;
  double y = ax - kf * 1.57079632673412561417e+00;
  y = y - kf * 6.07710050650619224932e-11;
  const double z = y * y;
  // sin kernel
  const double rs = 8.33333333332248946124e-03 +
                    z * (-1.98412698298579493134e-04 +
                         z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  const double sn = y + (z * y) * (-1.66666666666666324348e-01 + z * rs);
  // cos kernel
  const double rc = z * (4.16666666666666019037e-02 +
                         z * (-1.38888888888741095749e-03 +
                              z * (2.48015872894767294178e-05 +
                                   z * (-2.75573143513906633035e-07 +
                                        z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const double hz = 0.5 * z, w = 1.0 - hz;
  const double cs = w + (((1.0 - w) - hz) + z * rc);
  // cos(ax) = cos(y + k pi/2)
  const double v = (k & 1) ? sn : cs;
  return ((k + 1) & 2) ? -v : v;
}

// ------------------------------------------------------------------ log, and sincos beyond [-pi, pi]
// The library's log / sincos are 98 / 155 vector instructions a call (extended tables, the Payne-Hanek path for huge
// arguments inline): the kernels that call them once per spectral bin -- CheapTrick's log spectrum, the two half
// log-spectra and the two minimum-phase exponentials of every synthesis pulse -- spend a tenth to a quarter of their
// instructions there.  These are the fdlibm forms (e_log.c; k_sin.c / k_cos.c behind a two-constant fused reduction):
// < 1 ulp for log, < 1.5 ulp for sin / cos with |x| < 2^30 (tests/test_select_gpu.py checks both against numpy).
__device__ __forceinline__ double kwy_log(double x) {
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
               Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
               Lg7 = 1.479819860511658591e-01;
  const bool tiny = x < 2.2250738585072014e-308;            // subnormal (or zero / negative: fixed up below)
  const double xs = tiny ? x * 18014398509481984.0 : x;     // 2^54
  int e;
  double m = frexp(xs, &e);                                  // [0.5, 1)
  e -= tiny ? 54 : 0;
  const bool low = m < 0.70710678118654752440;
  m = low ? m + m : m;
  e -= low ? 1 : 0;
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s, w = z * z;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  const double R = t2 + t1;
  const double hfsq = 0.5 * f * f;
  const double dk = (double)e;
  double r = dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
  r = x == 0.0 ? -INFINITY : r;
  r = (x < 0.0 || x != x) ? NAN : r;
  r = x == INFINITY ? INFINITY : r;
  return r;
}

__device__ __forceinline__ void kwy_sincos_medium(double x, double *sn_out, double *cs_out) {
  const double kf = rint(x * 6.36619772367581382433e-01);    // x / (pi/2)
  double y = __builtin_fma(-kf, 1.57079632679489655800e+00, x);
  y = __builtin_fma(-kf, 6.12323399573676603587e-17, y);
  const int q = (int)kf;
  const double z = y * y;
  const double rs = 8.33333333332248946124e-03 +
                    z * (-1.98412698298579493134e-04 +
                         z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  const double sn = y + (z * y) * (-1.66666666666666324348e-01 + z * rs);
  const double rc = z * (4.16666666666666019037e-02 +
                         z * (-1.38888888888741095749e-03 +
                              z * (2.48015872894767294178e-05 +
                                   z * (-2.75573143513906633035e-07 +
                                        z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const double hz = 0.5 * z, w = 1.0 - hz;
  const double cs = w + (((1.0 - w) - hz) + z * rc);
  // (sin, cos)(y + q pi/2)
  const double s_ = (q & 1) ? cs : sn, c_ = (q & 1) ? sn : cs;
  *sn_out = (q & 2) ? -s_ : s_;
  *cs_out = ((q + 1) & 2) ? -c_ : c_;
}

// sin and cos on [-pi, pi] from the same reduction (the two kernel polynomials are evaluated by the routine above
// anyway).  A window function sampled at i = tid + NT r advances its argument by a constant per r: one call for
// r = 0, then the rotation kwy_rotate() per further element (6 instead of ~40 instructions; the error grows by about
// an ulp per step, 16 steps at most).
__device__ __forceinline__ void kwy_sincos_pi_range(double x, double *sn_out, double *cs_out) {
  const double ax = fabs(x);
  const double kf = rint(ax * 6.36619772367581382433e-01);
  const int k = (int)kf;
  double y = ax - kf * 1.57079632673412561417e+00;
  y = y - kf * 6.07710050650619224932e-11;
  const double z = y * y;
  const double rs = 8.33333333332248946124e-03 +
                    z * (-1.98412698298579493134e-04 +
                         z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  const double sn = y + (z * y) * (-1.66666666666666324348e-01 + z * rs);
  const double rc = z * (4.16666666666666019037e-02 +
                         z * (-1.38888888888741095749e-03 +
                              z * (2.48015872894767294178e-05 +
                                   z * (-2.75573143513906633035e-07 +
                                        z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const double hz = 0.5 * z, w = 1.0 - hz;
  const double cs = w + (((1.0 - w) - hz) + z * rc);
  // (cos, sin)(y + k pi/2)
  const double c = (k & 1) ? sn : cs, s_ = (k & 1) ? cs : sn;
  *cs_out = ((k + 1) & 2) ? -c : c;
  const double sa = (k & 2) ? -s_ : s_;
  *sn_out = x < 0.0 ? -sa : sa;
}

// (c, s) <- the same angle advanced by the angle whose cosine / sine are (cd, sd)
__device__ __forceinline__ void kwy_rotate(double &c, double &s, double cd, double sd) {
  const double c2 = c * cd - s * sd;
  s = s * cd + c * sd;
  c = c2;
}

// ------------------------------------------------------------ block reductions
// Cross-lane moves through the DPP path of the vector ALU (a few cycles) rather than
// ds_bpermute (__shfl_*: an LDS round trip per step, which is what the reductions and scans
// between two barriers used to spend most of their time on).  CTRL: 0x100+n row_shl:n (lane i
// reads lane i+n of its 16-lane row), 0x110+n row_shr:n, 0x142 row_bcast:15, 0x143 row_bcast:31.
// Lanes without a source (row boundary, masked row) read 0.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t kwy_dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, true);
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double kwy_dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double kwy_readlane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// sum over the wavefront; every lane gets the result
__device__ __forceinline__ double kwy_wave_sum(double v) {
  v += kwy_dpp_f64<0x101>(v);
  v += kwy_dpp_f64<0x102>(v);
  v += kwy_dpp_f64<0x104>(v);
  v += kwy_dpp_f64<0x108>(v);  // lane 0 of every row now holds its row's sum
  return (kwy_readlane_f64(v, 0) + kwy_readlane_f64(v, 16)) + (kwy_readlane_f64(v, 32) + kwy_readlane_f64(v, 48));
}

// minimum / maximum over the wavefront (every lane gets the result); lanes without a DPP source keep their own value
template <int CTRL>
__device__ __forceinline__ double kwy_dpp_keep_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double kwy_wave_min_f64(double v) {
  v = fmin(v, kwy_dpp_keep_f64<0x101>(v));
  v = fmin(v, kwy_dpp_keep_f64<0x102>(v));
  v = fmin(v, kwy_dpp_keep_f64<0x104>(v));
  v = fmin(v, kwy_dpp_keep_f64<0x108>(v));  // lane 0 of every row now holds its row's minimum
  return fmin(fmin(kwy_readlane_f64(v, 0), kwy_readlane_f64(v, 16)), fmin(kwy_readlane_f64(v, 32), kwy_readlane_f64(v, 48)));
}
__device__ __forceinline__ double kwy_wave_max_f64(double v) {
  v = fmax(v, kwy_dpp_keep_f64<0x101>(v));
  v = fmax(v, kwy_dpp_keep_f64<0x102>(v));
  v = fmax(v, kwy_dpp_keep_f64<0x104>(v));
  v = fmax(v, kwy_dpp_keep_f64<0x108>(v));
  return fmax(fmax(kwy_readlane_f64(v, 0), kwy_readlane_f64(v, 16)), fmax(kwy_readlane_f64(v, 32), kwy_readlane_f64(v, 48)));
}

// inclusive prefix sums over the wavefront
__device__ __forceinline__ uint32_t kwy_wave_scan_u32(uint32_t v) {
  v += kwy_dpp_u32<0x111>(v);
  v += kwy_dpp_u32<0x112>(v);
  v += kwy_dpp_u32<0x114>(v);
  v += kwy_dpp_u32<0x118>(v);
  v += kwy_dpp_u32<0x142, 0xa>(v);  // rows 1 and 3 += last lane of the row before
  v += kwy_dpp_u32<0x143, 0xc>(v);  // rows 2 and 3 += lane 31
  return v;
}
__device__ __forceinline__ double kwy_wave_scan_f64(double v) {
  v += kwy_dpp_f64<0x111>(v);
  v += kwy_dpp_f64<0x112>(v);
  v += kwy_dpp_f64<0x114>(v);
  v += kwy_dpp_f64<0x118>(v);
  v += kwy_dpp_f64<0x142, 0xa>(v);
  v += kwy_dpp_f64<0x143, 0xc>(v);
  return v;
}

// sum over the whole block of NT threads; every thread gets the result. red: >= NT/64 doubles.
template <int NT = KWY_THREADS>
__device__ __forceinline__ double kwy_block_sum(double v, double *red) {
  v = kwy_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) s += red[i];
  return s;
}

// in-place inclusive prefix sum of buf[0..L) (LDS).  Thread t owns the
// contiguous chunk [t*chunk, (t+1)*chunk).  tot: NT doubles of LDS.
template <int NT = KWY_THREADS>
__device__ inline void kwy_block_cumsum(double *buf, int L, double *tot) {
  constexpr int PER = NT / 64;  // chunk totals scanned per lane of wave 0
  const int t = threadIdx.x;
  const int chunk = (L + NT - 1) / NT;
  const int b0 = t * chunk;
  const int b1 = min(L, b0 + chunk);
  double run = 0.0;
  for (int i = b0; i < b1; ++i) { run += buf[i]; buf[i] = run; }
  tot[t] = run;
  __syncthreads();
  if (t < 64) {  // wave 0 scans the NT chunk totals, PER per lane
    double a[PER];
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < PER; ++q) { acc += tot[PER * t + q]; a[q] = acc; }
    const double inc = kwy_wave_scan_f64(acc);
    const double excl = inc - acc;  // sum of the lanes before this one
    tot[PER * t] = excl;
#pragma unroll
    for (int q = 1; q < PER; ++q) tot[PER * t + q] = excl + a[q - 1];
  }
  __syncthreads();
  const double off = tot[t];
  if (t > 0)
    for (int i = b0; i < b1; ++i) buf[i] += off;
  __syncthreads();
}

// The same prefix sum of values that are COMPUTED (value(i), i < L), left in buf: the thread's chunk stays in registers
// between its running sum and the addition of the offset, so the values are never stored, read back, summed in place
// and read again -- 2 LDS accesses per element instead of 6 and one barrier fewer than fill + kwy_block_cumsum.
// Same additions in the same order (bit-identical).  CH: compile-time bound of the chunk ceil(L / NT).
template <int NT, int CH, class F>
__device__ inline void kwy_block_cumsum_of(F value, double *buf, int L, double *tot) {
  constexpr int PER = NT / 64;
  const int t = threadIdx.x;
  const int chunk = (L + NT - 1) / NT;
  const int b0 = t * chunk;
  const int b1 = min(L, b0 + chunk);
  double r[CH];
  double run = 0.0;
#pragma unroll
  for (int q = 0; q < CH; ++q) {
    r[q] = 0.0;
    if (q < chunk && b0 + q < b1) { run += value(b0 + q); r[q] = run; }
  }
  tot[t] = run;
  __syncthreads();
  if (t < 64) {  // wave 0 scans the NT chunk totals, PER per lane
    double a[PER];
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < PER; ++q) { acc += tot[PER * t + q]; a[q] = acc; }
    const double inc = kwy_wave_scan_f64(acc);
    const double excl = inc - acc;  // sum of the lanes before this one
    tot[PER * t] = excl;
#pragma unroll
    for (int q = 1; q < PER; ++q) tot[PER * t + q] = excl + a[q - 1];
  }
  __syncthreads();
  const double off = tot[t];
#pragma unroll
  for (int q = 0; q < CH; ++q)
    if (q < chunk && b0 + q < b1) buf[b0 + q] = t > 0 ? r[q] + off : r[q];
  __syncthreads();
}

// offsets[i] = sum_{j<i} count(j) for i <= n, the counts given by a function of the index (evaluated twice: once for
// the chunk totals, once for the offsets) -- counting and scanning in ONE single-workgroup launch.  tot: NT uint64 of LDS.
template <int NT, class F>
__device__ inline void kwy_block_count_scan(F count, int64_t n, uint64_t *__restrict__ offsets, uint64_t *tot) {
  const int t = threadIdx.x;
  const int64_t chunk = (n + NT - 1) / NT;
  const int64_t b0 = t * chunk, b1 = min(n, b0 + chunk);
  uint64_t run = 0;
  for (int64_t i = b0; i < b1; ++i) run += count(i);
  tot[t] = run;
  __syncthreads();
  if (t < 64) {                      // wave 0: exclusive scan of the NT chunk totals, NT/64 per lane
    constexpr int PER = NT / 64;
    uint64_t a[PER], acc = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) { a[q] = acc; acc += tot[PER * t + q]; }
    uint64_t inc = acc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t up = __shfl_up(inc, o);
      if (t >= o) inc += up;
    }
    const uint64_t excl = inc - acc;
#pragma unroll
    for (int q = 0; q < PER; ++q) tot[PER * t + q] = excl + a[q];
  }
  __syncthreads();
  run = tot[t];
  for (int64_t i = b0; i < b1; ++i) { offsets[i] = run; run += count(i); }
  if (b0 < n && b1 == n) offsets[n] = run;
  if (n == 0 && t == 0) offsets[0] = 0;
}

// sums of two values over the block in one exchange; red: >= 2*NT/64 doubles
template <int NT = KWY_THREADS>
__device__ __forceinline__ void kwy_block_sum2(double a, double b, double *red, double *ta, double *tb) {
  a = kwy_wave_sum(a);
  b = kwy_wave_sum(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; red[NT / 64 + (threadIdx.x >> 6)] = b; }
  __syncthreads();
  double sa = red[0], sb = red[NT / 64];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) { sa += red[i]; sb += red[NT / 64 + i]; }
  *ta = sa; *tb = sb;
}

// exclusive scan of one int per thread over the block of NT threads; *total = the sum.  sh: NT / 64 ints of LDS.
template <int NT = KWY_THREADS>
__device__ __forceinline__ int kwy_block_exscan(int v, int *sh, int *total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int inc = (int)kwy_wave_scan_u32((uint32_t)v);
  __syncthreads();
  if (lane == 63) sh[wv] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    if (w < wv) base += sh[w];
    tot += sh[w];
  }
  *total = tot;
  return base + inc - v;
}

// --------------------------------------------------- routines that kernels share bit for bit
// Where two kernels must produce the same bits (the band track and the codec, the band rows and
// kwy_delta_features_dev) they call ONE routine; the library is built with -ffp-contract=off, so
// an expression here rounds the same wherever it is inlined.  (Left apart on purpose: k_delta of
// kwy_mlpg.hip, the interp1Q variants with D4C's decode, the two-pass moments kernels: DESIGN.md.)

// finite, and of the sign a site asks for (the three forms differ for negative values and zero)
__host__ __device__ __forceinline__ bool kwy_finite(double v) { return fabs(v) <= KWY_DBL_MAX; }
__host__ __device__ __forceinline__ bool kwy_finite_pos(double v) { return v > 0.0 && v <= KWY_DBL_MAX; }
__host__ __device__ __forceinline__ bool kwy_finite_nonneg(double v) { return v >= 0.0 && v <= KWY_DBL_MAX; }

// WORLD's aperiodicity bands (codec.cpp): centres at 3 kHz, 6 kHz, ... below fs / 2 - 3 kHz, at most 15 kHz
#define KWY_BAND_INTERVAL 3000.0
#define KWY_BAND_UPPER 15000.0
#define KWY_BAND_MAX 8
#define KWY_BAND_FLOOR -60.0                       // the decoder's node at 0 Hz
__host__ inline int kwy_band_count(int fs) {
  double lim = fs / 2.0 - KWY_BAND_INTERVAL;
  if (lim > KWY_BAND_UPPER) lim = KWY_BAND_UPPER;
  const int n = (int)(lim / KWY_BAND_INTERVAL);
  return n < 0 ? 0 : n;
}

// the coder's value of band b of a frame: interp1Q(0, fs / fft, 20 log10(row), K, 3000 (b + 1))
__device__ __forceinline__ double kwy_band_code(const double *__restrict__ row, int K, int fs, int fft_size, int b) {
  const double shift = (double)fs / fft_size;
  const double xi = KWY_BAND_INTERVAL * (b + 1.0);
  const int base = (int)((xi - 0) / shift);
  const double frac = (xi - 0) / shift - base;
  const double y0 = 20 * log10(row[base]);
  const double dy = (base >= K - 1) ? 0.0 : 20 * log10(row[base + 1]) - y0;
  return y0 + dy * frac;
}

// the decoder's value of bin k over the nodes {0: coarse[0], 3k (i + 1): coarse[i + 1], fs / 2: coarse[nb + 1]}
__device__ __forceinline__ double kwy_band_decode_bin(const double *coarse, int fs, int fft_size, int nb, int k) {
  const int nn = nb + 2;
  const double xi = (double)fs / fft_size * k;
  int seg = 0;  // number of nodes <= xi  (WORLD histc)
  for (int j = 0; j < nn; ++j) {
    const double xj = (j <= nb) ? j * KWY_BAND_INTERVAL : fs / 2.0;
    if (xj <= xi) seg = j + 1;
  }
  if (seg < 1) seg = 1;
  if (seg > nn - 1) seg = nn - 1;
  const double xa = (seg - 1 <= nb) ? (seg - 1) * KWY_BAND_INTERVAL : fs / 2.0;
  const double xb = (seg <= nb) ? seg * KWY_BAND_INTERVAL : fs / 2.0;
  const double s = (xi - xa) / (xb - xa);
  const double v = coarse[seg - 1] + s * (coarse[seg] - coarse[seg - 1]);
  return pow(10.0, v / 20.0);
}

// the reference's DELTA_WINDOWS [-0.5, 0, 0.5] and [1, -2, 1] on three neighbours (np.correlate: the products are
// summed in tap order; a neighbour outside the sequence is passed as 0.0)
__device__ __forceinline__ void kwy_delta_windows(double xm, double x0, double xp, double *d1, double *d2) {
  *d1 = (-0.5 * xm + 0.0 * x0) + 0.5 * xp;
  *d2 = (1.0 * xm + -2.0 * x0) + 1.0 * xp;
}

// the row count of a job: the host value, or the device word clamped to [0, rows] (rows is then the lists' capacity)
__device__ __forceinline__ int64_t kwy_device_count(int64_t rows, const int64_t *n_dev) {
  if (!n_dev) return rows;
  const int64_t w = *n_dev;
  return w < 0 ? 0 : (w < rows ? w : rows);
}

__device__ __forceinline__ int64_t kwy_clamp_row(int64_t r, int64_t rows) { return r < 0 ? 0 : (r >= rows ? rows - 1 : r); }

// One thread: the places of n jobs' rows in a matrix of capacity_rows, in job order behind the cursor; rows_word(k)
// is job k's row count.  A job that would not fit is dropped whole and flagged (count = -1 - rows it had).
template <class F>
__device__ __forceinline__ void kwy_place_rows(int n, F rows_word, int64_t *__restrict__ cursor, int64_t capacity_rows,
                                               int64_t *__restrict__ places) {
  int64_t at = cursor[0];
  for (int k = 0; k < n; ++k) {
    int64_t *word = rows_word(k);
    const int64_t r = word[0];
    if (at + r > capacity_rows) { places[k] = -1; word[0] = -1 - r; continue; }
    places[k] = at;
    at += r;
  }
  cursor[0] = at;
}

// Sum of the m smallest of n non-negative doubles, and the sum of all of them, without sorting.  Thread t holds the
// IEEE bit patterns of elements t, t+NT, ... in key[] (~0 for slots beyond n); the patterns order like the values
// for x >= 0.  The m-th smallest value v* is found, then sum_small = sum(v < v*) + (m - #{v < v*}) * v*.
//   hist: KWY_SELECT_WORDS uint32 of LDS (16-byte aligned), wide: KWY_SELECT_WIDE_WORDS uint32 of LDS (16-byte
//   aligned), red: >= 2*NT/64 doubles -- none of them touched by any thread any more when the call starts (a barrier
//   between two calls, or between the last read of the results' partial sums and the next call).
//   ALL = false: only thread 0 receives the two sums (D4C reads them there and nowhere else).
// Two ways to v*:
//  (1) FROM THE TOP, one histogram: bin = distance of the key's high word from the block's largest high word in
//      quarter binades (256 bins = 64 binades below the maximum, everything lower in the last bin).  The bin that
//      holds the wanted rank -- counted from the largest value -- is left with a few dozen keys of a 2 049-bin
//      spectrum; they are listed in LDS and ranked against each other with full keys.  Only the maximum is reduced,
//      the keys stay as they are.  D4C asks for the 66th largest of 2 049: always here.
//      The spectra are smooth and oversampled: the lanes of a wavefront hold neighbouring bins of the spectrum and
//      count into the same bin of the histogram, one same-address atomic after the other.  So the histogram is kept
//      in KWY_SELECT_COPIES private copies, the copy taken from the lane number, laid out bin-major (the copies of a
//      bin are consecutive words: lanes that share a bin hit different banks; copy-major they would share the bank).
//      One thread per bin adds the copies up with 16-byte reads and leaves the sum in hist[bin], which wavefront 0
//      scans as before.
//      Barriers: [maxima, wavefront sums of all keys, cleared copies] A [counting] B [adding the copies up] C [scan
//      by wavefront 0] S [list] L [ranking by the first threads] K [sum below v*] R [thread 0 / everyone adds the
//      wavefronts' partial sums]: seven, where the single histogram with kwy_block_sum2 behind it and its caller's
//      closing barrier made eight.  The sum of all keys needs nothing the selection finds and leaves with the
//      maxima; behind R nobody reads hist / wide any more, and red[] only in the threads that take the results.
//  (2) GENERAL, MSB-first radix select (KWY_SELECT_BITS bits a round) on key - min(key), starting at the highest bit
//      in which the block's keys differ; two barriers per round, histogram and control words double-buffered; a
//      round that leaves <= 124 keys hands over to the same ranking.  Taken when (1) ends in its last bin or with a
//      crowded one (flat data, ties by the hundred, a rank far from the top).
// The two results are summed as they always were -- per thread in slot order, over the wavefront (kwy_wave_sum), then
// the wavefronts' sums left to right -- and v* is one of the keys, fixed by the data: the bits do not depend on how
// v* was found.
// Digit width 8 (256 bins) is what the kernels use.  11 bits -- the whole exponent of a non-negative IEEE double in
// the first round -- was measured and is SLOWER (what the rounds save in barriers is lost clearing and scanning
// 2048 bins per round).  Wave-aggregated atomics (the lanes that share the first live lane's digit counted with one
// atomic) were measured too: on real group-delay spectra the ballots cost more issue slots than the same-address
// atomics they save (3 280 against 1 936 clocks for the nine slots of a round): KWY_SELECT_AGG=1 keeps that form.
// KWY_SELECT_COPIES (k_d4c_bands<12, true> per launch, one wave of 16 pairs on one stream, two runs each in one
// session, profiles/sel_variants_serial.txt; the single histogram with kwy_block_sum2 and the caller's barrier: 1.284 ms):
//   1 copy (the single histogram, with the barriers as above)   1.267 ms
//   16 copies   1.278 ms (16 B of scratch in the band kernel)      8 copies   1.255 ms (12 B)
//   4 copies    1.206 ms (no scratch)  <- chosen; LDS bank conflicts / LDS active and SQ_WAIT_ANY / wave cycles of the
//   kernel against the single histogram's: profiles/sel_*_pmc_sq_summary.json.  Every copy is a 16-byte clear and a
//   16-byte read per thread and call; no padding between the bins (neighbouring bins lie in different banks as it is).
// Measured in the same session and LEFT OUT, each slower than the form kept (the wavefronts of four workgroups share
// a SIMD: one that waits at a barrier leaves the issue slots to the others, while ballots and work repeated in every
// wavefront take them):
//   - the list appended per wavefront (a ballot per slot, one returning atomic per wavefront, the lane's place from
//     the prefix count of its ballot) instead of one returning atomic per key: 1.267 -> 1.295 ms;
//   - every wavefront scanning the histogram and ranking the list for itself, bin, rank and key in scalar registers,
//     barriers S and K gone: 1.267 -> 1.301 ms; both with 16 copies: 1.321 ms;
//   - wavefront 0 adding the copies up inside its scan (barrier C gone): 1.263 ms with 4 copies, 16 B of scratch.
#ifndef KWY_SELECT_BITS
#define KWY_SELECT_BITS 8
#endif
#define KWY_SELECT_BINS (1 << KWY_SELECT_BITS)
#ifndef KWY_SELECT_AGG
#define KWY_SELECT_AGG 0
#endif
#ifndef KWY_SELECT_COPIES
#define KWY_SELECT_COPIES 4
#endif
#define KWY_SELECT_WORDS(NT) (2 * KWY_SELECT_BINS + 64)
#define KWY_SELECT_WIDE_WORDS (KWY_SELECT_BINS * KWY_SELECT_COPIES)
#define KWY_SELECT_LIST (KWY_SELECT_BINS / 2 - 4)         // keys the ranking takes (the other histogram's words)

__device__ __forceinline__ uint32_t kwy_wave_max_u32(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x101, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x102, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x104, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x108, 0xf, 0xf, false));
  return max(max((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16)),
             max((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48)));
}

// one wavefront: the bin of h[0 .. BINS) that holds rank kk (1-based, bins taken in index order).  True in the one
// lane whose bins hold it, with c[0] = bin, c[1] = rank inside it, c[2] = its population, c[3] = keys in the bins
// before it.
// (Scan and ranking are each split into a part that finds and a part that publishes: with the bodies in one piece
// the register allocation of k_d4c_bands<12, true>, which sits at its cap of 128, spills 28 bytes per lane; so, none.)
__device__ __forceinline__ bool kwy_select_scan_lane(const uint32_t *h, int kk, int lane, uint32_t (&c)[4]) {
  constexpr int PERLANE = KWY_SELECT_BINS / 64;           // bins scanned per lane
  static_assert(PERLANE % 4 == 0 && PERLANE >= 4, "bins per lane must be a multiple of 4");
  // lane l owns bins [PERLANE l, PERLANE (l + 1)): their total first, then only the lane whose range holds the
  // wanted rank walks its bins again (the counts are not kept in registers)
  const uint4 *hp = (const uint4 *)h + lane * (PERLANE / 4);
  uint32_t tot = 0;
#pragma unroll
  for (int q = 0; q < PERLANE / 4; ++q) {
    const uint4 c4 = hp[q];
    tot += (c4.x + c4.y) + (c4.z + c4.w);
  }
  uint32_t before = kwy_wave_scan_u32(tot) - tot;
  const bool mine = (uint32_t)kk > before && (uint32_t)kk <= before + tot;
  c[0] = c[1] = c[2] = c[3] = 0u;
  if (mine) {
    const uint32_t *hb = h + PERLANE * lane;
    for (int q = 0; q < PERLANE; ++q) {
      const uint32_t n = hb[q];
      if ((uint32_t)kk <= before + n) {
        c[0] = PERLANE * lane + q;
        c[1] = (uint32_t)kk - before;
        c[2] = n;
        c[3] = before;
        break;
      }
      before += n;
    }
  }
  return mine;
}

// wavefront 0: the same into LDS -> ctl[0] = bin, ctl[1] = rank inside it, ctl[2] = its population, ctl[3] = keys in
// the bins before it
__device__ __forceinline__ void kwy_select_scan(const uint32_t *h, int kk, uint32_t *ctl, int lane) {
  uint32_t c[4];
  if (kwy_select_scan_lane(h, kk, lane, c)) { ctl[0] = c[0]; ctl[1] = c[1]; ctl[2] = c[2]; ctl[3] = c[3]; }
}

// the listed keys list[0 .. pop) ranked against each other (pop <= KWY_SELECT_LIST; four entries behind the list
// must be readable).  DESCENDING: the key with `rank - 1` listed keys in front of it when sorted from the largest.
// Thread tid < pop looks at entry tid; the one that holds the wanted key publishes it with out_count[0] = the number
// of listed keys in front of it (strictly) and out_count[1] = the listed keys equal to it.  Ascending order: the same
// with the comparison turned round.
template <bool DESCENDING>
__device__ __forceinline__ bool kwy_select_rank_entry(const unsigned long long *list, int pop, int rank, int e,
                                                      unsigned long long mine, int *front_out, int *ties_out) {
  int front = 0, tie_front = 0, ties = 0;
  for (int j = 0; j < pop; j += 4) {                       // four keys a trip: two 16-byte reads in flight
    const ulonglong2 o01 = *(const ulonglong2 *)(list + j), o23 = *(const ulonglong2 *)(list + j + 2);
    const unsigned long long o[4] = {o01.x, o01.y, o23.x, o23.y};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool in = j + q < pop;
      front += in & (DESCENDING ? o[q] > mine : o[q] < mine);
      const bool eq = in & (o[q] == mine);
      ties += eq;
      tie_front += eq & (j + q < e);
    }
  }
  *front_out = front; *ties_out = ties;
  return front + tie_front == rank - 1;
}
template <bool DESCENDING>
__device__ __forceinline__ void kwy_select_rank(const unsigned long long *list, int pop, int rank, int tid,
                                                unsigned long long *out_key, uint32_t *out_count) {
  if (tid < pop) {
    const unsigned long long mine = list[tid];
    int front, ties;
    if (kwy_select_rank_entry<DESCENDING>(list, pop, rank, tid, mine, &front, &ties)) {
      *out_key = mine; out_count[0] = (uint32_t)front; out_count[1] = (uint32_t)ties;
    }
  }
}
template <int RMAX, int NT = KWY_THREADS, bool ALL = true>
__device__ inline void kwy_block_smallest_sum(unsigned long long (&key)[RMAX], int n, int m,
                                              uint32_t *hist, uint32_t *wide, double *red, double *sum_small,
                                              double *sum_all) {
  constexpr int BITS = KWY_SELECT_BITS, BINS = 1 << BITS, C = KWY_SELECT_COPIES;
  constexpr int TOP_SHIFT = 18;                           // high word: 20 mantissa bits -> quarter binades
  static_assert(C == 1 || (C >= 4 && C <= 64 && (C & (C - 1)) == 0), "copies: one, or a power of two in whole 16-byte reads");
  static_assert(NT <= 512, "the general path's extrema take 4 NT / 64 control words");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t *ctlb = hist + 2 * BINS;  // 2 x {digit, rank, population, before}; [8..9] one 64-bit key; [10] list
                                     // length; [11..12] two counts; [16 ..] one word per wavefront; [32 ..] the
                                     // general path's extrema, two doubles per wavefront
  unsigned long long *k64 = (unsigned long long *)(ctlb + 8);
  unsigned long long *list = (unsigned long long *)(hist + BINS);
  unsigned long long vkey;           // bit pattern of v*
  int copies;                        // how many keys equal to v* belong to the m smallest

  // ---- (1) from the top.  The sum of all keys needs nothing the selection finds: its wavefront sums leave with the
  // exchange of the maxima (barrier A) and are read behind barrier R.
  uint32_t hmax = 0;
  double s_all = 0.0;
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    if (tid + NT * r < n) {
      hmax = max(hmax, (uint32_t)(key[r] >> 32));
      s_all += __longlong_as_double((long long)key[r]);
    }
  }
  hmax = kwy_wave_max_u32(hmax);
  s_all = kwy_wave_sum(s_all);
  if (lane == 0) { ctlb[16 + wv] = hmax; red[NT / 64 + wv] = s_all; }
  if constexpr (C > 1) {
    static_assert(C == 1 || BINS * C % 4 == 0, "cleared in 16-byte stores");
    for (int i = tid; i < BINS * C / 4; i += NT) ((uint4 *)wide)[i] = make_uint4(0u, 0u, 0u, 0u);
  } else {
    for (int i = tid; i < BINS; i += NT) hist[i] = 0;
  }
  if (tid == 0) ctlb[10] = 0;
  __syncthreads();                                        // A
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
      if constexpr (C > 1) atomicAdd(&wide[dg[r] * C + (lane & (C - 1))], 1u);
      else atomicAdd(&hist[dg[r]], 1u);
    }
  }
  __syncthreads();                                        // B
  if constexpr (C > 1) {
    // one thread per bin adds its copies up: 16-byte reads, the lanes of a read group that start in the same bank
    // (64 / C apart) at different quarters of their bins
    for (int b = tid; b < BINS; b += NT) {
      const uint4 *bp = (const uint4 *)(wide + b * C);
      uint32_t c = 0;
#pragma unroll
      for (int q = 0; q < C / 4; ++q) {
        const uint4 c4 = bp[(q + b / (64 / C)) & (C / 4 - 1)];
        c += (c4.x + c4.y) + (c4.z + c4.w);
      }
      hist[b] = c;
    }
    __syncthreads();                                      // C
  }
  if (wv == 0) kwy_select_scan(hist, n - m + 1, ctlb, lane);
  __syncthreads();                                        // S
  const uint32_t chosen = ctlb[0], pop = ctlb[2];
  const int rank = (int)ctlb[1], above = (int)ctlb[3];
  if (chosen < (uint32_t)(BINS - 1) && pop <= (uint32_t)KWY_SELECT_LIST) {
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
      if (dg[r] == chosen) list[atomicAdd(&ctlb[10], 1u)] = key[r];
    __syncthreads();                                      // L
    kwy_select_rank<true>(list, (int)pop, rank, tid, k64, &ctlb[11]);
    __syncthreads();                                      // K
    vkey = *k64;
    const int front = (int)ctlb[11], ties = (int)ctlb[12];
    copies = m - (n - above - front - ties);              // keys >= v*: above + listed in front + ties
  } else {
    // ---- (2) general: the block's smallest and largest key, relative keys, radix rounds
    double *ext = (double *)(ctlb + 32);
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
    if (lane == 0) { ext[wv] = lo; ext[NT / 64 + wv] = hi; }
    for (int i = tid; i < BINS; i += NT) hist[i] = 0;
    if (tid == 0) ctlb[10] = 0;
    __syncthreads();
    lo = ext[0]; hi = ext[NT / 64];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) { lo = fmin(lo, ext[i]); hi = fmax(hi, ext[NT / 64 + i]); }
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
  double s_less = 0.0;
#pragma unroll
  for (int r = 0; r < RMAX; ++r)
    if (tid + NT * r < n && key[r] < vkey) s_less += __longlong_as_double((long long)key[r]);
  s_less = kwy_wave_sum(s_less);
  if (lane == 0) red[wv] = s_less;
  __syncthreads();                                        // R
  if (ALL || tid == 0) {
    double t_less = red[0], t_all = red[NT / 64];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) { t_less += red[i]; t_all += red[NT / 64 + i]; }
    *sum_small = t_less + (double)copies * vstar;
    *sum_all = t_all;
  }
}

__device__ __forceinline__ int kwy_matlab_round(double x) {
  return x > 0 ? (int)(x + 0.5) : (int)(x - 0.5);
}
