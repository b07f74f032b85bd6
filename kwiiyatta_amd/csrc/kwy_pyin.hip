// kwy_pyin.hip -- probabilistic YIN (Mauch & Dixon 2014), the second f0 estimator beside DIO (include/kwy.h states the
// algorithm; the reference has no counterpart).
//
//   k_pyin_observe   one workgroup per frame, all frames of up to PYIN_BATCH utterances in one grid.  The frame's
//                    difference function, its cumulative-mean normalisation, the troughs, the ordered walk over the
//                    threshold prior and the pitch bins all stay in LDS; what leaves the chip is one row of nb + 1 log
//                    probabilities.  The correlation is two real transforms, a product and an inverse
//                    (kwy_rfft_inplace / kwy_irfft_inplace) in ONE buffer: the spectrum of the first half waits in
//                    registers (H / 256 + 1 complex a thread) while the whole frame is transformed, so a 4096-sample
//                    transform needs 32 KB of LDS for its data, not 64.
//   k_pyin_decode    one workgroup per utterance, one thread per state: the Viterbi recursion with delta double-buffered
//                    in LDS and one LDS-only barrier a frame, 16-bit back-pointers to the caller's scratch, and the
//                    back-trace on the first wavefront.
//
// Nothing here is contracted (-ffp-contract=off): delta is the sum a numpy model forms from the same rows, bit for bit.
#include <math.h>

#include <string>
#include <vector>

#include "kwy_internal.hpp"

#define PYIN_NT 256                  // threads of the observation kernel
#define PYIN_BATCH 32                // utterances of one pass of launches (as DIO's)
#define PYIN_TINY 1e-300             // floor of a probability in front of the logarithm
#define PYIN_MAX_STATES 1024
#define PYIN_MAX_RADIUS 8191         // the back-pointer keeps the offset in 15 bits

struct pyin_view {
  const double *x;       // waveform (null: the decoder does not look for non-finite samples)
  double *tpos, *f0;     // frame times (may be null) / coarse track
  int *status;
  double *L;             // T x (nb + 1)
  unsigned short *bp;    // T x 2 nb
  int n, T;
};
typedef kwy_batch<pyin_view, PYIN_BATCH> pyin_table;
struct pyin_par {
  double fs, f0_floor, frame_period, pa;
  int W, tau_min, tau_max, nb;
};
static_assert(sizeof(pyin_table) + sizeof(pyin_par) + 64 <= KWY_KERNARG_MAX, "the job table travels in the kernel arguments");

// F(v) = 1 - (1 - v)^18 (1 + 18 v): the distribution function of Beta(2, 18), the powers by squaring
__device__ __forceinline__ double pyin_prior_cdf(double v) {
  v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
  const double u = 1.0 - v;
  const double u2 = u * u, u4 = u2 * u2, u8 = u4 * u4, u16 = u8 * u8;
  return 1.0 - (u16 * u2) * (1.0 + 18.0 * v);
}

__global__ __launch_bounds__(64) void k_pyin_clear(pyin_table B) {
  if ((int)threadIdx.x < B.n) *B.u[threadIdx.x].status = 0;
}

template <int LOG2H>
__global__ __launch_bounds__(PYIN_NT) void k_pyin_observe(pyin_table B, pyin_par P, const kwy_c *__restrict__ twH,
                                                          const kwy_c *__restrict__ twP, const kwy_c *__restrict__ twN) {
  constexpr int H = 1 << LOG2H, N = 2 * H, NT = PYIN_NT, RS = H / NT, CH = H / NT + 1;
  extern __shared__ double smem[];
  kwy_c *z = (kwy_c *)smem;                 // H + 1 complex: the transforms; afterwards the sums, masses and bins
  kwy_c *twl = z + (H + 1);                 // exp(-2 pi i k / H), k < H/8
  double *eb = (double *)(twl + H / 8);     // H + 2: sliding energy -> d -> d'
  double *tot = eb + (H + 2);               // NT
  double *red = tot + NT;                   // 16
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int utt = B.find(blockIdx.x);
  const int frame = blockIdx.x - B.start[utt];
  const double *__restrict__ x = B.u[utt].x;
  const int n = B.u[utt].n;
  const int W = P.W, tau_max = P.tau_max, nb = P.nb;
  const int lo = P.tau_min > 1 ? P.tau_min : 1;
  const double tsec = frame * P.frame_period / 1000.0;
  const int c = (int)floor(tsec * P.fs + 0.5);
  bool bad = false;
  auto sample = [&](int q) {               // sample q of the frame x[c - W .. c + W), zeros outside the signal
    const int m = c - W + q;
    double v = 0.0;
    if (m >= 0 && m < n) {
      v = x[m];
      if (!kwy_finite(v)) { bad = true; v = 0.0; }
    }
    return v;
  };
  double *A = (double *)z;
  for (int i = tid; i < H / 8; i += NT) twl[i] = twH[i];
  // ---- the spectrum of the first W samples, kept in registers
#pragma unroll
  for (int j = 0; j < N / NT; ++j) {
    const int q = tid + NT * j;
    A[q] = q < W ? sample(q) : 0.0;
  }
  __syncthreads();
  const kwy_c twb = twN[tid];
  kwy_rfft_inplace<LOG2H, NT>(z, twl, twP, twb, twN);
  kwy_c SA[RS];
#pragma unroll
  for (int r = 0; r < RS; ++r) SA[r] = z[tid + NT * r];
  const double sah = z[H].x;
  __syncthreads();
  // ---- the whole frame: sliding energy by a prefix sum, then its spectrum
#pragma unroll
  for (int j = 0; j < N / NT; ++j) {
    const int q = tid + NT * j;
    A[q] = q < 2 * W ? sample(q) : 0.0;
  }
  __syncthreads();
  double part = 0.0;
  for (int q = tid; q < W; q += NT) part += A[q] * A[q];
  const double e0 = kwy_block_sum<NT>(part, red);
  // e(tau) = e(0) + sum_{i <= tau} (x[i - 1 + W]^2 - x[i - 1]^2)
  kwy_block_cumsum_of<NT, CH>([&](int i) { return i == 0 ? e0 : A[i - 1 + W] * A[i - 1 + W] - A[i - 1] * A[i - 1]; },
                              eb, W + 1, tot);
  kwy_rfft_inplace<LOG2H, NT>(z, twl, twP, twb, twN);
#pragma unroll
  for (int r = 0; r < RS; ++r) {
    const kwy_c a = SA[r];
    z[tid + NT * r] = cmul(kwy_c{a.x, -a.y}, z[tid + NT * r]);
  }
  if (tid == 0) z[H] = {sah * z[H].x, 0.0};
  kwy_irfft_inplace<LOG2H, NT>(z, twl, twP, twb, twN);      // A[tau] = N r(tau)
  // ---- the difference function d(tau), tau <= W = tau_max + 1, over e
  const double e0r = eb[0];
  __syncthreads();
  for (int tau = tid; tau <= W; tau += NT) {
    const double r = A[tau] * (1.0 / N);
    const double s = e0r + eb[tau];
    double d = s - 2.0 * r;
    if (d < 0x1p-40 * s || d < 0.0) d = 0.0;
    eb[tau] = d;
  }
  __syncthreads();
  // ---- d'(tau) = d(tau) tau / sum_{j = 1 .. tau} d(j), over d
  double *C = (double *)z;
  kwy_block_cumsum_of<NT, CH>([&](int i) { return i >= 1 ? eb[i] : 0.0; }, C, W + 1, tot);
  for (int tau = tid; tau <= W; tau += NT) {
    double dp = 1.0;
    if (tau >= 1 && C[tau] != 0.0) dp = eb[tau] * tau / C[tau];
    eb[tau] = dp;
  }
  __syncthreads();
  // ---- troughs and the ordered walk: thread t owns the lags [t chunk, (t + 1) chunk); the running minimum in front of
  //      a lag is a prefix minimum over the block
  double *mass = (double *)z;               // [0, W]
  int *bin = (int *)(mass + (H + 1));       // [0, W]
  const int chunk = (W + 1 + NT - 1) / NT, b0 = tid * chunk;
  double cv[CH], coff[CH], mloc[CH];
  bool cand[CH];
  double run = 1.0;
#pragma unroll
  for (int q = 0; q < CH; ++q) {
    const int tau = b0 + q;
    cand[q] = false;
    cv[q] = 1.0; coff[q] = 0.0; mloc[q] = run;
    if (q < chunk && tau >= lo && tau <= tau_max) {
      const double a = eb[tau - 1], b = eb[tau], cc = eb[tau + 1];
      if (b < a && b <= cc) {
        const double den = a - 2.0 * b + cc;
        double off = 0.0, v = b;
        if (den > 0.0) {
          off = 0.5 * (a - cc) / den;
          v = b - 0.25 * (a - cc) * off;
        }
        if (v < 0.0) v = 0.0;
        cand[q] = true; cv[q] = v; coff[q] = off;
        if (v < run) run = v;
      }
    }
  }
  double inc = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(inc, o);
    if (lane >= o) inc = fmin(inc, up);
  }
  double ex = __shfl_up(inc, 1);
  if (lane == 0) ex = 1.0;
  if (lane == 63) red[wv] = inc;
  __syncthreads();
  double gmin = 1.0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const double m = red[w];
    if (w < wv) ex = fmin(ex, m);
    gmin = fmin(gmin, m);
  }
#pragma unroll
  for (int q = 0; q < CH; ++q) {
    const int tau = b0 + q;
    if (q < chunk && tau <= W) {
      double ms = 0.0;
      int bi = -1;
      const double mb = fmin(ex, mloc[q]);
      if (cand[q] && cv[q] < mb) {
        const double fv = pyin_prior_cdf(cv[q]);
        ms = pyin_prior_cdf(mb) - fv;
        if (cv[q] == gmin) ms = ms + P.pa * fv;       // the last candidate that lowered the minimum
        const double f = P.fs / (tau + coff[q]);
        const double fb = floor(KWY_PYIN_BINS_PER_OCTAVE * log2(f / P.f0_floor));
        if (fb >= 0.0 && fb < (double)nb) bi = (int)fb;
      }
      mass[tau] = ms;
      bin[tau] = bi;
    }
  }
  __syncthreads();
  // ---- the bins: thread b adds the masses of its bin in ascending lag (the lags that can reach it, one more each side)
  double *__restrict__ Lrow = B.u[utt].L + (size_t)frame * (nb + 1);
  double psum = 0.0;
  for (int b = tid; b < nb; b += NT) {
    const double fhi = P.f0_floor * exp2((b + 1) / (double)KWY_PYIN_BINS_PER_OCTAVE);
    const double flo = P.f0_floor * exp2(b / (double)KWY_PYIN_BINS_PER_OCTAVE);
    int t0 = (int)floor(P.fs / fhi) - 1, t1 = (int)ceil(P.fs / flo) + 1;
    t0 = t0 < lo ? lo : t0;
    t1 = t1 > tau_max ? tau_max : t1;
    double p = 0.0;
    for (int tau = t0; tau <= t1; ++tau)
      if (bin[tau] == b) p += mass[tau];
    Lrow[b] = kwy_log(p > PYIN_TINY ? p : PYIN_TINY);
    psum += p;
  }
  const double total = kwy_block_sum<NT>(psum, red);
  if (tid == 0) {
    const double pu = (1.0 - total) / nb;
    Lrow[nb] = kwy_log(pu > PYIN_TINY ? pu : PYIN_TINY);
    if (B.u[utt].tpos) B.u[utt].tpos[frame] = tsec;
  }
  if (bad) *B.u[utt].status = 1;
}

// The Viterbi pass of one utterance.  States: s < nb voiced bin s, s >= nb unvoiced bin s - nb.  tr[j], j <= 2R: the log
// weight of a step from bin b - R + j to bin b with the voicing kept, tr[2R + 1 + j]: with the voicing changed.  The
// uniform start adds one constant to every state and is left out.  Back-pointer: j, bit 15 set where the voicing
// changed.  scan: look through the waveform for a non-finite sample first (the frames of a short window do not cover
// every sample).
__global__ __launch_bounds__(PYIN_MAX_STATES) void k_pyin_decode(pyin_table B, int nb, int R,
                                                                 const double *__restrict__ trans,
                                                                 const double *__restrict__ freq) {
  extern __shared__ double smem[];
  const int S = 2 * nb, NTR = 2 * R + 1;
  double *delta = smem;                      // [2][S]
  double *tr = smem + 2 * S;                 // [2][NTR]
  __shared__ int flag;
  const pyin_view &u = B.u[blockIdx.x];
  const int tid = threadIdx.x, NT = blockDim.x, T = u.T;
  if (tid == 0) flag = *u.status;
  for (int i = tid; i < 2 * NTR; i += NT) tr[i] = trans[i];
  __syncthreads();
  if (u.x) {
    bool bad = false;
    for (int i = tid; i < u.n; i += NT) bad |= !kwy_finite(u.x[i]);
    if (bad) flag = 1;
    __syncthreads();
  }
  if (flag) {                                // (uniform)
    for (int t = tid; t < T; t += NT) u.f0[t] = 0.0;
    if (tid == 0) *u.status = 1;
    return;
  }
  const bool live = tid < S, voiced = tid < nb;
  const int b = voiced ? tid : tid - nb;
  const double *__restrict__ Lc = u.L + (voiced ? b : nb);
  const int jlo = R - b > 0 ? R - b : 0, jhi = nb - 1 - b + R < 2 * R ? nb - 1 - b + R : 2 * R;
  unsigned short *__restrict__ bp = u.bp;
  if (live) delta[tid] = Lc[0];
  double next = live && T > 1 ? Lc[(size_t)(nb + 1)] : 0.0;
  kwy_lds_barrier();
  for (int t = 1; t < T; ++t) {
    const double obs = next;
    if (live && t + 1 < T) next = Lc[(size_t)(t + 1) * (nb + 1)];
    if (live) {
      const double *prev = delta + ((t - 1) & 1) * S;
      const double *same = prev + (voiced ? 0 : nb) + (b - R), *other = prev + (voiced ? nb : 0) + (b - R);
      double best = same[jlo] + tr[jlo];
      int code = jlo;
      for (int j = jlo + 1; j <= jhi; ++j) {
        const double v = same[j] + tr[j];
        if (v > best) { best = v; code = j; }
      }
      for (int j = jlo; j <= jhi; ++j) {
        const double v = other[j] + tr[NTR + j];
        if (v > best) { best = v; code = j | 0x8000; }
      }
      delta[(t & 1) * S + tid] = best + obs;
      bp[(size_t)t * S + tid] = (unsigned short)code;
    }
    kwy_lds_barrier();
  }
  __syncthreads();                           // the back-pointers of the whole block are visible to its first wavefront
  if (tid >= 64) return;
  const double *last = delta + ((T - 1) & 1) * S;
  double bv = last[tid < S ? tid : 0];
  int bs = tid < S ? tid : 0;
  for (int s = tid + 64; s < S; s += 64)
    if (last[s] > bv) { bv = last[s]; bs = s; }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(bv, o);
    const int os = __shfl_xor(bs, o);
    if (ov > bv || (ov == bv && os < bs)) { bv = ov; bs = os; }
  }
  int s = __builtin_amdgcn_readfirstlane(bs);
  for (int t = T - 1; t >= 0; --t) {
    if (tid == 0) u.f0[t] = s < nb ? freq[s] : 0.0;
    if (t == 0) break;
    const int code = bp[(size_t)t * S + s];
    const bool v = s < nb;
    int pb = (v ? s : s - nb) - R + (code & 0x7fff);
    pb = pb < 0 ? 0 : (pb >= nb ? nb - 1 : pb);
    const bool pv = (code & 0x8000) ? !v : v;
    s = pv ? pb : pb + nb;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
struct pyin_cfg {
  int W, tau_min, tau_max, nb, R, log2h;
};

extern "C" int kwy_pyin_fft_size(int fs, double f0_floor) {
  if (fs <= 0 || !(f0_floor > 0) || !((double)fs / f0_floor < 1e8)) return 0;
  const int64_t W = (int64_t)ceil((double)fs / f0_floor) + 1;
  int64_t N = 1024;
  while (N < 2 * W) N *= 2;
  return N > 0x40000000 ? 0 : (int)N;
}

extern "C" int kwy_pyin_bins(double f0_floor, double f0_ceil) {
  if (!(f0_floor > 0) || !(f0_ceil > f0_floor) || !(f0_ceil / f0_floor < 1e6)) return 0;
  return (int)ceil(KWY_PYIN_BINS_PER_OCTAVE * log2(f0_ceil / f0_floor));
}

extern "C" int kwy_pyin_radius(double frame_period_ms, double max_rate) {
  if (!(frame_period_ms > 0) || !(max_rate >= 0) || !(max_rate * frame_period_ms < 1e6)) return -1;
  return (int)ceil(max_rate * KWY_PYIN_BINS_PER_OCTAVE * frame_period_ms / 1000.0);
}

static size_t pyin_block_bytes(int64_t frames, int nb) {
  return kwy_pad(sizeof(double) * (size_t)frames * (nb + 1)) + kwy_pad(sizeof(unsigned short) * (size_t)frames * 2 * nb);
}

extern "C" size_t kwy_pyin_scratch_bytes(int64_t frames, int nb, int count) {
  if (frames <= 0 || nb <= 0 || count <= 0) return 0;
  return pyin_block_bytes(frames, nb) * (count < PYIN_BATCH ? count : PYIN_BATCH) + kwy_pad(sizeof(int) * PYIN_BATCH);
}

static int pyin_config(kwy_ctx *ctx, int fs, double f0_floor, double f0_ceil, double frame_period_ms, double max_rate,
                       pyin_cfg *out) {
  if (fs <= 0 || !(f0_floor > 0) || !(f0_ceil > f0_floor) || !(frame_period_ms > 0)) {
    ctx->err = "pyin: bad argument";
    return KWY_EINVAL;
  }
  const int N = kwy_pyin_fft_size(fs, f0_floor);
  if (N < 1024 || N > 4096) { ctx->err = "pyin: the frame of this rate and f0_floor needs a transform beyond 4096 samples"; return KWY_EINVAL; }
  pyin_cfg c;
  c.tau_min = (int)floor((double)fs / f0_ceil);
  c.tau_max = (int)ceil((double)fs / f0_floor);
  c.W = c.tau_max + 1;
  c.nb = kwy_pyin_bins(f0_floor, f0_ceil);
  if (c.nb < 1 || 2 * c.nb > PYIN_MAX_STATES) { ctx->err = "pyin: more than 1024 states (120 bins an octave from f0_floor to f0_ceil, voiced and unvoiced)"; return KWY_EINVAL; }
  c.R = kwy_pyin_radius(frame_period_ms, max_rate);
  if (c.R < 0 || c.R > PYIN_MAX_RADIUS) { ctx->err = "pyin: bad pitch rate"; return KWY_EINVAL; }
  c.log2h = kwy_ilog2(N) - 1;
  *out = c;
  return KWY_OK;
}

// the 2 (2R + 1) log transition values: [voicing kept | voicing changed][offset + R]
static std::vector<double> pyin_transitions(int R, double switch_prob) {
  std::vector<double> t(2 * (2 * R + 1));
  const double norm = (double)(R + 1) * (double)(R + 1);
  for (int j = 0; j <= 2 * R; ++j) {
    const int k = j - R;
    const double w = (R + 1 - (k < 0 ? -k : k)) / norm;
    t[j] = log(w * (1.0 - switch_prob));
    t[2 * R + 1 + j] = log(w * switch_prob);
  }
  return t;
}

static int pyin_launch_observe(kwy_ctx *ctx, const pyin_table &tb, const pyin_cfg &c, int fs, double f0_floor,
                               double frame_period_ms, double pa) {
  const kwy_c *twH, *twN, *twP;
  KWY_TRY(kwy_get_twiddles(ctx, c.log2h, &twH));
  KWY_TRY(kwy_get_twiddle_powers(ctx, c.log2h, &twP));
  KWY_TRY(kwy_get_twiddles(ctx, c.log2h + 1, &twN));
  const pyin_par P = {(double)fs, f0_floor, frame_period_ms, pa, c.W, c.tau_min, c.tau_max, c.nb};
  const int H = 1 << c.log2h;
  const size_t lds = sizeof(kwy_c) * (H + 1 + H / 8) + sizeof(double) * (H + 2 + PYIN_NT + 16);
  const dim3 grid((unsigned)tb.start[tb.n]), block(PYIN_NT);
  kwy_prof_scope ps_(ctx, "k_pyin_observe");
  if (c.log2h == 9) hipLaunchKernelGGL(k_pyin_observe<9>, grid, block, lds, ctx->stream, tb, P, twH, twP, twN);
  else if (c.log2h == 10) hipLaunchKernelGGL(k_pyin_observe<10>, grid, block, lds, ctx->stream, tb, P, twH, twP, twN);
  else hipLaunchKernelGGL(k_pyin_observe<11>, grid, block, lds, ctx->stream, tb, P, twH, twP, twN);
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

static int pyin_launch_decode(kwy_ctx *ctx, const pyin_table &tb, int nb, int R, const double *trans, const double *freq) {
  const int threads = (2 * nb + 63) / 64 * 64;
  const size_t lds = sizeof(double) * (4 * (size_t)nb + 2 * (2 * (size_t)R + 1));
  KWY_PROF(ctx, "k_pyin_decode", hipLaunchKernelGGL(k_pyin_decode, dim3(tb.n), dim3(threads), lds, ctx->stream, tb, nb, R,
                                                    trans, freq));
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

static int pyin_clear(kwy_ctx *ctx, const pyin_table &tb) {
  hipLaunchKernelGGL(k_pyin_clear, dim3(1), dim3(64), 0, ctx->stream, tb);
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

// The tables below are cached per parameter set in the context (under 4 KB each).  A caller that sweeps parameters must
// not grow the context without bound: at PYIN_MAX_TABLES cached tables the stream is drained and all of them go.
#define PYIN_MAX_TABLES 32
static int pyin_trim_tables(kwy_ctx *ctx) {
  std::vector<std::string> mine;
  for (const auto &kv : ctx->d_mats)
    if (kv.first.compare(0, 5, "pyin_") == 0) mine.push_back(kv.first);
  if (mine.size() < PYIN_MAX_TABLES) return KWY_OK;
  KWY_HIP(hipStreamSynchronize(ctx->stream));
  for (const std::string &key : mine) {
    (void)hipFree(ctx->d_mats[key]);
    ctx->d_mats.erase(key);
  }
  return KWY_OK;
}

// the device tables of the whole estimator: transitions and bin centres for (f0_floor, nb, R, switch_prob)
static int pyin_tables(kwy_ctx *ctx, const pyin_cfg &c, double f0_floor, double switch_prob, const double **trans,
                       const double **freq) {
  if (!(switch_prob > 0.0 && switch_prob < 1.0)) { ctx->err = "pyin: the switch probability lies within (0, 1)"; return KWY_EINVAL; }
  KWY_TRY(pyin_trim_tables(ctx));
  char key[160];
  snprintf(key, sizeof key, "pyin_tr/%d/%a", c.R, switch_prob);
  KWY_TRY(kwy_cached_table<double>(ctx, key, [&] { return pyin_transitions(c.R, switch_prob); }, trans));
  snprintf(key, sizeof key, "pyin_fq/%d/%a", c.nb, f0_floor);
  KWY_TRY(kwy_cached_table<double>(ctx, key, [&] {
    std::vector<double> f(c.nb);
    for (int b = 0; b < c.nb; ++b) f[b] = f0_floor * exp2((b + 0.5) / KWY_PYIN_BINS_PER_OCTAVE);
    return f;
  }, freq));
  return KWY_OK;
}

// One pass over jobs[0 .. count), count <= PYIN_BATCH (device pointers); scratch: `count` blocks of `block` bytes
static int pyin_pass(kwy_ctx *ctx, const kwy_f0_job *jobs, int count, const pyin_cfg &c, int fs, double f0_floor,
                     double frame_period_ms, double pa, const double *trans, const double *freq, char *scratch,
                     size_t block, int64_t T_max, int *spare) {
  pyin_table tb{};
  tb.n = count;
  for (int u = 0; u < count; ++u) {
    const kwy_f0_job &q = jobs[u];
    const int T = (int)kwy_dio_frames(fs, q.x_length, frame_period_ms);
    char *base = scratch + (size_t)u * block;
    tb.u[u] = pyin_view{q.x, q.temporal_positions, q.f0, q.status ? (int *)q.status : spare + u, (double *)base,
                        (unsigned short *)(base + kwy_pad(sizeof(double) * (size_t)T_max * (c.nb + 1))), (int)q.x_length, T};
    tb.start[u + 1] = tb.start[u] + T;
  }
  KWY_TRY(pyin_clear(ctx, tb));
  KWY_TRY(pyin_launch_observe(ctx, tb, c, fs, f0_floor, frame_period_ms, pa));
  return pyin_launch_decode(ctx, tb, c.nb, c.R, trans, freq);
}

static int pyin_check_jobs(kwy_ctx *ctx, const kwy_f0_job *jobs, int count, int fs, double frame_period_ms,
                           int64_t *T_max) {
  if (!jobs || count < 1 || fs <= 0 || !(frame_period_ms > 0)) { ctx->err = "pyin: bad argument"; return KWY_EINVAL; }
  *T_max = 0;
  for (int i = 0; i < count; ++i) {
    const kwy_f0_job &q = jobs[i];
    if (!q.x || !q.temporal_positions || !q.f0 || q.x_length <= 0 || q.x_length > 0x3fffffff) {
      ctx->err = "pyin: bad argument";
      return KWY_EINVAL;
    }
    const int64_t T = kwy_dio_frames(fs, q.x_length, frame_period_ms);
    if (T < 1 || T > 0x3fffffff) { ctx->err = "pyin: bad argument"; return KWY_EINVAL; }
    *T_max = T > *T_max ? T : *T_max;
  }
  return KWY_OK;
}

extern "C" int kwy_pyin_batch_dev(kwy_ctx *ctx, const kwy_f0_job *jobs, int count, int fs, double f0_floor,
                                  double f0_ceil, double frame_period_ms, double p_a, double switch_prob,
                                  double max_rate) {
  if (!ctx) return KWY_EINVAL;
  int64_t T_max;
  KWY_TRY(pyin_check_jobs(ctx, jobs, count, fs, frame_period_ms, &T_max));
  pyin_cfg c;
  KWY_TRY(pyin_config(ctx, fs, f0_floor, f0_ceil, frame_period_ms, max_rate, &c));
  if (!(p_a >= 0.0 && p_a <= 1.0)) { ctx->err = "pyin: p_a lies within [0, 1]"; return KWY_EINVAL; }
  KWY_HIP(hipSetDevice(ctx->device));
  const double *trans, *freq;
  KWY_TRY(pyin_tables(ctx, c, f0_floor, switch_prob, &trans, &freq));
  const size_t block = pyin_block_bytes(T_max, c.nb);
  const int per_pass = count < PYIN_BATCH ? count : PYIN_BATCH;
  KWY_TRY(kwy_arena_begin(ctx, kwy_pyin_scratch_bytes(T_max, c.nb, count)));
  char *scratch = (char *)kwy_arena_alloc(ctx, block * per_pass);
  int *spare = kwy_arena<int>(ctx, PYIN_BATCH);
  if (!scratch || !spare) { ctx->err = "pyin: scratch arena too small"; return KWY_ENOMEM; }
  // (the passes of a call share the scratch: they run one after the other on the context's stream)
  for (int i0 = 0; i0 < count; i0 += PYIN_BATCH)
    KWY_TRY(pyin_pass(ctx, jobs + i0, count - i0 < PYIN_BATCH ? count - i0 : PYIN_BATCH, c, fs, f0_floor,
                      frame_period_ms, p_a, trans, freq, scratch, block, T_max, spare));
  return KWY_OK;
}

extern "C" int kwy_pyin_dev(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor, double f0_ceil,
                            double frame_period_ms, double p_a, double switch_prob, double max_rate,
                            double *temporal_positions, double *f0, int32_t *status) {
  const kwy_f0_job job = {x, x_length, temporal_positions, f0, status};
  return kwy_pyin_batch_dev(ctx, &job, 1, fs, f0_floor, f0_ceil, frame_period_ms, p_a, switch_prob, max_rate);
}

// host pointers: the same pass on staged copies (a batch of one), synchronous
extern "C" int kwy_pyin(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor, double f0_ceil,
                        double frame_period_ms, double p_a, double switch_prob, double max_rate,
                        double *temporal_positions, double *f0) {
  if (!ctx) return KWY_EINVAL;
  kwy_f0_job job = {x, x_length, temporal_positions, f0, nullptr};
  int64_t T;
  KWY_TRY(pyin_check_jobs(ctx, &job, 1, fs, frame_period_ms, &T));
  pyin_cfg c;
  KWY_TRY(pyin_config(ctx, fs, f0_floor, f0_ceil, frame_period_ms, max_rate, &c));
  if (!(p_a >= 0.0 && p_a <= 1.0)) { ctx->err = "pyin: p_a lies within [0, 1]"; return KWY_EINVAL; }
  KWY_HIP(hipSetDevice(ctx->device));
  const double *trans, *freq;
  KWY_TRY(pyin_tables(ctx, c, f0_floor, switch_prob, &trans, &freq));
  const size_t block = pyin_block_bytes(T, c.nb);
  kwy_staging st(ctx, "pyin");
  int *dstatus, hstatus = 0;
  st.in(job.x, x, (size_t)x_length);
  st.out(job.temporal_positions, temporal_positions, (size_t)T);
  st.out(job.f0, f0, (size_t)T);
  st.tmp(dstatus, PYIN_BATCH);
  KWY_TRY(st.begin(kwy_pad(block)));
  char *scratch = (char *)kwy_arena_alloc(ctx, block);
  if (!scratch) { ctx->err = "pyin: scratch arena too small"; return KWY_ENOMEM; }
  KWY_TRY(pyin_pass(ctx, &job, 1, c, fs, f0_floor, frame_period_ms, p_a, trans, freq, scratch, block, T, dstatus));
  st.fetch(dstatus, &hstatus, 1);
  KWY_TRY(st.finish());
  if (hstatus != 0) { ctx->err = "pyin: a sample of the signal is not finite"; return KWY_EINVAL; }
  return KWY_OK;
}

// ---- the two stages on their own -------------------------------------------------------------------------------
static int pyin_observe_core(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor,
                             double frame_period_ms, double p_a, const pyin_cfg &c, int64_t T, double *L, int *status) {
  pyin_table tb{};
  tb.n = 1;
  tb.u[0] = pyin_view{x, nullptr, nullptr, status, L, nullptr, (int)x_length, (int)T};
  tb.start[1] = (int)T;
  KWY_TRY(pyin_clear(ctx, tb));
  return pyin_launch_observe(ctx, tb, c, fs, f0_floor, frame_period_ms, p_a);
}

static int pyin_observe_args(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor, double f0_ceil,
                             double frame_period_ms, double p_a, const double *L, pyin_cfg *c, int64_t *T) {
  if (!x || !L || x_length <= 0 || x_length > 0x3fffffff || fs <= 0 || !(frame_period_ms > 0) ||
      !(p_a >= 0.0 && p_a <= 1.0)) {
    ctx->err = "pyin_observe: bad argument";
    return KWY_EINVAL;
  }
  KWY_TRY(pyin_config(ctx, fs, f0_floor, f0_ceil, frame_period_ms, 0.0, c));
  *T = kwy_dio_frames(fs, x_length, frame_period_ms);
  if (*T < 1 || *T > 0x3fffffff) { ctx->err = "pyin_observe: bad argument"; return KWY_EINVAL; }
  KWY_HIP(hipSetDevice(ctx->device));
  return KWY_OK;
}

extern "C" int kwy_pyin_observe_dev(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor,
                                    double f0_ceil, double frame_period_ms, double p_a, double *L, int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  pyin_cfg c;
  int64_t T;
  KWY_TRY(pyin_observe_args(ctx, x, x_length, fs, f0_floor, f0_ceil, frame_period_ms, p_a, L, &c, &T));
  int *st = (int *)status;
  if (!st) {
    KWY_TRY(kwy_arena_begin(ctx, kwy_pad(sizeof(int))));
    st = kwy_arena<int>(ctx, 1);
    if (!st) { ctx->err = "pyin_observe: scratch arena too small"; return KWY_ENOMEM; }
  }
  return pyin_observe_core(ctx, x, x_length, fs, f0_floor, frame_period_ms, p_a, c, T, L, st);
}

extern "C" int kwy_pyin_observe(kwy_ctx *ctx, const double *x, int64_t x_length, int fs, double f0_floor, double f0_ceil,
                                double frame_period_ms, double p_a, double *L) {
  if (!ctx) return KWY_EINVAL;
  pyin_cfg c;
  int64_t T;
  KWY_TRY(pyin_observe_args(ctx, x, x_length, fs, f0_floor, f0_ceil, frame_period_ms, p_a, L, &c, &T));
  kwy_staging st(ctx, "pyin_observe");
  const double *dx;
  double *dL;
  int *dstatus, hstatus = 0;
  st.in(dx, x, (size_t)x_length);
  st.out(dL, L, (size_t)T * (c.nb + 1));
  st.tmp(dstatus, 1);
  KWY_TRY(st.begin());
  KWY_TRY(pyin_observe_core(ctx, dx, x_length, fs, f0_floor, frame_period_ms, p_a, c, T, dL, dstatus));
  st.fetch(dstatus, &hstatus, 1);
  KWY_TRY(st.finish());
  if (hstatus != 0) { ctx->err = "pyin: a sample of the signal is not finite"; return KWY_EINVAL; }
  return KWY_OK;
}

static int pyin_decode_args(kwy_ctx *ctx, const double *L, int64_t T, int nb, const double *trans, int R,
                            const double *freq, const double *f0) {
  if (!L || !trans || !freq || !f0 || T < 1 || T > 0x3fffffff || nb < 1 || R < 0 || R > PYIN_MAX_RADIUS) {
    ctx->err = "pyin_decode: bad argument";
    return KWY_EINVAL;
  }
  if (2 * nb > PYIN_MAX_STATES) { ctx->err = "pyin_decode: more than 1024 states"; return KWY_EINVAL; }
  KWY_HIP(hipSetDevice(ctx->device));
  return KWY_OK;
}

static int pyin_decode_core(kwy_ctx *ctx, const double *L, int64_t T, int nb, const double *trans, int R,
                            const double *freq, double *f0, unsigned short *bp, int *status) {
  pyin_table tb{};
  tb.n = 1;
  tb.u[0] = pyin_view{nullptr, nullptr, f0, status, (double *)L, bp, 0, (int)T};
  tb.start[1] = (int)T;
  KWY_TRY(pyin_clear(ctx, tb));
  return pyin_launch_decode(ctx, tb, nb, R, trans, freq);
}

extern "C" int kwy_pyin_decode_dev(kwy_ctx *ctx, const double *L, int64_t T, int nb, const double *trans, int R,
                                   const double *freq, double *f0) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(pyin_decode_args(ctx, L, T, nb, trans, R, freq, f0));
  KWY_TRY(kwy_arena_begin(ctx, kwy_pyin_scratch_bytes(T, nb, 1)));
  unsigned short *bp = kwy_arena<unsigned short>(ctx, (size_t)T * 2 * nb);
  int *status = kwy_arena<int>(ctx, 1);
  if (!bp || !status) { ctx->err = "pyin_decode: scratch arena too small"; return KWY_ENOMEM; }
  return pyin_decode_core(ctx, L, T, nb, trans, R, freq, f0, bp, status);
}

extern "C" int kwy_pyin_decode(kwy_ctx *ctx, const double *L, int64_t T, int nb, const double *trans, int R,
                               const double *freq, double *f0) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(pyin_decode_args(ctx, L, T, nb, trans, R, freq, f0));
  kwy_staging st(ctx, "pyin_decode");
  const double *dL, *dtrans, *dfreq;
  double *df0;
  unsigned short *bp;
  int *dstatus;
  st.in(dL, L, (size_t)T * (nb + 1));
  st.in(dtrans, trans, (size_t)2 * (2 * R + 1));
  st.in(dfreq, freq, (size_t)nb);
  st.out(df0, f0, (size_t)T);
  st.tmp(bp, (size_t)T * 2 * nb);
  st.tmp(dstatus, 1);
  KWY_TRY(st.begin());
  KWY_TRY(pyin_decode_core(ctx, dL, T, nb, dtrans, R, dfreq, df0, bp, dstatus));
  return st.finish();
}
