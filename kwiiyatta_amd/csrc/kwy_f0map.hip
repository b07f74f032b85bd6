// kwy_f0map.hip -- f0 conversion: the voiced log-f0 moments of f0 tracks, their corpus merge, and the per-frame map
//
//   log f0' = (log f0 - mu_src) * sigma_tgt / sigma_src + mu_tgt        (voiced frames, f0 > 0)
//   f0'     = exp(log f0') * ratio,   ratio = 2 ** (key / 12)
//
// The key transposition is the reference dialog's `feature.f0 = feature.f0 * (2.0 ** (transposeKey / 12))`
// (kwiiyatta/view/qt/kwiieiya.py:152-155); the normalised log-Gaussian transform is the usual f0 conversion that goes
// with a GMM spectral converter (the reference converts the mel-cepstrum only, kwiiyatta/convert_voice.py:35-46).
//
// Reductions are deterministic: one workgroup per track, a thread's frames added in index order, then
// kwy_block_sum (DPP over the 64 lanes of a wave, the waves' partial sums in wave order through LDS).  A track's
// triple therefore depends on its own frames only -- not on the run, nor on the other tracks of the launch -- and
// the corpus merge is a left fold of Chan's pairwise combination in index order on one lane (k_moments_merge,
// kwy_eval.hip).
//
// No kernel here allocates, synchronises or uses the context's arena: the _dev entries are legal inside a stream
// capture.  The host entries stage through the arena and synchronise, as kwy_synthesize does.
#include <math.h>

#include "kwy_internal.hpp"

#define F0M_GROUP 32      // tracks per launch

struct f0m_track {
  const double *f0;
  int64_t n;
  double *out;            // (count, mean, M2)
};
typedef kwy_group<f0m_track, F0M_GROUP> f0m_tracks;

struct f0m_map {
  const double *in;
  int64_t n;
  double *out;
  int32_t *status;        // frames out of range (may be NULL)
};
typedef kwy_group<f0m_map, F0M_GROUP> f0m_maps;

// one workgroup per track: (n, mean, M2) of log f0 over the frames with f0 > 0, in two passes
__global__ __launch_bounds__(KWY_THREADS) void k_logf0_moments(f0m_tracks B) {
  __shared__ double red[KWY_WAVES];
  const f0m_track &U = B.u[blockIdx.x];
  const int tid = threadIdx.x;
  double cnt = 0.0, sum = 0.0;
  for (int64_t i = tid; i < U.n; i += KWY_THREADS) {
    const double f = U.f0[i];
    if (f > 0.0) {
      cnt += 1.0;
      sum += kwy_log(f);
    }
  }
  cnt = kwy_block_sum(cnt, red);
  sum = kwy_block_sum(sum, red);
  const double mean = cnt > 0.0 ? sum / cnt : 0.0;
  double m2 = 0.0;
  for (int64_t i = tid; i < U.n; i += KWY_THREADS) {
    const double f = U.f0[i];
    if (f > 0.0) {
      const double d = kwy_log(f) - mean;
      m2 += d * d;
    }
  }
  m2 = kwy_block_sum(m2, red);
  if (tid == 0) {
    U.out[0] = cnt;
    U.out[1] = mean;
    U.out[2] = m2;
  }
}

// one workgroup per track; stats == NULL: voiced f0 * ratio (the dialog's product, bit for bit)
__global__ __launch_bounds__(KWY_THREADS) void k_f0_map(f0m_maps B, const double *__restrict__ stats, double ratio,
                                                         double limit) {
  __shared__ double red[KWY_WAVES];
  const f0m_map &U = B.u[blockIdx.x];
  const int tid = threadIdx.x;
  double ms = 0.0, ss = 1.0, mt = 0.0, st = 1.0;
  if (stats) { ms = stats[0]; ss = stats[1]; mt = stats[2]; st = stats[3]; }
  double bad = 0.0;
  for (int64_t i = tid; i < U.n; i += KWY_THREADS) {
    const double f = U.in[i];
    double y;
    if (f > 0.0 && stats) y = exp((kwy_log(f) - ms) * st / ss + mt) * ratio;
    else if (stats) y = f;                     // unvoiced (0) as it is
    else y = f * ratio;
    U.out[i] = y;
    // negative or non-finite input, or an output at or beyond the limit (a NaN output fails `y < limit`)
    if (!kwy_finite_nonneg(f) || !(y < limit)) bad += 1.0;
  }
  bad = kwy_block_sum(bad, red);
  if (tid == 0 && U.status) *U.status = (int32_t)fmin(bad, 2147483647.0);
}

static int f0m_check_tracks(kwy_ctx *ctx, const kwy_f0_track *tracks, int count, const double *moments) {
  if (!tracks || count < 1 || !moments) { ctx->err = "logf0_moments: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i)
    if (tracks[i].length < 0 || (tracks[i].length > 0 && !tracks[i].f0)) {
      ctx->err = "logf0_moments: bad argument";
      return KWY_EINVAL;
    }
  return KWY_OK;
}

static int f0m_launch_moments(kwy_ctx *ctx, const kwy_f0_track *tracks, int count, double *moments) {
  return kwy_for_tables<f0m_tracks>(
      count, [&](int i) { return f0m_track{tracks[i].f0, tracks[i].length, moments + 3 * (int64_t)i}; },
      [&](const f0m_tracks &B, int) {
        KWY_PROF(ctx, "k_logf0_moments",
                 hipLaunchKernelGGL(k_logf0_moments, dim3(B.n), dim3(KWY_THREADS), 0, ctx->stream, B));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

extern "C" int kwy_logf0_moments_batch_dev(kwy_ctx *ctx, const kwy_f0_track *tracks, int count, double *moments) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(f0m_check_tracks(ctx, tracks, count, moments));
  KWY_HIP(hipSetDevice(ctx->device));
  return f0m_launch_moments(ctx, tracks, count, moments);
}

// the corpus merge: kwy_eval.hip's fold (Chan's pairwise combination, left to right) over one column of triples
extern "C" int kwy_logf0_moments_merge_dev(kwy_ctx *ctx, const double *moments, int count, double *out) {
  return kwy_moments_merge_dev(ctx, moments, count, 1, out);
}

extern "C" int kwy_logf0_moments(kwy_ctx *ctx, const kwy_f0_track *tracks, int count, double *moments) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(f0m_check_tracks(ctx, tracks, count, moments));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "logf0_moments");
  double *dm;
  st.out(dm, moments, 3 * (size_t)count);
  std::vector<kwy_f0_track> staged(tracks, tracks + count);
  for (int i = 0; i < count; ++i) st.in(staged[i].f0, tracks[i].f0, (size_t)tracks[i].length);
  KWY_TRY(st.begin());
  KWY_TRY(f0m_launch_moments(ctx, staged.data(), count, dm));
  return st.finish();
}

extern "C" int kwy_logf0_moments_merge(kwy_ctx *ctx, const double *moments, int count, double *out) {
  return kwy_moments_merge(ctx, moments, count, 1, out);
}

static int f0m_check_maps(kwy_ctx *ctx, const kwy_f0_map_job *jobs, int count, int fs, double ratio) {
  if (!jobs || count < 1 || fs <= 0 || !(ratio > 0.0 && ratio < INFINITY)) {
    ctx->err = "f0_map: bad argument";
    return KWY_EINVAL;
  }
  for (int i = 0; i < count; ++i)
    if (jobs[i].length < 0 || (jobs[i].length > 0 && (!jobs[i].f0_in || !jobs[i].f0_out))) {
      ctx->err = "f0_map: bad argument";
      return KWY_EINVAL;
    }
  return KWY_OK;
}

static int f0m_launch_map(kwy_ctx *ctx, const kwy_f0_map_job *jobs, int count, int fs, const double *stats,
                          double ratio, int32_t *status) {
  const double limit = fs / 8.0;   // kwy_synth.hip's pulse capacity (y_length / 8 + 16) holds every such track
  return kwy_for_tables<f0m_maps>(
      count,
      [&](int i) { return f0m_map{jobs[i].f0_in, jobs[i].length, jobs[i].f0_out, status ? status + i : nullptr}; },
      [&](const f0m_maps &B, int) {
        KWY_PROF(ctx, "k_f0_map",
                 hipLaunchKernelGGL(k_f0_map, dim3(B.n), dim3(KWY_THREADS), 0, ctx->stream, B, stats, ratio, limit));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

extern "C" int kwy_f0_map_batch_dev(kwy_ctx *ctx, const kwy_f0_map_job *jobs, int count, int fs, const double *stats,
                                    double ratio, int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(f0m_check_maps(ctx, jobs, count, fs, ratio));
  KWY_HIP(hipSetDevice(ctx->device));
  return f0m_launch_map(ctx, jobs, count, fs, stats, ratio, status);
}

extern "C" int kwy_f0_map(kwy_ctx *ctx, const kwy_f0_map_job *jobs, int count, int fs, const double *stats,
                          double ratio, int32_t *status) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(f0m_check_maps(ctx, jobs, count, fs, ratio));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "f0_map");
  double *dstats;
  int32_t *dstatus;
  st.in(dstats, stats, 4);
  st.out(dstatus, status, (size_t)count);
  std::vector<kwy_f0_map_job> staged(jobs, jobs + count);
  for (int i = 0; i < count; ++i) {
    st.in(staged[i].f0_in, jobs[i].f0_in, (size_t)jobs[i].length);
    st.out(staged[i].f0_out, jobs[i].f0_out, (size_t)jobs[i].length);
  }
  KWY_TRY(st.begin());
  KWY_TRY(f0m_launch_map(ctx, staged.data(), count, fs, stats ? dstats : nullptr, ratio, dstatus));
  return st.finish();
}
