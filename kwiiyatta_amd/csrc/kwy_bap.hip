// kwy_bap.hip -- band-aperiodicity conversion on gfx950: the aperiodic component as a stream of the joint-density GMM
// conversion (Ohtani et al. 2006; the `codeap` mixture of sprocket), the contract being include/kwy.h, "aperiodicity
// conversion".  Four pieces around the generic fit and the prepared-model MLPG conversion:
//
//   kwy_bap_track_*   ap (T x K) -> S (T x (B + 1)): the voicing flag of the band codec's decoder and the coded bands,
//                     unvoiced frames holding the row of the nearest voiced frame before them (the leading run: after)
//   kwy_bap_rows_*    the joint rows [gx, dgx, ddgx | gy, dgy, ddgy] of an aligned pair's cells that are voiced on both
//                     sides, appended in order behind a device cursor
//   kwy_bap_apply_*   the converted bands decoded over the voiced rows of the analysed aperiodicity, in place
//   kwy_bap_error_*   (n, mean, M2) of the per-cell band error over the cells voiced on both sides
//
// The band codec's arithmetic is kwy_band_code() / kwy_band_decode_bin() of kwy_device.hpp, which kwy_codec.hip calls too.
//
// Nothing here allocates or synchronises in the _dev forms; kwy_bap_rows_batch_dev takes 8 bytes per pair from the
// context's arena (the pairs' places in the matrix), as kwy_train_rows_batch_dev does.
#include <math.h>

#include <algorithm>

#include "kwy_internal.hpp"

#define BAP_NT KWY_THREADS
#define BAP_PASS BAP_NT               // frames per pass of the track kernel: one thread per frame in the fill
#define BAP_GROUP 16                  // jobs per launch

// ---- band track ------------------------------------------------------------------------------------------------------
struct bap_track_view { const double *ap; int64_t T; double *track; };
typedef kwy_group<bap_track_view, BAP_GROUP> bap_track_table;

// One workgroup per utterance, BAP_PASS frames a pass.  Of a pass: the (frame, band) pairs are coded across the lanes
// (pair p = frame p / B, band p % B: every lane works where k_code_aperiodicity keeps 5 of 64 busy); a thread per frame
// folds its bands into the voicing flag; an inclusive max-scan over "index of the last voiced frame" tells every
// unvoiced frame whose row it holds, the frames before the pass's first voiced one taking the row carried over from
// the passes before; the rows go out with (frame, column) pairs across the lanes.  Frames in front of the utterance's
// first voiced frame are written as coded and overwritten with that frame's row at the end (the leading run); without
// any voiced frame they stay as coded.
__global__ __launch_bounds__(BAP_NT) void k_bap_track(bap_track_table tab, int fs, int fft_size, int B) {
  __shared__ double s_c[BAP_PASS * KWY_BAND_MAX];     // the pass's coded values
  __shared__ int s_last[2][BAP_PASS];                  // max-scan buffers: local index of the last voiced frame, or -1
  __shared__ double s_carry[KWY_BAND_MAX];            // the row of the last voiced frame of the passes before
  __shared__ double s_lead[KWY_BAND_MAX];             // the row of the utterance's first voiced frame
  __shared__ int s_have_carry;
  __shared__ long long s_first;                        // index of the utterance's first voiced frame, or -1
  const bap_track_view &U = tab.u[blockIdx.x];
  const int tid = threadIdx.x, K = fft_size / 2 + 1, W = B + 1;
  if (tid == 0) { s_have_carry = 0; s_first = -1; }
  __syncthreads();
  for (int64_t t0 = 0; t0 < U.T; t0 += BAP_PASS) {
    const int F = (int)(U.T - t0 < BAP_PASS ? U.T - t0 : BAP_PASS);
    for (int p = tid; p < F * B; p += BAP_NT) {
      const int f = p / B, b = p - f * B;
      s_c[f * B + b] = kwy_band_code(U.ap + (t0 + f) * K, K, fs, fft_size, b);
    }
    __syncthreads();
    // the decoder's test (k_decode_aperiodicity): a left fold, b ascending, compared with > -0.5
    bool voiced = false;
    if (tid < F) {
      double tmp = 0.0;
      for (int b = 0; b < B; ++b) tmp += s_c[tid * B + b];
      voiced = !(tmp / B > -0.5);
    }
    int cur = 0;
    s_last[0][tid] = voiced ? tid : -1;
    __syncthreads();
    for (int step = 1; step < BAP_PASS; step <<= 1) {
      const int mine = s_last[cur][tid], other = tid >= step ? s_last[cur][tid - step] : -1;
      s_last[cur ^ 1][tid] = mine > other ? mine : other;
      cur ^= 1;
      __syncthreads();
    }
    const int *last = s_last[cur];
    const bool had_carry = s_have_carry != 0;
    // the utterance's first voiced frame: voiced, nothing voiced before it in the pass nor in the passes before
    if (voiced && !had_carry && (tid == 0 || last[tid - 1] < 0)) {
      s_first = t0 + tid;
      for (int b = 0; b < B; ++b) s_lead[b] = s_c[tid * B + b];
    }
    for (int q = tid; q < F * W; q += BAP_NT) {
      const int f = q / W, col = q - f * W, src = last[f];
      double v;
      if (col == 0) v = src == f ? 1.0 : 0.0;
      else if (src >= 0) v = s_c[src * B + col - 1];
      else if (had_carry) v = s_carry[col - 1];
      else v = s_c[f * B + col - 1];                   // (in front of the first voiced frame: as coded, for now)
      U.track[t0 * W + q] = v;
    }
    __syncthreads();
    const int tail = last[F - 1];
    if (tail >= 0) {
      if (tid < B) s_carry[tid] = s_c[tail * B + tid];
      if (tid == 0) s_have_carry = 1;
    }
    __syncthreads();
  }
  const int64_t first = s_first;
  for (int64_t q = tid; q < first * B; q += BAP_NT) {
    const int64_t f = q / B;
    const int b = (int)(q - f * B);
    U.track[f * W + 1 + b] = s_lead[b];
  }
}

// ---- training rows ---------------------------------------------------------------------------------------------------
struct bap_rows_view {
  const double *tx, *ty;
  const int32_t *ix, *iy;
  const int64_t *n_dev;
  int64_t *n_rows;
  int64_t x_rows, y_rows, capacity;
};
typedef kwy_group<bap_rows_view, BAP_GROUP> bap_rows_table;

__device__ __forceinline__ bool bap_cell_kept(const bap_rows_view &U, int W, int64_t k) {
  const int64_t rx = kwy_clamp_row(U.ix[k], U.x_rows), ry = kwy_clamp_row(U.iy[k], U.y_rows);
  return U.tx[rx * W] == 1.0 && U.ty[ry * W] == 1.0;
}

// Cell k of a pair is kept when both sides are voiced there; WRITE: the kept cells' rows go to `joint` in order, the
// delta features taken over the gathered sequences of ALL n cells as k_tr_delta takes them (kwy_delta_windows) --
// else they are counted into n_rows.  One workgroup per pair, BAP_NT cells a round.
template <bool WRITE>
__device__ __forceinline__ void bap_rows_body(const bap_rows_view &U, int B, double *__restrict__ joint) {
  __shared__ int sh[BAP_NT / 64];
  __shared__ int s_dst[BAP_NT];
  const int tid = threadIdx.x, W = B + 1, D = 3 * B;
  const int64_t n = kwy_device_count(U.capacity, U.n_dev);
  int64_t run = 0;
  for (int64_t k0 = 0; k0 < n; k0 += BAP_NT) {
    const int64_t k = k0 + tid;
    const int keep = (k < n && bap_cell_kept(U, W, k)) ? 1 : 0;
    int tot;
    const int off = kwy_block_exscan<BAP_NT>(keep, sh, &tot);
    if (WRITE) {
      s_dst[tid] = keep ? off : -1;
      __syncthreads();
      const int cells = (int)(n - k0 < BAP_NT ? n - k0 : BAP_NT);
      for (int q = tid; q < cells * 2 * B; q += BAP_NT) {
        const int c = q / (2 * B), e = q - c * 2 * B, side = e / B, b = e - side * B;
        if (s_dst[c] < 0) continue;
        const int64_t kk = k0 + c;
        const double *__restrict__ tr = side ? U.ty : U.tx;
        const int32_t *__restrict__ idx = side ? U.iy : U.ix;
        const int64_t rows = side ? U.y_rows : U.x_rows;
        const double x0 = tr[kwy_clamp_row(idx[kk], rows) * W + 1 + b];
        const double xm = kk > 0 ? tr[kwy_clamp_row(idx[kk - 1], rows) * W + 1 + b] : 0.0;
        const double xp = kk + 1 < n ? tr[kwy_clamp_row(idx[kk + 1], rows) * W + 1 + b] : 0.0;
        double *o = joint + (size_t)(run + s_dst[c]) * 2 * D + side * D;
        o[b] = x0;
        kwy_delta_windows(xm, x0, xp, &o[B + b], &o[2 * B + b]);
      }
      __syncthreads();
    }
    run += tot;
  }
  if (!WRITE && tid == 0) U.n_rows[0] = run;
}

__global__ __launch_bounds__(BAP_NT) void k_bap_rows_count(bap_rows_table tab, int B) {
  bap_rows_body<false>(tab.u[blockIdx.x], B, nullptr);
}
__global__ void k_bap_rows_place(bap_rows_table tab, int64_t *__restrict__ cursor, int64_t capacity_rows,
                                 int64_t *__restrict__ places) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  kwy_place_rows(tab.n, [&](int k) { return tab.u[k].n_rows; }, cursor, capacity_rows, places);
}
__global__ __launch_bounds__(BAP_NT) void k_bap_rows_write(bap_rows_table tab, int B, double *__restrict__ joint,
                                                          const int64_t *__restrict__ places) {
  const int64_t at = places[blockIdx.x];
  if (at < 0) return;
  bap_rows_body<true>(tab.u[blockIdx.x], B, joint + (size_t)at * 6 * B);
}

// ---- apply -----------------------------------------------------------------------------------------------------------
struct bap_apply_view { const double *src, *conv; double *ap; };
typedef kwy_batch<bap_apply_view, BAP_GROUP> bap_apply_table;
static_assert(sizeof(bap_apply_table) + 64 <= KWY_KERNARG_MAX, "the apply kernel's arguments must fit the launch");

// One workgroup per frame of the batch, as k_decode_aperiodicity has it: a frame that is voiced in the source's track
// becomes the decode of its converted bands, clamped to [-60, -1e-12] dB; any other frame is not touched.
__global__ __launch_bounds__(BAP_NT) void k_bap_apply(bap_apply_table tab, int fs, int fft_size, int nb) {
  __shared__ double coarse[KWY_BAND_MAX + 2];
  __shared__ int s_unvoiced;
  const int u = tab.find(blockIdx.x);
  const bap_apply_view &U = tab.u[u];
  const int64_t frame = (int64_t)blockIdx.x - tab.start[u];
  const int tid = threadIdx.x, K = fft_size / 2 + 1, W = nb + 1;
  if (U.src[frame * W] != 1.0) return;                 // (uniform over the workgroup)
  double *o = U.ap + frame * K;
  if (tid == 0) {
    double tmp = 0.0;
    for (int i = 0; i < nb; ++i) {
      double v = U.conv[frame * W + 1 + i];
      v = v < KWY_BAND_FLOOR ? KWY_BAND_FLOOR : (v > -KWY_SAFE ? -KWY_SAFE : v);
      tmp += v;
      coarse[i + 1] = v;
    }
    coarse[0] = KWY_BAND_FLOOR;
    coarse[nb + 1] = -KWY_SAFE;
    s_unvoiced = nb <= 0 || (tmp / nb > -0.5);
  }
  __syncthreads();
  if (s_unvoiced) {
    for (int k = tid; k < K; k += BAP_NT) o[k] = 1.0 - KWY_SAFE;
    return;
  }
  for (int k = tid; k < K; k += BAP_NT) o[k] = kwy_band_decode_bin(coarse, fs, fft_size, nb, k);
}

// ---- band error ------------------------------------------------------------------------------------------------------
struct bap_error_view {
  const double *a, *b;
  const int32_t *ia, *ib;
  const int64_t *n_dev;
  double *per_row;
  double *moments;
  int64_t a_rows, b_rows, off_a, off_b, rows;
};
typedef kwy_group<bap_error_view, BAP_GROUP> bap_error_table;

// One workgroup per job, modelled on k_eval_f0 (kwy_eval.hip): a thread's cells in index order, the threads' sums
// through kwy_block_sum, M2 in a second pass about the mean of the first.
__global__ __launch_bounds__(BAP_NT) void k_bap_error(bap_error_table tab, int B) {
  __shared__ double red[KWY_WAVES];
  const bap_error_view &U = tab.u[blockIdx.x];
  const int tid = threadIdx.x, W = B + 1;
  const int64_t n = kwy_device_count(U.rows, U.n_dev);
  double cnt = 0.0, sum = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    const double mean = cnt > 0.0 ? sum / cnt : 0.0;
    double c_cnt = 0.0, acc = 0.0;
    for (int64_t t = tid; t < n; t += BAP_NT) {
      const int64_t ra = (U.ia ? (int64_t)U.ia[t] : t) - U.off_a, rb = (U.ib ? (int64_t)U.ib[t] : t) - U.off_b;
      const bool inside = ra >= 0 && ra < U.a_rows && rb >= 0 && rb < U.b_rows;
      const bool use = inside && U.a[ra * W] == 1.0 && U.b[rb * W] == 1.0;
      double v = __builtin_nan("");
      if (use) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) {
          const double d = U.a[ra * W + 1 + b] - U.b[rb * W + 1 + b];
          s += d * d;
        }
        v = sqrt(s / B);
        if (pass == 0) acc += v;
        else acc += (v - mean) * (v - mean);
        c_cnt += 1.0;
      }
      if (pass == 0 && U.per_row) U.per_row[t] = v;
    }
    if (pass == 0) {
      cnt = kwy_block_sum(c_cnt, red);
      sum = kwy_block_sum(acc, red);
    } else {
      const double m2 = kwy_block_sum(acc, red);
      if (tid == 0) {
        U.moments[0] = cnt;
        U.moments[1] = mean;
        U.moments[2] = m2;
      }
    }
  }
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------
// what every entry needs of (fs, fft_size): an even transform length and a rate with at least one band.  (The bins the
// coder reads need no check of their own: the highest band centre, 3000 B <= fs / 2 - 3000, lies below the last bin.)
static int bap_check_rate(kwy_ctx *ctx, const char *who, int fs, int fft_size, int *bands) {
  if (fs <= 0 || fft_size < 4 || (fft_size & 1)) { ctx->err = std::string(who) + ": bad argument"; return KWY_EINVAL; }
  const int B = kwy_aperiodicity_bands(fs);
  if (B < 1) {
    ctx->err = std::string(who) + ": the sampling rate has no aperiodicity band (it takes 12 kHz or more)";
    return KWY_EINVAL;
  }
  if (B > KWY_BAND_MAX) { ctx->err = std::string(who) + ": too many bands"; return KWY_EINVAL; }
  *bands = B;
  return KWY_OK;
}

static int bap_check_bands(kwy_ctx *ctx, const char *who, int B) {
  if (B < 1 || B > KWY_BAND_MAX) {
    ctx->err = std::string(who) + ": the band count must be within [1, 8] (a rate of 12 kHz or more)";
    return KWY_EINVAL;
  }
  return KWY_OK;
}

static int bap_track_check(kwy_ctx *ctx, const kwy_bap_track_job *jobs, int count, int fs, int fft_size, int *B) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(bap_check_rate(ctx, "bap_track", fs, fft_size, B));
  if (!jobs || count < 0) { ctx->err = "bap_track: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i)
    if (!jobs[i].ap || !jobs[i].track || jobs[i].T <= 0) { ctx->err = "bap_track: bad argument"; return KWY_EINVAL; }
  return KWY_OK;
}

static int bap_track_launch(kwy_ctx *ctx, const kwy_bap_track_job *jobs, int count, int fs, int fft_size, int B) {
  return kwy_for_tables<bap_track_table>(
      count, [&](int i) { return bap_track_view{jobs[i].ap, jobs[i].T, jobs[i].track}; },
      [&](const bap_track_table &t, int) {
        KWY_PROF(ctx, "k_bap_track",
                 hipLaunchKernelGGL(k_bap_track, dim3(t.n), dim3(BAP_NT), 0, ctx->stream, t, fs, fft_size, B));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

extern "C" int kwy_bap_track_batch_dev(kwy_ctx *ctx, const kwy_bap_track_job *jobs, int count, int fs, int fft_size) {
  int B = 0;
  KWY_TRY(bap_track_check(ctx, jobs, count, fs, fft_size, &B));
  if (count == 0) return KWY_OK;
  KWY_HIP(hipSetDevice(ctx->device));
  return bap_track_launch(ctx, jobs, count, fs, fft_size, B);
}

extern "C" int kwy_bap_track_dev(kwy_ctx *ctx, const double *ap, int64_t T, int fs, int fft_size, double *track) {
  const kwy_bap_track_job job = {ap, T, track};
  return kwy_bap_track_batch_dev(ctx, &job, 1, fs, fft_size);
}

extern "C" int kwy_bap_track(kwy_ctx *ctx, const kwy_bap_track_job *jobs, int count, int fs, int fft_size) {
  int B = 0;
  KWY_TRY(bap_track_check(ctx, jobs, count, fs, fft_size, &B));
  if (count == 0) return KWY_OK;
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "bap_track");
  std::vector<kwy_bap_track_job> staged(jobs, jobs + count);
  for (int i = 0; i < count; ++i) {
    st.in(staged[i].ap, jobs[i].ap, (size_t)jobs[i].T * (fft_size / 2 + 1));
    st.out(staged[i].track, jobs[i].track, (size_t)jobs[i].T * (B + 1));
  }
  KWY_TRY(st.begin());
  KWY_TRY(bap_track_launch(ctx, staged.data(), count, fs, fft_size, B));
  return st.finish();
}

static int bap_rows_check(kwy_ctx *ctx, const kwy_bap_rows_job *jobs, int count, int B, const double *joint,
                          int64_t capacity_rows, const int64_t *cursor, bool host) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(bap_check_bands(ctx, "bap_rows", B));
  if (!jobs || count < 0 || !joint || capacity_rows < 0 || !cursor) { ctx->err = "bap_rows: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i) {
    const kwy_bap_rows_job &j = jobs[i];
    const bool lists = j.capacity == 0 || (j.idx_x && j.idx_y && j.track_x && j.track_y && j.x_rows > 0 && j.y_rows > 0);
    if (j.capacity < 0 || !lists || !j.n_rows || (host && j.n_dev)) {
      ctx->err = host && j.n_dev ? "bap_rows: the host form takes its cell count by value" : "bap_rows: bad argument";
      return KWY_EINVAL;
    }
  }
  return KWY_OK;
}

// `places`: BAP_GROUP words of device scratch per launch, handed out by `next_places`
template <class PLACES>
static int bap_rows_launch(kwy_ctx *ctx, const kwy_bap_rows_job *jobs, int count, int B, double *joint,
                           int64_t capacity_rows, int64_t *cursor, PLACES next_places) {
  return kwy_for_tables<bap_rows_table>(
      count,
      [&](int i) {
        const kwy_bap_rows_job &j = jobs[i];
        return bap_rows_view{j.track_x, j.track_y, j.idx_x, j.idx_y, j.n_dev, j.n_rows, j.x_rows, j.y_rows, j.capacity};
      },
      [&](const bap_rows_table &t, int) {
        int64_t *places = next_places();
        if (!places) { ctx->err = "bap_rows: scratch"; return KWY_ENOMEM; }
        KWY_PROF(ctx, "k_bap_rows_count",
                 hipLaunchKernelGGL(k_bap_rows_count, dim3(t.n), dim3(BAP_NT), 0, ctx->stream, t, B));
        KWY_HIP(hipGetLastError());
        KWY_PROF(ctx, "k_bap_rows_place", hipLaunchKernelGGL(k_bap_rows_place, dim3(1), dim3(64), 0, ctx->stream, t, cursor,
                                                             capacity_rows, places));
        KWY_HIP(hipGetLastError());
        KWY_PROF(ctx, "k_bap_rows_write",
                 hipLaunchKernelGGL(k_bap_rows_write, dim3(t.n), dim3(BAP_NT), 0, ctx->stream, t, B, joint, places));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

static inline size_t bap_launches(int count) { return (size_t)((count + BAP_GROUP - 1) / BAP_GROUP); }

extern "C" int kwy_bap_rows_batch_dev(kwy_ctx *ctx, const kwy_bap_rows_job *jobs, int count, int B, double *joint,
                                      int64_t capacity_rows, int64_t *cursor) {
  KWY_TRY(bap_rows_check(ctx, jobs, count, B, joint, capacity_rows, cursor, false));
  if (count == 0) return KWY_OK;
  KWY_HIP(hipSetDevice(ctx->device));
  KWY_TRY(kwy_arena_begin(ctx, kwy_pad(sizeof(int64_t) * BAP_GROUP) * bap_launches(count)));
  return bap_rows_launch(ctx, jobs, count, B, joint, capacity_rows, cursor,
                         [&]() { return kwy_arena<int64_t>(ctx, BAP_GROUP); });
}

extern "C" int kwy_bap_rows(kwy_ctx *ctx, const kwy_bap_rows_job *jobs, int count, int B, double *joint,
                            int64_t capacity_rows, int64_t *cursor) {
  KWY_TRY(bap_rows_check(ctx, jobs, count, B, joint, capacity_rows, cursor, true));
  if (count == 0) return KWY_OK;
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "bap_rows");
  double *djoint;
  int64_t *dcursor, *dplaces;
  st.inout(djoint, joint, (size_t)capacity_rows * 6 * B);
  st.inout(dcursor, cursor, 1);
  st.tmp(dplaces, BAP_GROUP * bap_launches(count));
  std::vector<kwy_bap_rows_job> staged(jobs, jobs + count);
  for (int i = 0; i < count; ++i) {
    const kwy_bap_rows_job &j = jobs[i];
    kwy_bap_rows_job &s = staged[i];
    st.out(s.n_rows, j.n_rows, 1);
    if (j.capacity == 0) continue;
    st.in(s.track_x, j.track_x, (size_t)j.x_rows * (B + 1));
    st.in(s.track_y, j.track_y, (size_t)j.y_rows * (B + 1));
    st.in(s.idx_x, j.idx_x, (size_t)j.capacity);
    st.in(s.idx_y, j.idx_y, (size_t)j.capacity);
  }
  KWY_TRY(st.begin());
  size_t used = 0;
  KWY_TRY(bap_rows_launch(ctx, staged.data(), count, B, djoint, capacity_rows, dcursor, [&]() {
    int64_t *p = dplaces + used;
    used += BAP_GROUP;
    return p;
  }));
  return st.finish();
}

static int bap_apply_check(kwy_ctx *ctx, const kwy_bap_apply_job *jobs, int count, int fs, int fft_size, int *B) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(bap_check_rate(ctx, "bap_apply", fs, fft_size, B));
  if (!jobs || count < 0) { ctx->err = "bap_apply: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i) {
    const kwy_bap_apply_job &j = jobs[i];
    if (!j.track_src || !j.track_conv || !j.ap || j.T <= 0 || j.T > 0x7fffffff / BAP_GROUP) {
      ctx->err = "bap_apply: bad argument";
      return KWY_EINVAL;
    }
  }
  return KWY_OK;
}

static int bap_apply_launch(kwy_ctx *ctx, const kwy_bap_apply_job *jobs, int count, int fs, int fft_size, int B) {
  return kwy_for_tables<bap_apply_table>(
      count,
      [&](int i, int &blocks) {
        blocks = (int)jobs[i].T;
        return bap_apply_view{jobs[i].track_src, jobs[i].track_conv, jobs[i].ap};
      },
      [&](const bap_apply_table &t, int) {
        KWY_PROF(ctx, "k_bap_apply", hipLaunchKernelGGL(k_bap_apply, dim3((unsigned)t.start[t.n]), dim3(BAP_NT), 0,
                                                         ctx->stream, t, fs, fft_size, B));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

extern "C" int kwy_bap_apply_batch_dev(kwy_ctx *ctx, const kwy_bap_apply_job *jobs, int count, int fs, int fft_size) {
  int B = 0;
  KWY_TRY(bap_apply_check(ctx, jobs, count, fs, fft_size, &B));
  if (count == 0) return KWY_OK;
  KWY_HIP(hipSetDevice(ctx->device));
  return bap_apply_launch(ctx, jobs, count, fs, fft_size, B);
}

extern "C" int kwy_bap_apply_dev(kwy_ctx *ctx, const double *track_src, const double *track_conv, int64_t T, int fs,
                                 int fft_size, double *ap) {
  const kwy_bap_apply_job job = {track_src, track_conv, T, ap};
  return kwy_bap_apply_batch_dev(ctx, &job, 1, fs, fft_size);
}

extern "C" int kwy_bap_apply(kwy_ctx *ctx, const kwy_bap_apply_job *jobs, int count, int fs, int fft_size) {
  int B = 0;
  KWY_TRY(bap_apply_check(ctx, jobs, count, fs, fft_size, &B));
  if (count == 0) return KWY_OK;
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "bap_apply");
  std::vector<kwy_bap_apply_job> staged(jobs, jobs + count);
  for (int i = 0; i < count; ++i) {
    st.in(staged[i].track_src, jobs[i].track_src, (size_t)jobs[i].T * (B + 1));
    st.in(staged[i].track_conv, jobs[i].track_conv, (size_t)jobs[i].T * (B + 1));
    st.inout(staged[i].ap, jobs[i].ap, (size_t)jobs[i].T * (fft_size / 2 + 1));
  }
  KWY_TRY(st.begin());
  KWY_TRY(bap_apply_launch(ctx, staged.data(), count, fs, fft_size, B));
  return st.finish();
}

static int bap_error_check(kwy_ctx *ctx, const kwy_bap_error_job *jobs, int count, int B, const double *moments,
                           bool host) {
  if (!ctx) return KWY_EINVAL;
  KWY_TRY(bap_check_bands(ctx, "bap_error", B));
  if (!jobs || count < 1 || !moments) { ctx->err = "bap_error: bad argument"; return KWY_EINVAL; }
  for (int i = 0; i < count; ++i) {
    const kwy_bap_error_job &j = jobs[i];
    if (j.rows < 0 || j.a_rows < 0 || j.b_rows < 0 || (j.a_rows > 0 && !j.a) || (j.b_rows > 0 && !j.b) || (host && j.n_dev)) {
      ctx->err = host && j.n_dev ? "bap_error: the host form takes its row count by value" : "bap_error: bad argument";
      return KWY_EINVAL;
    }
  }
  return KWY_OK;
}

static int bap_error_launch(kwy_ctx *ctx, const kwy_bap_error_job *jobs, int count, int B, double *moments) {
  return kwy_for_tables<bap_error_table>(
      count,
      [&](int i) {
        const kwy_bap_error_job &j = jobs[i];
        return bap_error_view{j.a, j.b, j.idx_a, j.idx_b, j.n_dev, j.per_row, moments + 3 * (int64_t)i,
                              j.a_rows, j.b_rows, j.off_a, j.off_b, j.rows};
      },
      [&](const bap_error_table &t, int) {
        KWY_PROF(ctx, "k_bap_error", hipLaunchKernelGGL(k_bap_error, dim3(t.n), dim3(BAP_NT), 0, ctx->stream, t, B));
        KWY_HIP(hipGetLastError());
        return KWY_OK;
      });
}

extern "C" int kwy_bap_error_batch_dev(kwy_ctx *ctx, const kwy_bap_error_job *jobs, int count, int B, double *moments) {
  KWY_TRY(bap_error_check(ctx, jobs, count, B, moments, false));
  KWY_HIP(hipSetDevice(ctx->device));
  return bap_error_launch(ctx, jobs, count, B, moments);
}

extern "C" int kwy_bap_error(kwy_ctx *ctx, const kwy_bap_error_job *jobs, int count, int B, double *moments) {
  KWY_TRY(bap_error_check(ctx, jobs, count, B, moments, true));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "bap_error");
  double *dm;
  st.out(dm, moments, 3 * (size_t)count);
  std::vector<kwy_bap_error_job> staged(jobs, jobs + count);
  for (int i = 0; i < count; ++i) {
    const kwy_bap_error_job &j = jobs[i];
    kwy_bap_error_job &s = staged[i];
    st.in(s.a, j.a, (size_t)j.a_rows * (B + 1));
    st.in(s.b, j.b, (size_t)j.b_rows * (B + 1));
    if (j.idx_a) st.in(s.idx_a, j.idx_a, (size_t)j.rows);
    if (j.idx_b) st.in(s.idx_b, j.idx_b, (size_t)j.rows);
    if (j.per_row) st.out(s.per_row, j.per_row, (size_t)j.rows);
  }
  KWY_TRY(st.begin());
  KWY_TRY(bap_error_launch(ctx, staged.data(), count, B, dm));
  return st.finish();
}
