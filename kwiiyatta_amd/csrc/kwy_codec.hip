// kwy_codec.hip -- WORLD aperiodicity band codec on gfx950.
//
// Replaces pyworld.code_aperiodicity / pyworld.decode_aperiodicity, which the reference uses
// only to move aperiodicity between sampling rates or spectrum lengths
// (kwiiyatta/vocoder/world.py:98-145).  WORLD codec.cpp as shipped with pyworld 0.2.8:
//   code   : 20 log10(ap) sampled at 3 kHz, 6 kHz, ... by interp1Q on the bin grid
//   decode : linear interpolation over {0: -60 dB, 3k(i+1): coded[i], fs/2: -1e-12 dB}, 10^(dB/20);
//            frames whose mean coded value exceeds -0.5 dB stay at 1 - 1e-12
// One workgroup per frame; pure streaming (K*8 B in, bands*8 B out and vice versa).
#include <math.h>

#include "kwy_internal.hpp"

extern "C" int kwy_aperiodicity_bands(int fs) { return kwy_band_count(fs); }

__global__ __launch_bounds__(64) void k_code_aperiodicity(const double *__restrict__ ap, int64_t T, int fs,
                                                         int fft_size, int nb, double *__restrict__ coded) {
  const int64_t frame = blockIdx.x;
  const int b = threadIdx.x;
  if (b >= nb) return;
  const int K = fft_size / 2 + 1;
  coded[frame * nb + b] = kwy_band_code(ap + frame * K, K, fs, fft_size, b);
}

__global__ __launch_bounds__(KWY_THREADS) void k_decode_aperiodicity(const double *__restrict__ coded, int64_t T,
                                                                     int fs, int fft_size, int nb,
                                                                     double *__restrict__ ap) {
  __shared__ double coarse[KWY_BAND_MAX + 2];
  __shared__ int s_unvoiced;
  const int64_t frame = blockIdx.x;
  const int tid = threadIdx.x, K = fft_size / 2 + 1;
  double *o = ap + frame * K;
  if (tid == 0) {
    double tmp = 0.0;
    for (int i = 0; i < nb; ++i) { tmp += coded[frame * nb + i]; coarse[i + 1] = coded[frame * nb + i]; }
    coarse[0] = KWY_BAND_FLOOR;
    coarse[nb + 1] = -KWY_SAFE;
    s_unvoiced = nb <= 0 || (tmp / nb > -0.5);
  }
  __syncthreads();
  if (s_unvoiced) {
    for (int k = tid; k < K; k += KWY_THREADS) o[k] = 1.0 - KWY_SAFE;
    return;
  }
  for (int k = tid; k < K; k += KWY_THREADS) o[k] = kwy_band_decode_bin(coarse, fs, fft_size, nb, k);
}

static int codec_check(kwy_ctx *ctx, const void *a, const void *b, int64_t T, int fs, int fft_size, int nb) {
  if (!ctx) return KWY_EINVAL;
  if (!a || !b || T <= 0 || fs <= 0 || fft_size < 4 || (fft_size & 1) || nb < 0 || nb > KWY_BAND_MAX) {
    ctx->err = "aperiodicity codec: bad argument";
    return KWY_EINVAL;
  }
  // more bands than the rate has: the nodes 3 kHz, 6 kHz, ... would reach fs/2, the last node, and the grid would
  // no longer increase (WORLD derives the count from fs; the reference's caller truncates to the new rate's count)
  if (nb > kwy_band_count(fs)) {
    ctx->err = "aperiodicity codec: more bands than the sampling rate has";
    return KWY_EINVAL;
  }
  return KWY_OK;
}

extern "C" int kwy_code_aperiodicity_dev(kwy_ctx *ctx, const double *ap, int64_t T, int fs, int fft_size,
                                         double *coded) {
  const int nb = kwy_band_count(fs);
  KWY_TRY(codec_check(ctx, ap, coded, T, fs, fft_size, nb));
  KWY_HIP(hipSetDevice(ctx->device));
  if (nb == 0) return KWY_OK;
  hipLaunchKernelGGL(k_code_aperiodicity, dim3((unsigned)T), dim3(64), 0, ctx->stream, ap, T, fs, fft_size, nb, coded);
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

extern "C" int kwy_decode_aperiodicity_dev(kwy_ctx *ctx, const double *coded, int64_t T, int fs, int fft_size,
                                           int nb, double *ap) {
  KWY_TRY(codec_check(ctx, coded, ap, T, fs, fft_size, nb));
  KWY_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_decode_aperiodicity, dim3((unsigned)T), dim3(KWY_THREADS), 0, ctx->stream, coded, T, fs,
                     fft_size, nb, ap);
  KWY_HIP(hipGetLastError());
  return KWY_OK;
}

extern "C" int kwy_code_aperiodicity(kwy_ctx *ctx, const double *ap, int64_t T, int fs, int fft_size,
                                     double *coded) {
  const int nb = kwy_band_count(fs);
  KWY_TRY(codec_check(ctx, ap, coded, T, fs, fft_size, nb));
  KWY_HIP(hipSetDevice(ctx->device));
  if (nb == 0) return KWY_OK;
  kwy_staging st(ctx, "code_aperiodicity");
  double *dap, *dc;
  st.in(dap, ap, (size_t)T * (fft_size / 2 + 1));
  st.out(dc, coded, (size_t)T * nb);
  KWY_TRY(st.begin());
  KWY_TRY(kwy_code_aperiodicity_dev(ctx, dap, T, fs, fft_size, dc));
  return st.finish();
}

extern "C" int kwy_decode_aperiodicity(kwy_ctx *ctx, const double *coded, int64_t T, int fs, int fft_size, int nb,
                                       double *ap) {
  KWY_TRY(codec_check(ctx, coded, ap, T, fs, fft_size, nb));
  KWY_HIP(hipSetDevice(ctx->device));
  kwy_staging st(ctx, "decode_aperiodicity");
  double *dap, *dc;
  st.out(dap, ap, (size_t)T * (fft_size / 2 + 1));
  st.in(dc, coded, (size_t)T * nb);
  KWY_TRY(st.begin());
  KWY_TRY(kwy_decode_aperiodicity_dev(ctx, dc, T, fs, fft_size, nb, dap));
  return st.finish();
}
