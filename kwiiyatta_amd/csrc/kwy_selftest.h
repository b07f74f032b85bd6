/* kwy_selftest.h -- NOT part of the public ABI (include/kwy.h) and not in libkwy.so: entry points of the test-only
 * libkwy_selftest.so (selftest/kwy_selftest.hip), which let tests drive device-side building blocks on caller data. */
#ifndef KWY_SELFTEST_H_
#define KWY_SELFTEST_H_
#ifdef __cplusplus
extern "C" {
#endif
/* The block-wide "sum of the m smallest of n" used by D4C's band aperiodicity.
 * values: problems x n non-negative doubles (device); out: problems x {sum of the m smallest, sum of all} (device).
 * n <= 2304.  stream: a hipStream_t (NULL = the default stream).  Returns 0, -1 (arguments) or -2 (launch failed). */
int kwy_debug_smallest_sum_dev(void *stream, const double *values, int problems, int n, int m, double *out);
/* The same routine beside the reference copy of its earlier form (one histogram counted with same-address atomics,
 * kwy_block_sum2 behind the selection) that the self-test library keeps, both on the same keys; the current one in
 * the form the band kernel calls (sums in thread 0 only).  out_ref / out_new: problems x {sum of the m smallest, sum of all} (device); the two
 * are meant to agree bit for bit.  256 threads per problem, n <= 2304; the 512-thread form of the 96 kHz band kernel,
 * n <= 4608. */
int kwy_debug_select_paths_dev(void *stream, const double *values, int problems, int n, int m, double *out_ref,
                               double *out_new);
int kwy_debug_select_paths512_dev(void *stream, const double *values, int problems, int n, int m, double *out_ref,
                                  double *out_new);
/* kwy_log(x) and kwy_sincos_medium(x) of kwy_device.hpp for every element of x (n doubles, device). */
int kwy_debug_devmath_dev(void *stream, const double *x, int n, double *log_out, double *sin_out, double *cos_out);
/* kwy_block_exscan of kwy_device.hpp, one workgroup of 256 threads per problem.  values, offsets: problems x 256 ints
 * (device), offsets[i] = the sum of the problem's values before i; totals: problems ints (device), as the last thread
 * of the workgroup received them. */
int kwy_debug_block_exscan_dev(void *stream, const int *values, int problems, int *offsets, int *totals);
/* The real FFT of rows of 2^log2n samples through both closing passes of the LDS transform: the stored one and the
 * one drained into registers (kwy_fft_tail4_drain).  x: problems x 2^log2n doubles (device); out_old / out_new:
 * problems x (2^(log2n-1) + 1) x {re, im} (device), twice the bins 0 .. N/2.  log2n = 12 is the only size with a
 * drained pass; others return -1.  Synchronises the stream.  Returns 0, -1 (arguments) or -2 (HIP failure). */
int kwy_debug_rfft_paths_dev(void *stream, const double *x, int problems, int log2n, double *out_old, double *out_new);
/* The complex LDS transform of 2^log2h points (10, 11, 12) with nt threads (128 or 256; 256; 512), forward or inverse,
 * twice: the stride-64 radix-8 pass forms the powers of its factor per lane (out_lane), or takes them from the powers
 * table by scalar loads (out_table) as every kernel of the library does.  x, out_lane, out_table: problems x 2^log2h x
 * {re, im} (device).  tab receives the table as the library's fill kernel makes it, tab_ref and tab_ref_conj the
 * entries recomputed by one thread from w and from conj(w): 8 x 2^log2h / 512 x {re, im} each (device).
 * Synchronises the stream.  Returns 0, -1 (arguments) or -2 (HIP failure). */
int kwy_debug_fft_powers_dev(void *stream, const double *x, int problems, int log2h, int nt, int inverse,
                             double *out_lane, double *out_table, double *tab, double *tab_ref, double *tab_ref_conj);
/* The first passes and the real split of the 2048-point synthesis kernel (1024 complex points, 128 threads), every form
 * on the same rows.  x: problems x 1024 x {re, im} (device).  out_dense, out_sparse, out_half: problems x 1024 x {re, im}
 * (device): the complex transform through kwy_fft_pass8 (dense), kwy_fft_pass8_first_sparse_core (which takes x[0 .. 128]
 * from registers and assumes zeros behind) and kwy_fft_pass8_first_half_core (which reads x[0 .. 512] and assumes zeros
 * behind), the same remaining passes behind each.  fold_ref, fold_new: problems x 1025 doubles (device): the folded
 * cepstrum behind the dense transform by kwy_syn_rsplit + kwy_syn_fold and by kwy_syn_rsplit_fold.  Synchronises the
 * stream.  Returns 0, -1 (arguments) or -2 (HIP failure). */
int kwy_debug_syn_first_passes_dev(void *stream, const double *x, int problems, double *out_dense, double *out_sparse,
                                   double *out_half, double *fold_ref, double *fold_new);
/* The complex LDS transform on thread-held pass factors in the shapes of k_d4c_body (2^log2h = 1024 or 2048 points with
 * 256 threads, 4096 with 512), forward or inverse, twice on every row: kwy_fft_inplace_w on the whole row (out_dense),
 * and kwy_fft_inplace_sel_w with half = true on a buffer that holds points 0 .. H/2 of the row and, above them, the same points of
 * `stale` (out_half) -- the half transform takes the points above H/2 as zero and must not read them.  tail = 0 stops
 * both in front of the closing radix-4 / radix-2 pass (what the callers of kwy_fft_tail4_drain do).  x, stale,
 * out_dense, out_half: problems x 2^log2h x {re, im} (device).  Synchronises the stream.  Returns 0, -1 (arguments) or
 * -2 (HIP failure). */
int kwy_debug_fft_half_w_dev(void *stream, const double *x, const double *stale, int problems, int log2h, int inverse,
                             int tail, double *out_dense, double *out_half);
/* The 2048-point transform of the 4096-point D4C frames (256 threads) up to and including the drained closing pass,
 * twice on every row: the Stockham chain (kwy_fft_inplace_w / kwy_fft_inplace_sel_w / kwy_fft_pass8_first_sparse_core +
 * kwy_fft_inplace_rest_w, then kwy_fft_tail4_drain: out_old) and the wave-local form (kwy_fftwl_*: out_new).  Before
 * either runs, the whole buffer (2049 points) is filled with the row of `stale`.  kind: 0 dense (all 2048 points of the
 * row), 1 half (points 0 .. 1024 of the row, the half first pass), 2 half with point 1024 stored as zero, 3 sparse
 * (points 0 .. 256 of the row, from registers).  x: problems x 2048 x {re, im}; stale: problems x 2049 x {re, im};
 * out_old, out_new: problems x 256 threads x 9 x {re, im}: lo[0..3], hi[0..3], mid of kwy_fft_tail4_drain (all device).
 * Synchronises the stream.  Returns 0, -1 (arguments) or -2 (HIP failure). */
int kwy_debug_fft_wave_local_dev(void *stream, const double *x, const double *stale, int problems, int kind,
                                 double *out_old, double *out_new);
#ifdef __cplusplus
}
#endif
#endif
