// nmf_args_main.cpp -- the host arithmetic of kwy_nmf_convert (kwy_nmf_args.hpp: limits, pointer rules, scratch layout)
// walked by a plain host program, so that it can be built with -fsanitize=address,undefined and run without a device:
//   c++ -std=c++17 -fsanitize=address,undefined -o nmf_args selftest/nmf_args_main.cpp && ./nmf_args
// Not part of libkwy.so.
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "../kwy_nmf_args.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // the limits, each edge inside and outside
  EXPECT(!nmf_sizes_error(1, 2, 0, 0, 0.0));
  EXPECT(!nmf_sizes_error(8192, 2049, 0x7fffffffLL, 1000, 1e300));
  EXPECT(nmf_sizes_error(0, 2, 1, 1, 0.0) && nmf_sizes_error(8193, 2, 1, 1, 0.0));
  EXPECT(nmf_sizes_error(1, 1, 1, 1, 0.0) && nmf_sizes_error(1, 2050, 1, 1, 0.0));
  EXPECT(nmf_sizes_error(1, 2, -1, 1, 0.0) && nmf_sizes_error(1, 2, 0x80000000LL, 1, 0.0));
  EXPECT(nmf_sizes_error(1, 2, 1, -1, 0.0) && nmf_sizes_error(1, 2, 1, 1001, 0.0));
  EXPECT(nmf_sizes_error(1, 2, 1, 1, -1e-300) && nmf_sizes_error(1, 2, 1, 1, inf) && nmf_sizes_error(1, 2, 1, 1, nan));
  EXPECT(nmf_sizes_error(std::numeric_limits<int>::min(), std::numeric_limits<int>::max(),
                         std::numeric_limits<int64_t>::min(), std::numeric_limits<int>::min(), -inf));
  // the pointer rules
  double x = 0;
  EXPECT(!nmf_pointers_error(&x, &x, &x, &x, NULL, NULL) && !nmf_pointers_error(&x, NULL, &x, NULL, &x, NULL));
  EXPECT(nmf_pointers_error(NULL, &x, &x, &x, NULL, NULL) && nmf_pointers_error(&x, &x, NULL, &x, NULL, NULL));
  EXPECT(nmf_pointers_error(&x, &x, &x, NULL, &x, NULL) && nmf_pointers_error(&x, NULL, &x, &x, NULL, NULL));
  EXPECT(nmf_pointers_error(&x, NULL, &x, NULL, NULL, NULL));
  // the layout: parts in order, aligned, disjoint, inside the total less the alignment slack, every padded matrix whole
  const int As[] = {1, 15, 16, 17, 63, 64, 65, 2048, 8192}, Bs[] = {2, 63, 64, 65, 257, 2049};
  const int64_t Ts[] = {1, 31, 127, 128, 129, 2000, 512000, 0x7fffffffLL};
  for (int A : As) for (int B : Bs) for (int64_t T : Ts) {
    const nmf_layout L = nmf_make_layout(A, B, T);
    EXPECT(L.Ap >= A && L.Ap % NMF_COLS == 0 && L.Ap - A < NMF_COLS && L.A16 >= A && L.A16 % 16 == 0 && L.A16 <= L.Ap);
    EXPECT(L.Bp >= B && L.Bp % NMF_COLS == 0 && L.Bp - B < NMF_COLS && L.B16 >= B && L.B16 % 16 == 0 && L.B16 <= L.Bp);
    EXPECT(L.Tp >= T && L.Tp % NMF_ROWS == 0 && L.Tp - T < NMF_ROWS);
    const size_t atoms = sizeof(double) * (size_t)L.Ap * L.Bp, frames = sizeof(double) * (size_t)L.Tp * L.Bp;
    const size_t acts = sizeof(double) * (size_t)L.Tp * L.Ap;
    const size_t offs[] = {L.off_S, L.off_Tg, L.off_X, L.off_Q, L.off_H, L.off_bad, L.total - 256};
    const size_t sizes[] = {atoms, atoms, frames, frames, acts, sizeof(int) * 5 * NMF_PAD_BLOCKS};
    for (int i = 0; i < 6; ++i) EXPECT(offs[i] % 256 == 0 && offs[i] + sizes[i] <= offs[i + 1]);
    EXPECT(nmf_scratch_bytes(A, B, T) == L.total);
    // a tile never reads or writes outside a padded matrix: the last workgroup's rows and columns
    EXPECT((L.Tp / NMF_ROWS) * NMF_ROWS == L.Tp);
    EXPECT(((L.B16 / 16 + 3) / 4) * NMF_COLS <= L.Bp && ((L.A16 / 16 + 3) / 4) * NMF_COLS <= L.Ap);
  }
  EXPECT(nmf_scratch_bytes(1, 2, 0) == 0 && nmf_scratch_bytes(0, 2, 1) == 0 && nmf_scratch_bytes(1, 2, -5) == 0);
  // a small layout laid over real memory: every part written end to end under the sanitizer
  {
    const nmf_layout L = nmf_make_layout(17, 65, 33);
    std::vector<char> buf(L.total);
    char *base = (char *)(((uintptr_t)buf.data() + 255) & ~(uintptr_t)255);
    double *S = (double *)(base + L.off_S), *H = (double *)(base + L.off_H);
    int *bad = (int *)(base + L.off_bad);
    for (size_t i = 0; i < (size_t)L.Ap * L.Bp; ++i) S[i] = 1.0;
    for (size_t i = 0; i < (size_t)L.Tp * L.Ap; ++i) H[i] = 1.0;
    for (int i = 0; i < 5 * NMF_PAD_BLOCKS; ++i) bad[i] = 0;
    EXPECT((char *)(bad + 5 * NMF_PAD_BLOCKS) <= buf.data() + buf.size());
  }
  printf(failures ? "%d check(s) failed\n" : "nmf_args: all checks passed\n", failures);
  return failures ? 1 : 0;
}
