// How many 128-thread workgroups of a kernel with __launch_bounds__(128, 3) does the runtime place on a CU, as a function of
// the dynamic LDS request?  Asks hipOccupancyMaxActiveBlocksPerMultiprocessor over a range of sizes and prints every size
// at which the answer changes (k_syn_pulse<11, *>: where 6 workgroups turn into 5).  Launches nothing.
//   hipcc --offload-arch=gfx950 -O3 -o lds_blocks tools/ubench/lds_blocks.hip && ./lds_blocks [from to step]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
// registers like the pulse kernel's: the bound of three wavefronts per SIMD comes from __launch_bounds__, not from use
__global__ __launch_bounds__(128, 3) void k_dummy(double *out) {
  extern __shared__ double smem[];
  smem[threadIdx.x] = (double)threadIdx.x;
  __syncthreads();
  out[threadIdx.x] = smem[127 - threadIdx.x];
}
int main(int argc, char **argv) {
  const int from = argc > 3 ? atoi(argv[1]) : 20000, to = argc > 3 ? atoi(argv[2]) : 34000, step = argc > 3 ? atoi(argv[3]) : 16;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no device\n"); return 1; }
  printf("%s: %d CUs, %zu B of LDS per workgroup at most, %zu B per CU\n", prop.gcnArchName, prop.multiProcessorCount,
         prop.sharedMemPerBlock, (size_t)prop.maxSharedMemoryPerMultiProcessor);
  if (hipFuncSetAttribute((const void *)k_dummy, hipFuncAttributeMaxDynamicSharedMemorySize, to) != hipSuccess) return 1;
  int last = -1;
  for (int lds = from; lds <= to; lds += step) {
    int blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, (const void *)k_dummy, 128, (size_t)lds) != hipSuccess) return 1;
    if (blocks != last) printf("dynamic LDS %6d B: %d workgroups per CU%s\n", lds, blocks, last < 0 ? "" : "   <- changes here");
    last = blocks;
  }
  printf("dynamic LDS %6d B: %d workgroups per CU (end of the range)\n", to, last);
  return 0;
}
