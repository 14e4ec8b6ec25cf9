// hist_build probe #5 (gfx950): does ds_add_u64 speed up when the LDS bank
// of a cell depends on the FEATURE only and the 16 lanes of every lane group
// work on 16 different features?
//   hipcc --offload-arch=gfx950 -O3 tools/probe_hist5.hip -o probe_hist5
// Shape of the flagship block: 1024 threads, 64 features x 256 bins of u64
// cells (128 KiB, one block per CU), one row per lane per iteration, the row's
// 64 bin bytes read from memory as four uint4 pieces.  Modes:
//   0 loads only        : the same loads, no LDS traffic (floor)
//   1 (a) feature-major : lds[f*B + b], every lane on the same feature — the
//                         bank pair is b mod 16, i.e. random (today's kernel)
//   2 (b) bin-major+rot : lds[b*FG + f], lane l takes feature (k + l%16)%16 of
//                         a piece at step k — 16 different bank pairs per group
//   3 (c) bin-major     : lds[b*FG + f], every lane on the same feature —
//                         one bank pair per group, the 16-way worst case
// Rates are (row, feature) adds per clock per CU, from the blocks' own cycle
// counters (mean over blocks) and from the event time at the nominal clock.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

#define HIP_CHECK(x) do { hipError_t e = (x); if (e) { printf("HIPERR %s @%d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

constexpr int FG = 64;
constexpr int B = 256;
constexpr int THREADS = 1024;
constexpr int BLOCKS = 256;
constexpr int ROWS_PER_BLOCK = 16384;  // 16 rows per lane
constexpr int64_t N = (int64_t)BLOCKS * ROWS_PER_BLOCK;  // 4M rows, 256 MiB
constexpr int CELLS_TOTAL = FG * B;

// rotate the 16 bytes of a piece right by lam bytes: byte p of the result
// is byte (p + lam) % 16 of the input.  Dword rotate by lam >> 2 (two levels
// of selects), then a funnel shift by lam & 3 bytes.
__device__ inline void rotate16(unsigned (&w)[4], int lam) {
  const bool r1 = lam & 4, r2 = lam & 8;
  const unsigned a0 = r1 ? w[1] : w[0], a1 = r1 ? w[2] : w[1],
                 a2 = r1 ? w[3] : w[2], a3 = r1 ? w[0] : w[3];
  const unsigned b0 = r2 ? a2 : a0, b1 = r2 ? a3 : a1, b2 = r2 ? a0 : a2,
                 b3 = r2 ? a1 : a3;
  const unsigned t = lam & 3;
  w[0] = __builtin_amdgcn_alignbyte(b1, b0, t);
  w[1] = __builtin_amdgcn_alignbyte(b2, b1, t);
  w[2] = __builtin_amdgcn_alignbyte(b3, b2, t);
  w[3] = __builtin_amdgcn_alignbyte(b0, b3, t);
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void probe_kernel(
    unsigned long long* __restrict__ out,   // [8][CELLS_TOTAL]
    long long* __restrict__ cycles,         // [BLOCKS]
    const uint8_t* __restrict__ bins) {     // [N, FG]
  extern __shared__ unsigned long long lds64[];
  for (int i = threadIdx.x; i < CELLS_TOTAL; i += THREADS) lds64[i] = 0ull;
  __syncthreads();
  const long long t0 = clock64();

  const int lam = threadIdx.x & 15;
  // byte offset of the feature that byte p of a rotated piece belongs to
  unsigned foff[16];
#pragma unroll
  for (int p = 0; p < 16; ++p) foff[p] = ((p + lam) & 15) * 8;

  const int64_t start = (int64_t)blockIdx.x * ROWS_PER_BLOCK;
  unsigned sink = 0;
  char* base = reinterpret_cast<char*>(lds64);
  for (int i = threadIdx.x; i < ROWS_PER_BLOCK; i += THREADS) {
    const int64_t r = start + i;
    const unsigned long long addend = (1ull << 32) | 1ull;
#pragma unroll
    for (int hh = 0; hh < FG / 16; ++hh) {
      const uint4 bv =
          *reinterpret_cast<const uint4*>(bins + r * FG + 16 * hh);
      unsigned w[4] = {bv.x, bv.y, bv.z, bv.w};
      if (MODE == 0) {
        sink += w[0] ^ w[1] ^ w[2] ^ w[3];
        continue;
      }
      if (MODE == 2) rotate16(w, lam);
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        const unsigned b = (w[p >> 2] >> (8 * (p & 3))) & 0xff;
        unsigned long long* cell;
        if (MODE == 1)
          cell = lds64 + (16 * hh + p) * B + b;
        else if (MODE == 2)
          cell = reinterpret_cast<unsigned long long*>(
              base + b * (FG * 8) + foff[p] + hh * 128);
        else
          cell = lds64 + b * FG + 16 * hh + p;
        atomicAdd(cell, addend);
      }
    }
  }
  __syncthreads();
  const long long t1 = clock64();
  if (threadIdx.x == 0) cycles[blockIdx.x] = t1 - t0;
  // the first 8 blocks keep their histogram (the sink test keeps mode 0's
  // loads alive)
  if (blockIdx.x < 8 || sink == 0x9E3779B9u) {
    unsigned long long* dst = out + (int64_t)(blockIdx.x % 8) * CELLS_TOTAL;
    for (int i = threadIdx.x; i < CELLS_TOTAL; i += THREADS)
      dst[i] = lds64[i] + sink;
  }
}

__global__ void fill_kernel(uint8_t* bins) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < N * FG; i += stride) {
    uint64_t z = (uint64_t)i + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    bins[i] = (uint8_t)((z ^ (z >> 31)) >> 24);
  }
}

template <int MODE>
int run(const char* name, const uint8_t* bins, unsigned long long* out,
        long long* cycles, double clock_ghz,
        std::vector<unsigned long long>* keep) {
  const size_t lds = (size_t)CELLS_TOTAL * 8;
  HIP_CHECK(hipFuncSetAttribute(
      reinterpret_cast<const void*>(&probe_kernel<MODE>),
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipEvent_t a, b;
  HIP_CHECK(hipEventCreate(&a));
  HIP_CHECK(hipEventCreate(&b));
  hipLaunchKernelGGL(probe_kernel<MODE>, dim3(BLOCKS), dim3(THREADS), lds, 0,
                     out, cycles, bins);
  HIP_CHECK(hipDeviceSynchronize());
  const int iters = 5;
  HIP_CHECK(hipEventRecord(a));
  for (int it = 0; it < iters; ++it)
    hipLaunchKernelGGL(probe_kernel<MODE>, dim3(BLOCKS), dim3(THREADS), lds, 0,
                       out, cycles, bins);
  HIP_CHECK(hipEventRecord(b));
  HIP_CHECK(hipDeviceSynchronize());
  float ms;
  HIP_CHECK(hipEventElapsedTime(&ms, a, b));
  ms /= iters;
  std::vector<long long> cyc(BLOCKS);
  HIP_CHECK(hipMemcpy(cyc.data(), cycles, BLOCKS * 8, hipMemcpyDeviceToHost));
  double mean = 0;
  for (long long c : cyc) mean += (double)c / BLOCKS;
  const double adds_block = (double)ROWS_PER_BLOCK * FG;
  const double adds = adds_block * BLOCKS;
  printf("%-24s %7.3f ms  %7.1f G add/s  %5.2f add/clk/CU (block counter, "
         "%.0f cyc)  %5.2f add/clk/CU (event, %.2f GHz)\n",
         name, ms, adds / ms / 1e6, adds_block / mean, mean,
         adds / (ms * 1e-3) / (clock_ghz * 1e9) / BLOCKS, clock_ghz);
  if (keep) {
    keep->resize(CELLS_TOTAL);
    HIP_CHECK(hipMemcpy(keep->data(), out, lds, hipMemcpyDeviceToHost));
  }
  return 0;
}

int main() {
  uint8_t* bins;
  unsigned long long* out;
  long long* cycles;
  HIP_CHECK(hipMalloc(&bins, N * FG));
  HIP_CHECK(hipMalloc(&out, (size_t)8 * CELLS_TOTAL * 8));
  HIP_CHECK(hipMalloc(&cycles, BLOCKS * 8));
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, bins);
  HIP_CHECK(hipDeviceSynchronize());
  int khz = 0;
  HIP_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, 0));
  const double ghz = khz / 1e6;

  std::vector<unsigned long long> ha, hb, hc;
  if (run<0>("loads only", bins, out, cycles, ghz, nullptr)) return 1;
  if (run<1>("(a) feature-major", bins, out, cycles, ghz, &ha)) return 1;
  if (run<2>("(b) bin-major rotated", bins, out, cycles, ghz, &hb)) return 1;
  if (run<3>("(c) bin-major unrotated", bins, out, cycles, ghz, &hc)) return 1;

  // block 0's histogram must be the same under the three layouts
  long long bad = 0;
  unsigned long long total = 0;
  for (int f = 0; f < FG; ++f)
    for (int b = 0; b < B; ++b) {
      const unsigned long long v = ha[f * B + b];
      total += v & 0xffffffffull;
      if (hb[b * FG + f] != v || hc[b * FG + f] != v) ++bad;
    }
  if (total != (unsigned long long)ROWS_PER_BLOCK * FG) ++bad;
  printf("block 0 histograms %s (%llu adds counted)\n",
         bad ? "MISMATCH" : "equal under (a), (b), (c)", total);
  printf("done\n");
  return bad ? 1 : 0;
}
