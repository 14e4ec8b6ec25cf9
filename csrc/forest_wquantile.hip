// forest_wquantile: per-row weighted order statistics over the member values
// of a packed forest, in one launch, for gfx950.
//
//   v_t(i)    = leaf_t(x_i), t = 0 .. M-1          (one value per member)
//   out[i, q] = the first v, in ascending order of (v, t), whose cumulative
//               member weight reaches thresholds[q]; the smallest v when
//               none does
//
// With thresholds[q] = ceil(p_q * total weight) this is the weighted-median
// rule of AdaBoost.R2 (p = 0.5) and the weighted p-quantile of a bagged
// forest.  It is not a sum, so it cannot ride in forest_predict's weighted
// leaf sum; the torch route it replaces stacks M per-member predictions into
// [N, M], argsorts, gathers twice and runs an f32 cumsum: several [N, M]
// temporaries, one of them i64.
//
// Ranks, not values.  The host sorts the distinct leaf values of the whole
// forest into leaf_table[U] and writes each leaf's RANK into its node
// payload (dispatch._wquantile_ranks).  Order of ranks is order of values,
// equal values share a rank, and a member's value for a row packs with the
// member index into ONE u32 key, rank << 8 | t: M <= 256, U <= 2^24.
// Sorting keys sorts by (value, member), which is the stable order of the
// reference, and the selected value is one leaf_table[key >> 8] load.
//
// LDS split.  [ qweights 256 x i64 | thresholds 16 x i64 | key slab
// [M_pad][R] u32 | the group's nodes ].  The slab is key-major, one column
// per lane: lane l touches bank l % 64 whatever index it reads, and a lane is
// the only reader and writer of its column, so phases 2 and 3 need no
// barrier and no cross-lane traffic.  M_pad is M rounded up to a power of
// two; R = 256 / 128 / 64 rows per block for M_pad <= 64 / 128 / 256 keeps
// the slab within 64 KiB.  The rest of the CU's 160 KiB holds the group's
// nodes (kWqGroupNodes), so the forest is regrouped under that budget from
// the same arena layout the other forest ops read.  The launch reserves what
// the call needs (tables + M_pad * R * 4 + the largest group), so a small
// forest runs several blocks per CU.
//
// Phase 1, walk.  A block owns a tile of R rows, one row per lane, and walks
// the groups in order as forest_oob does: stage group g, barrier, every lane
// walks the group's trees for its row and stores the key of tree t at
// slab[t][lane].  Rows are f32 against f32 thresholds or u8 ranks against
// threshold ranks (forest_predict2's two exact forms).
//
// Phase 2, order.  Each lane sorts its column with a bitonic network over
// M_pad keys in LDS: a compare-exchange is 2 ds_read, min / max, 2 ds_write.
// The indices of the network are wave-uniform (scalar registers), the pairs
// of one pass are independent, and four are in flight per iteration.  A
// column of up to 32 keys is loaded into registers, sorted by the same
// network fully unrolled and stored back (measured: the sort of 32 keys
// falls from 0.18 to 0.04 ms at 2M rows; profiles/wquantile.md).  Pad keys
// are 0xFFFFFFFF: they sort last and phase 3 reads the first M only.
//
// Phase 3, select.  Per q a lane scans its sorted column, acc += qweights[key
// & 255] in i64, and stops at the first acc >= thresholds[q].  "First
// index" as written, so zero and negative member weights (AdaBoost.R2 keeps
// the stage whose error reached one half: its weight is <= 0) behave as in
// the reference.  The weights are exact integers (the host scales them by a
// power of two), so the rule is evaluated in exact arithmetic: no float sum,
// no atomics, bitwise reproducible.

#include <ATen/hip/HIPContext.h>

#include <tuple>

#include "common.h"

namespace {

constexpr int kWqMaxM = 256;  // member index is the low byte of a key
constexpr int kWqMaxQ = 16;
constexpr int kWqSlabBytes = 65536;
constexpr int kWqTabBytes = (kWqMaxM + kWqMaxQ) * 8;
constexpr int kWqLdsBytes = 163840;
constexpr int kWqGroupNodes =
    (kWqLdsBytes - kWqSlabBytes - kWqTabBytes) / 8;
constexpr int kWqMaxBlocks = 2048;  // row-tile blocks; tiles beyond wrap
constexpr unsigned kWqPadKey = 0xFFFFFFFFu;

// rows per block for a padded member count
constexpr int kWqR0 = 256, kWqM0 = 64;
constexpr int kWqR1 = 128, kWqM1 = 128;
constexpr int kWqR2 = 64, kWqM2 = kWqMaxM;

static_assert(kWqR0 * kWqM0 * 4 <= kWqSlabBytes &&
                  kWqR1 * kWqM1 * 4 <= kWqSlabBytes &&
                  kWqR2 * kWqM2 * 4 <= kWqSlabBytes,
              "the key slab fits its share of LDS");
static_assert(kWqTabBytes % 16 == 0 && kWqGroupNodes >= 1024,
              "tables and slab leave room for a group of nodes");

template <int R>
__device__ inline void wq_cmpx(unsigned* __restrict__ my, int i, int j,
                               bool up, unsigned a, unsigned b) {
  const unsigned lo = min(a, b);
  const unsigned hi = max(a, b);
  my[i * R] = up ? lo : hi;
  my[(i + j) * R] = up ? hi : lo;
}

// Switches of the measurement builds (profiles/wquantile.md); the shipped
// build defines neither.  WQ_PHASES = 1 stops after the walk, 2 after the
// sort (the row's first key is stored so that nothing before it is dead).
// WQ_REG_SORT = 0 sends every M_pad through the in-LDS network; 1 sorts
// columns of up to 32 keys in registers, measured 5x faster for the sort of
// 32 keys and level at 16.
#ifndef WQ_PHASES
#define WQ_PHASES 3
#endif
#ifndef WQ_REG_SORT
#define WQ_REG_SORT 1
#endif

#if WQ_REG_SORT
// the same network, fully unrolled over a column held in registers
template <int MP, int R>
__device__ inline void wq_sort_regs(unsigned* __restrict__ my) {
  unsigned v[MP];
#pragma unroll
  for (int i = 0; i < MP; ++i) v[i] = my[i * R];
#pragma unroll
  for (int k = 2; k <= MP; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int c = 0; c < MP / 2; ++c) {
        const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1));
        const unsigned lo = min(v[i], v[i + j]);
        const unsigned hi = max(v[i], v[i + j]);
        v[i] = (i & k) == 0 ? lo : hi;
        v[i + j] = (i & k) == 0 ? hi : lo;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < MP; ++i) my[i * R] = v[i];
}
#endif

template <int R, bool BINNED>
__global__ __launch_bounds__(R) void forest_wquantile_kernel(
    float* __restrict__ out,                       // [N, Q]
    const void* __restrict__ xv_,                  // [N, F] f32 | u8
    const unsigned long long* __restrict__ nodes,  // [total] packed, leaf
                                                   // payload = value rank
    const int* __restrict__ tree_off,              // [M] global node base
    const int* __restrict__ groups,                // [G, 4]
    const long long* __restrict__ qtab,            // [M + Q] weights, thresholds
    const float* __restrict__ leaf_table,          // [U] sorted leaf values
    int64_t n, int F, int G, int M, int Mp, int Q, int U, int64_t n_tiles) {
  extern __shared__ __align__(16) unsigned char smem[];
  long long* __restrict__ qw = reinterpret_cast<long long*>(smem);
  long long* __restrict__ thr = qw + kWqMaxM;
  unsigned* __restrict__ slab =
      reinterpret_cast<unsigned*>(smem + kWqTabBytes);  // [Mp][R]
  unsigned long long* __restrict__ tlds =
      reinterpret_cast<unsigned long long*>(smem + kWqTabBytes +
                                            (size_t)Mp * R * 4);
  unsigned* __restrict__ my = slab + threadIdx.x;  // this lane's column

  // every slot is written, so key & 255 never reads past the table; the
  // first group's barrier below orders these stores before phase 3
  for (int i = threadIdx.x; i < kWqMaxM; i += R) qw[i] = i < M ? qtab[i] : 0;
  if (threadIdx.x < kWqMaxQ)
    thr[threadIdx.x] = (int)threadIdx.x < Q ? qtab[M + threadIdx.x] : 0;

  // block-uniform trip count: every thread reaches every barrier
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row = tile * R + threadIdx.x;
    const bool live = row < n;
    const float* xr = BINNED ? nullptr : (const float*)xv_ + row * F;
    const uint8_t* br = BINNED ? (const uint8_t*)xv_ + row * F : nullptr;
    for (int i = M; i < Mp; ++i) my[i * R] = kWqPadKey;

    // ---- phase 1: one key per (member, row)
    for (int g = 0; g < G; ++g) {
      const int* grp = groups + g * 4;
      const int first_tree = grp[0];
      const int n_trees = grp[1];
      const int node_base = grp[2];
      const int n_nodes = grp[3];
      __syncthreads();  // the previous group's walks are done
      for (int i = threadIdx.x; i < n_nodes; i += R)
        tlds[i] = nodes[node_base + i];
      __syncthreads();

      for (int t = 0; t < n_trees; ++t) {
        const int gt = first_tree + t;  // member index
        const int toff = tree_off[gt] - node_base;
        if (live) {
          unsigned long long nd = tlds[toff];
          int f = (short)(nd & 0xFFFFu);
          while (f >= 0) {
            const int left = (short)((nd >> 16) & 0xFFFFu);
            bool go_left;
            if (BINNED)
              go_left = br[f] <= (unsigned)(nd >> 32);
            else
              go_left = xr[f] <= __uint_as_float((unsigned)(nd >> 32));
            nd = tlds[toff + left + (go_left ? 0 : 1)];
            f = (short)(nd & 0xFFFFu);
          }
          my[gt * R] = ((unsigned)(nd >> 32) << 8) | (unsigned)gt;
        }
      }
    }
    if (!live) continue;  // no barrier below this line in the tile

#if WQ_PHASES >= 2
    // ---- phase 2: bitonic network down this lane's column
    const int half = Mp >> 1;
#if WQ_REG_SORT
    bool sorted = true;
    switch (Mp) {
      case 1: break;
      case 2: wq_sort_regs<2, R>(my); break;
      case 4: wq_sort_regs<4, R>(my); break;
      case 8: wq_sort_regs<8, R>(my); break;
      case 16: wq_sort_regs<16, R>(my); break;
      case 32: wq_sort_regs<32, R>(my); break;
      default: sorted = false;
    }
    for (int k = sorted ? Mp + 1 : 2; k <= Mp; k <<= 1) {
#else
    for (int k = 2; k <= Mp; k <<= 1) {
#endif
      for (int j = k >> 1; j > 0; j >>= 1) {
        // pair c of the pass: i has bit j clear, its partner is i + j
        if (half >= 4) {
          for (int c = 0; c < half; c += 4) {
            int ii[4];
            unsigned a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int cc = c + u;
              ii[u] = ((cc & ~(j - 1)) << 1) | (cc & (j - 1));
              a[u] = my[ii[u] * R];
              b[u] = my[(ii[u] + j) * R];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
              wq_cmpx<R>(my, ii[u], j, (ii[u] & k) == 0, a[u], b[u]);
          }
        } else {
          for (int c = 0; c < half; ++c) {
            const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1));
            wq_cmpx<R>(my, i, j, (i & k) == 0, my[i * R], my[(i + j) * R]);
          }
        }
      }
    }

#endif  // WQ_PHASES >= 2

#if WQ_PHASES < 3
    for (int q = 0; q < Q; ++q)
      out[row * Q + q] = leaf_table[min((int)(my[0] >> 8), U - 1)];
#else
    // ---- phase 3: first key whose cumulative weight reaches the threshold
    for (int q = 0; q < Q; ++q) {
      const long long th = thr[q];
      long long acc = 0;
      unsigned sel = my[0];  // none reaches it: the smallest value
      for (int i = 0; i < M; ++i) {
        const unsigned key = my[i * R];
        acc += qw[key & 255u];
        if (acc >= th) {
          sel = key;
          break;
        }
      }
      out[row * Q + q] = leaf_table[min((int)(sel >> 8), U - 1)];
    }
#endif
  }
}

}  // namespace

// (rows per block, member limit) x 3 in ascending member limit, row-tile grid
// cap, key slab bytes, nodes per LDS group
std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
           int64_t, int64_t>
forest_wquantile_geometry() {
  return {kWqR0, kWqM0, kWqR1, kWqM1, kWqR2, kWqM2,
          kWqMaxBlocks, kWqSlabBytes, kWqGroupNodes};
}

void forest_wquantile(torch::Tensor out, torch::Tensor x, torch::Tensor nodes,
                      torch::Tensor tree_off, torch::Tensor groups,
                      torch::Tensor qtab, torch::Tensor leaf_table,
                      int64_t max_group_nodes) {
  CHECK_GPU(out); CHECK_GPU(x); CHECK_GPU(nodes); CHECK_GPU(tree_off);
  CHECK_GPU(groups); CHECK_GPU(qtab); CHECK_GPU(leaf_table);
  CHECK_CONTIG(out); CHECK_CONTIG(x); CHECK_CONTIG(nodes);
  CHECK_CONTIG(tree_off); CHECK_CONTIG(groups); CHECK_CONTIG(qtab);
  CHECK_CONTIG(leaf_table);
  const bool binned = x.scalar_type() == torch::kUInt8;
  TORCH_CHECK((binned || x.scalar_type() == torch::kFloat32) && x.dim() == 2,
              "forest_wquantile: x is [N, F] f32 or u8");
  const int64_t n = x.size(0);
  const int64_t F = x.size(1);
  const int64_t G = groups.numel() / 4;
  const int64_t M = tree_off.numel();
  TORCH_CHECK(n >= 1 && F >= 1 && F < 32768, "forest_wquantile: x shape");
  TORCH_CHECK(out.scalar_type() == torch::kFloat32 && out.dim() == 2 &&
                  out.size(0) == n && out.size(1) >= 1 &&
                  out.size(1) <= kWqMaxQ,
              "forest_wquantile: out is [N, Q] f32, 1 <= Q <= 16");
  const int64_t Q = out.size(1);
  TORCH_CHECK(nodes.scalar_type() == torch::kInt64 &&
                  tree_off.scalar_type() == torch::kInt32 &&
                  groups.scalar_type() == torch::kInt32 &&
                  groups.numel() == G * 4,
              "forest_wquantile: pack tensors");
  TORCH_CHECK(M >= 1 && M <= kWqMaxM && G >= 1 && G <= M,
              "forest_wquantile: 1 <= members <= 256, groups cover them");
  TORCH_CHECK(qtab.scalar_type() == torch::kInt64 && qtab.numel() == M + Q,
              "forest_wquantile: qtab is [M + Q] i64");
  const int64_t U = leaf_table.numel();
  TORCH_CHECK(leaf_table.scalar_type() == torch::kFloat32 && U >= 1 &&
                  U <= (1 << 24),
              "forest_wquantile: leaf_table is [U] f32, 1 <= U <= 2^24");
  TORCH_CHECK(max_group_nodes >= 1 && max_group_nodes <= nodes.numel() &&
                  max_group_nodes <= kWqGroupNodes,
              "forest_wquantile: group too big for LDS");
  int Mp = 1;
  while (Mp < M) Mp <<= 1;
  const int R = Mp <= kWqM0 ? kWqR0 : Mp <= kWqM1 ? kWqR1 : kWqR2;
  const size_t lds = (size_t)kWqTabBytes + (size_t)Mp * R * 4 +
                     (size_t)max_group_nodes * 8;
  const int64_t n_tiles = ceil_div(n, (int64_t)R);
  const int blocks = (int)std::min<int64_t>(n_tiles, kWqMaxBlocks);
  auto stream = at::hip::getCurrentHIPStream();
#define WQ_LAUNCH(RR, BB)                                                     \
  do {                                                                        \
    if (lds > 65536)                                                          \
      TORCH_CHECK(                                                            \
          hipFuncSetAttribute(                                                \
              reinterpret_cast<const void*>(                                  \
                  &forest_wquantile_kernel<RR, BB>),                          \
              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) ==        \
              hipSuccess,                                                     \
          "forest_wquantile: cannot reserve ", lds, " bytes of LDS");         \
    hipLaunchKernelGGL((forest_wquantile_kernel<RR, BB>), dim3(blocks),       \
                       dim3(RR), lds, stream, out.data_ptr<float>(),          \
                       x.data_ptr(),                                          \
                       (const unsigned long long*)nodes.data_ptr<int64_t>(),  \
                       tree_off.data_ptr<int>(), groups.data_ptr<int>(),      \
                       (const long long*)qtab.data_ptr<int64_t>(),            \
                       leaf_table.data_ptr<float>(), n, (int)F, (int)G,       \
                       (int)M, Mp, (int)Q, (int)U, n_tiles);                  \
  } while (0)
#define WQ_ROWS(RR)                  \
  do {                               \
    if (binned) WQ_LAUNCH(RR, true); \
    else WQ_LAUNCH(RR, false);       \
  } while (0)
  if (R == kWqR0) WQ_ROWS(kWqR0);
  else if (R == kWqR1) WQ_ROWS(kWqR1);
  else WQ_ROWS(kWqR2);
#undef WQ_ROWS
#undef WQ_LAUNCH
  // a refused launch must raise: out is uninitialised memory
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "forest_wquantile: kernel launch failed: ",
              hipGetErrorString(err));
}
