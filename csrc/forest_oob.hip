// forest_oob: out-of-bag sums and counts of a bagged forest, in one pass over
// the rows, for gfx950.
//
//   sums[i, :] = sum over t with bit t of row i's mask CLEAR, t = 0 .. T-1 in
//                order, of leaf_t(x_i)                          f32 [N, D]
//   counts[i]  = number of such t                               i32 [N]
//
// A set bit means "row i was in tree t's bag".  A per-member loop (predict
// every row, mask, add) walks all N * T (row, tree) pairs and throws ~63 % of
// them away under a bootstrap; here a lane whose bit is set skips the walk.
// The skip is per lane: at bootstrap density nearly every wave has an
// out-of-bag lane for every tree, so a wave still issues about a full walk
// and what the skipped lanes save is their gathers of x and of LDS nodes,
// not issue time: measured, the kernel is 26-30 % faster than a full
// forest_predict of the same rows, not 63 % (profiles/oob.md).
//
// Mapping.  That of forest_staged_loss (csrc/forest_staged.hip): the forest
// arrives as forest_predict2 packs it, one u64 per node (feature s16 | left
// child s16 | threshold or leaf f32), trees cut into LDS groups.  A block
// owns a tile of kOobThreads * kOobRows rows and walks the groups IN ORDER:
// stage group g's nodes into LDS, barrier, every lane walks the group's
// trees for its rows, next group.  A row's acc[D] and its count stay in
// registers from the first group to the last and are stored once: no
// atomics, no pre-zeroed output, and the sums are in tree order, so integer
// leaves give bitwise the result of the reference op.
//
// Mask.  [W, N] i32, W = ceil(T / 32): word t >> 5, bit t & 31 of row i at
// mask[(t >> 5) * N + i].  Word-major, so the 64 lanes of a wave (64
// consecutive rows) read 256 consecutive bytes.  The tree index is the GLOBAL
// one (first_tree + t), never reset at a group, and a lane reloads its words
// whenever that index enters another word; a group boundary may fall inside
// a word.
//
// Rows per lane.  One block per CU fits beside a full group of nodes, so 16
// waves per CU leave 128 VGPRs per lane.  At D = 8 a row holds 8 sums, a
// count and a mask word.  The compiler's resource report for the D = 8
// instances (profiles/oob.md): kOobRows = 4 takes 68 VGPRs and no scratch;
// 8 rows take 126 of the 128, scratch-free only by two registers, for half
// as many stagings of a group.  4 it is, as in forest_staged_loss.  The rows
// of a lane are walked one after the other, each in a loop of its own, under
// a per-lane branch on the mask bit; forest_predict2 and forest_staged_loss
// both measured merged multi-row walk loops as slower.
//
// Leaves.  D == 1 takes the leaf from the node payload (the pack is built
// with tree weights 1.0).  D > 1 reads leaves[(node_base + node) * D + d].
//
// Row access is forest_predict2's: f32 rows against f32 thresholds, or u8
// rank rows (bin_features against the pack's own threshold sets) against
// threshold ranks.  Either is exact; the caller picks by a static rule.

#include <ATen/hip/HIPContext.h>

#include <tuple>

#include "common.h"

namespace {

constexpr int kOobThreads = 1024;
constexpr int kOobRows = 4;  // rows per lane, walked one after the other
constexpr int kOobTile = kOobThreads * kOobRows;
constexpr int kOobMaxBlocks = 512;  // two rounds of one block per CU

template <int D, bool BINNED>
__global__ __launch_bounds__(kOobThreads) void forest_oob_kernel(
    float* __restrict__ sums,                      // [N, D]
    int* __restrict__ counts,                      // [N]
    const void* __restrict__ xv_,                  // [N, F] f32 | u8
    const unsigned long long* __restrict__ nodes,  // [total] packed
    const float* __restrict__ leaves,              // [total, D] (D > 1)
    const int* __restrict__ tree_off,              // [T] global node base
    const int* __restrict__ groups,                // [G, 4]
    const int* __restrict__ mask,                  // [W, N] in-bag bits
    int64_t n, int F, int G, int64_t n_tiles) {
  extern __shared__ __align__(16) unsigned long long tlds[];  // group nodes

  // block-uniform trip count: every thread reaches every barrier
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kOobTile + threadIdx.x;
    float acc[kOobRows][D];
    int cnt[kOobRows];
    unsigned mw[kOobRows];
#pragma unroll
    for (int r = 0; r < kOobRows; ++r) {
      cnt[r] = 0;
      mw[r] = 0u;
#pragma unroll
      for (int d = 0; d < D; ++d) acc[r][d] = 0.0f;
    }

    int word = -1;  // the mask word held in mw, block-uniform
    for (int g = 0; g < G; ++g) {
      const int* grp = groups + g * 4;
      const int first_tree = grp[0];
      const int n_trees = grp[1];
      const int node_base = grp[2];
      const int n_nodes = grp[3];
      __syncthreads();  // the previous group's walks are done
      for (int i = threadIdx.x; i < n_nodes; i += kOobThreads)
        tlds[i] = nodes[node_base + i];
      __syncthreads();

      for (int t = 0; t < n_trees; ++t) {
        const int gt = first_tree + t;  // global tree index selects the bit
        if ((gt >> 5) != word) {
          word = gt >> 5;
#pragma unroll
          for (int r = 0; r < kOobRows; ++r) {
            const int64_t row = row0 + (int64_t)r * kOobThreads;
            mw[r] = row < n ? (unsigned)mask[(int64_t)word * n + row] : ~0u;
          }
        }
        const int bit = gt & 31;
        const int toff = tree_off[gt] - node_base;
#pragma unroll
        for (int r = 0; r < kOobRows; ++r) {
          const int64_t row = row0 + (int64_t)r * kOobThreads;
          // per-lane branch: an in-bag (or dead) lane skips the walk
          if (row < n && !((mw[r] >> bit) & 1u)) {
            const float* xr = BINNED ? nullptr : (const float*)xv_ + row * F;
            const uint8_t* br =
                BINNED ? (const uint8_t*)xv_ + row * F : nullptr;
            int node = toff;
            unsigned long long nd = tlds[node];
            int f = (short)(nd & 0xFFFFu);
            while (f >= 0) {
              const int left = (short)((nd >> 16) & 0xFFFFu);
              bool go_left;
              if (BINNED)
                go_left = br[f] <= (unsigned)(nd >> 32);
              else
                go_left = xr[f] <= __uint_as_float((unsigned)(nd >> 32));
              node = toff + left + (go_left ? 0 : 1);
              nd = tlds[node];
              f = (short)(nd & 0xFFFFu);
            }
            if (D == 1) {
              acc[r][0] += __uint_as_float((unsigned)(nd >> 32));
            } else {
              const float* lv = leaves + (int64_t)(node_base + node) * D;
#pragma unroll
              for (int d = 0; d < D; ++d) acc[r][d] += lv[d];
            }
            ++cnt[r];
          }
        }
      }
    }

#pragma unroll
    for (int r = 0; r < kOobRows; ++r) {
      const int64_t row = row0 + (int64_t)r * kOobThreads;
      if (row < n) {
        counts[row] = cnt[r];
#pragma unroll
        for (int d = 0; d < D; ++d) sums[row * D + d] = acc[r][d];
      }
    }
  }
}

}  // namespace

std::tuple<int64_t, int64_t, int64_t> forest_oob_geometry() {
  return {kOobThreads, kOobRows, kOobMaxBlocks};
}

void forest_oob(torch::Tensor sums, torch::Tensor counts, torch::Tensor x,
                torch::Tensor nodes, torch::Tensor leaves,
                torch::Tensor tree_off, torch::Tensor groups,
                torch::Tensor mask, int64_t dim, int64_t max_group_nodes) {
  CHECK_GPU(sums); CHECK_GPU(counts); CHECK_GPU(x); CHECK_GPU(nodes);
  CHECK_GPU(leaves); CHECK_GPU(tree_off); CHECK_GPU(groups); CHECK_GPU(mask);
  CHECK_CONTIG(sums); CHECK_CONTIG(counts); CHECK_CONTIG(x);
  CHECK_CONTIG(nodes); CHECK_CONTIG(leaves); CHECK_CONTIG(tree_off);
  CHECK_CONTIG(groups); CHECK_CONTIG(mask);
  const bool binned = x.scalar_type() == torch::kUInt8;
  TORCH_CHECK((binned || x.scalar_type() == torch::kFloat32) && x.dim() == 2,
              "forest_oob: x is [N, F] f32 or u8");
  TORCH_CHECK(dim >= 1 && dim <= 8, "forest_oob: 1 <= dim <= 8");
  const int64_t n = x.size(0);
  const int64_t F = x.size(1);
  const int64_t G = groups.numel() / 4;
  const int64_t T = tree_off.numel();
  TORCH_CHECK(n >= 1 && F >= 1 && F < 32768, "forest_oob: x shape");
  TORCH_CHECK(sums.scalar_type() == torch::kFloat32 &&
                  sums.numel() == n * dim,
              "forest_oob: sums is [N, dim] f32");
  TORCH_CHECK(counts.scalar_type() == torch::kInt32 && counts.numel() == n,
              "forest_oob: counts is [N] i32");
  TORCH_CHECK(nodes.scalar_type() == torch::kInt64 &&
                  tree_off.scalar_type() == torch::kInt32 &&
                  groups.scalar_type() == torch::kInt32 &&
                  groups.numel() == G * 4,
              "forest_oob: pack tensors");
  TORCH_CHECK(T >= 1 && G >= 1 && G <= T, "forest_oob: groups cover trees");
  TORCH_CHECK(leaves.scalar_type() == torch::kFloat32 &&
                  leaves.numel() == nodes.numel() * dim,
              "forest_oob: leaves is [total nodes, dim] f32");
  const int64_t W = ceil_div(T, (int64_t)32);
  TORCH_CHECK(mask.scalar_type() == torch::kInt32 && mask.numel() == W * n,
              "forest_oob: mask is [ceil(T / 32), N] i32");
  const size_t lds = (size_t)max_group_nodes * 8;
  TORCH_CHECK(max_group_nodes >= 1 && max_group_nodes <= nodes.numel() &&
                  lds <= 163840,
              "forest_oob: group too big for LDS");
  const int64_t n_tiles = ceil_div(n, (int64_t)kOobTile);
  auto stream = at::hip::getCurrentHIPStream();
  const int blocks = (int)std::min<int64_t>(n_tiles, kOobMaxBlocks);
#define FO_LAUNCH(DD, BB)                                                     \
  do {                                                                        \
    if (lds > 65536)                                                          \
      TORCH_CHECK(                                                            \
          hipFuncSetAttribute(                                                \
              reinterpret_cast<const void*>(&forest_oob_kernel<DD, BB>),      \
              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) ==        \
              hipSuccess,                                                     \
          "forest_oob: cannot reserve ", lds, " bytes of LDS");               \
    hipLaunchKernelGGL((forest_oob_kernel<DD, BB>), dim3(blocks),             \
                       dim3(kOobThreads), lds, stream,                        \
                       sums.data_ptr<float>(), counts.data_ptr<int>(),        \
                       x.data_ptr(),                                          \
                       (const unsigned long long*)nodes.data_ptr<int64_t>(),  \
                       leaves.data_ptr<float>(), tree_off.data_ptr<int>(),    \
                       groups.data_ptr<int>(), mask.data_ptr<int>(), n,       \
                       (int)F, (int)G, n_tiles);                              \
  } while (0)
#define FO_DIM(DD)                   \
  case DD:                           \
    if (binned) FO_LAUNCH(DD, true); \
    else FO_LAUNCH(DD, false);       \
    break;
  switch (dim) {
    FO_DIM(1) FO_DIM(2) FO_DIM(3) FO_DIM(4)
    FO_DIM(5) FO_DIM(6) FO_DIM(7) FO_DIM(8)
  }
#undef FO_DIM
#undef FO_LAUNCH
  // a refused launch must raise: sums and counts are uninitialised memory
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "forest_oob: kernel launch failed: ",
              hipGetErrorString(err));
}
