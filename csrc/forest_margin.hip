// forest_margin: the margins of a multi-plane boosted forest of scalar-leaf
// trees, every plane in one pass over the rows, for gfx950.
//
//   out[i, j] = sum over trees t with plane(t) = j, in pack order, of
//               payload(leaf_t(x_i))                        f32 [N, P], P >= 2
//
// A K-class GBM holds stages x K scalar regression trees; tree (stage, j)
// adds weight * leaf to margin column j.  forest_predict2 serves one column
// per call (its D > 1 form wants D-wide leaf rows, K - 1 zeros per leaf here,
// and stops at D = 8), so the rows were rank-transformed and walked once per
// class.  What this forest has and the others lack is the PLANE of a tree:
// known on the host and the same for every row.
//
// Pack order is plane-major: the host sorts the trees stably by plane (stage
// order survives inside a plane) and cuts them into forest_predict2's LDS
// groups of u64 node words (feature s16 | left child s16 | 32-bit payload).
// A leaf's payload is the f32 bits of weight * leaf, so no leaf tensor is
// read.  A per-tree i32 plane table rides beside tree_off.
//
// Mapping.  That of forest_vote / forest_oob: a block owns a tile of
// kMarginThreads * kMarginRows rows and walks the groups IN ORDER: stage
// group g's nodes into LDS, barrier, every lane walks the group's trees for
// its rows, one row after the other, each in a walk loop of its own (merged
// multi-row walk loops measured slower in three kernels of this tree).  Trip
// counts are block-uniform, so every thread reaches every barrier.
//
// One accumulator per row, acc[R], statically indexed, whatever P is.  The
// plane of the current tree is a block-uniform scalar read from the table.
// When it changes, the lane stores acc[r] to out[row_r * P + cur], clears it
// and goes on.  The accumulator carries across group boundaries (a plane may
// straddle groups, a group may hold many planes) and the last plane is stored
// after the last group.  No atomics, no pre-zeroed output (a plane WITHOUT
// trees is never stored: the host zero-fills out when there is one), no
// local array indexed by a runtime value.  Each element is a sum in stage
// order from +0.0f: bit-reproducible, and bitwise forest_predict2's D == 1
// result wherever that forest fits one group.
//
// Stores.  A flush is one 4-byte store per row at stride P * 4 bytes across
// the lanes, P flushes per tile.  They are LEFT as they are, not transposed
// through LDS into full lines: a full node group leaves 1 KiB of the CU's
// 160 KiB of LDS, a tile's plane is 16 KiB, so a transpose buffer would have
// to come out of the group budget (more groups, more stagings, and packs that
// no longer share forest_predict2's group rule) or reuse the node LDS under
// two more barriers and a restaging per flush.  The traffic does not pay for
// that: N * P * 4 bytes are written once against N * T * depth dependent LDS
// hops.  Measured (profiles/forest_margin.md): the same 2600 trees cut into
// 2 planes or into 26 take the same time within the spread.
//
// Rows per lane.  One block per CU beside a full node group: 16 waves per
// CU, 128 VGPRs per lane.  A row costs one accumulator and its row pointer.
// The compiler's resource report for gfx950 (profiles/forest_margin.md) has
// no scratch at R = 4 or 8 in either row form; R = 4 is used, as in the
// sibling kernels: staging a group is ~1.5 % of a depth-8 tile's hops at
// R = 4 already, and a tile of 4096 rows fills 256 CUs from 1M rows on where
// 8192 would need 2M.
//
// Row access is forest_predict2's row-major forms: f32 rows against f32
// thresholds, or u8 rank rows (bin_features against the pack's own threshold
// sets) against threshold ranks.  Either is exact; the caller picks by a
// static rule.  There is no transposed u8 form here, and it is missed: with
// 256-byte rows every hop of a wave touches 64 cache lines, and the per-class
// forest_predict2 route in its transposed form is 3.9x faster at 2M x 256
// rows, while at 16 features this kernel is level or ahead
// (profiles/forest_margin.md).  ensemble.utils.packed_forest_margins routes
// by the feature count for that reason.

#include <ATen/hip/HIPContext.h>

#include <tuple>

#include "common.h"

namespace {

constexpr int kMarginThreads = 1024;
constexpr int kMarginRows = 4;         // rows per lane, walked one by one
constexpr int kMarginMaxBlocks = 512;  // two rounds of one block per CU

// Walks one tree of the staged group for one row; returns the leaf's payload.
template <bool BINNED>
__device__ __forceinline__ float margin_walk(
    const unsigned long long* __restrict__ tlds, int toff,
    const void* __restrict__ xrow) {
  const float* xr = (const float*)xrow;
  const uint8_t* br = (const uint8_t*)xrow;
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
  return __uint_as_float((unsigned)(nd >> 32));  // weight * leaf
}

template <int R, bool BINNED>
__global__ __launch_bounds__(kMarginThreads) void forest_margin_kernel(
    float* __restrict__ out,                       // [N, P]
    const void* __restrict__ xv_,                  // [N, F] f32 | u8
    const unsigned long long* __restrict__ nodes,  // [total] packed
    const int* __restrict__ tree_off,              // [T] global node base
    const int* __restrict__ tree_plane,            // [T] non-decreasing
    const int* __restrict__ groups,                // [G, 4]
    int64_t n, int F, int P, int G, int64_t n_tiles) {
  extern __shared__ __align__(16) unsigned long long tlds[];  // group nodes
  constexpr int kTile = kMarginThreads * R;
  const int64_t xstride = (int64_t)F * (BINNED ? 1 : 4);

  // block-uniform trip count: every thread reaches every barrier
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kTile + threadIdx.x;
    float acc[R];
    const char* xp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      acc[r] = 0.0f;
      const int64_t row = row0 + (int64_t)r * kMarginThreads;
      // a dead row keeps row 0's pointer and is never walked
      xp[r] = (const char*)xv_ + (row < n ? row : 0) * xstride;
    }

    int cur = tree_plane[0];  // the plane acc holds, block-uniform
    for (int g = 0; g < G; ++g) {
      const int* grp = groups + g * 4;
      const int first_tree = grp[0];
      const int n_trees = grp[1];
      const int node_base = grp[2];
      const int n_nodes = grp[3];
      __syncthreads();  // the previous group's walks are done
      for (int i = threadIdx.x; i < n_nodes; i += kMarginThreads)
        tlds[i] = nodes[node_base + i];
      __syncthreads();

      for (int t = 0; t < n_trees; ++t) {
        const int gt = first_tree + t;
        const int plane = tree_plane[gt];
        if (plane != cur) {  // block-uniform: flush the finished plane
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int64_t row = row0 + (int64_t)r * kMarginThreads;
            if (row < n) out[row * P + cur] = acc[r];
            acc[r] = 0.0f;
          }
          cur = plane;
        }
        const int toff = tree_off[gt] - node_base;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t row = row0 + (int64_t)r * kMarginThreads;
          if (row < n) acc[r] += margin_walk<BINNED>(tlds, toff, xp[r]);
        }
      }
    }

#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row0 + (int64_t)r * kMarginThreads;
      if (row < n) out[row * P + cur] = acc[r];
    }
  }
}

}  // namespace

// (threads, rows per lane, grid cap)
std::tuple<int64_t, int64_t, int64_t> forest_margin_geometry() {
  return {kMarginThreads, kMarginRows, kMarginMaxBlocks};
}

// tree_plane is in pack order and non-decreasing (the host sorts by plane and
// checks the range); a plane that no tree names is left unwritten.
void forest_margin(torch::Tensor out, torch::Tensor x, torch::Tensor nodes,
                   torch::Tensor tree_off, torch::Tensor tree_plane,
                   torch::Tensor groups, int64_t num_planes,
                   int64_t max_group_nodes) {
  CHECK_GPU(out); CHECK_GPU(x); CHECK_GPU(nodes); CHECK_GPU(tree_off);
  CHECK_GPU(tree_plane); CHECK_GPU(groups);
  CHECK_CONTIG(out); CHECK_CONTIG(x); CHECK_CONTIG(nodes);
  CHECK_CONTIG(tree_off); CHECK_CONTIG(tree_plane); CHECK_CONTIG(groups);
  const bool binned = x.scalar_type() == torch::kUInt8;
  TORCH_CHECK((binned || x.scalar_type() == torch::kFloat32) && x.dim() == 2,
              "forest_margin: x is [N, F] f32 or u8");
  const int64_t P = num_planes;
  const int64_t n = x.size(0);
  const int64_t F = x.size(1);
  const int64_t G = groups.numel() / 4;
  const int64_t T = tree_off.numel();
  TORCH_CHECK(P >= 2 && P < (1 << 20), "forest_margin: num_planes >= 2");
  TORCH_CHECK(F >= 1 && F < 32768, "forest_margin: x shape");
  TORCH_CHECK(out.scalar_type() == torch::kFloat32 && out.numel() == n * P,
              "forest_margin: out is [N, num_planes] f32");
  TORCH_CHECK(nodes.scalar_type() == torch::kInt64 &&
                  tree_off.scalar_type() == torch::kInt32 &&
                  tree_plane.scalar_type() == torch::kInt32 &&
                  tree_plane.numel() == T &&
                  groups.scalar_type() == torch::kInt32 &&
                  groups.numel() == G * 4,
              "forest_margin: pack tensors");
  TORCH_CHECK(T >= 1 && G >= 1 && G <= T, "forest_margin: groups cover trees");
  const size_t lds = (size_t)max_group_nodes * 8;
  TORCH_CHECK(max_group_nodes >= 1 && max_group_nodes <= nodes.numel() &&
                  lds <= 163840,
              "forest_margin: group too big for LDS");
  if (n == 0) return;  // the grid is sized by N
  auto stream = at::hip::getCurrentHIPStream();
  const int64_t n_tiles = ceil_div(n, (int64_t)kMarginThreads * kMarginRows);
  const int blocks = (int)std::min<int64_t>(n_tiles, kMarginMaxBlocks);
#define FM_LAUNCH(BB)                                                         \
  do {                                                                        \
    if (lds > 65536)                                                          \
      TORCH_CHECK(                                                            \
          hipFuncSetAttribute(                                                \
              reinterpret_cast<const void*>(                                  \
                  &forest_margin_kernel<kMarginRows, BB>),                    \
              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) ==        \
              hipSuccess,                                                     \
          "forest_margin: cannot reserve ", lds, " bytes of LDS");            \
    hipLaunchKernelGGL((forest_margin_kernel<kMarginRows, BB>), dim3(blocks), \
                       dim3(kMarginThreads), lds, stream,                     \
                       out.data_ptr<float>(), x.data_ptr(),                   \
                       (const unsigned long long*)nodes.data_ptr<int64_t>(),  \
                       tree_off.data_ptr<int>(), tree_plane.data_ptr<int>(),  \
                       groups.data_ptr<int>(), n, (int)F, (int)P, (int)G,     \
                       n_tiles);                                              \
  } while (0)
  if (binned) FM_LAUNCH(true);
  else FM_LAUNCH(false);
#undef FM_LAUNCH
  // a refused launch must raise: out is uninitialised memory
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "forest_margin: kernel launch failed: ",
              hipGetErrorString(err));
}
