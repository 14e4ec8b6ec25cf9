// forest_staged_loss: the loss of a boosted forest after EVERY stage, in one
// pass over the rows, for gfx950.
//
//   out[s] = sum_i w_i * loss(label_i, init_i + sum_{t < s * DIM} w_t leaf_t(x_i))
//
// for s = 0 .. S.  Tree t belongs to stage t / DIM and adds into margin
// column t % DIM.  The per-stage loop this replaces reads x once per stage
// and launches a predict, an add and a loss reduction per stage; here x is
// read once for the whole curve and no [N, S] intermediate exists.
//
// Mapping.  The forest arrives as forest_predict2 packs it (csrc/ops.hip):
// one u64 per node (feature s16 | left child s16 | threshold or weighted
// leaf f32), trees cut into groups of at most ~159 KiB of nodes.  A block
// owns a tile of kStagedThreads * kStagedRows rows and walks the groups IN
// ORDER: stage group g's nodes into LDS, barrier, every lane walks the
// group's trees for its rows, next group.  A row's margins (DIM <= 8), its
// label and its weight stay in registers from the first group to the last.
// A group boundary may fall inside a stage, so the stage and column counters
// run over the whole forest and are never reset at a group.
//
// Rows per lane.  One block per CU fits beside 159 KiB of nodes, and every
// (tile, group) pair re-reads the group from L2, so a lane takes
// kStagedRows = 4 rows: 4096 rows share one staging.  The rows are walked
// one after the other, each in a loop of its own; forest_predict2 found
// merged multi-row walk loops 1.5-4x slower.  The budget is registers: 16
// waves per CU leave 128 VGPRs per lane, and at DIM = 8 four rows hold
// 4 * (8 margins + 8 labels + 1 weight) = 68 of them.  Eight rows would not
// fit without spilling; the compiler's resource report for the DIM = 8
// instance is in profiles/staged_eval.md.
//
// Loss and reduction.  After the last tree of a stage every lane evaluates
// w * loss(label, margin) in f32 for its rows: the scalar losses through
// scalar_loss_grad (gradient and hessian discarded), logloss through
// softmax_xent (csrc/gbm_loss.h).  Nothing is clamped: a NaN or an inf
// reaches the result.  The lane's rows are summed in f64, the wave reduces by
// shuffle, and lane 0 stores the wave's sum at partials[tile * 16 + wave][s],
// a cell no other wave writes and that is written exactly once.  No atomics,
// no block barrier per stage.  forest_staged_reduce_kernel then sums the
// slots of each stage in a fixed order.  Every sum past the per-row f32 loss
// is f64 in a fixed order, so the result is bitwise reproducible and its
// rounding is that of the per-row loss alone.
//
// Row access is forest_predict2's: f32 rows against f32 thresholds, or u8
// rank rows (bin_features against the pack's own threshold sets) against
// threshold ranks.  Either is exact; the caller picks by a static rule.

#include <ATen/hip/HIPContext.h>

#include <tuple>

#include "common.h"
#include "gbm_loss.h"

namespace {

constexpr int kStagedThreads = 1024;
constexpr int kStagedWaves = kStagedThreads / 64;
constexpr int kStagedRows = 4;  // rows per lane, walked one after the other
constexpr int kStagedTile = kStagedThreads * kStagedRows;
constexpr int kStagedMaxBlocks = 512;  // two rounds of one block per CU
constexpr int kReduceThreads = 256;

template <int DIM>
__device__ __forceinline__ float staged_row_loss(int loss_id, float param,
                                                 const float* label,
                                                 const float* margin) {
  if (loss_id == L_LOGLOSS) return softmax_xent<DIM>(label, margin);
  float g, h;
  return scalar_loss_grad(loss_id, param, label[0], margin[0], &g, &h);
}

template <int DIM, bool BINNED>
__global__ __launch_bounds__(kStagedThreads) void forest_staged_kernel(
    double* __restrict__ partials,                 // [n_tiles * 16, S + 1]
    const void* __restrict__ xv_,                  // [N, F] f32 | u8
    const unsigned long long* __restrict__ nodes,  // [total] packed
    const int* __restrict__ tree_off,              // [T] global node base
    const int* __restrict__ groups,                // [G, 4]
    const float* __restrict__ init,                // [N, DIM]
    const float* __restrict__ label,               // [N, DIM]
    const float* __restrict__ weight,              // [N]
    int64_t n, int F, int G, int S1, int loss_id, float param,
    int64_t n_tiles) {
  extern __shared__ __align__(16) unsigned long long tlds[];  // group nodes
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  // block-uniform trip count: every thread reaches every barrier
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kStagedTile + threadIdx.x;
    float mg[kStagedRows][DIM], lab[kStagedRows][DIM], wt[kStagedRows];
#pragma unroll
    for (int r = 0; r < kStagedRows; ++r) {
      const int64_t row = row0 + (int64_t)r * kStagedThreads;
      const bool live = row < n;
      wt[r] = live ? weight[row] : 0.0f;
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        mg[r][d] = live ? init[row * DIM + d] : 0.0f;
        lab[r][d] = live ? label[row * DIM + d] : 0.0f;
      }
    }
    double* __restrict__ prow =
        partials + (tile * kStagedWaves + wave) * (int64_t)S1;

    // the wave's weighted loss at the current margins -> prow[s]; called
    // from wave-uniform control flow only, so every lane runs the shuffles
    auto emit = [&](int s) {
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < kStagedRows; ++r) {
        const float l = wt[r] * staged_row_loss<DIM>(loss_id, param, lab[r],
                                                     mg[r]);
        if (row0 + (int64_t)r * kStagedThreads < n) acc += (double)l;
      }
      for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
      if (lane == 0) prow[s] = acc;
    };

    emit(0);
    int stage = 0, col = 0;  // run over the whole forest, not per group
    for (int g = 0; g < G; ++g) {
      const int* grp = groups + g * 4;
      const int first_tree = grp[0];
      const int n_trees = grp[1];
      const int node_base = grp[2];
      const int n_nodes = grp[3];
      __syncthreads();  // the previous group's walks are done
      for (int i = threadIdx.x; i < n_nodes; i += kStagedThreads)
        tlds[i] = nodes[node_base + i];
      __syncthreads();

      for (int t = 0; t < n_trees; ++t) {
        const int toff = tree_off[first_tree + t] - node_base;
#pragma unroll
        for (int r = 0; r < kStagedRows; ++r) {
          const int64_t row = row0 + (int64_t)r * kStagedThreads;
          if (row < n) {
            const float* xr = BINNED ? nullptr : (const float*)xv_ + row * F;
            const uint8_t* br =
                BINNED ? (const uint8_t*)xv_ + row * F : nullptr;
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
            const float v = __uint_as_float((unsigned)(nd >> 32));
            // col is wave-uniform; the select keeps mg in registers
#pragma unroll
            for (int d = 0; d < DIM; ++d) mg[r][d] += (d == col) ? v : 0.0f;
          }
        }
        if (++col == DIM) {
          col = 0;
          emit(++stage);
        }
      }
    }
  }
}

// out[s] = sum over slots of partials[slot][s]: thread j sums slots j,
// j + 256, ... in order, then the 256 thread sums are added in order.
__global__ __launch_bounds__(kReduceThreads) void forest_staged_reduce_kernel(
    double* __restrict__ out, const double* __restrict__ partials,
    int64_t n_slots, int S1) {
  __shared__ double lp[kReduceThreads];
  const int s = blockIdx.x;
  double v = 0.0;
  for (int64_t k = threadIdx.x; k < n_slots; k += kReduceThreads)
    v += partials[k * S1 + s];
  lp[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int j = 0; j < kReduceThreads; ++j) t += lp[j];
    out[s] = t;
  }
}

}  // namespace

std::tuple<int64_t, int64_t, int64_t> forest_staged_geometry() {
  return {kStagedThreads, kStagedRows, kStagedMaxBlocks};
}

void forest_staged_loss(torch::Tensor out, torch::Tensor partials,
                        torch::Tensor x, torch::Tensor nodes,
                        torch::Tensor tree_off, torch::Tensor groups,
                        torch::Tensor init, torch::Tensor label,
                        torch::Tensor weight, int64_t dim,
                        int64_t max_group_nodes, int64_t loss_id,
                        double param) {
  CHECK_GPU(out); CHECK_GPU(partials); CHECK_GPU(x); CHECK_GPU(nodes);
  CHECK_GPU(tree_off); CHECK_GPU(groups); CHECK_GPU(init); CHECK_GPU(label);
  CHECK_GPU(weight);
  CHECK_CONTIG(out); CHECK_CONTIG(partials); CHECK_CONTIG(x);
  CHECK_CONTIG(nodes); CHECK_CONTIG(tree_off); CHECK_CONTIG(groups);
  CHECK_CONTIG(init); CHECK_CONTIG(label); CHECK_CONTIG(weight);
  const bool binned = x.scalar_type() == torch::kUInt8;
  TORCH_CHECK((binned || x.scalar_type() == torch::kFloat32) && x.dim() == 2,
              "forest_staged_loss: x is [N, F] f32 or u8");
  TORCH_CHECK(dim >= 1 && dim <= 8, "forest_staged_loss: 1 <= dim <= 8");
  TORCH_CHECK(loss_id >= L_SQUARED && loss_id <= L_BERNOULLI,
              "forest_staged_loss: unknown loss id");
  TORCH_CHECK(dim == 1 || loss_id == L_LOGLOSS,
              "forest_staged_loss: dim > 1 only for logloss");
  const int64_t n = x.size(0);
  const int64_t F = x.size(1);
  const int64_t G = groups.numel() / 4;
  const int64_t T = tree_off.numel();
  TORCH_CHECK(T % dim == 0, "forest_staged_loss: trees are whole stages");
  const int64_t S1 = T / dim + 1;
  TORCH_CHECK(out.scalar_type() == torch::kFloat64 && out.numel() == S1,
              "forest_staged_loss: out is [S + 1] f64");
  TORCH_CHECK(nodes.scalar_type() == torch::kInt64 &&
                  tree_off.scalar_type() == torch::kInt32 &&
                  groups.scalar_type() == torch::kInt32 &&
                  groups.numel() == G * 4,
              "forest_staged_loss: pack tensors");
  TORCH_CHECK((G == 0) == (T == 0), "forest_staged_loss: groups cover trees");
  TORCH_CHECK(init.scalar_type() == torch::kFloat32 &&
                  label.scalar_type() == torch::kFloat32 &&
                  weight.scalar_type() == torch::kFloat32,
              "forest_staged_loss: init, label and weight are f32");
  TORCH_CHECK(init.numel() == n * dim && label.numel() == n * dim &&
                  weight.numel() == n,
              "forest_staged_loss: init / label / weight do not match x");
  TORCH_CHECK(n >= 1 && F >= 1 && F < 32768, "forest_staged_loss: x shape");
  const int64_t n_tiles = ceil_div(n, (int64_t)kStagedTile);
  const int64_t n_slots = n_tiles * kStagedWaves;
  TORCH_CHECK(partials.scalar_type() == torch::kFloat64 &&
                  partials.numel() == n_slots * S1,
              "forest_staged_loss: partials is [tiles * 16, S + 1] f64");
  // one reduce block per curve entry: gridDim.x holds up to 2^31 - 1
  TORCH_CHECK(S1 <= 0x7FFFFFFF, "forest_staged_loss: stage count");
  const size_t lds = (size_t)max_group_nodes * 8;
  TORCH_CHECK(max_group_nodes >= 0 && lds <= 163840,
              "forest_staged_loss: group too big for LDS");
  auto stream = at::hip::getCurrentHIPStream();
  const int blocks = (int)std::min<int64_t>(n_tiles, kStagedMaxBlocks);
#define FS_LAUNCH(DD, BB)                                                     \
  do {                                                                        \
    if (lds > 65536)                                                          \
      TORCH_CHECK(                                                            \
          hipFuncSetAttribute(                                                \
              reinterpret_cast<const void*>(&forest_staged_kernel<DD, BB>),   \
              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) ==        \
              hipSuccess,                                                     \
          "forest_staged_loss: cannot reserve ", lds, " bytes of LDS");       \
    hipLaunchKernelGGL((forest_staged_kernel<DD, BB>), dim3(blocks),          \
                       dim3(kStagedThreads), lds, stream,                     \
                       partials.data_ptr<double>(), x.data_ptr(),             \
                       (const unsigned long long*)nodes.data_ptr<int64_t>(),  \
                       tree_off.data_ptr<int>(), groups.data_ptr<int>(),      \
                       init.data_ptr<float>(), label.data_ptr<float>(),       \
                       weight.data_ptr<float>(), n, (int)F, (int)G, (int)S1,  \
                       (int)loss_id, (float)param, n_tiles);                  \
  } while (0)
#define FS_DIM(DD)                  \
  case DD:                          \
    if (binned) FS_LAUNCH(DD, true); \
    else FS_LAUNCH(DD, false);      \
    break;
  switch (dim) {
    FS_DIM(1) FS_DIM(2) FS_DIM(3) FS_DIM(4)
    FS_DIM(5) FS_DIM(6) FS_DIM(7) FS_DIM(8)
  }
#undef FS_DIM
#undef FS_LAUNCH
  // a refused launch must raise: out and partials are uninitialised memory
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "forest_staged_loss: kernel launch failed: ",
              hipGetErrorString(err));
  hipLaunchKernelGGL(forest_staged_reduce_kernel, dim3((unsigned)S1),
                     dim3(kReduceThreads), 0, stream, out.data_ptr<double>(),
                     partials.data_ptr<double>(), n_slots, (int)S1);
  err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "forest_staged_loss: reduce launch failed: ",
              hipGetErrorString(err));
}
