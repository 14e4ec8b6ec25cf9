// Shared by every csrc/*.hip: argument
// checks, the pinned upload helper with its slot table, the sortable-float
// encoding of the split scans, and the entry points that cross files.
#pragma once

#include <torch/extension.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <tuple>

#define CHECK_GPU(x) TORCH_CHECK(x.is_cuda(), #x " must be on GPU")
#define CHECK_CONTIG(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// order-preserving f32 <-> u32 (packed atomicMax split search)
__device__ inline unsigned f32_sortable(float f) {
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float sortable_f32(unsigned s) {
  unsigned u = (s & 0x80000000u) ? (s & 0x7FFFFFFFu) : ~s;
  return __uint_as_float(u);
}

// Pinned ping-pong staging slots of h2d_async, one name per call site.
// gather_ranges and leaf_scatter share a slot; every other site owns its.
enum UploadSlot : int {
  kSlotHistChunks = 0,      // hist_build: scales + chunk table
  kSlotHistNodes = 1,       // hist_build: staging slot -> node
  kSlotPartCursors = 2,     // partition_rows: per-node cursors
  kSlotPartChunks = 3,      // partition_rows: chunk table
  kSlotPartSegStart = 4,    // partition_rows: segment starts
  kSlotGatherSegs = 5,      // gather_ranges: prefix + starts
  kSlotLeafSegs = kSlotGatherSegs,  // leaf_scatter: prefix + starts
  kSlotLeafTree = 6,        // leaf_scatter: tree ids
  kSlotLeafVal = 7,         // leaf_scatter: leaf values
  kSlotClassChunks = 8,     // hist_build_class: scale + chunk table
  kSlotClassNodes = 9,      // hist_build_class: slot -> node + scales
  kSlotLevelTable = 10,     // level_split: per-node source rows
  kUploadSlots = 12,
};

// csrc/ops.hip: async H2D of a small host table through pinned staging
torch::Tensor h2d_async(const void* src, size_t bytes, UploadSlot slot,
                        const torch::Device& dev);

// csrc/ops.hip: decode the i64 staging sums of multi-chunk nodes into f32,
// out[nodes[slot]] = stage[slot] / scales[channel]; nodes and scales are
// device pointers
void launch_hist_decode(float* out, const long long* stage, const int* nodes,
                        const float* scales, int n_multi, int64_t FBC, int C,
                        hipStream_t stream);

// csrc/wide_class.hip
void split_argmax_wide(torch::Tensor gain, torch::Tensor feat,
                       torch::Tensor bin, torch::Tensor left_stats,
                       torch::Tensor hist, int D, double lam,
                       double min_child_weight, double min_instances,
                       double min_info_gain);
int64_t hist_build_class(torch::Tensor out, torch::Tensor bins,
                         torch::Tensor bins_t, torch::Tensor label,
                         torch::Tensor weight, torch::Tensor row_idx,
                         torch::Tensor node_offsets, torch::Tensor node_col0,
                         int64_t num_bins, int64_t num_classes, int64_t nn,
                         double w_max, bool identity_rows);

// csrc/tree_contrib.hip
void forest_contrib(torch::Tensor out, torch::Tensor x, torch::Tensor ranges,
                    torch::Tensor path_off, torch::Tensor path_m,
                    torch::Tensor path_v, torch::Tensor e_feat,
                    torch::Tensor e_lo, torch::Tensor e_hi, torch::Tensor e_z,
                    int64_t rows_per_tile, double scale);

// csrc/forest_staged.hip
void forest_staged_loss(torch::Tensor out, torch::Tensor partials,
                        torch::Tensor x, torch::Tensor nodes,
                        torch::Tensor tree_off, torch::Tensor groups,
                        torch::Tensor init, torch::Tensor label,
                        torch::Tensor weight, int64_t dim,
                        int64_t max_group_nodes, int64_t loss_id,
                        double param);
std::tuple<int64_t, int64_t, int64_t> forest_staged_geometry();

// csrc/forest_oob.hip
void forest_oob(torch::Tensor sums, torch::Tensor counts, torch::Tensor x,
                torch::Tensor nodes, torch::Tensor leaves,
                torch::Tensor tree_off, torch::Tensor groups,
                torch::Tensor mask, int64_t dim, int64_t max_group_nodes);
std::tuple<int64_t, int64_t, int64_t> forest_oob_geometry();

// csrc/forest_permute.hip
void forest_permute_loss(torch::Tensor out, torch::Tensor partials,
                         torch::Tensor x, torch::Tensor nodes,
                         torch::Tensor tree_off, torch::Tensor groups,
                         torch::Tensor init, torch::Tensor label,
                         torch::Tensor weight, torch::Tensor donor,
                         int64_t max_group_nodes, int64_t loss_id,
                         double param);
std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>
forest_permute_geometry();

// csrc/linear.hip
void logreg_loss_grad(torch::Tensor payload, torch::Tensor x, torch::Tensor y,
                      torch::Tensor w, torch::Tensor wmat, bool has_bias);
bool logreg_fused_supported(int64_t F, int64_t K);
