// forest_permute_loss: the loss of a forest with ONE feature column shuffled,
// for every feature and every repeat, in one launch, for gfx950.
//
//   base      = sum_i w_i * loss(label_i, init_i + sum_t w_t leaf_t(x_i))
//   perm[r,f] = sum_i w_i * loss(label_i, init_i + sum_t w_t leaf_t(x^(r,f)_i))
//
// x^(r,f) is x with column f of every row i replaced by x[donor[r, i], f].
// The column-swap loop this replaces runs F * R full forest passes.  For one
// (row, tree) pair the swap of f can change the leaf only if f is on the
// row's own root-to-leaf path, so one walk of that path plus a short sub-walk
// per disagreeing path feature gives the permuted leaf of every feature:
// about depth^2 node visits instead of F * depth.
//
// Mapping.  The forest arrives as forest_predict2 packs it, one u64 per node
// (feature s16 | left child s16 | threshold or weighted leaf f32), regrouped
// under this op's own node budget (below).  A block owns (row tile, feature
// chunk, repeat): kPermThreads rows, ONE row per lane for all trees in tree
// order, the kPermFC features f0 .. f0 + FC - 1, the donors of repeat r.  It
// walks the groups IN ORDER as forest_staged_loss and forest_oob do: stage
// group g's nodes into LDS, barrier, every lane walks the group's trees for
// its row, next group.  Per (row, tree):
//   1. base walk to the leaf v0; m0 += v0 in a register (the D == 1 pack
//      folds the tree weight into the payload: no multiply here);
//   2. divergence walk of the same path: at a node that splits on a feature
//      f of the block's chunk, gather the donor's value of f and compare
//      directions;
//   3. at the FIRST node of the path where the donor's value of f goes the
//      other way, sub-walk from the other child to a leaf v': f takes the
//      donor's value at every later node that splits on f, every other
//      feature keeps the row's own value; acc[f] += v' - v0.
// A chunk repeats the base walk but gathers donors for its own features only.
//
// First disagreement.  A path may split on f several times; once the donor
// has disagreed at one of those nodes the permuted path has left the base
// path, and later base-path nodes that split on f must not start a second
// sub-walk.  The obvious ways to know are a register list of the diverged
// features (with a depth cap) or a re-scan of the path prefix.  Neither is
// needed: a chunk has at most 64 features, so the set of features already
// diverged on this path is ONE u64 bit mask per lane (bit f - f0), cleared per
// tree, tested and set with a shift.  Two VGPRs, no dynamic register
// indexing, no scratch, no depth cap (forest_permute_geometry reports
// max_depth = 0), and O(1) per node where the re-scan is O(depth) dependent
// LDS reads.  An earlier node on f where the donor AGREES sets no bit, so a
// later disagreement on f is still the first.
//
// LDS split.  Accumulators acc[FC][kPermThreads] f32, feature-major, one
// column per lane: lane l always touches bank l % 64 (l % 32 within its half
// for the b32 forms), whatever mix of features the wave's lanes hit, and a
// lane is the only writer of its column: no atomics, no barrier around acc.
// FC * kPermThreads * 4 = 64 KiB; the other 96 KiB of the CU's 160 KiB hold
// the group's nodes (kPermGroupNodes = 12288), so the forest is regrouped
// under that budget (dispatch._permute_groups) from the same node64 / node64b
// arena the other ops read.  Threads and FC at 64 KiB of accumulators come
// from one sweep (profiles/permute.md): 256 x 64 beat 512 x 32 and 1024 x 16
// at F = 256 (every chunk repeats the base and divergence walks, and that
// repeated work outweighs the latency more waves would hide); 512 x 32 was
// ahead only on the 16-column frame, one chunk either way.  53 VGPRs, no
// scratch.
//
// Loss and reduction.  After the last group a lane forms init + (m0 + acc[f])
// for every f of the chunk and evaluates w * loss in f32 through the device
// forms of csrc/gbm_loss.h, unclamped: a NaN or an inf reaches the
// result.  f64 wave shuffle reduce, lane 0 adds the wave's sum into
// partials[block.x * waves + wave][r * F + f], a cell only that wave touches
// (the first tile of the block stores, later tiles of a wrapped grid add, in
// tile order).  base comes from m0 alone in the blocks of chunk 0, repeat 0,
// in column R * F.  forest_permute_reduce_kernel sums the slots of a column
// in a fixed order.  The grid is a function of the shapes alone, so the
// result is bitwise reproducible run to run.
//
// Rounding.  The kernel forms m0 + sum(v' - v0), not the direct sum of the
// permuted leaves.  With integer leaves (and weights that keep every partial
// sum exact) the two are identical; in general they differ by a rounding of
// the order of T ulp of the margin.
//
// Row access is forest_predict2's: f32 rows against f32 thresholds, or u8
// rank rows (bin_features against the pack's own threshold sets) against
// threshold ranks.  Donor values are gathered from the same row matrix, so a
// donor's NaN goes right and its +-inf compares as a float in either form.

#include <ATen/hip/HIPContext.h>

#include <tuple>

#include "common.h"
#include "gbm_loss.h"

namespace {

constexpr int kPermThreads = 256;  // one row per lane
constexpr int kPermWaves = kPermThreads / 64;
constexpr int kPermFC = 64;  // features per chunk
constexpr int kPermAccBytes = kPermFC * kPermThreads * 4;
constexpr int kPermLdsBytes = 163840;
constexpr int kPermGroupNodes = (kPermLdsBytes - kPermAccBytes) / 8;
constexpr int kPermMaxBlocks = 512;  // row-tile blocks; tiles beyond wrap
constexpr int kPermReduceThreads = 256;

static_assert(kPermThreads % 64 == 0 && kPermThreads <= 1024, "whole waves");
static_assert(kPermFC >= 1 && kPermFC <= 64, "the diverged set is one u64");
static_assert(kPermAccBytes % 16 == 0 && kPermGroupNodes >= 1024,
              "accumulators leave room for a group of nodes");

template <bool BINNED>
__global__ __launch_bounds__(kPermThreads) void forest_permute_kernel(
    double* __restrict__ partials,                 // [slots, R * F + 1]
    const void* __restrict__ xv_,                  // [N, F] f32 | u8
    const unsigned long long* __restrict__ nodes,  // [total] packed
    const int* __restrict__ tree_off,              // [T] global node base
    const int* __restrict__ groups,                // [G, 4]
    const float* __restrict__ init,                // [N]
    const float* __restrict__ label,               // [N]
    const float* __restrict__ weight,              // [N]
    const int* __restrict__ donor,                 // [R, N]
    int64_t n, int F, int G, int64_t C, int loss_id, float param,
    int64_t n_tiles) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* __restrict__ acc = reinterpret_cast<float*>(smem);  // [FC][threads]
  unsigned long long* __restrict__ tlds =
      reinterpret_cast<unsigned long long*>(smem + kPermAccBytes);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int f0 = blockIdx.y * kPermFC;
  const int fc = min(kPermFC, F - f0);  // features of this chunk, >= 1
  const int rep = blockIdx.z;
  const bool emit_base = blockIdx.y == 0 && blockIdx.z == 0;
  const int* __restrict__ dn = donor + (int64_t)rep * n;
  double* __restrict__ prow =
      partials + ((int64_t)blockIdx.x * kPermWaves + wave) * C;
  float* __restrict__ my = acc + threadIdx.x;  // this lane's column

  // block-uniform trip count: every thread reaches every barrier
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row = tile * kPermThreads + threadIdx.x;
    const bool live = row < n;
    const int64_t drow = live ? (int64_t)dn[row] : 0;
    const float* xr = BINNED ? nullptr : (const float*)xv_ + row * F;
    const float* xd = BINNED ? nullptr : (const float*)xv_ + drow * F;
    const uint8_t* br = BINNED ? (const uint8_t*)xv_ + row * F : nullptr;
    const uint8_t* bd = BINNED ? (const uint8_t*)xv_ + drow * F : nullptr;
    for (int j = 0; j < fc; ++j) my[j * kPermThreads] = 0.0f;
    float m0 = 0.0f;

    for (int g = 0; g < G; ++g) {
      const int* grp = groups + g * 4;
      const int first_tree = grp[0];
      const int n_trees = grp[1];
      const int node_base = grp[2];
      const int n_nodes = grp[3];
      __syncthreads();  // the previous group's walks are done
      for (int i = threadIdx.x; i < n_nodes; i += kPermThreads)
        tlds[i] = nodes[node_base + i];
      __syncthreads();

      for (int t = 0; t < n_trees; ++t) {
        const int toff = tree_off[first_tree + t] - node_base;
        if (live) {
          // 1. base walk
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
          const float v0 = __uint_as_float((unsigned)(nd >> 32));
          m0 += v0;

          // 2. divergence walk of the same path
          unsigned long long diverged = 0ull;  // bit f - f0: f has left
          nd = tlds[toff];
          f = (short)(nd & 0xFFFFu);
          while (f >= 0) {
            const int left = (short)((nd >> 16) & 0xFFFFu);
            const unsigned pay = (unsigned)(nd >> 32);
            bool go_left;
            if (BINNED)
              go_left = br[f] <= pay;
            else
              go_left = xr[f] <= __uint_as_float(pay);
            const unsigned j = (unsigned)(f - f0);
            if (j < (unsigned)fc && !((diverged >> j) & 1ull)) {
              // the donor's value of f, as the row matrix holds it
              unsigned dbin = 0u;
              float dval = 0.0f;
              bool d_left;
              if (BINNED) {
                dbin = bd[f];
                d_left = dbin <= pay;
              } else {
                dval = xd[f];
                d_left = dval <= __uint_as_float(pay);
              }
              if (d_left != go_left) {
                // 3. first disagreement on f: sub-walk from the other child
                diverged |= 1ull << j;
                unsigned long long n2 = tlds[toff + left + (d_left ? 0 : 1)];
                int f2 = (short)(n2 & 0xFFFFu);
                while (f2 >= 0) {
                  const int l2 = (short)((n2 >> 16) & 0xFFFFu);
                  const unsigned p2 = (unsigned)(n2 >> 32);
                  bool gl;
                  if (BINNED)
                    gl = (f2 == f ? dbin : (unsigned)br[f2]) <= p2;
                  else
                    gl = (f2 == f ? dval : xr[f2]) <= __uint_as_float(p2);
                  n2 = tlds[toff + l2 + (gl ? 0 : 1)];
                  f2 = (short)(n2 & 0xFFFFu);
                }
                my[j * kPermThreads] +=
                    __uint_as_float((unsigned)(n2 >> 32)) - v0;
              }
            }
            nd = tlds[toff + left + (go_left ? 0 : 1)];
            f = (short)(nd & 0xFFFFu);
          }
        }
      }
    }

    // every column of the chunk, then base: wave-uniform control flow, so
    // every lane runs the shuffles
    const float wt = live ? weight[row] : 0.0f;
    const float lab = live ? label[row] : 0.0f;
    const float ini = live ? init[row] : 0.0f;
    const bool first = tile == (int64_t)blockIdx.x;
    auto emit = [&](float margin, int64_t col) {
      float gr, he;
      // dim 1: logloss is the one-class cross-entropy, as forest_staged_loss
      const float l =
          wt * (loss_id == L_LOGLOSS
                    ? softmax_xent<1>(&lab, &margin)
                    : scalar_loss_grad(loss_id, param, lab, margin, &gr, &he));
      double s = live ? (double)l : 0.0;
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
      if (lane == 0) prow[col] = first ? s : prow[col] + s;
    };
    // init + (forest sum): the reference op's order, so exact forest sums
    // give bitwise its margins
    for (int j = 0; j < fc; ++j)
      emit(ini + (m0 + my[j * kPermThreads]), (int64_t)rep * F + f0 + j);
    if (emit_base) emit(ini + m0, C - 1);
  }
}

// out[c] = sum over slots of partials[slot][c]: thread j sums slots j,
// j + 256, ... in order, then the 256 thread sums are added in order
// (forest_staged_reduce_kernel's scheme).
__global__ __launch_bounds__(kPermReduceThreads) void
forest_permute_reduce_kernel(double* __restrict__ out,
                             const double* __restrict__ partials,
                             int64_t n_slots, int64_t C) {
  __shared__ double lp[kPermReduceThreads];
  const int64_t c = blockIdx.x;
  double v = 0.0;
  for (int64_t k = threadIdx.x; k < n_slots; k += kPermReduceThreads)
    v += partials[k * C + c];
  lp[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int j = 0; j < kPermReduceThreads; ++j) t += lp[j];
    out[c] = t;
  }
}

}  // namespace

// (threads, rows per lane, row-tile grid cap, features per chunk, nodes per
// LDS group, depth cap: 0 = none)
std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>
forest_permute_geometry() {
  return {kPermThreads, 1, kPermMaxBlocks, kPermFC, kPermGroupNodes, 0};
}

void forest_permute_loss(torch::Tensor out, torch::Tensor partials,
                         torch::Tensor x, torch::Tensor nodes,
                         torch::Tensor tree_off, torch::Tensor groups,
                         torch::Tensor init, torch::Tensor label,
                         torch::Tensor weight, torch::Tensor donor,
                         int64_t max_group_nodes, int64_t loss_id,
                         double param) {
  CHECK_GPU(out); CHECK_GPU(partials); CHECK_GPU(x); CHECK_GPU(nodes);
  CHECK_GPU(tree_off); CHECK_GPU(groups); CHECK_GPU(init); CHECK_GPU(label);
  CHECK_GPU(weight); CHECK_GPU(donor);
  CHECK_CONTIG(out); CHECK_CONTIG(partials); CHECK_CONTIG(x);
  CHECK_CONTIG(nodes); CHECK_CONTIG(tree_off); CHECK_CONTIG(groups);
  CHECK_CONTIG(init); CHECK_CONTIG(label); CHECK_CONTIG(weight);
  CHECK_CONTIG(donor);
  const bool binned = x.scalar_type() == torch::kUInt8;
  TORCH_CHECK((binned || x.scalar_type() == torch::kFloat32) && x.dim() == 2,
              "forest_permute_loss: x is [N, F] f32 or u8");
  TORCH_CHECK(loss_id >= L_SQUARED && loss_id <= L_BERNOULLI,
              "forest_permute_loss: unknown loss id");
  const int64_t n = x.size(0);
  const int64_t F = x.size(1);
  const int64_t G = groups.numel() / 4;
  const int64_t T = tree_off.numel();
  TORCH_CHECK(n >= 1 && n <= 0x7FFFFFFF && F >= 1 && F < 32768,
              "forest_permute_loss: x shape");
  TORCH_CHECK(donor.scalar_type() == torch::kInt32 && donor.dim() == 2 &&
                  donor.size(1) == n && donor.size(0) >= 1 &&
                  donor.size(0) <= 65535,
              "forest_permute_loss: donor is [R, N] i32, 1 <= R <= 65535");
  const int64_t R = donor.size(0);
  const int64_t C = R * F + 1;
  // one reduce block per column: gridDim.x holds up to 2^31 - 1
  TORCH_CHECK(C <= 0x7FFFFFFF, "forest_permute_loss: R * F too large");
  TORCH_CHECK(out.scalar_type() == torch::kFloat64 && out.numel() == C,
              "forest_permute_loss: out is [R * F + 1] f64");
  TORCH_CHECK(nodes.scalar_type() == torch::kInt64 &&
                  tree_off.scalar_type() == torch::kInt32 &&
                  groups.scalar_type() == torch::kInt32 &&
                  groups.numel() == G * 4,
              "forest_permute_loss: pack tensors");
  TORCH_CHECK(T >= 1 && G >= 1 && G <= T,
              "forest_permute_loss: groups cover trees");
  TORCH_CHECK(init.scalar_type() == torch::kFloat32 &&
                  label.scalar_type() == torch::kFloat32 &&
                  weight.scalar_type() == torch::kFloat32,
              "forest_permute_loss: init, label and weight are f32");
  TORCH_CHECK(init.numel() == n && label.numel() == n && weight.numel() == n,
              "forest_permute_loss: init / label / weight do not match x");
  TORCH_CHECK(max_group_nodes >= 1 && max_group_nodes <= nodes.numel() &&
                  max_group_nodes <= kPermGroupNodes,
              "forest_permute_loss: group too big for LDS");
  const int64_t n_tiles = ceil_div(n, (int64_t)kPermThreads);
  const int blocks = (int)std::min<int64_t>(n_tiles, kPermMaxBlocks);
  const int64_t n_slots = (int64_t)blocks * kPermWaves;
  TORCH_CHECK(partials.scalar_type() == torch::kFloat64 &&
                  partials.numel() == n_slots * C,
              "forest_permute_loss: partials is [blocks * waves, R * F + 1]");
  const int64_t chunks = ceil_div(F, (int64_t)kPermFC);
  const size_t lds = (size_t)kPermAccBytes + (size_t)max_group_nodes * 8;
  auto stream = at::hip::getCurrentHIPStream();
#define FP_LAUNCH(BB)                                                         \
  do {                                                                        \
    if (lds > 65536)                                                          \
      TORCH_CHECK(                                                            \
          hipFuncSetAttribute(                                                \
              reinterpret_cast<const void*>(&forest_permute_kernel<BB>),      \
              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) ==        \
              hipSuccess,                                                     \
          "forest_permute_loss: cannot reserve ", lds, " bytes of LDS");      \
    hipLaunchKernelGGL((forest_permute_kernel<BB>),                           \
                       dim3(blocks, (unsigned)chunks, (unsigned)R),           \
                       dim3(kPermThreads), lds, stream,                       \
                       partials.data_ptr<double>(), x.data_ptr(),             \
                       (const unsigned long long*)nodes.data_ptr<int64_t>(),  \
                       tree_off.data_ptr<int>(), groups.data_ptr<int>(),      \
                       init.data_ptr<float>(), label.data_ptr<float>(),       \
                       weight.data_ptr<float>(), donor.data_ptr<int>(), n,    \
                       (int)F, (int)G, C, (int)loss_id, (float)param,         \
                       n_tiles);                                              \
  } while (0)
  if (binned) FP_LAUNCH(true);
  else FP_LAUNCH(false);
#undef FP_LAUNCH
  // a refused launch must raise: out and partials are uninitialised memory
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "forest_permute_loss: kernel launch failed: ",
              hipGetErrorString(err));
  hipLaunchKernelGGL(forest_permute_reduce_kernel, dim3((unsigned)C),
                     dim3(kPermReduceThreads), 0, stream,
                     out.data_ptr<double>(), partials.data_ptr<double>(),
                     n_slots, C);
  err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "forest_permute_loss: reduce launch failed: ",
              hipGetErrorString(err));
}
