// forest_vote: vote sums of a K-class bagged forest, 9 <= K <= 32, in one
// pass over the rows, for gfx950.
//
//   sums[i, c] = sum over members t = 0 .. T-1 in order (MASKED: only t whose
//                in-bag bit of row i is CLEAR) of vote_t(x_i)[c]   f32 [N, K]
//   counts[i]  = number of members summed (MASKED only)            i32 [N]
//
// vote_t is the per-node leaf transform of a voting classifier: the one-hot
// of the leaf's argmax (hard), or its normalised probability row (soft).
// forest_predict2 and forest_oob stop at 8 outputs, so a 9-32 class
// ensemble used to be served by the v1 kernel: every node hop a dependent
// global load and every leaf a K-wide, mostly-zero row read from global
// memory.  Voting has structure a wider forest_predict2 would waste:
//
// Hard votes read no leaf tensor at all.  A leaf's payload IS its class id
// (the host takes the argmax of the one-hot row, so ties are resolved
// there).  A row's 32 counters are 16-bit fields of 8 u64 words (16 VGPRs);
// a vote adds  1 << ((c & 3) * 16)  to word  c >> 2  through a compare /
// select over the 8 words, written out, never a runtime index into the
// local array (that would become scratch).  Counts are exact integers; a
// field holds T <= 65535 votes, which the host checks.  At the end the
// fields are unpacked, converted to f32 and stored as K columns.
//
// Soft votes read a compact leaf table [n_leaves, KP] f32: one row per LEAF
// node, zero-padded to KP columns, so a row is 16-byte aligned and a lane
// fetches it with KP / 4 float4 loads.  A leaf's payload is its row index.
// acc[rows][KP] is statically indexed under fully unrolled loops over the
// compile-time KP in {12, 16, 24, 32}; runtime K <= KP.  Adds are in member
// order, one f32 add per class, so the result equals that of the v1 route
// and of the reference op bit for bit.
//
// Mapping.  That of forest_oob / forest_staged_loss: nodes are
// forest_predict2's u64 words (feature s16 | left child s16 | 32-bit
// payload), trees are cut into LDS groups.  A block owns a tile of
// kVoteThreads * R rows and walks the groups IN ORDER: stage group g's
// nodes into LDS, barrier, every lane walks the group's trees for its rows,
// one row after the other, each in a walk loop of its own (merged multi-row
// walk loops measured slower in three kernels of this tree).  Accumulators
// stay in registers from the first group to the last and are stored once:
// no atomics, no pre-zeroed output.
//
// Mask (MASKED).  forest_oob's: [W, N] i32 word-major in-bag bits, the
// GLOBAL tree index selects the bit, a lane reloads its words when that
// index enters another word (a group boundary may fall inside a word), and
// an in-bag or dead lane skips the walk.
//
// Rows per lane.  One block per CU beside a full node group: 16 waves per
// CU, 128 VGPRs per lane.  R per instantiation comes from the compiler's
// resource report for gfx950 (profiles/forest_vote.md); no instantiation
// uses scratch.  Hard: 16 counter VGPRs per row, R = 4.  Soft: KP
// accumulator VGPRs per row: R = 4 at KP = 12 and 16, 3 at 24, 2 at 32.
//
// Row access is forest_predict2's: f32 rows against f32 thresholds, or u8
// rank rows (bin_features against the pack's own threshold sets) against
// threshold ranks.  Either is exact; the caller picks by a static rule.

#include <ATen/hip/HIPContext.h>

#include <tuple>

#include "common.h"

namespace {

constexpr int kVoteThreads = 1024;
constexpr int kVoteMaxBlocks = 512;  // two rounds of one block per CU
constexpr int kVoteHardRows = 4;
constexpr int kVoteHardWords = 8;    // 32 classes x 16 bits
constexpr int vote_soft_rows(int kp) {
  return kp <= 16 ? 4 : (kp <= 24 ? 3 : 2);
}

// Walks one tree of the staged group for one row; returns the leaf's word.
template <bool BINNED>
__device__ __forceinline__ unsigned long long vote_walk(
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
  return nd;
}

// SOFT: KP accumulators per row, leaf rows from `table`.  !SOFT: KP is
// unused (32), 8 packed counter words per row, `table` is not read.
template <bool SOFT, int KP, int R, bool BINNED, bool MASKED>
__global__ __launch_bounds__(kVoteThreads) void forest_vote_kernel(
    float* __restrict__ sums,                      // [N, K]
    int* __restrict__ counts,                      // [N] (MASKED)
    const void* __restrict__ xv_,                  // [N, F] f32 | u8
    const unsigned long long* __restrict__ nodes,  // [total] packed
    const float* __restrict__ table,               // [n_leaves, KP] (SOFT)
    const int* __restrict__ tree_off,              // [T] global node base
    const int* __restrict__ groups,                // [G, 4]
    const int* __restrict__ mask,                  // [W, N] in-bag bits
    int64_t n, int F, int K, int G, int64_t n_tiles) {
  extern __shared__ __align__(16) unsigned long long tlds[];  // group nodes
  constexpr int kTile = kVoteThreads * R;
  constexpr int kAcc = SOFT ? KP : 1;
  constexpr int kWords = SOFT ? 1 : kVoteHardWords;
  const int xbytes = BINNED ? 1 : 4;

  // block-uniform trip count: every thread reaches every barrier
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kTile + threadIdx.x;
    float acc[R][kAcc];
    unsigned long long cw[R][kWords];
    int cnt[R];
    unsigned mw[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      cnt[r] = 0;
      mw[r] = 0u;
#pragma unroll
      for (int j = 0; j < kAcc; ++j) acc[r][j] = 0.0f;
#pragma unroll
      for (int j = 0; j < kWords; ++j) cw[r][j] = 0ull;
    }

    int word = -1;  // the mask word held in mw, block-uniform
    for (int g = 0; g < G; ++g) {
      const int* grp = groups + g * 4;
      const int first_tree = grp[0];
      const int n_trees = grp[1];
      const int node_base = grp[2];
      const int n_nodes = grp[3];
      __syncthreads();  // the previous group's walks are done
      for (int i = threadIdx.x; i < n_nodes; i += kVoteThreads)
        tlds[i] = nodes[node_base + i];
      __syncthreads();

      for (int t = 0; t < n_trees; ++t) {
        const int gt = first_tree + t;  // global tree index selects the bit
        if (MASKED && (gt >> 5) != word) {
          word = gt >> 5;
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int64_t row = row0 + (int64_t)r * kVoteThreads;
            mw[r] = row < n ? (unsigned)mask[(int64_t)word * n + row] : ~0u;
          }
        }
        const int bit = gt & 31;
        const int toff = tree_off[gt] - node_base;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t row = row0 + (int64_t)r * kVoteThreads;
          // per-lane branch: an in-bag (or dead) lane skips the walk
          if (row < n && !(MASKED && ((mw[r] >> bit) & 1u))) {
            const unsigned long long nd = vote_walk<BINNED>(
                tlds, toff, (const char*)xv_ + row * F * xbytes);
            const unsigned pay = (unsigned)(nd >> 32);
            if (SOFT) {
              const float4* lv = (const float4*)(table + (int64_t)pay * KP);
#pragma unroll
              for (int j = 0; j < KP / 4; ++j) {
                const float4 v = lv[j];
                acc[r][4 * j + 0] += v.x;
                acc[r][4 * j + 1] += v.y;
                acc[r][4 * j + 2] += v.z;
                acc[r][4 * j + 3] += v.w;
              }
            } else {
              // the class id picks a 16-bit field; selects, not an index
              const unsigned long long inc = 1ull << ((pay & 3u) * 16u);
              const unsigned w = pay >> 2;
#pragma unroll
              for (int j = 0; j < kWords; ++j)
                cw[r][j] += (w == (unsigned)j) ? inc : 0ull;
            }
            if (MASKED) ++cnt[r];
          }
        }
      }
    }

#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row0 + (int64_t)r * kVoteThreads;
      if (row < n) {
        if (MASKED) counts[row] = cnt[r];
        float* o = sums + row * K;
        if (SOFT) {
#pragma unroll
          for (int c = 0; c < KP; ++c)
            if (c < K) o[c] = acc[r][c];
        } else {
#pragma unroll
          for (int c = 0; c < 4 * kWords; ++c)
            if (c < K)
              o[c] = (float)(unsigned)((cw[r][c >> 2] >> ((c & 3) * 16)) &
                                       0xFFFFull);
        }
      }
    }
  }
}

inline int vote_kp(int64_t K) {
  return K <= 12 ? 12 : (K <= 16 ? 16 : (K <= 24 ? 24 : 32));
}

}  // namespace

// (threads, rows per lane: hard, soft KP = 12, 16, 24, 32, grid cap)
std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>
forest_vote_geometry() {
  return {kVoteThreads,       kVoteHardRows,      vote_soft_rows(12),
          vote_soft_rows(16), vote_soft_rows(24), vote_soft_rows(32),
          kVoteMaxBlocks};
}

// counts and mask are empty tensors for an unmasked call; table is empty
// for hard votes (n_leaves == 0).
void forest_vote(torch::Tensor sums, torch::Tensor counts, torch::Tensor x,
                 torch::Tensor nodes, torch::Tensor table,
                 torch::Tensor tree_off, torch::Tensor groups,
                 torch::Tensor mask, int64_t num_classes, bool soft,
                 bool masked, int64_t max_group_nodes) {
  CHECK_GPU(sums); CHECK_GPU(counts); CHECK_GPU(x); CHECK_GPU(nodes);
  CHECK_GPU(table); CHECK_GPU(tree_off); CHECK_GPU(groups); CHECK_GPU(mask);
  CHECK_CONTIG(sums); CHECK_CONTIG(counts); CHECK_CONTIG(x);
  CHECK_CONTIG(nodes); CHECK_CONTIG(table); CHECK_CONTIG(tree_off);
  CHECK_CONTIG(groups); CHECK_CONTIG(mask);
  const bool binned = x.scalar_type() == torch::kUInt8;
  TORCH_CHECK((binned || x.scalar_type() == torch::kFloat32) && x.dim() == 2,
              "forest_vote: x is [N, F] f32 or u8");
  const int64_t K = num_classes;
  TORCH_CHECK(K >= 9 && K <= 32, "forest_vote: 9 <= num_classes <= 32");
  const int kp = vote_kp(K);
  const int64_t n = x.size(0);
  const int64_t F = x.size(1);
  const int64_t G = groups.numel() / 4;
  const int64_t T = tree_off.numel();
  TORCH_CHECK(n >= 1 && F >= 1 && F < 32768, "forest_vote: x shape");
  TORCH_CHECK(sums.scalar_type() == torch::kFloat32 && sums.numel() == n * K,
              "forest_vote: sums is [N, num_classes] f32");
  TORCH_CHECK(nodes.scalar_type() == torch::kInt64 &&
                  tree_off.scalar_type() == torch::kInt32 &&
                  groups.scalar_type() == torch::kInt32 &&
                  groups.numel() == G * 4,
              "forest_vote: pack tensors");
  TORCH_CHECK(T >= 1 && G >= 1 && G <= T, "forest_vote: groups cover trees");
  TORCH_CHECK(T <= 65535, "forest_vote: at most 65535 members");
  TORCH_CHECK(table.scalar_type() == torch::kFloat32,
              "forest_vote: table is f32");
  if (soft)
    TORCH_CHECK(table.numel() >= kp && table.numel() % kp == 0 &&
                    table.numel() / kp <= nodes.numel() &&
                    (reinterpret_cast<uintptr_t>(table.data_ptr()) & 15) == 0,
                "forest_vote: table is [n_leaves, ", kp,
                "] f32, 16-byte aligned");
  if (masked) {
    const int64_t W = ceil_div(T, (int64_t)32);
    TORCH_CHECK(mask.scalar_type() == torch::kInt32 && mask.numel() == W * n,
                "forest_vote: mask is [ceil(T / 32), N] i32");
    TORCH_CHECK(counts.scalar_type() == torch::kInt32 && counts.numel() == n,
                "forest_vote: counts is [N] i32");
  }
  const size_t lds = (size_t)max_group_nodes * 8;
  TORCH_CHECK(max_group_nodes >= 1 && max_group_nodes <= nodes.numel() &&
                  lds <= 163840,
              "forest_vote: group too big for LDS");
  auto stream = at::hip::getCurrentHIPStream();
  const int* mask_p = masked ? mask.data_ptr<int>() : nullptr;
  int* counts_p = masked ? counts.data_ptr<int>() : nullptr;
#define FV_LAUNCH(SS, KK, RR, BB, MM)                                         \
  do {                                                                        \
    const int64_t n_tiles = ceil_div(n, (int64_t)kVoteThreads * (RR));        \
    const int blocks = (int)std::min<int64_t>(n_tiles, kVoteMaxBlocks);       \
    if (lds > 65536)                                                          \
      TORCH_CHECK(                                                            \
          hipFuncSetAttribute(                                                \
              reinterpret_cast<const void*>(                                  \
                  &forest_vote_kernel<SS, KK, RR, BB, MM>),                   \
              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) ==        \
              hipSuccess,                                                     \
          "forest_vote: cannot reserve ", lds, " bytes of LDS");              \
    hipLaunchKernelGGL((forest_vote_kernel<SS, KK, RR, BB, MM>),              \
                       dim3(blocks), dim3(kVoteThreads), lds, stream,         \
                       sums.data_ptr<float>(), counts_p, x.data_ptr(),        \
                       (const unsigned long long*)nodes.data_ptr<int64_t>(),  \
                       table.data_ptr<float>(), tree_off.data_ptr<int>(),     \
                       groups.data_ptr<int>(), mask_p, n, (int)F, (int)K,     \
                       (int)G, n_tiles);                                      \
  } while (0)
#define FV_FLAGS(SS, KK, RR)                               \
  do {                                                     \
    if (binned && masked) FV_LAUNCH(SS, KK, RR, true, true);       \
    else if (binned) FV_LAUNCH(SS, KK, RR, true, false);           \
    else if (masked) FV_LAUNCH(SS, KK, RR, false, true);           \
    else FV_LAUNCH(SS, KK, RR, false, false);                      \
  } while (0)
  if (!soft) {
    FV_FLAGS(false, 32, kVoteHardRows);
  } else {
    switch (kp) {
      case 12: FV_FLAGS(true, 12, vote_soft_rows(12)); break;
      case 16: FV_FLAGS(true, 16, vote_soft_rows(16)); break;
      case 24: FV_FLAGS(true, 24, vote_soft_rows(24)); break;
      default: FV_FLAGS(true, 32, vote_soft_rows(32)); break;
    }
  }
#undef FV_FLAGS
#undef FV_LAUNCH
  // a refused launch must raise: sums and counts are uninitialised memory
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "forest_vote: kernel launch failed: ",
              hipGetErrorString(err));
}
