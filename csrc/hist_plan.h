// Chunk policy of the per-level histogram kernels (hist_build in ops.hip,
// hist_build_class in wide_class.hip).  Plain C++: no torch types, no
// knowledge of either kernel.  The rules themselves (chunk size, records and
// staging slot of a node, fixed-point scale) are HIST_PLAN_HD functions: the
// host planner below walks the nodes with them, and level_plan_kernel in
// ops.hip applies the same functions on the device.
//
// A level is cut into chunks of at most chunk_rows rows; one block per
// (chunk, feature group) accumulates its chunk in LDS.  chunk_rows targets a
// grid of ~resident-blocks x oversubscription (SEA_HIST_OVERSUB overrides),
// floored at 4096 rows and capped at 2^20 so a chunk's fixed-point sums and
// row counts keep their 2^30 headroom.  A node that fits one chunk flushes
// with plain stores (slot -1); a multi-chunk node gets a staging slot that a
// second pass sums over the node's chunks and converts.  The records of a
// node are consecutive, so a slot is named by its first record and record
// count.  Every node gets at least one record, so a zero-row node's block
// writes its zeros itself.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <vector>

#ifdef __HIPCC__
#define HIST_PLAN_HD __host__ __device__
#else
#define HIST_PLAN_HD
#endif

// Chunks a level is cut into when its nodes are large: ~resident blocks x
// oversubscription, shared among the feature groups.  Host only: it reads
// SEA_HIST_OVERSUB; the device planner is handed the number.
inline int64_t hist_target_chunks(size_t lds_bytes, int n_groups) {
  const int blocks_per_cu =
      std::max<int>(1, (int)(163840 / std::max<size_t>(1, lds_bytes)));
  const int64_t resident = (int64_t)256 * blocks_per_cu;
  // exactly-resident grids measured fastest at 1 block/CU
  // (profiles/r01_hist_probe3); modest oversubscription amortizes
  // imbalance otherwise
  static const double oversub_env = []() {
    const char* e = getenv("SEA_HIST_OVERSUB");
    return e ? atof(e) : 0.0;
  }();
  const double oversub =
      oversub_env > 0 ? oversub_env : (blocks_per_cu == 1 ? 1.0 : 1.5);
  return std::max<int64_t>(
      1, (int64_t)(resident * oversub) / std::max(1, n_groups));
}

HIST_PLAN_HD inline int64_t hist_chunk_rows(int64_t total_rows,
                                            int64_t target_chunks) {
  int64_t r = (total_rows + target_chunks - 1) / target_chunks;
  if (r < 4096) r = 4096;
  if (r > (1 << 20)) r = 1 << 20;
  return r;
}

// every node gets at least one record
HIST_PLAN_HD inline int hist_node_records(int64_t len, int64_t chunk_rows) {
  return len > chunk_rows ? (int)((len + chunk_rows - 1) / chunk_rows) : 1;
}

HIST_PLAN_HD inline bool hist_node_is_multi(int64_t len, int64_t chunk_rows) {
  return len > chunk_rows;
}

// Records of the level, whatever the node sizes turn out to be: with R >= the
// level's rows, sum_i max(1, ceil(len_i / chunk_rows)) <= total / chunk_rows
// + n_nodes, and total / chunk_rows <= target_chunks unless chunk_rows hit
// its 2^20 cap, where it is <= ceil(R / 2^20) (the 4096 floor only makes
// chunk_rows larger).
HIST_PLAN_HD inline int64_t hist_chunk_bound(int64_t R, int64_t target_chunks,
                                             int64_t n_nodes) {
  const int64_t capped = (R + (1 << 20) - 1) >> 20;
  return (target_chunks > capped ? target_chunks : capped) + n_nodes;
}

// Writes the records (node, start, len, slot, col0) of node nd, rows [start,
// start + len), at ``rec``, and for a multi-chunk node its staging slot
// record (node, first record, record count, first slab) at ``slot_rec``.
// ``slot`` is -1 for a single-chunk node.
HIST_PLAN_HD inline void hist_emit_node(int* rec, int* slot_rec, int nd,
                                        int64_t start, int64_t len, int col0,
                                        int64_t chunk_rows, int first_rec,
                                        int slot, int first_slab) {
  const int n = hist_node_records(len, chunk_rows);
  for (int k = 0; k < n; ++k) {
    const int64_t done = (int64_t)k * chunk_rows;
    const int64_t left = len - done;
    rec[5 * k + 0] = nd;
    rec[5 * k + 1] = (int)(start + done);
    rec[5 * k + 2] = (int)(left < chunk_rows ? left : chunk_rows);
    rec[5 * k + 3] = slot;
    rec[5 * k + 4] = col0;
  }
  if (slot >= 0) {
    slot_rec[0] = nd;
    slot_rec[1] = first_rec;
    slot_rec[2] = n;
    slot_rec[3] = first_slab;
  }
}

// Fixed-point scale 2^30 / (chunk_rows * max_abs), clamped so a single
// value cannot overflow int32 either; a non-positive or non-finite max_abs
// counts as 1.
HIST_PLAN_HD inline double hist_fixed_scale(int64_t chunk_rows,
                                            double max_abs) {
  if (!(max_abs > 0.0) || !(max_abs <= std::numeric_limits<double>::max()))
    max_abs = 1.0;
  const double s = (double)(1u << 30) / ((double)chunk_rows * max_abs);
  const double one = (double)(1u << 30) / max_abs;
  return s < one ? s : one;
}

struct HistPlan {
  int64_t chunk_rows = 0;
  int n_chunks = 0;
  int header_words = 0;
  // header_words reserved for the caller, then n_chunks records of
  // (node, start, len, slot, col0)
  std::vector<int> table;
  std::vector<int> slots;        // (node, first record, count, first slab)
  std::vector<int> multi_nodes;  // node id of each staging slot
  std::vector<int> slot_first;   // first chunk record of each staging slot
  std::vector<int> slot_count;   // its number of (consecutive) records
};

inline HistPlan plan_hist_chunks(const int64_t* offs, int n_nodes,
                                 const int* col0 /* null -> 0 */,
                                 int64_t row_bound, int col_bound,
                                 size_t lds_bytes, int n_groups,
                                 int header_words) {
  int64_t total_rows = 0;
  for (int nd = 0; nd < n_nodes; ++nd) {
    const int64_t s = offs[nd], e = offs[nd + 1];
    if (s < 0 || e < s || e > row_bound ||
        e > std::numeric_limits<int>::max())
      throw std::invalid_argument("hist plan: node_offsets out of range");
    const int c0 = col0 ? col0[nd] : 0;
    if (c0 < 0 || c0 >= col_bound)
      throw std::invalid_argument("hist plan: node_col0 out of range");
    total_rows += e - s;
  }

  HistPlan p;
  p.chunk_rows =
      hist_chunk_rows(total_rows, hist_target_chunks(lds_bytes, n_groups));
  p.header_words = header_words;
  p.table.assign(header_words, 0);
  int n_slabs = 0;
  for (int nd = 0; nd < n_nodes; ++nd) {
    const int64_t s = offs[nd], len = offs[nd + 1] - s;
    const bool multi = hist_node_is_multi(len, p.chunk_rows);
    const int n = hist_node_records(len, p.chunk_rows);
    const int slot = multi ? (int)p.multi_nodes.size() : -1;
    const size_t at = p.table.size();
    p.table.resize(at + 5 * (size_t)n);
    if (multi) p.slots.resize(p.slots.size() + 4);
    hist_emit_node(p.table.data() + at,
                   multi ? p.slots.data() + 4 * slot : nullptr, nd, s, len,
                   col0 ? col0[nd] : 0, p.chunk_rows, p.n_chunks, slot,
                   n_slabs);
    if (multi) {
      p.multi_nodes.push_back(nd);
      p.slot_first.push_back(p.n_chunks);
      p.slot_count.push_back(n);
      n_slabs += n;
    }
    // at most n_nodes + 2^31 / 4096 records: fits int
    p.n_chunks += n;
  }
  return p;
}
