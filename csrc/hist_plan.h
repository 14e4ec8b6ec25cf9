// Host-side chunk policy of the per-level histogram kernels (hist_build in
// ops.hip, hist_build_class in wide_class.hip).  Plain C++: no torch types,
// no knowledge of either kernel.
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

struct HistPlan {
  int64_t chunk_rows = 0;
  int n_chunks = 0;
  int header_words = 0;
  // header_words reserved for the caller, then n_chunks records of
  // (node, start, len, slot, col0)
  std::vector<int> table;
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
  const int64_t target_chunks = std::max<int64_t>(
      1, (int64_t)(resident * oversub) / std::max(1, n_groups));

  HistPlan p;
  p.chunk_rows = std::max<int64_t>(
      4096, (total_rows + target_chunks - 1) / target_chunks);
  p.chunk_rows = std::min<int64_t>(p.chunk_rows, 1 << 20);
  p.header_words = header_words;
  p.table.assign(header_words, 0);
  for (int nd = 0; nd < n_nodes; ++nd) {
    const int64_t s = offs[nd], e = offs[nd + 1];
    int slot = -1;
    if (e - s > p.chunk_rows) {
      slot = (int)p.multi_nodes.size();
      p.multi_nodes.push_back(nd);
      p.slot_first.push_back((int)((p.table.size() - header_words) / 5));
      p.slot_count.push_back((int)((e - s + p.chunk_rows - 1) / p.chunk_rows));
    }
    int64_t c = s;
    do {
      const int rec[5] = {nd, (int)c,
                          (int)std::min<int64_t>(p.chunk_rows, e - c), slot,
                          col0 ? col0[nd] : 0};
      p.table.insert(p.table.end(), rec, rec + 5);
      c += p.chunk_rows;
    } while (c < e);
  }
  // at most n_nodes + 2^31 / 4096 records: fits int
  p.n_chunks = (int)((p.table.size() - header_words) / 5);
  return p;
}

// Fixed-point scale 2^30 / (chunk_rows * max_abs), clamped so a single
// value cannot overflow int32 either; a non-positive or non-finite max_abs
// counts as 1.
inline double hist_fixed_scale(int64_t chunk_rows, double max_abs) {
  if (!(max_abs > 0.0) || !std::isfinite(max_abs)) max_abs = 1.0;
  const double s = (double)(1u << 30) / ((double)chunk_rows * max_abs);
  return std::min(s, (double)(1u << 30) / max_abs);
}
