// Wide-multiclass gini kernels for gfx950 (CDNA4 / MI355X).
//
//   * hist_build_class  — label-indexed histograms for K-class gini trees
//                         (7 <= K <= 32 is the intended range, 2..32 works)
//   * split_argmax_wide — the split_argmax gain scan for 9 <= C <= 34
//                         channels (K one-hot channels + hess (+ count))
//
// hist_build_class.  A row of a gini tree belongs to exactly ONE class, so
// the generic [N, C] gradient-matrix kernel (ops.hip hist_build_kernel)
// spends up to 7 ds_add_u64 per (row, feature) of which all but one add
// zero, and needs ceil(K / 6) launches over the whole binned matrix.  Here
// the LDS histogram is [FG][B][K] u64 cells and a row issues ONE
// ds_add_u64 per feature, to cell [f][bin][label]:
//     high 32 bits = fixed-point weight sum, low 32 bits = row count.
// The hess channel (sum over classes) and the count channel are derived in
// the flush by integer sums over the K cells of a bin — no LDS cells or
// adds are spent on them.  Output layout is the grower's
// [n_nodes, F, B, K + NN]: classes, hess, (count when NN == 2).
//
// The quantisation scale is ONE power of two,
//     2^floor(log2(2^30 / (chunk_rows * w_max))),
// so weights that are integer multiples of 1/scale (unit weights, Poisson
// bootstrap counts) histogram EXACTLY, and decoding is an exact multiply.
// Chunking, the single-chunk plain-store flush and the i64 staging slots of
// multi-chunk nodes (bitwise deterministic) come from csrc/hist_plan.h, the
// same plan hist_build uses; the staging decode is ops.hip's.

#include <ATen/hip/HIPContext.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "hist_plan.h"

// chunk table: int32 [2 + n_chunks * 5]; words 0/1 are the f32 scale and
// its exact reciprocal, then the plan's records (node, start, len,
// stage_slot, col0) with stage_slot < 0 for single-chunk nodes.
__global__ __launch_bounds__(1024) void hist_class_kernel(
    float* __restrict__ out,              // [n_nodes, F, B, K + NN]
    long long* __restrict__ stage,        // [n_multi, F, B, K + NN] i64
    const uint8_t* __restrict__ bins,     // [N, F] (row-major source)
    const uint8_t* __restrict__ bins_t,   // [F, N] (transposed source) or null
    const uint8_t* __restrict__ label,    // [N]
    const float* __restrict__ weight,     // [N, T]
    const int* __restrict__ row_idx,      // [M]
    const int* __restrict__ chunks, int64_t N, int F, int B, int K, int NN,
    int FG, int T, int identity_rows) {
  extern __shared__ unsigned long long cls_lds[];  // FG * B * K cells
  const float scale = __int_as_float(chunks[0]);
  const float inv_scale = __int_as_float(chunks[1]);
  const int* chk = chunks + 2 + blockIdx.x * 5;
  const int node = chk[0];
  const int start = chk[1];
  const int len = chk[2];
  const int slot = chk[3];
  const int col0 = chk[4];
  const int f0 = blockIdx.y * FG;
  const int nf = min(FG, F - f0);
  const int C = K + NN;

  const int lds_cells = nf * B * K;
  for (int i = threadIdx.x; i < lds_cells; i += blockDim.x) cls_lds[i] = 0ull;
  __syncthreads();

  for (int i = threadIdx.x; i < len; i += blockDim.x) {
    const int r = identity_rows ? start + i : row_idx[start + i];
    const int k = label[r];
    if (k >= K) continue;  // contract: label in [0, K); never index past LDS
    const float w = weight[(int64_t)r * T + col0];
    const unsigned q = (unsigned)__float2int_rn(w * scale);
    const unsigned long long addend = ((unsigned long long)q << 32) | 1ull;
    if (bins_t != nullptr) {
      const uint8_t* bc = bins_t + (int64_t)f0 * N + r;
      for (int f = 0; f < nf; ++f) {
        const int b = bc[(int64_t)f * N];
        if (b < B) atomicAdd(cls_lds + ((f * B) + b) * K + k, addend);
      }
    } else {
      const uint8_t* br = bins + (int64_t)r * F + f0;
      for (int f = 0; f < nf; ++f) {
        const int b = br[f];
        if (b < B) atomicAdd(cls_lds + ((f * B) + b) * K + k, addend);
      }
    }
  }
  __syncthreads();

  // flush: one thread per (feature, bin) walks the bin's K cells.  The
  // walk starts at class (fb % K) and wraps, so the lanes of a wave hit
  // different LDS banks even when K * 8 B is a multiple of the bank row
  // (K = 32 would otherwise serialise 32-way).  hess and count are the
  // INTEGER sums over the classes, decoded once.
  for (int fb = threadIdx.x; fb < nf * B; fb += blockDim.x) {
    const unsigned long long* cell = cls_lds + (int64_t)fb * K;
    const int64_t o_off = (((int64_t)f0 * B) + fb) * C;
    long long hs = 0, cs = 0;
    int k = fb % K;
    if (slot < 0) {
      float* o = out + (int64_t)node * F * B * C + o_off;
      for (int j = 0; j < K; ++j) {
        const unsigned long long v = cell[k];
        const unsigned hi = (unsigned)(v >> 32);
        o[k] = (float)hi * inv_scale;
        hs += hi;
        cs += (unsigned)(v & 0xFFFFFFFFull);
        if (++k == K) k = 0;
      }
      o[K] = (float)hs * inv_scale;
      if (NN == 2) o[K + 1] = (float)cs;
    } else {
      long long* o = stage + (int64_t)slot * F * B * C + o_off;
      for (int j = 0; j < K; ++j) {
        const unsigned long long v = cell[k];
        const unsigned hi = (unsigned)(v >> 32);
        if (hi) atomicAdd((unsigned long long*)(o + k), (unsigned long long)hi);
        hs += hi;
        cs += (unsigned)(v & 0xFFFFFFFFull);
        if (++k == K) k = 0;
      }
      if (hs) atomicAdd((unsigned long long*)(o + K), (unsigned long long)hs);
      if (NN == 2 && cs)
        atomicAdd((unsigned long long*)(o + K + 1), (unsigned long long)cs);
    }
  }
}

// Returns the number of multi-chunk nodes (callers/tests can tell which
// flush path a launch took).
int64_t hist_build_class(torch::Tensor out, torch::Tensor bins,
                         torch::Tensor bins_t, torch::Tensor label,
                         torch::Tensor weight, torch::Tensor row_idx,
                         torch::Tensor node_offsets, torch::Tensor node_col0,
                         int64_t num_bins, int64_t num_classes, int64_t nn,
                         double w_max, bool identity_rows) {
  CHECK_GPU(out); CHECK_GPU(bins); CHECK_GPU(label);
  CHECK_GPU(weight); CHECK_GPU(row_idx);
  CHECK_CONTIG(out); CHECK_CONTIG(bins); CHECK_CONTIG(label);
  CHECK_CONTIG(weight); CHECK_CONTIG(row_idx);
  TORCH_CHECK(!node_offsets.is_cuda(), "node_offsets stays on host");
  TORCH_CHECK(!node_col0.is_cuda(), "node_col0 stays on host");
  TORCH_CHECK(bins.scalar_type() == torch::kUInt8 &&
                  label.scalar_type() == torch::kUInt8,
              "bins and label must be uint8");
  TORCH_CHECK(weight.scalar_type() == torch::kFloat32 && weight.dim() == 2,
              "weight must be [N, T] f32");
  TORCH_CHECK(row_idx.scalar_type() == torch::kInt32, "row_idx must be i32");
  TORCH_CHECK(node_offsets.scalar_type() == torch::kInt64 &&
                  node_col0.scalar_type() == torch::kInt32,
              "node_offsets i64 / node_col0 i32");
  const int64_t N = bins.size(0);
  const int F = (int)bins.size(1);
  const int B = (int)num_bins;
  const int K = (int)num_classes;
  const int NN = (int)nn;
  const int T = (int)weight.size(1);
  const int C = K + NN;
  const int n_nodes = (int)node_offsets.numel() - 1;
  TORCH_CHECK(B >= 1 && B <= 256, "hist_build_class: 1 <= B <= 256");
  TORCH_CHECK(K >= 2 && K <= 32, "hist_build_class: 2 <= K <= 32");
  TORCH_CHECK(NN == 1 || NN == 2, "hist_build_class: NN in {1, 2}");
  TORCH_CHECK(label.numel() == N && weight.size(0) == N,
              "label / weight rows must match bins");
  TORCH_CHECK(node_col0.numel() == n_nodes,
              "node_col0 must have one entry per node");
  TORCH_CHECK(out.numel() == (int64_t)n_nodes * F * B * C,
              "out must be [n_nodes, F, B, K + NN]");
  const bool transposed = bins_t.numel() > 0;
  if (transposed) {
    CHECK_GPU(bins_t); CHECK_CONTIG(bins_t);
    TORCH_CHECK(bins_t.size(0) == F && bins_t.size(1) == N,
                "bins_t must be the [F, N] transpose of bins");
  }
  if (n_nodes == 0 || F == 0) return 0;

  // feature-group size under the LDS budget FG * B * K * 8 <= 160 KiB
  // (FG = 2 at B=256, K=32; FG = 3 at K=26), capped at 16 and evened out
  // over the groups so F need not be a multiple of it
  const int budget = 163840;
  int FG = std::max(1, std::min(F, budget / (B * K * 8)));
  FG = std::min(FG, 16);
  const int n_groups = (int)ceil_div(F, FG);
  FG = (int)ceil_div(F, n_groups);
  const size_t lds_bytes = (size_t)FG * B * K * 8;
  const int blocks_per_cu = std::max<int>(1, (int)(budget / lds_bytes));
  const int threads = blocks_per_cu == 1 ? 1024 : (blocks_per_cu == 2 ? 512 : 256);

  CHECK_CONTIG(node_offsets); CHECK_CONTIG(node_col0);
  HistPlan plan = plan_hist_chunks(
      node_offsets.data_ptr<int64_t>(), n_nodes, node_col0.data_ptr<int>(),
      identity_rows ? N : row_idx.numel(), T, lds_bytes, n_groups, 2);

  // header: the fixed-point scale rounded DOWN to a power of two, and its
  // exact reciprocal
  const float scale = (float)std::exp2(
      std::floor(std::log2(hist_fixed_scale(plan.chunk_rows, w_max))));
  const float inv_scale = 1.0f / scale;
  std::memcpy(&plan.table[0], &scale, 4);
  std::memcpy(&plan.table[1], &inv_scale, 4);
  auto chunks = h2d_async(plan.table.data(), plan.table.size() * 4,
                          kSlotClassChunks, bins.device())
                    .view(torch::kInt32);

  const int n_multi = (int)plan.multi_nodes.size();
  torch::Tensor stage;
  long long* stage_ptr = nullptr;
  if (n_multi) {
    stage = torch::zeros({(int64_t)n_multi, (int64_t)F, (int64_t)B, (int64_t)C},
                         out.options().dtype(torch::kInt64));
    stage_ptr = reinterpret_cast<long long*>(stage.data_ptr<int64_t>());
  }

  auto stream = at::hip::getCurrentHIPStream();
  if (lds_bytes > 65536)
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(&hist_class_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  hipLaunchKernelGGL(
      hist_class_kernel, dim3(plan.n_chunks, n_groups), dim3(threads), lds_bytes,
      stream, out.data_ptr<float>(), stage_ptr, bins.data_ptr<uint8_t>(),
      transposed ? bins_t.data_ptr<uint8_t>() : (const uint8_t*)nullptr,
      label.data_ptr<uint8_t>(), weight.data_ptr<float>(),
      row_idx.data_ptr<int>(), chunks.data_ptr<int>(), N, F, B, K, NN, FG, T,
      identity_rows ? 1 : 0);
  if (n_multi) {
    // one upload: node of each staging slot, then the decode divisors (the
    // scale for the K class channels and hess, 1 for the count channel)
    std::vector<int> dec(plan.multi_nodes);
    dec.resize(n_multi + C);
    float* div = reinterpret_cast<float*>(dec.data() + n_multi);
    for (int c = 0; c < C; ++c) div[c] = c > K ? 1.0f : scale;
    auto dec_d = h2d_async(dec.data(), dec.size() * 4, kSlotClassNodes,
                           bins.device())
                     .view(torch::kInt32);
    launch_hist_decode(
        out.data_ptr<float>(), stage_ptr, dec_d.data_ptr<int>(),
        reinterpret_cast<const float*>(dec_d.data_ptr<int>() + n_multi),
        n_multi, (int64_t)F * B * C, C, stream);
  }
  return n_multi;
}

// ---------------------------------------------------------------------------
// split_argmax_wide: the split_argmax_kernel semantics for 9 <= C <= 34.
//   The narrow kernel keeps loc[4][C] per lane in registers; at C = 34
//   that spills.  Here ONE wave (a 64-thread block) owns a (node, feature):
//   the feature's [B, C] slice is staged channel-major in LDS with
//   coalesced global reads, then a runtime loop over channels does one wave
//   prefix scan per channel while each lane keeps only the running
//   gl / gr / hl / cl of its <= 4 consecutive bins.  Same gain formula,
//   same validity tests, same packed atomicMax tie rule.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(64) void split_argmax_wide_kernel(
    unsigned long long* __restrict__ best,  // [n_nodes] pre-zeroed
    const float* __restrict__ hist,         // [n_nodes, F, B, C]
    int F, int B, int C, int D, float lam, float min_child_weight,
    float min_instances) {
  extern __shared__ float split_lds[];  // [C][Bp] channel-major
  const int node = blockIdx.x;
  const int f = blockIdx.y;
  const int lane = threadIdx.x;
  const float* h = hist + (((int64_t)node * F + f) * (int64_t)B) * C;
  const int BPL = (B + 63) >> 6;  // <= 4 for B <= 256
  const int Bp = B + 1;           // odd pitch: spreads the transposing writes
  const int idx_c = C - 1;        // count channel

  for (int j = lane; j < B * C; j += 64) {
    const int b = j / C, c = j - b * C;
    split_lds[c * Bp + b] = h[j];
  }
  __syncthreads();

  float gl[4], gr[4], hl[4], cl[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) gl[i] = gr[i] = hl[i] = cl[i] = 0.0f;
  float pg2 = 0.0f, parent_h = 0.0f, parent_c = 0.0f;
  const int b0 = lane * BPL;

  for (int c = 0; c < C; ++c) {
    const float* row = split_lds + c * Bp;
    float v[4];
    float tot = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = b0 + i;
      v[i] = (i < BPL && b < B) ? row[b] : 0.0f;
      tot += v[i];
    }
    // wave-wide inclusive scan of the lane totals
    float s = tot;
    for (int off = 1; off < 64; off <<= 1) {
      const float u = __shfl_up(s, off, 64);
      if (lane >= off) s += u;
    }
    const float parent = __shfl(s, 63, 64);
    float run = s - tot;  // exclusive prefix
    const bool is_g = c < D;
    if (is_g) pg2 += parent * parent;
    if (c == D) parent_h = parent;
    if (c == idx_c) parent_c = parent;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      run += v[i];
      if (is_g) {
        const float r = parent - run;
        gl[i] += run * run;
        gr[i] += r * r;
      }
      if (c == D) hl[i] = run;
      if (c == idx_c) cl[i] = run;
    }
  }
  const float parent_score = pg2 / (parent_h + lam);

  unsigned best_s = 0u;
  int best_b = -1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = b0 + i;
    if (i < BPL && b < B - 1) {  // last bin cannot split
      const float hr = parent_h - hl[i];
      const float cr = parent_c - cl[i];
      if (hl[i] >= min_child_weight && hr >= min_child_weight &&
          cl[i] >= min_instances && cr >= min_instances) {
        const float gain =
            gl[i] / (hl[i] + lam) + gr[i] / (hr + lam) - parent_score;
        const unsigned sg = f32_sortable(gain);
        if (sg > best_s) { best_s = sg; best_b = b; }
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned os = __shfl_down(best_s, off, 64);
    const int ob = __shfl_down(best_b, off, 64);
    if (os > best_s) { best_s = os; best_b = ob; }
  }
  if (lane == 0 && best_b >= 0) {
    const unsigned long long packed =
        ((unsigned long long)best_s << 32) | (unsigned)(f * B + best_b);
    atomicMax(&best[node], packed);
  }
}

__global__ __launch_bounds__(64) void split_decode_wide_kernel(
    float* __restrict__ gain, int* __restrict__ feat, int* __restrict__ bin,
    float* __restrict__ left_stats,  // [n, C]
    const unsigned long long* __restrict__ best,
    const float* __restrict__ hist, int F, int B, int C,
    float min_info_gain) {
  const int node = blockIdx.x;
  const int c = threadIdx.x;
  const unsigned long long p = best[node];
  const float g = sortable_f32((unsigned)(p >> 32));
  if (p == 0ull || !(g >= min_info_gain)) {
    if (c == 0) {
      gain[node] = -INFINITY;
      feat[node] = -1;
      bin[node] = -1;
    }
    if (c < C) left_stats[(int64_t)node * C + c] = 0.0f;
    return;
  }
  const int fb = (int)(p & 0xFFFFFFFFull);
  const int f = fb / B, b = fb % B;
  const float* h = hist + (((int64_t)node * F + f) * (int64_t)B) * C;
  if (c < C) {
    float acc = 0.0f;
    for (int i = 0; i <= b; ++i) acc += h[(int64_t)i * C + c];
    left_stats[(int64_t)node * C + c] = acc;
  }
  if (c == 0) {
    gain[node] = g;
    feat[node] = f;
    bin[node] = b;
  }
}

// called from split_argmax (csrc/ops.hip) for C > 8; arguments are already
// validated there except the wide channel cap
void split_argmax_wide(torch::Tensor gain, torch::Tensor feat,
                       torch::Tensor bin, torch::Tensor left_stats,
                       torch::Tensor hist, int D, double lam,
                       double min_child_weight, double min_instances,
                       double min_info_gain) {
  const int n = (int)hist.size(0);
  const int F = (int)hist.size(1);
  const int B = (int)hist.size(2);
  const int C = (int)hist.size(3);
  TORCH_CHECK(C >= 9 && C <= 34, "split_argmax_wide: 9 <= C <= 34");
  TORCH_CHECK(gain.numel() == n && feat.numel() == n && bin.numel() == n &&
                  left_stats.numel() == (int64_t)n * C,
              "split_argmax_wide: output shapes");
  if (n == 0) return;
  auto best = torch::zeros({n}, hist.options().dtype(torch::kInt64));
  auto stream = at::hip::getCurrentHIPStream();
  if (F > 0) {
    const size_t lds = (size_t)C * (B + 1) * sizeof(float);  // <= 34952 B
    hipLaunchKernelGGL(split_argmax_wide_kernel, dim3(n, F), dim3(64), lds,
                       stream, (unsigned long long*)best.data_ptr<int64_t>(),
                       hist.data_ptr<float>(), F, B, C, D, (float)lam,
                       (float)min_child_weight, (float)min_instances);
  }
  hipLaunchKernelGGL(split_decode_wide_kernel, dim3(n), dim3(64), 0, stream,
                     gain.data_ptr<float>(), feat.data_ptr<int>(),
                     bin.data_ptr<int>(), left_stats.data_ptr<float>(),
                     (unsigned long long*)best.data_ptr<int64_t>(),
                     hist.data_ptr<float>(), F, B, C, (float)min_info_gain);
}
