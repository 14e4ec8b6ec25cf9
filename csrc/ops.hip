// spark_ensemble_amd gfx950 (CDNA4 / MI355X) kernels.
//
// Hand-written HIP for the framework's hot path (SURVEY.md section 2.7 maps
// each kernel to the reference semantics it replaces):
//   * hist_build      — LDS-staged per-(node, feature, bin) grad/hess/count
//                       histograms (replaces MLlib DecisionTree's
//                       treeAggregate histogram rounds)
//   * partition_rows  — block-aggregated two-pass node partition
//   * bin_features    — quantile binning (raw f32 -> uint8 bin ids)
//   * tree_predict /
//     forest_predict  — batched node-array tree walks
//   * sample_weights  — counter-based Poisson/Bernoulli row sampling
//   * grad_hess /
//     line_search_eval— fused per-row GBM loss work (one pass over the
//                       shard + one short reduction payload)
//
// Design notes (MI355X_MICROARCH.md): 64-wide waves, 256-thread blocks;
// histograms live in LDS; the host cuts each level into chunks sized to the
// resident grid (policy in csrc/hist_plan.h, shared with wide_class.hip);
// single-chunk nodes flush with plain stores.

#include <ATen/hip/HIPContext.h>

#include <chrono>
#include <cstring>
#include <tuple>
#include <vector>

#include "common.h"
#include "gbm_loss.h"
#include "hist_plan.h"

// Persistent pinned staging for the small per-launch host tables (chunk
// lists, cursors): a pageable .to(device) blocks the HOST until the copy
// completes, and the stream-ordered copy waits for every queued kernel —
// serializing each tree level behind the previous one.  Pinned source +
// non_blocking copy keeps the host running ahead.  Slots rotate per call
// site; reuse is safe because every level ends in a host sync (the split
// fetch) before the slot is touched again.
torch::Tensor h2d_async(const void* src, size_t bytes, UploadSlot slot,
                        const torch::Device& dev) {
  static thread_local torch::Tensor pin[2 * kUploadSlots];
  static thread_local hipEvent_t done[2 * kUploadSlots] = {};
  static thread_local unsigned char flip[kUploadSlots] = {};
  // the PREVIOUS copy from this slot may still be pending on the
  // stream: overwriting (or freeing, when the slot grows) the pinned
  // staging before the DMA reads it feeds the kernels garbage
  // descriptors — the depth-12 / 100M-row GPU memory faults.  Each
  // slot PING-PONGS between two buffers so the completion wait below
  // lands on the copy from TWO calls ago — with the host running at
  // most one level ahead that copy has long executed, preserving the
  // run-ahead pipelining the level loop depends on.
  flip[slot] ^= 1;
  const int bi = slot * 2 + flip[slot];
  auto& b = pin[bi];
  if (done[bi]) (void)hipEventSynchronize(done[bi]);
  if (!b.defined() || (size_t)b.numel() < bytes) {
    size_t cap = 4096;
    while (cap < bytes) cap *= 2;
    b = torch::empty({(int64_t)cap},
                     torch::TensorOptions().dtype(torch::kByte)
                         .pinned_memory(true));
  }
  std::memcpy(b.data_ptr(), src, bytes);
  auto d = torch::empty({(int64_t)bytes},
                        torch::TensorOptions().dtype(torch::kByte).device(dev));
  // raw async copy on the current stream: torch's copy_(non_blocking)
  // proved to still block the host behind queued kernels here
  auto stream = at::hip::getCurrentHIPStream();
  (void)hipMemcpyAsync(d.data_ptr(), b.data_ptr(), bytes,
                       hipMemcpyHostToDevice, stream);
  if (!done[bi])
    (void)hipEventCreateWithFlags(&done[bi], hipEventDisableTiming);
  (void)hipEventRecord(done[bi], stream);
  return d;
}

// ---------------------------------------------------------------------------
// sample_weights: counter-based RNG (splitmix64), one state per row
// ---------------------------------------------------------------------------

__device__ inline uint64_t splitmix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

__device__ inline float u01(uint64_t z) {
  return ((z >> 40) + 1) * (1.0f / 16777216.0f);  // upper 24 bits -> (0, 1]
}

__global__ void sample_weights_kernel(float* __restrict__ out, int64_t n,
                                      int replacement, float ratio,
                                      uint64_t seed) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    uint64_t s = seed ^ (0x9e3779b97f4a7c15ull * (uint64_t)(i + 1));
    if (!replacement) {
      uint64_t z = splitmix64(s);
      out[i] = (u01(z) <= ratio) ? 1.0f : 0.0f;
    } else {
      // Knuth Poisson(ratio): E[iters] = ratio + 1 (ratio <= 1 in practice)
      float L = __expf(-ratio);
      float p = 1.0f;
      int k = 0;
      uint64_t z = s;
      do {
        z = splitmix64(z);
        p *= u01(z);
        k++;
      } while (p > L && k < 64);
      out[i] = (float)(k - 1);
    }
  }
}

void sample_weights(torch::Tensor out, bool replacement, double ratio,
                    int64_t seed, int64_t rank) {
  CHECK_GPU(out);
  CHECK_CONTIG(out);
  int64_t n = out.numel();
  auto stream = at::hip::getCurrentHIPStream();
  uint64_t s = (uint64_t)seed * 0x100000001b3ull + (uint64_t)rank * 0x9e3779b9ull;
  int threads = 256;
  int blocks = (int)std::min<int64_t>(ceil_div(n, threads), 8192);
  hipLaunchKernelGGL(sample_weights_kernel, dim3(blocks), dim3(threads), 0,
                     stream, out.data_ptr<float>(), n, replacement ? 1 : 0,
                     (float)ratio, s);
}

// ---------------------------------------------------------------------------
// bin_features: [N, F] f32 + [F, B-1] edges -> [N, F] u8
//   edges for one feature stay in registers? no — binary search in L1/L2.
//   Thread covers one (row, feature); consecutive threads cover consecutive
//   features of one row so the x reads coalesce.
// ---------------------------------------------------------------------------

// Feature-tiled: grid (row_chunks, F/16); each block stages its 16
// features' quantile edges in LDS (16 x nedges f32 <= 16 KiB at 255
// edges), then loops rows with 64-B coalesced x row-slice loads and
// LDS binary searches — the naive per-element global-edge search ran at
// 34 GB/s, this at HBM row-read rate.
__global__ void bin_features_kernel(uint8_t* __restrict__ out,
                                    const float* __restrict__ x,
                                    const float* __restrict__ edges, int64_t n,
                                    int F, int nedges) {
  constexpr int FT = 16;
  extern __shared__ float elds[];  // [FT][nedges]
  const int f0 = blockIdx.y * FT;
  const int nf = min(FT, F - f0);
  for (int i = threadIdx.x; i < nf * nedges; i += blockDim.x)
    elds[i] = edges[(int64_t)f0 * nedges + i];
  __syncthreads();

  const bool full = (nf == FT) && ((F & 15) == 0);
  int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t rstride = gridDim.x * (int64_t)blockDim.x;
  for (; r < n; r += rstride) {
    float v[FT];
    if (full) {
      const float4* xr = reinterpret_cast<const float4*>(x + r * F + f0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 t = xr[q];
        v[q * 4 + 0] = t.x; v[q * 4 + 1] = t.y;
        v[q * 4 + 2] = t.z; v[q * 4 + 3] = t.w;
      }
    } else {
      for (int j = 0; j < nf; ++j) v[j] = x[r * F + f0 + j];
    }
    uint8_t b[FT];
    for (int j = 0; j < nf; ++j) {
      const float* e = elds + j * nedges;
      int lo = 0, hi = nedges;  // first index with e[idx] >= v
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] >= v[j]) hi = mid; else lo = mid + 1;
      }
      b[j] = (uint8_t)lo;
    }
    if (full) {
      uint4 packed;
      unsigned* w = reinterpret_cast<unsigned*>(&packed);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        w[q] = (unsigned)b[q * 4] | ((unsigned)b[q * 4 + 1] << 8) |
               ((unsigned)b[q * 4 + 2] << 16) | ((unsigned)b[q * 4 + 3] << 24);
      *reinterpret_cast<uint4*>(out + r * F + f0) = packed;
    } else {
      for (int j = 0; j < nf; ++j) out[r * F + f0 + j] = b[j];
    }
  }
}

void bin_features(torch::Tensor out, torch::Tensor x, torch::Tensor edges) {
  CHECK_GPU(out); CHECK_GPU(x); CHECK_GPU(edges);
  CHECK_CONTIG(out); CHECK_CONTIG(x); CHECK_CONTIG(edges);
  int64_t n = x.size(0);
  int F = (int)x.size(1);
  int nedges = (int)edges.size(1);
  TORCH_CHECK(nedges <= 1024, "bin_features: too many edges for LDS staging");
  auto stream = at::hip::getCurrentHIPStream();
  const int threads = 256;
  const int fgroups = (int)ceil_div(F, 16);
  // 4 blocks/CU: a 1-block/CU grid (old 4096/fgroups cap) left the
  // float4 row loads latency-bound at ~1.2 TB/s (rocprof r02)
  int rblocks = (int)std::min<int64_t>(
      ceil_div(n, threads), std::max<int64_t>(1, 16384 / fgroups));
  const size_t lds = (size_t)16 * nedges * 4;
  hipLaunchKernelGGL(bin_features_kernel, dim3(rblocks, fgroups),
                     dim3(threads), lds, stream, out.data_ptr<uint8_t>(),
                     x.data_ptr<float>(), edges.data_ptr<float>(), n, F,
                     nedges);
}

// ---------------------------------------------------------------------------
// hist_build
//   grid = (row_chunks, feature_groups); LDS histogram of FG*B*CELLS u64.
//
//   LDS LAYOUT (tools/probe_hist5.hip + profiles/hist_layout.md): an 8-byte
//   LDS atomic is serviced in 4 groups of 16 contiguous lanes over 16 bank
//   pairs, one extra cycle per extra address on a busy pair.  With cells
//   [f][b][c] and every lane on the same feature the pair is b mod 16 —
//   16 random bins into 16 pairs, 3.07 deep on average (the 67 %
//   SQ_LDS_BANK_CONFLICT share).  The vectorised path (full groups of FG in
//   {16, 32, 64}) therefore keeps cells BIN-MAJOR, [c][b][f], so the pair is
//   f mod 16 whatever the bin, and lane l walks the 16 features of a piece
//   rotated by l % 16: 16 contiguous lanes always hit 16 different pairs
//   (probe: 9.1 vs 4.5 adds/clk/CU).  The byte-wise fallback (ragged or
//   small groups) has all lanes on one feature, where bin-major would be a
//   16-way conflict; it keeps [f][b][c].
//
//   KEY gfx950 design point (measured, tools/probe_hist2.hip +
//   profiles/r01_hist_probe.md): LDS f32 atomicAdd (ds_add_f32) runs ~13x
//   slower than LDS u64 integer atomicAdd (ds_add_u64) — 101 vs 1395 G
//   bump/s at B=256 — so the histogram accumulates in FIXED POINT: each
//   64-bit cell packs one SIGNED channel (gradient, high 32) and one
//   NON-NEGATIVE channel (hessian/count, low 32) and is bumped with ONE
//   ds_add_u64.  Channel convention (tree_grower.py): channels [0, D) are
//   signed gradients, channels [D, C) are non-negative hess/count, so
//   CELLS = max(D, C - D).  Host-chosen per-channel scales guarantee
//   |sum| < 2^30 per chunk per bin (no field overflow, low->high carries
//   impossible since low fields are non-negative and bounded).
//
//   chunks: int32 [n_chunks, 5] = (node, start, len, stage_slot, col0)
//   as planned by csrc/hist_plan.h; quantization scales ride in the same
//   upload (one H2D per launch).  ``col0`` is the node's base column in a gh matrix of row
//   stride CH — 0/CH==C for single-tree builds; a FOREST build (K trees
//   or K classes grown level-synchronously, reference
//   GBMClassifier.scala:377-411 parallel futures) interleaves per-tree
//   channel groups [g_t, h_t(, cnt_t)] and sets col0 = tree * C, so one
//   launch histograms every active node of every tree.
//   ``gh_pos``: gh is the compact [M, CH] matrix gather_ranges_gh built
//   alongside row_idx, so position start + i reads gh row start + i (a
//   stream) while bins are still fetched through row_idx.
//   Flush, single-chunk nodes (stage_slot < 0): convert back to f32 straight
//   into out [n_nodes, F, B, C] with plain stores, 16 B per lane for C = 2.
//   Multi-chunk nodes of the one-cell bin-major kernel: each block copies
//   its LDS image as it stands into its own slab of ``partial``
//   ([multi records, n_groups, FG*B] u64); hist_reduce_kernel sums a node's
//   slabs in int64 and converts.  After the chunk records the table carries
//   (node, first record, record count, first slab) per staging slot.
//   Kernels of two and more cells, the byte-wise fallback and a partial
//   buffer over its size bound add integer atomics into the slot of the i64
//   ``stage`` buffer instead, which hist_decode_kernel converts.
// ---------------------------------------------------------------------------

// rotate the 16 bytes of a bins piece right by lam bytes: byte p of the
// result is byte (p + lam) % 16 of the input.  A dword rotate by lam >> 2
// (two levels of selects) and a funnel shift by lam & 3 bytes, so the bytes
// are still extracted with compile-time indices (no dynamic register index).
__device__ inline void rotate_piece(unsigned (&w)[4], int lam) {
  const bool r1 = lam & 4, r2 = lam & 8;
  const unsigned a0 = r1 ? w[1] : w[0], a1 = r1 ? w[2] : w[1],
                 a2 = r1 ? w[3] : w[2], a3 = r1 ? w[0] : w[3];
  const unsigned b0 = r2 ? a2 : a0, b1 = r2 ? a3 : a1, b2 = r2 ? a0 : a2,
                 b3 = r2 ? a1 : a3;
  const unsigned t = lam & 3;
  w[0] = __builtin_amdgcn_alignbyte(b1, b0, t);
  w[1] = __builtin_amdgcn_alignbyte(b2, b1, t);
  w[2] = __builtin_amdgcn_alignbyte(b3, b2, t);
  w[3] = __builtin_amdgcn_alignbyte(b0, b3, t);
}

// Which instantiations flush multi-chunk nodes as slabs: the one-cell kernel
// (C = 2, the flagship).  With two cells the slabs measured slower than the
// staged atomics on three hist_bench rows (profiles/hist_flush.md), so two
// and more cells keep the atomics.
template <int DC, int NC>
constexpr bool kHistSlabFlush = (DC > NC ? DC : NC) == 1;

// BM (bin-major) is the vectorised path: every feature group is a full
// FG in {16, 32, 64} features.  !BM is the byte-wise fallback.
template <int DC, int NC, bool BM>
__global__ void hist_build_kernel(
    float* __restrict__ out,            // [n_nodes, F, B, C]
    long long* __restrict__ stage,      // [n_multi, F, B, C] i64, or null
    unsigned long long* __restrict__ partial,  // LDS-image slabs (BM), or null
    const uint8_t* __restrict__ bins,   // [N, F]
    const float* __restrict__ gh,       // [N, CH], or [M, CH] with gh_pos
    const int* __restrict__ row_idx,    // [M]
    const int* __restrict__ chunks,     // scales, chunk records, slot records
    int F, int B, int FG, int CH, int identity_rows, int gh_pos) {
  constexpr int C = DC + NC;
  constexpr int CELLS = DC > NC ? DC : NC;
  extern __shared__ unsigned long long lds64[];  // FG * B * CELLS
  const float* scales = reinterpret_cast<const float*>(chunks);
  const int* chk = chunks + 2 * C + blockIdx.x * 5;
  const int fg = blockIdx.y;
  const int f0 = fg * FG;
  const int nf = min(FG, F - f0);
  const int node = chk[0];
  const int start = chk[1];
  const int len = chk[2];
  const int slot = chk[3];
  const int col0 = chk[4];

  const int lds_cells = FG * B * CELLS;
  for (int i = threadIdx.x; i < lds_cells; i += blockDim.x) lds64[i] = 0ull;
  __syncthreads();

  // BM: the host's FG choice gives FG <= 64 / 32 / 16 for CELLS 1 / 2 / >= 3
  constexpr int MAXNH = CELLS == 1 ? 4 : (CELLS == 2 ? 2 : 1);
  const int nh = FG >> 4;
  const int lam = threadIdx.x & 15;
  const int bshift = 31 - __clz(FG) + 3;      // log2(FG * 8)
  const unsigned plane = (unsigned)B * FG * 8;  // bytes per cell plane
  // BM: byte offset of the feature that byte p of a rotated piece holds
  unsigned foff[16];
#pragma unroll
  for (int p = 0; p < 16; ++p) foff[p] = ((p + lam) & 15) * 8;

  for (int i = threadIdx.x; i < len; i += blockDim.x) {
    const int r = identity_rows ? start + i : row_idx[start + i];
    const float* g = gh + (int64_t)(gh_pos ? start + i : r) * CH + col0;
    // quantize once per row, pack one u64 addend per cell
    unsigned long long addend[CELLS];
#pragma unroll
    for (int c = 0; c < CELLS; ++c) addend[c] = 0ull;
#pragma unroll
    for (int d = 0; d < DC; ++d) {
      const int iv = __float2int_rn(g[d] * scales[d]);
      addend[d] |= ((unsigned long long)(unsigned)iv) << 32;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int iv = __float2int_rn(g[DC + c] * scales[DC + c]);
      addend[c] |= (unsigned)iv;
    }
    if constexpr (BM) {
      // the row's FG bytes in 16-B uint4 pieces; at step p of piece hh this
      // lane bumps feature 16*hh + (p + lam) % 16, so any 16 contiguous
      // lanes hit 16 different bank pairs whatever their bins are
      const uint8_t* br = bins + (int64_t)r * F + f0;
      uint4 bv[MAXNH];
#pragma unroll
      for (int hh = 0; hh < MAXNH; ++hh) {
        bv[hh] = make_uint4(0, 0, 0, 0);
        if (hh < nh) bv[hh] = *reinterpret_cast<const uint4*>(br + 16 * hh);
      }
      char* base = reinterpret_cast<char*>(lds64);
#pragma unroll
      for (int hh = 0; hh < MAXNH; ++hh) {
        if (hh >= nh) break;
        unsigned w[4] = {bv[hh].x, bv[hh].y, bv[hh].z, bv[hh].w};
        rotate_piece(w, lam);
#pragma unroll
        for (int p = 0; p < 16; ++p) {
          const unsigned b = (w[p >> 2] >> (8 * (p & 3))) & 0xff;
          char* cell = base + ((b << bshift) + foff[p]) + hh * 128;
#pragma unroll
          for (int c = 0; c < CELLS; ++c)
            atomicAdd(reinterpret_cast<unsigned long long*>(cell + c * plane),
                      addend[c]);
        }
      }
    } else {
      const uint8_t* br = bins + (int64_t)r * F + f0;
      for (int f = 0; f < nf; ++f) {
        const int b = br[f];
        unsigned long long* cell = lds64 + ((f * B) + b) * CELLS;
#pragma unroll
        for (int c = 0; c < CELLS; ++c) atomicAdd(cell + c, addend[c]);
      }
    }
  }
  __syncthreads();

  // flush. Single-chunk nodes: decode fixed point -> f32 straight into
  // out (plain stores).  Multi-chunk nodes: accumulate INTEGER partials
  // into the i64 staging buffer — integer atomics are order-independent,
  // so histograms stay bitwise deterministic across runs (decode kernel
  // below converts once at the end).
  // cell c of (f, b) is cell[c * cstride]
  auto flush_cell = [&](int f, int b, const unsigned long long* cell,
                        int cstride) {
    if (slot < 0) {
      float* o = out + (((int64_t)node * F + f0 + f) * B + b) * C;
#pragma unroll
      for (int d = 0; d < DC; ++d)
        o[d] = (float)(int)(unsigned)(cell[d * cstride] >> 32) / scales[d];
#pragma unroll
      for (int c = 0; c < NC; ++c)
        o[DC + c] = (float)(int)(unsigned)(cell[c * cstride] & 0xFFFFFFFFull) /
                    scales[DC + c];
    } else {
      long long* o = stage + (((int64_t)slot * F + f0 + f) * B + b) * C;
#pragma unroll
      for (int d = 0; d < DC; ++d) {
        const int v = (int)(unsigned)(cell[d * cstride] >> 32);
        if (v) atomicAdd((unsigned long long*)(o + d),
                         (unsigned long long)(long long)v);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int v = (int)(unsigned)(cell[c * cstride] & 0xFFFFFFFFull);
        if (v) atomicAdd((unsigned long long*)(o + DC + c),
                         (unsigned long long)(long long)v);
      }
    }
  };
  if constexpr (BM) {
    if constexpr (kHistSlabFlush<DC, NC>) {
      if (slot >= 0 && partial) {
        // multi-chunk node: the LDS image goes as it stands, 16 B per lane,
        // into this block's slab; hist_reduce_kernel sums the node's slabs.
        // slot record = (node, first record, record count, first slab)
        const int* srec = chunks + 2 * C + (int)gridDim.x * 5 + slot * 4;
        const int64_t slab =
            (int64_t)(srec[3] + (int)blockIdx.x - srec[1]) * gridDim.y + fg;
        uint4* dst = reinterpret_cast<uint4*>(partial + slab * lds_cells);
        const uint4* img = reinterpret_cast<const uint4*>(lds64);
        for (int i = threadIdx.x; i < lds_cells / 2; i += blockDim.x)
          dst[i] = img[i];
        return;
      }
    }
    // single-chunk node, C = 2: a lane converts two adjacent bins of one
    // feature and stores them as one float4; a wave covers 8 features x 16
    // bins, 128 contiguous bytes of out per feature.  (The same with 4 bins
    // = three float4 per lane for C = 3 measured slower than the 8 x 8 tile,
    // profiles/hist_flush.md, so C = 3 stays on the tile.)
    constexpr int NB = C == 2 ? 2 : 1;
    if (NB > 1 && slot < 0 && B % NB == 0 &&  // NB == 1: never taken
        (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
      const int nbt = (B + 8 * NB - 1) / (8 * NB);
      const int n_tiles = (FG >> 3) * nbt;
      for (int i = threadIdx.x; i < n_tiles * 64; i += blockDim.x) {
        const int t = i >> 6, l = i & 63;
        const int ft = t / nbt, bt = t - ft * nbt;
        const int f = ft * 8 + (l >> 3), b = (bt * 8 + (l & 7)) * NB;
        if (b >= B) continue;
        float v[NB * C];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          const unsigned long long* cell = lds64 + (b + k) * FG + f;
#pragma unroll
          for (int d = 0; d < DC; ++d)
            v[k * C + d] =
                (float)(int)(unsigned)(cell[d * B * FG] >> 32) / scales[d];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            v[k * C + DC + c] =
                (float)(int)(unsigned)(cell[c * B * FG] & 0xFFFFFFFFull) /
                scales[DC + c];
        }
        float4* o = reinterpret_cast<float4*>(
            out + (((int64_t)node * F + f0 + f) * B + b) * C);
#pragma unroll
        for (int q = 0; q < NB * C / 4; ++q)
          o[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2],
                             v[4 * q + 3]);
      }
      return;
    }
    // consecutive bins of a feature are FG*8 bytes apart here, one bank for
    // a whole wave; walk tiles of 8 features x 8 bins per wave instead (8
    // bank pairs per group of 16 lanes, 8-bin runs of out per feature)
    constexpr int TBL = 3;           // log2 bins per tile
    constexpr int TB = 1 << TBL, TF = 64 >> TBL;
    const int nbt = (B + TB - 1) >> TBL;
    const int n_tiles = (FG / TF) * nbt;
    for (int i = threadIdx.x; i < n_tiles * 64; i += blockDim.x) {
      const int t = i >> 6, l = i & 63;
      const int ft = t / nbt, bt = t - ft * nbt;
      const int f = ft * TF + (l >> TBL), b = bt * TB + (l & (TB - 1));
      if (b < B) flush_cell(f, b, lds64 + b * FG + f, B * FG);
    }
  } else {
    for (int i = threadIdx.x; i < nf * B; i += blockDim.x) {
      const int f = i / B, b = i - f * B;
      flush_cell(f, b, lds64 + ((f * B) + b) * CELLS, 1);
    }
  }
}

// decode the i64 staging sums of multi-chunk nodes into f32 out
__global__ void hist_decode_kernel(float* __restrict__ out,
                                   const long long* __restrict__ stage,
                                   const int* __restrict__ nodes,  // [n_multi] node of each slot
                                   const float* __restrict__ scales,  // [C]
                                   int64_t FBC, int C) {
  const int64_t obase = (int64_t)nodes[blockIdx.y] * FBC;
  const int64_t sbase = (int64_t)blockIdx.y * FBC;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < FBC;
       i += gridDim.x * (int64_t)blockDim.x) {
    const int c = (int)(i % C);
    out[obase + i] = (float)stage[sbase + i] / scales[c];
  }
}

void launch_hist_decode(float* out, const long long* stage, const int* nodes,
                        const float* scales, int n_multi, int64_t FBC, int C,
                        hipStream_t stream) {
  const int dblocks = (int)std::min<int64_t>(ceil_div(FBC, 256), 1024);
  hipLaunchKernelGGL(hist_decode_kernel, dim3(dblocks, n_multi), dim3(256), 0,
                     stream, out, stage, nodes, scales, FBC, C);
}

// Sum the LDS-image slabs of each multi-chunk node of the bin-major path and
// convert: out[node, f, b, :] = (float)(int64 sum over the node's records of
// the fields of partial[slab, group of f][cell][b][f % FG]) / scale.  The
// integers and the divide are those of the staged-atomics path, and integer
// sums have no order, so both give the same bits.  Lanes walk the flush's
// 8 features x 8 bins tile: 64-byte runs on both sides.
__global__ void hist_reduce_kernel(
    float* __restrict__ out,                         // [n_nodes, F, B, C]
    const unsigned long long* __restrict__ partial,  // slabs
    const int* __restrict__ slots,   // [n_multi, 4] node, first, count, slab
    const float* __restrict__ scales,  // [C]
    int F, int B, int FG, int DC, int NC) {
  const int* srec = slots + blockIdx.y * 4;
  const int node = srec[0], count = srec[2];
  const int C = DC + NC, CELLS = DC > NC ? DC : NC;
  const int n_groups = F / FG;
  const int nbt = (B + 7) >> 3;
  const int group_tiles = (FG >> 3) * nbt;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = i >> 6, l = i & 63;
  const int g = t / group_tiles;
  if (g >= n_groups) return;
  const int tt = t - g * group_tiles;
  const int ft = tt / nbt, bt = tt - ft * nbt;
  const int f = ft * 8 + (l >> 3), b = bt * 8 + (l & 7);
  if (b >= B) return;
  const int64_t plane = (int64_t)B * FG;
  const int64_t kstride = (int64_t)n_groups * plane * CELLS;
  const unsigned long long* p =
      partial + ((int64_t)srec[3] * n_groups + g) * plane * CELLS + b * FG + f;
  float* o = out + (((int64_t)node * F + g * FG + f) * B + b) * C;
  for (int c = 0; c < CELLS; ++c) {
    long long hi = 0, lo = 0;
#pragma unroll 4
    for (int k = 0; k < count; ++k) {
      const unsigned long long v = p[k * kstride + c * plane];
      hi += (int)(unsigned)(v >> 32);
      lo += (int)(unsigned)(v & 0xFFFFFFFFull);
    }
    if (c < DC) o[c] = (float)hi / scales[c];
    if (c < NC) o[DC + c] = (float)lo / scales[DC + c];
  }
}

// The partial buffer of the slab flush is at most (records of multi-chunk
// nodes) x n_groups x lds_bytes; the planner keeps the records near one
// resident grid (32 MiB at 10M x 256 x 256 bins), but rows past 2^26 or very
// wide rows can outgrow that.  Above this bound the launch falls back to the
// staged atomics.
constexpr int64_t kHistPartialMaxBytes = (int64_t)1 << 30;

// Returns the number of multi-chunk nodes.  ``gh_by_position``: gh is the
// compact [row_idx.numel(), CH] matrix of gather_ranges_gh, read by position.
int64_t hist_build(torch::Tensor out, torch::Tensor bins, torch::Tensor gh,
                   torch::Tensor row_idx, torch::Tensor node_offsets,
                   int64_t num_bins, int64_t d_dims, torch::Tensor max_abs,
                   bool identity_rows, torch::Tensor node_col0,
                   int64_t c_per_node, bool gh_by_position) {
  CHECK_GPU(out); CHECK_GPU(bins); CHECK_GPU(gh); CHECK_GPU(row_idx);
  CHECK_CONTIG(out); CHECK_CONTIG(bins); CHECK_CONTIG(gh); CHECK_CONTIG(row_idx);
  TORCH_CHECK(!node_offsets.is_cuda(), "node_offsets stays on host");
  TORCH_CHECK(!max_abs.is_cuda(), "max_abs stays on host");
  TORCH_CHECK(!node_col0.is_cuda(), "node_col0 stays on host");
  CHECK_CONTIG(node_offsets); CHECK_CONTIG(node_col0);
  const int F = (int)bins.size(1);
  const int B = (int)num_bins;
  const int CH = (int)gh.size(1);  // gh row stride
  // channels PER NODE: gh width for single-tree builds; explicit for
  // forest builds where gh interleaves per-tree channel groups
  const int C = c_per_node > 0 ? (int)c_per_node : CH;
  const int n_nodes = (int)node_offsets.numel() - 1;
  const bool forest = node_col0.numel() > 0;
  TORCH_CHECK(!forest || node_col0.numel() == n_nodes,
              "node_col0 must have one entry per node");
  const int D = d_dims > 0 ? (int)d_dims : (C >= 3 ? C - 2 : C - 1);
  const int NN = C - D;
  TORCH_CHECK(C <= 8, "gh channels capped at 8 (grad dims + hess + count)");
  TORCH_CHECK(D >= 1 && NN >= 1 && NN <= 2,
              "hist_build: channels must be D grads + 1-2 nonneg, got C=", C,
              " D=", D);
  TORCH_CHECK(max_abs.numel() == C, "max_abs must have C entries");
  TORCH_CHECK(out.numel() == (int64_t)n_nodes * F * B * C,
              "out must be [n_nodes, F, B, C]");
  TORCH_CHECK(!gh_by_position ||
                  (!identity_rows && gh.size(0) == row_idx.numel()),
              "gh_by_position: gh must have one row per row_idx entry");
  if (n_nodes == 0 || F == 0) return 0;
  const int CELLS = std::max(D, NN);

  // feature-group size by CELLS, probe-measured
  // (profiles/r01_hist_probe3): CELLS==1 -> FG=64 / 1024 threads / 128 KiB
  // LDS (1 block/CU; 64-B row slices quarter the random-row fetch
  // amplification); CELLS==2 -> FG=32 / 1024; CELLS>=3 (multiclass) ->
  // FG=16 / 512 in ~99 KiB, which keeps the vectorized uint4 row loads.
  // SEA_HIST_FG caps FG, SEA_HIST_LDS the LDS budget.
  static const int fg_env = []() {
    const char* e = getenv("SEA_HIST_FG");
    return e ? atoi(e) : 0;
  }();
  static const int lds_budget = []() {
    const char* e = getenv("SEA_HIST_LDS");
    return e ? atoi(e) : 163840;  // up to the full 160 KiB LDS per CU
  }();
  int FG = std::max<int>(1, std::min<int>(F, lds_budget / (B * CELLS * 8)));
  if (CELLS == 1 && FG >= 64 && (F % 64) == 0) FG = 64;
  else if (CELLS <= 2 && FG >= 32 && (F % 32) == 0) FG = 32;
  else if (FG >= 16) FG = 16;
  else if (FG >= 8) FG = 8;
  else if (FG >= 4) FG = 4;
  if (fg_env == 16 || fg_env == 32 || fg_env == 64)
    FG = std::min(FG, fg_env);
  const int threads =
      (FG >= 64 || (CELLS == 2 && FG >= 32)) ? 1024
      : ((FG >= 32 || (CELLS >= 3 && FG >= 16)) ? 512 : 256);
  const int n_groups = (int)ceil_div(F, FG);
  const size_t lds_bytes = (size_t)FG * B * CELLS * 8;

  HistPlan plan = plan_hist_chunks(
      node_offsets.data_ptr<int64_t>(), n_nodes,
      forest ? node_col0.data_ptr<int>() : nullptr,
      identity_rows ? bins.size(0) : row_idx.numel(), CH - C + 1, lds_bytes,
      n_groups, 2 * C);

  // full 16-aligned groups take the vectorised bin-major kernel (FG <= 64 /
  // 32 / 16 for CELLS 1 / 2 / >= 3 by the choice above, as it assumes)
  const bool bin_major =
      (FG == 16 || FG == 32 || FG == 64) && (F % FG) == 0;
  TORCH_CHECK(!bin_major || FG <= (CELLS == 1 ? 64 : (CELLS == 2 ? 32 : 16)),
              "hist_build: FG ", FG, " too wide for CELLS ", CELLS);

  // staging slot records after the chunk records: (node, first record,
  // record count, first slab); a node's slabs follow its records' order
  const int n_multi = (int)plan.multi_nodes.size();
  const size_t slots_at = plan.table.size();
  int64_t n_slabs = 0;
  for (int s = 0; s < n_multi; ++s) {
    const int rec[4] = {plan.multi_nodes[s], plan.slot_first[s],
                        plan.slot_count[s], (int)n_slabs};
    plan.table.insert(plan.table.end(), rec, rec + 4);
    n_slabs += plan.slot_count[s];
  }
  const int64_t partial_bytes = n_slabs * n_groups * (int64_t)lds_bytes;
  const bool use_partial = bin_major && CELLS == 1 /* kHistSlabFlush */ &&
                           n_multi && partial_bytes <= kHistPartialMaxBytes;

  // header: per-channel quantization scales
  auto max_abs_f = max_abs.to(torch::kFloat32).contiguous();
  auto ma = max_abs_f.accessor<float, 1>();
  float* scales_f = reinterpret_cast<float*>(plan.table.data());
  for (int c = 0; c < C; ++c)
    scales_f[c] = (float)hist_fixed_scale(plan.chunk_rows, ma[c]);
  auto chunks = h2d_async(plan.table.data(), plan.table.size() * 4,
                          kSlotHistChunks, bins.device())
                    .view(torch::kInt32);

  // multi-chunk nodes: every block's LDS image in its own slab (no fill
  // needed: each slab is written whole), or the zero-filled i64 staging the
  // atomics add into.  Integer sums either way, so histograms are bitwise
  // deterministic.
  torch::Tensor stage, partial;
  long long* stage_ptr = nullptr;
  unsigned long long* partial_ptr = nullptr;
  if (use_partial) {
    partial = torch::empty({partial_bytes / 8},
                           out.options().dtype(torch::kInt64));
    partial_ptr =
        reinterpret_cast<unsigned long long*>(partial.data_ptr<int64_t>());
  } else if (n_multi) {
    stage = torch::zeros({(int64_t)n_multi, (int64_t)F, (int64_t)B, (int64_t)C},
                         out.options().dtype(torch::kInt64));
    stage_ptr = reinterpret_cast<long long*>(stage.data_ptr<int64_t>());
  }

  auto stream = at::hip::getCurrentHIPStream();
#define HB_LAUNCH_L(DD, NNN, BM)                                             \
  do {                                                                       \
    if (lds_bytes > 65536)                                                   \
      (void)hipFuncSetAttribute(                                             \
          reinterpret_cast<const void*>(&hist_build_kernel<DD, NNN, BM>),    \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);       \
    hipLaunchKernelGGL((hist_build_kernel<DD, NNN, BM>),                     \
                       dim3(plan.n_chunks, n_groups), dim3(threads),         \
                       lds_bytes, stream, out.data_ptr<float>(), stage_ptr,  \
                       partial_ptr, bins.data_ptr<uint8_t>(),                \
                       gh.data_ptr<float>(), row_idx.data_ptr<int>(),        \
                       chunks.data_ptr<int>(), F, B, FG, CH,                 \
                       identity_rows ? 1 : 0, gh_by_position ? 1 : 0);       \
  } while (0)
#define HB_LAUNCH(DD, NNN)                                                   \
  do {                                                                       \
    if (bin_major) HB_LAUNCH_L(DD, NNN, true);                               \
    else HB_LAUNCH_L(DD, NNN, false);                                        \
  } while (0)
  const int key = D * 10 + NN;
  switch (key) {
    case 11: HB_LAUNCH(1, 1); break;
    case 12: HB_LAUNCH(1, 2); break;
    case 21: HB_LAUNCH(2, 1); break;
    case 22: HB_LAUNCH(2, 2); break;
    case 31: HB_LAUNCH(3, 1); break;
    case 32: HB_LAUNCH(3, 2); break;
    case 41: HB_LAUNCH(4, 1); break;
    case 42: HB_LAUNCH(4, 2); break;
    case 51: HB_LAUNCH(5, 1); break;
    case 52: HB_LAUNCH(5, 2); break;
    case 61: HB_LAUNCH(6, 1); break;
    case 62: HB_LAUNCH(6, 2); break;
    case 71: HB_LAUNCH(7, 1); break;
    default: TORCH_CHECK(false, "hist_build: unsupported D/NN ", D, "/", NN);
  }
#undef HB_LAUNCH
#undef HB_LAUNCH_L
  if (use_partial) {
    const int64_t lanes = (int64_t)n_groups * (FG >> 3) * ((B + 7) >> 3) * 64;
    hipLaunchKernelGGL(hist_reduce_kernel,
                       dim3((unsigned)ceil_div(lanes, 256), n_multi),
                       dim3(256), 0, stream, out.data_ptr<float>(),
                       partial_ptr, chunks.data_ptr<int>() + slots_at,
                       reinterpret_cast<const float*>(chunks.data_ptr<int>()),
                       F, B, FG, D, NN);
  } else if (n_multi) {
    auto nodes = h2d_async(plan.multi_nodes.data(), (size_t)n_multi * 4,
                           kSlotHistNodes, bins.device());
    launch_hist_decode(out.data_ptr<float>(), stage_ptr,
                       (const int*)nodes.data_ptr(),
                       reinterpret_cast<const float*>(chunks.data_ptr<int>()),
                       n_multi, (int64_t)F * B * C, C, stream);
  }
  return n_multi;
}

// ---------------------------------------------------------------------------
// partition_rows: two passes per chunk, ONE bins read.
//   pass 1: decide left/right per row, stash the decision as a ballot
//           bitmask in LDS (1 bit/row, chunk <= 64 Ki rows = 8 KiB), count
//           via popcount, ONE global atomic per block per side
//   pass 2: replay from the LDS bitmask (no second random bins gather),
//           scatter via ballot prefix + LDS block cursors
// ---------------------------------------------------------------------------

__global__ void partition_kernel(
    int* __restrict__ new_rows,        // [M]
    int* __restrict__ cursors,         // [n_nodes, 2] = {lcur, rcur}
    const uint8_t* __restrict__ bins,  // [N, F]
    const uint8_t* __restrict__ bins_t,  // [F, N] or null
    const int* __restrict__ row_idx,   // [M]
    const int* __restrict__ chunks,    // [n_chunks, 3]
    const int* __restrict__ feat,      // [n_nodes]
    const int* __restrict__ thr,       // [n_nodes]
    int F, long long Nrows) {
  __shared__ int base_l, base_r, loc_l, loc_r;
  __shared__ int wl[8];
  extern __shared__ unsigned long long bits[];  // ceil(chunk_rows/64)
  const int chunk = blockIdx.x;
  const int node = chunks[chunk * 3 + 0];
  const int start = chunks[chunk * 3 + 1];
  const int len = chunks[chunk * 3 + 2];
  const int f = feat[node];
  const int t = thr[node];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  // pass 1: decide + stash bitmask + count
  int my_l = 0;
  for (int i = threadIdx.x; i < ((len + 63) & ~63); i += blockDim.x) {
    const bool active = i < len;
    bool left = false;
    if (active) {
      const int r = row_idx[start + i];
      if (f < 0) {
        left = true;  // unsplit node: every row goes left (no load!)
      } else {
        // the transposed matrix turns the per-row gather (1 useful byte
        // per 64-B line with the row-major layout) into a locally-dense
        // read: a node's rows at level L are ~2^-L dense in [0, N), so
        // a line yields ~64/2^L useful bytes at shallow levels
        const uint8_t bv = bins_t ? bins_t[(int64_t)f * Nrows + r]
                                  : bins[(int64_t)r * F + f];
        left = bv <= t;
      }
    }
    const unsigned long long m = __ballot(active && left);
    if (lane == 0) {
      bits[i >> 6] = m;
      my_l += (int)__popcll(m);
    }
  }
  if (lane == 0) wl[wave] = my_l;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w0 = 0; w0 < (int)(blockDim.x / 64); ++w0) tot += wl[w0];
    base_l = atomicAdd(cursors + node * 2 + 0, tot);
    base_r = atomicAdd(cursors + node * 2 + 1, -(len - tot)) - (len - tot);
    loc_l = 0;
    loc_r = 0;
  }
  __syncthreads();

  // pass 2: scatter from the stashed decisions (row_idx re-read is
  // sequential; bins is NOT touched again)
  for (int i = threadIdx.x; i < ((len + 63) & ~63); i += blockDim.x) {
    const bool active = i < len;
    const unsigned long long word = bits[i >> 6];
    const bool left = (word >> lane) & 1ull;
    const unsigned long long lmask = word;
    const unsigned long long rmask = __ballot(active) & ~word;
    int lbase = 0, rbase = 0;
    if (lane == 0) {
      lbase = atomicAdd(&loc_l, (int)__popcll(lmask));
      rbase = atomicAdd(&loc_r, (int)__popcll(rmask));
    }
    lbase = __shfl(lbase, 0, 64);
    rbase = __shfl(rbase, 0, 64);
    if (active) {
      const int r = row_idx[start + i];
      if (left) {
        const int pos = base_l + lbase + (int)__popcll(lmask & ((1ull << lane) - 1ull));
        new_rows[pos] = r;
      } else {
        const int pos = base_r + rbase + (int)__popcll(rmask & ((1ull << lane) - 1ull));
        new_rows[pos] = r;
      }
    }
  }
}

// Queues the partition of every node and returns the device cursor table
// [n_nodes, 2] = {lcur, rcur}: once the kernel has run, lcur - offs[node] is
// the node's left count.
static torch::Tensor partition_launch(torch::Tensor new_rows,
                                      torch::Tensor bins, torch::Tensor bins_t,
                                      torch::Tensor row_idx,
                                      torch::Tensor node_offsets,
                                      torch::Tensor feat, torch::Tensor thr) {
  auto tpA = std::chrono::steady_clock::now();
  CHECK_GPU(new_rows); CHECK_GPU(bins); CHECK_GPU(row_idx);
  CHECK_GPU(feat); CHECK_GPU(thr);
  const int F = (int)bins.size(1);
  const int n_nodes = (int)node_offsets.numel() - 1;
  auto offs = node_offsets.accessor<int64_t, 1>();

  std::vector<int> cur_v(n_nodes * 2);
  std::vector<int> chunk_v;
  int64_t total_rows = offs[n_nodes];
  int64_t chunk_rows =
      std::max<int64_t>(8192, ceil_div(total_rows, (int64_t)2048));
  chunk_rows = std::min<int64_t>(chunk_rows, 65536);  // 8 KiB LDS bitmask
  for (int nd = 0; nd < n_nodes; ++nd) {
    cur_v[nd * 2 + 0] = (int)offs[nd];
    cur_v[nd * 2 + 1] = (int)offs[nd + 1];
    for (int64_t c = offs[nd]; c < offs[nd + 1]; c += chunk_rows) {
      chunk_v.push_back(nd);
      chunk_v.push_back((int)c);
      chunk_v.push_back((int)std::min<int64_t>(chunk_rows, offs[nd + 1] - c));
    }
  }
  auto stream = at::hip::getCurrentHIPStream();
  static const bool part_dbg = getenv("SEA_PART_DEBUG") != nullptr;
  auto tp0 = std::chrono::steady_clock::now();
  auto cursors_b = h2d_async(cur_v.data(), cur_v.size() * 4,
                             kSlotPartCursors, bins.device());
  auto cursors = cursors_b.view(torch::kInt32);
  auto tp1 = std::chrono::steady_clock::now();
  if (!chunk_v.empty()) {
    auto chunks_b = h2d_async(chunk_v.data(), chunk_v.size() * 4, kSlotPartChunks,
                              bins.device());
    auto chunks = chunks_b.view(torch::kInt32);
    auto tp2 = std::chrono::steady_clock::now();
    const int n_chunks = (int)(chunk_v.size() / 3);
    const size_t bit_lds = (size_t)((chunk_rows + 63) / 64) * 8;
    const uint8_t* bt_ptr =
        bins_t.defined() && bins_t.numel() ? bins_t.data_ptr<uint8_t>()
                                           : nullptr;
    hipLaunchKernelGGL(partition_kernel, dim3(n_chunks), dim3(256), bit_lds,
                       stream,
                       new_rows.data_ptr<int>(), cursors.data_ptr<int>(),
                       bins.data_ptr<uint8_t>(), bt_ptr,
                       row_idx.data_ptr<int>(),
                       chunks.data_ptr<int>(), feat.data_ptr<int>(),
                       thr.data_ptr<int>(), F, (long long)bins.size(0));
    if (part_dbg) {
      auto tp3 = std::chrono::steady_clock::now();
      auto us = [](auto a, auto b) {
        return std::chrono::duration_cast<std::chrono::microseconds>(b - a)
            .count();
      };
      fprintf(stderr,
              "[part c++] entry=%ldus cursors=%ldus chunks=%ldus launch=%ldus\n",
              (long)us(tpA, tp0), (long)us(tp0, tp1), (long)us(tp1, tp2),
              (long)us(tp2, tp3));
    }
  }
  return cursors.view({n_nodes, 2});
}

void partition_rows(torch::Tensor new_rows, torch::Tensor left_counts,
                    torch::Tensor bins, torch::Tensor bins_t,
                    torch::Tensor row_idx,
                    torch::Tensor node_offsets, torch::Tensor feat,
                    torch::Tensor thr) {
  CHECK_GPU(left_counts);
  auto cursors = partition_launch(new_rows, bins, bins_t, row_idx,
                                  node_offsets, feat, thr);
  const int n_nodes = (int)node_offsets.numel() - 1;
  auto offs = node_offsets.accessor<int64_t, 1>();
  auto lcur = cursors.select(1, 0);
  // NOTE: this upload was a pageable .to(device) — a SYNCHRONOUS copy that
  // stalled the host ~1 ms/level behind the queued hist/split kernels
  // (found via SEA_PART_DEBUG bracketing); pinned async staging fixes it
  std::vector<int> seg_v(n_nodes);
  for (int nd = 0; nd < n_nodes; ++nd) seg_v[nd] = (int)offs[nd];
  auto seg_b = h2d_async(seg_v.data(), seg_v.size() * 4, kSlotPartSegStart,
                         bins.device());
  auto seg_start = seg_b.view(torch::kInt32);
  left_counts.copy_(lcur - seg_start);
}

// partition_rows without the device bookkeeping: feat / thr are the int32
// device tensors of level_split, and the cursor table itself is returned for
// the caller to copy to the host, where left = lcur - segment start.
torch::Tensor partition_rows_cursors(torch::Tensor new_rows,
                                     torch::Tensor bins, torch::Tensor bins_t,
                                     torch::Tensor row_idx,
                                     torch::Tensor node_offsets,
                                     torch::Tensor feat, torch::Tensor thr) {
  CHECK_CONTIG(new_rows); CHECK_CONTIG(row_idx); CHECK_CONTIG(feat);
  CHECK_CONTIG(thr);
  const int64_t n_nodes = node_offsets.numel() - 1;
  TORCH_CHECK(feat.scalar_type() == torch::kInt32 &&
                  thr.scalar_type() == torch::kInt32 &&
                  feat.numel() == n_nodes && thr.numel() == n_nodes,
              "partition_rows_cursors: feat and thr are int32 [n_nodes]");
  TORCH_CHECK(new_rows.numel() == row_idx.numel(),
              "partition_rows_cursors: new_rows must match row_idx");
  return partition_launch(new_rows, bins, bins_t, row_idx, node_offsets, feat,
                          thr);
}

// ---------------------------------------------------------------------------
// tree walks
// ---------------------------------------------------------------------------

__global__ void tree_predict_kernel(float* __restrict__ out,       // [N, D]
                                    const float* __restrict__ x,   // [N, F]
                                    const int* __restrict__ feat,  // [nodes]
                                    const float* __restrict__ thr,
                                    const int* __restrict__ left,
                                    const float* __restrict__ leaf,  // [nodes, D]
                                    int64_t n, int F, int D) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    const float* xr = x + i * F;
    int node = 0;
    int f = feat[0];
    while (f >= 0) {
      node = left[node] + (xr[f] <= thr[node] ? 0 : 1);
      f = feat[node];
    }
    const float* lv = leaf + (int64_t)node * D;
    float* o = out + i * D;
    for (int d = 0; d < D; ++d) o[d] = lv[d];
  }
}

void tree_predict(torch::Tensor out, torch::Tensor x, torch::Tensor feat,
                  torch::Tensor thr, torch::Tensor left, torch::Tensor leaf) {
  CHECK_GPU(out); CHECK_GPU(x);
  int64_t n = x.size(0);
  int F = (int)x.size(1);
  int D = (int)leaf.size(1);
  auto stream = at::hip::getCurrentHIPStream();
  int blocks = (int)std::min<int64_t>(ceil_div(n, 256), 16384);
  hipLaunchKernelGGL(tree_predict_kernel, dim3(blocks), dim3(256), 0, stream,
                     out.data_ptr<float>(), x.data_ptr<float>(),
                     feat.data_ptr<int>(), thr.data_ptr<float>(),
                     left.data_ptr<int>(), leaf.data_ptr<float>(), n, F, D);
}

__global__ void forest_predict_kernel(
    float* __restrict__ out,           // [N, D] (+=)
    const float* __restrict__ x,       // [N, F]
    const int* __restrict__ feat,      // concat nodes
    const float* __restrict__ thr,
    const int* __restrict__ left,
    const float* __restrict__ leaf,    // concat [nodes, D]
    const int* __restrict__ tree_off,  // [T]
    const float* __restrict__ w,       // [T]
    int64_t n, int F, int D, int T) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    const float* xr = x + i * F;
    float* o = out + i * D;
    for (int t = 0; t < T; ++t) {
      const int base = tree_off[t];
      int node = base;
      int f = feat[node];
      while (f >= 0) {
        node = base + left[node] + (xr[f] <= thr[node] ? 0 : 1);
        f = feat[node];
      }
      const float* lv = leaf + (int64_t)node * D;
      const float wt = w[t];
      for (int d = 0; d < D; ++d) o[d] += wt * lv[d];
    }
  }
}

void forest_predict(torch::Tensor out, torch::Tensor x, torch::Tensor feat,
                    torch::Tensor thr, torch::Tensor left, torch::Tensor leaf,
                    torch::Tensor tree_off, torch::Tensor w, int64_t D) {
  CHECK_GPU(out); CHECK_GPU(x);
  int64_t n = x.size(0);
  int F = (int)x.size(1);
  int T = (int)tree_off.numel();
  auto stream = at::hip::getCurrentHIPStream();
  int blocks = (int)std::min<int64_t>(ceil_div(n, 256), 16384);
  hipLaunchKernelGGL(forest_predict_kernel, dim3(blocks), dim3(256), 0, stream,
                     out.data_ptr<float>(), x.data_ptr<float>(),
                     feat.data_ptr<int>(), thr.data_ptr<float>(),
                     left.data_ptr<int>(), leaf.data_ptr<float>(),
                     tree_off.data_ptr<int>(), w.data_ptr<float>(), n, F,
                     (int)D, T);
}

// ---------------------------------------------------------------------------
// forest_predict2: LDS-staged tree-group-tiled forest inference.
//
//   The v1 kernel above walks ALL T trees per row with every node fetch a
//   dependent global load (L1-thrashing: 64 lanes x ~800 scattered node +
//   feature reads) — measured 72.7M rows/s for a 100-tree depth-8 forest
//   (docs/performance.md r01).  v2 restructures serving the MI355X way:
//
//   * nodes are packed host-side into ONE u64 per node:
//       low 16  = feature (s16, -1 leaf)   | mid 16 = left-child (s16,
//       sibling right = left+1)            | high 32 = f32 bits of the
//       threshold — or, for D == 1, the WEIGHTED leaf value when feat < 0
//       (leaf tensors never touched in-kernel for scalar outputs).
//   * trees are tiled into groups of <= 16 Ki nodes (128 KiB); each block
//     stages its group's packed nodes in LDS once (ds_read_b64 is 256
//     B/clk/CU vs ~200-900 cyc global latency per dependent node hop),
//     then grid-strides over rows: per (row, group) all walks hit LDS.
//   * one f32 atomicAdd per (row, channel, group) merges group partials —
//     different rows never contend.
//
//   grid (row_chunks, n_groups) x 1024 threads; 1 block/CU at 128 KiB LDS
//   = 16 waves covering the ds_read dependent-latency chain.
//   Reference semantics: the model transform loops at reference
//   BaggingRegressor.scala:221-228, GBMClassifier.scala:567-589.
// ---------------------------------------------------------------------------

// BINNED == false: x is [N, F] f32, payload high-32 = f32 threshold bits.
// BINNED == true:  x is u8 rank-transformed rows (each feature value
//   replaced by its lower-bound rank within the forest's OWN sorted
//   per-feature threshold set — an EXACT transform: x <= thr  <=>
//   rank(x) <= rank(thr)), payload high-32 = the threshold's rank.
//   Rows shrink 4x (u8 vs f32), so the divergent per-lane gathers stop
//   thrashing L1 (256 B rows: 4 cache lines instead of 16).
//   xt != 0: the u8 matrix is TRANSPOSED [F, N] — consecutive lanes hold
//   consecutive rows, and all lanes of a wave sit on the SAME node for
//   the first tree levels (they entered the tree together), so their
//   gathers land on consecutive bytes of one feature column: hop h costs
//   <= min(2^h, 64) cache lines instead of 64.
template <bool D1, bool BINNED>
__global__ void forest_predict2_kernel(
    float* __restrict__ out,                       // [N, D] (+=, pre-zeroed)
    const void* __restrict__ xv_,                  // [N, F] f32 | u8
    const unsigned long long* __restrict__ nodes,  // [total] packed
    const float* __restrict__ leaf,                // [total, D] (D > 1)
    const int* __restrict__ tree_off,              // [T] global node base
    const float* __restrict__ w,                   // [T]
    const int* __restrict__ groups,                // [G, 4]
    int64_t n, int F, int D, int xt) {
  extern __shared__ unsigned long long tlds[];  // group nodes
  const int* grp = groups + blockIdx.y * 4;
  const int first_tree = grp[0];
  const int n_trees = grp[1];
  const int node_base = grp[2];
  const int n_nodes = grp[3];
  for (int i = threadIdx.x; i < n_nodes; i += blockDim.x)
    tlds[i] = nodes[node_base + i];
  __syncthreads();

  // one row per lane: a 2-row-per-lane ILP variant was measured 1.5-4x
  // SLOWER (merged divergent walk loops serialize both chains through
  // every iteration); wave-level parallelism already covers the latency
  int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; r < n; r += stride) {
    const float* xr = BINNED ? nullptr : (const float*)xv_ + r * F;
    const uint8_t* br =
        BINNED ? (const uint8_t*)xv_ + (xt ? r : r * F) : nullptr;
    // transposed stride: br[f * n] addresses feature f of this row
    float acc[8];
    if (!D1)
#pragma unroll
      for (int d = 0; d < 8; ++d) acc[d] = 0.0f;
    float acc1 = 0.0f;
    for (int t = 0; t < n_trees; ++t) {
      const int toff = tree_off[first_tree + t] - node_base;
      int node = toff;
      unsigned long long nd = tlds[node];
      int f = (short)(nd & 0xFFFFu);
      while (f >= 0) {
        const int left = (short)((nd >> 16) & 0xFFFFu);
        bool go_left;
        if (BINNED) {
          const uint8_t bv = xt ? br[(int64_t)f * n] : br[f];
          go_left = bv <= (unsigned)(nd >> 32);
        } else {
          go_left = xr[f] <= __uint_as_float((unsigned)(nd >> 32));
        }
        node = toff + left + (go_left ? 0 : 1);
        nd = tlds[node];
        f = (short)(nd & 0xFFFFu);
      }
      if (D1) {
        acc1 += __uint_as_float((unsigned)(nd >> 32));  // weighted leaf
      } else {
        const float wt = w[first_tree + t];
        const float* lv = leaf + (int64_t)(node_base + node) * D;
        for (int d = 0; d < D; ++d) acc[d] += wt * lv[d];
      }
    }
    if (D1) {
      atomicAdd(out + r, acc1);
    } else {
      float* o = out + r * D;
      for (int d = 0; d < D; ++d)
        if (acc[d] != 0.0f) atomicAdd(o + d, acc[d]);
    }
  }
}

// ---------------------------------------------------------------------------
// transpose_u8: [N, F] u8 -> [F, N] u8 for the transposed serving walk.
// torch's generic u8 2D transpose measured 19 ms at 10M x 256 (~26x off
// bandwidth); this is a 64x64 LDS-tiled transpose moving u32 quads on
// both sides (full tiles) — byte path only on edge tiles.
// ---------------------------------------------------------------------------
// gather_ranges / leaf_scatter: the forest grower's per-level row-arena
// maintenance.  Both replace a 3-kernel torch expansion
// (repeat_interleave + cumsum + arange gather — the reference's per-node
// driver loops have no on-GPU analog) with ONE pass:
// each output position binary-searches the tiny per-segment prefix table
// (L2-resident) and streams contiguous source ranges.
// ---------------------------------------------------------------------------

__device__ inline int seg_of(const long long* __restrict__ cum, int n_segs,
                             long long p) {
  int lo = 0, hi = n_segs;  // cum[0] = 0, cum[n_segs] = total
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void gather_ranges_kernel(
    int* __restrict__ out,               // [total]
    const int* __restrict__ src,
    const long long* __restrict__ seg,   // [n_segs+1 cum..., n_segs starts...]
    int n_segs, long long total) {
  const long long* cum = seg;
  const long long* starts = seg + n_segs + 1;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       p < total; p += stride) {
    const int s = seg_of(cum, n_segs, p);
    out[p] = src[starts[s] + (p - cum[s])];
  }
}

// gather_ranges that also brings the rows' gradients along: gh_out[p, :] =
// gh[out[p], col0[s] : col0[s] + C] for position p of range s, so the
// histogram kernel streams gh by position instead of gathering it once per
// feature group
__global__ void gather_ranges_gh_kernel(
    int* __restrict__ out,               // [total]
    float* __restrict__ gh_out,          // [total, C]
    const int* __restrict__ src,
    const float* __restrict__ gh,        // [N, CH]
    const long long* __restrict__ seg,   // [cum n_segs+1, starts, col0]
    int n_segs, long long total, int C, int CH) {
  const long long* cum = seg;
  const long long* starts = seg + n_segs + 1;
  const long long* col0 = starts + n_segs;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       p < total; p += stride) {
    const int s = seg_of(cum, n_segs, p);
    const int r = src[starts[s] + (p - cum[s])];
    out[p] = r;
    const float* g = gh + (long long)r * CH + col0[s];
    for (int c = 0; c < C; ++c) gh_out[p * C + c] = g[c];
  }
}

__global__ void leaf_scatter_kernel(
    float* __restrict__ tp,              // [N, T] row-major
    const int* __restrict__ row_idx,     // level row arena
    const long long* __restrict__ seg,   // [n_segs+1 cum..., n_segs starts...]
    const int* __restrict__ tree,        // [n_segs]
    const float* __restrict__ val,       // [n_segs]
    int T, int n_segs, long long total) {
  const long long* cum = seg;
  const long long* starts = seg + n_segs + 1;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       p < total; p += stride) {
    const int s = seg_of(cum, n_segs, p);
    const int r = row_idx[starts[s] + (p - cum[s])];
    tp[(long long)r * T + tree[s]] = val[s];
  }
}

void gather_ranges(torch::Tensor out, torch::Tensor src,
                   torch::Tensor starts, torch::Tensor lens) {
  CHECK_GPU(out); CHECK_GPU(src);
  const int n_segs = (int)starts.numel();
  const long long total = out.numel();
  if (n_segs == 0 || total == 0) return;
  auto st = starts.accessor<int64_t, 1>();
  auto ln = lens.accessor<int64_t, 1>();
  std::vector<long long> seg_v(2 * n_segs + 1);
  seg_v[0] = 0;
  for (int i = 0; i < n_segs; ++i) {
    seg_v[i + 1] = seg_v[i] + ln[i];
    seg_v[n_segs + 1 + i] = st[i];
  }
  TORCH_CHECK(seg_v[n_segs] == total, "gather_ranges: lens sum != out size");
  auto seg_b = h2d_async(seg_v.data(), seg_v.size() * 8, kSlotGatherSegs,
                         src.device());
  auto stream = at::hip::getCurrentHIPStream();
  const int blocks =
      (int)std::min<long long>(8192, ceil_div(total, (long long)1024));
  hipLaunchKernelGGL(gather_ranges_kernel, dim3(blocks), dim3(256), 0, stream,
                     out.data_ptr<int>(), src.data_ptr<int>(),
                     (const long long*)seg_b.data_ptr(), n_segs, total);
}

// src rows are trusted like hist_build's row_idx; the column window
// [col0, col0 + C) of every range is checked against gh's width here
void gather_ranges_gh(torch::Tensor out, torch::Tensor gh_out,
                      torch::Tensor src, torch::Tensor gh,
                      torch::Tensor starts, torch::Tensor lens,
                      torch::Tensor col0) {
  CHECK_GPU(out); CHECK_GPU(gh_out); CHECK_GPU(src); CHECK_GPU(gh);
  CHECK_CONTIG(out); CHECK_CONTIG(gh_out); CHECK_CONTIG(src); CHECK_CONTIG(gh);
  TORCH_CHECK(gh.dim() == 2 && gh_out.dim() == 2 &&
                  gh_out.size(0) == out.numel(),
              "gather_ranges_gh: gh_out must be [out.numel(), C]");
  const int n_segs = (int)starts.numel();
  const long long total = out.numel();
  const int C = (int)gh_out.size(1), CH = (int)gh.size(1);
  TORCH_CHECK(lens.numel() == n_segs && col0.numel() == n_segs,
              "gather_ranges_gh: one len and col0 per range");
  if (n_segs == 0 || total == 0) return;
  auto st = starts.accessor<int64_t, 1>();
  auto ln = lens.accessor<int64_t, 1>();
  auto c0 = col0.accessor<int64_t, 1>();
  std::vector<long long> seg_v(3 * n_segs + 1);
  seg_v[0] = 0;
  for (int i = 0; i < n_segs; ++i) {
    TORCH_CHECK(ln[i] >= 0 && st[i] >= 0 && st[i] + ln[i] <= src.numel(),
                "gather_ranges_gh: range outside src");
    TORCH_CHECK(c0[i] >= 0 && c0[i] + C <= CH,
                "gather_ranges_gh: col0 outside gh");
    seg_v[i + 1] = seg_v[i] + ln[i];
    seg_v[n_segs + 1 + i] = st[i];
    seg_v[2 * n_segs + 1 + i] = c0[i];
  }
  TORCH_CHECK(seg_v[n_segs] == total,
              "gather_ranges_gh: lens sum != out size");
  auto seg_b = h2d_async(seg_v.data(), seg_v.size() * 8, kSlotGatherSegs,
                         src.device());
  auto stream = at::hip::getCurrentHIPStream();
  const int blocks =
      (int)std::min<long long>(8192, ceil_div(total, (long long)1024));
  hipLaunchKernelGGL(gather_ranges_gh_kernel, dim3(blocks), dim3(256), 0,
                     stream, out.data_ptr<int>(), gh_out.data_ptr<float>(),
                     src.data_ptr<int>(), gh.data_ptr<float>(),
                     (const long long*)seg_b.data_ptr(), n_segs, total, C, CH);
}

void leaf_scatter(torch::Tensor tp, torch::Tensor row_idx,
                  torch::Tensor starts, torch::Tensor lens,
                  torch::Tensor tree, torch::Tensor val) {
  CHECK_GPU(tp); CHECK_GPU(row_idx);
  const int n_segs = (int)starts.numel();
  if (n_segs == 0) return;
  const int T = (int)tp.size(1);
  auto st = starts.accessor<int64_t, 1>();
  auto ln = lens.accessor<int64_t, 1>();
  std::vector<long long> seg_v(2 * n_segs + 1);
  seg_v[0] = 0;
  for (int i = 0; i < n_segs; ++i) {
    seg_v[i + 1] = seg_v[i] + ln[i];
    seg_v[n_segs + 1 + i] = st[i];
  }
  const long long total = seg_v[n_segs];
  if (total == 0) return;
  auto seg_b = h2d_async(seg_v.data(), seg_v.size() * 8, kSlotLeafSegs,
                         tp.device());
  std::vector<int> tv(n_segs);
  std::vector<float> vv(n_segs);
  auto ta = tree.accessor<int64_t, 1>();
  auto va = val.accessor<float, 1>();
  for (int i = 0; i < n_segs; ++i) { tv[i] = (int)ta[i]; vv[i] = va[i]; }
  auto tree_b = h2d_async(tv.data(), tv.size() * 4, kSlotLeafTree, tp.device());
  std::vector<char> vb(n_segs * 4);
  std::memcpy(vb.data(), vv.data(), n_segs * 4);
  auto val_b = h2d_async(vb.data(), vb.size(), kSlotLeafVal, tp.device());
  auto stream = at::hip::getCurrentHIPStream();
  const int blocks =
      (int)std::min<long long>(8192, ceil_div(total, (long long)1024));
  hipLaunchKernelGGL(leaf_scatter_kernel, dim3(blocks), dim3(256), 0, stream,
                     tp.data_ptr<float>(), row_idx.data_ptr<int>(),
                     (const long long*)seg_b.data_ptr(),
                     (const int*)tree_b.data_ptr(),
                     (const float*)val_b.data_ptr(), T, n_segs, total);
}

// ---------------------------------------------------------------------------

__global__ void transpose_u8_kernel(uint8_t* __restrict__ out,  // [F, N]
                                    const uint8_t* __restrict__ in,  // [N, F]
                                    int64_t n, int F) {
  __shared__ uint8_t tile[64][68];  // row stride 68 = 4*17: aligned, unbanked
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int f0 = blockIdx.y * 64;
  const int tid = threadIdx.x;  // 256 threads
  const bool full = (r0 + 64 <= n) && (f0 + 64 <= F) && ((F & 3) == 0) &&
                    ((n & 3) == 0);
  if (full) {
    for (int i = tid; i < 1024; i += 256) {
      const int rr = i >> 4;
      const int cq = i & 15;
      const unsigned v = *reinterpret_cast<const unsigned*>(
          in + (r0 + rr) * F + f0 + cq * 4);
      *reinterpret_cast<unsigned*>(&tile[rr][cq * 4]) = v;
    }
    __syncthreads();
    for (int i = tid; i < 1024; i += 256) {
      const int ff = i >> 4;
      const int rq = i & 15;
      const unsigned v =
          (unsigned)tile[rq * 4 + 0][ff] |
          ((unsigned)tile[rq * 4 + 1][ff] << 8) |
          ((unsigned)tile[rq * 4 + 2][ff] << 16) |
          ((unsigned)tile[rq * 4 + 3][ff] << 24);
      *reinterpret_cast<unsigned*>(out + (int64_t)(f0 + ff) * n + r0 +
                                   rq * 4) = v;
    }
  } else {
    for (int i = tid; i < 4096; i += 256) {
      const int rr = i >> 6;
      const int ff = i & 63;
      if (r0 + rr < n && f0 + ff < F)
        tile[rr][ff] = in[(r0 + rr) * F + f0 + ff];
    }
    __syncthreads();
    for (int i = tid; i < 4096; i += 256) {
      const int ff = i >> 6;
      const int rr = i & 63;
      if (r0 + rr < n && f0 + ff < F)
        out[(int64_t)(f0 + ff) * n + r0 + rr] = tile[rr][ff];
    }
  }
}

void transpose_u8(torch::Tensor out, torch::Tensor in) {
  CHECK_GPU(out); CHECK_GPU(in);
  CHECK_CONTIG(out); CHECK_CONTIG(in);
  TORCH_CHECK(in.scalar_type() == torch::kUInt8, "u8 only");
  const int64_t n = in.size(0);
  const int F = (int)in.size(1);
  TORCH_CHECK(out.size(0) == F && out.size(1) == n, "shape mismatch");
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(transpose_u8_kernel,
                     dim3((unsigned)ceil_div(n, 64), (unsigned)ceil_div(F, 64)),
                     dim3(256), 0, stream, out.data_ptr<uint8_t>(),
                     in.data_ptr<uint8_t>(), n, F);
}

void forest_predict2(torch::Tensor out, torch::Tensor x, torch::Tensor nodes,
                     torch::Tensor leaf, torch::Tensor tree_off,
                     torch::Tensor w, torch::Tensor groups, int64_t D,
                     int64_t max_group_nodes, int64_t x_transposed) {
  CHECK_GPU(out); CHECK_GPU(x); CHECK_GPU(nodes); CHECK_GPU(groups);
  CHECK_CONTIG(out); CHECK_CONTIG(x); CHECK_CONTIG(nodes);
  TORCH_CHECK(D <= 8, "forest_predict2: D <= 8");
  const bool binned = x.scalar_type() == torch::kUInt8;
  TORCH_CHECK(!x_transposed || binned, "x_transposed implies u8 input");
  int64_t n = x.size(x_transposed ? 1 : 0);
  int F = (int)x.size(x_transposed ? 0 : 1);
  const int G = (int)groups.size(0);
  const size_t lds = (size_t)max_group_nodes * 8;
  TORCH_CHECK(lds <= 163840, "forest_predict2: group too big for LDS");
  auto stream = at::hip::getCurrentHIPStream();
  const int threads = 1024;
  int rblocks = (int)std::min<int64_t>(ceil_div(n, threads), 8192);
  // fill the chip even for few groups
  rblocks = std::max(rblocks, (int)std::min<int64_t>(
                                  ceil_div(512, (int64_t)G), ceil_div(n, 64)));
#define FP2_LAUNCH(DD1, BB)                                                   \
  do {                                                                        \
    if (lds > 65536)                                                          \
      (void)hipFuncSetAttribute(                                              \
          reinterpret_cast<const void*>(&forest_predict2_kernel<DD1, BB>),    \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);              \
    hipLaunchKernelGGL((forest_predict2_kernel<DD1, BB>), dim3(rblocks, G),   \
                       dim3(threads), lds, stream, out.data_ptr<float>(),     \
                       x.data_ptr(),                                          \
                       (const unsigned long long*)nodes.data_ptr<int64_t>(),  \
                       leaf.numel() ? leaf.data_ptr<float>() : nullptr,       \
                       tree_off.data_ptr<int>(), w.data_ptr<float>(),         \
                       groups.data_ptr<int>(), n, F, (int)D,                  \
                       (int)x_transposed);                                    \
  } while (0)
  if (D == 1 && binned) FP2_LAUNCH(true, true);
  else if (D == 1) FP2_LAUNCH(true, false);
  else if (binned) FP2_LAUNCH(false, true);
  else FP2_LAUNCH(false, false);
#undef FP2_LAUNCH
}

// ---------------------------------------------------------------------------
// fused GBM loss kernels
//   loss ids match spark_ensemble_amd/boosting/losses.py LOSS_IDS; the
//   per-row device forms live in csrc/gbm_loss.h
// ---------------------------------------------------------------------------

// grad_hess: per-row fused pseudo-residual inputs.
//   dim == 1 scalar losses, or logloss with dim = K (softmax).
__global__ void grad_hess_kernel(float* __restrict__ grad,  // [N, D]
                                 float* __restrict__ hess,  // [N, D] or null
                                 const float* __restrict__ label,  // [N, D]
                                 const float* __restrict__ pred,   // [N, D]
                                 int64_t n, int D, int loss_id, float param,
                                 int want_hess) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (; i < n; i += stride) {
    if (loss_id == L_LOGLOSS) {
      // two passes over d; no local arrays (rule: runtime-indexed locals
      // become register-select chains or scratch)
      const float* pr = pred + i * D;
      const float* lr = label + i * D;
      float m = pr[0];
      for (int d = 1; d < D; ++d) m = fmaxf(m, pr[d]);
      float s = 0.0f;
      for (int d = 0; d < D; ++d) s += __expf(pr[d] - m);
      float inv = 1.0f / s;
      for (int d = 0; d < D; ++d) {
        float q = __expf(pr[d] - m) * inv;
        grad[i * D + d] = q - lr[d];
        if (want_hess) hess[i * D + d] = q * (1.0f - q);
      }
    } else {
      float g, h;
      scalar_loss_grad(loss_id, param, label[i], pred[i], &g, &h);
      grad[i] = g;
      if (want_hess) hess[i] = h;
    }
  }
}

void grad_hess(torch::Tensor grad, torch::Tensor hess, torch::Tensor label,
               torch::Tensor pred, int64_t loss_id, double param,
               bool want_hess) {
  CHECK_GPU(grad); CHECK_GPU(label); CHECK_GPU(pred);
  int64_t n = pred.size(0);
  int D = (int)pred.size(1);
  auto stream = at::hip::getCurrentHIPStream();
  int blocks = (int)std::min<int64_t>(ceil_div(n, 256), 16384);
  hipLaunchKernelGGL(grad_hess_kernel, dim3(blocks), dim3(256), 0, stream,
                     grad.data_ptr<float>(),
                     want_hess ? hess.data_ptr<float>() : nullptr,
                     label.data_ptr<float>(), pred.data_ptr<float>(), n, D,
                     (int)loss_id, (float)param, want_hess ? 1 : 0);
}

// line_search_eval: one pass computing
//   payload[0]   = sum_i w_i * loss(y_i, p_i + a . d_i)
//   payload[1+d] = sum_i w_i * d_id * dloss/dp_id
//   payload[1+D] = sum_i w_i * d_i^2 * d2loss/dp_i^2   (want_hess, D == 1;
//                  feeds the safeguarded-Newton stage-weight search)
template <int D>
__global__ void line_search_eval_kernel(
    float* __restrict__ payload,        // [1 + D (+1)] (pre-zeroed)
    const float* __restrict__ label,    // [N, D]
    const float* __restrict__ pred,     // [N, D]
    const float* __restrict__ dir,      // [N, D]
    const float* __restrict__ weight,   // [N]
    const float* __restrict__ coeff,    // [D]
    int64_t n, int loss_id, float param, int want_hess) {
  __shared__ float wacc[4][2 + D];  // per-wave partials (256 threads = 4 waves)
  __syncthreads();

  float cf[D];
#pragma unroll
  for (int d = 0; d < D; ++d) cf[d] = coeff[d];

  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int64_t stride = gridDim.x * (int64_t)blockDim.x;
  float loss_sum = 0.0f;
  float hsum = 0.0f;
  float gsum[D];
#pragma unroll
  for (int d = 0; d < D; ++d) gsum[d] = 0.0f;

  for (; i < n; i += stride) {
    const float w = weight[i];
    if (D > 1 || loss_id == L_LOGLOSS) {
      const float* pr = pred + i * D;
      const float* dr = dir + i * D;
      const float* lr = label + i * D;
      float pv[D];
      float m = -1e30f;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        pv[d] = pr[d] + cf[d] * dr[d];
        m = fmaxf(m, pv[d]);
      }
      float s = 0.0f;
#pragma unroll
      for (int d = 0; d < D; ++d) s += __expf(pv[d] - m);
      float lse = m + __logf(s);
      float l = 0.0f;
      float inv = 1.0f / s;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        l += -lr[d] * (pv[d] - lse);
        float q = __expf(pv[d] - m) * inv;
        gsum[d] += w * dr[d] * (q - lr[d]);
      }
      loss_sum += w * l;
    } else {
      float g, h;
      float l = scalar_loss_grad(loss_id, param, label[i],
                                 pred[i] + cf[0] * dir[i], &g, &h);
      if (!isfinite(l)) l = 3.0e38f;
      loss_sum += w * l;
      gsum[0] += w * dir[i] * g;
      if (want_hess) hsum += w * dir[i] * dir[i] * h;
    }
  }

  // wave reduce then LDS
  for (int off = 32; off > 0; off >>= 1) {
    loss_sum += __shfl_down(loss_sum, off, 64);
    hsum += __shfl_down(hsum, off, 64);
#pragma unroll
    for (int d = 0; d < D; ++d) gsum[d] += __shfl_down(gsum[d], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    const int wv = threadIdx.x >> 6;
    wacc[wv][0] = loss_sum;
    wacc[wv][1 + D] = hsum;
#pragma unroll
    for (int d = 0; d < D; ++d) wacc[wv][1 + d] = gsum[d];
  }
  __syncthreads();
  // per-block partial, waves summed in FIXED order (no atomics anywhere)
  // -> bitwise deterministic; final fixed-order reduction in
  // ls_reduce_kernel
  if (threadIdx.x == 0) {
    float* row = payload + (int64_t)blockIdx.x * (2 + D);
    const int nw = (int)(blockDim.x >> 6);
    for (int k = 0; k < 2 + D; ++k) {
      float v = 0.0f;
      for (int wv = 0; wv < nw; ++wv) v += wacc[wv][k];
      row[k] = v;
    }
  }
}

// sum the [n_blocks, stride] partials with a FIXED thread->block
// assignment (grid of one block; lane j sums rows j, j+J, ... then lane 0
// of each slot adds the J lane-partials in order => bitwise deterministic)
__global__ void ls_reduce_kernel(float* __restrict__ out,      // [out_width]
                                 const float* __restrict__ partials,
                                 int n_blocks, int stride, int out_width) {
  __shared__ float lp[256];
  const int k = threadIdx.x % stride;        // payload slot
  const int j = threadIdx.x / stride;        // lane within slot
  const int J = blockDim.x / stride;         // lanes per slot
  float s = 0.0f;
  if (j < J) {
    for (int b = j; b < n_blocks; b += J)
      s += partials[(int64_t)b * stride + k];
  }
  lp[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < out_width) {
    float v = 0.0f;
    for (int jj = 0; jj < J; ++jj) v += lp[jj * stride + threadIdx.x];
    out[threadIdx.x] = v;
  }
}

// Safeguarded-Newton update on the 1-D stage-weight search state —
// the device side of the chained line search (line_search.py _newton_1d):
// state = [a, blo, bhi, best_a, best_f, evals, done]; payload = [f, g, h]
// from the preceding eval at coeff = &state[0].  Mirrors the host loop
// exactly so a chain interrupted mid-way can resume on the host.
__global__ void newton_update_kernel(float* __restrict__ st,
                                     const float* __restrict__ p,
                                     float tol) {
  if (st[6] != 0.0f) return;
  const float f = p[0], g = p[1], h = p[2];
  if (!isfinite(f) || !isfinite(g) || !isfinite(h)) { st[6] = 2.0f; return; }
  st[5] += 1.0f;
  const float a = st[0];
  if (f < st[4]) { st[4] = f; st[3] = a; }
  if (g > 0.0f) st[2] = a; else st[1] = a;
  if (fabsf(g) <= tol * fmaxf(1.0f, fabsf(f)) || (st[2] - st[1]) <= tol) {
    st[6] = 1.0f;
    return;
  }
  float nxt;
  if (h > 1e-12f) {
    nxt = a - g / h;
    if (!(st[1] < nxt && nxt < st[2])) nxt = 0.5f * (st[1] + st[2]);
    if (fabsf(nxt - a) <= tol * fmaxf(1.0f, fabsf(a))) {
      st[0] = nxt;
      st[6] = 1.0f;
      return;
    }
  } else {
    nxt = 0.5f * (st[1] + st[2]);
  }
  st[0] = nxt;
}

void newton_chain_1d(torch::Tensor state, torch::Tensor payloads,
                     torch::Tensor label, torch::Tensor pred,
                     torch::Tensor dir, torch::Tensor weight,
                     int64_t loss_id, double param, double tol,
                     int64_t iters) {
  // queue `iters` x (eval -> reduce -> update) with NO host sync: the
  // eval kernel reads the live alpha from state[0] (its coeff pointer),
  // the update kernel advances it.  Steps after convergence evaluate at
  // a frozen alpha and are discarded by the update's done guard — the
  // caller sizes `iters` from the previous round's eval count, so the
  // overshoot is ~0 in steady state.
  CHECK_GPU(state); CHECK_GPU(pred);
  const int64_t n = pred.size(0);
  TORCH_CHECK(pred.size(1) == 1, "newton_chain_1d is scalar-dim only");
  TORCH_CHECK(state.numel() >= 7 && payloads.numel() >= 3 * iters, "sizes");
  auto stream = at::hip::getCurrentHIPStream();
  const int blocks = (int)std::min<int64_t>(ceil_div(n, 256 * 8), 2048);
  auto partials = torch::empty({(int64_t)blocks * 3}, state.options());
  const int rthreads = (256 / 3) * 3;
  for (int k = 0; k < (int)iters; ++k) {
    float* pay = payloads.data_ptr<float>() + 3 * k;
    hipLaunchKernelGGL(line_search_eval_kernel<1>, dim3(blocks), dim3(256), 0,
                       stream, partials.data_ptr<float>(),
                       label.data_ptr<float>(), pred.data_ptr<float>(),
                       dir.data_ptr<float>(), weight.data_ptr<float>(),
                       state.data_ptr<float>(), n, (int)loss_id,
                       (float)param, 1);
    hipLaunchKernelGGL(ls_reduce_kernel, dim3(1), dim3(rthreads), 0, stream,
                       pay, partials.data_ptr<float>(), blocks, 3, 3);
    hipLaunchKernelGGL(newton_update_kernel, dim3(1), dim3(1), 0, stream,
                       state.data_ptr<float>(), pay, (float)tol);
  }
}

void line_search_eval(torch::Tensor payload, torch::Tensor label,
                      torch::Tensor pred, torch::Tensor dir,
                      torch::Tensor weight, torch::Tensor coeff,
                      int64_t loss_id, double param, bool want_hess) {
  CHECK_GPU(payload); CHECK_GPU(pred);
  int64_t n = pred.size(0);
  int D = (int)pred.size(1);
  TORCH_CHECK(D <= 8, "line_search_eval supports dim <= 8");
  TORCH_CHECK(D == 1 || loss_id == L_LOGLOSS,
              "vector line search only for logloss");
  TORCH_CHECK(!want_hess || D == 1, "hessian accumulation is scalar-only");
  TORCH_CHECK(payload.numel() >= 1 + D + (want_hess ? 1 : 0), "payload size");
  auto stream = at::hip::getCurrentHIPStream();
  int blocks = (int)std::min<int64_t>(ceil_div(n, 256 * 8), 2048);
  const int width = 2 + D;
  auto partials = torch::empty({(int64_t)blocks * width},
                               payload.options());
#define LS_LAUNCH(DD)                                                         \
  hipLaunchKernelGGL(line_search_eval_kernel<DD>, dim3(blocks), dim3(256), 0, \
                     stream, partials.data_ptr<float>(),                      \
                     label.data_ptr<float>(), pred.data_ptr<float>(),         \
                     dir.data_ptr<float>(), weight.data_ptr<float>(),         \
                     coeff.data_ptr<float>(), n, (int)loss_id, (float)param,  \
                     want_hess ? 1 : 0)
  switch (D) {
    case 1: LS_LAUNCH(1); break;
    case 2: LS_LAUNCH(2); break;
    case 3: LS_LAUNCH(3); break;
    case 4: LS_LAUNCH(4); break;
    case 5: LS_LAUNCH(5); break;
    case 6: LS_LAUNCH(6); break;
    case 7: LS_LAUNCH(7); break;
    case 8: LS_LAUNCH(8); break;
  }
#undef LS_LAUNCH
  const int rthreads = (256 / width) * width;  // whole lanes per slot
  hipLaunchKernelGGL(ls_reduce_kernel, dim3(1), dim3(rthreads), 0, stream,
                     payload.data_ptr<float>(), partials.data_ptr<float>(),
                     blocks, width, std::min(width, (int)payload.numel()));
}

// ---------------------------------------------------------------------------
// split_argmax: fused best-split search over node histograms.
//   Replaces the eager chain cumsum -> score -> where -> argmax -> gather of
//   reference.split_search (ops/reference.py:150-204; semantics: XGBoost-style
//   newton gain |G|^2/(H+lam), reference analog: the split evaluation inside
//   MLlib DecisionTree invoked via fitBaseLearner, ensembleParams.scala:64-81).
//   One wave scans one feature's B bins (lane-chunked + wave prefix scan in
//   registers), packs (sortable gain, feat*B+bin) into a u64 and atomicMax's
//   a per-node cell — no [n,F,B,C] cumsum/gain tensors ever touch HBM.
// ---------------------------------------------------------------------------

// The scan of one wave over the B bins of one (node, feature) slice, shared
// by split_argmax_kernel and level_scan_kernel: loc holds the lane's BPL
// bins, tot their per-channel sums.
template <int C>
__device__ __forceinline__ void split_scan_wave(
    unsigned long long* __restrict__ best, float (&loc)[4][C], float (&tot)[C],
    int node, int f, int lane, int B, int D, float lam,
    float min_child_weight, float min_instances) {
  const int BPL = (B + 63) >> 6;  // <= 4 for B <= 256
  const int idx_c = C - 1;        // count channel
  // wave-wide exclusive prefix + parent totals (shfl scan per channel)
  float pre[C], parent[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float v = tot[c];
    for (int off = 1; off < 64; off <<= 1) {
      const float u = __shfl_up(v, off, 64);
      if (lane >= off) v += u;
    }
    pre[c] = v - tot[c];
    parent[c] = __shfl(v, 63, 64);
  }
  float pg2 = 0.0f;
#pragma unroll
  for (int d = 0; d < C; ++d)
    if (d < D) pg2 += parent[d] * parent[d];
  const float parent_score = pg2 / (parent[D] + lam);

  float run[C];
#pragma unroll
  for (int c = 0; c < C; ++c) run[c] = pre[c];
  unsigned best_s = 0u;
  int best_b = -1;
  for (int i = 0; i < BPL; ++i) {
    const int b = lane * BPL + i;
    if (b >= B) break;
#pragma unroll
    for (int c = 0; c < C; ++c) run[c] += loc[i][c];
    if (b < B - 1) {  // last bin cannot split
      const float hl = run[D], hr = parent[D] - run[D];
      const float cl = run[idx_c], cr = parent[idx_c] - run[idx_c];
      if (hl >= min_child_weight && hr >= min_child_weight &&
          cl >= min_instances && cr >= min_instances) {
        float gl = 0.0f, gr = 0.0f;
#pragma unroll
        for (int d = 0; d < C; ++d)
          if (d < D) {
            const float l = run[d], r = parent[d] - run[d];
            gl += l * l;
            gr += r * r;
          }
        const float gain =
            gl / (hl + lam) + gr / (hr + lam) - parent_score;
        const unsigned s = f32_sortable(gain);
        if (s > best_s) { best_s = s; best_b = b; }
      }
    }
  }
  // wave argmax
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

template <int C>
__global__ void split_argmax_kernel(
    unsigned long long* __restrict__ best,  // [n_nodes] pre-zeroed
    const float* __restrict__ hist,         // [n_nodes, F, B, C]
    int F, int B, int D, float lam, float min_child_weight,
    float min_instances) {
  const int node = blockIdx.x;
  const int f = blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (f >= F) return;
  const float* h = hist + (((int64_t)node * F + f) * (int64_t)B) * C;
  const int BPL = (B + 63) >> 6;  // <= 4 for B <= 256

  float loc[4][C];
  float tot[C];
#pragma unroll
  for (int c = 0; c < C; ++c) tot[c] = 0.0f;
  for (int i = 0; i < BPL; ++i) {
    const int b = lane * BPL + i;
#pragma unroll
    for (int c = 0; c < C; ++c) loc[i][c] = 0.0f;
    if (b < B) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        loc[i][c] = h[(int64_t)b * C + c];
        tot[c] += loc[i][c];
      }
    }
  }
  split_scan_wave<C>(best, loc, tot, node, f, lane, B, D, lam,
                     min_child_weight, min_instances);
}

// split_argmax_kernel for one tree level that reads its sources in place.
// tab[node] = (built_row, parent_row, sibling_built_row): a built node
// (built_row >= 0) scans built[built_row]; a derived node scans
// parent[parent_row] - built[sibling_built_row], subtracted here in f32.
// Every wave stores the slice it scanned into level[node], which is the next
// level's ``parent``; at the root level IS built (store == 0) and nothing is
// copied, so built and level carry no __restrict__.
template <int C>
__global__ void level_scan_kernel(
    unsigned long long* __restrict__ best,  // [n_nodes] pre-zeroed
    float* level,                           // [n_nodes, F, B, C]
    const float* built,                     // [n_built, F, B, C]
    const float* __restrict__ parent,       // [n_prev, F, B, C]
    const int* __restrict__ tab,            // [n_nodes, 3]
    int store, int F, int B, int D, float lam, float min_child_weight,
    float min_instances) {
  const int node = blockIdx.x;
  const int f = blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (f >= F) return;
  const int b_row = tab[node * 3 + 0];
  const int64_t slice = (int64_t)B * C;
  const float* h = built + ((int64_t)(b_row >= 0 ? b_row : tab[node * 3 + 2]) *
                                F + f) * slice;
  const float* ph =
      b_row >= 0 ? nullptr
                 : parent + ((int64_t)tab[node * 3 + 1] * F + f) * slice;
  float* o = level + ((int64_t)node * F + f) * slice;
  const int BPL = (B + 63) >> 6;  // <= 4 for B <= 256

  float loc[4][C];
  float tot[C];
#pragma unroll
  for (int c = 0; c < C; ++c) tot[c] = 0.0f;
  for (int i = 0; i < BPL; ++i) {
    const int b = lane * BPL + i;
#pragma unroll
    for (int c = 0; c < C; ++c) loc[i][c] = 0.0f;
    if (b < B) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float v = h[(int64_t)b * C + c];
        if (ph) v = ph[(int64_t)b * C + c] - v;
        if (store) o[(int64_t)b * C + c] = v;
        loc[i][c] = v;
        tot[c] += loc[i][c];
      }
    }
  }
  split_scan_wave<C>(best, loc, tot, node, f, lane, B, D, lam,
                     min_child_weight, min_instances);
}

// PACK: the level_split outputs.  ``gain`` is then the [n * (3 + C)] f32
// buffer (gain[n], feat[n], bin[n], left_stats[n, C]) that goes to the host
// in one copy, left_stats points into it, and feat / bin are the int32
// tensors the partition kernel reads.
template <int C, bool PACK = false>
__global__ void split_decode_kernel(
    float* __restrict__ gain, int* __restrict__ feat, int* __restrict__ bin,
    float* __restrict__ left_stats,  // [n, C]
    const unsigned long long* __restrict__ best,
    const float* __restrict__ hist, int F, int B, float min_info_gain) {
  const int node = blockIdx.x;
  const unsigned long long p = best[node];
  const float g = sortable_f32((unsigned)(p >> 32));
  __shared__ float acc[C];
  if (threadIdx.x < C) acc[threadIdx.x] = 0.0f;
  __syncthreads();
  if (p == 0ull || !(g >= min_info_gain)) {
    if (threadIdx.x == 0) {
      gain[node] = -INFINITY;
      feat[node] = -1;
      bin[node] = -1;
      if (PACK) {
        gain[gridDim.x + node] = -1.0f;
        gain[2 * gridDim.x + node] = -1.0f;
      }
    }
    if (threadIdx.x < C) left_stats[node * C + threadIdx.x] = 0.0f;
    return;
  }
  const int fb = (int)(p & 0xFFFFFFFFull);
  const int f = fb / B, b = fb % B;
  const float* h = hist + (((int64_t)node * F + f) * (int64_t)B) * C;
  float part[C];
#pragma unroll
  for (int c = 0; c < C; ++c) part[c] = 0.0f;
  for (int i = threadIdx.x; i <= b; i += blockDim.x)
#pragma unroll
    for (int c = 0; c < C; ++c) part[c] += h[(int64_t)i * C + c];
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (part[c] != 0.0f) atomicAdd(&acc[c], part[c]);
  __syncthreads();
  if (threadIdx.x == 0) {
    gain[node] = g;
    feat[node] = f;
    bin[node] = b;
    if (PACK) {
      gain[gridDim.x + node] = (float)f;
      gain[2 * gridDim.x + node] = (float)b;
    }
  }
  if (threadIdx.x < C) left_stats[node * C + threadIdx.x] = acc[threadIdx.x];
}

void split_argmax(torch::Tensor gain, torch::Tensor feat, torch::Tensor bin,
                  torch::Tensor left_stats, torch::Tensor hist, int64_t d_dims,
                  double lam, double min_child_weight, double min_instances,
                  double min_info_gain) {
  CHECK_GPU(hist); CHECK_CONTIG(hist);
  const int n = (int)hist.size(0);
  const int F = (int)hist.size(1);
  const int B = (int)hist.size(2);
  const int C = (int)hist.size(3);
  const int D = d_dims > 0 ? (int)d_dims : C - 2;
  TORCH_CHECK(C >= 2 && C <= 34, "split_argmax: 2 <= C <= 34");
  TORCH_CHECK(B >= 2 && B <= 256, "split_argmax: 2 <= B <= 256");
  TORCH_CHECK(D >= 1 && D < C, "split_argmax: bad D");
  if (C > 8) {
    // wide one-hot channels (gini trees with 7..32 classes)
    CHECK_GPU(gain); CHECK_GPU(feat); CHECK_GPU(bin); CHECK_GPU(left_stats);
    split_argmax_wide(gain, feat, bin, left_stats, hist, D, lam,
                      min_child_weight, min_instances, min_info_gain);
    return;
  }
  auto best = torch::zeros({n}, hist.options().dtype(torch::kInt64));
  auto stream = at::hip::getCurrentHIPStream();
  const int fpb = 4;  // features (waves) per block
#define SA_LAUNCH(CC)                                                         \
  do {                                                                        \
    hipLaunchKernelGGL(split_argmax_kernel<CC>,                               \
                       dim3(n, (F + fpb - 1) / fpb), dim3(64 * fpb), 0,       \
                       stream,                                                \
                       (unsigned long long*)best.data_ptr<int64_t>(),         \
                       hist.data_ptr<float>(), F, B, D, (float)lam,           \
                       (float)min_child_weight, (float)min_instances);        \
    hipLaunchKernelGGL(split_decode_kernel<CC>, dim3(n), dim3(64), 0, stream, \
                       gain.data_ptr<float>(), feat.data_ptr<int>(),          \
                       bin.data_ptr<int>(), left_stats.data_ptr<float>(),     \
                       (unsigned long long*)best.data_ptr<int64_t>(),         \
                       hist.data_ptr<float>(), F, B, (float)min_info_gain);   \
  } while (0)
  switch (C) {
    case 2: SA_LAUNCH(2); break;
    case 3: SA_LAUNCH(3); break;
    case 4: SA_LAUNCH(4); break;
    case 5: SA_LAUNCH(5); break;
    case 6: SA_LAUNCH(6); break;
    case 7: SA_LAUNCH(7); break;
    case 8: SA_LAUNCH(8); break;
  }
#undef SA_LAUNCH
}

// level_split: the split search of one tree level on its sources in place
// (level_scan_kernel above).  ``table`` is a host int32 [n, 3] of
// (built_row, parent_row, sibling_built_row) per active node; siblings are
// neighbours (j ^ 1), as the grower lays them out.  ``level`` receives the
// level's full histograms; at the root it may be ``built`` itself.  ``pack``
// is the f32 [n * (3 + C)] host-bound result, feat / bin the int32 device
// copies for the partition kernel.  Every row the kernels will touch is
// checked here, before anything is queued.
void level_split(torch::Tensor level, torch::Tensor pack, torch::Tensor feat,
                 torch::Tensor bin, torch::Tensor built, torch::Tensor parent,
                 torch::Tensor table, int64_t d_dims, double lam,
                 double min_child_weight, double min_instances,
                 double min_info_gain) {
  CHECK_GPU(level); CHECK_GPU(pack); CHECK_GPU(feat); CHECK_GPU(bin);
  CHECK_GPU(built);
  CHECK_CONTIG(level); CHECK_CONTIG(pack); CHECK_CONTIG(feat);
  CHECK_CONTIG(bin); CHECK_CONTIG(built); CHECK_CONTIG(parent);
  CHECK_CONTIG(table);
  TORCH_CHECK(!table.is_cuda() && table.scalar_type() == torch::kInt32 &&
                  table.dim() == 2 && table.size(1) == 3,
              "level_split: table must be a host int32 [n, 3]");
  TORCH_CHECK(level.dim() == 4 && built.dim() == 4,
              "level_split: level and built must be [n, F, B, C]");
  TORCH_CHECK(level.scalar_type() == torch::kFloat32 &&
                  built.scalar_type() == torch::kFloat32 &&
                  pack.scalar_type() == torch::kFloat32 &&
                  feat.scalar_type() == torch::kInt32 &&
                  bin.scalar_type() == torch::kInt32,
              "level_split: f32 histograms and pack, int32 feat and bin");
  const int64_t n = level.size(0);
  const int64_t n_built = built.size(0);
  const int F = (int)level.size(1);
  const int B = (int)level.size(2);
  const int C = (int)level.size(3);
  const int D = d_dims > 0 ? (int)d_dims : C - 2;
  TORCH_CHECK(built.size(1) == F && built.size(2) == B && built.size(3) == C,
              "level_split: built and level disagree in F, B, C");
  const bool has_parent = parent.numel() > 0;
  int64_t n_prev = 0;
  if (has_parent) {
    CHECK_GPU(parent);
    TORCH_CHECK(parent.dim() == 4 && parent.scalar_type() == torch::kFloat32 &&
                    parent.size(1) == F && parent.size(2) == B &&
                    parent.size(3) == C,
                "level_split: parent and level disagree in F, B, C");
    n_prev = parent.size(0);
    TORCH_CHECK(parent.data_ptr() != level.data_ptr(),
                "level_split: level must not be parent");
  }
  TORCH_CHECK(level.device() == built.device() &&
                  pack.device() == built.device() &&
                  feat.device() == built.device() &&
                  bin.device() == built.device() &&
                  (!has_parent || parent.device() == built.device()),
              "level_split: all device tensors on one device");
  TORCH_CHECK(n < ((int64_t)1 << 31), "level_split: too many nodes");
  TORCH_CHECK(C >= 2 && C <= 8, "level_split: 2 <= C <= 8");
  TORCH_CHECK(B >= 2 && B <= 256, "level_split: 2 <= B <= 256");
  TORCH_CHECK(D >= 1 && D < C, "level_split: bad D");
  TORCH_CHECK(table.size(0) == n, "level_split: one table row per node");
  TORCH_CHECK(pack.numel() == n * (3 + C) && feat.numel() == n &&
                  bin.numel() == n,
              "level_split: pack is [n * (3 + C)], feat and bin are [n]");
  const bool alias = level.data_ptr() == built.data_ptr();
  TORCH_CHECK(!alias || n == n_built,
              "level_split: level may alias built only when every node is "
              "built in place");
  auto overlaps = [](const torch::Tensor& a, const torch::Tensor& b) {
    const char* a0 = (const char*)a.data_ptr();
    const char* b0 = (const char*)b.data_ptr();
    return a0 < b0 + b.nbytes() && b0 < a0 + a.nbytes();
  };
  TORCH_CHECK(alias || !overlaps(level, built),
              "level_split: level overlaps built without being it");
  TORCH_CHECK(!has_parent || !overlaps(level, parent),
              "level_split: level overlaps parent");
  auto tb = table.accessor<int, 2>();
  for (int64_t j = 0; j < n; ++j) {
    const int br = tb[j][0];
    if (br >= 0) {
      TORCH_CHECK(br < n_built, "level_split: built_row ", br, " of node ", j,
                  " out of range");
      TORCH_CHECK(!alias || br == j,
                  "level_split: level aliases built but node ", j,
                  " is built in row ", br);
      continue;
    }
    TORCH_CHECK(br == -1, "level_split: built_row of node ", j, " is ", br);
    TORCH_CHECK(!alias, "level_split: level aliases built but node ", j,
                " is derived");
    TORCH_CHECK(tb[j][1] >= 0 && tb[j][1] < n_prev,
                "level_split: parent_row ", tb[j][1], " of node ", j,
                " out of range");
    TORCH_CHECK(tb[j][2] >= 0 && tb[j][2] < n_built,
                "level_split: sibling_built_row ", tb[j][2], " of node ", j,
                " out of range");
    const int64_t sib = j ^ 1;
    TORCH_CHECK(sib < n && tb[sib][0] == tb[j][2],
                "level_split: the sibling of derived node ", j,
                " is not the built node in row ", tb[j][2]);
  }
  if (n == 0 || F == 0) return;
  auto tab = h2d_async(table.data_ptr(), (size_t)n * 12, kSlotLevelTable,
                       level.device());
  auto best = torch::zeros({n}, level.options().dtype(torch::kInt64));
  auto stream = at::hip::getCurrentHIPStream();
  const int fpb = 4;  // features (waves) per block
  float* pk = pack.data_ptr<float>();
#define LS_LAUNCH(CC)                                                         \
  do {                                                                        \
    hipLaunchKernelGGL(level_scan_kernel<CC>,                                 \
                       dim3((unsigned)n, (F + fpb - 1) / fpb),                \
                       dim3(64 * fpb), 0, stream,                             \
                       (unsigned long long*)best.data_ptr<int64_t>(),         \
                       level.data_ptr<float>(), built.data_ptr<float>(),      \
                       has_parent ? parent.data_ptr<float>() : nullptr,       \
                       (const int*)tab.data_ptr(), alias ? 0 : 1, F, B, D,    \
                       (float)lam, (float)min_child_weight,                   \
                       (float)min_instances);                                 \
    hipLaunchKernelGGL((split_decode_kernel<CC, true>), dim3((unsigned)n),    \
                       dim3(64), 0, stream, pk, feat.data_ptr<int>(),         \
                       bin.data_ptr<int>(), pk + 3 * n,                       \
                       (unsigned long long*)best.data_ptr<int64_t>(),         \
                       level.data_ptr<float>(), F, B, (float)min_info_gain);  \
  } while (0)
  switch (C) {
    case 2: LS_LAUNCH(2); break;
    case 3: LS_LAUNCH(3); break;
    case 4: LS_LAUNCH(4); break;
    case 5: LS_LAUNCH(5); break;
    case 6: LS_LAUNCH(6); break;
    case 7: LS_LAUNCH(7); break;
    case 8: LS_LAUNCH(8); break;
  }
#undef LS_LAUNCH
}

// csrc/hist_plan.h on host tensors, for tests: touches no device
std::tuple<int64_t, torch::Tensor, torch::Tensor> hist_plan_debug(
    torch::Tensor node_offsets, torch::Tensor node_col0, int64_t row_bound,
    int64_t col_bound, int64_t lds_bytes, int64_t n_groups) {
  auto offs = node_offsets.to(torch::kInt64).contiguous();
  auto col0 = node_col0.to(torch::kInt32).contiguous();
  const int n_nodes = (int)offs.numel() - 1;
  TORCH_CHECK(col0.numel() == 0 || col0.numel() == n_nodes,
              "node_col0 must be empty or have one entry per node");
  HistPlan plan = plan_hist_chunks(
      offs.data_ptr<int64_t>(), n_nodes,
      col0.numel() ? col0.data_ptr<int>() : nullptr, row_bound,
      (int)col_bound, (size_t)lds_bytes, (int)n_groups, 0);
  auto i32 = torch::TensorOptions().dtype(torch::kInt32);
  auto chunks = torch::tensor(plan.table, i32).view({plan.n_chunks, 5});
  auto multi = torch::tensor(plan.multi_nodes, i32);
  return {plan.chunk_rows, chunks, multi};
}

// the same plan's staging slots: (first record, record count) per slot, in
// the order of _hist_plan's multi_nodes
std::tuple<torch::Tensor, torch::Tensor> hist_plan_slots_debug(
    torch::Tensor node_offsets, torch::Tensor node_col0, int64_t row_bound,
    int64_t col_bound, int64_t lds_bytes, int64_t n_groups) {
  auto offs = node_offsets.to(torch::kInt64).contiguous();
  auto col0 = node_col0.to(torch::kInt32).contiguous();
  const int n_nodes = (int)offs.numel() - 1;
  TORCH_CHECK(col0.numel() == 0 || col0.numel() == n_nodes,
              "node_col0 must be empty or have one entry per node");
  HistPlan plan = plan_hist_chunks(
      offs.data_ptr<int64_t>(), n_nodes,
      col0.numel() ? col0.data_ptr<int>() : nullptr, row_bound,
      (int)col_bound, (size_t)lds_bytes, (int)n_groups, 0);
  auto i32 = torch::TensorOptions().dtype(torch::kInt32);
  return {torch::tensor(plan.slot_first, i32),
          torch::tensor(plan.slot_count, i32)};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("_hist_plan", &hist_plan_debug,
        "host-side chunk plan of the histogram kernels (no device)");
  m.def("_hist_plan_slots", &hist_plan_slots_debug,
        "first record and record count of each staging slot of _hist_plan");
  m.def("gather_ranges_gh", &gather_ranges_gh,
        "gather_ranges plus the compact gh rows of the gathered rows");
  m.def("logreg_loss_grad", &logreg_loss_grad,
        "single-pass fused logistic loss+gradient");
  m.def("logreg_fused_supported", &logreg_fused_supported);
  m.def("split_argmax", &split_argmax,
        "fused best-split gain scan + argmax over node histograms");
  m.def("sample_weights", &sample_weights, "counter-based Poisson/Bernoulli row weights");
  m.def("bin_features", &bin_features, "quantile binning f32 -> u8");
  m.def("hist_build", &hist_build, "LDS-staged node histograms",
        py::arg("out"), py::arg("bins"), py::arg("gh"), py::arg("row_idx"),
        py::arg("node_offsets"), py::arg("num_bins"), py::arg("d_dims"),
        py::arg("max_abs"), py::arg("identity_rows"), py::arg("node_col0"),
        py::arg("c_per_node"), py::arg("gh_by_position") = false);
  m.def("hist_build_class", &hist_build_class,
        "label-indexed node histograms for K-class gini trees");
  m.def("partition_rows", &partition_rows, "block-aggregated node partition");
  m.def("partition_rows_cursors", &partition_rows_cursors,
        "node partition that returns its cursor table");
  m.def("level_split", &level_split,
        "split search of one tree level on built / parent - sibling in place");
  m.def("tree_predict", &tree_predict, "single-tree batched predict");
  m.def("forest_predict", &forest_predict, "packed-forest weighted predict");
  m.def("forest_predict2", &forest_predict2,
        "LDS-staged tree-group-tiled forest predict");
  m.def("forest_contrib", &forest_contrib,
        "per-row feature contributions (TreeSHAP) of a packed forest");
  m.def("forest_staged_loss", &forest_staged_loss,
        "per-stage weighted loss sums of a packed boosted forest");
  m.def("forest_staged_geometry", &forest_staged_geometry,
        "(threads, rows per lane, grid cap) of forest_staged_loss");
  m.def("forest_oob", &forest_oob,
        "out-of-bag leaf sums and counts of a packed forest under a mask");
  m.def("forest_oob_geometry", &forest_oob_geometry,
        "(threads, rows per lane, grid cap) of forest_oob");
  m.def("forest_permute_loss", &forest_permute_loss,
        "loss sums of a packed forest with each feature column shuffled");
  m.def("forest_permute_geometry", &forest_permute_geometry,
        "(threads, rows per lane, grid cap, feature chunk, group nodes, "
        "depth cap) of forest_permute_loss");
  m.def("transpose_u8", &transpose_u8, "tiled u8 matrix transpose");
  m.def("gather_ranges", &gather_ranges,
        "one-pass concat of contiguous index ranges");
  m.def("leaf_scatter", &leaf_scatter,
        "scatter per-segment leaf values into the [N, T] train-pred matrix");
  m.def("grad_hess", &grad_hess, "fused per-row loss gradient/hessian");
  m.def("line_search_eval", &line_search_eval, "fused loss+grad line-search payload");
  m.def("newton_chain_1d", &newton_chain_1d,
        "device-chained safeguarded-Newton stage-weight search");
}
