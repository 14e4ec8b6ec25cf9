// Weighted augmented Gram matrix for LinearRegression's normal equations:
//   G = sum_i w_i * z_i z_i^T,   z_i = [x_i (F values), 1, y_i],   D = F + 2
// as a dense, exactly symmetric [D, D] f64 tensor, in one pass over x[N, F]
// (f32, row-major), y[N] and w[N].  G[:F+1, :F+1] is X_a^T W X_a,
// G[:F+1, F+1] is X_a^T W y.  The ones and y columns are generated while a
// row tile is staged; neither cat([x, ones]) nor x * w ever exists in memory.
// The weight scales the A operand only (no sqrt), so zero and negative
// weights follow the formula.
//
// Products are v_mfma_f32_16x16x4f32 tiles that contract over rows.  D pads
// to T = ceil(D/16) column tiles; only tile pairs ti <= tj are computed and
// linear_gram_reduce_kernel mirrors them, which makes G exactly symmetric and
// halves the flops of the GEMM.  f32 MFMA runs at the vector rate on gfx950:
// N*D^2 flop over 4*N*F bytes is D/4 flop/byte, so the kernel is HBM-bound
// up to D of about 128 and bound by the matrix pipe above.
//
// Geometry (host planner lg_plan, exposed as linear_gram_geometry):
//   work unit   a "super pair" (I, J), I <= J, of 32-column super tiles: 2 x 2
//               MFMA tiles = 16 accumulator registers.  Per 4-row k-step a
//               wave reads the two fragments of I and the two of J (4
//               ds_read_b32), scales the I copies by w and issues 4 MFMAs.
//               (Where I == J the tile below the diagonal is computed and
//               ignored: skipping it costs a branch between the MFMAs.)
//   block       512 threads = 8 waves, persistent over row tiles of R rows in
//               grid-stride order.  Super pairs go round-robin over the
//               waves, at most kLgSpMax = 8 each (128 accumulator registers),
//               and stay in registers across row tiles.  With 4 or fewer
//               super pairs (D <= 64) the waves left over split the 16-row
//               groups of a tile instead of idling, 8 / pairs ways.
//   panels      S = ceil(T/2) super tiles.  S <= 10 (D <= 320) is 55 super
//               pairs and fits one block.  Above that the super tiles split
//               into NP = ceil(S/8) panels of ps = ceil(S/NP) <= 8; a block
//               owns one panel pair (<= 64 super pairs) and stages only its
//               two column ranges.  The grid is (panel pairs) x (row
//               workers); a pair on the diagonal has about half the work of
//               one off it and gets half the workers.
//   staging     the row tile is in LDS once (row stride 16*Wt + 2 floats, Wt
//               the widest block's tile count rounded up to even).  The next
//               tile's global loads (non-temporal: every row is read once per
//               block) are issued into registers before the MFMA loop and
//               stored after it.  R is the largest multiple of 16 <= 128 that
//               keeps those at 8 float4 per thread, whole rows per pass.  Rows past N are
//               zero-filled, never loaded; F % 4 != 0 takes scalar loads.
//
// LDS banks: both MFMA operands are column reads of the tile, the transposed
// ds_read_b32 of linear_wide.hip's phase 2.  MFMA j of a 16-row group reads
// row 8*(q&1) + 4*(q>>1) + j for lane group q (the contraction order is free
// as both operands and w use the same row): the two rows of a 32-lane group
// are 8 apart, 8 * stride = 16 mod 32, so 2 x 16 contiguous floats cover all
// 32 banks.
//
// Precision and determinism: no atomics.  Every (block, wave) owns a slot of
// f64 copies of its accumulators.  An f32 accumulator runs over at most
// kLgFlushRows rows before it is added into the slot and cleared.  The
// reduce kernel sums the slots of an entry in f64 in block order.  Grid and
// flush points depend only on N, F and the device's CU count, so the result
// is bitwise reproducible.

#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

constexpr int kLgThreads = 512;
constexpr int kLgWaves = kLgThreads / 64;
constexpr int kLgMaxD = 1024;
constexpr int kLgSpMax = 8;          // super pairs per wave
constexpr int kLgPfMax = 8;          // staged float4 per thread
constexpr int kLgRowsMax = 128;      // rows per tile
constexpr int kLgFlushRows = 16384;  // rows per f32 accumulator run
constexpr int kLgSlotSp = 16 * 64;   // doubles per (wave, super pair)

typedef float lg_f4 __attribute__((ext_vector_type(4)));
typedef float lg_f2 __attribute__((ext_vector_type(2)));

// row groups that share one super pair where a block has few of them
__host__ __device__ inline int lg_row_groups(int count) {
  return count <= 4 ? kLgWaves / count : 1;
}

struct LgPlan {
  bool ok = false;
  int D = 0, T = 0, S = 0;
  int NP = 0;           // panels
  int ps = 0;           // super tiles per panel
  int R = 0;            // rows per tile
  int stride = 0;       // LDS row stride, floats
  int nsp = 0;          // super pairs per wave, most loaded block
  int NSP = 0;          // nsp rounded up to a power of two (template size)
  int flush_tiles = 0;  // row tiles between flushes
  size_t lds = 0;
};

LgPlan lg_plan(int64_t F) {
  LgPlan p;
  if (F < 1 || F + 2 > kLgMaxD) return p;
  p.D = (int)F + 2;
  p.T = (int)ceil_div(p.D, 16);
  p.S = (p.T + 1) / 2;
  int count, wt;
  if (p.S * (p.S + 1) / 2 <= kLgWaves * kLgSpMax) {
    p.NP = 1; p.ps = p.S;
    count = p.S * (p.S + 1) / 2;
    wt = 2 * p.S;
  } else {
    p.NP = (int)ceil_div(p.S, 8);
    p.ps = (int)ceil_div(p.S, p.NP);
    count = p.ps * p.ps;
    wt = 4 * p.ps;
  }
  p.nsp = (int)ceil_div(count, kLgWaves);
  p.NSP = 1;
  while (p.NSP < p.nsp) p.NSP <<= 1;
  p.stride = 16 * wt + 2;
  // a staging pass covers at least 512 / (4 * wt) rows, kLgPfMax passes
  p.R = std::min(kLgRowsMax, kLgPfMax * (kLgThreads / (4 * wt)) / 16 * 16);
  p.flush_tiles = kLgFlushRows / p.R;
  p.lds = ((size_t)p.R * p.stride + p.R) * 4;
  p.ok = true;
  return p;
}

struct LgArgs {
  int F, T, S, NP, ps, R, stride, nsp, flush_tiles;
  int ud, uo;  // row workers of a diagonal / off-diagonal panel pair
  int vec;
  int64_t n, n_tiles;
};

// index of the off-diagonal panel pair (pa < pb) in lexicographic order
__device__ inline int lg_off_index(int pa, int pb, int NP) {
  return pa * (NP - 1) - pa * (pa - 1) / 2 + (pb - pa - 1);
}

template <int NSP>
__global__ __launch_bounds__(kLgThreads) void linear_gram_kernel(
    double* __restrict__ slots,   // [grid][8 waves][nsp][4][64][4]
    const float* __restrict__ x,  // [N, F]
    const float* __restrict__ y,  // [N]
    const float* __restrict__ w,  // [N]
    const LgArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m16 = lane & 15;
  const int q = lane >> 4;
  const int F = a.F, R = a.R, stride = a.stride;
  float* const xt = lds;
  float* const wbuf = lds + R * stride;

  // block -> panel pair (pa <= pb) and row worker
  int pa, pb, worker, workers;
  {
    const int b = blockIdx.x, nd = a.NP * a.ud;
    if (b < nd) {
      pa = pb = b / a.ud; worker = b - pa * a.ud; workers = a.ud;
    } else {
      const int o = (b - nd) / a.uo;
      worker = (b - nd) - o * a.uo; workers = a.uo;
      int rem = o;
      pa = 0;
      while (rem >= a.NP - 1 - pa) { rem -= a.NP - 1 - pa; ++pa; }
      pb = pa + 1 + rem;
    }
  }
  const bool diag = pa == pb;
  const int psa = min(a.ps, a.S - pa * a.ps);
  const int psb = min(a.ps, a.S - pb * a.ps);
  const int ta0 = 2 * pa * a.ps, tb0 = 2 * pb * a.ps;
  const int na = min(2 * psa, a.T - ta0);  // even off the diagonal: pa < NP-1
  const int nb = min(2 * psb, a.T - tb0);
  const int offB = diag ? 0 : na;          // local tile of range B

  // this wave's super pairs: the first nlive of its NSP, as local columns
  const int count = diag ? psa * (psa + 1) / 2 : psa * psb;
  const int rgc = lg_row_groups(count);
  const int rg = rgc > 1 ? wv / count : 0;
  const int nlive = rgc > 1 ? (rg < rgc ? 1 : 0)
                            : (count - wv + kLgWaves - 1) / kLgWaves;
  int oa[NSP], ob[NSP];
#pragma unroll
  for (int k = 0; k < NSP; ++k) {
    const int L = rgc > 1 ? wv % count : wv + kLgWaves * k;
    int I = 0, J = 0;
    if (k < nlive) {
      if (diag) {
        int rem = L;
        while (rem >= psa - I) { rem -= psa - I; ++I; }
        J = I + rem;
      } else {
        I = L / psb; J = L - I * psb;
      }
    }
    oa[k] = 2 * I * 16;
    ob[k] = (offB + 2 * J) * 16;
  }
  lg_f4 acc[NSP][4];
#pragma unroll
  for (int k = 0; k < NSP; ++k)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[k][t] = lg_f4{0.f, 0.f, 0.f, 0.f};

  // staging: the x columns of the two ranges are C4 = C4a + C4b float4 wide.
  // A pass covers rpp = 512 / C4 whole rows, a thread keeps its column and
  // moves down rpp rows per pass; the planner's R needs at most kLgPfMax.
  const int xa_end = min(F, (ta0 + na) * 16), xb_end = min(F, (tb0 + nb) * 16);
  const int C4a = max(0, (xa_end - ta0 * 16 + 3) >> 2);
  const int C4b = diag ? 0 : max(0, (xb_end - tb0 * 16 + 3) >> 2);
  const int C4 = C4a + C4b;
  const int C4d = max(C4, 1);
  const int rpp = kLgThreads / C4d;
  const int srow = tid / C4d, scol = tid - srow * C4d;
  const bool s_on = C4 > 0 && srow < rpp;
  const bool inA = scol < C4a;
  const int gcol = inA ? ta0 * 16 + 4 * scol : tb0 * 16 + 4 * (scol - C4a);
  const int left = (inA ? xa_end : xb_end) - gcol;  // >= 1 where s_on
  const unsigned voff = (unsigned)(srow * F + gcol);
  float* const sdst =  // 8-byte aligned
      xt + srow * stride + (inA ? 4 * scol : offB * 16 + 4 * (scol - C4a));
  // local columns of the ones and y columns, -1 where outside both ranges
  auto local_col = [&](int c) {
    if (c >= ta0 * 16 && c < (ta0 + na) * 16) return c - ta0 * 16;
    if (!diag && c >= tb0 * 16 && c < (tb0 + nb) * 16)
      return offB * 16 + c - tb0 * 16;
    return -1;
  };
  const int l_one = local_col(F), l_y = local_col(F + 1);

  lg_f4 pf[kLgPfMax];
  float pf_w = 0.f, pf_y = 0.f, pf_one = 0.f;
  auto load_tile = [&](int64_t row0) {
#pragma unroll
    for (int u = 0; u < kLgPfMax; ++u) {
      const int row = srow + u * rpp;
      lg_f4 v = lg_f4{0.f, 0.f, 0.f, 0.f};
      if (s_on && row < R && row0 + row < a.n) {
        const float* p = x + (row0 + u * rpp) * F + voff;
        if (a.vec) {
          // every row is read once per block: keep it out of the caches
          v = __builtin_nontemporal_load(reinterpret_cast<const lg_f4*>(p));
        } else {
          v.x = p[0];
          if (left > 1) v.y = p[1];
          if (left > 2) v.z = p[2];
          if (left > 3) v.w = p[3];
        }
      }
      pf[u] = v;
    }
    if (tid < R) {
      const bool valid = row0 + tid < a.n;
      pf_w = valid ? w[row0 + tid] : 0.f;
      pf_y = valid ? y[row0 + tid] : 0.f;
      pf_one = valid ? 1.f : 0.f;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int u = 0; u < kLgPfMax; ++u) {
      if (s_on && srow + u * rpp < R) {
        float* d = sdst + u * rpp * stride;
        if (a.vec) {
          *reinterpret_cast<lg_f2*>(d) = lg_f2{pf[u].x, pf[u].y};
          *reinterpret_cast<lg_f2*>(d + 2) = lg_f2{pf[u].z, pf[u].w};
        } else {
          // the ones and y columns may follow within this float4
          d[0] = pf[u].x;
          if (left > 1) d[1] = pf[u].y;
          if (left > 2) d[2] = pf[u].z;
          if (left > 3) d[3] = pf[u].w;
        }
      }
    }
    if (tid < R) {
      wbuf[tid] = pf_w;
      if (l_one >= 0) xt[tid * stride + l_one] = pf_one;
      if (l_y >= 0) xt[tid * stride + l_y] = pf_y;
    }
  };

  // The owner alone touches its slot [nsp][4 tiles][64 lanes][4]: it clears
  // it here and adds to it at every flush.  The lane offset is made opaque
  // inside flush so the 32 addresses per super pair are formed there, one
  // tile at a time, instead of living in registers across the MFMA loop.
  double* const sbase =
      slots + ((int64_t)blockIdx.x * kLgWaves + wv) * a.nsp * kLgSlotSp;
#pragma unroll
  for (int k = 0; k < NSP; ++k)
    if (k < nlive)
      for (int t = 0; t < 4; ++t)
        for (int i = 0; i < 4; ++i)
          sbase[((k * 4 + t) * 64 + lane) * 4 + i] = 0.0;
  auto flush = [&]() {
    unsigned ln = lane;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int k = 0; k < NSP; ++k) {
      if (k < nlive) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          double* s = sbase + ((k * 4 + t) * 64 + ln) * 4;
#pragma unroll
          for (int i = 0; i < 4; ++i) s[i] += (double)acc[k][t][i];
          acc[k][t] = lg_f4{0.f, 0.f, 0.f, 0.f};
          asm volatile("" ::: "memory");
        }
      }
    }
  };

  // columns past D are never staged: zero them once
  for (int i = tid; i < R * stride + R; i += kLgThreads) lds[i] = 0.0f;
  __syncthreads();
  int64_t bt = worker;  // < n_tiles: no panel pair has more workers than tiles
  load_tile(bt * R);
  store_tile();
  __syncthreads();

  const int prow = 8 * (q & 1) + 4 * (q >> 1);  // row of MFMA j = 0
  int since = 0;
  for (; bt < a.n_tiles; bt += workers) {
    const int64_t nb_t = bt + workers;
    const bool more = nb_t < a.n_tiles;
    if (more) load_tile(nb_t * R);

    // a tile past the block's columns (odd tile count) reads the zero padding
    for (int kg = rg; kg < R / 16; kg += rgc) {
      const int r0 = kg * 16 + prow;
      // opaque: one base per row group, fragment addresses formed at their
      // reads, not 8 induction registers per super pair
      unsigned ro = r0 * stride + m16;
      asm volatile("" : "+v"(ro));
      const float* rp = xt + ro;
      float wr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) wr[j] = wbuf[r0 + j];
#pragma unroll
      for (int k = 0; k < NSP; ++k) {
        if (k < nlive) {
          // 16 reads, then 16 MFMAs on 4 independent accumulators
          float fa[4][2], fb[4][2];
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              fa[j][h] = rp[j * stride + oa[k] + 16 * h];
              fb[j][h] = rp[j * stride + ob[k] + 16 * h];
            }
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const float aw = fa[j][h] * wr[j];
              acc[k][2 * h] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  aw, fb[j][0], acc[k][2 * h], 0, 0, 0);
              acc[k][2 * h + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  aw, fb[j][1], acc[k][2 * h + 1], 0, 0, 0);
            }
        }
      }
    }
    if (++since == a.flush_tiles && more) {
      flush();
      since = 0;
    }
    __syncthreads();  // the tile is read to the end of the MFMA loop
    if (more) store_tile();
    __syncthreads();
  }
  flush();
}

// G[i][j] = G[j][i] = sum over the slots that hold entry (i, j), i <= j, in
// f64 in block order (row groups of a block inside it).  One block per tile
// pair; the ones below the diagonal leave at once.
__global__ __launch_bounds__(256) void linear_gram_reduce_kernel(
    double* __restrict__ G, const double* __restrict__ slots, int D,
    const LgArgs a) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (ti > tj) return;
  const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
  const int i = ti * 16 + r, j = tj * 16 + c;
  if (i > j || j >= D) return;
  const int si = ti >> 1, sj = tj >> 1;
  const int pa = si / a.ps, pb = sj / a.ps;
  const int I = si - pa * a.ps, J = sj - pb * a.ps;
  const int psa = min(a.ps, a.S - pa * a.ps);
  const int psb = min(a.ps, a.S - pb * a.ps);
  int L, count, block0, workers;
  if (pa == pb) {
    L = I * psa - I * (I - 1) / 2 + (J - I);
    count = psa * (psa + 1) / 2;
    block0 = pa * a.ud; workers = a.ud;
  } else {
    L = I * psb + J;
    count = psa * psb;
    block0 = a.NP * a.ud + lg_off_index(pa, pb, a.NP) * a.uo; workers = a.uo;
  }
  const int rgc = lg_row_groups(count);
  const int t4 = (ti & 1) * 2 + (tj & 1);
  const int64_t in_slot = (t4 * 64 + (r >> 2) * 16 + c) * 4 + (r & 3);
  double sum = 0.0;
  for (int wk = 0; wk < workers; ++wk)
    for (int g = 0; g < rgc; ++g) {
      const int Lr = L + count * g;  // < 8 where rgc > 1
      const int64_t sl =
          ((int64_t)(block0 + wk) * kLgWaves + (Lr & 7)) * a.nsp + (Lr >> 3);
      sum += slots[sl * kLgSlotSp + in_slot];
    }
  G[(int64_t)i * D + j] = sum;
  G[(int64_t)j * D + i] = sum;
}

}  // namespace

bool linear_gram_supported(int64_t F) { return lg_plan(F).ok; }

// (column tiles, panels, rows per tile, LDS bytes, rows between f32 flushes,
// largest single-panel F); all 0 where unsupported
std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>
linear_gram_geometry(int64_t F) {
  const LgPlan p = lg_plan(F);
  if (!p.ok) return {0, 0, 0, 0, 0, 0};
  int64_t single = 1;
  while (lg_plan(single + 1).ok && lg_plan(single + 1).NP == 1) ++single;
  return {p.T, p.NP, p.R, (int64_t)p.lds, (int64_t)p.flush_tiles * p.R, single};
}

void linear_gram(torch::Tensor G, torch::Tensor x, torch::Tensor y,
                 torch::Tensor w) {
  CHECK_GPU(G); CHECK_GPU(x); CHECK_GPU(y); CHECK_GPU(w);
  CHECK_CONTIG(G); CHECK_CONTIG(x); CHECK_CONTIG(y); CHECK_CONTIG(w);
  TORCH_CHECK(x.dim() == 2, "x must be 2-d");
  const int64_t n = x.size(0);
  const int64_t F = x.size(1);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32 &&
                  y.scalar_type() == torch::kFloat32 &&
                  w.scalar_type() == torch::kFloat32,
              "x, y and w must be f32");
  TORCH_CHECK(G.scalar_type() == torch::kFloat64, "G must be f64");
  TORCH_CHECK(n >= 1 && y.numel() == n && w.numel() == n, "row counts");
  const LgPlan p = lg_plan(F);
  TORCH_CHECK(p.ok, "unsupported F for linear_gram: ", F);
  TORCH_CHECK(G.dim() == 2 && G.size(0) == p.D && G.size(1) == p.D,
              "G must be [F+2, F+2]");

  LgArgs a;
  a.F = (int)F; a.T = p.T; a.S = p.S; a.NP = p.NP; a.ps = p.ps; a.R = p.R;
  a.stride = p.stride; a.nsp = p.nsp; a.flush_tiles = p.flush_tiles;
  a.n = n;
  a.n_tiles = ceil_div(n, p.R);
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int n_off = p.NP * (p.NP - 1) / 2;
  const int u = std::max(1, cus / (p.NP + 2 * n_off));
  a.ud = (int)std::min<int64_t>(u, a.n_tiles);
  a.uo = (int)std::min<int64_t>(2 * u, a.n_tiles);
  a.vec = (F % 4 == 0) && (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0);
  const int grid = p.NP * a.ud + n_off * a.uo;
  // every entry the reduction reads is cleared and summed by its owner
  auto slots = torch::empty({(int64_t)grid * kLgWaves * p.nsp * kLgSlotSp},
                            G.options());
  auto stream = at::hip::getCurrentHIPStream();
  bool done = false;
#define LG_LAUNCH(NN)                                                        \
  do {                                                                       \
    if (p.lds > 65536)                                                       \
      TORCH_CHECK(                                                           \
          hipFuncSetAttribute(                                               \
              reinterpret_cast<const void*>(&linear_gram_kernel<NN>),        \
              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds) ==     \
              hipSuccess,                                                    \
          "linear_gram: cannot reserve ", p.lds, " bytes of LDS");           \
    hipLaunchKernelGGL((linear_gram_kernel<NN>), dim3(grid),                 \
                       dim3(kLgThreads), p.lds, stream,                      \
                       slots.data_ptr<double>(), x.data_ptr<float>(),        \
                       y.data_ptr<float>(), w.data_ptr<float>(), a);         \
    done = true;                                                             \
  } while (0)
  switch (p.NSP) {
    case 1: LG_LAUNCH(1); break;
    case 2: LG_LAUNCH(2); break;
    case 4: LG_LAUNCH(4); break;
    case 8: LG_LAUNCH(8); break;
  }
#undef LG_LAUNCH
  TORCH_CHECK(done, "linear_gram dispatch failed for F=", F);
  hipLaunchKernelGGL(linear_gram_reduce_kernel, dim3(p.T, p.T), dim3(256), 0,
                     stream, G.data_ptr<double>(), slots.data_ptr<double>(),
                     p.D, a);
  // a refused launch must raise: G is uninitialised memory
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "linear_gram: kernel launch failed: ",
              hipGetErrorString(err));
}
