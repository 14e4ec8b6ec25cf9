// Fused logistic-regression loss+gradient on the matrix pipe, for the shapes
// csrc/linear.hip declines: 2 <= K <= 32 classes, 1 <= F <= 1024 features.
//
// Same payload contract as linear.hip ([1 + (F+1)*K] f32 = loss_sum,
// grad[F][K], grad_bias[K], unnormalised sums), same single pass over X, but
// both products run as f32 MFMA tiles (v_mfma_f32_16x16x4f32): at 9..32
// classes X@W and X^T@G are real GEMM tiles, and the matrix pipe does the
// cross-lane reduction the narrow kernel pays 6*K shuffles per row for.  f32
// MFMA runs at the vector rate on gfx950, so the gain is data layout and
// register economy, not a higher peak: 4*F*KP flop over 4*F bytes per row is
// KP flop/byte, about level with HBM at KP = 32 and HBM-bound at KP = 16.
//
// Geometry (host planner lw_plan, exposed as logreg_wide_geometry):
//   classes pad to KP in {16, 32}, features to T = ceil(F/16) tiles of 16.
//   A block is 512 threads = 8 waves = S feature slices x R = 8/S row
//   groups, one block per CU, persistent over block tiles of R*16 rows in
//   grid-stride order.  Wave (s, g) owns the tiles [s*nts, (s+1)*nts) of the
//   feature axis, nts = ceil(T/S), for BOTH products:
//     W slice      as MFMA B-fragments in registers, loaded once per launch
//     grad slice   as MFMA accumulators, live for the whole launch
//   The planner takes the smallest S with nts <= 8 whose LDS fits 160 KiB:
//   8 tiles are 64 registers each for W and the gradient at KP = 32 and 32
//   each at KP = 16.  (Deviation from a flat 4096-element budget: 16 tiles
//   at KP = 16 spilled 408 bytes per lane once the prefetch registers joined
//   the two 64-register slices, so KP = 16 stops at 2048 elements.)
//
// Per block tile:
//   1. the R*16 x F tile of X is in LDS (row stride T*16 + 2 floats).  The
//      next tile's global loads are issued into registers first, so they fly
//      under the MFMA work; they are staged in two halves to halve the
//      registers they hold.
//   2. phase 1, contraction over features: A = X[row][f] read as ds_read_b64
//      (lane (m, q) reads features 8h+2q, 8h+2q+1 of row m; the contraction
//      index may be permuted freely as long as the W fragment agrees),
//      B = W fragment, accumulator = the slice's partial margins [16][KP].
//   3. partial margins go to LDS [R][S][16][KP]; slice 0's wave of each row
//      group sums them in slice order, adds the bias and computes the
//      max-subtracted softmax, the row loss, G = (p - onehot) * w and the
//      bias gradient ONCE per row (4 lanes per row).  Padded classes are
//      masked out of max and sum, rows past N get G = 0 (and their X rows are
//      zero-filled in LDS, never loaded).
//   4. phase 2, contraction over rows: A = X^T[f][row] read as ds_read_b32
//      from the same LDS tile (that transpose is why X is staged),
//      B = G fragment (4*KP/16 registers, reused over every feature tile).
//   5. where two tiles fit in LDS the first half is written to the other
//      buffer after phase 1 and the second after phase 2, both loaded under
//      MFMA work; with one buffer the first half waits for the end of phase 2
//      and the second half's load is exposed.
//
// LDS banks (32 four-byte banks; b32 served per 32 lanes, b64 per 16 lanes):
//   stride = T*16 + 2 is 2 or 18 mod 32, an odd multiple of 2, so the 16 rows
//   of a b64 group land on 16 different bank pairs (phase 1).  Phase 2 reads
//   row 8*(q&1) + 4*(q>>1) + j in MFMA j: the two rows of a 32-lane group are
//   8 apart, 8*stride = 16 mod 32, so 2 x 16 contiguous floats cover all 32
//   banks.  The G buffer's stride KP + 2 gives the same property.
//
// Deterministic: no atomics.  Every (block, row group) writes its whole
// partial payload into its own slot, and logreg_wide_reduce_kernel sums the
// slots in f64 in an order fixed by their count.  The grid is min(CUs, block tiles), so results
// depend only on N and the device.  (Deviation from one slot per block: the R
// row groups of a block keep separate accumulators, and summing them through
// LDS would need up to 128 KiB more than the tile leaves; their slots are
// summed by the same ordered f64 pass instead.)

#include <ATen/hip/HIPContext.h>

#include <limits>

#include "common.h"

namespace {

constexpr int kLwThreads = 512;
constexpr int kLwWaves = kLwThreads / 64;
constexpr int kLwNtMax = 8;              // 16-feature tiles per wave
constexpr int kLwLdsBudget = 160 * 1024;
constexpr int kLwMaxK = 32;
constexpr int kLwMaxF = 1024;

typedef float lw_f4 __attribute__((ext_vector_type(4)));
typedef float lw_f2 __attribute__((ext_vector_type(2)));

struct LwPlan {
  bool ok = false;
  int KP = 0;        // padded classes
  int T = 0;         // 16-feature tiles
  int S = 0;         // feature slices
  int log2S = 0;
  int nts = 0;       // tiles per slice
  int NT = 0;        // nts rounded up to a power of two (template size)
  int db = 0;        // two X tiles in LDS
  size_t lds = 0;
};

LwPlan lw_plan(int64_t F, int64_t K) {
  LwPlan p;
  if (K < 2 || K > kLwMaxK || F < 1 || F > kLwMaxF) return p;
  p.KP = K <= 16 ? 16 : 32;
  p.T = (int)ceil_div(F, 16);
  for (int ls = 0; ls <= 3; ++ls) {
    const int S = 1 << ls, R = kLwWaves / S;
    const int nts = (int)ceil_div(p.T, S);
    if (nts > kLwNtMax) continue;
    const size_t xbytes = (size_t)R * 16 * (p.T * 16 + 2) * 4;
    const size_t fixed = (size_t)kLwWaves * 16 * p.KP * 4 +  // partial margins
                         (size_t)R * 16 * (p.KP + 2) * 4 +   // G
                         (size_t)R * 16 * p.KP * 4;          // bias gradient
    if (xbytes + fixed > (size_t)kLwLdsBudget) continue;
    p.S = S; p.log2S = ls; p.nts = nts;
    p.NT = 1;
    while (p.NT < nts) p.NT <<= 1;
    p.db = 2 * xbytes + fixed <= (size_t)kLwLdsBudget;
    p.lds = (p.db ? 2 : 1) * xbytes + fixed;
    p.ok = true;
    break;
  }
  return p;
}

// KP: padded classes; NT: register tiles per wave (>= tiles per slice).
template <int KP, int NT>
__global__ __launch_bounds__(kLwThreads) void logreg_wide_kernel(
    float* __restrict__ slots,       // [grid * R][1 + (F+1)*K]
    const float* __restrict__ x,     // [N, F]
    const int* __restrict__ y,       // [N]
    const float* __restrict__ w,     // [N]
    const float* __restrict__ wmat,  // [F (+1), K]
    int64_t n, int F, int K, int has_bias, int vec, int T, int log2S, int nts,
    int db, int64_t n_tiles) {
  constexpr int CB = KP / 16;   // 16-class blocks
  constexpr int CPL = KP / 4;   // classes per softmax lane
  constexpr int GS = KP + 2;    // G row stride
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int S = 1 << log2S;
  const int R = kLwWaves >> log2S;
  const int s = wv & (S - 1);
  const int g = wv >> log2S;
  const int m16 = lane & 15;
  const int q = lane >> 4;
  const int stride = T * 16 + 2;
  const int RB = R * 16;
  const int xelems = RB * stride;
  float* const xb0 = lds;
  float* const xb1 = db ? lds + xelems : lds;
  float* const mbuf = lds + (db ? 2 : 1) * xelems;  // [R][S][16][KP]
  float* const gbuf = mbuf + kLwWaves * 16 * KP;    // [R][16][GS]
  float* const bacc = gbuf + RB * GS;               // [R][16][KP] bias grad

  const int tile0 = s * nts;
  const int nt = max(0, min(nts, T - tile0));

  // W slice as B-fragments: MFMA (t, h, j) contracts features
  // (tile0+t)*16 + 8h + 2q + j over q
  float wf[NT][2][2][CB];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          const int f = (tile0 + t) * 16 + 8 * h + 2 * q + j;
          const int c = cb * 16 + m16;
          const bool live = t < nt && f < F && c < K;
          const float wv_ = wmat[live ? (int64_t)f * K + c : 0];
          wf[t][h][j][cb] = live ? wv_ : 0.0f;
        }
  lw_f4 gacc[NT][CB];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) gacc[t][cb] = lw_f4{0.f, 0.f, 0.f, 0.f};
  double loss_acc = 0.0;

  // tile staging: float4 i = tid + 512*u of the [RB][C4] tile; (row, col)
  // advance by (512 / C4, 512 % C4) with carry, no division in the loop
  const int C4 = (F + 3) >> 2;
  const int dq = kLwThreads / C4, dr = kLwThreads % C4;
  const int row_init = tid / C4, col_init = tid - row_init * C4;
  // staged in two halves so only NT/2 float4 are ever held in registers
  constexpr int H0 = (NT + 1) / 2;
  lw_f4 pf[H0];
  auto load_half = [&](int64_t row0, int half) {
    int row = row_init + half * H0 * dq, col = col_init + half * H0 * dr;
    row += col / C4; col %= C4;
#pragma unroll
    for (int u = 0; u < H0; ++u) {
      lw_f4 v = lw_f4{0.f, 0.f, 0.f, 0.f};
      if (row < RB && row0 + row < n) {
        const float* p = x + (row0 + row) * F + col * 4;
        if (vec) {
          // each X row is read once per launch: keep it out of the caches
          v = __builtin_nontemporal_load(reinterpret_cast<const lw_f4*>(p));
        } else {
          const int left = F - col * 4;  // >= 1
          v.x = p[0];
          if (left > 1) v.y = p[1];
          if (left > 2) v.z = p[2];
          if (left > 3) v.w = p[3];
        }
      }
      pf[u] = v;
      col += dr; row += dq;
      if (col >= C4) { col -= C4; ++row; }
    }
  };
  auto store_half = [&](float* xb, int half) {
    int row = row_init + half * H0 * dq, col = col_init + half * H0 * dr;
    row += col / C4; col %= C4;
#pragma unroll
    for (int u = 0; u < H0; ++u) {
      if (row < RB) {
        float* d = xb + row * stride + col * 4;  // 8-byte aligned
        *reinterpret_cast<lw_f2*>(d) = lw_f2{pf[u].x, pf[u].y};
        *reinterpret_cast<lw_f2*>(d + 2) = lw_f2{pf[u].z, pf[u].w};
      }
      col += dr; row += dq;
      if (col >= C4) { col -= C4; ++row; }
    }
  };

  // columns past ceil4(F) are never written by store_half: zero them once
  for (int i = tid; i < (db ? 2 : 1) * xelems; i += kLwThreads) lds[i] = 0.0f;
  for (int i = tid; i < RB * KP; i += kLwThreads) bacc[i] = 0.0f;
  __syncthreads();
  int64_t bt = blockIdx.x;  // < n_tiles: the grid never exceeds it
  load_half(bt * RB, 0);
  store_half(xb0, 0);
  load_half(bt * RB, 1);
  store_half(xb0, 1);
  __syncthreads();

  int cur = 0;
  const int prow = 8 * (q & 1) + 4 * (q >> 1);  // phase-2 row of MFMA j = 0
  for (; bt < n_tiles; bt += gridDim.x) {
    const int64_t row0 = bt * RB;
    const int64_t nb = bt + gridDim.x;
    const bool more = nb < n_tiles;
    if (more) load_half(nb * RB, 0);
    const float* xc = cur ? xb1 : xb0;
    float* xn = cur ? xb0 : xb1;

    // phase 1: partial margins of this slice
    lw_f4 macc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) macc[cb] = lw_f4{0.f, 0.f, 0.f, 0.f};
    const float* xrow = xc + (g * 16 + m16) * stride + tile0 * 16 + 2 * q;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t < nt) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const lw_f2 a =
              *reinterpret_cast<const lw_f2*>(xrow + t * 16 + 8 * h);
#pragma unroll
          for (int cb = 0; cb < CB; ++cb) {
            macc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a.x, wf[t][h][0][cb], macc[cb], 0, 0, 0);
            macc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a.y, wf[t][h][1][cb], macc[cb], 0, 0, 0);
          }
        }
      }
    }
    float* mb = mbuf + ((g * S + s) * 16) * KP;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        mb[(4 * q + i) * KP + cb * 16 + m16] = macc[cb][i];
    __syncthreads();

    // softmax, loss, G and bias gradient, once per row: 4 lanes per row
    if (s == 0) {
      const int r = lane >> 2, part = lane & 3;
      const int64_t gr = row0 + g * 16 + r;
      const bool valid = gr < n;
      float v[CPL];
      float mx = -std::numeric_limits<float>::infinity();
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const int cls = part * CPL + c;
        float a = 0.0f;
        for (int s2 = 0; s2 < S; ++s2)  // fixed slice order
          a += mbuf[((g * S + s2) * 16 + r) * KP + cls];
        if (has_bias && cls < K) a += wmat[(int64_t)F * K + cls];
        v[c] = a;
        if (cls < K) mx = fmaxf(mx, v[c]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
      const int yr = valid ? y[gr] : -1;
      const float wr = valid ? w[gr] : 0.0f;
      float e[CPL];
      float se = 0.0f, my = 0.0f;
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const int cls = part * CPL + c;
        e[c] = cls < K ? expf(v[c] - mx) : 0.0f;
        se += e[c];
        if (cls == yr) my = v[c];
      }
      se += __shfl_xor(se, 1, 64);
      se += __shfl_xor(se, 2, 64);
      my += __shfl_xor(my, 1, 64);
      my += __shfl_xor(my, 2, 64);
      if (valid && part == 0)
        loss_acc += (double)(wr * ((mx - my) + logf(se)));
      const float inv = 1.0f / se;
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const int cls = part * CPL + c;
        const float gv =
            valid ? (e[c] * inv - (cls == yr ? 1.0f : 0.0f)) * wr : 0.0f;
        gbuf[(g * 16 + r) * GS + cls] = gv;
        bacc[(g * 16 + r) * KP + cls] += gv;  // this lane's own cell
      }
    }
    // with two buffers the first half lands under phase 1 and the second
    // under the softmax and phase 2
    if (db && more) {
      store_half(xn, 0);
      load_half(nb * RB, 1);
    }
    __syncthreads();

    // phase 2: grad slice += X^T G over the 16 rows
    float gf[4][CB];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
        gf[j][cb] = gbuf[(g * 16 + prow + j) * GS + cb * 16 + m16];
    const float* xcol = xc + (g * 16 + prow) * stride + tile0 * 16 + m16;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t < nt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float a = xcol[j * stride + t * 16];
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            gacc[t][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a, gf[j][cb], gacc[t][cb], 0, 0, 0);
        }
      }
    }
    if (!db) {
      __syncthreads();  // the tile is read to the end of phase 2
      if (more) {
        store_half(xn, 0);
        load_half(nb * RB, 1);
      }
    }
    if (more) store_half(xn, 1);
    __syncthreads();
    if (db) cur ^= 1;
  }

  // every entry of the slot is written exactly once: the slices cover all T
  // tiles, slice 0 writes loss and bias gradient
  const int64_t P = 1 + (int64_t)(F + 1) * K;
  float* slot = slots + ((int64_t)blockIdx.x * R + g) * P;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t < nt) {
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int f = (tile0 + t) * 16 + 4 * q + i;
          const int c = cb * 16 + m16;
          if (f < F && c < K) slot[1 + (int64_t)f * K + c] = gacc[t][cb][i];
        }
    }
  }
  if (s == 0) {
#pragma unroll
    for (int off = 4; off < 64; off <<= 1)
      loss_acc += __shfl_xor(loss_acc, off, 64);
    if (lane == 0) slot[0] = (float)loss_acc;
    if (lane < K) {  // K <= 32: one lane per class, rows in order
      float gb = 0.0f;
      for (int r = 0; r < 16; ++r) gb += bacc[(g * 16 + r) * KP + lane];
      slot[1 + (int64_t)F * K + lane] = has_bias ? gb : 0.0f;
    }
  }
}

// payload[i] = sum over slots in f64, in an order fixed by n_slots alone: 16
// threads per entry each sum a contiguous run of slots in order (one long
// dependent chain measured 0.35 ms at 1256 slots), then the 16 partial sums
// are added in order
__global__ __launch_bounds__(256) void logreg_wide_reduce_kernel(
    float* __restrict__ payload, const float* __restrict__ slots, int n_slots,
    int64_t P) {
  __shared__ double part_sum[16][16];
  const int tx = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int64_t i = (int64_t)blockIdx.x * 16 + tx;
  const int chunk = (n_slots + 15) / 16;
  const int lo = part * chunk, hi = min(n_slots, lo + chunk);
  double a = 0.0;
  if (i < P)
    for (int sl = lo; sl < hi; ++sl) a += (double)slots[sl * P + i];
  part_sum[part][tx] = a;
  __syncthreads();
  if (part == 0 && i < P) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += part_sum[k][tx];
    payload[i] = (float)t;
  }
}

}  // namespace

bool logreg_wide_supported(int64_t F, int64_t K) { return lw_plan(F, K).ok; }

// (KP, S, rows per block tile, LDS bytes, NT, db); all 0 where unsupported
std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>
logreg_wide_geometry(int64_t F, int64_t K) {
  const LwPlan p = lw_plan(F, K);
  if (!p.ok) return {0, 0, 0, 0, 0, 0};
  return {p.KP, p.S, (kLwWaves / p.S) * 16, (int64_t)p.lds, p.NT, p.db};
}

void logreg_loss_grad_wide(torch::Tensor payload, torch::Tensor x,
                           torch::Tensor y, torch::Tensor w,
                           torch::Tensor wmat, bool has_bias) {
  CHECK_GPU(payload); CHECK_GPU(x); CHECK_GPU(y); CHECK_GPU(w);
  CHECK_GPU(wmat);
  CHECK_CONTIG(payload); CHECK_CONTIG(x); CHECK_CONTIG(y);
  CHECK_CONTIG(w); CHECK_CONTIG(wmat);
  TORCH_CHECK(x.dim() == 2 && wmat.dim() == 2, "x and wmat must be 2-d");
  const int64_t n = x.size(0);
  const int F = (int)x.size(1);
  const int K = (int)wmat.size(1);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32 &&
                  w.scalar_type() == torch::kFloat32 &&
                  wmat.scalar_type() == torch::kFloat32 &&
                  payload.scalar_type() == torch::kFloat32,
              "x, w, wmat and payload must be f32");
  TORCH_CHECK(y.scalar_type() == torch::kInt, "y must be int32");
  TORCH_CHECK(n >= 1 && y.numel() == n && w.numel() == n, "row counts");
  TORCH_CHECK(wmat.size(0) == F + (has_bias ? 1 : 0), "wmat rows mismatch");
  const int64_t P = 1 + (int64_t)(F + 1) * K;
  TORCH_CHECK(payload.numel() == P, "payload size");
  const LwPlan p = lw_plan(F, K);
  TORCH_CHECK(p.ok, "unsupported (F, K) for wide logreg: ", F, ", ", K);

  const int R = kLwWaves / p.S;
  const int64_t n_tiles = ceil_div(n, (int64_t)R * 16);
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int grid = (int)std::min<int64_t>(cus, n_tiles);
  const int n_slots = grid * R;
  auto slots = torch::empty({(int64_t)n_slots, P}, payload.options());
  const int vec =
      (F % 4 == 0) && (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0);
  auto stream = at::hip::getCurrentHIPStream();
  bool done = false;
#define LW_LAUNCH(KPP, NTT)                                                   \
  do {                                                                        \
    if (p.lds > 65536)                                                        \
      TORCH_CHECK(                                                            \
          hipFuncSetAttribute(                                                \
              reinterpret_cast<const void*>(&logreg_wide_kernel<KPP, NTT>),   \
              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds) ==      \
              hipSuccess,                                                     \
          "logreg wide: cannot reserve ", p.lds, " bytes of LDS");            \
    hipLaunchKernelGGL((logreg_wide_kernel<KPP, NTT>), dim3(grid),            \
                       dim3(kLwThreads), p.lds, stream,                       \
                       slots.data_ptr<float>(), x.data_ptr<float>(),          \
                       y.data_ptr<int>(), w.data_ptr<float>(),                \
                       wmat.data_ptr<float>(), n, F, K, has_bias ? 1 : 0,     \
                       vec, p.T, p.log2S, p.nts, p.db, n_tiles);              \
    done = true;                                                              \
  } while (0)
  if (p.KP == 16) {
    switch (p.NT) {
      case 1: LW_LAUNCH(16, 1); break;
      case 2: LW_LAUNCH(16, 2); break;
      case 4: LW_LAUNCH(16, 4); break;
      case 8: LW_LAUNCH(16, 8); break;
    }
  } else {
    switch (p.NT) {
      case 1: LW_LAUNCH(32, 1); break;
      case 2: LW_LAUNCH(32, 2); break;
      case 4: LW_LAUNCH(32, 4); break;
      case 8: LW_LAUNCH(32, 8); break;
    }
  }
#undef LW_LAUNCH
  TORCH_CHECK(done, "logreg wide dispatch failed for F=", F, " K=", K);
  hipLaunchKernelGGL(logreg_wide_reduce_kernel, dim3((int)ceil_div(P, 16)),
                     dim3(256), 0, stream, payload.data_ptr<float>(),
                     slots.data_ptr<float>(), n_slots, P);
  // a refused launch must raise: payload is uninitialised memory
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "logreg wide: kernel launch failed: ",
              hipGetErrorString(err));
}
