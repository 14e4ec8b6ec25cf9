// forest_contrib: per-row additive feature contributions (path-dependent
// TreeSHAP) of a packed tree ensemble, for gfx950.
//
// The host packs every root-to-leaf path into its UNIQUE-feature elements
// (docs/contributions.md): element e carries a feature id, the merged
// interval (lo, hi] the row's value must fall in, and z_e, the product of
// child/parent covers over the merged nodes.  With o_e = [x in (lo, hi]] the
// path adds to the feature of element e
//
//     v * (o_e - z_e) * S_e,
//     S_e = sum_k k!(m-1-k)!/m! [t^k] prod_{j != e} (z_j + o_j t)
//         = integral_0^1 prod_{j != e} (z_j (1-s) + o_j s) ds
//
// (k!(m-1-k)!/m! is the Beta integral of s^k (1-s)^(m-1-k)).  The integrand
// is a polynomial of degree m-1 in s, so a Gauss-Legendre rule with G/2
// nodes is exact for every m <= G.  Every factor and every quadrature
// weight is positive: no term cancels, unlike the divide-out of an
// EXTEND/UNWIND recurrence.
//
// Mapping.  A block owns (row tile, plane): it stages the tile's R rows of x
// in LDS as f32 next to an [R][F] i64 fixed-point accumulator, loops over all
// of the plane's paths, and writes the tile once with plain coalesced
// stores.  No global atomics.  A path occupies one lane GROUP of G = 8, 16
// or 32 lanes of the 64-wide wave, one element per lane (paths are sorted by
// plane and by group width, so the 64/G paths of a wave share G).  A lane
// keeps its element in registers and walks the tile's rows; per row and
// quadrature node the product over the other lanes of the group is a
// log2(G)-step butterfly that carries the block product and the product
// excluding the lane's own factor, so nothing is divided out.
//
// Accumulation.  ds_add_f32 is instruction-rate bound on gfx950 (the first
// version of this kernel spent its time there: profiles/tree_contrib.md, as
// profiles/r01_hist_probe.md found for the histograms), ds_add_u64 runs at
// ds_write speed.  So each f32 term is scaled by a power of two chosen on
// the host from the bound  |sum of a cell's terms| <= 2 sum_t |w_t| max|leaf_t|
// (per tree and feature the path terms are v_p times a difference of two
// probability distributions over the leaves), rounded to an integer below
// 2^51 with the 1.5 * 2^52 double trick, and added as i64.  Integer adds
// commute, so the result does not depend on the order in which lane groups
// reach a cell: it is bitwise reproducible, and its only roundings are the
// terms' own and the final i64 -> f32.  The bias column is row-independent
// and is filled in by the caller.

#include <ATen/hip/HIPContext.h>

#include <cmath>

#include "common.h"

namespace {

constexpr int kContribThreads = 1024;
constexpr int kFeatMask = 0x00FFFFFF;
constexpr int kHasLo = 1 << 29;
constexpr int kHasHi = 1 << 30;

// Gauss-Legendre rules on [0, 1]: nodes s, their complements a = 1 - s
// (rounded from the double value, not computed in f32) and weights w.
template <int Q> struct GaussLegendre;
template <> struct GaussLegendre<4> {
  static constexpr float s[4] = {6.943184420e-02f, 3.300094782e-01f,
                                 6.699905218e-01f, 9.305681558e-01f};
  static constexpr float a[4] = {9.305681558e-01f, 6.699905218e-01f,
                                 3.300094782e-01f, 6.943184420e-02f};
  static constexpr float w[4] = {1.739274226e-01f, 3.260725774e-01f,
                                 3.260725774e-01f, 1.739274226e-01f};
};
template <> struct GaussLegendre<8> {
  static constexpr float s[8] = {
      1.985507175e-02f, 1.016667613e-01f, 2.372337950e-01f, 4.082826788e-01f,
      5.917173212e-01f, 7.627662050e-01f, 8.983332387e-01f, 9.801449282e-01f};
  static constexpr float a[8] = {
      9.801449282e-01f, 8.983332387e-01f, 7.627662050e-01f, 5.917173212e-01f,
      4.082826788e-01f, 2.372337950e-01f, 1.016667613e-01f, 1.985507175e-02f};
  static constexpr float w[8] = {
      5.061426815e-02f, 1.111905172e-01f, 1.568533229e-01f, 1.813418917e-01f,
      1.813418917e-01f, 1.568533229e-01f, 1.111905172e-01f, 5.061426815e-02f};
};
template <> struct GaussLegendre<16> {
  static constexpr float s[16] = {
      5.299532504e-03f, 2.771248846e-02f, 6.718439881e-02f, 1.222977958e-01f,
      1.910618778e-01f, 2.709916112e-01f, 3.591982246e-01f, 4.524937451e-01f,
      5.475062549e-01f, 6.408017754e-01f, 7.290083888e-01f, 8.089381222e-01f,
      8.777022042e-01f, 9.328156012e-01f, 9.722875115e-01f, 9.947004675e-01f};
  static constexpr float a[16] = {
      9.947004675e-01f, 9.722875115e-01f, 9.328156012e-01f, 8.777022042e-01f,
      8.089381222e-01f, 7.290083888e-01f, 6.408017754e-01f, 5.475062549e-01f,
      4.524937451e-01f, 3.591982246e-01f, 2.709916112e-01f, 1.910618778e-01f,
      1.222977958e-01f, 6.718439881e-02f, 2.771248846e-02f, 5.299532504e-03f};
  static constexpr float w[16] = {
      1.357622971e-02f, 3.112676197e-02f, 4.757925584e-02f, 6.231448563e-02f,
      7.479799441e-02f, 8.457825970e-02f, 9.130170752e-02f, 9.472530523e-02f,
      9.472530523e-02f, 9.130170752e-02f, 8.457825970e-02f, 7.479799441e-02f,
      6.231448563e-02f, 4.757925584e-02f, 3.112676197e-02f, 1.357622971e-02f};
};

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  // every lane has a source lane under these controls, so neither `old` nor
  // bound_ctrl matters; full masks + bound_ctrl let the move fold into the
  // multiply that consumes it
  const int i = __float_as_int(v);
  return __int_as_float(
      __builtin_amdgcn_update_dpp(i, i, CTRL, 0xF, 0xF, true));
}

// Butterfly step over lane groups of width G: every lane of an aligned block
// of D lanes reads v from a lane of the SIBLING block (the other half of the
// aligned 2D block).  Callers only pass values that are equal across a
// D-block, so which lane of the sibling answers does not matter: the mirrors
// (lane i <-> 7-i, i <-> 15-i) stand in for xor 4 and xor 8, which DPP lacks.
template <int D, int G>
__device__ __forceinline__ float sibling_block(float v) {
  static_assert(D < G && G <= 32, "step stays inside the lane group");
  if constexpr (D == 1) return dpp_f32<0xB1>(v);        // quad_perm [1,0,3,2]
  else if constexpr (D == 2) return dpp_f32<0x4E>(v);   // quad_perm [2,3,0,1]
  else if constexpr (D == 4) return dpp_f32<0x141>(v);  // row_half_mirror
  else if constexpr (D == 8) return dpp_f32<0x140>(v);  // row_mirror
  else return __shfl_xor(v, D, G);                      // D == 16, G == 32
}

// Product of f over the OTHER lanes of the lane group of width G.
template <int G>
__device__ __forceinline__ float group_product_excl(float f) {
  float incl = f, excl = 1.0f;
#define CONTRIB_STEP(D)                                      \
  if constexpr (D < G) {                                     \
    const float t = sibling_block<(D < G ? D : 1), G>(incl); \
    excl *= t;                                               \
    incl *= t;                                               \
  }
  CONTRIB_STEP(1)
  CONTRIB_STEP(2)
  CONTRIB_STEP(4)
  CONTRIB_STEP(8)
  CONTRIB_STEP(16)
#undef CONTRIB_STEP
  return excl;
}

// All paths [p0, p1) of one (plane, group width) against the staged tile.
template <int G>
__device__ __forceinline__ void contrib_bucket(
    const float* __restrict__ xs, unsigned long long* __restrict__ acc,
    int rows, int F, double scale, int p0, int p1,
    const int* __restrict__ path_off, const int* __restrict__ path_m,
    const float* __restrict__ path_v,
    const int* __restrict__ e_feat, const float* __restrict__ e_lo,
    const float* __restrict__ e_hi, const float* __restrict__ e_z) {
  constexpr int Q = G / 2;
  constexpr int PPW = 64 / G;  // paths per wave
  using GL = GaussLegendre<Q>;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n_waves = blockDim.x >> 6;
  const int sub = lane / G;
  const int li = lane % G;

  // wave-uniform loop bounds: every lane of the wave runs every shuffle
  for (int base = p0 + wave * PPW; base < p1; base += n_waves * PPW) {
    const int p = base + sub;
    int m = 0, off = 0;
    float v = 0.0f;
    if (p < p1) {
      m = path_m[p];
      off = path_off[p];
      v = path_v[p];
    }
    const bool active = li < m;
    int ff = 0;
    float lo = 0.0f, hi = 0.0f, z = 0.0f;
    if (active) {
      ff = e_feat[off + li];
      lo = e_lo[off + li];
      hi = e_hi[off + li];
      z = e_z[off + li];
    }
    // the packer checks every id against F; the clamp keeps a bad table
    // from reaching past the tile all the same
    const int feat = min(ff & kFeatMask, F - 1);
    const bool has_lo = (ff & kHasLo) != 0;
    const bool has_hi = (ff & kHasHi) != 0;
    const float c_in = v * (1.0f - z);  // v * (o - z) for o = 1
    const float c_out = -v * z;         //               for o = 0

    float x_next = xs[feat];
    for (int r = 0; r < rows; ++r) {
      // the next row's value is fetched under this row's arithmetic
      const float xv = x_next;
      x_next = xs[min(r + 1, rows - 1) * F + feat];
      const bool o = (!has_lo || xv > lo) && (!has_hi || xv <= hi);
      float S = 0.0f;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        float f = fmaf(z, GL::a[q], o ? GL::s[q] : 0.0f);
        f = active ? f : 1.0f;
        S = fmaf(GL::w[q], group_product_excl<G>(f), S);
      }
      if (active) {
        // rint(term * scale) as i64: |term * scale| < 2^51 by the host's
        // bound, so adding 1.5 * 2^52 leaves the integer in the mantissa
        const double d = (double)((o ? c_in : c_out) * S) * scale;
        const long long q =
            __double_as_longlong(d + 6755399441055744.0) - 0x4338000000000000LL;
        atomicAdd(&acc[r * F + feat], (unsigned long long)q);
      }
    }
  }
}

__global__ __launch_bounds__(kContribThreads) void forest_contrib_kernel(
    float* __restrict__ out, const float* __restrict__ x,
    const int* __restrict__ ranges,  // [num_planes][4] bucket starts + end
    const int* __restrict__ path_off, const int* __restrict__ path_m,
    const float* __restrict__ path_v, const int* __restrict__ e_feat,
    const float* __restrict__ e_lo, const float* __restrict__ e_hi,
    const float* __restrict__ e_z, int64_t n, int F, int R, int num_planes,
    double scale, double inv_scale) {
  extern __shared__ __align__(16) unsigned long long lds[];
  unsigned long long* acc = lds;                // [R][F] i64 contributions
  float* xs = (float*)(lds + (size_t)R * F);    // [R][F] staged rows
  const int plane = blockIdx.y;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int rows = (int)min((int64_t)R, n - row0);
  const int cells = rows * F;

  const float* xt = x + row0 * F;  // the tile's rows are contiguous
  for (int i = threadIdx.x; i < cells; i += blockDim.x) {
    xs[i] = xt[i];
    acc[i] = 0ull;
  }
  __syncthreads();

  const int* rg = ranges + plane * 4;
  contrib_bucket<8>(xs, acc, rows, F, scale, rg[0], rg[1], path_off, path_m,
                    path_v, e_feat, e_lo, e_hi, e_z);
  contrib_bucket<16>(xs, acc, rows, F, scale, rg[1], rg[2], path_off, path_m,
                     path_v, e_feat, e_lo, e_hi, e_z);
  contrib_bucket<32>(xs, acc, rows, F, scale, rg[2], rg[3], path_off, path_m,
                     path_v, e_feat, e_lo, e_hi, e_z);
  __syncthreads();

  // out is [n, num_planes, F + 1]; column F (bias) belongs to the caller
  for (int i = threadIdx.x; i < cells; i += blockDim.x) {
    const int r = i / F;
    const int f = i - r * F;
    out[((row0 + r) * num_planes + plane) * (int64_t)(F + 1) + f] =
        (float)((double)(long long)acc[i] * inv_scale);
  }
}

}  // namespace

// LDS bytes of a tile of R rows: [R][F] i64 accumulators and [R][F] f32 of x
static size_t contrib_lds_bytes(int64_t R, int64_t F) {
  return (size_t)R * (size_t)F * (sizeof(long long) + sizeof(float));
}

void forest_contrib(torch::Tensor out, torch::Tensor x, torch::Tensor ranges,
                    torch::Tensor path_off, torch::Tensor path_m,
                    torch::Tensor path_v, torch::Tensor e_feat,
                    torch::Tensor e_lo, torch::Tensor e_hi, torch::Tensor e_z,
                    int64_t rows_per_tile, double scale) {
  CHECK_GPU(out); CHECK_GPU(x); CHECK_GPU(ranges); CHECK_GPU(path_off);
  CHECK_GPU(path_m); CHECK_GPU(path_v); CHECK_GPU(e_feat); CHECK_GPU(e_lo);
  CHECK_GPU(e_hi); CHECK_GPU(e_z);
  CHECK_CONTIG(out); CHECK_CONTIG(x); CHECK_CONTIG(ranges);
  CHECK_CONTIG(path_off); CHECK_CONTIG(path_m); CHECK_CONTIG(path_v);
  CHECK_CONTIG(e_feat); CHECK_CONTIG(e_lo); CHECK_CONTIG(e_hi);
  CHECK_CONTIG(e_z);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32 && x.dim() == 2,
              "forest_contrib: x is [N, F] f32");
  TORCH_CHECK(out.scalar_type() == torch::kFloat32 && out.dim() == 3,
              "forest_contrib: out is [N, planes, F + 1] f32");
  TORCH_CHECK(ranges.scalar_type() == torch::kInt32 &&
                  path_off.scalar_type() == torch::kInt32 &&
                  path_m.scalar_type() == torch::kInt32 &&
                  e_feat.scalar_type() == torch::kInt32,
              "forest_contrib: index tables are int32");
  TORCH_CHECK(path_v.scalar_type() == torch::kFloat32 &&
                  e_lo.scalar_type() == torch::kFloat32 &&
                  e_hi.scalar_type() == torch::kFloat32 &&
                  e_z.scalar_type() == torch::kFloat32,
              "forest_contrib: value tables are f32");
  const int64_t n = x.size(0);
  const int64_t F = x.size(1);
  const int64_t planes = out.size(1);
  const int64_t R = rows_per_tile;
  TORCH_CHECK(out.size(0) == n && out.size(2) == F + 1,
              "forest_contrib: out does not match x");
  TORCH_CHECK(ranges.numel() == planes * 4,
              "forest_contrib: ranges is [planes, 4]");
  TORCH_CHECK(planes >= 1 && planes <= 65535, "forest_contrib: plane count");
  TORCH_CHECK(F >= 1 && F <= kFeatMask, "forest_contrib: feature count");
  TORCH_CHECK(path_m.numel() == path_off.numel() &&
                  path_v.numel() == path_off.numel(),
              "forest_contrib: path tables differ in length");
  TORCH_CHECK(e_lo.numel() == e_feat.numel() &&
                  e_hi.numel() == e_feat.numel() &&
                  e_z.numel() == e_feat.numel(),
              "forest_contrib: element tables differ in length");
  const size_t lds = contrib_lds_bytes(R, F);
  TORCH_CHECK(R >= 1 && lds <= 163840,
              "forest_contrib: row tile does not fit the LDS");
  TORCH_CHECK(scale > 0.0 && std::isfinite(scale) && std::isfinite(1.0 / scale),
              "forest_contrib: fixed-point scale");
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  if (lds > 65536)
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(&forest_contrib_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(
      forest_contrib_kernel,
      dim3((unsigned)ceil_div(n, R), (unsigned)planes), dim3(kContribThreads),
      lds, stream, out.data_ptr<float>(), x.data_ptr<float>(),
      ranges.data_ptr<int>(), path_off.data_ptr<int>(),
      path_m.data_ptr<int>(), path_v.data_ptr<float>(),
      e_feat.data_ptr<int>(), e_lo.data_ptr<float>(), e_hi.data_ptr<float>(),
      e_z.data_ptr<float>(), n, (int)F, (int)R, (int)planes, scale,
      1.0 / scale);
}
