// gbm_round_prologue: everything a dim-1 gradient-boosting round needs from
// its rows before the tree grows, in one pass.
//   per row:   g = d loss / d pred (scalar_loss_grad, as grad_hess_kernel),
//              grad = weight * (-g), gh[i] = (grad, weight[, 1]), grad[i]
//   per block: max |grad|, NaN kept as torch.amax keeps it
//   then a one-block fixed-order reduce of the block maxima (no atomics)
// It replaces grad_hess + neg + mul + cat + abs + amax of the composed round
// (spark_ensemble_amd/ops/reference.py gbm_round_prologue).  The gradient SUM
// is deliberately not taken here: its summation order is part of the fitted
// model, so the caller keeps torch's reduction over the grad this writes.
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "gbm_loss.h"

namespace {

constexpr int kPrologueThreads = 256;
constexpr int kPrologueMaxBlocks = 8192;

// max that keeps a NaN once it has one (fmaxf would drop it)
__device__ inline float nan_max(float m, float a) {
  return (a > m || a != a) ? a : m;
}

template <bool UNIT>
__global__ void gbm_round_prologue_kernel(
    float* __restrict__ gh,            // [N, UNIT ? 2 : 3]
    float* __restrict__ grad,          // [N]
    float* __restrict__ partials,      // [gridDim.x]
    const float* __restrict__ label,   // [N]
    const float* __restrict__ pred,    // [N]
    const float* __restrict__ weight,  // [N], not read when UNIT
    int64_t n, int loss_id, float param) {
  __shared__ float wmax[kPrologueThreads / 64];
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  float m = 0.0f;
  for (; i < n; i += stride) {
    float g, h;
    scalar_loss_grad(loss_id, param, label[i], pred[i], &g, &h);
    const float w = UNIT ? 1.0f : weight[i];
    const float v = w * (-g);
    if (UNIT) {
      reinterpret_cast<float2*>(gh)[i] = make_float2(v, 1.0f);
    } else {
      float* row = gh + i * 3;
      row[0] = v;
      row[1] = w;
      row[2] = 1.0f;
    }
    grad[i] = v;
    m = nan_max(m, fabsf(v));
  }
  for (int off = 32; off > 0; off >>= 1)
    m = nan_max(m, __shfl_down(m, off, 64));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = wmax[0];
    for (int k = 1; k < kPrologueThreads / 64; ++k) v = nan_max(v, wmax[k]);
    partials[blockIdx.x] = v;
  }
}

// one block; lane j takes partials j, j + 256, ... and thread 0 the 256 lanes
__global__ void gbm_round_max_kernel(float* __restrict__ out,
                                     const float* __restrict__ partials,
                                     int n_blocks) {
  __shared__ float lp[kPrologueThreads];
  float m = 0.0f;
  for (int b = threadIdx.x; b < n_blocks; b += kPrologueThreads)
    m = nan_max(m, partials[b]);
  lp[threadIdx.x] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = lp[0];
    for (int j = 1; j < kPrologueThreads; ++j) v = nan_max(v, lp[j]);
    out[0] = v;
  }
}

}  // namespace

std::tuple<int64_t, int64_t> gbm_round_prologue_geometry(int64_t n) {
  return {kPrologueThreads,
          std::min<int64_t>(ceil_div(n, kPrologueThreads),
                            kPrologueMaxBlocks)};
}

void gbm_round_prologue(torch::Tensor gh, torch::Tensor grad,
                        torch::Tensor gmax, torch::Tensor label,
                        torch::Tensor pred, torch::Tensor weight,
                        int64_t loss_id, double param, bool unit_weight) {
  CHECK_GPU(gh); CHECK_GPU(grad); CHECK_GPU(gmax); CHECK_GPU(label);
  CHECK_GPU(pred); CHECK_GPU(weight);
  CHECK_CONTIG(gh); CHECK_CONTIG(grad); CHECK_CONTIG(gmax);
  CHECK_CONTIG(label); CHECK_CONTIG(pred); CHECK_CONTIG(weight);
  const int64_t n = pred.numel();
  const int64_t C = unit_weight ? 2 : 3;
  TORCH_CHECK(loss_id >= 0 && loss_id <= L_BERNOULLI && loss_id != L_LOGLOSS,
              "gbm_round_prologue: scalar losses only");
  TORCH_CHECK(n > 0, "gbm_round_prologue: no rows");
  TORCH_CHECK(label.numel() == n && grad.numel() == n &&
                  gh.numel() == n * C && gmax.numel() >= 1 &&
                  (unit_weight || weight.numel() == n),
              "gbm_round_prologue: sizes");
  for (const torch::Tensor& t : {gh, grad, gmax, label, pred, weight})
    TORCH_CHECK(t.scalar_type() == torch::kFloat32,
                "gbm_round_prologue: float32 tensors");
  // the unit-weight kernel stores gh rows as float2
  TORCH_CHECK(reinterpret_cast<uintptr_t>(gh.data_ptr<float>()) % 8 == 0,
              "gbm_round_prologue: gh must be 8-byte aligned");
  auto stream = at::hip::getCurrentHIPStream();
  const int blocks = (int)std::get<1>(gbm_round_prologue_geometry(n));
  auto partials = torch::empty({(int64_t)blocks}, gmax.options());
#define PROLOGUE_LAUNCH(U)                                                   \
  hipLaunchKernelGGL(gbm_round_prologue_kernel<U>, dim3(blocks),             \
                     dim3(kPrologueThreads), 0, stream,                      \
                     gh.data_ptr<float>(), grad.data_ptr<float>(),           \
                     partials.data_ptr<float>(), label.data_ptr<float>(),    \
                     pred.data_ptr<float>(), weight.data_ptr<float>(), n,    \
                     (int)loss_id, (float)param)
  if (unit_weight) PROLOGUE_LAUNCH(true); else PROLOGUE_LAUNCH(false);
#undef PROLOGUE_LAUNCH
  hipLaunchKernelGGL(gbm_round_max_kernel, dim3(1), dim3(kPrologueThreads), 0,
                     stream, gmax.data_ptr<float>(),
                     partials.data_ptr<float>(), blocks);
}
