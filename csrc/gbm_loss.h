// Device forms of the GBM losses, shared by csrc/ops.hip (grad_hess,
// line_search_eval) and csrc/forest_staged.hip (per-stage loss curves).
//   loss ids match spark_ensemble_amd/boosting/losses.py LOSS_IDS
#pragma once

#include <hip/hip_runtime.h>

#define L_SQUARED 0
#define L_ABSOLUTE 1
#define L_LOGCOSH 2
#define L_SCALEDLOGCOSH 3
#define L_HUBER 4
#define L_QUANTILE 5
#define L_LOGLOSS 6
#define L_EXPONENTIAL 7
#define L_BERNOULLI 8

__device__ inline float logcosh_f(float d) {
  float a = fabsf(d);
  return a + log1pf(__expf(-2.0f * a)) - 0.6931471805599453f;
}

// scalar (dim=1) losses: returns loss, writes d(loss)/d(pred) and hessian
__device__ inline float scalar_loss_grad(int loss_id, float param, float y,
                                         float p, float* grad, float* hess) {
  switch (loss_id) {
    case L_SQUARED: {
      float d = y - p;
      *grad = -d;
      *hess = 1.0f;
      return 0.5f * d * d;
    }
    case L_ABSOLUTE: {
      float d = y - p;
      // -sign(d) with sign(+-0) = 0, as losses.py (torch.sign) and the
      // reference (math.signum): an exact tie has pseudo-residual 0
      *grad = (d > 0.0f) ? -1.0f : ((d < 0.0f) ? 1.0f : 0.0f);
      *hess = 0.0f;
      return fabsf(d);
    }
    case L_LOGCOSH: {
      float d = y - p;
      float t = tanhf(d);
      *grad = -t;
      *hess = 1.0f - t * t;
      return logcosh_f(d);
    }
    case L_SCALEDLOGCOSH: {
      float d = y - p;
      float s = (y > p) ? param : 1.0f - param;
      float t = tanhf(d);
      *grad = -s * t;
      *hess = s * (1.0f - t * t);
      return s * logcosh_f(d);
    }
    case L_HUBER: {
      float d = y - p;
      float ad = fabsf(d);
      if (ad <= param) {
        *grad = -d;
        *hess = 1.0f;
        return 0.5f * d * d;
      }
      *grad = -param * copysignf(1.0f, d);
      *hess = 0.0f;
      return param * (ad - 0.5f * param);
    }
    case L_QUANTILE: {
      float d = y - p;
      *grad = (d > 0.0f) ? -param : (1.0f - param);
      *hess = 0.0f;
      return (d > 0.0f) ? param * d : (param - 1.0f) * d;
    }
    case L_EXPONENTIAL: {
      // y in {-1, 1}.  expf, not __expf: the loss IS the exponential, so
      // the fast form's relative error (~|y p| * 2^-24 from rounding
      // y p * log2(e)) reaches loss, gradient and hessian undamped, about
      // 5e-6 at |y p| = 80 (profiles/loss_kernels.md)
      float e = expf(-y * p);
      *grad = -y * e;
      *hess = e;  // y^2 = 1
      return e;
    }
    case L_BERNOULLI: {
      // overflow-safe forms: exp(z) -> inf past |z|~88 made the naive
      // hess 4e/(1+e)^2 = inf/inf = NaN once boosting margins grow,
      // kicking the stage-weight search from 3-6 Newton evals to ~25
      // Brent evals per round (measured +4 ms/round after round ~40).
      // sigmoid(-z) = t/(1+t) with t = exp(-|z|) in (0,1] is finite
      // everywhere; grad = -2y*sigmoid(-z), hess = 4*sig*(1-sig).
      float z = 2.0f * y * p;
      float az = fabsf(z);
      float t = __expf(-az);
      float sig_neg = (z >= 0.0f) ? t / (1.0f + t) : 1.0f / (1.0f + t);
      *grad = -2.0f * y * sig_neg;
      *hess = 4.0f * sig_neg * (1.0f - sig_neg);
      return fmaxf(-z, 0.0f) + log1pf(t);
    }
  }
  *grad = 0.0f;
  *hess = 0.0f;
  return 0.0f;
}

// Softmax cross-entropy of one row, -sum_d label_d * log softmax(pred)_d, in
// the max-shifted log-sum-exp form.  expf / logf, not the fast forms: this
// is the evaluated loss itself, not a line-search objective whose minimiser
// is all that matters.  csrc/ops.hip deliberately does NOT use this helper:
// line_search_eval_kernel and grad_hess_kernel keep their inline softmax
// with __expf / __logf, fused with the gradient terms they need from the
// same exponentials, so the fits they drive stay bit for bit what they were.
// Only csrc/forest_staged.hip evaluates a loss for its own sake.
template <int D>
__device__ inline float softmax_xent(const float* label, const float* pred) {
  float m = pred[0];
#pragma unroll
  for (int d = 1; d < D; ++d) m = fmaxf(m, pred[d]);
  float s = 0.0f;
#pragma unroll
  for (int d = 0; d < D; ++d) s += expf(pred[d] - m);
  const float lse = m + logf(s);
  float l = 0.0f;
#pragma unroll
  for (int d = 0; d < D; ++d) l += -label[d] * (pred[d] - lse);
  return l;
}
