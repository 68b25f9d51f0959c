// The likelihood head of one row, in a header of its own: the evaluation kernels (mile_predict.h) and the function-space
// diagnostics (mile_fdiag.hip) both include it, and the latter needs nothing else of the forward kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mile_hip.h"

// The likelihood head of every evaluation kernel that does not share it with a backward pass: log p(y[row] | z) for the K head
// outputs z of one row -- Normal(mu, sigma clipped to [1e-6, 1e6]) of z = (mu, log sigma), or log-softmax(z) at the label.
__device__ __forceinline__ float row_loglik(const float *z, int K, int task, const void *y, long long row) {
  if (task == MILE_TASK_REGRESSION) {
    const float es = expf(z[1]);
    const float sig = isnan(es) ? es : fminf(fmaxf(es, 1e-6f), 1e6f);
    const float r = (((const float *)y)[row] - z[0]) / sig;
    return -0.5f * r * r - logf(sig) - 0.91893853320467274f;
  }
  const int yi = ((const int32_t *)y)[row];
  float m = z[0];
  for (int c = 1; c < K; ++c) m = fmaxf(m, z[c]);
  float se = 0.0f;
  for (int c = 0; c < K; ++c) se += expf(z[c] - m);
  return z[yi] - (m + logf(se));
}
