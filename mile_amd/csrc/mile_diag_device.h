// Device helpers of the chain-diagnostics kernels (mile_diag.hip, mile_dtail.hip): the normal quantile, the fp32 key of the
// (key, index) words that mile_block.h's bitonic network sorts, and the tie-averaged normal score of a sorted position.  One
// statement of each, so that two kernels that rank the same draws write the same bits.  The fixed-order wave and workgroup sums
// are mile_block.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mile_block.h"

// ---- normal quantile ---------------------------------------------------------------------------------------------------
// x <= 0 with Phi(x) = q for q in (0, 0.5]: Acklam's rational approximation (relative error 1.2e-9), then two Halley
// steps on Phi(x) - q through erfc, which leave fp64 rounding error only.  The caller hands in the SMALLER tail, so the
// upper half loses nothing to 1 - p.
__host__ __device__ static inline double diag_ndtri_lower(double q) {
  double x;
  if (q < 0.02425) {
    const double t = sqrt(-2.0 * log(q));
    x = (((((-7.784894002430293e-03 * t - 3.223964580411365e-01) * t - 2.400758277161838e+00) * t - 2.549732539343734e+00) * t +
          4.374664141464968e+00) * t + 2.938163982698783e+00) /
        ((((7.784695709041462e-03 * t + 3.224671290700398e-01) * t + 2.445134137142996e+00) * t + 3.754408661907416e+00) * t + 1.0);
  } else {
    const double t = q - 0.5, r = t * t;
    x = (((((-3.969683028665376e+01 * r + 2.209460984245205e+02) * r - 2.759285104469687e+02) * r + 1.383577518672690e+02) * r -
          3.066479806614716e+01) * r + 2.506628277459239e+00) * t /
        (((((-5.447609879822406e+01 * r + 1.615858368580409e+02) * r - 1.556989798598866e+02) * r + 6.680131188771972e+01) * r -
          1.328068155288572e+01) * r + 1.0);
  }
  for (int it = 0; it < 2; ++it) {
    const double e = 0.5 * erfc(-x * 0.70710678118654752440) - q;
    const double u = e * 2.50662827463100050242 * exp(0.5 * x * x);
    x -= u / (1.0 + 0.5 * x * u);
  }
  return x;
}
// ndtri((rank - 0.375) / (n + 0.25)), rank in [1, n]
__host__ __device__ static inline double diag_score(double rank, int n) {
  const double den = (double)n + 0.25, p = (rank - 0.375) / den;
  return p <= 0.5 ? diag_ndtri_lower(p) : -diag_ndtri_lower(((double)n + 0.625 - rank) / den);
}

// ---- sorting -----------------------------------------------------------------------------------------------------------
// fp32 -> uint32 with the same order (-0 counts as +0, as in a float comparison); NaNs land at either end and are dealt
// with by the callers before any rank is used.
__device__ __forceinline__ uint32_t diag_key(float x) {
  if (x == 0.0f) x = 0.0f;
  return f32_key(x);
}

// Normal score of sorted position i of the n real entries: the average of the ranks of its tie group, whose ends come
// from two bounded binary searches (taken only when a neighbour holds the same key).
__device__ static double diag_rank_score(const uint64_t *a, int n, int i) {
  const uint32_t key = (uint32_t)(a[i] >> 32);
  int lo = i, hi = i + 1;
  if (i > 0 && (uint32_t)(a[i - 1] >> 32) == key) {
    int b = 0, e = i;
    while (b < e) { const int m = (b + e) >> 1; if ((uint32_t)(a[m] >> 32) < key) b = m + 1; else e = m; }
    lo = b;
  }
  if (i + 1 < n && (uint32_t)(a[i + 1] >> 32) == key) {
    int b = i + 1, e = n;
    while (b < e) { const int m = (b + e) >> 1; if ((uint32_t)(a[m] >> 32) <= key) b = m + 1; else e = m; }
    hi = b;
  }
  return diag_score(0.5 * (double)(lo + hi + 1), n);     // ranks lo+1 .. hi
}
