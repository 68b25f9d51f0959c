// Workgroup primitives of the statistics kernels (PSIS, quantiles, CRPS, calibration, moments, chain diagnostics): the test for
// a finite float, the order-preserving key of a float, the fixed-order fp64 sums and maxima of a wave and of a workgroup, and
// the LDS bitonic network.  One statement of each, so that two kernels that reduce or rank the same values write the same bits.
// Every function that holds a barrier is called by all threads of a one-dimensional workgroup with the same arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= 3.402823466e+38f; }   // false for NaN and +-inf

// the order-preserving 32-bit image of a float, and back (-0 sorts below +0; NaNs land at either end)
__device__ __forceinline__ uint32_t f32_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// sum of v over the wave, the same bits in every lane: the xor butterfly 32 .. 1 (mile_device.h has the fp32 sum of this name)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// Sum and maximum of v over a workgroup of NW waves, the same bits in every thread: the butterfly inside the wave, then the
// waves in index order through red [NW], red[0] first.  (A sum that began at 0.0 would differ only for a total of -0.0, which
// takes every thread's partial at -0.0: a thread's sum that starts at +0.0 never gets there by additions.)
template <int NW>
__device__ __forceinline__ double block_sum(double v, double *red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += red[w];
  __syncthreads();
  return t;
}
template <int NW>
__device__ __forceinline__ double block_max(double v, double *red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t = fmax(t, red[w]);
  __syncthreads();
  return t;
}

// Ascending bitonic network over a[0, n2), n2 a power of two, by nt threads: integer comparisons, a fixed number of stages.
// The caller has synchronised after filling a[]; ends on a barrier.
template <class T>
__device__ static void bitonic(T *a, int n2, int tid, int nt) {
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (n2 >> 1); i += nt) {
        const int l = ((i & ~(j - 1)) << 1) | (i & (j - 1)), r = l | j;
        const T x = a[l], y = a[r];
        if ((x > y) == ((l & k) == 0)) { a[l] = y; a[r] = x; }
      }
      __syncthreads();
    }
}
