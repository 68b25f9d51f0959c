// Chan's merge of two Welford records, shared by the statistics that fold draws per column (mile_sens.hip, mile_pdp.hip).
#pragma once
#include <hip/hip_runtime.h>

// (nb, mb, M2b) into (na, ma, M2a); nb > 0
__device__ __forceinline__ void chan_merge(int &na, double &ma, double &M2a, int nb, double mb, double M2b) {
  if (na == 0) { na = nb; ma = mb; M2a = M2b; return; }
  const double nt = (double)na + (double)nb, delta = mb - ma;
  ma += delta * ((double)nb / nt);
  M2a += M2b + delta * delta * ((double)na * (double)nb / nt);
  na += nb;
}
