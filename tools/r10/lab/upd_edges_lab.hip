// Dev harness (round 10): the two steady-state update launches of a B2 step alone (E = 128, d = 8834, S = 2, 768 threads):
// k_update_fast<3,2,false,MID> with its E noise-prefill workgroups, and <..,REC> reading that noise.  HIP-event time per launch
// and, built with -DMILE_LAB_UPD_EDGES, the s_memtime stamps of thread 0 of particle 0 averaged over the timed launches.
// Prints a bit checksum of (x, u, logp) after a fixed MID / REC sequence: equal between two builds = the same results.
#include "../../../mile_amd/csrc/mile_update.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <cmath>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)
template <class T> static T *dev(size_t n) { T *q; CK(hipMalloc(&q, n * sizeof(T))); CK(hipMemset(q, 0, n * sizeof(T))); return q; }
int main(int argc, char **argv) {
  const int E = argc > 1 ? atoi(argv[1]) : 128, d = argc > 2 ? atoi(argv[2]) : 8834, reps = argc > 3 ? atoi(argv[3]) : 200, S = 2;
  const int dp = (d + 3) & ~3, nt = 768;
  if (d % 2 || ((d >> 2) + 2) / 3 > nt) { printf("this harness is the NK = 3, AL = 2 form\n"); return 1; }
  srand(2);
  auto rnd = []() { return (float)rand() / (float)RAND_MAX * 2.0f - 1.0f; };
  std::vector<float> hx((size_t)E * d), hu((size_t)E * d), hs((size_t)E * S * dp), hl((size_t)E * S), heps(E, 0.02f), hL(E, 1.5f);
  for (auto &v : hx) v = 0.3f * rnd();
  for (int e = 0; e < E; ++e) {
    double n = 0;
    for (int i = 0; i < d; ++i) { hu[(size_t)e * d + i] = rnd(); n += (double)hu[(size_t)e * d + i] * hu[(size_t)e * d + i]; }
    for (int i = 0; i < d; ++i) hu[(size_t)e * d + i] /= (float)std::sqrt(n);
  }
  for (auto &v : hs) v = 5.0f * rnd();
  for (auto &v : hl) v = -300.0f + rnd();
  UpdParams p{};
  p.d = d; p.E = E; p.S = S; p.dp = dp; p.prior = MILE_PRIOR_NORMAL; p.prior_loc = 0.0f; p.prior_scale = 1.0f;
  p.x = dev<float>((size_t)E * d); p.u = dev<float>((size_t)E * d); p.g = dev<float>((size_t)E * d); p.logp = dev<float>(E);
  float *sl = dev<float>((size_t)E * S * dp), *ll = dev<float>((size_t)E * S), *eps = dev<float>(E), *L = dev<float>(E);
  p.slabs = sl; p.llpart = ll; p.eps = eps; p.L = L; p.dK = dev<float>(E); p.lold = dev<float>(E);
  float *nzA = dev<float>((size_t)E * d), *nzB = dev<float>((size_t)E * d), *info = dev<float>((size_t)E * 3);
  long long *dbg = dev<long long>(64);
  p.seed = 1234;
#ifdef MILE_LAB_UPD_EDGES
  p.dbg_buf = dbg;
#endif
  CK(hipMemcpy(p.x, hx.data(), hx.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(p.u, hu.data(), hu.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(sl, hs.data(), hs.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(ll, hl.data(), hl.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(eps, heps.data(), E * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(L, hL.data(), E * 4, hipMemcpyHostToDevice));
  const float b1 = 0.1931833275037836f;
  UpdParams mid = p;    // B(1 - 2 b1) . A(1/2), prefilling the record launch's two noise vectors
  mid.flags = UPD_KIND_MID; mid.coef_b1 = 1.0f - 2.0f * b1; mid.coef_a = 0.5f;
  mid.nz_A = nzA; mid.nz_B = nzB; mid.nz_stepA = 7; mid.nz_stageA = 1; mid.nz_stepB = 8; mid.nz_stageB = 0;
  UpdParams rec = p;    // B(b1) . O(zA) . record . O(zB) . B(b1) . A(1/2)
  rec.flags = UPD_KIND_REC; rec.coef_b1 = b1; rec.coef_b2 = b1; rec.coef_a = 0.5f; rec.hA = 0.5f; rec.hB = 0.5f;
  rec.zA = nzA; rec.zB = nzB; rec.stepA = 7; rec.stageA = 1; rec.stepB = 8; rec.stageB = 0; rec.out_info = info;
  auto kmid = k_update_fast<3, 2, false, UPD_KIND_MID>;
  auto krec = k_update_fast<3, 2, false, UPD_KIND_REC>;
  // results: a fixed sequence from the initial state
  for (int i = 0; i < 5; ++i) { kmid<<<2 * E, nt>>>(mid); krec<<<E, nt>>>(rec); }
  CK(hipDeviceSynchronize());
  std::vector<float> rx((size_t)E * d), ru((size_t)E * d), rl(E);
  CK(hipMemcpy(rx.data(), p.x, rx.size() * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(ru.data(), p.u, ru.size() * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(rl.data(), p.logp, E * 4, hipMemcpyDeviceToHost));
  unsigned cs = 0;
  auto mix = [&](const std::vector<float> &v) { for (float f : v) { unsigned u; memcpy(&u, &f, 4); cs = cs * 2654435761u + u; } };
  mix(rx); mix(ru); mix(rl);
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  float ms[2];
  for (int which = 0; which < 2; ++which) {
    // (the state moves on while timing; restore it so that both kinds see ordinary finite values)
    CK(hipMemcpy(p.x, hx.data(), hx.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(p.u, hu.data(), hu.size() * 4, hipMemcpyHostToDevice));
    kmid<<<2 * E, nt>>>(mid);
    CK(hipDeviceSynchronize());
    CK(hipMemset(dbg, 0, 64 * 8));
    CK(hipEventRecord(e0));
    for (int i = 0; i < reps; ++i) { if (which == 0) kmid<<<2 * E, nt>>>(mid); else krec<<<E, nt>>>(rec); }
    CK(hipEventRecord(e1)); CK(hipDeviceSynchronize());
    CK(hipEventElapsedTime(&ms[which], e0, e1));
    printf("%-16s %s E=%d d=%d us/launch %7.3f  result bits %08x\n", LAB_NAME, which ? "REC" : "MID", E, d, ms[which] / reps * 1e3, cs);
#ifdef MILE_LAB_UPD_EDGES
    long long t[64]; CK(hipMemcpy(t, dbg, 512, hipMemcpyDeviceToHost));
    const double n = t[0] > 0 ? (double)t[0] : 1, mhz = t[10] > 0 ? (double)t[9] / (double)t[10] * 100.0 : 0.0;
    printf("  (%lld launches, %.0f MHz) stamps after entry, us:", t[0], mhz);
    for (int k = 1; k < 10; ++k) printf(" [%d] %.3f", k, t[k] / n / mhz);
    printf("\n      segments, us:");
    for (int k = 1; k < 10; ++k) printf(" %d>%d %.3f", k - 1, k, (t[k] - (k > 1 ? t[k - 1] : 0)) / n / mhz);
    if (which == 0) printf("\n      noise workgroup E, entry to stores acknowledged: %.3f us", t[16] / n / mhz);
    printf("\n");
#endif
  }
  return 0;
}
