"""mile_layer_plan.h on the host: the one LayerPlan against the three computations it replaced -- the geometry loop of
launch_grad_wide<TERMS>, the one of launch_fwd_wide and lenet_dense_dims with the ldin of lenet_dense_chunk -- restated here
literally as the oracle, and against the up8 / offsets restatement of tests/wide_schedule.py, in a program of its own built with
the address and undefined-behaviour sanitizers.

The plan is integer arithmetic, so the bound is equality of every per-layer field, of wt_elems for TERMS 1 and 3, of the widest
padded width and of per_row, at every point of the grid: F in {1, 5, 54, 130} with Fp = F rounded up to 8 as mile_set_data does,
the hidden structures below; flat in {16, 400, 576} and K in {1, 2, 10, 17} for LeNet."""
import shutil
import subprocess
from pathlib import Path

import pytest

from tests import wide_schedule as W

ROOT = Path(__file__).resolve().parent.parent
MAX_LAYERS = 16                                                   # MILE_MAX_LAYERS (the program asserts it)
FS = (1, 5, 54, 130)
HIDDEN = ((96, 4), (24, 17, 2), (129, 127, 1), (200, 136, 3), (256, 256, 256, 256, 7),
          (40, 33, 24, 17, 9, 96, 8, 7, 130, 12, 64, 5, 31, 16, 100, 3))
assert len(HIDDEN[-1]) == MAX_LAYERS

_MAIN = r'''
#include <stdio.h>
#include <algorithm>
#include "mile_layer_plan.h"
static_assert(MILE_MAX_LAYERS == @MAX_LAYERS@, "the grid's deepest net has MILE_MAX_LAYERS layers");
// what the launchers read of DevSpec and LeNetGeom
struct DevSpec { int n_layers, in_features, widths[MILE_MAX_LAYERS], w_off[MILE_MAX_LAYERS], b_off[MILE_MAX_LAYERS]; };
struct LeNetGeom { int K, flat, b_f1, k_f1, b_f2, k_f2, b_f3, k_f3; };

static int bad = 0;
static const char *what = "";
static long long gF, gi, gl;
#define CHECK(c) do { if (!(c)) { if (bad < 40) printf("line %d: %s fails for %s at F/flat=%lld net/K=%lld layer=%lld\n", __LINE__, #c, what, gF, gi, gl); ++bad; } } while (0)

// ---- the three computations before there was one plan, as the launchers had them ----
template <int TERMS>
static void old_grad_wide(const DevSpec &ds, int Fp) {
  const LayerPlan pl = layer_plan_fcn(ds, Fp, TERMS);
  const int L = ds.n_layers;
  auto up8 = [](int v) { return (v + 7) / 8 * 8; };
  int wp[MILE_MAX_LAYERS], fin[MILE_MAX_LAYERS], finp[MILE_MAX_LAYERS];
  size_t per_row = 0, wt_elems = 0, wt_off[MILE_MAX_LAYERS];
  int maxwp = 0;
  for (int l = 0; l < L; ++l) {
    wp[l] = up8(ds.widths[l]);
    fin[l] = l == 0 ? ds.in_features : ds.widths[l - 1];
    finp[l] = l == 0 ? Fp : wp[l - 1];
    per_row += wp[l];
    maxwp = std::max(maxwp, wp[l]);
    wt_off[l] = wt_elems;
    wt_elems += (size_t)TERMS * fin[l] * wp[l];
  }
  per_row += 2 * (size_t)maxwp;
  what = TERMS == 3 ? "launch_grad_wide<3>" : "launch_grad_wide<1>";
  CHECK(pl.L == L && pl.terms == TERMS && pl.maxwp == maxwp && pl.per_row() == per_row && pl.wt_elems == wt_elems);
  for (int l = 0; l < L; ++l) {
    gl = l;
    CHECK(pl.wp[l] == wp[l] && pl.fin[l] == fin[l] && pl.ldin[l] == finp[l] && pl.fout[l] == ds.widths[l]);
    CHECK(pl.wt_off[l] == wt_off[l] && pl.plane(l) == (size_t)((long long)fin[l] * wp[l]));
    CHECK(pl.w_off[l] == ds.w_off[l] && pl.b_off[l] == ds.b_off[l]);
  }
  gl = -1;
}
static void old_fwd_wide(const DevSpec &ds, int Fp, const LayerPlan &pl) {
  const int L = ds.n_layers;
  auto up8 = [](int v) { return (v + 7) / 8 * 8; };
  int wp[MILE_MAX_LAYERS], fin[MILE_MAX_LAYERS];
  size_t wt_elems = 0, wt_off[MILE_MAX_LAYERS];
  int maxwp = 0;
  for (int l = 0; l < L; ++l) {
    wp[l] = up8(ds.widths[l]);
    fin[l] = l == 0 ? ds.in_features : ds.widths[l - 1];
    maxwp = std::max(maxwp, wp[l]);
    wt_off[l] = wt_elems;
    wt_elems += (size_t)3 * fin[l] * wp[l];
  }
  what = "launch_fwd_wide";
  CHECK(pl.L == L && pl.maxwp == maxwp && pl.wt_elems == wt_elems);
  for (int l = 0; l < L; ++l) {
    gl = l;
    CHECK(pl.wp[l] == wp[l] && pl.fin[l] == fin[l] && pl.fout[l] == ds.widths[l] && pl.wt_off[l] == wt_off[l]);
    CHECK(pl.ldin[l] == (l == 0 ? Fp : wp[l - 1]));              // its lda, written in place: Fp, else wp[l - 1]
    CHECK(pl.plane(l) == (size_t)((long long)fin[l] * wp[l]));   // its tB
  }
  gl = -1;
}
static void lenet_dense_dims(const LeNetGeom &g, int (&fin)[3], int (&fout)[3], int (&ld)[3], int (&woff)[3], int (&boff)[3], size_t (&pl)[3],
                             size_t &elems) {
  fin[0] = g.flat; fin[1] = 120; fin[2] = 84;
  fout[0] = 120; fout[1] = 84; fout[2] = g.K;
  woff[0] = g.k_f1; woff[1] = g.k_f2; woff[2] = g.k_f3;
  boff[0] = g.b_f1; boff[1] = g.b_f2; boff[2] = g.b_f3;
  elems = 0;
  for (int l = 0; l < 3; ++l) { ld[l] = (fout[l] + 7) / 8 * 8; pl[l] = elems; elems += (size_t)3 * fin[l] * ld[l]; }
}
static void old_lenet(const LeNetGeom &g, const LayerPlan &p) {
  int fin[3], fout[3], ld[3], woff[3], boff[3]; size_t pl[3], elems;
  lenet_dense_dims(g, fin, fout, ld, woff, boff, pl, elems);
  const int ldin[3] = {g.flat, ld[0], ld[1]};                    // lenet_dense_chunk
  what = "lenet_dense_dims";
  CHECK(p.L == 3 && p.terms == 3 && p.wt_elems == elems && p.maxwp == std::max({ld[0], ld[1], ld[2]}));
  for (int l = 0; l < 3; ++l) {
    gl = l;
    CHECK(p.fin[l] == fin[l] && p.fout[l] == fout[l] && p.wp[l] == ld[l] && p.ldin[l] == ldin[l]);
    CHECK(p.w_off[l] == woff[l] && p.b_off[l] == boff[l] && p.wt_off[l] == pl[l] && p.plane(l) == (size_t)((long long)fin[l] * ld[l]));
  }
  gl = -1;
}

// ---- tests/wide_schedule.py's restatement of the same nets: up8, offsets, the per-row floats of layout_rows ----
struct Expect { int F, L, hidden[MILE_MAX_LAYERS], wp[MILE_MAX_LAYERS], b_off[MILE_MAX_LAYERS], w_off[MILE_MAX_LAYERS]; long long per_row, d; };
static const Expect EXPECT[] = {
@EXPECT@
};

int main() {
  int net = 0;
  for (const Expect &x : EXPECT) {
    gF = x.F; gi = net++; gl = -1;
    DevSpec ds{};
    ds.n_layers = x.L; ds.in_features = x.F;
    long long off = 0;                                           // layout_fcn without the sort by layer name: bias before kernel
    for (int l = 0; l < x.L; ++l) {
      ds.widths[l] = x.hidden[l];
      ds.b_off[l] = (int)off; off += x.hidden[l];
      ds.w_off[l] = (int)off; off += (long long)(l ? x.hidden[l - 1] : x.F) * x.hidden[l];
    }
    const int Fp = (x.F + 7) / 8 * 8;                            // mile_set_data
    const LayerPlan pl = layer_plan_fcn(ds, Fp, 3);
    old_grad_wide<3>(ds, Fp);
    old_grad_wide<1>(ds, Fp);
    old_fwd_wide(ds, Fp, pl);
    what = "tests/wide_schedule.py";
    CHECK(off == x.d && (long long)pl.per_row() == x.per_row);
    for (int l = 0; l < x.L; ++l) {
      gl = l;
      CHECK(pl.wp[l] == x.wp[l] && pl.b_off[l] == x.b_off[l] && pl.w_off[l] == x.w_off[l]);
    }
  }
  for (int flat : {16, 400, 576}) for (int K : {1, 2, 10, 17}) {
    gF = flat; gi = K; gl = -1;
    LeNetGeom g{};
    g.flat = flat; g.K = K;
    long long o = 6 + 25 * 6 + 16 + 150 * 16;                    // layout_lenet behind the two convolutions of a one-channel image
    g.b_f1 = (int)o; o += 120; g.k_f1 = (int)o; o += (long long)flat * 120;
    g.b_f2 = (int)o; o += 84;  g.k_f2 = (int)o; o += 120LL * 84;
    g.b_f3 = (int)o; o += K;   g.k_f3 = (int)o; o += 84LL * K;
    old_lenet(g, layer_plan_lenet(g));
  }
  printf("%s\n", bad ? "FAILED" : "layer plan ok");
  return bad != 0;
}
'''


def _expect():
    """The FCN grid as tests/wide_schedule.py restates it, printed into the program's source."""
    def arr(v):
        return '{' + ', '.join(str(int(i)) for i in v) + '}'
    rows = []
    for F in FS:
        for hs in HIDDEN:
            b_off, w_off, d, _ = W.offsets(W._c('plan', F, hs, 'relu', 'classification', 1))
            wp = [W.up8(w) for w in hs]
            per_row = sum(wp) + 2 * max(wp)                       # layout_rows
            rows.append(f'  {{{F}, {len(hs)}, {arr(hs)}, {arr(wp)}, {arr(b_off)}, {arr(w_off)}, {per_row}, {d}}},')
    return '\n'.join(rows)


def test_layer_plan_is_the_three_computations_it_replaced_under_sanitizers(tmp_path):
    """layer_plan_fcn and layer_plan_lenet give, at every grid point, the integers of the gradient's loop (TERMS 1 and 3), of the
    evaluation's loop and of lenet_dense_dims, and those of tests/wide_schedule.py; -fsanitize=address,undefined has nothing to
    report (no array of the plan is indexed past MILE_MAX_LAYERS layers)."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    assert W.layout_rows((256,) * 4 + (7,), 128, 232404) == (int(W.WS_GB * (1 << 30) / 4) // (128 * (4 * 256 + 8 + 2 * 256))) // 128 * 128
    (tmp_path / 'main.cpp').write_text(_MAIN.replace('@MAX_LAYERS@', str(MAX_LAYERS)).replace('@EXPECT@', _expect()))
    exe = tmp_path / 'layer_plan'
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', str(ROOT / 'mile_amd' / 'csrc'), str(tmp_path / 'main.cpp'), '-o', str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and 'layer plan ok' in res.stdout and 'runtime error' not in res.stderr, (res.stdout[-2000:], res.stderr[-2000:])
