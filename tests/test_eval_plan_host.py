"""mile_eval_plan.h on the host: the one tile_rows and the one pass_draws against the formulas they replaced, restated here
literally as the oracle, in a program of its own built with the address and undefined-behaviour sanitizers.  Below that, the
boundary between mile_hip.hip and the evaluation layer (mile_eval.hip behind mile_eval_handle.h), read from the source.

The formulas are integer arithmetic, so the bound is equality, at every point of the grid: S in {1, 2, 31, 32, 33, 12000, 2^20,
2^20 + 1, 2^31 - 1}, N in {1, 31, 32, 33, 301, 1052, 10^5, 2^30 - 1}, C in {1, 3, 128, 1024, 65535} and the caller's cap in {0, 1,
31, 32, 33, 10^9}."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

_MAIN = r'''
#include <stdio.h>
#include <algorithm>
#include "mile_eval_plan.h"
// ---- the formulas before there was one rule, as the statistics had them ----
static const int64_t TARGET = (int64_t)256 << 20, CAL_TARGET = (int64_t)128 << 20;
static const int64_t QNT_TILE = 32, LOO_TILE = 32, CAL_NT = 64, LPPD_J_MAX = 65535, CAL_REC = 48;
static int64_t old_qnt_tile_rows(int64_t S, int64_t N, int64_t max_rows) {
  int64_t nt = std::max<int64_t>(1, TARGET / (S * 16));
  if (nt >= QNT_TILE) nt = nt / QNT_TILE * QNT_TILE;
  if (max_rows > 0) nt = std::min(nt, max_rows);
  return std::min(nt, N);
}
static int64_t old_loo_tile_rows(int64_t S, int64_t N, int64_t max_rows) {
  int64_t nt = std::max<int64_t>(1, TARGET / (S * 8));
  if (nt >= LOO_TILE) nt = nt / LOO_TILE * LOO_TILE;
  if (max_rows > 0) nt = std::min(nt, max_rows);
  return std::min(nt, N);
}
static size_t cal_row_bytes(int C, int K) { return (size_t)C * ((size_t)K * 8 + 4) + (size_t)(C + 1) * CAL_REC; }
static int64_t old_cal_tile_rows(int C, int K, int64_t N, int64_t max_rows) {
  int64_t nt = std::max<int64_t>(1, CAL_TARGET / (int64_t)cal_row_bytes(C, K));
  if (nt >= CAL_NT) nt = nt / CAL_NT * CAL_NT;
  if (max_rows > 0) nt = std::min(nt, max_rows);
  return std::min(nt, N);
}
static int64_t old_cal_pass_draws(int C, int K, int64_t S, int64_t Nt, int64_t max_draws) {
  const int64_t J = max_draws ? max_draws : std::max<int64_t>(1, CAL_TARGET / ((int64_t)C * Nt * K * 4));
  return std::min(J, S);
}
static int64_t old_mixture_quantiles_rows(int64_t S, int64_t N) { return std::min<int64_t>(N, std::max<int64_t>(1, TARGET / (S * 8))); }
static int64_t old_psis_loo_rows(int64_t S, int64_t N) { return std::min<int64_t>(N, std::max<int64_t>(1, TARGET / (S * 4))); }
static int64_t old_moments_pass(int64_t S, int64_t N, int O, int64_t max_draws) {
  const int64_t per_draw = N * O * 4;
  int64_t chunk = max_draws ? max_draws : std::max<int64_t>(1, TARGET / per_draw);
  chunk = std::min<int64_t>(chunk, S);
  return chunk;
}
static int64_t old_lppd_pass(int32_t C, int32_t S, int64_t N, int64_t max_draws) {
  const int64_t per_draw = (int64_t)C * N * 4;
  int64_t J = max_draws ? max_draws : std::max<int64_t>(1, TARGET / per_draw);
  J = std::min<int64_t>(std::min<int64_t>(J, S), LPPD_J_MAX);
  return J;
}
static int64_t old_tile_pass(int64_t S, int64_t max_draws) { return std::min<int64_t>(S, max_draws ? max_draws : S); }

static int bad = 0;
static long long gS, gN, gC, gcap;
#define CHECK(c) do { if (!(c)) { if (bad < 40) printf("line %d: %s fails at S=%lld N=%lld C=%lld cap=%lld\n", __LINE__, #c, gS, gN, gC, gcap); ++bad; } } while (0)
#define SAME_ROWS(now, then) do { const int64_t a = (now), b = (then); CHECK(a == b); CHECK(a >= 1 && a <= N); } while (0)
#define SAME_PASS(now, then) do { const int64_t a = (now), b = (then); CHECK(a == b); CHECK(a >= 1 && a <= S); } while (0)
int main() {
  const int64_t Ss[] = {1, 2, 31, 32, 33, 12000, 1 << 20, (1 << 20) + 1, 0x7fffffff};
  const int64_t Ns[] = {1, 31, 32, 33, 301, 1052, 100000, (1 << 30) - 1};
  const int64_t Cs[] = {1, 3, 128, 1024, 65535};
  const int64_t caps[] = {0, 1, 31, 32, 33, 1000000000};
  static_assert(EVAL_PASS_TARGET == TARGET, "the budget is part of the rule");
  for (int64_t S : Ss) for (int64_t N : Ns) for (int64_t cap : caps) {
    gS = S; gN = N; gC = 0; gcap = cap;
    SAME_ROWS(tile_rows(EVAL_PASS_TARGET, S * 16, QNT_TILE, cap, N), old_qnt_tile_rows(S, N, cap));
    SAME_ROWS(tile_rows(EVAL_PASS_TARGET, S * 8, LOO_TILE, cap, N), old_loo_tile_rows(S, N, cap));
    SAME_ROWS(tile_rows(EVAL_PASS_TARGET, S * 8, 1, 0, N), old_mixture_quantiles_rows(S, N));
    SAME_ROWS(tile_rows(EVAL_PASS_TARGET, S * 4, 1, 0, N), old_psis_loo_rows(S, N));
    SAME_PASS(pass_draws(EVAL_NO_BUDGET, 1, cap, S), old_tile_pass(S, cap));
    for (int O : {2, 3, 10}) SAME_PASS(pass_draws(EVAL_PASS_TARGET, N * O * 4, cap, S), old_moments_pass(S, N, O, cap));
    for (int64_t C : Cs) {
      gC = C;
      SAME_PASS(pass_draws(EVAL_PASS_TARGET, C * N * 4, cap, std::min<int64_t>(S, LPPD_J_MAX)), old_lppd_pass((int32_t)C, (int32_t)S, N, cap));
      for (int K : {2, 3, 64}) {
        const int64_t Nt = tile_rows(CAL_TARGET, (int64_t)cal_row_bytes((int)C, K), CAL_NT, cap, N);
        SAME_ROWS(Nt, old_cal_tile_rows((int)C, K, N, cap));
        for (int64_t draws : caps) SAME_PASS(pass_draws(CAL_TARGET, C * Nt * K * 4, draws, S), old_cal_pass_draws((int)C, K, S, Nt, draws));
      }
    }
  }
  gS = gN = gC = gcap = 0;
  CHECK(r256(0) == 0 && r256(1) == 256 && r256(256) == 256 && r256(257) == 512);
  printf("%s\n", bad ? "FAILED" : "evaluation sizing ok");
  return bad != 0;
}
'''


def test_tile_rows_and_pass_draws_are_the_formulas_they_replaced_under_sanitizers(tmp_path):
    """tile_rows and pass_draws give, at every grid point, the integers of qnt_ / loo_ / cal_tile_rows, of the two unrounded
    tensor-input forms, of cal_pass_draws and of the moments and LPPD pass sizes; 1 <= tile <= N and 1 <= pass <= S; and
    -fsanitize=address,undefined has nothing to report (no overflow at S = 2^31 - 1, N = 2^30 - 1, C = 65535)."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    (tmp_path / 'main.cpp').write_text(_MAIN)
    exe = tmp_path / 'eval_sizing'
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', str(ROOT / 'mile_amd' / 'csrc'), str(tmp_path / 'main.cpp'), '-o', str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and 'evaluation sizing ok' in res.stdout and 'runtime error' not in res.stderr, (res.stdout[-2000:], res.stderr[-2000:])


# ---- the boundary between the sampler's translation unit and the evaluation layer, read from the source --------------------
CSRC = ROOT / 'mile_amd' / 'csrc'
MOVED = ['mile_pointwise_loglik', 'mile_predict', 'mile_predict_moments_width', 'mile_predict_moments', 'mile_mixture_quantiles',
         'mile_predict_quantiles_workspace', 'mile_predict_quantiles', 'mile_debug_quantile_sweeps', 'mile_psis_loo',
         'mile_loo_stream_workspace', 'mile_loo_stream', 'mile_chain_loo_stream_workspace', 'mile_chain_loo_stream', 'mile_mixture_crps',
         'mile_crps_stream_workspace', 'mile_crps_stream', 'mile_stack_eval', 'mile_calibration', 'mile_calibration_stream_workspace',
         'mile_calibration_stream', 'mile_lppd_stream_workspace', 'mile_lppd_stream', 'mile_chain_diagnostics_workspace',
         'mile_chain_diagnostics', 'mile_function_diagnostics_workspace', 'mile_function_diagnostics']


def _code(name):
    """The file without its // comments (none of these files has a string with // in it)."""
    return re.sub(r'//[^\n]*', '', (CSRC / name).read_text())


def test_only_the_samplers_unit_defines_the_handle():
    owners = [p.name for p in sorted(CSRC.iterdir()) if p.suffix in ('.hip', '.h', '.inc') and 'struct mile_sampler {' in p.read_text()]
    assert owners == ['mile_hip.hip']


def test_the_evaluation_layer_includes_no_kernel_header_and_launches_nothing():
    for name in ('mile_eval.hip', 'mile_eval_handle.h'):
        included = re.findall(r'#include\s+"([^"]+)"', (CSRC / name).read_text())
        assert included, name
        banned = [h for h in included if re.search(r'mile_grad_|mile_predict\.h|mile_device\.h|mile_update\.h|mile_nuts\.h', h)]
        assert not banned, (name, banned)
    ev = _code('mile_eval.hip')
    assert '__global__' not in ev and '<<<' not in ev
    assert '"mile_eval_handle.h"' in ev and 's->' not in ev   # the handle is an incomplete type there: nothing of it is read


def test_every_evaluation_entry_point_moved_out_of_the_samplers_unit():
    hip, ev = _code('mile_hip.hip'), _code('mile_eval.hip')
    for fn in MOVED:
        definition = re.compile(r'\b(?:int32_t|int64_t)\s+' + fn + r'\s*\(')
        assert not definition.search(hip), fn
        assert len(definition.findall(ev)) == 1, fn
    for helper in ('forward_draws', 'forward_chains', 'evaluate_rows', 'eval_args', 'with_call_ws'):
        assert not re.search(r'\b' + helper + r'\s*\(', hip), helper
    for stays in ('stage_rows', 'eval_forward', 'reserve_eval_ws', 'k_pad_x<<<'):
        assert stays in hip, stays
