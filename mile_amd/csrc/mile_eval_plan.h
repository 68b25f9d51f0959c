// The sizing rules that the evaluation statistics share on the host: how many rows a tile takes, how many draws a pass takes,
// and the 256-byte rounding of every block of a workspace.  Plain C++17, nothing from HIP: host tests include this file alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

static const int64_t EVAL_PASS_TARGET = (int64_t)256 << 20;   // bytes of a pass's (or tile's) forward outputs and their copies when the caller leaves the choice
static const int64_t EVAL_NO_BUDGET = INT64_MAX;              // as a budget at 1 byte per item: only the caller's cap and the extent bind

static inline size_t r256(size_t b) { return (b + 255) / 256 * 256; }

// Rows of a tile: as many as `budget` bytes hold at `per_row` bytes each, at least one; whole multiples of `quantum` once there
// is one (1: no rounding); at most max_rows where the caller gives one (> 0); at most the N rows there are.
static inline int64_t tile_rows(int64_t budget, int64_t per_row, int64_t quantum, int64_t max_rows, int64_t N) {
  int64_t nt = budget / per_row;
  if (nt < 1) nt = 1;
  if (nt >= quantum) nt = nt / quantum * quantum;
  if (max_rows > 0 && nt > max_rows) nt = max_rows;
  return nt < N ? nt : N;
}
// Draws of a pass: the caller's max_draws where given (> 0), else as many as `budget` bytes hold at `per_draw` bytes each, at
// least one; at most the S draws there are.
static inline int64_t pass_draws(int64_t budget, int64_t per_draw, int64_t max_draws, int64_t S) {
  int64_t j = max_draws ? max_draws : budget / per_draw;
  if (j < 1) j = 1;
  return j < S ? j : S;
}
