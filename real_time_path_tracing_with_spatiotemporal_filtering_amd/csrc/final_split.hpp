// final_split.hpp — the layout of a tracing launch that carries the previous frame's final filter pass (kernels.hip:
// k_pathtrace_final), stated once: how the host cuts the pass's work list into two groups of filter workgroups
// (final_split_plan), which tile columns it serves in runs of tiles (final_full_columns, final_run) and which role a workgroup of
// that grid has (final_role).  Plain C++ that the host, the kernel and csrc/tests/final_split_host_check.cpp and
// empty_runs_host_check.cpp all compile; it includes nothing of HIP.
//
// One grid, four groups of workgroups in dispatch order (= order of blockIdx.x):
//
//   [ n_front filter | n_tiles tracing tiles | n_runs run workgroups | n_tail filter ]
//
// The front group owns items [0, front_items) of the pass's work list, the tail group items [front_items, items); a group that
// owns no item has no workgroup.  Every tile and every item has exactly one owner and no workgroup waits for another.
//
// Run workgroups: the tiles are dispatched column by column from the middle of the frame outwards (tile_order_column), so the
// columns that no triangle's screen bounds reach (final_full_columns: the host has the bounds anyway) sit in one block at the end
// of the order.  Their tiles trace one ray per pixel into the sky or the light and live 3.5 us each; a launch of them runs at the
// rate at which workgroups start and retire, not at the rate of its arithmetic.  With run_len > 0 the tiles of the first
// full_cols columns of the order are ordinary tile workgroups, n_tiles = full_cols x tiles_y of them, and every later column is
// cut into runs of run_len vertically consecutive tiles (the last run of a column is shorter), one workgroup each (final_run).
// With n_runs = 0 — no such column, or runs turned off — the launch is the three groups it was before.
//
// (A third filter group — the second one dispatched in front of the tile columns that see only sky, the last ones dispatched — was
// built and measured, profiles/r19_final_place_ab.txt: at every share it beat the same share behind the last tile and lost
// to the whole list in front, so it is not here.  DESIGN §7 has the numbers.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RTPT_FS_HD __host__ __device__
#else
#define RTPT_FS_HD
#endif

namespace rt {

struct FinalSplit {
  uint32_t n_front, n_tail;      // workgroups, multiples of 8 (0: the group owns no item)
  uint32_t front_items, items;   // of the final pass's work list
  uint32_t tiles_x, n_tiles;     // the tile grid is tiles_x columns wide; n_tiles tile workgroups: the whole grid (tiles_x x
                                 // PathtraceArgs::tiles_y) without runs, the first full_cols columns of the order with them
  uint32_t n_runs, run_len;      // run workgroups (0: none) of at most run_len tiles each
  uint32_t runs_per_col, tiles_y;  // runs a column is cut into (ceil(tiles_y / run_len)); rows of the tile grid.  0 without runs
};

enum : uint32_t { kFinalRoleTile = 0, kFinalRoleFront = 1, kFinalRoleTail = 2, kFinalRoleRun = 3 };
struct FinalRole {
  uint32_t role;   // kFinalRole*
  uint32_t index;  // tile: its place in the tiles' dispatch order; run, filter: the workgroup's number within its group
};

// workgroup `block` of a grid of final_grid(sp) workgroups
RTPT_FS_HD inline FinalRole final_role(const FinalSplit& sp, uint32_t block) {
  const uint32_t t = block - sp.n_front;  // (unsigned: a front workgroup wraps past the tiles)
  if (t < sp.n_tiles) return FinalRole{kFinalRoleTile, t};
  if (block < sp.n_front) return FinalRole{kFinalRoleFront, block};
  const uint32_t u = t - sp.n_tiles;
  if (u < sp.n_runs) return FinalRole{kFinalRoleRun, u};
  return FinalRole{kFinalRoleTail, u - sp.n_runs};
}
RTPT_FS_HD inline uint32_t final_grid(const FinalSplit& sp) { return sp.n_front + sp.n_tiles + sp.n_runs + sp.n_tail; }

// The tile column (0 = leftmost) that is `col`-th in the dispatch order of a grid tiles_x columns wide: the middle one first,
// then alternately right and left of it (pathtrace_tile.hpp computes its bx_ the same way)
RTPT_FS_HD inline uint32_t tile_order_column(uint32_t tiles_x, uint32_t col) {
  return (col & 1u) ? (tiles_x - 1u) / 2u + (col + 1u) / 2u : (tiles_x - 1u) / 2u - col / 2u;
}

// run workgroup `index` (FinalRole::index of a kFinalRoleRun): tiles [row0, row0 + rows) of tile column `column`
struct FinalRun {
  uint32_t column, row0, rows;
};
RTPT_FS_HD inline FinalRun final_run(const FinalSplit& sp, uint32_t index) {
  const uint32_t c = index / sp.runs_per_col, row0 = (index - c * sp.runs_per_col) * sp.run_len;
  const uint32_t left = sp.tiles_y - row0;
  return FinalRun{tile_order_column(sp.tiles_x, sp.n_tiles / sp.tiles_y + c), row0, left < sp.run_len ? left : sp.run_len};
}

// The columns of the order that stay ordinary tiles: one past the last column, in dispatch order, that some triangle's padded
// screen bounds reach within frame rows [y0, y1) of a frame W pixels wide (tile column bx holds pixel columns [64 bx,
// min(64 bx + 64, W))).  bounds[i].{x0, y0, x1, y1} are inclusive pixel bounds (kernels.hpp: TriBounds; x0 > x1 marks a
// triangle no primary ray can hit).  No primary ray of a later column can hit a triangle; an unreached column in front of a
// reached one stays a column of tiles.  tiles_x: the last column of the order is reached; 0: no column is.
constexpr int kTileColumnPixels = 64;
template <class Bounds>
inline uint32_t final_full_columns(const Bounds* bounds, uint32_t n, int W, int y0, int y1, uint32_t tiles_x) {
  for (uint32_t col = tiles_x; col > 0; col--) {
    const int cx0 = static_cast<int>(tile_order_column(tiles_x, col - 1u)) * kTileColumnPixels;
    const int cx1 = (cx0 + kTileColumnPixels < W ? cx0 + kTileColumnPixels : W) - 1;
    for (uint32_t i = 0; i < n; i++) {
      const Bounds& b = bounds[i];
      if (b.x0 > b.x1) continue;
      if (!(b.x0 > cx1 || b.x1 < cx0 || b.y0 > y1 - 1 || b.y1 < y0)) return col;
    }
  }
  return 0u;
}

// The groups of a launch (FilterPolicy: RTPT_FINAL_FRONT=<front>[,<share>]).
//   front   the front group's size: 0 none; 1 .. per_cu - 1 that many workgroups per CU; per_cu and above a TOTAL number of
//           workgroups, rounded down to a multiple of 8 and capped at per_cu - 1 per CU
//   share   percent of the work list the front group owns (the tail group owns the rest); < 0: the built-in choice — the whole
//           list where it has at least kFinalWholeListItems items per workgroup the front group may have, 75 % below that.
//           Measured at two sizes (profiles/r19_final_place_ab.txt, 256 workgroups in front): a 4K frame, 63 items per
//           workgroup, loses 2.5 us of a 405 us launch to a tail group of any size from 3 % on and 8 us to one of 25 %; a
//           1080p frame, 16 items per workgroup, gains 1.7 us of 112 with the 25 % tail, step by step from 100 % down to 80 %.
//           The threshold is the geometric middle of the two; nothing between them has been measured.
// n_cu compute units, per_cu resident workgroups of either kind on one.  A group takes every slot it may hold, dealt in per-XCD
// runs (workgroup b runs on XCD b & 7), but no more workgroups than an XCD's eighth of its range has items.
constexpr uint32_t kFinalWholeListItems = 32;
inline FinalSplit final_split_plan(uint32_t items, uint32_t tiles_x, uint32_t tiles_y, uint32_t n_cu, uint32_t per_cu, int front, int share) {
  const uint32_t cu8 = (n_cu + 7u) / 8u;
  auto clamp = [](int v, uint32_t hi) { return v < 0 ? 0u : (static_cast<uint32_t>(v) > hi ? hi : static_cast<uint32_t>(v)); };
  const uint32_t front_max = cu8 * (per_cu - 1u);  // slots per XCD
  uint32_t front_slots = front <= 0 ? 0u : (static_cast<uint32_t>(front) < per_cu ? cu8 * static_cast<uint32_t>(front) : static_cast<uint32_t>(front) / 8u);
  front_slots = front_slots < front_max ? front_slots : front_max;
  FinalSplit sp;
  sp.tiles_x = tiles_x;
  sp.n_tiles = tiles_x * tiles_y;
  sp.items = items;
  if (share < 0) share = items >= kFinalWholeListItems * 8u * front_slots ? 100 : 75;
  sp.front_items = front_slots ? static_cast<uint32_t>(static_cast<uint64_t>(items) * clamp(share, 100u) / 100u) : 0u;
  auto group = [](uint32_t n_items, uint32_t slots_per_xcd) {
    const uint32_t per_xcd = (n_items + 7u) / 8u;
    return n_items ? 8u * (per_xcd < slots_per_xcd ? per_xcd : slots_per_xcd) : 0u;
  };
  sp.n_front = group(sp.front_items, front_slots);
  sp.n_tail = group(items - sp.front_items, cu8 * per_cu - front_slots);
  sp.n_runs = sp.run_len = sp.runs_per_col = sp.tiles_y = 0u;
  return sp;
}

// The same launch with the columns of the order from full_cols on (final_full_columns) served in runs of run_len tiles
// (FilterPolicy: RTPT_EMPTY_RUN).  run_len 0, or no column behind full_cols: the launch above, member for member.
inline FinalSplit final_split_plan(uint32_t items, uint32_t tiles_x, uint32_t tiles_y, uint32_t n_cu, uint32_t per_cu, int front, int share,
                                   uint32_t full_cols, uint32_t run_len) {
  FinalSplit sp = final_split_plan(items, tiles_x, tiles_y, n_cu, per_cu, front, share);
  if (run_len == 0u || full_cols >= tiles_x || tiles_y == 0u) return sp;
  run_len = run_len < tiles_y ? run_len : tiles_y;
  sp.n_tiles = full_cols * tiles_y;
  sp.run_len = run_len;
  sp.runs_per_col = (tiles_y + run_len - 1u) / run_len;
  sp.tiles_y = tiles_y;
  sp.n_runs = (tiles_x - full_cols) * sp.runs_per_col;
  return sp;
}

}  // namespace rt
