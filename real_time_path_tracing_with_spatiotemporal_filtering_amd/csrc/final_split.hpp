// final_split.hpp — the layout of a tracing launch that carries the previous frame's final filter pass (kernels.hip:
// k_pathtrace_final), stated once: how the host cuts the pass's work list into two groups of filter workgroups
// (final_split_plan) and which role a workgroup of that grid has (final_role).  Plain C++ that the host, the kernel and
// csrc/tests/final_split_host_check.cpp all compile; it includes nothing of HIP.
//
// One grid, three runs of workgroups in dispatch order (= order of blockIdx.x):
//
//   [ n_front filter | n_tiles tracing tiles | n_tail filter ]
//
// The front group owns items [0, front_items) of the pass's work list, the tail group items [front_items, items); a group that
// owns no item has no workgroup.  Every tile and every item has exactly one owner and no workgroup waits for another.
//
// (A fourth run — the second group dispatched in front of the tile columns that see only sky, the last ones dispatched — was
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
  uint32_t tiles_x, n_tiles;     // the tile grid is tiles_x x PathtraceArgs::tiles_y = n_tiles tiles
};

enum : uint32_t { kFinalRoleTile = 0, kFinalRoleFront = 1, kFinalRoleTail = 2 };
struct FinalRole {
  uint32_t role;   // kFinalRole*
  uint32_t index;  // tile: its place in the tiles' dispatch order; filter: the workgroup's number within its group
};

// workgroup `block` of a grid of final_grid(sp) workgroups
RTPT_FS_HD inline FinalRole final_role(const FinalSplit& sp, uint32_t block) {
  const uint32_t t = block - sp.n_front;  // (unsigned: a front workgroup wraps past the tiles)
  if (t < sp.n_tiles) return FinalRole{kFinalRoleTile, t};
  if (block < sp.n_front) return FinalRole{kFinalRoleFront, block};
  return FinalRole{kFinalRoleTail, t - sp.n_tiles};
}
RTPT_FS_HD inline uint32_t final_grid(const FinalSplit& sp) { return sp.n_front + sp.n_tiles + sp.n_tail; }

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
  return sp;
}

}  // namespace rt
