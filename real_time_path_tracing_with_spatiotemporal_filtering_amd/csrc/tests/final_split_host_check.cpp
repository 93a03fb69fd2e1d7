// final_split_host_check.cpp — a plain C++ program (no HIP, no device) over final_split.hpp: the layout of the tracing launch
// that carries the previous frame's final filter pass.  For every frame and policy of the lists below it builds the launch's
// FinalSplit as the host does and walks the whole grid with final_role, the function the kernel calls:
//   * every block index has exactly one role, the tiles come out in dispatch order and each exactly once;
//   * every item of the pass's work list is taken by exactly one filter workgroup (the dealing inside a group is restated here
//     from atrous_comb.hpp: comb_items, ROLE: XCD x = b & 7 owns the x-th eighth of the group's range, its workgroups take
//     every (workgroups / 8)-th item of it);
//   * a group has a multiple of 8 workgroups, or none, and none exactly when it owns no item;
//   * with the front group given per CU the launch is the one that was written before this header existed, restated below.
// `make -C csrc final-split-host-check` builds it with -fsanitize=address,undefined and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../final_split.hpp"

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

using namespace rt;

// the launch as kernels.hip stated it before this header (front group per CU only), and its kernel's test for a tile
struct Parent {
  uint32_t n_front, n_tail, front_items, items;
};
static Parent parent_split(uint32_t items, uint32_t n_cu, uint32_t per_cu, int front, int share) {
  const uint32_t cu8 = (n_cu + 7u) / 8u;
  auto clamp = [](int v, int hi) { return static_cast<uint32_t>(v < 0 ? 0 : (v > hi ? hi : v)); };
  const uint32_t front_wg = clamp(front, static_cast<int>(per_cu) - 1), sh = clamp(share, 100);
  Parent p;
  p.items = items;
  p.front_items = front_wg ? static_cast<uint32_t>(static_cast<uint64_t>(items) * sh / 100u) : 0u;
  auto group = [&](uint32_t n, uint32_t slots_per_xcd) {
    const uint32_t per_xcd = (n + 7u) / 8u;
    return n ? 8u * (per_xcd < slots_per_xcd ? per_xcd : slots_per_xcd) : 0u;
  };
  p.n_front = group(p.front_items, cu8 * front_wg);
  p.n_tail = group(items - p.front_items, cu8 * (per_cu - front_wg));
  return p;
}

// the items workgroup b of a group of nb workgroups takes from [lo, hi): comb_items' loop
static void take_items(std::vector<uint8_t>& owner, uint32_t b, uint32_t nb, uint32_t lo, uint32_t hi) {
  const uint32_t nlb = hi - lo, xcd = b & 7u, jx = b >> 3, per_xcd = nb >> 3;
  const uint32_t x_lo = lo + static_cast<uint32_t>((static_cast<uint64_t>(nlb) * xcd) >> 3);
  const uint32_t x_hi = lo + static_cast<uint32_t>((static_cast<uint64_t>(nlb) * (xcd + 1)) >> 3);
  CHECK(per_xcd > 0);
  for (uint32_t lb = x_lo + jx; lb < x_hi; lb += per_xcd) {
    CHECK(lb < owner.size());
    CHECK(owner[lb] == 0);
    owner[lb] = 1;
  }
}

static unsigned long long g_grids = 0, g_blocks = 0;

static void check_grid(const FinalSplit& sp) {
  CHECK(sp.n_front % 8u == 0 && sp.n_tail % 8u == 0);
  CHECK(sp.front_items <= sp.items);
  CHECK((sp.n_front == 0) == (sp.front_items == 0));
  CHECK((sp.n_tail == 0) == (sp.items == sp.front_items));
  const uint32_t grid = final_grid(sp);
  CHECK(grid == sp.n_front + sp.n_tail + sp.n_tiles);
  std::vector<uint8_t> tile(sp.n_tiles, 0), item(sp.items, 0), wg_front(sp.n_front, 0), wg_tail(sp.n_tail, 0);
  for (uint32_t b = 0; b < grid; b++) {
    const FinalRole r = final_role(sp, b);
    switch (r.role) {
      case kFinalRoleTile:
        CHECK(r.index < sp.n_tiles && !tile[r.index] && b == sp.n_front + r.index);  // in dispatch order, between the groups
        tile[r.index] = 1;
        break;
      case kFinalRoleFront:
        CHECK(b < sp.n_front && r.index == b && !wg_front[r.index]);
        wg_front[r.index] = 1;
        take_items(item, r.index, sp.n_front, 0u, sp.front_items);
        break;
      case kFinalRoleTail:
        CHECK(r.index < sp.n_tail && !wg_tail[r.index] && b == sp.n_front + sp.n_tiles + r.index);
        wg_tail[r.index] = 1;
        take_items(item, r.index, sp.n_tail, sp.front_items, sp.items);
        break;
      default:
        CHECK(!"a role outside the three");
    }
  }
  for (uint8_t v : tile) CHECK(v == 1);
  for (uint8_t v : item) CHECK(v == 1);
  for (uint8_t v : wg_front) CHECK(v == 1);
  for (uint8_t v : wg_tail) CHECK(v == 1);
  g_grids++;
  g_blocks += grid;
}

int main() {
  const int widths[] = {1, 63, 64, 65, 200, 257, 3840}, heights[] = {1, 4, 5, 37, 83, 2160};
  const int share[] = {-1 /* left out: the built-in choice */, 0, 1, 50, 99, 100, 250};
  const uint32_t cus[] = {256, 304, 1}, per_cu = 8;
  const int k = 5, comb_m = 2, sh_waves = 4;  // the final pass of N = 5 (atrous.hip: comb_list)
  for (int W : widths)
    for (int H : heights) {
      const uint32_t tiles_x = (W + 63) / 64, tiles_y = (H + 3) / 4, n_tiles = tiles_x * tiles_y;
      const uint32_t chunks = (H + comb_m * k - 1) / (comb_m * k);
      const uint32_t items = tiles_x * ((chunks + sh_waves - 1) / sh_waves) * k;
      // front: none (and a negative value), 1, 2 and 7 per CU, totals of 8, 128, 192, 256, 512 workgroups, more workgroups than
      // there are items (twice)
      const int front[] = {-1, 0, 1, 2, 7, 8, 128, 192, 256, 512, static_cast<int>(items) + 8, 1 << 20};
      for (uint32_t n_cu : cus)
        for (int f : front)
          for (int s : share) {
            const FinalSplit sp = final_split_plan(items, tiles_x, tiles_y, n_cu, per_cu, f, s);
            CHECK(sp.tiles_x == tiles_x && sp.n_tiles == n_tiles && sp.items == items);
            CHECK(sp.n_front <= 8u * ((n_cu + 7u) / 8u) * (per_cu - 1u));
            if (f >= static_cast<int>(per_cu)) CHECK(sp.n_front <= static_cast<uint32_t>(f));  // a total is a ceiling
            if (f <= 0 || s == 0) CHECK(sp.n_front == 0 && sp.front_items == 0);
            if (f > 0 && s >= 100) CHECK(sp.n_tail == 0 && sp.front_items == items);
            if (s < 0) {  // the built-in share is one of the two measured ones, and the whole list only on a long list
              const FinalSplit whole = final_split_plan(items, tiles_x, tiles_y, n_cu, per_cu, f, 100);
              const FinalSplit part = final_split_plan(items, tiles_x, tiles_y, n_cu, per_cu, f, 75);
              const bool is_whole = sp.front_items == whole.front_items && sp.n_front == whole.n_front && sp.n_tail == whole.n_tail;
              const bool is_part = sp.front_items == part.front_items && sp.n_front == part.n_front && sp.n_tail == part.n_tail;
              CHECK(is_whole || is_part);
              if (f == 1 && n_cu == 256) CHECK(is_whole == (items >= kFinalWholeListItems * 256u) || whole.front_items == part.front_items);
            }
            check_grid(sp);
            if (f < static_cast<int>(per_cu) && s >= 0) {  // front given per CU, share named: the earlier statement of the launch
              const Parent p = parent_split(items, n_cu, per_cu, f, s);
              CHECK(p.n_front == sp.n_front && p.n_tail == sp.n_tail && p.front_items == sp.front_items && p.items == sp.items);
              for (uint32_t b = 0; b < final_grid(sp); b++) {
                const FinalRole r = final_role(sp, b);
                const uint32_t t = b - p.n_front;  // (that kernel: unsigned, a front workgroup wraps past the tiles)
                if (t < n_tiles) {
                  CHECK(r.role == kFinalRoleTile && r.index == t);
                } else if (b < p.n_front) {
                  CHECK(r.role == kFinalRoleFront && r.index == b);
                } else {
                  CHECK(r.role == kFinalRoleTail && r.index == t - n_tiles);
                }
              }
            }
          }
    }
  {  // the two frames the built-in share was measured on (N = 5, 256 CUs, 1 workgroup per CU in front)
    const FinalSplit k4 = final_split_plan(60 * 54 * 5, 60, 540, 256, 8, 1, -1), hd = final_split_plan(30 * 27 * 5, 30, 270, 256, 8, 1, -1);
    CHECK(k4.n_front == 256 && k4.n_tail == 0 && k4.front_items == 16200);
    CHECK(hd.n_front == 256 && hd.front_items == 4050 * 75 / 100 && hd.n_tail == 8 * 127);
  }
  std::printf("final_split_host_check: %llu grids, %llu workgroups, every tile and item owned once\n", g_grids, g_blocks);
  return 0;
}
