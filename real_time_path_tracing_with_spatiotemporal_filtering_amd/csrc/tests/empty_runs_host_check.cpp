// empty_runs_host_check.cpp — a plain C++ program (no HIP, no device) over the run workgroups of final_split.hpp: the tile
// columns at the end of the dispatch order that no triangle's screen bounds reach, served in runs of tiles.  For frame widths that
// are no multiple of 64, tile grids from one column on, several row bands, run lengths from 1 to beyond the grid's height and
// seeded random bounds — "never" entries, bounds outside the frame, bounds that touch a column by one pixel — it checks that
//   * the columns final_full_columns leaves to the runs are the suffix of the dispatch order that a brute-force test of every tile
//     against every bound finds empty, and no shorter one;
//   * every block index of the launch has exactly one role, the groups in the order of the layout;
//   * every tile is owned exactly once, as a tile workgroup or inside one run; runs hold only tiles of suffix columns, lie within
//     one column, and none is longer than R;
//   * run length 0, and a frame whose last column is reached, give the launch of the seven-argument plan, member for member.
// `make -C csrc empty-runs-host-check` builds it with -fsanitize=address,undefined and runs it.
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

struct Bounds {  // kernels.hpp: TriBounds
  int16_t x0, y0, x1, y1;
};

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return static_cast<uint32_t>((z ^ (z >> 31)) >> 16);
}
static int rnd_in(int lo, int hi) { return lo + static_cast<int>(rnd() % static_cast<uint32_t>(hi - lo + 1)); }

// does some pixel of tile (bx, by) of the band [y0, y1) lie inside some bound?  The tile kernel's own pixels: columns below W,
// rows below y1.
static bool tile_reached(const std::vector<Bounds>& bs, int W, int y0, int y1, uint32_t bx, uint32_t by) {
  for (int y = y0 + 4 * static_cast<int>(by); y < y0 + 4 * static_cast<int>(by) + 4 && y < y1; y++)
    for (int x = 64 * static_cast<int>(bx); x < 64 * static_cast<int>(bx) + 64 && x < W; x++)
      for (const Bounds& b : bs)
        if (b.x0 <= b.x1 && x >= b.x0 && x <= b.x1 && y >= b.y0 && y <= b.y1) return true;
  return false;
}

static unsigned long long g_grids = 0, g_blocks = 0, g_with_runs = 0;

static void check_launch(const std::vector<Bounds>& bs, int W, int y0, int y1, uint32_t run_len, int front, int share) {
  const uint32_t tiles_x = (W + 63) / 64, tiles_y = (y1 - y0 + 3) / 4, items = tiles_x * ((tiles_y + 3) / 4) * 5;
  // brute force: one past the last column of the dispatch order with a reached tile
  uint32_t want = 0;
  for (uint32_t col = 0; col < tiles_x; col++) {
    bool reached = false;
    for (uint32_t by = 0; by < tiles_y && !reached; by++) reached = tile_reached(bs, W, y0, y1, tile_order_column(tiles_x, col), by);
    if (reached) want = col + 1;
  }
  const uint32_t full = final_full_columns(bs.data(), static_cast<uint32_t>(bs.size()), W, y0, y1, tiles_x);
  CHECK(full == want);
  {  // the order visits every column once
    std::vector<uint8_t> seen(tiles_x, 0);
    for (uint32_t col = 0; col < tiles_x; col++) {
      const uint32_t bx = tile_order_column(tiles_x, col);
      CHECK(bx < tiles_x && !seen[bx]);
      seen[bx] = 1;
    }
  }
  const FinalSplit base = final_split_plan(items, tiles_x, tiles_y, 256, 8, front, share);
  const FinalSplit sp = final_split_plan(items, tiles_x, tiles_y, 256, 8, front, share, full, run_len);
  CHECK(sp.n_front == base.n_front && sp.n_tail == base.n_tail && sp.front_items == base.front_items && sp.items == base.items && sp.tiles_x == tiles_x);
  if (run_len == 0 || full == tiles_x) {  // the launch without runs
    CHECK(sp.n_runs == 0 && sp.n_tiles == base.n_tiles && final_grid(sp) == final_grid(base));
    for (uint32_t b = 0; b < final_grid(sp); b++) {
      const FinalRole r = final_role(sp, b), q = final_role(base, b);
      CHECK(r.role == q.role && r.index == q.index && r.role != kFinalRoleRun);
    }
  } else {
    CHECK(sp.n_runs > 0 && sp.n_tiles == full * tiles_y);
    g_with_runs++;
  }
  const uint32_t grid = final_grid(sp);
  CHECK(grid == sp.n_front + sp.n_tiles + sp.n_runs + sp.n_tail);
  std::vector<uint8_t> owner(tiles_x * tiles_y, 0);  // by tile (by * tiles_x + bx)
  uint32_t last_role_rank = 0, n_front = 0, n_tail = 0, n_tile = 0, n_run = 0;
  for (uint32_t b = 0; b < grid; b++) {
    const FinalRole r = final_role(sp, b);
    uint32_t rank = 0;
    switch (r.role) {
      case kFinalRoleFront:
        rank = 0;
        CHECK(r.index == n_front++ && b < sp.n_front);
        break;
      case kFinalRoleTile: {
        rank = 1;
        CHECK(r.index == n_tile++ && r.index < sp.n_tiles);
        const uint32_t col = r.index / tiles_y, by = r.index % tiles_y;  // pathtrace_tile's own map
        CHECK(col < (sp.n_runs ? full : tiles_x));
        const uint32_t t = by * tiles_x + tile_order_column(tiles_x, col);
        CHECK(!owner[t]);
        owner[t] = 1;
        break;
      }
      case kFinalRoleRun: {
        rank = 2;
        CHECK(r.index == n_run++ && r.index < sp.n_runs);
        const FinalRun run = final_run(sp, r.index);
        CHECK(run.rows >= 1 && run.rows <= run_len && run.row0 + run.rows <= tiles_y && run.column < tiles_x);
        bool suffix = false;  // the run's column is one of the order's columns from `full` on
        for (uint32_t col = full; col < tiles_x; col++) suffix = suffix || tile_order_column(tiles_x, col) == run.column;
        CHECK(suffix);
        for (uint32_t by = run.row0; by < run.row0 + run.rows; by++) {
          CHECK(!tile_reached(bs, W, y0, y1, run.column, by));
          CHECK(!owner[by * tiles_x + run.column]);
          owner[by * tiles_x + run.column] = 2;
        }
        break;
      }
      case kFinalRoleTail:
        rank = 3;
        CHECK(r.index == n_tail++ && r.index < sp.n_tail);
        break;
      default:
        CHECK(!"a role outside the four");
    }
    CHECK(rank >= last_role_rank);  // front, tiles, runs, tail: the layout's order
    last_role_rank = rank;
  }
  CHECK(n_front == sp.n_front && n_tile == sp.n_tiles && n_run == sp.n_runs && n_tail == sp.n_tail);
  for (uint8_t v : owner) CHECK(v != 0);
  g_grids++;
  g_blocks += grid;
}

int main() {
  const int widths[] = {1, 63, 64, 65, 130, 200, 257, 449, 1000};
  const int bands[][2] = {{0, 4}, {0, 1}, {0, 37}, {0, 83}, {12, 40}, {5, 6}, {27, 83}};
  for (int W : widths)
    for (const auto& band : bands) {
      const int y0 = band[0], y1 = band[1];
      const uint32_t tiles_x = (W + 63) / 64, tiles_y = (y1 - y0 + 3) / 4;
      const uint32_t lens[] = {0, 1, 2, 3, 5, 16, tiles_y, tiles_y + 1, tiles_y + 7, 1000};
      for (int trial = 0; trial < 24; trial++) {
        std::vector<Bounds> bs;
        const int n = trial == 0 ? 0 : rnd_in(1, 12);
        for (int i = 0; i < n; i++) {
          Bounds b;
          switch (rnd() % 6u) {
            case 0:  // "never"
              b = Bounds{static_cast<int16_t>(rnd_in(0, W)), static_cast<int16_t>(rnd_in(-5, y1)), static_cast<int16_t>(rnd_in(-40, -1)), static_cast<int16_t>(rnd_in(y0, y1 + 5))};
              b.x1 = static_cast<int16_t>(b.x0 - 1 - rnd_in(0, 70));
              break;
            case 1: {  // outside the frame: left of it, right of it, above or below the band
              const int side = rnd_in(0, 3);
              if (side == 0) b = Bounds{-300, static_cast<int16_t>(y0), -1, static_cast<int16_t>(y1)};
              else if (side == 1) b = Bounds{static_cast<int16_t>(W), static_cast<int16_t>(y0), static_cast<int16_t>(W + 200), static_cast<int16_t>(y1)};
              else if (side == 2) b = Bounds{0, static_cast<int16_t>(y0 - 50), static_cast<int16_t>(W), static_cast<int16_t>(y0 - 1)};
              else b = Bounds{0, static_cast<int16_t>(y1), static_cast<int16_t>(W), static_cast<int16_t>(y1 + 50)};
              break;
            }
            case 2: {  // touches a column by one pixel: ends on its first pixel column, or starts on its last
              const int bx = rnd_in(0, static_cast<int>(tiles_x) - 1), yy = rnd_in(y0, y1 - 1);
              if (rnd() & 1u) b = Bounds{static_cast<int16_t>(64 * bx - rnd_in(0, 30)), static_cast<int16_t>(yy), static_cast<int16_t>(64 * bx), static_cast<int16_t>(yy)};
              else {
                const int last = 64 * bx + 63 < W ? 64 * bx + 63 : W - 1;
                b = Bounds{static_cast<int16_t>(last), static_cast<int16_t>(yy), static_cast<int16_t>(last + rnd_in(0, 30)), static_cast<int16_t>(yy)};
              }
              break;
            }
            case 3: {  // misses a column by one pixel, misses the band by one row
              const int bx = rnd_in(0, static_cast<int>(tiles_x) - 1);
              b = Bounds{static_cast<int16_t>(64 * bx - 20), static_cast<int16_t>(y1), static_cast<int16_t>(64 * bx - 1), static_cast<int16_t>(y1 + 3)};
              break;
            }
            default: {  // a small box somewhere about the frame
              const int x = rnd_in(-40, W + 40), y = rnd_in(y0 - 10, y1 + 10);
              b = Bounds{static_cast<int16_t>(x), static_cast<int16_t>(y), static_cast<int16_t>(x + rnd_in(0, 90)), static_cast<int16_t>(y + rnd_in(0, 12))};
            }
          }
          bs.push_back(b);
        }
        for (uint32_t R : lens) check_launch(bs, W, y0, y1, R, trial & 1 ? 1 : 0, trial % 3 == 0 ? 50 : -1);
      }
    }
  {  // the 4K frame with the middle 34 columns reached: 26 columns in runs of 8
    const Bounds b{13 * 64, 0, 46 * 64 + 63, 2159};
    const uint32_t full = final_full_columns(&b, 1, 3840, 0, 2160, 60);
    const FinalSplit sp = final_split_plan(16200, 60, 540, 256, 8, 1, -1, full, 8);
    CHECK(full == 34 && sp.n_tiles == 34 * 540 && sp.runs_per_col == 68 && sp.n_runs == 26 * 68 && final_grid(sp) == 256 + 18360 + 1768);
  }
  CHECK(g_with_runs > 1000);
  std::printf("empty_runs_host_check: %llu launches (%llu with runs), %llu workgroups, every tile owned once\n", g_grids, g_with_runs, g_blocks);
  return 0;
}
