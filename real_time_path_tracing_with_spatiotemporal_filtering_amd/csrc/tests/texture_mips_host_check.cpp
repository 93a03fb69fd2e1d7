// texture_mips_host_check.cpp — a plain C++ program (no HIP, no device) over the mip-chain part of texture_host.hpp: the
// chain's geometry, what check_textures refuses for the two mip flags, the level table and the byte formula, with the 64-bit
// cases (a 65536 x 65536 chain, an atlas that ends at 2^32 - 1).  `make -C csrc texture-mips-host-check` builds it with
// -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../texture_host.hpp"

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

using namespace rtpt_tex;

static const char* check(const std::vector<rtpt_texture>& tex, size_t n_texels) {
  static const float uv[6] = {0, 0, 1, 0, 0, 1};
  static const uint32_t tri[1] = {1};
  return check_textures(uv, tri, 1, 1, tex.data(), static_cast<uint32_t>(tex.size()), n_texels);
}

int main() {
  // geometry: levels, dimensions, texel counts
  struct Case {
    uint32_t w, h, levels;
    uint64_t texels;
  };
  const Case cases[] = {{1, 1, 1, 1},   {1, 7, 3, 7 + 3 + 1}, {5, 3, 3, 15 + 2 + 1}, {8, 8, 4, 64 + 16 + 4 + 1}, {16, 4, 5, 64 + 16 + 4 + 2 + 1},
                        {33, 17, 6, 561 + 128 + 32 + 8 + 2 + 1}, {65536, 1, 17, 131071}, {65536, 65536, 17, 5726623061ull}};
  for (const Case& c : cases) {
    CHECK(chain_levels(c.w, c.h) == c.levels);
    CHECK(chain_texels(c.w, c.h) == c.texels);
    CHECK(level_dim(c.w, c.levels - 1) == 1 && level_dim(c.h, c.levels - 1) == 1);
    CHECK(chain_levels(c.w, c.h) <= kMaxTexLevels);
  }
  CHECK(level_dim(5, 1) == 2 && level_dim(5, 2) == 1 && level_dim(5, 3) == 1 && level_dim(5, 31) == 1 && level_dim(5, 32) == 1);

  // flags
  CHECK(check({{8, 8, 0, 0}}, 64) == nullptr);
  CHECK(check({{8, 8, 0, RTPT_TEX_MIPMAP}}, 64) == nullptr);                             // generated: level 0 only
  CHECK(check({{8, 8, 0, RTPT_TEX_MIPMAP | RTPT_TEX_NEAREST}}, 64) == nullptr);
  CHECK(check({{8, 8, 0, RTPT_TEX_MIPS_GIVEN}}, 85) != nullptr);                          // GIVEN without MIPMAP
  CHECK(check({{8, 8, 0, RTPT_TEX_MIPMAP | RTPT_TEX_MIPS_GIVEN}}, 85) == nullptr);
  CHECK(check({{8, 8, 0, RTPT_TEX_MIPMAP | RTPT_TEX_MIPS_GIVEN}}, 84) != nullptr);        // the chain ends beyond n_texels
  CHECK(check({{8, 8, 3, RTPT_TEX_MIPMAP | RTPT_TEX_MIPS_GIVEN}}, 87) != nullptr);
  CHECK(check({{8, 8, 3, RTPT_TEX_MIPMAP | RTPT_TEX_MIPS_GIVEN}}, 88) == nullptr);
  for (uint32_t bad : {0x2u, 0x4u, 0x8u, 0x40u, 0x80000000u}) {
    CHECK(check({{8, 8, 0, bad}}, 64) != nullptr);
    CHECK(check({{8, 8, 0, bad | RTPT_TEX_MIPMAP}}, 64) != nullptr);
  }
  // 64 bits: a given 65536 x 65536 chain cannot fit below 2^32 - 1 texels, whatever n_texels claims; its level 0 alone can
  CHECK(check({{65536, 65536, 0, RTPT_TEX_MIPMAP | RTPT_TEX_MIPS_GIVEN}}, static_cast<size_t>(6000000000ull)) != nullptr);
  CHECK(check({{65535, 65535, 0, 0}}, static_cast<size_t>(4294836225ull)) == nullptr);
  // ... and generating its chain would take the atlas beyond 2^32 - 1
  CHECK(check({{65535, 65535, 0, RTPT_TEX_MIPMAP}}, static_cast<size_t>(4294836225ull)) != nullptr);
  // the atlas may end exactly at 2^32 - 1: 65536 x 32768 (2^31) + its generated levels (715,827,882) + padding
  {
    const uint64_t gen = chain_texels(65536, 32768) - (1ull << 31);
    const uint64_t room = 0xFFFFFFFFull - (1ull << 31) - gen;
    CHECK(check({{65536, 32768, static_cast<uint32_t>(room), RTPT_TEX_MIPMAP}}, static_cast<size_t>((1ull << 31) + room)) == nullptr);
    CHECK(check({{65536, 32768, static_cast<uint32_t>(room + 1), RTPT_TEX_MIPMAP}}, static_cast<size_t>((1ull << 31) + room + 1)) != nullptr);
  }

  // the level table: a plain texture, a generated chain, a given chain, another generated chain
  const std::vector<rtpt_texture> tex = {{3, 5, 2, RTPT_TEX_NEAREST},
                                         {5, 3, 17, RTPT_TEX_MIPMAP},
                                         {8, 8, 40, RTPT_TEX_MIPMAP | RTPT_TEX_MIPS_GIVEN},
                                         {1, 7, 32, RTPT_TEX_MIPMAP | RTPT_TEX_NEAREST}};
  const size_t n_texels = 40 + 85 + 4;
  CHECK(check(tex, n_texels) == nullptr);
  CHECK(any_mipmap(tex.data(), 4) && !any_mipmap(tex.data(), 1));
  CHECK(generated_texels(tex.data(), 4) == (2 + 1) + (3 + 1));
  std::vector<uint32_t> table(4 * kLevelRow, 0xDEADBEEFu);
  build_level_table(tex.data(), 4, n_texels, table.data());
  const uint32_t want[4][kLevelRow] = {
      {2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0},
      {17, 129, 131, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0},
      {40, 104, 120, 124, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0},
      {32, 132, 135, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0},
  };
  CHECK(std::memcmp(table.data(), want, sizeof want) == 0);
  // every level of every row lies inside the device atlas
  const uint64_t atlas = n_texels + generated_texels(tex.data(), 4);
  for (uint32_t i = 0; i < 4; i++) {
    const uint32_t* row = table.data() + kLevelRow * i;
    CHECK(row[kLevelRowCount] >= 1 && row[kLevelRowCount] <= kMaxTexLevels);
    for (uint32_t l = 0; l < row[kLevelRowCount]; l++)
      CHECK(static_cast<uint64_t>(row[l]) + static_cast<uint64_t>(level_dim(tex[i].width, l)) * level_dim(tex[i].height, l) <= atlas);
  }
  CHECK(atlas == 136);

  // bytes: the plain formula without a mip flag, + 16 per generated texel + 80 per texture with one
  CHECK(device_bytes(7, tex.data(), 1, 100) == device_bytes(7, 1, 100));
  CHECK(device_bytes(7, tex.data(), 4, n_texels) == 32 * 7 + 16 * 4 + 16 * n_texels + 16 * 7 + 80 * 4);
  std::puts("texture_mips_host_check: ok");
  return 0;
}
