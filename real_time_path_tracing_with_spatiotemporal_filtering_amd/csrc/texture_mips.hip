// texture_mips.hip — the generated mip chain of a texture with RTPT_TEX_MIPMAP (rtpt_scene_set_textures): one launch per
// level, one texel per lane, 16-byte loads and stores.  The arithmetic is the header's: ((a + b) + (c + d)) * 0.25f per
// channel, alpha included.
#include "kernels.hpp"

namespace rt {
namespace {

// Every index is bounded by the level's own dimensions: a lane beyond dw * dh leaves, and the source columns and rows are
// clamped to sw - 1 and sh - 1 (what keeps the last column or row of a 1-wide or 1-high level, and drops an odd one otherwise).
__global__ __launch_bounds__(256) void k_mip_downsample(float4* __restrict__ atlas, uint32_t src, uint32_t sw, uint32_t sh, uint32_t dst,
                                                        uint32_t dw, uint32_t dh) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // dw * dh <= 2^30
  if (i >= dw * dh) return;
  const uint32_t x = i % dw, y = i / dw;
  const uint32_t x0 = 2u * x < sw - 1u ? 2u * x : sw - 1u, x1 = 2u * x + 1u < sw - 1u ? 2u * x + 1u : sw - 1u;
  const uint32_t y0 = 2u * y < sh - 1u ? 2u * y : sh - 1u, y1 = 2u * y + 1u < sh - 1u ? 2u * y + 1u : sh - 1u;
  const float4* s = atlas + src;
  const size_t r0 = static_cast<size_t>(y0) * sw, r1 = static_cast<size_t>(y1) * sw;
  const float4 a = s[r0 + x0], b = s[r0 + x1], c = s[r1 + x0], d = s[r1 + x1];
  atlas[static_cast<size_t>(dst) + i] = make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f,
                                                    ((a.z + b.z) + (c.z + d.z)) * 0.25f, ((a.w + b.w) + (c.w + d.w)) * 0.25f);
}

}  // namespace

void launch_mip_downsample(float4* atlas, uint32_t src, uint32_t sw, uint32_t sh, uint32_t dst, hipStream_t s) {
  if (!sw || !sh) return;
  const uint32_t dw = sw >> 1 ? sw >> 1 : 1u, dh = sh >> 1 ? sh >> 1 : 1u;
  hipLaunchKernelGGL(k_mip_downsample, dim3((dw * dh + 255u) / 256u), dim3(256), 0, s, atlas, src, sw, sh, dst, dw, dh);
}

}  // namespace rt
