// light_table.hip — the cumulative table of the weighted light pick (RTPT_FLAG_EXT_NEE_POWER; light_sample.hpp states the
// arithmetic: weight, maximum, quantised weight, C_i).  Built on the device because the posed triangles exist only there on the
// BVH path and move without an upload; everything runs on the caller's stream, without synchronisation or readback:
//   1. one lane per entry: w_i (from the scene, or given), "counts as 0", its bits into scratch; the maximum of the bits of a
//      wave by __shfl_down, of the table by one atomicMax a wave into one word
//   2. one lane per entry: q_i from w_i and the maximum; the inclusive scan of a workgroup's kLightTableBlock entries (64-wide
//      __shfl_up within a wave, LDS across the 16 waves) into C, the workgroup's total into sums[b]
//   3. the same scan over the sums, level by level, until one workgroup holds a level (2^24 entries: 16,384 sums, then 16)
//   4. back down: every entry of workgroup b > 0 gains the scanned sum of workgroup b - 1
// Integer sums and an integer maximum: any order gives the same bits.  Plain vector loads, stores and atomics.
#include "light_sample.hpp"

namespace rt {
namespace {

constexpr uint32_t kBlock = kLightTableBlock;
constexpr uint32_t kWaves = kBlock / 64u;
static_assert(kBlock == 1024u && kWaves == 16u, "one wave scans the totals of the workgroup's waves");

// the scratch area: word 0 the maximum's bits (8 bytes, so that the sums behind it are aligned), the sums of every level, the
// weights' bits
struct Levels {
  size_t count[4];  // workgroups of level l: count[0] = ceil(n / kBlock), count[l + 1] = ceil(count[l] / kBlock)
  int n;            // levels that have sums: every level but the last has more than one workgroup
  size_t sums;      // entries of all levels' sums together
};
inline Levels levels_of(size_t n) {
  Levels lv{};
  size_t m = n;
  do {
    m = (m + kBlock - 1) / kBlock;
    lv.count[lv.n++] = m;
    lv.sums += m;
  } while (m > 1 && lv.n < 4);
  return lv;
}

// step 1.  FROM_SCENE: entry i is ids[i], a posed id + 1 whose shade record and material record give w_i; else w_i = w[i].
// Lanes beyond n hold 0 and take part in the wave's maximum.
template <bool FROM_SCENE>
__global__ __launch_bounds__(256) void k_light_weights(LightTableArgs a, const float* __restrict__ w, uint32_t n, uint32_t* __restrict__ bits,
                                                       uint32_t* __restrict__ w_max) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t b = 0u;
  if (i < n) {
    float wi;
    if constexpr (FROM_SCENE) {
      const uint32_t id1 = a.ids[i];
      const float4* ls = a.shade + 3 * static_cast<size_t>(id1 - 1);
      const float4 l0 = ls[0], l1 = ls[1], l2 = ls[2];
      const float4 ke = a.materials[2 * static_cast<size_t>((id1 - 1) % a.n_base_tris) + 1];
      wi = light::weight(xyz(l0), xyz(l1), xyz(l2), xyz(ke));
    } else {
      wi = w[i];
    }
    b = light::weight_bits(wi);
    bits[i] = b;
  }
  uint32_t m = b;
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = __shfl_down(m, d, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63u) == 0u && m != 0u) atomicMax(w_max, m);
}

// the inclusive scan of a workgroup's values, one per lane (0 beyond the end); `waves` is LDS for kWaves totals
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* waves) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_up(static_cast<unsigned long long>(v), d, 64);
    if (lane >= static_cast<uint32_t>(d)) v += o;
  }
  if (lane == 63u) waves[wave] = v;
  __syncthreads();
  if (wave == 0u) {
    uint64_t t = lane < kWaves ? waves[lane] : 0ull;
    for (int d = 1; d < static_cast<int>(kWaves); d <<= 1) {
      const uint64_t o = __shfl_up(static_cast<unsigned long long>(t), d, 64);
      if (lane >= static_cast<uint32_t>(d)) t += o;
    }
    if (lane < kWaves) waves[lane] = t;  // inclusive over the waves
  }
  __syncthreads();
  return wave ? v + waves[wave - 1u] : v;
}

// steps 2 and 3.  QUANTISE: the values are q_i of bits[i] and *w_max, written to out as their scan; else the values are
// out[i] themselves, scanned in place.  sums: the workgroups' totals, NULL where the level has one workgroup.
template <bool QUANTISE>
__global__ __launch_bounds__(kBlock) void k_light_scan(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ w_max, uint64_t* out, size_t n,
                                                       uint64_t* __restrict__ sums) {
  __shared__ uint64_t waves[kWaves];
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  uint64_t v = 0ull;
  if (i < n) {
    if constexpr (QUANTISE)
      v = light::quantise(bits[i], *w_max);
    else
      v = out[i];
  }
  v = block_scan(v, waves);
  if (i < n) out[i] = v;
  if (sums && threadIdx.x == kBlock - 1u) sums[blockIdx.x] = v;  // (lanes beyond the end added 0: the last lane holds the total)
}

// step 4: the entries of workgroup b > 0 of a level gain what the workgroups in front of it sum to
__global__ __launch_bounds__(kBlock) void k_light_offsets(uint64_t* __restrict__ out, size_t n, const uint64_t* __restrict__ sums) {
  if (blockIdx.x == 0u) return;
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) out[i] += sums[blockIdx.x - 1u];
}

__global__ __launch_bounds__(256) void k_selftest_light_pick(const uint64_t* __restrict__ cdf, uint32_t n, const float* __restrict__ u_l, size_t k,
                                                             uint32_t* __restrict__ index_out, float* __restrict__ inv_p_out) {
  const size_t j = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
  if (j >= k) return;
  const light::Pick p = light::pick_power(u_l[j], cdf, n);
  index_out[j] = p.i;
  inv_p_out[j] = p.inv_p;
}

// the table of n entries (1 <= n <= 2^24) whose weights are a's or w's
void build(const LightTableArgs* a, const float* w, size_t n, uint64_t* cdf, void* scratch, hipStream_t s) {
  if (!n || n > light::kMaxLights) return;
  const Levels lv = levels_of(n);
  uint32_t* const w_max = static_cast<uint32_t*>(scratch);
  uint64_t* const sums = reinterpret_cast<uint64_t*>(static_cast<char*>(scratch) + 8);
  uint32_t* const bits = reinterpret_cast<uint32_t*>(sums + lv.sums);
  const uint32_t n32 = static_cast<uint32_t>(n);
  (void)hipMemsetAsync(w_max, 0, 8, s);
  const dim3 wgrid(static_cast<uint32_t>((n + 255) / 256));
  if (a)
    hipLaunchKernelGGL(k_light_weights<true>, wgrid, dim3(256), 0, s, *a, nullptr, n32, bits, w_max);
  else
    hipLaunchKernelGGL(k_light_weights<false>, wgrid, dim3(256), 0, s, LightTableArgs{}, w, n32, bits, w_max);
  // down: level l scans its values into place and leaves its workgroups' totals, the values of level l + 1
  uint64_t* level[5] = {cdf, nullptr, nullptr, nullptr, nullptr};
  size_t count[5] = {n, 0, 0, 0, 0};
  {
    uint64_t* p = sums;
    for (int l = 0; l < lv.n; l++) {
      level[l + 1] = p;
      count[l + 1] = lv.count[l];
      p += lv.count[l];
    }
  }
  for (int l = 0; l < lv.n; l++) {
    const dim3 grid(static_cast<uint32_t>(lv.count[l]));
    uint64_t* const totals = lv.count[l] > 1 ? level[l + 1] : nullptr;
    if (l == 0)
      hipLaunchKernelGGL(k_light_scan<true>, grid, dim3(kBlock), 0, s, bits, w_max, level[0], count[0], totals);
    else
      hipLaunchKernelGGL(k_light_scan<false>, grid, dim3(kBlock), 0, s, nullptr, nullptr, level[l], count[l], totals);
    if (lv.count[l] <= 1) break;
  }
  // up: level l's workgroups take their offsets from the scanned level l + 1
  for (int l = lv.n - 1; l >= 0; l--)
    if (lv.count[l] > 1)
      hipLaunchKernelGGL(k_light_offsets, dim3(static_cast<uint32_t>(lv.count[l])), dim3(kBlock), 0, s, level[l], count[l], level[l + 1]);
}

}  // namespace

size_t light_table_scratch_bytes(size_t n) { return 8 + 8 * levels_of(n).sums + 4 * n; }

void launch_light_table(const LightTableArgs& a, hipStream_t s) {
  if (!a.ids || !a.shade || !a.materials || !a.n_base_tris || !a.cdf || !a.scratch) return;
  build(&a, nullptr, a.n, a.cdf, a.scratch, s);
}

void launch_light_table_weights(const float* w, size_t n, uint64_t* cdf, void* scratch, hipStream_t s) {
  if (!w || !cdf || !scratch) return;
  build(nullptr, w, n, cdf, scratch, s);
}

void launch_selftest_light_pick(const uint64_t* cdf, uint32_t n, const float* u_l, size_t k, uint32_t* index_out, float* inv_p_out, hipStream_t s) {
  if (!n || !k) return;
  hipLaunchKernelGGL(k_selftest_light_pick, dim3(static_cast<uint32_t>((k + 255) / 256)), dim3(256), 0, s, cdf, n, u_l, k, index_out, inv_p_out);
}

}  // namespace rt
