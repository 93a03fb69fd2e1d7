// quotient_positive_host_check.cpp — a plain C++ program (no device) over exact::quotient_positive of rtpt_math.hpp: the same
// text the kernels compile, against `num / den > 0.0f` of the host's IEEE division.  The contract is zero mismatches over
//   * every exponent field x both signs x a few significands, for both operands (all pairs),
//   * zeros, subnormals, the smallest normals, infinities and NaNs (they are among the patterns above, and listed again),
//   * pairs whose quotient lies in [2^-151, 2^-148], around the tie at 2^-150 that rounds to zero,
//   * 2^28 pairs of random bits.
// `make -C csrc quotient-positive-host-check` builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../rtpt_math.hpp"

using rt::f2u;
using rt::u2f;

static uint64_t g_checked = 0, g_bad = 0, g_true = 0, g_long = 0;

static inline void check(uint32_t un, uint32_t ud) {
  const float num = u2f(un), den = u2f(ud);
  volatile float q = num / den;  // the division itself, whatever the optimiser thinks of its sign
  const bool want = q > 0.0f;
  const bool got = rt::exact::quotient_positive(num, den);
  g_checked++;
  g_true += want;
  g_long += !((den >= 0x1p-126f) & (den < 0x1p63f) & !((num > 0.0f) & (num < 0x1p-86f)));
  if (got != want) {
    if (g_bad < 8) std::fprintf(stderr, "mismatch: num %08x den %08x: quotient_positive %d, num / den > 0 %d\n", un, ud, got, want);
    g_bad++;
  }
}

int main() {
  // 1. structured: 256 exponent fields x 2 signs x 7 significands = 3584 patterns per operand, all 12.8 M pairs
  std::vector<uint32_t> pat;
  const uint32_t sig[] = {0x000000u, 0x000001u, 0x000002u, 0x400000u, 0x555555u, 0x7ffffeu, 0x7fffffu};
  for (uint32_t e = 0; e < 256; e++)
    for (uint32_t s = 0; s < 2; s++)
      for (uint32_t m : sig) pat.push_back((s << 31) | (e << 23) | m);
  // 2. the special values by name (most are in the list already)
  const uint32_t special[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u,
                              0x00800001u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7f800001u, 0x7fc00000u, 0xffc00000u,
                              0xffffffffu, 0x3f800000u, 0xbf800000u, 0x5f000000u /* 2^63 */, 0x5effffffu, 0x14800000u /* 2^-86 */, 0x147fffffu,
                              0x14800001u};
  for (uint32_t v : special) pat.push_back(v);
  for (uint32_t a : pat)
    for (uint32_t b : pat) check(a, b);
  const uint64_t n_structured = g_checked;

  // 3. quotients in [2^-151, 2^-148]: den = m_d 2^e_d, num = den x 2^k x (1 + j ulp) for k = -151 .. -148 built by exponent
  //    arithmetic (so num and den are exact patterns, whatever the quotient rounds to), and neighbours of the tie
  uint64_t n_edge = 0;
  const uint32_t dsig[] = {0x000000u, 0x000001u, 0x2aaaaau, 0x400000u, 0x7fffffu};
  for (int ed = 1; ed <= 254; ed++)          // den's exponent field
    for (uint32_t md : dsig)
      for (int sd = 0; sd < 2; sd++)
        for (int k = -152; k <= -147; k++) {
          const uint32_t ud = (static_cast<uint32_t>(sd) << 31) | (static_cast<uint32_t>(ed) << 23) | md;
          const int en = ed + k;             // num = den x 2^k where that is a normal or subnormal number
          uint32_t un;
          if (en >= 1)
            un = (static_cast<uint32_t>(en) << 23) | md;
          else if (en >= -22)
            un = (0x800000u | md) >> (1 - en);   // subnormal num (truncated: still a pattern next to the tie)
          else
            continue;
          for (int j = -2; j <= 2; j++)
            for (int sn = 0; sn < 2; sn++) {
              const uint32_t v = un + static_cast<uint32_t>(j);
              if (static_cast<int32_t>(v) < 0 || v > 0x7f800000u) continue;
              check((static_cast<uint32_t>(sn) << 31) | v, ud);
              n_edge++;
            }
        }

  // 4. 2^28 pairs of random bits (xorshift64*)
  uint64_t st = 0x9e3779b97f4a7c15ull;
  for (uint64_t i = 0; i < (1ull << 28); i++) {
    st ^= st >> 12;
    st ^= st << 25;
    st ^= st >> 27;
    const uint64_t r = st * 0x2545f4914f6cdd1dull;
    check(static_cast<uint32_t>(r), static_cast<uint32_t>(r >> 32));
  }

  std::printf("quotient_positive_host_check: %llu pairs (%llu structured, %llu around the tie, 2^28 random), %llu positive, %llu through the division, %llu mismatches\n",
              static_cast<unsigned long long>(g_checked), static_cast<unsigned long long>(n_structured), static_cast<unsigned long long>(n_edge),
              static_cast<unsigned long long>(g_true), static_cast<unsigned long long>(g_long), static_cast<unsigned long long>(g_bad));
  if (g_bad || g_true == 0 || g_long == 0 || n_edge < 10000) return 1;
  std::printf("quotient_positive_host_check: ok\n");
  return 0;
}
