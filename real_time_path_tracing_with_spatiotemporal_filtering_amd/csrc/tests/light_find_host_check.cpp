// light_find_host_check.cpp — a plain C++ program (no HIP, no device) over rtpt_light::find (light_list_host.hpp): the binary search
// that RTPT_FLAG_EXT_NEE_MIS uses to find a hit emitter's entry of the light list.  Every list is an allocation of exactly its
// length, so that a read outside [0, n) is the address sanitizer's to report; `make -C csrc light-find-host-check` builds it with
// -fsanitize=address,undefined and runs it.  Lists of 0, 1, 2, 3, 1,000 and 2^20 + 1,025 ids; queries at both ends, at every
// entry, in every gap, below and above the list; and lists that are not ascending, on which only the bounds are asked for.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../light_list_host.hpp"

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

using rtpt_light::find;

// the answer by its definition
static uint32_t linear(const uint32_t* ids, uint32_t n, uint32_t id1) {
  for (uint32_t i = 0; i < n; i++)
    if (ids[i] == id1) return i;
  return n;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// an ascending list of n ids from `first` on, gaps of 1 to max_gap between neighbours, in an allocation of exactly n words
static std::unique_ptr<uint32_t[]> ascending(uint32_t n, uint32_t first, uint32_t max_gap, uint32_t seed) {
  std::unique_ptr<uint32_t[]> ids(new uint32_t[n]);
  uint32_t v = first;
  for (uint32_t i = 0; i < n; i++) {
    ids[i] = v;
    v += 1u + lcg(seed) % max_gap;
  }
  return ids;
}

static void check_list(const uint32_t* ids, uint32_t n, bool every_gap) {
  // both ends, below and above
  const uint32_t outside[] = {0u, 1u, 0xFFFFFFFFu, 0x80000000u};
  for (uint32_t q : outside) CHECK(find(ids, n, q) == linear(ids, n, q));
  if (!n) return;
  CHECK(find(ids, n, ids[0]) == 0u && find(ids, n, ids[n - 1]) == n - 1u);
  if (ids[0] > 0u) CHECK(find(ids, n, ids[0] - 1u) == n);
  if (ids[n - 1] < 0xFFFFFFFFu) CHECK(find(ids, n, ids[n - 1] + 1u) == n);
  const uint32_t step = every_gap ? 1u : 97u;
  for (uint32_t i = 0; i < n; i += step) {
    CHECK(find(ids, n, ids[i]) == i);                          // every entry
    if (i + 1u < n && ids[i] + 1u < ids[i + 1u]) {             // every gap: its first, its last and a middle id
      CHECK(find(ids, n, ids[i] + 1u) == n);
      CHECK(find(ids, n, ids[i + 1u] - 1u) == n);
      CHECK(find(ids, n, ids[i] + (ids[i + 1u] - ids[i]) / 2u) == n);
    }
  }
}

int main() {
  // the empty list: nothing is read (a null pointer)
  CHECK(find(nullptr, 0u, 0u) == 0u && find(nullptr, 0u, 7u) == 0u);
  const uint32_t sizes[] = {1u, 2u, 3u, 1000u, (1u << 20) + 1025u};
  for (uint32_t n : sizes) {
    for (uint32_t max_gap : {1u, 2u, 5u}) {  // 1: consecutive ids, no gap at all
      const std::unique_ptr<uint32_t[]> ids = ascending(n, 1u + n % 3u, max_gap, 17u + n);
      check_list(ids.get(), n, n <= 1000u);
      if (n > 1000u) check_list(ids.get(), 4099u, true);  // a prefix of it, every gap
    }
  }
  // the largest ids: the list ends at 2^32 - 1
  {
    const uint32_t n = 5u;
    std::unique_ptr<uint32_t[]> ids(new uint32_t[n]{0xFFFFFFF0u, 0xFFFFFFF1u, 0xFFFFFFF8u, 0xFFFFFFFEu, 0xFFFFFFFFu});
    check_list(ids.get(), n, true);
  }
  // whatever the operands hold: lists that are not ascending (random, descending, constant).  The answer is then some index
  // whose entry is the id, or n; what is asked for is that no read leaves the allocation
  {
    uint32_t seed = 99u;
    for (uint32_t n : {1u, 2u, 3u, 64u, 1000u}) {
      std::unique_ptr<uint32_t[]> ids(new uint32_t[n]);
      for (int kind = 0; kind < 3; kind++) {
        for (uint32_t i = 0; i < n; i++) ids[i] = kind == 0 ? lcg(seed) : (kind == 1 ? n - i : 7u);
        for (uint32_t k = 0; k < 4096u; k++) {
          const uint32_t q = k < n ? ids[k] : lcg(seed) % (2u * n + 1u);
          const uint32_t r = find(ids.get(), n, q);
          CHECK(r <= n && (r == n || ids[r] == q));
        }
      }
    }
  }
  std::puts("light_find_host_check: ok");
  return 0;
}
