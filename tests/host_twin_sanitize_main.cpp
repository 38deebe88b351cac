// Stand-alone driver of csrc/host_twin.cpp for tests/test_twin_host.py: the order tables of every superc (Sz) and nonsu2
// (Ntot) sector of Ns = 2 .. 7 and one larger superc sector, the twin of every sector of the three modes and of the
// per-orbital form, and the refusals, built with -fsanitize=address,undefined and run as a program.  Every table is
// checked as the kernel uses it (an index into the source vector) and against a stable sort of the flipped states.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "host_twin.hpp"

using namespace edigpu;

static int failures = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);    \
      failures++;                                            \
    }                                                        \
  } while (0)

// the ascending states iup + idw 2^ns of a superc (Nup - Ndw = q) or nonsu2 (Nup + Ndw = q) sector
static std::vector<int32_t> sector_states(int mode, int ns, int q) {
  std::vector<int32_t> m;
  const uint32_t low = (1u << ns) - 1u;
  for (uint32_t x = 0; x < (1u << (2 * ns)); x++) {
    const int nu = __builtin_popcount(x & low), nd = __builtin_popcount(x >> ns);
    if ((mode == kTwinSuperc ? nu - nd : nu + nd) == q) m.push_back((int32_t)x);
  }
  return m;
}

static uint32_t flip(int mode, int ns, uint32_t x) {
  const uint32_t low = (1u << ns) - 1u, all = (1u << (2 * ns)) - 1u;
  return mode == kTwinSuperc ? ((x & low) << ns) | (x >> ns) : (~x & all);
}

static void check_order(int mode, int ns, int q) {
  const std::vector<int32_t> map = sector_states(mode, ns, q);
  int t1 = 0, t2 = 0;
  bool self = false;
  CHECK(twin_sector(mode, ns, q, 0, t1, t2, self).empty());
  const std::vector<int32_t> twin = sector_states(mode, ns, t1);
  CHECK(twin.size() == map.size() && t2 == 0 && self == (t1 == q));
  std::vector<int32_t> order;
  CHECK(twin_order(mode, map.data(), (int64_t)map.size(), ns, order).empty());
  CHECK(order.size() == map.size());
  if (order.size() != map.size() || twin.size() != map.size()) return;
  std::vector<int32_t> want(map.size());
  std::iota(want.begin(), want.end(), 0);
  std::stable_sort(want.begin(), want.end(), [&](int32_t a, int32_t b) {
    return flip(mode, ns, (uint32_t)map[(size_t)a]) < flip(mode, ns, (uint32_t)map[(size_t)b]);
  });
  std::vector<char> seen(map.size(), 0);
  for (size_t i = 0; i < order.size(); i++) {
    CHECK(order[i] >= 0 && (size_t)order[i] < map.size());  // what the kernel indexes the source vector with
    if (order[i] < 0 || (size_t)order[i] >= map.size()) return;
    CHECK(!seen[(size_t)order[i]]);
    seen[(size_t)order[i]] = 1;
    CHECK(order[i] == want[i]);
    CHECK(flip(mode, ns, (uint32_t)map[(size_t)order[i]]) == (uint32_t)twin[i]);  // state i of the twin is the flipped source state
  }
}

int main() {
  for (int ns = 2; ns <= 7; ns++) {
    for (int sz = -ns; sz <= ns; sz++) check_order(kTwinSuperc, ns, sz);
    for (int n = 0; n <= 2 * ns; n++) check_order(kTwinNonsu2, ns, n);
  }
  check_order(kTwinSuperc, 10, 1);
  // the twin of every sector
  for (int ns = 1; ns <= 6; ns++) {
    int t1, t2;
    bool self;
    for (int nu = 0; nu <= ns; nu++)
      for (int nd = 0; nd <= ns; nd++) {
        CHECK(twin_sector(kTwinNormal, ns, nu, nd, t1, t2, self).empty() && t1 == nd && t2 == nu && self == (nu == nd));
      }
    for (int sz = -ns; sz <= ns; sz++) CHECK(twin_sector(kTwinSuperc, ns, sz, 7, t1, t2, self).empty() && t1 == -sz && t2 == 0 && self == (sz == 0));
    for (int n = 0; n <= 2 * ns; n++) CHECK(twin_sector(kTwinNonsu2, ns, n, 7, t1, t2, self).empty() && t1 == 2 * ns - n && self == (n == ns));
    CHECK(!twin_sector(kTwinNormal, ns, ns + 1, 0, t1, t2, self).empty());
    CHECK(!twin_sector(kTwinNormal, ns, 0, -1, t1, t2, self).empty());
    CHECK(!twin_sector(kTwinSuperc, ns, ns + 1, 0, t1, t2, self).empty());
    CHECK(!twin_sector(kTwinNonsu2, ns, 2 * ns + 1, 0, t1, t2, self).empty());
    CHECK(!twin_sector(3, ns, 0, 0, t1, t2, self).empty());
  }
  {
    int t1, t2;
    bool self;
    CHECK(!twin_sector(kTwinNormal, 0, 0, 0, t1, t2, self).empty() && !twin_sector(kTwinNormal, 32, 0, 0, t1, t2, self).empty());
    CHECK(twin_sector(kTwinNormal, 16, 8, 7, t1, t2, self).empty() && t1 == 7 && t2 == 8);
    CHECK(!twin_sector(kTwinSuperc, 16, 0, 0, t1, t2, self).empty() && !twin_sector(kTwinNonsu2, 16, 0, 0, t1, t2, self).empty());
    const int nups[3] = {2, 1, 0}, ndws[3] = {1, 2, 0};
    int tu[3], td[3];
    twin_sector_orbs(3, nups, ndws, tu, td, self);
    CHECK(!self && tu[0] == 1 && tu[1] == 2 && tu[2] == 0 && td[0] == 2 && td[1] == 1 && td[2] == 0);
    int u[2] = {1, 3}, d[2] = {1, 3};
    twin_sector_orbs(2, u, d, u, d, self);  // in place
    CHECK(self && u[0] == 1 && u[1] == 3 && d[0] == 1 && d[1] == 3);
    int a[1] = {0}, b[1] = {4};
    twin_sector_orbs(1, a, b, a, b, self);
    CHECK(!self && a[0] == 4 && b[0] == 0);
  }
  // refusals of the table
  {
    std::vector<int32_t> order;
    const std::vector<int32_t> map = sector_states(kTwinSuperc, 3, 0);
    CHECK(!twin_order(kTwinNormal, map.data(), (int64_t)map.size(), 3, order).empty() && order.empty());
    CHECK(!twin_order(kTwinSuperc, map.data(), (int64_t)map.size(), 0, order).empty());
    CHECK(!twin_order(kTwinSuperc, map.data(), (int64_t)map.size(), 16, order).empty());
    CHECK(!twin_order(kTwinSuperc, nullptr, 3, 3, order).empty());
    CHECK(!twin_order(kTwinSuperc, map.data(), -1, 3, order).empty());
    CHECK(!twin_order(kTwinSuperc, map.data(), (int64_t)map.size(), 2, order).empty());  // states past 2^(2 Ns)
    std::vector<int32_t> bad = map;
    std::swap(bad[1], bad[2]);
    CHECK(!twin_order(kTwinSuperc, bad.data(), (int64_t)bad.size(), 3, order).empty());  // not ascending
    bad = map;
    bad[0] = -1;
    CHECK(!twin_order(kTwinSuperc, bad.data(), (int64_t)bad.size(), 3, order).empty());
    CHECK(twin_order(kTwinSuperc, map.data(), 0, 3, order).empty() && order.empty());  // an empty sector is no error
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
