// host_twin.cpp -- see host_twin.hpp
#include "host_twin.hpp"

namespace edigpu {

std::string twin_sector(int mode, int ns, int q1, int q2, int& t1, int& t2, bool& self) {
  t1 = t2 = 0;
  self = false;
  // (a superc / nonsu2 state has 2 Ns bits of an int32; a normal-mode word Ns)
  if (ns < 1 || ns > (mode == kTwinNormal ? 31 : 15)) return "Ns out of range";
  switch (mode) {
    case kTwinNormal:
      if (q1 < 0 || q1 > ns || q2 < 0 || q2 > ns) return "sector (Nup, Ndw) out of range";
      t1 = q2;
      t2 = q1;
      self = q1 == q2;
      return "";
    case kTwinSuperc:
      if (q1 < -ns || q1 > ns) return "sector Sz out of range";
      t1 = -q1;
      self = q1 == 0;
      return "";
    case kTwinNonsu2:
      if (q1 < 0 || q1 > 2 * ns) return "sector Ntot out of range";
      t1 = 2 * ns - q1;
      self = q1 == ns;
      return "";
  }
  return "mode must be 0 (normal), 1 (superc) or 2 (nonsu2)";
}

void twin_sector_orbs(int norb, const int* nups, const int* ndws, int* tnups, int* tndws, bool& self) {
  self = true;
  for (int a = 0; a < norb; a++) {
    self = self && nups[a] == ndws[a];
    const int u = nups[a], d = ndws[a];  // (the outputs may alias the inputs)
    tnups[a] = d;
    tndws[a] = u;
  }
}

std::string twin_order(int mode, const int32_t* map, int64_t n, int ns, std::vector<int32_t>& order) {
  order.clear();
  if (mode != kTwinSuperc && mode != kTwinNonsu2) return "mode must be 1 (superc) or 2 (nonsu2)";
  if (ns < 1 || ns > 15) return "Ns out of range";
  if (n < 0 || n > INT32_MAX || (n > 0 && !map)) return "bad sector map";
  const int64_t nstates = (int64_t)1 << (2 * ns);
  for (int64_t i = 0; i < n; i++)
    if (map[i] < 0 || map[i] >= nstates || (i > 0 && map[i] <= map[i - 1])) return "the sector map is not ascending states of 2 Ns levels";
  order.resize((size_t)n);
  if (mode == kTwinNonsu2) {
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = (int32_t)(n - 1 - i);
    return "";
  }
  const int32_t low = (int32_t)((1u << ns) - 1u);
  std::vector<int64_t> start(((size_t)1 << ns) + 1, 0);
  for (int64_t i = 0; i < n; i++) start[(size_t)(map[i] & low) + 1]++;
  for (size_t u = 1; u < start.size(); u++) start[u] += start[u - 1];
  for (int64_t i = 0; i < n; i++) order[(size_t)start[(size_t)(map[i] & low)]++] = (int32_t)i;
  return "";
}

}  // namespace edigpu
