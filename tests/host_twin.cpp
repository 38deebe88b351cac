// extern "C" wrapper of csrc/host_twin.cpp for tests/test_twin_host.py (g++, no HIP).
#include <cstring>
#include <vector>

#include "host_twin.hpp"

using namespace edigpu;

static int finish(const std::string& why, char* err) {
  std::strncpy(err, why.c_str(), 255);
  err[255] = 0;
  return why.empty() ? 0 : 1;
}

extern "C" {

// out: t1, t2, self; err: 256 bytes.  Returns 0, or 1 with the reason in err.
int ht_twin_sector(int mode, int ns, int q1, int q2, int32_t* out, char* err) {
  int t1 = 0, t2 = 0;
  bool self = false;
  const std::string why = twin_sector(mode, ns, q1, q2, t1, t2, self);
  out[0] = t1;
  out[1] = t2;
  out[2] = self ? 1 : 0;
  return finish(why, err);
}

// tud: norb ups, then norb downs of the twin; returns self
int ht_twin_sector_orbs(int norb, const int32_t* nups, const int32_t* ndws, int32_t* tud) {
  std::vector<int> u(nups, nups + norb), d(ndws, ndws + norb), tu((size_t)norb), td((size_t)norb);
  bool self = false;
  twin_sector_orbs(norb, u.data(), d.data(), tu.data(), td.data(), self);
  for (int a = 0; a < norb; a++) {
    tud[a] = tu[(size_t)a];
    tud[norb + a] = td[(size_t)a];
  }
  return self ? 1 : 0;
}

// order: n entries
int ht_twin_order(int mode, const int32_t* map, int64_t n, int ns, int32_t* order, char* err) {
  std::vector<int32_t> o;
  const std::string why = twin_order(mode, map, n, ns, o);
  if (why.empty() && !o.empty()) std::memcpy(order, o.data(), o.size() * sizeof(int32_t));
  return finish(why, err);
}

}  // extern "C"
