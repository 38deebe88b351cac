// extern "C" wrapper of csrc/host_axisop.cpp for tests/test_axisop_host.py (g++, no HIP).
#include <cstring>
#include <vector>

#include "host_axisop.hpp"

using namespace edigpu;

static std::vector<AxisOp> ops_of(int nterms, const int32_t* o) {
  std::vector<AxisOp> v;
  for (int k = 0; k < nterms && k < 64; k++) v.push_back(AxisOp{o[3 * k], o[3 * k + 1], o[3 * k + 2]});
  return v;
}

static int finish(const std::string& why, const AxisTables& t, int64_t* shape, uint32_t* part, char* err) {
  std::strncpy(err, why.c_str(), 255);
  err[255] = 0;
  if (!why.empty()) return 1;
  const int64_t v[5] = {t.I, t.a_src, t.a_dst, t.O, (int64_t)t.part.size()};
  std::memcpy(shape, v, sizeof(v));
  if (part && !t.part.empty()) std::memcpy(part, t.part.data(), t.part.size() * sizeof(uint32_t));
  return 0;
}

extern "C" {

// ops: nterms x (create, iorb, ispin); shape: I, a_src, a_dst, O, entries of part; dest: nup, ndw; part may be NULL
// (sizes only); err: 256 bytes.  Returns 0, or 1 with the reason in err.
int ha_build_normal(int nup, int ndw, int ns, int norb, int nblk, int cplx, int nterms, const int32_t* ops, int32_t* dest,
                    int64_t* shape, uint32_t* part, char* err) {
  const std::vector<AxisOp> o = ops_of(nterms, ops);
  AxisTables t;
  int nu = 0, nd = 0;
  const std::string why = axisop_build_normal(nup, ndw, ns, norb, nblk, cplx != 0, nterms, o.data(), nu, nd, t);
  dest[0] = nu;
  dest[1] = nd;
  return finish(why, t, shape, part, err);
}

// dest: norb ups, then norb downs
int ha_build_orbs(int norb, int nbath, const int32_t* nups, const int32_t* ndws, int nterms, const int32_t* ops, int32_t* dest,
                  int64_t* shape, uint32_t* part, char* err) {
  const std::vector<AxisOp> o = ops_of(nterms, ops);
  AxisTables t;
  std::vector<int> u(nups, nups + norb), d(ndws, ndws + norb), u2((size_t)norb), d2((size_t)norb);
  const std::string why = axisop_build_orbs(norb, nbath, u.data(), d.data(), nterms, o.data(), u2.data(), d2.data(), t);
  for (int a = 0; a < norb; a++) {
    dest[a] = u2[(size_t)a];
    dest[norb + a] = d2[(size_t)a];
  }
  return finish(why, t, shape, part, err);
}

}  // extern "C"
