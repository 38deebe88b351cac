// ctypes shim over csrc/host_rdm_flat.cpp for tests/test_rdm_flat_host.py (compiled with g++, no HIP).  With
// -DHRF_MAIN it is a stand-alone program (built with -fsanitize=address,undefined by the same test): it makes the sector
// map of every shape given on its command line, walks the host reference and the emulated work list at two widths and
// compares them.
#include "host_rdm_flat.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace edigpu;

static int fail(char* msg, const std::string& why) {
  std::snprintf(msg, 256, "%s", why.c_str());
  return 1;
}

extern "C" {

// 0 when the map has the structure of the sector, else 1 with the reason in msg (256 bytes); info[0..2] = ntri, the
// classes, the largest block
int hrf_tables(const int32_t* map, int64_t n, int ns, int norb, int mode, int q, int64_t* info, char* msg) {
  RdmFlatTables t;
  const std::string why = rdm_flat_tables(map, n, ns, norb, mode, q, t);
  if (!why.empty()) return fail(msg, why);
  info[0] = t.ntri;
  info[1] = t.nclass;
  info[2] = 0;
  for (int c = 0; c < t.nclass; c++) info[2] = info[2] > t.bn[c] ? info[2] : t.bn[c];
  return 0;
}

// dense[D][D] (cw doubles each) of one vector: which = 0 rdm_flat_host_reference, 1 the work list of the kernel emulated
// (rdm_flat_plan + rdm_flat_plan_emulate, target_wgs workgroups); info[0..4] = workgroups, groups, partial entries, LDS
// doubles, panels
int hrf_dense(const int32_t* map, int64_t n, int ns, int norb, int mode, int q, int nblk, const double* v, int cw, int which,
              int target_wgs, double* dense, int64_t* info, char* msg) {
  RdmFlatTables t;
  std::string why = rdm_flat_tables(map, n, ns, norb, mode, q, t);
  if (!why.empty()) return fail(msg, why);
  std::vector<double> tri((size_t)t.ntri * cw, 0.0);
  if (which == 0) {
    rdm_flat_host_reference(t, nblk, v, cw, tri.data());
  } else {
    RdmFlatPlan p;
    rdm_flat_plan(t, nblk, cw, target_wgs, p);
    why = rdm_flat_plan_emulate(p, t.ntri, n * nblk, v, cw, tri.data());
    if (!why.empty()) return fail(msg, why);
    info[0] = (int64_t)p.work.size();
    info[1] = (int64_t)p.groups.size();
    info[2] = p.partial_entries;
    info[3] = ((int64_t)p.stage_max + (int64_t)p.ept_max * kRdmFlatThreads) * cw + (p.rel_max + 3) / 4;
    info[4] = (int64_t)p.panels.size();
  }
  rdm_flat_place(t, tri.data(), cw, dense);
  return 0;
}

}  // extern "C"

#ifdef HRF_MAIN
static int popc(uint32_t x) {
  int c = 0;
  for (; x; x &= x - 1) c++;
  return c;
}

// arguments: groups of "ns norb mode q"
int main(int argc, char** argv) {
  for (int a = 1; a + 3 < argc; a += 4) {
    const int ns = std::atoi(argv[a]), norb = std::atoi(argv[a + 1]), mode = std::atoi(argv[a + 2]), q = std::atoi(argv[a + 3]);
    std::vector<int32_t> map;
    for (uint32_t d = 0; d < (1u << ns); d++) {
      const int nup = mode == 2 ? q - popc(d) : q + popc(d);
      for (uint32_t u = 0; u < (1u << ns); u++)
        if (popc(u) == nup) map.push_back((int32_t)(u | d << ns));
    }
    const int64_t n = (int64_t)map.size(), D = (int64_t)1 << (2 * norb);
    char msg[256] = "";
    for (int cw = 1; cw <= 2; cw++) {
      const int nblk = cw;  // the complex pass also has two phonon blocks
      std::vector<double> v((size_t)n * nblk * cw);
      uint64_t x = 88172645463325252ull + (uint64_t)a;
      double n2 = 0.0;
      for (double& e : v) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        e = (double)(x >> 11) / 9007199254740992.0 - 0.5;
        n2 += e * e;
      }
      std::vector<double> ref((size_t)(D * D * cw)), got((size_t)(D * D * cw));
      int64_t info[5] = {0};
      if (hrf_dense(map.data(), n, ns, norb, mode, q, nblk, v.data(), cw, 0, 0, ref.data(), info, msg)) {
        std::printf("FAIL ns=%d norb=%d mode=%d q=%d: %s\n", ns, norb, mode, q, msg);
        return 1;
      }
      for (int wgs : {2048, 3}) {
        if (hrf_dense(map.data(), n, ns, norb, mode, q, nblk, v.data(), cw, 1, wgs, got.data(), info, msg)) {
          std::printf("FAIL ns=%d norb=%d mode=%d q=%d wgs=%d: %s\n", ns, norb, mode, q, wgs, msg);
          return 1;
        }
        double err = 0.0;
        for (size_t i = 0; i < ref.size(); i++) err = std::fmax(err, std::fabs(ref[i] - got[i]));
        if (!(err <= 4.0 * (double)(n * nblk) * 1.1102230246251565e-16 * n2)) {
          std::printf("FAIL ns=%d norb=%d mode=%d q=%d wgs=%d: error %g\n", ns, norb, mode, q, wgs, err);
          return 1;
        }
      }
    }
    std::printf("ok ns=%d norb=%d mode=%d q=%d dim=%lld\n", ns, norb, mode, q, (long long)n);
  }
  return 0;
}
#endif
