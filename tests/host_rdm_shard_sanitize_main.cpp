// Stand-alone driver of the shard plan of csrc/host_rdm.cpp for tests/test_rdm_shard_host.py: the whole sharded call
// emulated on the host (tests/host_rdm_shard.cpp hrs_world) for two, three and five orbitals, worlds of 1 .. 10 ranks,
// 1 and 4 phonon blocks, real and complex vectors, built with -fsanitize=address,undefined and run as a program.  The
// vectors hold small integers, so the ranks' sums must equal rdm_host_reference exactly.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host_rdm.hpp"

using namespace edigpu;

extern "C" {
int hrs_reference(const int32_t* mu, int64_t nu, const int32_t* md, int64_t nd, int norb, int nblk, int cw, const double* v,
                  double* tri, char* msg);
int hrs_world(const int32_t* mu, int64_t nu, const int32_t* md, int64_t nd, int norb, int nblk, int cw, int target_wgs, int world,
              const double* v, double* tri, int64_t* hmax, char* msg);
int hrs_whole_equals_plan(const int32_t* mu, int64_t nu, const int32_t* md, int64_t nd, int norb, int nblk, int cw,
                          int target_wgs, char* msg);
}

static int failures = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);    \
      failures++;                                            \
    }                                                        \
  } while (0)

static uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// the sector map of one spin: the words of ns bits with n bits set, ascending
static std::vector<int32_t> spin_map(int ns, int n) {
  std::vector<int32_t> m;
  for (int32_t w = 0; w < (1 << ns); w++)
    if (__builtin_popcount((unsigned)w) == n) m.push_back(w);
  return m;
}

int main() {
  uint32_t seed = 2024u;
  char msg[256] = {0};
  const int shapes[][4] = {{2, 5, 2, 3}, {3, 6, 3, 2}, {3, 6, 3, 1}, {5, 7, 3, 4}};  // norb, ns, nup, ndw
  for (const auto& sh : shapes) {
    const int norb = sh[0];
    const std::vector<int32_t> mu = spin_map(sh[1], sh[2]), md = spin_map(sh[1], sh[3]);
    const int64_t nu = (int64_t)mu.size(), nd = (int64_t)md.size();
    RdmRanks rk;
    RdmLayout l;
    rdm_rank_tables(norb, rk);
    rdm_layout(rk, l);
    for (int nblk : {1, 4})
      for (int cw : {1, 2}) {
        std::vector<double> v((size_t)(nblk * nu * nd * cw));
        for (double& x : v) x = (double)((int)(rnd(seed) >> 16) % 17 - 8);
        std::vector<double> ref((size_t)(l.ntri * cw)), tri((size_t)(l.ntri * cw));
        CHECK(hrs_reference(mu.data(), nu, md.data(), nd, norb, nblk, cw, v.data(), ref.data(), msg) == 0);
        CHECK(hrs_whole_equals_plan(mu.data(), nu, md.data(), nd, norb, nblk, cw, 64, msg) == 0);
        for (int world : {1, 2, 3, 5, 10}) {
          int64_t H = -1;
          const int rc = hrs_world(mu.data(), nu, md.data(), nd, norb, nblk, cw, world == 3 ? 3 : 2048, world, v.data(), tri.data(), &H, msg);
          if (rc) std::printf("norb %d nd %lld world %d: %s\n", norb, (long long)nd, world, msg);
          CHECK(rc == 0 && H >= 0 && H <= kRdmMaxRun - 1);
          CHECK(world > 1 || H == 0);
          CHECK(tri == ref);
        }
      }
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
