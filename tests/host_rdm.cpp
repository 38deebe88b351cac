// ctypes shim over csrc/host_rdm.cpp for tests/test_rdm_host.py (compiled with g++, no HIP).
#include "host_rdm.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace edigpu;

static int fail(char* msg, const std::string& why) {
  std::snprintf(msg, 256, "%s", why.c_str());
  return 1;
}

extern "C" {

// nk: 6, pat_of: 6 x 10, rank_of: 32
void hr_ranks(int norb, int32_t* nk, uint8_t* pat_of, uint8_t* rank_of) {
  RdmRanks r;
  rdm_rank_tables(norb, r);
  for (int k = 0; k <= kRdmMaxOrb; k++) nk[k] = r.nk[k];
  std::memcpy(pat_of, r.pat_of, sizeof(r.pat_of));
  std::memcpy(rank_of, r.rank_of, sizeof(r.rank_of));
}

// start: n + 1 entries, k: n entries at the most; returns the number of runs, -1 with msg (256 bytes) on refusal
int64_t hr_runs(const int32_t* map, int64_t n, int norb, int32_t* start, uint8_t* k, char* msg) {
  RdmRanks r;
  rdm_rank_tables(norb, r);
  RdmRuns runs;
  const std::string why = rdm_runs(map, n, norb, r, runs);
  if (!why.empty()) return fail(msg, why) ? -1 : -1;
  std::memcpy(start, runs.start.data(), runs.start.size() * sizeof(int32_t));
  if (!runs.k.empty()) std::memcpy(k, runs.k.data(), runs.k.size());
  return (int64_t)runs.k.size();
}

int64_t hr_ntri(int norb) {
  RdmRanks r;
  RdmLayout l;
  rdm_rank_tables(norb, r);
  rdm_layout(r, l);
  return l.ntri;
}

// dense[D][D] (cw doubles each) of one vector: which = 0 rdm_host_reference, 1 the work list of the kernel emulated
// (rdm_plan + rdm_plan_emulate, target_wgs workgroups); info[0..3] = workgroups, groups, partial entries, LDS doubles
int hr_dense(const int32_t* mu, int64_t nu, const int32_t* md, int64_t nd, int norb, int nblk, const double* v, int cw,
             int which, int target_wgs, double* dense, int64_t* info, char* msg) {
  RdmRanks r;
  RdmLayout l;
  rdm_rank_tables(norb, r);
  rdm_layout(r, l);
  RdmRuns up, dw;
  std::string why = rdm_runs(mu, nu, norb, r, up);
  if (why.empty()) why = rdm_runs(md, nd, norb, r, dw);
  if (!why.empty()) return fail(msg, why);
  std::vector<double> tri((size_t)l.ntri * cw, 0.0);
  if (which == 0) {
    rdm_host_reference(r, l, up, dw, nu, nd, nblk, v, cw, tri.data());
  } else {
    RdmPlan p;
    rdm_plan(r, l, up, dw, nu, nd, nblk, cw, target_wgs, p);
    why = rdm_plan_emulate(p, l.ntri, nu * nd * nblk, nu, nd, v, cw, tri.data());
    if (!why.empty()) return fail(msg, why);
    info[0] = (int64_t)p.work.size();
    info[1] = (int64_t)p.groups.size();
    info[2] = p.partial_entries;
    info[3] = ((int64_t)p.ld_max * p.stride + (int64_t)p.ept_max * kRdmThreads) * cw;
  }
  rdm_place(r, l, tri.data(), cw, dense);
  return 0;
}

}  // extern "C"
