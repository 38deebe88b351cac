// ctypes shim over the shard plan of csrc/host_rdm.cpp (RdmShardPlan) for tests/test_rdm_shard_host.py, compiled with g++
// (no HIP); tests/host_rdm_shard_sanitize_main.cpp links the same functions into a stand-alone program.
#include "host_rdm.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace edigpu;

namespace {

int fail(char* msg, const std::string& why) {
  std::snprintf(msg, 256, "%s", why.c_str());
  return 1;
}

struct Sector {
  RdmRanks rk;
  RdmLayout l;
  RdmRuns up, dw;
  int64_t nu = 0, nd = 0;
};

std::string sector(const int32_t* mu, int64_t nu, const int32_t* md, int64_t nd, int norb, Sector& s) {
  rdm_rank_tables(norb, s.rk);
  rdm_layout(s.rk, s.l);
  s.nu = nu;
  s.nd = nd;
  std::string why = rdm_runs(mu, nu, norb, s.rk, s.up);
  if (why.empty()) why = rdm_runs(md, nd, norb, s.rk, s.dw);
  return why;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

}  // namespace

extern "C" {

// The plan of the rows [first, first + count) (uncut) of `world` ranges.  info[16]: first, count, rank, H, tail_row,
// tail_own, tail_ld, tail_k, workgroups of `in`, of `slab`, groups, partial entries, interior runs, q.  heads[world];
// in_start / in_len [nd]: the interior runs (start relative to first, length); pack / fill: 3 x 10 (sel, rank, row) and
// their nrows in rows[2].
int hrs_plan(const int32_t* mu, int64_t nu, const int32_t* md, int64_t nd, int norb, int nblk, int cw, int target_wgs, int world,
             int64_t first, int64_t count, int64_t* info, int32_t* heads, int32_t* in_start, int32_t* in_len, int32_t* pack,
             int32_t* fill, int32_t* rows, char* msg) {
  Sector s;
  std::string why = sector(mu, nu, md, nd, norb, s);
  if (!why.empty()) return fail(msg, why);
  RdmShardPlan p;
  why = rdm_shard_plan(s.rk, s.l, s.up, s.dw, nu, nd, nblk, cw, target_wgs, world, first, count, p);
  if (!why.empty()) return fail(msg, why);
  const int64_t out[14] = {p.first, p.count, p.rank, p.H, p.tail_row, p.tail_own, p.tail_ld, p.tail_k, (int64_t)p.in.work.size(),
                           (int64_t)p.slab.work.size(), (int64_t)p.groups.size(), p.partial_entries, 0, p.q};
  std::copy(out, out + 14, info);
  std::copy(p.heads.begin(), p.heads.end(), heads);
  // the interior runs as the device walks them: p.in.rows holds their starts class after class
  int64_t n = 0;
  for (const RdmWork& w : p.in.work)
    for (int32_t j = 0; j < w.nruns; j++) {
      const int32_t st = p.in.rows[(size_t)(w.row_list + j)];
      bool seen = false;
      for (int64_t i = 0; i < n; i++) seen = seen || in_start[i] == st;
      if (seen) continue;
      if (n >= nd) return fail(msg, "more interior runs than rows");
      in_start[n] = st;
      in_len[n++] = w.ld;
    }
  info[12] = n;
  for (int which = 0; which < 2; which++) {
    const RdmRowCopy& t = which ? p.fill : p.pack;
    int32_t* o = which ? fill : pack;
    rows[which] = t.nrows;
    for (int i = 0; i < kRdmMaxRun; i++) {
      o[i] = t.sel[i];
      o[kRdmMaxRun + i] = t.rank[i];
      o[2 * kRdmMaxRun + i] = t.row[i];
    }
  }
  return 0;
}

// 0 when the shard plan of the whole sector in a world of one equals rdm_plan of the sector field by field
int hrs_whole_equals_plan(const int32_t* mu, int64_t nu, const int32_t* md, int64_t nd, int norb, int nblk, int cw,
                          int target_wgs, char* msg) {
  Sector s;
  std::string why = sector(mu, nu, md, nd, norb, s);
  if (!why.empty()) return fail(msg, why);
  RdmShardPlan p;
  why = rdm_shard_plan(s.rk, s.l, s.up, s.dw, nu, nd, nblk, cw, target_wgs, 1, 0, nd, p);
  if (!why.empty()) return fail(msg, why);
  RdmPlan w;
  rdm_plan(s.rk, s.l, s.up, s.dw, nu, nd, nblk, cw, target_wgs, w);
  const RdmPlan& a = p.in;
  if (a.stride != w.stride || a.ld_max != w.ld_max || a.ept_max != w.ept_max || a.rel_max != w.rel_max) return fail(msg, "sizes differ");
  if (a.partial_entries != w.partial_entries || p.partial_entries != w.partial_entries) return fail(msg, "partial_entries differ");
  if (!same(a.rows, w.rows) || !same(a.rel, w.rel) || !same(a.ent, w.ent)) return fail(msg, "tables differ");
  if (a.work.size() != w.work.size() || p.groups.size() != w.groups.size()) return fail(msg, "list lengths differ");
  for (size_t i = 0; i < w.work.size(); i++) {
    const RdmWork &x = a.work[i], &y = w.work[i];
    if (x.row_list != y.row_list || x.nruns != y.nruns || x.j0 != y.j0 || x.j1 != y.j1 || x.ld != y.ld || x.c0 != y.c0 ||
        x.clen != y.clen || x.rel0 != y.rel0 || x.e0 != y.e0 || x.e1 != y.e1 || x.pad != y.pad || x.pofs != y.pofs ||
        std::memcmp(x.kb, y.kb, sizeof(x.kb)) != 0)
      return fail(msg, "workgroup " + std::to_string(i) + " differs");
  }
  for (size_t i = 0; i < w.groups.size(); i++) {
    const RdmGroup &x = p.groups[i], &y = w.groups[i];
    if (x.e0 != y.e0 || x.e1 != y.e1 || x.nwg != y.nwg || x.pad != y.pad || x.pbase != y.pbase) return fail(msg, "a group differs");
  }
  if (p.H != 0 || p.tail_ld != 0 || !p.slab.work.empty() || p.pack.nrows != 0 || p.fill.nrows != 0) return fail(msg, "a halo or a slab in a world of one");
  return 0;
}

// packed triangles (ntri * cw doubles) of v[nblk][nd][nu] by rdm_host_reference
int hrs_reference(const int32_t* mu, int64_t nu, const int32_t* md, int64_t nd, int norb, int nblk, int cw, const double* v,
                  double* tri, char* msg) {
  Sector s;
  const std::string why = sector(mu, nu, md, nd, norb, s);
  if (!why.empty()) return fail(msg, why);
  std::fill(tri, tri + s.l.ntri * cw, 0.0);
  rdm_host_reference(s.rk, s.l, s.up, s.dw, nu, nd, nblk, v, cw, tri);
  return 0;
}

// The whole sharded call on the host for `world` ranks, each asked with its uncut range (r q, q): every rank packs its
// halo, the halos are gathered, every rank fills its slab and walks its two work lists (all emulations, every index
// checked); tri = the packed sums added over the ranks in rank order.  hmax[0] = H.
int hrs_world(const int32_t* mu, int64_t nu, const int32_t* md, int64_t nd, int norb, int nblk, int cw, int target_wgs, int world,
              const double* v, double* tri, int64_t* hmax, char* msg) {
  Sector s;
  std::string why = sector(mu, nu, md, nd, norb, s);
  if (!why.empty()) return fail(msg, why);
  const int64_t q = (nd + world - 1) / world, rowlen = nu * cw, ntri = s.l.ntri;
  std::vector<RdmShardPlan> plans((size_t)world);
  for (int r = 0; r < world; r++) {
    why = rdm_shard_plan(s.rk, s.l, s.up, s.dw, nu, nd, nblk, cw, target_wgs, world, (int64_t)r * q, q, plans[(size_t)r]);
    if (!why.empty()) return fail(msg, "rank " + std::to_string(r) + ": " + why);
    if (plans[(size_t)r].H != plans[0].H || plans[(size_t)r].heads != plans[0].heads) return fail(msg, "the ranks disagree on the halo");
  }
  const int H = plans[0].H;
  hmax[0] = H;
  if (H > kRdmMaxRun - 1) return fail(msg, "H exceeds kRdmMaxRun - 1");
  auto shard_of = [&](const RdmShardPlan& p) {
    std::vector<double> sh((size_t)(nblk * p.count * rowlen));
    for (int b = 0; b < nblk; b++)
      for (int64_t i = 0; i < p.count * rowlen; i++) sh[(size_t)(b * p.count * rowlen + i)] = v[(b * nd + p.first) * rowlen + i];
    return sh;
  };
  const int64_t hlen = (int64_t)nblk * H * rowlen;
  std::vector<double> halos((size_t)(hlen * world), -77.0);
  for (int r = 0; r < world; r++) {
    const RdmShardPlan& p = plans[(size_t)r];
    const std::vector<double> sh = shard_of(p);
    why = rdm_rows_emulate(p, p.pack, nblk, rowlen, p.count ? sh.data() : nullptr, nullptr, halos.data() + (size_t)(r * hlen));
    if (!why.empty()) return fail(msg, "pack of rank " + std::to_string(r) + ": " + why);
  }
  std::fill(tri, tri + ntri * cw, 0.0);
  std::vector<double> mine((size_t)(ntri * cw));
  for (int r = 0; r < world; r++) {
    const RdmShardPlan& p = plans[(size_t)r];
    const std::vector<double> sh = shard_of(p);
    std::vector<double> slab((size_t)((int64_t)nblk * p.tail_ld * rowlen), -99.0);
    why = rdm_rows_emulate(p, p.fill, nblk, rowlen, p.count ? sh.data() : nullptr, halos.data(), slab.data());
    if (!why.empty()) return fail(msg, "slab of rank " + std::to_string(r) + ": " + why);
    why = rdm_shard_emulate(p, ntri, nu, nblk, p.count ? sh.data() : nullptr, p.tail_ld ? slab.data() : nullptr, cw, mine.data());
    if (!why.empty()) return fail(msg, "rank " + std::to_string(r) + ": " + why);
    for (int64_t i = 0; i < ntri * cw; i++) tri[i] += mine[(size_t)i];
  }
  return 0;
}

}  // extern "C"
