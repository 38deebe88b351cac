// ctypes shim over csrc/host_rdm_flat.cpp for tests/test_rdm_flat_shard_host.py (compiled with g++, no HIP): the shard plan
// behind edigpu_imp_rdm_flat_sharded and its emulations.  With -DHFS_MAIN it is a stand-alone program (built with
// -fsanitize=address,undefined by the same test): it makes the sector map of every shape given on its command line and
// runs emulated worlds on integer vectors, whose sums must equal the host reference exactly.
#include "host_rdm_flat.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace edigpu;

static int fail(char* msg, const std::string& why) {
  std::snprintf(msg, 256, "%s", why.c_str());
  return 1;
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// "" when the two plans are equal field by field
static std::string plans_differ(const RdmFlatPlan& a, const RdmFlatPlan& b) {
  if (a.norb != b.norb || a.dim_el != b.dim_el) return "norb / dim_el";
  if (a.stage_max != b.stage_max || a.ept_max != b.ept_max || a.rel_max != b.rel_max) return "the LDS sizes";
  if (a.partial_entries != b.partial_entries) return "partial_entries";
  if (!same(a.rowstart, b.rowstart)) return "rowstart";
  if (!same(a.bdw, b.bdw)) return "bdw";
  if (!same(a.rel, b.rel)) return "rel";
  if (!same(a.ent, b.ent)) return "ent";
  if (!same(a.panels, b.panels)) return "panels";
  if (!same(a.work, b.work)) return "work";
  if (!same(a.groups, b.groups)) return "groups";
  return "";
}

extern "C" {

// The plan of the range (first, count) of `world`.  info = first count rank H q nslab_in tail_start tail_len tail_own
// tail_bdw nin nslab ngroups partial_entries npack nfill; heads[world]; pack / fill: rows of (sel, rank, src, dst, len),
// at most maxseg of them; in_bdw: the bath words of the nslab_in interior slabs (at most 2^(ns - norb)).
int hfs_plan(const int32_t* map, int64_t n, int ns, int norb, int mode, int q, int nblk, int cw, int target_wgs, int world,
             int64_t first, int64_t count, int64_t* info, int64_t* heads, int64_t* pack, int64_t* fill, int maxseg, int32_t* in_bdw,
             char* msg) {
  RdmFlatTables t;
  std::string why = rdm_flat_tables(map, n, ns, norb, mode, q, t);
  if (!why.empty()) return fail(msg, why);
  RdmFlatShardPlan p;
  why = rdm_flat_shard_plan(t, nblk, cw, target_wgs, world, first, count, p);
  if (!why.empty()) return fail(msg, why);
  if ((int)p.pack.size() > maxseg || (int)p.fill.size() > maxseg) return fail(msg, "more segments than the caller holds");
  const int64_t v[16] = {p.first,    p.count,    p.rank,     p.H,        p.q,        p.nslab_in, p.tail_start, p.tail_len,
                         p.tail_own, p.tail_bdw, (int64_t)p.in.work.size(), (int64_t)p.slab.work.size(), (int64_t)p.groups.size(),
                         p.partial_entries, (int64_t)p.pack.size(), (int64_t)p.fill.size()};
  std::memcpy(info, v, sizeof(v));
  for (int r = 0; r < world; r++) heads[r] = p.heads[(size_t)r];
  auto put = [](const std::vector<RdmFlatSeg>& s, int64_t* out) {
    for (size_t i = 0; i < s.size(); i++) {
      const int64_t row[5] = {s[i].sel, s[i].rank, s[i].src, s[i].dst, s[i].len};
      std::memcpy(out + 5 * i, row, sizeof(row));
    }
  };
  put(p.pack, pack);
  put(p.fill, fill);
  for (int32_t b : p.in.bdw)  // (the lists also hold the bath words whose slab is empty)
    if (t.rowstart[(size_t)b << norb] != t.rowstart[(size_t)(b + 1) << norb]) *in_bdw++ = b;
  return 0;
}

// 0 when the shard plan of the whole sector (world 1) equals rdm_flat_plan field by field
int hfs_whole_equals_plan(const int32_t* map, int64_t n, int ns, int norb, int mode, int q, int nblk, int cw, int target_wgs,
                          char* msg) {
  RdmFlatTables t;
  std::string why = rdm_flat_tables(map, n, ns, norb, mode, q, t);
  if (!why.empty()) return fail(msg, why);
  RdmFlatPlan whole;
  rdm_flat_plan(t, nblk, cw, target_wgs, whole);
  RdmFlatShardPlan p;
  why = rdm_flat_shard_plan(t, nblk, cw, target_wgs, 1, 0, n, p);
  if (!why.empty()) return fail(msg, why);
  why = plans_differ(p.in, whole);
  if (!why.empty()) return fail(msg, "the plans differ in " + why);
  if (!same(p.groups, whole.groups) || p.partial_entries != whole.partial_entries) return fail(msg, "the groups differ");
  if (p.H != 0 || p.tail_len != 0 || !p.pack.empty() || !p.fill.empty() || !p.slab.work.empty()) return fail(msg, "a world of one has a halo");
  return 0;
}

int hfs_reference(const int32_t* map, int64_t n, int ns, int norb, int mode, int q, int nblk, int cw, const double* v, double* tri,
                  char* msg) {
  RdmFlatTables t;
  const std::string why = rdm_flat_tables(map, n, ns, norb, mode, q, t);
  if (!why.empty()) return fail(msg, why);
  std::fill(tri, tri + t.ntri * cw, 0.0);
  rdm_flat_host_reference(t, nblk, v, cw, tri);
  return 0;
}

// tri[ntri cw] = the sums of an emulated world on v[nblk][n]; *H = its halo
int hfs_world(const int32_t* map, int64_t n, int ns, int norb, int mode, int q, int nblk, int cw, int target_wgs, int world,
              const double* v, double* tri, int64_t* H, char* msg) {
  RdmFlatTables t;
  std::string why = rdm_flat_tables(map, n, ns, norb, mode, q, t);
  if (!why.empty()) return fail(msg, why);
  why = rdm_flat_world_emulate(t, nblk, cw, target_wgs, world, v, tri, H);
  return why.empty() ? 0 : fail(msg, why);
}

int64_t hfs_ntri(const int32_t* map, int64_t n, int ns, int norb, int mode, int q) {
  RdmFlatTables t;
  return rdm_flat_tables(map, n, ns, norb, mode, q, t).empty() ? t.ntri : -1;
}

}  // extern "C"

#ifdef HFS_MAIN
static int popc(uint32_t x) {
  int c = 0;
  for (; x; x &= x - 1) c++;
  return c;
}

// arguments: groups of "ns norb mode q"
int main(int argc, char** argv) {
  int failures = 0;
  for (int a = 1; a + 3 < argc; a += 4) {
    const int ns = std::atoi(argv[a]), norb = std::atoi(argv[a + 1]), mode = std::atoi(argv[a + 2]), q = std::atoi(argv[a + 3]);
    std::vector<int32_t> map;
    for (uint32_t d = 0; d < (1u << ns); d++) {
      const int nup = mode == 2 ? q - popc(d) : q + popc(d);
      for (uint32_t u = 0; u < (1u << ns); u++)
        if (popc(u) == nup) map.push_back((int32_t)(u | d << ns));
    }
    const int64_t n = (int64_t)map.size(), ntri = hfs_ntri(map.data(), n, ns, norb, mode, q);
    char msg[256] = "";
    if (ntri < 0) {
      std::printf("FAIL ns=%d norb=%d mode=%d q=%d: no tables\n", ns, norb, mode, q);
      failures++;
      continue;
    }
    for (int cw = 1; cw <= 2; cw++)
      for (int nblk : {1, 4}) {
        std::vector<double> v((size_t)(n * nblk * cw));
        uint64_t x = 88172645463325252ull + (uint64_t)(a + 7 * cw + nblk);
        for (double& e : v) {
          x ^= x << 13, x ^= x >> 7, x ^= x << 17;
          e = (double)(int)(x % 17) - 8.0;
        }
        std::vector<double> ref((size_t)(ntri * cw)), got((size_t)(ntri * cw));
        if (hfs_reference(map.data(), n, ns, norb, mode, q, nblk, cw, v.data(), ref.data(), msg)) {
          std::printf("FAIL ns=%d norb=%d mode=%d q=%d: %s\n", ns, norb, mode, q, msg);
          failures++;
          continue;
        }
        for (int wgs : {2048, 3}) {
          if (hfs_whole_equals_plan(map.data(), n, ns, norb, mode, q, nblk, cw, wgs, msg)) {
            std::printf("FAIL ns=%d norb=%d mode=%d q=%d wgs=%d: %s\n", ns, norb, mode, q, wgs, msg);
            failures++;
          }
          for (int world : {1, 2, 3, 5, 10}) {
            int64_t H = -1;
            if (hfs_world(map.data(), n, ns, norb, mode, q, nblk, cw, wgs, world, v.data(), got.data(), &H, msg)) {
              std::printf("FAIL ns=%d norb=%d mode=%d q=%d world=%d: %s\n", ns, norb, mode, q, world, msg);
              failures++;
            } else if (got != ref) {
              std::printf("FAIL ns=%d norb=%d mode=%d q=%d world=%d: the sums differ from the reference\n", ns, norb, mode, q, world);
              failures++;
            }
          }
        }
      }
    std::printf("ok ns=%d norb=%d mode=%d q=%d dim=%lld\n", ns, norb, mode, q, (long long)n);
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
#endif
