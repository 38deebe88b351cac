// CPU-side sanitizer harness (ASan + UBSan) for the host builders of libedigpu (csrc/host_build.cpp): every bath type,
// mode and sector of a few small models, shards included; the image encoders of the generic kernels (csrc/host_pack.cpp)
// on one sector with Hnd terms; the three snapshots of the environment switches (csrc/switches.cpp).  Built and run by
// tests/test_host_sanitizers.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include "host_build.hpp"
#include "host_ib.hpp"
#include "host_pack.hpp"
#include "switches.hpp"
using namespace edigpu;
static void fill(edigpu_model& m, int mode, int bath, int norb, int nbath) {
  memset(&m, 0, sizeof(m));
  m.ed_mode = mode; m.bath_type = bath; m.norb = norb; m.nbath = nbath; m.nspin = mode == 2 ? 2 : 1; m.hfmode = 1;
  std::mt19937 g(7); std::uniform_real_distribution<double> u(0.1, 0.6), e(-2, 2);
  for (int a = 0; a < norb; a++) { m.uloc[a] = 2.0; for (int b = 0; b < norb; b++) if (a != b) { m.ust[a*EDIGPU_MAXORB+b] = 1.5; m.jh[a*EDIGPU_MAXORB+b] = 0.25; m.jx[a*EDIGPU_MAXORB+b] = bath==0&&mode==0? 0.25:0.25; m.jp[a*EDIGPU_MAXORB+b] = 0.25; } }
  for (int s = 0; s < 2; s++) for (int a = 0; a < norb; a++) for (int k = 0; k < nbath; k++) {
    m.bv[(s*EDIGPU_MAXORB+a)*EDIGPU_MAXBATH+k] = u(g); m.be[(s*EDIGPU_MAXORB+a)*EDIGPU_MAXBATH+k] = e(g);
    m.bd[(s*EDIGPU_MAXORB+a)*EDIGPU_MAXBATH+k] = 0.05; m.bu[(s*EDIGPU_MAXORB+a)*EDIGPU_MAXBATH+k] = 0.1; }
  for (int is = 0; is < 2; is++) for (int js = 0; js < 2; js++) for (int a = 0; a < norb; a++) for (int b = 0; b < norb; b++) for (int k = 0; k < nbath; k++) {
    double* p = &m.hb[(((((is*2)+js)*EDIGPU_MAXORB+a)*EDIGPU_MAXORB+b)*EDIGPU_MAXBATH+k)*2];
    p[0] = (a==b && is==js) ? e(g) : 0.1; p[1] = 0.0; }
}
static bool mode_jz(int bath, int norb, int nbath) { return norb == 3 && (bath >= 2 || nbath == 1) && 2 * (bath == 1 ? nbath + norb : (nbath + 1) * norb) <= 14; }
// every encoder of host_pack.hpp on the sector (4, 4) of norb = 2, nbath = 3 (Jx = Jp != 0: Hnd terms), whole and as a sub-range
static int pack_images() {
  edigpu_model m; fill(m, 0, 0, 2, 3);
  HostNormal hn; if (!build_normal(m, 4, 4, 0, -1, hn, false).empty() || !hn.fac.valid || hn.fac.nterms == 0) return 1;
  int nell = 0, nsell = 0, nlist = 0, nblk = 0;
  for (int lds = 0; lds < 2; lds++) for (int opt = 0; opt < 3; opt++) nell += !encode_ell(hn.up, lds != 0, opt != 1, opt != 2).pk.empty();
  HostCsr many;  // 130 distinct |values| on 65 rows: the plain ELL image; 260 values: the plain SELL image
  many.nrow = many.ncol = 65; many.rowptr.push_back(0);
  for (int i = 0; i < 65; i++) { for (int j = 0; j < 4; j++) { many.col.push_back((i + 7 * j) % 65); many.val.push_back(1.0 + 0.01 * (4 * i + j)); } many.rowptr.push_back((int64_t)many.col.size()); }
  nell += !encode_ell(many, true, true, true).col.empty();
  for (int loc = 0; loc < 2; loc++) for (int pk = 0; pk < 2; pk++) {
    nsell += encode_sell(hn.dw.nrow, hn.dw.ncol, hn.dw.rowptr.data(), hn.dw.col.data(), hn.dw.val.data(), 0, loc != 0, 16.0, pk != 0).built;
    nsell += encode_sell(many.nrow, many.ncol, many.rowptr.data(), many.col.data(), many.val.data(), 0, loc != 0, 16.0, pk != 0).built;
  }
  std::vector<double> zv(many.val.size() * 2, 0.5);  // the same pattern as a complex block
  nsell += encode_sell(many.nrow, many.ncol, many.rowptr.data(), many.col.data(), zv.data(), 1, true, 16.0, true).built;
  for (int sub = 0; sub < 2; sub++) for (int rmax : {8, 64}) {
    const int64_t first = sub ? 5 : 0, count = sub ? 40 : hn.dim_dw;
    std::vector<int32_t> starts; int longest = 0;
    plan_tile_chunks(hn.dw, first, count, rmax, starts, longest);
    nlist += !build_tile_lists(hn.dw, hn.dim_dw, first, count, starts, &hn.fac).col.empty();
    nlist += !build_tile_lists(hn.dw, hn.dim_dw, first, count, starts, nullptr).col.empty();
    nlist += !merge_dw_lists(hn.dw, hn.fac, first, count, hn.dim_dw).col.empty();
  }
  for (int shift = 4; shift <= 6; shift++) for (int kb : {4, 32}) nblk += build_block_lists(hn.dw, hn.fac, hn.dim_dw, shift, kb).fits;
  const int halo = factored_col_halo(hn.fac, hn.dim_up);
  // every image was built
  if (nell == 7 && nsell == 9 && nlist == 12 && nblk == 6 && halo > 0) return 0;
  printf("host_pack: %d of 7 ELL, %d of 9 SELL, %d of 12 tile / merged lists, %d of 6 block lists, col_halo %d\n", nell, nsell, nlist, nblk, halo);
  return 1;
}
// the three snapshots with an empty environment, with every switch set to "" and to 4 KiB of digits (out of every range)
static int switch_snapshots() {
  int n = 0, bad = 0;
  const SwitchRow* rows = switch_table(&n);
  const std::string digits(4096, '7');
  clearenv();
  for (const char* text : {(const char*)nullptr, "", digits.c_str()}) {
    for (int i = 0; text && i < n; i++) setenv(rows[i].name, text, 1);
    const Switches sw = Switches::sample();
    const CommSwitches cs = CommSwitches::sample();
    const LoopSwitches ls = LoopSwitches::sample();
    const bool given = text != nullptr, empty = given && !text[0];
    bad += sw.lanczos_unfused != given || cs.force_collectives != given || ls.lanczos_exactbeta != given;  // presence
    bad += sw.ell16 != !empty || sw.posrows != (given && !empty) || sw.normal_explicit;                    // atoi, first character
    bad += sw.rows_td.has_value() != given || ls.trl_thr.has_value() != given;                              // derived defaults
    if (!given || empty)  // (what atoi makes of 4 KiB of digits is the C library's business: only that nothing breaks)
      bad += sw.ib_rows != (empty ? 4 : 480) || sw.tile_rows != (empty ? 8 : 32) || sw.ib_min_row_bytes() != (empty ? 0 : 40 * 1024);
  }
  clearenv();
  if (bad) printf("switch snapshots: %d wrong values\n", bad);
  return bad != 0;
}
int main() {
  int nfail = pack_images() + switch_snapshots(), nib = 0, njz = 0;
  for (int bath = 0; bath < 4; bath++) for (int norb = 1; norb <= 3; norb++) for (int nbath = 1; nbath <= 3; nbath++) {
    edigpu_model m; fill(m, 0, bath, norb, nbath);
    int ns = model_ns(m);
    for (int nup = 0; nup <= ns; nup += 1) for (int ndw = 0; ndw <= ns; ndw += 2) {
      HostNormal hn; std::string e = build_normal(m, nup, ndw, 0, -1, hn, (nup + ndw) % 3 == 0);
      if (!e.empty()) { printf("normal %d %d %d (%d,%d): %s\n", bath, norb, nbath, nup, ndw, e.c_str()); nfail++; }
      if (hn.dim_dw > 2) { HostNormal h2; e = build_normal(m, nup, ndw, 1, hn.dim_dw - 2, h2, true); if (!e.empty()) nfail++; }
      // the impurity-block image (csrc/host_ib.cpp): whole rows, rows in two halves, small chunks; a refusal is fine
      if (e.empty() && hn.dim_up > 0 && hn.dim_dw > 0) {
        HostNormal hf2; std::string e3 = build_normal(m, nup, ndw, 0, -1, hf2, true);
        if (e3.empty()) { HostIb a, b, c; build_ib(hf2, 480, a); build_ib(hf2, 6, b, -1); build_ib(hf2, 24, c, 64); nib += a.valid + b.valid + c.valid; }
      }
    }
    for (int mode = 1; mode <= 2; mode++) {
      fill(m, mode, bath, norb, nbath);
      if (2 * ns > 14) continue;
      for (int sec = (mode == 1 ? -ns : 0); sec <= (mode == 1 ? ns : 2 * ns); sec++) {
        HostFlat hf; std::string e = build_flat(m, sec, 0, -1, hf);
        HostDirect hd; std::string e2 = build_direct(m, sec, 0, -1, hd);
        if (!e.empty() || !e2.empty()) { printf("flat %d %d %d %d sec %d: %s %s\n", mode, bath, norb, nbath, sec, e.c_str(), e2.c_str()); nfail++; }
        if (hf.dim != hd.dim) nfail++;
        if (hf.dim > 3) { HostFlat h2; build_flat(m, sec, 1, hf.dim - 2, h2); HostDirect d2; build_direct(m, sec, 2, hf.dim - 3, d2); }
      }
    }
    if (mode_jz(bath, norb, nbath)) {
      // Jz_basis sectors: the map and the on-the-fly description (two-table rank inside (occupation, Lz) classes); this
      // model does not conserve Jz, so build_direct must refuse it after building the tables
      fill(m, 2, bath, norb, nbath);
      for (int ntot = 0; ntot <= 2 * ns; ntot += 3) for (int tj = -3; tj <= 3; tj += 2) {
        std::vector<int32_t> st; std::string e = sector_map_jz(m, ntot, tj, st);
        if (!e.empty()) { printf("jz map: %s\n", e.c_str()); nfail++; }
        HostDirect hd; e = build_direct(m, ntot, 0, -1, hd, true, tj);
        njz += (int)st.size() > 0;
        if (e.empty() && hd.dim != (int64_t)st.size()) nfail++;
      }
    }
    if (bath == 0) {
      fill(m, 0, 0, norb, nbath);
      int nups[3] = {1, 0, nbath + 1}, ndws[3] = {0, 1, 1};
      HostOrbs ho; std::string e = build_orbs(m, nups, ndws, ho, true);
      if (!e.empty()) { printf("orbs: %s\n", e.c_str()); nfail++; }
    }
  }
  printf("host builders under sanitizers: %d failures (%d impurity-block images, %d Jz sectors)\n", nfail, nib, njz);
  if (nib == 0 || njz == 0) nfail++;
  return nfail != 0;
}
