// host_rdm_flat.cpp -- host tables of the impurity reduced density matrix of superc / nonsu2 sectors (host_rdm_flat.hpp).
#include "host_rdm_flat.hpp"

#include <algorithm>

namespace edigpu {

static int popc(uint32_t x) {
  int c = 0;
  for (; x; x &= x - 1) c++;
  return c;
}

static int64_t binom(int n, int k) {
  if (k < 0 || k > n) return 0;
  int64_t r = 1;
  for (int i = 1; i <= k; i++) r = r * (n - k + i) / i;
  return r;
}

std::string rdm_flat_tables(const int32_t* map, int64_t n, int ns, int norb, int mode, int q, RdmFlatTables& t) {
  t = RdmFlatTables();
  if (norb < 1 || norb > kRdmFlatMaxOrb) return "norb must be 1 .. 4";
  if (ns < norb || ns > 15) return "ns out of range";
  if (mode != 1 && mode != 2) return "the sector is neither superc nor nonsu2";
  if (!map || n < 0) return "no sector map";
  t.ns = ns;
  t.norb = norb;
  t.mode = mode;
  t.q = q;
  rdm_rank_tables(norb, t.ranks);
  for (int pc = 0; pc <= 32; pc++) {
    const int nup = t.nup_row(pc);
    t.nup_of[pc] = (pc <= ns && nup >= 0 && nup <= ns) ? nup : -1;
  }
  const uint32_t nw = 1u << ns, wmask = nw - 1u;
  t.rowstart.assign((size_t)nw + 1, 0);
  for (uint32_t d = 0; d < nw; d++) t.rowstart[d + 1] = t.rowstart[d] + binom(ns, t.nup_of[popc(d)]);
  t.dim_el = t.rowstart[nw];
  if (t.dim_el != n) return "the sector map does not have the dimension of its sector";
  // every row is the ascending list of the up words of its particle number; the first row of a number gives its runs
  std::vector<std::vector<int32_t>> words((size_t)ns + 1);
  t.run_of.assign((size_t)ns + 1, std::vector<int32_t>());
  for (uint32_t d = 0; d < nw; d++) {
    const int64_t r0 = t.rowstart[d], len = t.rowstart[d + 1] - r0;
    if (len == 0) continue;
    const int nup = t.nup_of[popc(d)];
    for (int64_t i = 0; i < len; i++) {
      if (map[r0 + i] < 0 || ((uint32_t)map[r0 + i] >> ns) != d) return "a row of the sector map does not hold one down word";
      if (r0 + i > 0 && map[r0 + i] <= map[r0 + i - 1]) return "the sector map does not ascend";
    }
    std::vector<int32_t>& w = words[(size_t)nup];
    if (w.empty()) {
      w.resize((size_t)len);
      for (int64_t i = 0; i < len; i++) {
        w[(size_t)i] = (int32_t)((uint32_t)map[r0 + i] & wmask);
        if (popc((uint32_t)w[(size_t)i]) != nup) return "a row of the sector map holds a word of another particle number";
      }
      RdmRuns runs;
      const std::string why = rdm_runs(w.data(), len, norb, t.ranks, runs);
      if (!why.empty()) return why;
      std::vector<int32_t>& ro = t.run_of[(size_t)nup];
      ro.assign((size_t)1 << (ns - norb), -1);
      for (size_t j = 0; j < runs.k.size(); j++) ro[(size_t)((uint32_t)w[(size_t)runs.start[j]] >> norb)] = runs.start[j];
    } else {
      for (int64_t i = 0; i < len; i++)
        if ((int32_t)((uint32_t)map[r0 + i] & wmask) != w[(size_t)i]) return "two rows of one particle number differ";
    }
  }
  // blocks
  t.nclass = 2 * norb + 1;
  for (int c = 0; c < t.nclass; c++) {
    t.tri_off[c] = t.ntri;
    for (int idw = 0; idw < (1 << norb); idw++) {
      const int ku = t.ku_of(c, popc((uint32_t)idw));
      if (ku < 0 || ku > norb) continue;
      for (int r = 0; r < t.ranks.nk[ku]; r++) t.member[c][t.bn[c]++] = (uint8_t)(t.ranks.pat_of[ku][r] + (idw << norb));
    }
    t.ntri += rdm_tri_size(t.bn[c]);
  }
  for (int c = t.nclass; c <= kRdmFlatClasses; c++) t.tri_off[c] = t.ntri;
  return "";
}

void rdm_flat_place(const RdmFlatTables& t, const double* tri, int cw, double* dense) {
  const int64_t D = (int64_t)1 << (2 * t.norb);
  std::fill(dense, dense + D * D * cw, 0.0);
  for (int c = 0; c < t.nclass; c++) {
    const int n = t.bn[c];
    const double* e = tri + t.tri_off[c] * cw;
    for (int p = 0; p < n; p++) {
      const int64_t io = t.member[c][p];
      for (int q = p; q < n; q++, e += cw) {
        const int64_t jo = t.member[c][q];
        dense[(io * D + jo) * cw] = dense[(jo * D + io) * cw] = e[0];
        if (cw == 2) {
          dense[(io * D + jo) * 2 + 1] = e[1];
          dense[(jo * D + io) * 2 + 1] = p == q ? e[1] : -e[1];
        }
      }
    }
  }
}

double rdm_flat_trace(const RdmFlatTables& t, const double* tri, int cw) {
  double tr = 0.0;
  for (int c = 0; c < t.nclass; c++)
    for (int p = 0; p < t.bn[c]; p++) tr += tri[(t.tri_off[c] + rdm_tri_index(t.bn[c], p, p)) * cw];
  return tr;
}

// class of the tile (bath word up of popcount bu, bath word down of popcount bd), -1: the tile has no element
static int tile_class(const RdmFlatTables& t, int bu, int bd) {
  for (int kd = 0; kd <= t.norb; kd++) {
    const int nup = t.nup_of[kd + bd];
    if (nup < 0) continue;
    const int ku = nup - bu;
    if (ku < 0 || ku > t.norb) continue;
    return t.mode == 2 ? ku + kd : ku - kd + t.norb;
  }
  return -1;
}

void rdm_flat_host_reference(const RdmFlatTables& t, int nblk, const double* v, int cw, double* tri) {
  const int norb = t.norb, nbw = 1 << (t.ns - norb), imask = (1 << norb) - 1;
  double x[kRdmFlatMaxBlock * 2];
  for (int b = 0; b < nblk; b++)
    for (int bdw = 0; bdw < nbw; bdw++)
      for (int bup = 0; bup < nbw; bup++) {
        const int bu = popc((uint32_t)bup), bd = popc((uint32_t)bdw);
        const int c = tile_class(t, bu, bd);
        if (c < 0) continue;
        const int n = t.bn[c];
        for (int p = 0; p < n; p++) {
          const int idw = t.member[c][p] >> norb, iup = t.member[c][p] & imask, kd = popc((uint32_t)idw);
          const int nup = t.nup_of[kd + bd];
          const int64_t i = (int64_t)b * t.dim_el + t.rowstart[(size_t)((bdw << norb) + idw)] + t.run_of[(size_t)nup][(size_t)bup] +
                            t.ranks.rank_of[iup];
          const double s = (bu & 1) && (kd & 1) ? -1.0 : 1.0;
          for (int k = 0; k < cw; k++) x[p * cw + k] = s * v[i * cw + k];
        }
        double* e = tri + t.tri_off[c] * cw;
        for (int p = 0; p < n; p++)
          for (int q = p; q < n; q++, e += cw) {
            if (cw == 1) {
              e[0] += x[p] * x[q];
            } else {
              e[0] += x[2 * p] * x[2 * q] + x[2 * p + 1] * x[2 * q + 1];
              e[1] += x[2 * p + 1] * x[2 * q] - x[2 * p] * x[2 * q + 1];
            }
          }
      }
}

// rdm_flat_plan of the bath words down that `keep` names (null: all), on a vector whose element 0 is element `base` of the
// sector and whose blocks are `stride` elements apart.  The panels and the class groups are those of the whole sector
// whatever is kept, so every such list splits the packed entries alike and two of them can share their partial sums.
static void flat_plan_core(const RdmFlatTables& t, int nblk, int cw, int target_wgs, const std::vector<char>* keep, int64_t base,
                           int64_t stride, RdmFlatPlan& p) {
  p = RdmFlatPlan();
  const int norb = t.norb, nbw = 1 << (t.ns - norb), imask = (1 << norb) - 1, nrow = 1 << norb;
  p.norb = norb;
  p.dim_el = stride;
  p.rowstart = t.rowstart;
  for (int64_t& r : p.rowstart) r -= base;
  int bmax = 1;
  for (int c = 0; c < t.nclass; c++) bmax = std::max(bmax, t.bn[c]);
  const int nb = kRdmFlatStageElems / bmax;  // bath words up of a chunk: its tiles hold at most nb * bmax elements
  bool present[kRdmFlatClasses] = {false};
  for (int bd = 0; bd <= t.ns - norb; bd++) {
    const int32_t bdw0 = (int32_t)p.bdw.size();
    for (int b = 0; b < nbw; b++)
      if (popc((uint32_t)b) == bd && (!keep || (*keep)[(size_t)b])) p.bdw.push_back(b);
    const int32_t nbdw = (int32_t)p.bdw.size() - bdw0;
    for (int b0 = 0; b0 < nbw; b0 += nb) {
      const int b1 = std::min(nbw, b0 + nb);
      RdmFlatPanel P = RdmFlatPanel();
      P.bdw0 = bdw0;
      P.nbdw = nbdw;
      for (int kd = 0; kd <= norb; kd++) {
        const int nup = t.nup_of[kd + bd];
        if (nup < 0) continue;
        const std::vector<int32_t>& ro = t.run_of[(size_t)nup];
        if (ro.empty()) continue;
        int32_t lo = -1, hi = -1;
        for (int b = b0; b < b1; b++)
          if (ro[(size_t)b] >= 0) {
            if (lo < 0) lo = ro[(size_t)b];
            hi = ro[(size_t)b] + t.ranks.nk[nup - popc((uint32_t)b)];
          }
        if (lo < 0) continue;
        P.seg[kd] = lo;
        P.len[kd] = hi - lo;
      }
      for (int idw = 0; idw < nrow; idw++) {
        P.soff[idw] = P.total;
        P.total += P.len[popc((uint32_t)idw)];
      }
      std::vector<int> cls((size_t)(b1 - b0));
      for (int b = b0; b < b1; b++) cls[(size_t)(b - b0)] = tile_class(t, popc((uint32_t)b), bd);
      std::vector<int> tiles;
      for (int c = 0; c < t.nclass; c++) {
        P.kb[c] = (int32_t)tiles.size();
        for (int b = b0; b < b1; b++)
          if (cls[(size_t)(b - b0)] == c) tiles.push_back(b);
        if ((int32_t)tiles.size() > P.kb[c]) present[c] = true;
      }
      P.ntile = (int32_t)tiles.size();
      for (int c = t.nclass; c <= kRdmFlatClasses; c++) P.kb[c] = P.ntile;
      if (P.ntile == 0) continue;
      P.rel0 = (int32_t)p.rel.size();
      for (int kd = 0; kd <= norb; kd++) {
        const int nup = t.nup_of[kd + bd];
        for (int b : tiles) {
          const uint16_t par = (uint16_t)((popc((uint32_t)b) & 1) << 15);
          uint16_t r = kRdmFlatNoRun;
          if (nup >= 0 && !t.run_of[(size_t)nup].empty() && t.run_of[(size_t)nup][(size_t)b] >= 0)
            r = (uint16_t)(t.run_of[(size_t)nup][(size_t)b] - P.seg[kd]);
          p.rel.push_back((uint16_t)(r | par));
        }
      }
      p.rel_max = std::max(p.rel_max, (norb + 1) * P.ntile);
      p.stage_max = std::max(p.stage_max, (int)P.total);
      p.panels.push_back(P);
    }
  }
  // entries
  p.ent.assign((size_t)t.ntri, 0u);
  for (int c = 0; c < t.nclass; c++) {
    uint32_t* e = p.ent.data() + t.tri_off[c];
    for (int a = 0; a < t.bn[c]; a++)
      for (int b = a; b < t.bn[c]; b++) {
        const uint32_t ia = t.member[c][a] >> norb, ib = t.member[c][b] >> norb;
        const uint32_t ra = t.ranks.rank_of[t.member[c][a] & imask], rb = t.ranks.rank_of[t.member[c][b] & imask];
        const uint32_t ka = (uint32_t)popc(ia), kb = (uint32_t)popc(ib);
        *e++ = (uint32_t)c | ia << 4 | ra << 8 | ib << 11 | rb << 15 | ((ka + kb) & 1u) << 18 | ka << 19 | kb << 22;
      }
  }
  // groups: consecutive classes of the sector while their accumulators fit
  struct Want {
    int c0, c1;
  };
  std::vector<Want> wants;
  for (int c = 0; c < t.nclass;) {
    if (!present[c]) {
      c++;
      continue;
    }
    int c1 = c;
    for (int d = c + 1; d < t.nclass; d++)
      if (present[d] && (t.tri_off[d + 1] - t.tri_off[c]) * cw * 8 <= kRdmFlatAccBytes) c1 = d;
      else if (present[d]) break;
    wants.push_back({c, c1});
    c = c1 + 1;
  }
  const int64_t total = (int64_t)wants.size() * stride * nblk;
  for (const Want& w : wants) {
    RdmGroup g;
    g.e0 = (int32_t)t.tri_off[w.c0];
    g.e1 = (int32_t)t.tri_off[w.c1 + 1];
    g.nwg = 0;
    g.pad = 0;
    g.pbase = p.partial_entries;
    const int32_t E = g.e1 - g.e0;
    const int64_t per = std::max<int64_t>({total / std::max(target_wgs, 1), (int64_t)4096, (int64_t)8 * E});
    for (size_t ip = 0; ip < p.panels.size(); ip++) {
      const RdmFlatPanel& P = p.panels[ip];
      if (P.kb[w.c1 + 1] == P.kb[w.c0]) continue;  // no tile of these classes in the panel
      const int64_t nj = (int64_t)P.nbdw * nblk;
      const int64_t step = std::max<int64_t>(1, per / std::max<int64_t>(P.total, 1));
      for (int64_t j0 = 0; j0 < nj; j0 += step) {
        RdmFlatWork k;
        k.panel = (int32_t)ip;
        k.j0 = (int32_t)j0;
        k.j1 = (int32_t)std::min<int64_t>(j0 + step, nj);
        k.e0 = g.e0;
        k.e1 = g.e1;
        k.pad = 0;
        k.pofs = g.pbase + (int64_t)g.nwg * E;
        p.work.push_back(k);
        g.nwg++;
      }
    }
    if (g.nwg == 0) continue;
    p.partial_entries += (int64_t)g.nwg * E;
    p.ept_max = std::max(p.ept_max, (E + kRdmFlatThreads - 1) / kRdmFlatThreads);
    p.groups.push_back(g);
  }
}

void rdm_flat_plan(const RdmFlatTables& t, int nblk, int cw, int target_wgs, RdmFlatPlan& p) {
  flat_plan_core(t, nblk, cw, target_wgs, nullptr, 0, t.dim_el, p);
}

// the tiles kernel on the work list of p: v holds nel elements in blocks p.dim_el apart; partial / written: the buffer of
// partial sums (partial_entries of them) and which of them a workgroup has written
static std::string emulate_tiles(const RdmFlatPlan& p, int64_t ntri, int64_t nel, const double* v, int cw, int64_t partial_entries,
                                 std::vector<double>& partial, std::vector<char>& written) {
  const int norb = p.norb, nrow = 1 << norb;
  const int64_t stage_n = p.stage_max, acc_n = (int64_t)p.ept_max * kRdmFlatThreads;
  if (stage_n > kRdmFlatStageElems) return "a staged slab exceeds the staging area";
  std::vector<double> stage((size_t)stage_n * cw), acc((size_t)acc_n * cw);
  std::vector<int64_t> loaded((size_t)stage_n, -1);
  std::vector<uint16_t> rel((size_t)p.rel_max);
  if ((int64_t)p.ent.size() != ntri) return "ent does not have ntri entries";
  if (!p.work.empty() && !v) return "a work list without a vector";
  int64_t slab = 0;
  for (const RdmFlatWork& w : p.work) {
    if (w.panel < 0 || w.panel >= (int64_t)p.panels.size()) return "panel out of range";
    const RdmFlatPanel& P = p.panels[(size_t)w.panel];
    const int nrel = (norb + 1) * P.ntile;
    if (nrel > p.rel_max || P.rel0 < 0 || P.rel0 + nrel > (int64_t)p.rel.size()) return "rel list out of range";
    for (int i = 0; i < nrel; i++) rel[(size_t)i] = p.rel[(size_t)(P.rel0 + i)];
    if (w.e0 < 0 || w.e1 > ntri || w.e1 < w.e0 || w.e1 - w.e0 > acc_n) return "entries out of range";
    if (P.total > stage_n) return "slab larger than the staging area";
    if (w.j0 < 0 || P.nbdw < 1) return "slab range out of range";
    std::fill(acc.begin(), acc.end(), 0.0);
    for (int32_t j = w.j0; j < w.j1; j++, slab++) {
      const int32_t b = j / P.nbdw, jj = j - b * P.nbdw;
      if (P.bdw0 + jj >= (int64_t)p.bdw.size()) return "bath word list out of range";
      const int64_t row0 = (int64_t)p.bdw[(size_t)(P.bdw0 + jj)] << norb;
      for (int idw = 0; idw < nrow; idw++) {
        const int kd = popc((uint32_t)idw), L = P.len[kd];
        if (L == 0) continue;
        if (row0 + idw + 1 >= (int64_t)p.rowstart.size()) return "row out of range";
        const int64_t r0 = p.rowstart[(size_t)(row0 + idw)], r1 = p.rowstart[(size_t)(row0 + idw + 1)];
        if (P.seg[kd] < 0 || L < 0 || P.seg[kd] + L > r1 - r0) return "segment outside its row";
        if (r0 < 0 || r1 > p.dim_el) return "row outside its block";
        const int64_t g0 = (int64_t)b * p.dim_el + r0 + P.seg[kd];
        if (g0 < 0 || g0 + L > nel) return "vector read out of range";
        if (P.soff[idw] < 0 || P.soff[idw] + L > stage_n) return "staged write out of range";
        for (int i = 0; i < L; i++) {
          for (int c = 0; c < cw; c++) stage[(size_t)(P.soff[idw] + i) * cw + c] = v[(g0 + i) * cw + c];
          loaded[(size_t)(P.soff[idw] + i)] = slab;
        }
      }
      for (int t = 0; t < kRdmFlatThreads; t++)
        for (int e = w.e0 + t, k = 0; e < w.e1; e += kRdmFlatThreads, k++) {
          const uint32_t d = p.ent[(size_t)e];
          const int c = d & 15u;
          if (c > kRdmFlatClasses - 1) return "class out of range";
          const int offp = P.soff[(d >> 4) & 15u] + (int)((d >> 8) & 7u), offq = P.soff[(d >> 11) & 15u] + (int)((d >> 15) & 7u);
          const int relp = (int)((d >> 19) & 7u) * P.ntile, relq = (int)((d >> 22) & 7u) * P.ntile;
          const uint32_t par = (d >> 18) & 1u;
          double* a = &acc[((size_t)k * kRdmFlatThreads + t) * cw];
          for (int i = P.kb[c]; i < P.kb[c + 1]; i++) {
            if (i < 0 || relp + i >= nrel || relq + i >= nrel) return "run index out of range";
            const uint16_t rp = rel[(size_t)(relp + i)], rq = rel[(size_t)(relq + i)];
            if ((rp & 0x7fff) == kRdmFlatNoRun || (rq & 0x7fff) == kRdmFlatNoRun) return "a tile has no run in a row of its class";
            const int ip = offp + (rp & 0x7fff), iq = offq + (rq & 0x7fff);
            if (ip >= stage_n || iq >= stage_n) return "staged read out of range";
            if (loaded[(size_t)ip] != slab || loaded[(size_t)iq] != slab) return "staged read of an element not loaded";
            const double sg = (par & (uint32_t)(rp >> 15)) ? -1.0 : 1.0;
            const double* x = &stage[(size_t)ip * cw];
            const double* y = &stage[(size_t)iq * cw];
            if (cw == 1) {
              a[0] += sg * (x[0] * y[0]);
            } else {
              a[0] += sg * (x[0] * y[0] + x[1] * y[1]);
              a[1] += sg * (x[1] * y[0] - x[0] * y[1]);
            }
          }
        }
    }
    for (int t = 0; t < kRdmFlatThreads; t++)
      for (int e = w.e0 + t, k = 0; e < w.e1; e += kRdmFlatThreads, k++) {
        const int64_t o = w.pofs + (e - w.e0);
        if (o < 0 || o >= partial_entries) return "partial sum out of range";
        if (written[(size_t)o]) return "a partial sum is written twice";
        written[(size_t)o] = 1;
        for (int c = 0; c < cw; c++) partial[(size_t)o * cw + c] = acc[((size_t)k * kRdmFlatThreads + t) * cw + c];
      }
  }
  return "";
}

// the final kernel over the groups: tri[ntri] = the workgroups' partial sums in workgroup order, 0 where no group writes
static std::string emulate_final(const std::vector<RdmGroup>& groups, int64_t ntri, int cw, int64_t partial_entries,
                                 const std::vector<double>& partial, const std::vector<char>& written, double* tri) {
  for (char c : written)
    if (!c) return "a partial sum is never written";
  std::fill(tri, tri + ntri * cw, 0.0);
  std::vector<char> done((size_t)ntri, 0);
  for (const RdmGroup& g : groups) {
    const int64_t E = g.e1 - g.e0;
    if (g.e0 < 0 || g.e1 > ntri || g.pbase + (int64_t)g.nwg * E > partial_entries) return "group out of range";
    for (int64_t e = 0; e < E; e++) {
      if (done[(size_t)(g.e0 + e)]) return "two groups write one entry";
      done[(size_t)(g.e0 + e)] = 1;
      for (int c = 0; c < cw; c++) {
        double s = 0.0;
        for (int w = 0; w < g.nwg; w++) s += partial[(size_t)(g.pbase + (int64_t)w * E + e) * cw + c];
        tri[(g.e0 + e) * cw + c] = s;
      }
    }
  }
  return "";
}

std::string rdm_flat_plan_emulate(const RdmFlatPlan& p, int64_t ntri, int64_t nel, const double* v, int cw, double* tri) {
  std::vector<double> partial((size_t)p.partial_entries * cw, 0.0);
  std::vector<char> written((size_t)p.partial_entries, 0);
  const std::string why = emulate_tiles(p, ntri, nel, v, cw, p.partial_entries, partial, written);
  return why.empty() ? emulate_final(p.groups, ntri, cw, p.partial_entries, partial, written, tri) : why;
}

// the non-empty slabs of the sector in ascending order: [start[j], start[j + 1]) is the slab of bath word down bdw[j]
struct FlatSlabs {
  std::vector<int64_t> start;
  std::vector<int32_t> bdw;
};
static void flat_slabs(const RdmFlatTables& t, FlatSlabs& s) {
  const int nbw = 1 << (t.ns - t.norb);
  for (int b = 0; b < nbw; b++) {
    const int64_t s0 = t.rowstart[(size_t)b << t.norb], s1 = t.rowstart[(size_t)(b + 1) << t.norb];
    if (s1 == s0) continue;
    s.start.push_back(s0);
    s.bdw.push_back(b);
  }
  s.start.push_back(t.dim_el);
}

// elements from `first` up to the first slab start in [first, first + count) (count when there is none); *slab = that slab
static int64_t flat_head(const FlatSlabs& s, int64_t first, int64_t count, size_t* slab) {
  const size_t j = (size_t)(std::lower_bound(s.start.begin(), s.start.end() - 1, first) - s.start.begin());
  if (slab) *slab = j;
  if (j >= s.bdw.size() || s.start[j] >= first + count) return count;
  return s.start[j] - first;
}

std::string rdm_flat_shard_plan(const RdmFlatTables& t, int nblk, int cw, int target_wgs, int world, int64_t first,
                                int64_t count, RdmFlatShardPlan& p) {
  p = RdmFlatShardPlan();
  if (world < 1 || first < 0 || count < 0) return "bad range";
  if (t.rowstart.empty() || t.rowstart.back() != t.dim_el) return "no tables of the sector";
  const int64_t dim = t.dim_el;
  p.world = world;
  p.q = (dim + world - 1) / world;
  p.first = std::min(first, dim);
  p.count = std::max<int64_t>(0, std::min(count, dim - p.first));
  p.rank = -1;
  if (p.count > 0) {
    if (p.first % p.q != 0 || p.count != std::min(p.q, dim - p.first)) return "the elements are not a rank's range of edigpu_shard_plan";
    p.rank = (int)(p.first / p.q);
  }
  FlatSlabs sl;
  flat_slabs(t, sl);
  int64_t longest = 0;
  for (size_t j = 0; j < sl.bdw.size(); j++) longest = std::max(longest, sl.start[j + 1] - sl.start[j]);
  p.heads.assign((size_t)world, 0);
  for (int r = 0; r < world; r++) {
    const int64_t f = std::min<int64_t>((int64_t)r * p.q, dim), c = std::max<int64_t>(0, std::min(p.q, dim - f));
    p.heads[(size_t)r] = flat_head(sl, f, c, nullptr);
    p.H = std::max(p.H, p.heads[(size_t)r]);
  }
  if (p.H > 0 && p.H >= longest) return "a halo as long as a slab";
  // the halo this rank sends: its head, then zeros
  const int64_t head = p.rank >= 0 ? p.heads[(size_t)p.rank] : 0;
  if (head > 0) p.pack.push_back({1, 0, 0, 0, head});
  if (p.H > head) p.pack.push_back({0, 0, 0, head, p.H - head});
  // interior slabs and the tail slab
  const int nbw = 1 << (t.ns - t.norb);
  std::vector<char> keep((size_t)nbw, 0);
  for (int b = 0; b < nbw; b++)  // empty slabs stay in the lists (no panel names them): a world of one IS rdm_flat_plan
    keep[(size_t)b] = t.rowstart[(size_t)b << t.norb] == t.rowstart[(size_t)(b + 1) << t.norb];
  const std::vector<char> empty = keep;
  size_t j = 0;
  if (p.count > 0) flat_head(sl, p.first, p.count, &j);
  for (; p.count > 0 && j < sl.bdw.size() && sl.start[j] < p.first + p.count; j++) {
    if (sl.start[j + 1] <= p.first + p.count) {
      keep[(size_t)sl.bdw[j]] = 1;
      p.nslab_in++;
      continue;
    }
    p.tail_start = sl.start[j] - p.first;
    p.tail_own = p.count - p.tail_start;
    p.tail_len = sl.start[j + 1] - sl.start[j];
    p.tail_bdw = sl.bdw[j];
  }
  flat_plan_core(t, nblk, cw, target_wgs, &keep, p.first, p.count, p.in);
  if (p.tail_len > 0) {
    p.fill.push_back({1, 0, p.tail_start, 0, p.tail_own});
    int64_t n = p.tail_own;
    for (int r = p.rank + 1; r < world && n < p.tail_len; r++) {
      const int64_t take = std::min(p.heads[(size_t)r], p.tail_len - n);
      if (take <= 0) continue;
      p.fill.push_back({2, r, 0, n, take});
      n += take;
    }
    if (n != p.tail_len) return "the following ranks' heads do not complete the tail slab";
    keep = empty;
    keep[(size_t)p.tail_bdw] = 1;
    flat_plan_core(t, nblk, cw, target_wgs, &keep, p.first + p.tail_start, p.tail_len, p.slab);
  }
  // one buffer of partial sums: per group the workgroups of `in`, then those of `slab` (no slab: `in` as it stands)
  for (const RdmFlatPlan* q : {&p.in, &p.slab})
    for (const RdmGroup& g : q->groups) {
      auto it = std::find_if(p.groups.begin(), p.groups.end(), [&](const RdmGroup& m) { return m.e0 == g.e0; });
      if (it == p.groups.end()) {
        p.groups.push_back(g);
      } else {
        if (it->e1 != g.e1) return "the two work lists split the classes differently";
        it->nwg += g.nwg;
      }
    }
  for (RdmGroup& g : p.groups) {
    g.pbase = p.partial_entries;
    p.partial_entries += (int64_t)g.nwg * (g.e1 - g.e0);
  }
  std::vector<int32_t> next(p.groups.size(), 0);
  for (RdmFlatPlan* q : {&p.in, &p.slab})
    for (RdmFlatWork& w : q->work) {
      const size_t g = (size_t)(std::find_if(p.groups.begin(), p.groups.end(), [&](const RdmGroup& m) { return m.e0 == w.e0; }) -
                                p.groups.begin());
      if (g >= p.groups.size() || p.groups[g].e1 != w.e1) return "a workgroup without a group";
      w.pofs = p.groups[g].pbase + (int64_t)next[g]++ * (w.e1 - w.e0);
    }
  return "";
}

std::string rdm_flat_segs_emulate(const RdmFlatShardPlan& p, const std::vector<RdmFlatSeg>& segs, int64_t dlen, int nblk, int cw,
                                  const double* v, const double* halos, double* dst) {
  const int64_t rank_stride = (int64_t)nblk * p.H;  // elements of one vector's halo
  std::vector<char> written((size_t)dlen, 0);
  for (int b = 0; b < nblk; b++) {
    std::fill(written.begin(), written.end(), 0);
    for (const RdmFlatSeg& s : segs) {
      if (s.len <= 0 || s.dst < 0 || s.dst + s.len > dlen) return "segment outside its destination";
      if (s.sel == 1) {
        if (s.src < 0 || s.src + s.len > p.count || !v) return "shard element out of range";
      } else if (s.sel == 2) {
        if (s.rank < 0 || s.rank >= p.world || !halos) return "halo rank out of range";
        if (s.src < 0 || s.src + s.len > p.heads[(size_t)s.rank]) return "halo element past its rank's head";
      } else if (s.sel != 0) {
        return "unknown segment source";
      }
      for (int64_t i = 0; i < s.len; i++) {
        if (written[(size_t)(s.dst + i)]) return "a destination element is written twice";
        written[(size_t)(s.dst + i)] = 1;
        for (int c = 0; c < cw; c++) {
          double x = 0.0;
          if (s.sel == 1) x = v[((int64_t)b * p.count + s.src + i) * cw + c];
          else if (s.sel == 2) x = halos[(s.rank * rank_stride + (int64_t)b * p.H + s.src + i) * cw + c];
          dst[((int64_t)b * dlen + s.dst + i) * cw + c] = x;
        }
      }
    }
    for (char c : written)
      if (!c) return "a destination element is never written";
  }
  return "";
}

std::string rdm_flat_shard_emulate(const RdmFlatShardPlan& p, int64_t ntri, int nblk, const double* v_shard, const double* slab,
                                   int cw, double* tri) {
  std::vector<double> partial((size_t)p.partial_entries * cw, 0.0);
  std::vector<char> written((size_t)p.partial_entries, 0);
  std::string why = emulate_tiles(p.in, ntri, p.count * nblk, v_shard, cw, p.partial_entries, partial, written);
  if (why.empty() && p.tail_len > 0) why = emulate_tiles(p.slab, ntri, p.tail_len * nblk, slab, cw, p.partial_entries, partial, written);
  return why.empty() ? emulate_final(p.groups, ntri, cw, p.partial_entries, partial, written, tri) : why;
}

std::string rdm_flat_world_emulate(const RdmFlatTables& t, int nblk, int cw, int target_wgs, int world, const double* v,
                                   double* tri, int64_t* H_out) {
  if (world < 1) return "bad world";
  const int64_t dim = t.dim_el, q = (dim + world - 1) / world;
  std::vector<RdmFlatShardPlan> plans((size_t)world);
  for (int r = 0; r < world; r++) {
    const std::string why = rdm_flat_shard_plan(t, nblk, cw, target_wgs, world, (int64_t)r * q, q, plans[(size_t)r]);
    if (!why.empty()) return why;
    if (plans[(size_t)r].H != plans[0].H || plans[(size_t)r].heads != plans[0].heads) return "the ranks disagree on the heads";
  }
  const int64_t H = plans[0].H;
  if (H_out) *H_out = H;
  // one owner per slab, every element read once
  FlatSlabs sl;
  flat_slabs(t, sl);
  std::vector<int> owners(sl.bdw.size(), 0);
  std::vector<int> reads((size_t)dim, 0);
  auto slab_of = [&](int32_t bdw) { return (size_t)(std::find(sl.bdw.begin(), sl.bdw.end(), bdw) - sl.bdw.begin()); };
  for (int r = 0; r < world; r++) {
    const RdmFlatShardPlan& p = plans[(size_t)r];
    int64_t walked = 0;
    for (int32_t b : p.in.bdw) {
      if (t.rowstart[(size_t)b << t.norb] == t.rowstart[(size_t)(b + 1) << t.norb]) continue;
      const size_t j = slab_of(b);
      if (j >= sl.bdw.size()) return "an interior slab that is no slab of the sector";
      if (sl.start[j] < p.first || sl.start[j + 1] > p.first + p.count) return "an interior slab outside the range";
      owners[j]++;
      walked++;
      for (int64_t i = sl.start[j]; i < sl.start[j + 1]; i++) reads[(size_t)i]++;
    }
    if (walked != p.nslab_in) return "the bath word lists do not hold the interior slabs";
    if (p.tail_len > 0) {
      const size_t j = slab_of(p.tail_bdw);
      if (j >= sl.bdw.size() || sl.start[j] != p.first + p.tail_start || sl.start[j + 1] - sl.start[j] != p.tail_len)
        return "the tail slab is no slab of the sector";
      owners[j]++;
      int64_t want = sl.start[j];
      for (const RdmFlatSeg& s : p.fill) {
        const int64_t g0 = s.sel == 1 ? p.first + s.src : s.sel == 2 ? std::min<int64_t>((int64_t)s.rank * q, dim) + s.src : -1;
        if (g0 != want) return "the tail slab is not filled in order";
        for (int64_t i = 0; i < s.len; i++) reads[(size_t)(g0 + i)]++;
        want += s.len;
      }
      if (want != sl.start[j + 1]) return "the tail slab is not filled to its end";
    }
  }
  for (int o : owners)
    if (o != 1) return "a slab without exactly one owner";
  for (int n : reads)
    if (n != 1) return "an element that is not read exactly once";
  // pack, all-gather
  std::vector<std::vector<double>> shards((size_t)world);
  std::vector<double> halos((size_t)(world * nblk * H * cw), 0.0);
  for (int r = 0; r < world; r++) {
    const RdmFlatShardPlan& p = plans[(size_t)r];
    std::vector<double>& s = shards[(size_t)r];
    s.resize((size_t)(p.count * nblk * cw));
    for (int b = 0; b < nblk; b++)
      for (int64_t i = 0; i < p.count * cw; i++) s[(size_t)(b * p.count * cw + i)] = v[((int64_t)b * dim + p.first) * cw + i];
    if (H > 0) {
      const std::string why = rdm_flat_segs_emulate(p, p.pack, H, nblk, cw, p.count > 0 ? s.data() : nullptr, nullptr,
                                                    halos.data() + (size_t)r * nblk * H * cw);
      if (!why.empty()) return why;
    }
  }
  std::fill(tri, tri + t.ntri * cw, 0.0);
  std::vector<double> mine((size_t)t.ntri * cw);
  for (int r = 0; r < world; r++) {
    const RdmFlatShardPlan& p = plans[(size_t)r];
    std::vector<double> slab((size_t)(p.tail_len * nblk * cw));
    if (p.tail_len > 0) {
      const std::string why = rdm_flat_segs_emulate(p, p.fill, p.tail_len, nblk, cw, shards[(size_t)r].data(),
                                                    H > 0 ? halos.data() : nullptr, slab.data());
      if (!why.empty()) return why;
    }
    const std::string why = rdm_flat_shard_emulate(p, t.ntri, nblk, p.count > 0 ? shards[(size_t)r].data() : nullptr,
                                                   p.tail_len > 0 ? slab.data() : nullptr, cw, mine.data());
    if (!why.empty()) return why;
    for (size_t i = 0; i < mine.size(); i++) tri[i] += mine[i];
  }
  return "";
}

}  // namespace edigpu
