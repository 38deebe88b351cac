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

void rdm_flat_plan(const RdmFlatTables& t, int nblk, int cw, int target_wgs, RdmFlatPlan& p) {
  p = RdmFlatPlan();
  const int norb = t.norb, nbw = 1 << (t.ns - norb), imask = (1 << norb) - 1, nrow = 1 << norb;
  p.norb = norb;
  p.dim_el = t.dim_el;
  p.rowstart = t.rowstart;
  int bmax = 1;
  for (int c = 0; c < t.nclass; c++) bmax = std::max(bmax, t.bn[c]);
  const int nb = kRdmFlatStageElems / bmax;  // bath words up of a chunk: its tiles hold at most nb * bmax elements
  bool present[kRdmFlatClasses] = {false};
  for (int bd = 0; bd <= t.ns - norb; bd++) {
    const int32_t bdw0 = (int32_t)p.bdw.size();
    for (int b = 0; b < nbw; b++)
      if (popc((uint32_t)b) == bd) p.bdw.push_back(b);
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
  const int64_t total = (int64_t)wants.size() * t.dim_el * nblk;
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

std::string rdm_flat_plan_emulate(const RdmFlatPlan& p, int64_t ntri, int64_t nel, const double* v, int cw, double* tri) {
  const int norb = p.norb, nrow = 1 << norb;
  const int64_t stage_n = p.stage_max, acc_n = (int64_t)p.ept_max * kRdmFlatThreads;
  if (stage_n > kRdmFlatStageElems) return "a staged slab exceeds the staging area";
  std::vector<double> stage((size_t)stage_n * cw), acc((size_t)acc_n * cw), partial((size_t)p.partial_entries * cw, 0.0);
  std::vector<int64_t> loaded((size_t)stage_n, -1);
  std::vector<uint16_t> rel((size_t)p.rel_max);
  std::vector<char> written((size_t)p.partial_entries, 0);
  if ((int64_t)p.ent.size() != ntri) return "ent does not have ntri entries";
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
        if (o < 0 || o >= p.partial_entries) return "partial sum out of range";
        if (written[(size_t)o]) return "a partial sum is written twice";
        written[(size_t)o] = 1;
        for (int c = 0; c < cw; c++) partial[(size_t)o * cw + c] = acc[((size_t)k * kRdmFlatThreads + t) * cw + c];
      }
  }
  for (char c : written)
    if (!c) return "a partial sum is never written";
  std::fill(tri, tri + ntri * cw, 0.0);
  std::vector<char> done((size_t)ntri, 0);
  for (const RdmGroup& g : p.groups) {
    const int64_t E = g.e1 - g.e0;
    if (g.e0 < 0 || g.e1 > ntri || g.pbase + (int64_t)g.nwg * E > p.partial_entries) return "group out of range";
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

}  // namespace edigpu
