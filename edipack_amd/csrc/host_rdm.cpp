// host_rdm.cpp -- host tables of the impurity reduced density matrix (host_rdm.hpp).
#include "host_rdm.hpp"

#include <algorithm>

namespace edigpu {

static int popcount5(uint32_t x) {
  int c = 0;
  for (; x; x &= x - 1) c++;
  return c;
}

void rdm_rank_tables(int norb, RdmRanks& r) {
  r = RdmRanks();
  r.norb = norb;
  for (int pat = 0; pat < (1 << norb); pat++) {
    const int k = popcount5((uint32_t)pat);
    r.rank_of[pat] = (uint8_t)r.nk[k];
    r.pat_of[k][r.nk[k]++] = (uint8_t)pat;
  }
}

std::string rdm_runs(const int32_t* map, int64_t n, int norb, const RdmRanks& rk, RdmRuns& out) {
  out.start.clear();
  out.k.clear();
  const uint32_t mask = (1u << norb) - 1u;
  int64_t i = 0;
  while (i < n) {
    const uint32_t bath = (uint32_t)map[i] >> norb;
    const int k = popcount5((uint32_t)map[i] & mask);
    int64_t j = i;
    for (; j < n && ((uint32_t)map[j] >> norb) == bath; j++) {
      if (j > 0 && map[j] <= map[j - 1]) return "the sector map does not ascend";
      const uint32_t pat = (uint32_t)map[j] & mask;
      if (j - i >= rk.nk[k] || rk.pat_of[k][j - i] != pat) return "a run of the sector map is not the ascending list of its impurity patterns";
    }
    if (j - i != rk.nk[k]) return "a run of the sector map misses impurity patterns";
    if (j < n && map[j] <= map[j - 1]) return "the sector map does not ascend";
    out.start.push_back((int32_t)i);
    out.k.push_back((uint8_t)k);
    i = j;
  }
  out.start.push_back((int32_t)n);
  return "";
}

void rdm_layout(const RdmRanks& rk, RdmLayout& l) {
  l = RdmLayout();
  l.norb = rk.norb;
  for (int kd = 0; kd <= rk.norb; kd++)
    for (int ku = 0; ku <= rk.norb; ku++) {
      l.tri_off[ku][kd] = l.ntri;
      l.ntri += rdm_tri_size(rk.nk[ku] * rk.nk[kd]);
    }
}

void rdm_place(const RdmRanks& rk, const RdmLayout& l, const double* tri, int cw, double* dense) {
  const int norb = rk.norb;
  const int64_t D = (int64_t)1 << (2 * norb);
  std::fill(dense, dense + D * D * cw, 0.0);
  for (int kd = 0; kd <= norb; kd++)
    for (int ku = 0; ku <= norb; ku++) {
      const int lu = rk.nk[ku], n = lu * rk.nk[kd];
      const double* t = tri + l.tri_off[ku][kd] * cw;
      for (int p = 0; p < n; p++) {
        const int64_t io = rk.pat_of[ku][p % lu] + ((int64_t)rk.pat_of[kd][p / lu] << norb);
        for (int q = p; q < n; q++, t += cw) {
          const int64_t jo = rk.pat_of[ku][q % lu] + ((int64_t)rk.pat_of[kd][q / lu] << norb);
          dense[(io * D + jo) * cw] = dense[(jo * D + io) * cw] = t[0];
          if (cw == 2) {
            dense[(io * D + jo) * 2 + 1] = t[1];
            dense[(jo * D + io) * 2 + 1] = p == q ? t[1] : -t[1];
          }
        }
      }
    }
}

void rdm_host_reference(const RdmRanks& rk, const RdmLayout& l, const RdmRuns& up, const RdmRuns& dw, int64_t dim_up,
                        int64_t dim_dw, int nblk, const double* v, int cw, double* tri) {
  double x[kRdmMaxRun * kRdmMaxRun * 2];
  for (int b = 0; b < nblk; b++)
    for (size_t jd = 0; jd < dw.k.size(); jd++)
      for (size_t ju = 0; ju < up.k.size(); ju++) {
        const int ku = up.k[ju], kd = dw.k[jd], lu = rk.nk[ku], ld = rk.nk[kd], n = lu * ld;
        for (int rd = 0; rd < ld; rd++)
          for (int ru = 0; ru < lu; ru++) {
            const int64_t i = ((int64_t)b * dim_dw + dw.start[jd] + rd) * dim_up + up.start[ju] + ru;
            for (int c = 0; c < cw; c++) x[(ru + lu * rd) * cw + c] = v[i * cw + c];
          }
        double* t = tri + l.tri_off[ku][kd] * cw;
        for (int p = 0; p < n; p++)
          for (int q = p; q < n; q++, t += cw) {
            if (cw == 1) {
              t[0] += x[p] * x[q];
            } else {
              t[0] += x[2 * p] * x[2 * q] + x[2 * p + 1] * x[2 * q + 1];
              t[1] += x[2 * p + 1] * x[2 * q] - x[2 * p] * x[2 * q + 1];
            }
          }
      }
}

void rdm_plan(const RdmRanks& rk, const RdmLayout& l, const RdmRuns& up, const RdmRuns& dw, int64_t dim_up, int64_t dim_dw,
              int nblk, int cw, int target_wgs, RdmPlan& p) {
  (void)dim_dw;
  p = RdmPlan();
  const int norb = rk.norb;
  const int chmax = kRdmStageElems / rk.nk[norb / 2];
  p.stride = chmax | 1;
  // down runs by class
  int32_t row_off[kRdmMaxOrb + 2] = {0};
  for (int kd = 0; kd <= norb; kd++) {
    row_off[kd] = (int32_t)p.rows.size();
    for (size_t j = 0; j < dw.k.size(); j++)
      if (dw.k[j] == kd) p.rows.push_back(dw.start[j]);
  }
  row_off[norb + 1] = (int32_t)p.rows.size();
  // chunks of columns, ending on run boundaries, and their runs by class
  struct Chunk {
    int32_t c0, clen, rel0, kb[kRdmMaxOrb + 2];
  };
  std::vector<Chunk> chunks;
  bool ku_present[kRdmMaxOrb + 1] = {false};
  for (size_t r0 = 0; r0 < up.k.size();) {
    size_t r1 = r0 + 1;
    while (r1 < up.k.size() && up.start[r1 + 1] - up.start[r0] <= chmax) r1++;
    Chunk c;
    c.c0 = up.start[r0];
    c.clen = up.start[r1] - up.start[r0];
    c.rel0 = (int32_t)p.rel.size();
    for (int ku = 0; ku <= norb; ku++) {
      c.kb[ku] = (int32_t)p.rel.size() - c.rel0;
      for (size_t r = r0; r < r1; r++)
        if (up.k[r] == ku) {
          p.rel.push_back((uint16_t)(up.start[r] - c.c0));
          ku_present[ku] = true;
        }
    }
    for (int ku = norb + 1; ku < kRdmMaxOrb + 2; ku++) c.kb[ku] = (int32_t)p.rel.size() - c.rel0;
    p.rel_max = std::max(p.rel_max, c.kb[norb + 1]);
    chunks.push_back(c);
    r0 = r1;
  }
  // entries
  p.ent.assign((size_t)l.ntri, 0u);
  for (int kd = 0; kd <= norb; kd++)
    for (int ku = 0; ku <= norb; ku++) {
      const int lu = rk.nk[ku], n = lu * rk.nk[kd];
      uint32_t* e = p.ent.data() + l.tri_off[ku][kd];
      for (int a = 0; a < n; a++)
        for (int b = a; b < n; b++)
          *e++ = (uint32_t)ku | (uint32_t)(a % lu) << 4 | (uint32_t)(a / lu) << 8 | (uint32_t)(b % lu) << 12 | (uint32_t)(b / lu) << 16;
    }
  // groups: a down class with the up classes of the sector, one by one where the accumulators would not fit
  struct Want {
    int kd, ku0, ku1;
  };
  std::vector<Want> wants;
  int64_t total = 0;
  for (int kd = 0; kd <= norb; kd++) {
    if (row_off[kd + 1] == row_off[kd]) continue;
    int ku0 = 0, ku1 = norb;
    while (ku0 <= norb && !ku_present[ku0]) ku0++;
    while (ku1 >= 0 && !ku_present[ku1]) ku1--;
    if (ku0 > ku1) continue;
    const int64_t e0 = l.tri_off[ku0][kd], e1 = l.tri_off[ku1][kd] + rdm_tri_size(rk.nk[ku1] * rk.nk[kd]);
    const int64_t rows = (int64_t)(row_off[kd + 1] - row_off[kd]) * nblk * rk.nk[kd];
    if ((e1 - e0) * cw * 8 > kRdmAccBytes) {
      for (int ku = ku0; ku <= ku1; ku++)
        if (ku_present[ku]) {
          wants.push_back({kd, ku, ku});
          total += rows * dim_up;
        }
    } else {
      wants.push_back({kd, ku0, ku1});
      total += rows * dim_up;
    }
  }
  for (const Want& w : wants) {
    RdmGroup g;
    g.e0 = (int32_t)l.tri_off[w.ku0][w.kd];
    g.e1 = (int32_t)(l.tri_off[w.ku1][w.kd] + rdm_tri_size(rk.nk[w.ku1] * rk.nk[w.kd]));
    g.nwg = 0;
    g.pad = 0;
    g.pbase = p.partial_entries;
    const int32_t E = g.e1 - g.e0, ld = rk.nk[w.kd];
    const int32_t nruns = row_off[w.kd + 1] - row_off[w.kd];
    const int64_t per = std::max<int64_t>({total / std::max(target_wgs, 1), (int64_t)16384, (int64_t)8 * E});
    for (const Chunk& c : chunks) {
      if (c.kb[w.ku1 + 1] == c.kb[w.ku0]) continue;  // no run of these classes in the chunk
      const int64_t step = std::max<int64_t>(1, per / ((int64_t)ld * c.clen));
      for (int64_t j0 = 0; j0 < (int64_t)nruns * nblk; j0 += step) {
        RdmWork k;
        k.row_list = row_off[w.kd];
        k.nruns = nruns;
        k.j0 = (int32_t)j0;
        k.j1 = (int32_t)std::min<int64_t>(j0 + step, (int64_t)nruns * nblk);
        k.ld = ld;
        k.c0 = c.c0;
        k.clen = c.clen;
        k.rel0 = c.rel0;
        k.e0 = g.e0;
        k.e1 = g.e1;
        std::copy(c.kb, c.kb + kRdmMaxOrb + 2, k.kb);
        k.pad = 0;
        k.pofs = g.pbase + (int64_t)g.nwg * E;
        p.work.push_back(k);
        g.nwg++;
      }
    }
    if (g.nwg == 0) continue;
    p.partial_entries += (int64_t)g.nwg * E;
    p.ld_max = std::max(p.ld_max, (int)ld);
    p.ept_max = std::max(p.ept_max, (E + kRdmThreads - 1) / kRdmThreads);
    p.groups.push_back(g);
  }
}

// rdm_tiles_kernel over the work list of p: the workgroups' sums into partial (written: one flag per entry)
static std::string emulate_tiles(const RdmPlan& p, int64_t ntri, int64_t nel, int64_t dim_up, int64_t dim_dw, const double* v,
                                 int cw, std::vector<double>& partial, std::vector<char>& written) {
  const int64_t stage_n = (int64_t)p.ld_max * p.stride, acc_n = (int64_t)p.ept_max * kRdmThreads;
  const int64_t partial_entries = (int64_t)written.size();
  std::vector<double> stage((size_t)stage_n * cw), acc((size_t)acc_n * cw);
  std::vector<uint16_t> rel((size_t)p.rel_max);
  if ((int64_t)p.ent.size() != ntri) return "ent does not have ntri entries";
  for (const RdmWork& w : p.work) {
    const int nrel = w.kb[kRdmMaxOrb + 1];
    if (nrel > p.rel_max || w.rel0 < 0 || w.rel0 + nrel > (int64_t)p.rel.size()) return "rel list out of range";
    for (int i = 0; i < nrel; i++) rel[i] = p.rel[w.rel0 + i];
    if (w.e0 < 0 || w.e1 > ntri || w.e1 - w.e0 > acc_n) return "entries out of range";
    if (w.ld > p.ld_max || w.clen > p.stride) return "slab larger than the staging area";
    std::fill(acc.begin(), acc.end(), 0.0);
    for (int32_t j = w.j0; j < w.j1; j++) {
      const int32_t b = j / w.nruns, jj = j - b * w.nruns;
      if (w.row_list + jj >= (int64_t)p.rows.size()) return "row list out of range";
      const int64_t row0 = p.rows[w.row_list + jj] + (int64_t)b * dim_dw;
      for (int rd = 0; rd < w.ld; rd++)
        for (int c = 0; c < w.clen * cw; c++) {
          const int64_t g = ((row0 + rd) * dim_up + w.c0) * cw + c;
          if (g < 0 || g >= nel * cw) return "vector read out of range";
          stage[(size_t)rd * p.stride * cw + c] = v[g];
        }
      for (int t = 0; t < kRdmThreads; t++)
        for (int e = w.e0 + t, k = 0; e < w.e1; e += kRdmThreads, k++) {
          const uint32_t d = p.ent[e];
          const int ku = d & 15;
          const int offp = ((d >> 8) & 15) * p.stride + ((d >> 4) & 15), offq = ((d >> 16) & 15) * p.stride + ((d >> 12) & 15);
          double* a = &acc[((size_t)k * kRdmThreads + t) * cw];
          for (int i = w.kb[ku]; i < w.kb[ku + 1]; i++) {
            if (i >= nrel) return "run index out of range";
            const int u = rel[i];
            if (offp + u >= stage_n || offq + u >= stage_n) return "staged read out of range";
            if (((d >> 8) & 15) >= (uint32_t)w.ld || ((d >> 16) & 15) >= (uint32_t)w.ld) return "staged read of a row not loaded";
            if ((int)((d >> 4) & 15) + u >= w.clen || (int)((d >> 12) & 15) + u >= w.clen) return "staged read of a column not loaded";
            const double* x = &stage[(size_t)(offp + u) * cw];
            const double* y = &stage[(size_t)(offq + u) * cw];
            if (cw == 1) {
              a[0] += x[0] * y[0];
            } else {
              a[0] += x[0] * y[0] + x[1] * y[1];
              a[1] += x[1] * y[0] - x[0] * y[1];
            }
          }
        }
    }
    for (int t = 0; t < kRdmThreads; t++)
      for (int e = w.e0 + t, k = 0; e < w.e1; e += kRdmThreads, k++) {
        const int64_t o = w.pofs + (e - w.e0);
        if (o < 0 || o >= partial_entries) return "partial sum out of range";
        if (written[(size_t)o]) return "a partial sum is written twice";
        written[(size_t)o] = 1;
        for (int c = 0; c < cw; c++) partial[(size_t)o * cw + c] = acc[((size_t)k * kRdmThreads + t) * cw + c];
      }
  }
  return "";
}

// rdm_final_kernel over the groups (after the memset of the packed result)
static std::string emulate_final(const std::vector<RdmGroup>& groups, int64_t ntri, int cw, const std::vector<double>& partial,
                                 const std::vector<char>& written, double* tri) {
  for (char c : written)
    if (!c) return "a partial sum is never written";
  std::fill(tri, tri + ntri * cw, 0.0);
  std::vector<char> done((size_t)ntri, 0);
  for (const RdmGroup& g : groups) {
    const int64_t E = g.e1 - g.e0;
    if (g.e0 < 0 || g.e1 > ntri || g.pbase < 0 || g.pbase + (int64_t)g.nwg * E > (int64_t)written.size()) return "group out of range";
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

std::string rdm_plan_emulate(const RdmPlan& p, int64_t ntri, int64_t nel, int64_t dim_up, int64_t dim_dw, const double* v,
                             int cw, double* tri) {
  std::vector<double> partial((size_t)p.partial_entries * cw, 0.0);
  std::vector<char> written((size_t)p.partial_entries, 0);
  const std::string why = emulate_tiles(p, ntri, nel, dim_up, dim_dw, v, cw, partial, written);
  return why.empty() ? emulate_final(p.groups, ntri, cw, partial, written, tri) : why;
}

// rows from `first` up to the first run start in [first, first + count) (count when there is none); *run = that run
static int32_t shard_head(const RdmRuns& dw, int64_t first, int64_t count, size_t* run) {
  const size_t j = (size_t)(std::lower_bound(dw.start.begin(), dw.start.end() - 1, (int32_t)first) - dw.start.begin());
  if (run) *run = j;
  if (j >= dw.k.size() || dw.start[j] >= first + count) return (int32_t)count;
  return (int32_t)(dw.start[j] - first);
}

std::string rdm_shard_plan(const RdmRanks& rk, const RdmLayout& l, const RdmRuns& up, const RdmRuns& dw, int64_t dim_up,
                           int64_t dim_dw, int nblk, int cw, int target_wgs, int world, int64_t first, int64_t count,
                           RdmShardPlan& p) {
  p = RdmShardPlan();
  if (world < 1 || first < 0 || count < 0) return "bad range";
  if (dw.start.empty() || dw.start.back() != dim_dw) return "the down runs do not have the sector's rows";
  p.world = world;
  p.q = (dim_dw + world - 1) / world;
  p.first = std::min(first, dim_dw);
  p.count = std::max<int64_t>(0, std::min(count, dim_dw - p.first));
  p.rank = -1;
  if (p.count > 0) {
    if (p.first % p.q != 0 || p.count != std::min(p.q, dim_dw - p.first)) return "the rows are not a rank's range of edigpu_shard_plan";
    p.rank = (int)(p.first / p.q);
  }
  auto range = [&](int r, int64_t& f, int64_t& c) {
    f = std::min<int64_t>((int64_t)r * p.q, dim_dw);
    c = std::max<int64_t>(0, std::min(p.q, dim_dw - f));
  };
  p.heads.assign((size_t)world, 0);
  for (int r = 0; r < world; r++) {
    int64_t f, c;
    range(r, f, c);
    p.heads[(size_t)r] = shard_head(dw, f, c, nullptr);
    p.H = std::max(p.H, (int)p.heads[(size_t)r]);
  }
  if (p.H > kRdmMaxRun - 1) return "a halo longer than a run";
  // the halo this rank sends
  p.pack.nrows = p.H;
  const int32_t head = p.rank >= 0 ? p.heads[(size_t)p.rank] : 0;
  for (int i = 0; i < head; i++) {
    p.pack.sel[i] = 1;
    p.pack.row[i] = i;
  }
  // interior runs and the tail run
  RdmRuns in;
  size_t j = 0;
  if (p.count > 0) shard_head(dw, p.first, p.count, &j);
  for (; p.count > 0 && j < dw.k.size() && dw.start[j] < p.first + p.count; j++) {
    if (dw.start[j + 1] <= p.first + p.count) {
      in.start.push_back((int32_t)(dw.start[j] - p.first));
      in.k.push_back(dw.k[j]);
      continue;
    }
    p.tail_row = (int32_t)(dw.start[j] - p.first);
    p.tail_own = (int32_t)(p.count - p.tail_row);
    p.tail_ld = dw.start[j + 1] - dw.start[j];
    p.tail_k = dw.k[j];
  }
  in.start.push_back((int32_t)p.count);
  rdm_plan(rk, l, up, in, dim_up, p.count, nblk, cw, target_wgs, p.in);
  if (p.tail_ld > 0) {
    p.fill.nrows = p.tail_ld;
    int n = 0;
    for (; n < p.tail_own; n++) {
      p.fill.sel[n] = 1;
      p.fill.row[n] = p.tail_row + n;
    }
    for (int r = p.rank + 1; r < world && n < p.tail_ld; r++)
      for (int i = 0; i < p.heads[(size_t)r] && n < p.tail_ld; i++, n++) {
        p.fill.sel[n] = 2;
        p.fill.rank[n] = r;
        p.fill.row[n] = i;
      }
    if (n != p.tail_ld) return "the following ranks' heads do not complete the tail run";
    RdmRuns one;
    one.start = {0, p.tail_ld};
    one.k = {(uint8_t)p.tail_k};
    rdm_plan(rk, l, up, one, dim_up, p.tail_ld, nblk, cw, target_wgs, p.slab);
  }
  // one buffer of partial sums: per group the workgroups of `in`, then those of `slab` (no slab: `in` as it stands)
  for (const RdmPlan* q : {&p.in, &p.slab})
    for (const RdmGroup& g : q->groups) {
      auto it = std::find_if(p.groups.begin(), p.groups.end(), [&](const RdmGroup& m) { return m.e0 == g.e0; });
      if (it == p.groups.end()) {
        p.groups.push_back(g);
      } else {
        if (it->e1 != g.e1) return "the two work lists split a down class differently";
        it->nwg += g.nwg;
      }
    }
  for (RdmGroup& g : p.groups) {
    g.pbase = p.partial_entries;
    p.partial_entries += (int64_t)g.nwg * (g.e1 - g.e0);
  }
  std::vector<int32_t> next(p.groups.size(), 0);
  for (RdmPlan* q : {&p.in, &p.slab})
    for (RdmWork& w : q->work) {
      const size_t g = (size_t)(std::find_if(p.groups.begin(), p.groups.end(), [&](const RdmGroup& m) { return m.e0 == w.e0; }) -
                                p.groups.begin());
      if (g >= p.groups.size() || p.groups[g].e1 != w.e1) return "a workgroup without a group";
      w.pofs = p.groups[g].pbase + (int64_t)next[g]++ * (w.e1 - w.e0);
    }
  return "";
}

std::string rdm_rows_emulate(const RdmShardPlan& p, const RdmRowCopy& t, int nblk, int64_t rowlen, const double* v,
                             const double* halos, double* dst) {
  if (t.nrows < 0 || t.nrows > kRdmMaxRun) return "more rows than a run";
  const int64_t rank_stride = (int64_t)nblk * p.H * rowlen;  // of one vector
  for (int b = 0; b < nblk; b++)
    for (int r = 0; r < t.nrows; r++)
      for (int64_t c = 0; c < rowlen; c++) {
        double x = 0.0;
        if (t.sel[r] == 1) {
          if (t.row[r] < 0 || t.row[r] >= p.count || !v) return "shard row out of range";
          x = v[((int64_t)b * p.count + t.row[r]) * rowlen + c];
        } else if (t.sel[r] == 2) {
          if (t.rank[r] < 0 || t.rank[r] >= p.world || !halos) return "halo rank out of range";
          if (t.row[r] < 0 || t.row[r] >= p.heads[(size_t)t.rank[r]]) return "halo row past its rank's head";
          x = halos[t.rank[r] * rank_stride + ((int64_t)b * p.H + t.row[r]) * rowlen + c];
        } else if (t.sel[r] != 0) {
          return "unknown row source";
        }
        dst[((int64_t)b * t.nrows + r) * rowlen + c] = x;
      }
  return "";
}

std::string rdm_shard_emulate(const RdmShardPlan& p, int64_t ntri, int64_t dim_up, int nblk, const double* v_shard,
                              const double* slab, int cw, double* tri) {
  std::vector<double> partial((size_t)p.partial_entries * cw, 0.0);
  std::vector<char> written((size_t)p.partial_entries, 0);
  std::string why = emulate_tiles(p.in, ntri, p.count * dim_up * nblk, dim_up, p.count, v_shard, cw, partial, written);
  if (why.empty() && p.tail_ld > 0)
    why = emulate_tiles(p.slab, ntri, (int64_t)p.tail_ld * dim_up * nblk, dim_up, p.tail_ld, slab, cw, partial, written);
  return why.empty() ? emulate_final(p.groups, ntri, cw, partial, written, tri) : why;
}

}  // namespace edigpu
