// Test-only shim: the local-block tables (csrc/host_sb.cpp) and the per-block routines the gfx950 kernels run
// (csrc/sb_core.hpp) evaluated on the host, against the explicit arrays of the same sector (hd, Hup, Hdw, Hnd CSR from
// csrc/host_build.cpp).  Compiled with g++ by tests/test_host_sb.py; never part of the product.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "host_build.hpp"
#include "host_ib.hpp"
#include "host_sb.hpp"
#include "sb_core.hpp"
#include "switches.cpp"  // (compiled into this shim: it samples the environment at every call, like the C-ABI builders)
using namespace edigpu;

static std::string g_err;
extern "C" const char* host_sb_error() { return g_err.c_str(); }

namespace {

int64_t vec_len(const HostIb& ib) { return (int64_t)ib.npanels * kIbPanel * ib.dw.dim; }
int64_t vec_at(const HostIb& ib, int64_t row, int pos) {
  return (int64_t)(pos / kIbPanel) * ib.dw.dim * kIbPanel + row * kIbPanel + pos % kIbPanel;
}

// rows [row0, row0 + nrows) of the sector; at(r, p): element of row row0 + r, padded position p
template <int NIMP, int NB0, int AMODE, class At>
void emulate_rows(const HostIb& ib, const HostSb& sbt, const std::vector<double>& v, std::vector<double>& hv, int64_t row0,
                  int64_t nrows, At&& at) {
  constexpr int NLOC = NIMP + NB0;
  const int plen = ib.npanels * kIbPanel, nimp = 1 << NIMP, nwv = sbt.rows_nt / 64;
  std::vector<double> img((size_t)sbt.rimg_len, 0.0), res((size_t)sbt.rimg_len, 0.0);
  sb::RowImage im;
  im.row = img.data();
  im.rank = sbt.urank.data();
  im.ebath = sbt.ebw.data();
  im.cs = sbt.rcs;
  for (int64_t r = 0; r < nrows; r++) {
    const int64_t rg = row0 + r;
    for (int p = 0; p < plen; p++) img[sbt.rmap[p]] = v[at(r, p)];  // (padding: zeros into the last word)
    res = img;
    for (int s = 0; s < sbt.rows_nbt; s++)
      for (int wv = 0; wv < nwv; wv++) {
        const int32_t sd = sbt.uslot[(size_t)s * nwv + wv];
        if (sd < 0) continue;
        const int n = sd & 0xFF, i0 = sd >> 8;
        for (int l = 0; l < 64; l++) {
          const uint16_t e = sbt.ublist[((size_t)s * nwv + wv) * 64 + l];
          const uint32_t w = e & 0x7FFFu, i = (uint32_t)(i0 + l);
          sb::for_class<NLOC>(n, [&](auto N) {
            constexpr int nn = decltype(N)::value;
            double acc[sb::binom(NLOC, nn)];
            sb::rows_block<NIMP, NB0, AMODE, nn, 0>(im, w, i, sbt.up.nbw, sbt.up.vtab.data(), 4, sbt.up.korb.data(), sbt.up.tloc.data(),
                                                 ib.ed[rg], &ib.xu[(size_t)ib.impd[rg] * nimp], sbt.e0.data(), acc);
            if (!(e & kIbSkip))
              for (int j = 0; j < sb::binom(NLOC, nn); j++) res[(size_t)(sb::wbase(NLOC, nn) + j) * sbt.rcs + i] = acc[j];
          });
        }
      }
    for (int p = 0; p < plen; p++) hv[at(r, p)] = res[sbt.rmap[p]];
  }
}

template <int NIMP, int NB0, int AMODE>
void emulate_rows(const HostIb& ib, const HostSb& sbt, const std::vector<double>& v, std::vector<double>& hv) {
  emulate_rows<NIMP, NB0, AMODE>(ib, sbt, v, hv, 0, ib.dw.dim, [&](int64_t r, int p) { return vec_at(ib, r, p); });
}

// rows staged in halves: one image per value of the top walked bit, the hop over the top level from the vector itself
template <int NIMP, int NB0, int AMODE>
void emulate_rows_split(const HostIb& ib, const HostSb& sbt, const std::vector<double>& v, std::vector<double>& hv) {
  constexpr int NLOC = NIMP + NB0;
  const int nimp = 1 << NIMP, nwv = sbt.rows_nt / 64, top = sbt.up.nbw - 1;
  for (int h = 0; h < 2; h++) {
    const SbUpHalf& hf = sbt.half[h];
    const int plen = hf.npanels * kIbPanel, p00 = hf.panel0 * kIbPanel;
    std::vector<double> img((size_t)sbt.rimg_len, 0.0), res((size_t)sbt.rimg_len, 0.0);
    sb::RowImage im;
    im.row = img.data();
    im.rank = sbt.urank.data();
    im.ebath = hf.ebw.data();
    im.cs = sbt.rcs;
    for (int64_t r = 0; r < ib.dw.dim; r++) {
      for (int p = 0; p < plen; p++) img[hf.rmap[p]] = v[vec_at(ib, r, p00 + p)];
      res = img;
      for (int s = 0; s < sbt.rows_nbt; s++)
        for (int wv = 0; wv < nwv; wv++) {
          const int32_t sd = hf.uslot[(size_t)s * nwv + wv];
          if (sd < 0) continue;
          const int n = sd & 0xFF, i0 = sd >> 8;
          for (int l = 0; l < 64; l++) {
            const size_t at = ((size_t)s * nwv + wv) * 64 + l;
            const uint16_t e = hf.ublist[at];
            const uint32_t wl = e & 0x7FFFu, i = (uint32_t)(i0 + l);
            sb::for_class<NLOC>(n, [&](auto N) {
              constexpr int nn = decltype(N)::value;
              double acc[sb::binom(NLOC, nn)];
              sb::rows_block<NIMP, NB0, AMODE, nn, 0>(im, wl, i, top, sbt.up.vtab.data(), 4, sbt.up.korb.data(), sbt.up.tloc.data(),
                                                   ib.ed[r], &ib.xu[(size_t)ib.impd[r] * nimp], sbt.e0.data(), acc);
              auto top_hop = [&](auto TS) {
                constexpr bool ts = decltype(TS)::value;
                constexpr int MP = sb::rows_top_words<NLOC, nn, ts>();
                if constexpr (MP > 0) {
                  double xp[MP];
                  const int jg = hf.ugap[at] & 0x0F, g = hf.ugap[at] >> 4;
                  for (int j = 0; j < MP; j++)
                    xp[j] = hf.utop[at] == kIbNone ? 0.0 : v[vec_at(ib, r, hf.utop[at] + j + (j >= jg ? g : 0))];
                  sb::rows_top<NIMP, NB0, nn, ts>(wl, &sbt.up.vtab[(size_t)top * 4], xp, acc);
                }
              };
              if (h) top_hop(std::true_type{}); else top_hop(std::false_type{});
              if (!(e & kIbSkip))
                for (int j = 0; j < sb::binom(NLOC, nn); j++) res[(size_t)(sb::wbase(NLOC, nn) + j) * sbt.rcs + i] = acc[j];
            });
          }
        }
      for (int p = 0; p < plen; p++) hv[vec_at(ib, r, p00 + p)] = res[hf.rmap[p]];
    }
  }
}

template <int NIMP, int NB0, int AMODE, class T>
void emulate_cols(const HostIb& ib, const HostSb& sbt, const std::vector<double>& v, std::vector<double>& hv) {
  constexpr int NLOC = NIMP + NB0;
  constexpr int CW = (int)(sizeof(T) / sizeof(double));
  const int gs = sbt.cols_gs;
  const int64_t dd = ib.dw.dim, ps = dd * kIbPanel;
  const int nch = (int)sbt.chunk_row.size() - 1;
  for (int pn = 0; pn < ib.npanels; pn++)
    for (int c = 0; c < nch; c++) {
      const int row0 = sbt.chunk_row[c];
      const double* chunk = &v[(size_t)pn * ps + (size_t)row0 * kIbPanel];
      for (int q = sbt.chunk_slot[c]; q < sbt.chunk_slot[c + 1]; q++) {
        const int n = sbt.dslot[q];
        if (n < 0) continue;
        for (int g = 0; g < gs; g++) {
          const uint16_t e = sbt.dblist[(size_t)q * gs + g];
          if (e & kIbSkip) continue;
          const uint32_t w = e & 0x7FFFu;
          const int own = sbt.dw.first[w];
          for (int col = 0; col < kIbPanel; col += CW)
            sb::for_class<NLOC>(n, [&](auto N) {
              constexpr int nn = decltype(N)::value;
              constexpr int M = sb::binom(NLOC, nn);
              T acc[M];
              std::memset(acc, 0, sizeof(acc));
              auto gload = [&](int grow) -> const double* { return &v[(size_t)pn * ps + (size_t)grow * kIbPanel + col]; };
              sb::cols_block<NIMP, NB0, AMODE, nn, T>(chunk, row0, w, w >> sbt.lowbits, own, &sbt.dmeta[(size_t)w * 16], sbt.dw.nbw, sbt.lowbits,
                                                   sbt.dw.vtab.data(), 4, sbt.dw.korb.data(), sbt.dw.tloc.data(), col, gload, acc, [] {});
              if (ib.nterms > 0)
                sb::cols_block_nd<NIMP, NB0, nn, T>(chunk, own - row0, col, ib.nterms, ib.ndcoef.data(), sbt.nd_dw.data(),
                                                 &ib.nd_up[(size_t)pn * kIbPanel], ib.npanels * kIbPanel, acc);
              for (int j = 0; j < M; j++) {
                double* h = &hv[(size_t)pn * ps + (size_t)(own + j) * kIbPanel + col];
                for (int cc = 0; cc < CW; cc++) h[cc] += reinterpret_cast<const double*>(&acc[j])[cc];
              }
            });
        }
      }
    }
}

template <int NIMP, int NB0>
void emulate(const HostIb& ib, const HostSb& sbt, const std::vector<double>& v, std::vector<double>& hv) {
  if (sbt.amode == 1) {
    if constexpr (NIMP > 1) {
      if (sbt.nhalf == 2) emulate_rows_split<NIMP, NB0, 1>(ib, sbt, v, hv); else emulate_rows<NIMP, NB0, 1>(ib, sbt, v, hv);
      if (sbt.cols_gs == 8) emulate_cols<NIMP, NB0, 1, sb::Pair>(ib, sbt, v, hv); else emulate_cols<NIMP, NB0, 1, double>(ib, sbt, v, hv);
    }
  } else {
    if (sbt.nhalf == 2) emulate_rows_split<NIMP, NB0, 0>(ib, sbt, v, hv); else emulate_rows<NIMP, NB0, 0>(ib, sbt, v, hv);
    if (sbt.cols_gs == 8) emulate_cols<NIMP, NB0, 0, sb::Pair>(ib, sbt, v, hv); else emulate_cols<NIMP, NB0, 0, double>(ib, sbt, v, hv);
  }
}

// sb_cols_kernel<SH> on the panels [p0, p0 + np) of one rank (kernels_sb_impl.hpp): v = what the all-to-all delivered
// (slot s = rank s's q rows of these panels), out = (Hdw (x) 1 + Hnd) v in the same form, every row reached through the
// owner-rank arithmetic the kernel uses (sb::shard_roff): the chunk's rows staged one by one, the partner rows of the high
// levels read one by one (LINEAR = false).  false when an address leaves the buffer.
template <int NIMP, int NB0, int AMODE, class T>
bool emulate_cols_shard(const HostIb& ib, const HostSb& sbt, const std::vector<double>& v, std::vector<double>& out, int p0, int np,
                        int64_t q, int npmax, uint32_t magic) {
  constexpr int NLOC = NIMP + NB0;
  constexpr int CW = (int)(sizeof(T) / sizeof(double));
  const int gs = sbt.cols_gs;
  const int64_t kslot = sb::shard_slot(1, npmax, q) - q * 16, len = (int64_t)v.size();
  const int nch = (int)sbt.chunk_row.size() - 1;
  bool inside = true;
  const std::vector<double> zeros(16, 0.0);
  for (int pl = 0; pl < np; pl++) {
    const int pn = p0 + pl;
    const int64_t base = (int64_t)pl * q * 16;
    auto off = [&](int g, int col, int n) -> int64_t {  // (n doubles from there on must lie inside the buffer)
      const int64_t o = base + sb::shard_roff(g, magic, kslot) + col;
      if (o < 0 || o + n > len) {
        inside = false;
        return -1;
      }
      return o;
    };
    for (int c = 0; c < nch; c++) {
      const int row0 = sbt.chunk_row[c], nrows = sbt.chunk_row[c + 1] - row0;
      std::vector<double> chunk((size_t)nrows * kIbPanel, 0.0);
      for (int u = 0; u < nrows; u++) {
        const int64_t o = off(row0 + u, 0, 16);
        if (o >= 0) std::copy(&v[(size_t)o], &v[(size_t)o] + 16, &chunk[(size_t)u * kIbPanel]);
      }
      for (int qs = sbt.chunk_slot[c]; qs < sbt.chunk_slot[c + 1]; qs++) {
        const int n = sbt.dslot[qs];
        if (n < 0) continue;
        for (int g = 0; g < gs; g++) {
          const uint16_t e = sbt.dblist[(size_t)qs * gs + g];
          if (e & kIbSkip) continue;
          const uint32_t w = e & 0x7FFFu;
          const int own = sbt.dw.first[w];
          for (int col = 0; col < kIbPanel; col += CW)
            sb::for_class<NLOC>(n, [&](auto N) {
              constexpr int nn = decltype(N)::value;
              constexpr int M = sb::binom(NLOC, nn);
              T acc[M];
              std::memset(acc, 0, sizeof(acc));
              auto gload = [&](int grow) -> const double* {
                const int64_t o = off(grow, col, CW);
                return o >= 0 ? &v[(size_t)o] : zeros.data();
              };
              sb::cols_block<NIMP, NB0, AMODE, nn, T, false>(chunk.data(), row0, w, w >> sbt.lowbits, own, &sbt.dmeta[(size_t)w * 16], sbt.dw.nbw,
                                                          sbt.lowbits, sbt.dw.vtab.data(), 4, sbt.dw.korb.data(), sbt.dw.tloc.data(), col, gload, acc, [] {});
              if (ib.nterms > 0)
                sb::cols_block_nd<NIMP, NB0, nn, T>(chunk.data(), own - row0, col, ib.nterms, ib.ndcoef.data(), sbt.nd_dw.data(),
                                                 &ib.nd_up[(size_t)pn * kIbPanel], ib.npanels * kIbPanel, acc);
              for (int j = 0; j < M; j++) {
                const int64_t o = off(own + j, col, CW);
                if (o >= 0)
                  for (int cc = 0; cc < CW; cc++) out[(size_t)o + cc] = reinterpret_cast<const double*>(&acc[j])[cc];
              }
            });
        }
      }
    }
  }
  return inside;
}

// the rows kernel on a rank's rows [row0, row0 + count), both vectors in the shard form (launch_sb_rows_shard)
template <int NIMP, int NB0>
void emulate_shard_rows(const HostIb& ib, const HostSb& sbt, int64_t row0, int64_t count, int64_t q, const std::vector<double>& v,
                        std::vector<double>& hv) {
  auto at = [&](int64_t r, int p) { return sb::shard_at(p, r, q); };
  if (sbt.amode == 1) {
    if constexpr (NIMP > 1) emulate_rows<NIMP, NB0, 1>(ib, sbt, v, hv, row0, count, at);
  } else {
    emulate_rows<NIMP, NB0, 0>(ib, sbt, v, hv, row0, count, at);
  }
}

template <int NIMP, int NB0>
bool emulate_shard_cols(const HostIb& ib, const HostSb& sbt, const std::vector<double>& v, std::vector<double>& out, int p0, int np,
                        int64_t q, int npmax, uint32_t magic) {
  if (sbt.amode == 1) {
    if constexpr (NIMP > 1)
      return sbt.cols_gs == 8 ? emulate_cols_shard<NIMP, NB0, 1, sb::Pair>(ib, sbt, v, out, p0, np, q, npmax, magic)
                              : emulate_cols_shard<NIMP, NB0, 1, double>(ib, sbt, v, out, p0, np, q, npmax, magic);
    return false;
  }
  return sbt.cols_gs == 8 ? emulate_cols_shard<NIMP, NB0, 0, sb::Pair>(ib, sbt, v, out, p0, np, q, npmax, magic)
                          : emulate_cols_shard<NIMP, NB0, 0, double>(ib, sbt, v, out, p0, np, q, npmax, magic);
}

// the sector's explicit-array product (hd, Hup, Hdw, Hnd CSR) of a seeded vector: the reference of every check here
void explicit_product(const HostNormal& hn, std::vector<double>& v, std::vector<double>& ref) {
  const int64_t du = hn.dim_up, dd = hn.dim_dw, dim = du * dd;
  v.assign((size_t)dim, 0.0);
  ref.assign((size_t)dim, 0.0);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (auto& x : v) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    x = (double)((int64_t)(s >> 11) - ((int64_t)1 << 52)) / (double)((int64_t)1 << 52);
  }
  for (int64_t idw = 0; idw < dd; idw++)
    for (int64_t iup = 0; iup < du; iup++) {
      const int64_t i = iup + idw * du;
      double t = hn.hd[i] * v[i];
      for (int64_t k = hn.up.rowptr[iup]; k < hn.up.rowptr[iup + 1]; k++) t += hn.up.val[k] * v[hn.up.col[k] + idw * du];
      for (int64_t k = hn.dw.rowptr[idw]; k < hn.dw.rowptr[idw + 1]; k++) t += hn.dw.val[k] * v[iup + hn.dw.col[k] * du];
      if (hn.has_nd)
        for (int64_t k = hn.nd.rowptr[i]; k < hn.nd.rowptr[i + 1]; k++) t += hn.nd.val[k] * v[hn.nd.col[k]];
      ref[i] = t;
    }
}

}  // namespace

// H*v of the sector (nup, ndw) for a seeded vector, through the explicit arrays and through the local-block tables with
// nb0 low bath levels folded into the blocks.  info: [0] valid, [1] lowbits, [2] chunks, [3] largest chunk, [4] amode,
// [5] Hnd terms, [6] wave-slots of the rows kernel in use, [7] local levels.
// Returns 0 and *maxdiff = max |difference| / max |reference|; 1 when the tables are refused (message in
// host_sb_error()); 2 on a builder error.
static int sb_check(const edigpu_model* m, int nup, int ndw, int nb0, int max_chunk_rows, int rows_nt, int rows_nbt,
                    int cols_nw, int cols_gs, int lds_budget, int32_t* info, double* maxdiff);
extern "C" int host_sb_check(const edigpu_model* m, int nup, int ndw, int nb0, int max_chunk_rows, int rows_nt, int rows_nbt,
                             int cols_nw, int cols_gs, int32_t* info, double* maxdiff) {
  return sb_check(m, nup, ndw, nb0, max_chunk_rows, rows_nt, rows_nbt, cols_nw, cols_gs, 0, info, maxdiff);
}
// the same with the rows staged in halves (impurity-block image built with lds_budget < 0: always split)
extern "C" int host_sb_check_split(const edigpu_model* m, int nup, int ndw, int nb0, int max_chunk_rows, int rows_nt, int rows_nbt,
                                   int cols_nw, int cols_gs, int32_t* info, double* maxdiff) {
  return sb_check(m, nup, ndw, nb0, max_chunk_rows, rows_nt, rows_nbt, cols_nw, cols_gs, -1, info, maxdiff);
}
static int sb_check(const edigpu_model* m, int nup, int ndw, int nb0, int max_chunk_rows, int rows_nt, int rows_nbt,
                    int cols_nw, int cols_gs, int lds_budget, int32_t* info, double* maxdiff) {
  HostNormal hn;
  const Switches sw = Switches::sample();
  g_err = build_normal(*m, nup, ndw, 0, -1, hn, true, !sw.nd_no_merge);
  if (!g_err.empty()) return 2;
  HostIb ib;
  build_ib(hn, max_chunk_rows, ib, lds_budget);
  std::memset(info, 0, 8 * sizeof(int32_t));
  if (!ib.valid) {
    g_err = ib.why;
    return 1;
  }
  HostSb sbt;
  build_sb(hn, ib, nb0, max_chunk_rows, rows_nt, rows_nbt, cols_nw, sbt, cols_gs, sw.sb_amode);
  if (!sbt.valid) {
    g_err = sbt.why;
    return 1;
  }
  info[0] = 1;
  info[1] = sbt.lowbits;
  info[2] = (int)sbt.chunk_row.size() - 1;
  info[3] = sbt.max_chunk_rows;
  info[4] = sbt.amode;
  info[5] = ib.nterms;
  for (int32_t sd : sbt.uslot) info[6] += sd >= 0;
  if (sbt.nhalf == 2) info[6] = 200 + (int)sbt.half[0].uslot.size();
  info[7] = sbt.nloc;
  const int64_t du = hn.dim_up, dd = hn.dim_dw;
  std::vector<double> v, ref;
  explicit_product(hn, v, ref);
  std::vector<double> vi((size_t)vec_len(ib), 0.0), hi((size_t)vec_len(ib), 0.0);
  for (int64_t idw = 0; idw < dd; idw++)
    for (int64_t iup = 0; iup < du; iup++) vi[vec_at(ib, idw, ib.pos[iup])] = v[iup + idw * du];
  const int key = sbt.norb * 10 + sbt.nb0;
  switch (key) {
    case 11: emulate<1, 1>(ib, sbt, vi, hi); break;
    case 12: emulate<1, 2>(ib, sbt, vi, hi); break;
    case 13: emulate<1, 3>(ib, sbt, vi, hi); break;
    case 14: emulate<1, 4>(ib, sbt, vi, hi); break;
    case 21: emulate<2, 1>(ib, sbt, vi, hi); break;
    case 22: emulate<2, 2>(ib, sbt, vi, hi); break;
    case 23: emulate<2, 3>(ib, sbt, vi, hi); break;
    case 31: emulate<3, 1>(ib, sbt, vi, hi); break;
    case 32: emulate<3, 2>(ib, sbt, vi, hi); break;
    case 33: emulate<3, 3>(ib, sbt, vi, hi); break;
    default: g_err = "no instantiation for this (norb, nb0)"; return 2;
  }
  double worst = 0.0, scale = 0.0;
  for (int64_t idw = 0; idw < dd; idw++)
    for (int64_t iup = 0; iup < du; iup++) {
      const double got = hi[vec_at(ib, idw, ib.pos[iup])], want = ref[iup + idw * du];
      worst = std::max(worst, std::fabs(got - want));
      scale = std::max(scale, std::fabs(want));
    }
  {  // the padding columns must stay zero
    std::vector<char> real((size_t)ib.npanels * kIbPanel, 0);
    for (int64_t iup = 0; iup < du; iup++) real[ib.pos[iup]] = 1;
    for (int p = 0; p < ib.npanels * kIbPanel; p++)
      if (!real[p])
        for (int64_t idw = 0; idw < dd; idw++)
          if (hi[vec_at(ib, idw, p)] != 0.0) {
            g_err = "a padding column received a value";
            return 2;
          }
  }
  *maxdiff = scale > 0.0 ? worst / scale : worst;
  return 0;
}

// The sharded product of edigpu_shard.hip (sharded_hv_panels) over `world` ranks on the host, rank by rank in the shard
// form: the conversion of a rank's rows to that form, the rows kernel on them, the all-to-all as plain copies of the
// npmax q 16-double slots, the columns kernel on the rank's panels, the exchange back and the sum in the reference's row
// layout -- against the explicit arrays.  Buffers the library does not clear (the rows half past a rank's count, the
// column half when the rank owns npmax panels) start as NaN: a read of them shows.  info: [0] valid, [1] q, [2] npmax,
// [3] panels, [4] ranks without rows, [5] ranks without panels, [6] Hnd terms, [7] local levels.
// Returns 0 and *maxdiff; 1 when the tables are refused or shard_geometry would not take the shard form (message in
// host_sb_error()); 2 on a builder error, a NaN that reached the result, an address outside a buffer.
extern "C" int host_sb_check_shard(const edigpu_model* m, int nup, int ndw, int nb0, int max_chunk_rows, int rows_nt, int rows_nbt,
                                   int cols_nw, int cols_gs, int world, int32_t* info, double* maxdiff) {
  std::memset(info, 0, 8 * sizeof(int32_t));
  HostNormal hn;
  const Switches sw = Switches::sample();
  g_err = build_normal(*m, nup, ndw, 0, -1, hn, true, !sw.nd_no_merge);
  if (!g_err.empty()) return 2;
  HostIb ib;
  build_ib(hn, max_chunk_rows, ib, 0);
  if (!ib.valid || ib.nhalf != 1) {
    g_err = ib.valid ? "rows staged in halves: no shard form" : ib.why;
    return 1;
  }
  HostSb sbt;
  build_sb(hn, ib, nb0, max_chunk_rows, rows_nt, rows_nbt, cols_nw, sbt, cols_gs, sw.sb_amode);
  if (!sbt.valid) {
    g_err = sbt.why;
    return 1;
  }
  const int64_t du = hn.dim_up, dd = hn.dim_dw, q = (dd + world - 1) / world;
  if (!sb::shard_exact(world, q)) {
    g_err = "no exact owner rank for these rows per rank: the column-block exchange";
    return 1;
  }
  const int npmax = (ib.npanels + world - 1) / world;
  const int64_t per = sb::shard_slot(1, npmax, q), len = sb::shard_slot(world, npmax, q);
  const uint32_t magic = sb::shard_magic(q);
  info[0] = 1;
  info[1] = (int32_t)q;
  info[2] = npmax;
  info[3] = ib.npanels;
  info[6] = ib.nterms;
  info[7] = sbt.nloc;
  std::vector<int32_t> colof((size_t)ib.npanels * kIbPanel, -1);
  for (int64_t iup = 0; iup < du; iup++) colof[(size_t)ib.pos[iup]] = (int32_t)iup;
  std::vector<double> v, ref;
  explicit_product(hn, v, ref);
  const double nan = std::nan("");
  std::vector<std::vector<double>> shard(world), rowh(world), recv(world), colh(world), back(world);
  for (int r = 0; r < world; r++) {
    const int64_t first = std::min<int64_t>(r * q, dd), count = std::max<int64_t>(0, std::min<int64_t>(q, dd - first));
    info[4] += count == 0;
    shard[r].assign((size_t)len, 0.0);  // k_shard_to_panels
    for (int64_t e = 0; e < len; e++) {
      int64_t p, i;
      int l;
      sb::shard_pos(e, q, p, i, l);
      const int c = p < ib.npanels ? colof[(size_t)p * kIbPanel + l] : -1;
      shard[r][(size_t)e] = (c >= 0 && i < count) ? v[(size_t)((first + i) * du + c)] : 0.0;
    }
    rowh[r].assign((size_t)len, nan);
    const int key = sbt.norb * 10 + sbt.nb0;
#define SHARD_ROWS(N, B) \
  case N * 10 + B: emulate_shard_rows<N, B>(ib, sbt, first, count, q, shard[r], rowh[r]); break;
    switch (key) {
      SHARD_ROWS(1, 1) SHARD_ROWS(1, 2) SHARD_ROWS(1, 3) SHARD_ROWS(1, 4) SHARD_ROWS(2, 1) SHARD_ROWS(2, 2) SHARD_ROWS(2, 3)
      SHARD_ROWS(3, 1) SHARD_ROWS(3, 2) SHARD_ROWS(3, 3)
      default: g_err = "no instantiation for this (norb, nb0)"; return 2;
    }
#undef SHARD_ROWS
  }
  for (int d = 0; d < world; d++) {  // the all-to-all: slot s of rank d <- slot d of rank s
    recv[d].assign((size_t)len, nan);
    for (int s = 0; s < world; s++) std::copy(&shard[s][(size_t)(d * per)], &shard[s][(size_t)(d * per)] + per, &recv[d][(size_t)(s * per)]);
  }
  for (int d = 0; d < world; d++) {
    const int p0 = d * npmax, np = std::max(0, std::min(npmax, ib.npanels - p0));
    info[5] += np == 0;
    colh[d].assign((size_t)len, np < npmax ? 0.0 : nan);  // (sharded_hv_panels clears it only then)
    bool inside = true;
    const int key = sbt.norb * 10 + sbt.nb0;
#define SHARD_COLS(N, B) \
  case N * 10 + B: inside = np == 0 || emulate_shard_cols<N, B>(ib, sbt, recv[d], colh[d], p0, np, q, npmax, magic); break;
    switch (key) {
      SHARD_COLS(1, 1) SHARD_COLS(1, 2) SHARD_COLS(1, 3) SHARD_COLS(1, 4) SHARD_COLS(2, 1) SHARD_COLS(2, 2) SHARD_COLS(2, 3)
      SHARD_COLS(3, 1) SHARD_COLS(3, 2) SHARD_COLS(3, 3)
      default: g_err = "no instantiation for this (norb, nb0)"; return 2;
    }
#undef SHARD_COLS
    if (!inside) {
      g_err = "the columns kernel addressed a row outside the buffer";
      return 2;
    }
  }
  for (int s = 0; s < world; s++) {  // the exchange back
    back[s].assign((size_t)len, nan);
    for (int d = 0; d < world; d++) std::copy(&colh[d][(size_t)(s * per)], &colh[d][(size_t)(s * per)] + per, &back[s][(size_t)(d * per)]);
  }
  double worst = 0.0, scale = 0.0;
  for (int r = 0; r < world; r++) {  // k_shard_from_panels_add
    const int64_t first = std::min<int64_t>(r * q, dd), count = std::max<int64_t>(0, std::min<int64_t>(q, dd - first));
    for (int64_t i = 0; i < count; i++)
      for (int64_t c = 0; c < du; c++) {
        const int64_t at = sb::shard_at(ib.pos[(size_t)c], i, q);
        const double got = rowh[r][(size_t)at] + back[r][(size_t)at], want = ref[(size_t)((first + i) * du + c)];
        if (!std::isfinite(got)) {
          g_err = "rank " + std::to_string(r) + " read a buffer element nothing wrote (row " + std::to_string(first + i) + ")";
          return 2;
        }
        worst = std::max(worst, std::fabs(got - want));
        scale = std::max(scale, std::fabs(want));
      }
  }
  *maxdiff = scale > 0.0 ? worst / scale : worst;
  return 0;
}

extern "C" int host_sb_shard_exact(int64_t world, int64_t q) { return sb::shard_exact(world, q) ? 1 : 0; }

// The owner rank of the columns kernel in the shard form (sb::shard_owner) against integer division at the boundaries of
// every rank's rows, g = k q - 1 and g = k q (k = 0 .. world, g < world q), for q in [1, max_q] and world in [1, max_world]
// wherever sb::shard_exact admits the pair; and shard_exact itself against the same boundaries of the 32-bit magic
// (q >= 2: admitted exactly when every one of them is right).  out: [0] admitted pairs, [1] owner evaluations,
// [2] wrong owners, [3] pairs where shard_exact disagrees with the magic's boundaries, [4] refused pairs.
extern "C" void host_sb_owner_check(int max_world, int max_q, int64_t* out) {
  for (int k = 0; k < 5; k++) out[k] = 0;
  for (int64_t q = 1; q <= max_q; q++) {
    const uint32_t magic = sb::shard_magic(q);
    int64_t exact_to = 0;  // largest world up to which the magic is right at every boundary (q >= 2)
    if (q >= 2) {
      const uint32_t m32 = (uint32_t)(((uint64_t)1 << 32) / (uint64_t)q + 1);
      while (exact_to < max_world) {
        const uint64_t g = (uint64_t)(exact_to + 1) * q - 1;
        if ((uint32_t)((g * m32) >> 32) != (uint32_t)(g / q)) break;
        exact_to++;
      }
    }
    for (int64_t world = 1; world <= max_world; world++) {
      const bool ok = sb::shard_exact(world, q);
      if (q >= 2 && q <= 0xFFFF && ok != (world <= exact_to)) out[3]++;
      if (!ok) {
        out[4]++;
        continue;
      }
      out[0]++;
      for (int64_t k = 0; k <= world; k++)
        for (int64_t g = k * q - 1; g <= k * q; g++) {
          if (g < 0 || g >= world * q) continue;
          out[1]++;
          if (sb::shard_owner((uint32_t)g, magic) != (uint32_t)(g / q)) out[2]++;
        }
    }
  }
}
