// host_pack.cpp -- see host_pack.hpp.  Product code (host side of the generic kernels); shares nothing with oracle/.
#include "host_pack.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace edigpu {

HostEll encode_ell(const HostCsr& a, bool lds, bool allow_typed, bool allow_16) {
  HostEll e;
  const uint32_t cmul = lds ? 8u : 1u;
  e.nrow = a.nrow;
  e.pitch = (a.nrow + 63) / 64 * 64;
  int w = 0;
  for (int64_t i = 0; i < a.nrow; i++) w = std::max<int>(w, (int)(a.rowptr[i + 1] - a.rowptr[i]));
  e.width = w;
  if (w == 0 || a.nrow == 0) return e;
  // distinct |values| -> coefficient table (slot 0 = 0.0 for padding)
  std::vector<double> coef(1, 0.0);
  bool packable = (a.nrow + 1) * (int64_t)cmul < ((int64_t)1 << 24);
  std::vector<uint8_t> cid((size_t)a.nnz());
  for (int64_t p = 0; p < a.nnz() && packable; p++) {
    const double m = std::fabs(a.val[p]);
    size_t k = 0;
    for (; k < coef.size(); k++)
      if (coef[k] == m) break;
    if (k == coef.size()) {
      if (coef.size() >= 128) {
        packable = false;
        break;
      }
      coef.push_back(m);
    }
    cid[p] = (uint8_t)k;
  }
  // typed layout: slot = (distinct |value|, occurrence of it inside the row), so that every slot has one
  // wave-uniform amplitude.  With generic bath parameters each hop has its own amplitude and a row
  // holds it at most once; symmetric baths repeat amplitudes and get one slot per repetition.
  bool typed = packable && coef.size() > 1 && allow_typed;
  std::vector<int> maxmult(coef.size(), 0), base(coef.size() + 1, 0);
  if (typed) {
    std::vector<int> cnt(coef.size());
    for (int64_t i = 0; i < a.nrow; i++) {
      std::fill(cnt.begin(), cnt.end(), 0);
      for (int64_t p = a.rowptr[i]; p < a.rowptr[i + 1]; p++) cnt[cid[p]]++;
      for (size_t v = 1; v < coef.size(); v++) maxmult[v] = std::max(maxmult[v], cnt[v]);
    }
    for (size_t v = 1; v < coef.size(); v++) base[v + 1] = base[v] + maxmult[v];
    const int nt = base[coef.size()];
    typed = nt >= 1 && nt <= 127 && nt <= std::max(2 * w, w + 8);  // else too many dead slots
  }
  if (typed) {
    const int nt = base[coef.size()];
    e.width = nt;
    e.typed = 1;
    std::vector<double> tc(128, 0.0);
    for (size_t v = 1; v < coef.size(); v++)
      for (int j = 0; j < maxmult[v]; j++) tc[base[v] + j] = coef[v];
    // dead slots: the zero slot of the staged row / column 0 with the live bit (24) clear
    std::vector<uint32_t> pk((size_t)nt * e.pitch, lds ? (uint32_t)a.nrow * 8u : 0u);
    std::vector<int> occ(coef.size());
    for (int64_t i = 0; i < a.nrow; i++) {
      std::fill(occ.begin(), occ.end(), 0);
      for (int64_t p = a.rowptr[i]; p < a.rowptr[i + 1]; p++) {
        if (cid[p] == 0) continue;  // explicit zero
        const int slot = base[cid[p]] + occ[cid[p]]++;
        pk[(size_t)slot * e.pitch + i] = (uint32_t)a.col[p] * cmul | (lds ? 0u : 1u << 24) |
                                         (std::signbit(a.val[p]) ? 0x80000000u : 0u);
      }
    }
    e.coef = std::move(tc);
    // 16-bit image for staged rows whose zero slot lies within 15 bits of byte offset (DimUp <= 4095): entry = byte
    // offset | sign << 15, two consecutive slots of a column in one word (slot 2q low, 2q + 1 high), words column-major
    // [slot pair][column]: a lane's 16-byte load brings 2 slots of its 4 adjacent columns, a wave's load is one
    // contiguous 1 KiB piece, and the table is half the size of the 32-bit one.  An odd width is padded with a dead
    // slot (zero slot of the row, amplitude tc[nt] = 0).  allow_16 off keeps such sectors on the 32-bit image.
    if (lds && (uint64_t)a.nrow * 8u <= 0x7FFFu && allow_16) {
      const uint32_t dead = (uint32_t)a.nrow * 8u;
      const int np = (nt + 1) / 2;
      std::vector<uint32_t> pk16((size_t)np * e.pitch, dead | dead << 16);
      for (int k = 0; k < nt; k++)
        for (int64_t i = 0; i < a.nrow; i++) {
          const uint32_t p = pk[(size_t)k * e.pitch + i];
          const uint32_t h = (p & 0x7FFFu) | (p >> 31) << 15;
          uint32_t& wd = pk16[(size_t)(k >> 1) * e.pitch + i];
          wd = (k & 1) ? (wd & 0xFFFFu) | h << 16 : (wd & 0xFFFF0000u) | h;
        }
      if (a.nrow % 2 == 0) {
        // the same words in ownership order (ell16_owned_col); a thread that owns a column below nrow reads four
        // words of its 256-position block, so the pitch rounds up to 256; positions of columns past the row are dead
        e.pitch16o = (a.nrow + 255) / 256 * 256;
        e.pk16o.assign((size_t)np * e.pitch16o, dead | dead << 16);
        for (int q = 0; q < np; q++)
          for (int64_t pos = 0; pos < e.pitch16o; pos++) {
            const int64_t c = ell16_owned_col(pos);
            if (c < a.nrow) e.pk16o[(size_t)q * e.pitch16o + pos] = pk16[(size_t)q * e.pitch + c];
          }
      }
      e.pk16 = std::move(pk16);
    }
    e.pk = std::move(pk);
    return e;
  }
  if (packable) {
    coef.resize(128, 0.0);
    std::vector<uint32_t> pk((size_t)w * e.pitch);
    for (int k = 0; k < w; k++)
      for (int64_t i = 0; i < e.pitch; i++) pk[(size_t)k * e.pitch + i] = (uint32_t)std::min(i, a.nrow - 1) * cmul;
    for (int64_t i = 0; i < a.nrow; i++) {
      int k = 0;
      for (int64_t p = a.rowptr[i]; p < a.rowptr[i + 1]; p++, k++)
        pk[(size_t)k * e.pitch + i] = (uint32_t)a.col[p] * cmul | ((uint32_t)cid[p] << 24) |
                                      (std::signbit(a.val[p]) ? 0x80000000u : 0u);
    }
    e.pk = std::move(pk);
    e.coef = std::move(coef);
    return e;
  }
  std::vector<int32_t> col((size_t)w * e.pitch);
  std::vector<double> val((size_t)w * e.pitch, 0.0);
  for (int k = 0; k < w; k++)
    for (int64_t i = 0; i < e.pitch; i++) col[(size_t)k * e.pitch + i] = (int32_t)std::min(i, a.nrow - 1);
  for (int64_t i = 0; i < a.nrow; i++) {
    int k = 0;
    for (int64_t p = a.rowptr[i]; p < a.rowptr[i + 1]; p++, k++) {
      col[(size_t)k * e.pitch + i] = a.col[p];
      val[(size_t)k * e.pitch + i] = a.val[p];
    }
  }
  e.col = std::move(col);
  e.val = std::move(val);
  return e;
}

// SELL-64 image of a CSR block (sell_rows_kernel): rows sorted by column, 64 rows per
// slice, column-major inside the slice.  Built when the padding stays below 60 % of the entries.
// max_pad: padded slots allowed per stored entry (1.6 for the dense-ish flat Hamiltonians; the sparse Hnd
// block -- most rows empty -- is cheap in absolute terms and takes more)
HostSell encode_sell(int64_t nrow, int64_t ncol, const int64_t* rowptr, const int32_t* col, const double* val, int cplx,
                     bool is_loc, double max_pad, bool allow_packed) {
  HostSell h;
  if (nrow == 0 || rowptr[nrow] == 0) return h;
  const int w = cplx ? 2 : 1;
  // ---- value dictionary (off-diagonal entries; the loc block's diagonal goes to its own array) ----
  bool packed = ncol < ((int64_t)1 << 24) && allow_packed;
  std::vector<double> dict(w, 0.0);  // id 0 = zero (padding)
  std::vector<uint8_t> ids;
  std::vector<double> diag;
  if (packed) {
    ids.assign((size_t)rowptr[nrow], 0);
    if (is_loc) diag.assign((size_t)nrow * w, 0.0);
    for (int64_t i = 0; i < nrow && packed; i++)
      for (int64_t k = rowptr[i]; k < rowptr[i + 1]; k++) {
        if (is_loc && col[k] == i) {
          for (int q = 0; q < w; q++) diag[i * w + q] += val[k * w + q];
          continue;
        }
        const size_t n = dict.size() / w;
        size_t id = 0;
        for (; id < n; id++)
          if (memcmp(&dict[id * w], &val[k * w], sizeof(double) * w) == 0) break;
        if (id == n) {
          if (n >= 256) {
            packed = false;
            break;
          }
          for (int q = 0; q < w; q++) dict.push_back(val[k * w + q]);
        }
        ids[k] = (uint8_t)id;
      }
  }
  const bool skip_diag = packed && is_loc;
  const int64_t ns = (nrow + 63) / 64;
  std::vector<int32_t> sp((size_t)ns + 1, 0);
  int64_t tot = 0, nent = 0;
  for (int64_t s = 0; s < ns; s++) {
    int64_t mx = 0;
    for (int64_t i = s * 64; i < std::min<int64_t>(nrow, s * 64 + 64); i++) {
      int64_t n = rowptr[i + 1] - rowptr[i];
      if (skip_diag)
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; k++)
          if (col[k] == i) n--;
      mx = std::max(mx, n);
      nent += n;
    }
    tot += mx;
    if (tot >= ((int64_t)1 << 31) / 64) return h;
    sp[s + 1] = (int32_t)tot;
  }
  if (nent > 0 && (double)tot * 64.0 > max_pad * (double)nent) return h;  // too ragged: keep the CSR kernel
  std::vector<int32_t> sc;
  std::vector<uint32_t> spk;
  std::vector<double> sv;
  if (packed) spk.assign((size_t)tot * 64, 0u);
  else {
    sc.assign((size_t)tot * 64, 0);
    sv.assign((size_t)tot * 64 * w, 0.0);
  }
  std::vector<std::pair<int32_t, int64_t>> ord;
  for (int64_t s = 0; s < ns; s++) {
    const int64_t width = sp[s + 1] - sp[s];
    for (int l = 0; l < 64; l++) {
      const int64_t i = s * 64 + l;
      ord.clear();
      if (i < nrow)
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; k++)
          if (!(skip_diag && col[k] == i)) ord.emplace_back(col[k], k);
      std::sort(ord.begin(), ord.end());
      for (int64_t k = 0; k < width; k++) {
        const size_t o = ((size_t)sp[s] + k) * 64 + l;
        const bool live = k < (int64_t)ord.size();
        // padding: repeat the last column (same cache line), value 0 / dictionary id 0
        const int32_t c = live ? ord[k].first : (ord.empty() ? 0 : ord.back().first);
        if (packed) {
          spk[o] = (uint32_t)c | ((uint32_t)(live ? ids[ord[k].second] : 0) << 24);
        } else {
          sc[o] = c;
          if (live)
            for (int q = 0; q < w; q++) sv[o * w + q] = val[ord[k].second * w + q];
        }
      }
    }
  }
  h.built = true;
  h.nslice = ns;
  h.ptr = std::move(sp);
  if (packed) {
    h.packed = true;
    dict.resize((size_t)256 * w, 0.0);
    h.pk = std::move(spk);
    h.dict = std::move(dict);
    if (is_loc) h.diag = std::move(diag);
  } else {
    h.col = std::move(sc);
    h.val = std::move(sv);
  }
  return h;
}

// Row chunks of the LDS-tiled panel sweep (normal_dw_tile_kernel): consecutive local down rows,
// at most rmax per chunk, cut where few SHORT hops (|partner - row| < rmax: the ones a chunk could keep inside)
// cross.  The sorted basis puts rows that share their high bath bits next to each other and the hops among the low
// levels stay inside such a block, so the cheapest cuts are the block boundaries.  Any partition is valid -- the
// kernel tests "partner inside my chunk" by range -- the plan only decides how many gathers are served from LDS.
void plan_tile_chunks(const HostCsr& dw, int64_t dw_first, int64_t dw_count, int rmax, std::vector<int32_t>& starts,
                      int& longest) {
  const int64_t n = dw_count;
  std::vector<int32_t> cross((size_t)n + 2, 0);
  for (int64_t r = 0; r < n; r++) {
    const int64_t g = dw_first + r;
    for (int64_t q = dw.rowptr[g]; q < dw.rowptr[g + 1]; q++) {
      const int64_t pl = (int64_t)dw.col[q] - dw_first;
      if (pl > r && pl < n && pl - r < rmax) {  // crosses every cut i with r < i <= pl
        cross[r + 1]++;
        cross[pl + 1]--;
      }
    }
  }
  for (int64_t i = 1; i <= n; i++) cross[i] += cross[i - 1];
  starts.assign(1, 0);
  longest = 0;
  int64_t s0 = 0;
  while (s0 < n) {
    int64_t cut = n;
    if (n - s0 > rmax) {
      cut = s0 + rmax;
      for (int64_t i = s0 + rmax; i > s0 + rmax / 2; i--)
        if (cross[i] < cross[cut]) cut = i;
    }
    longest = std::max<int>(longest, (int)(cut - s0));
    starts.push_back((int32_t)cut);
    s0 = cut;
  }
}

HostMergedList merge_dw_lists(const HostCsr& dw, const HostFactored& f, int64_t dw_first, int64_t dw_count, int64_t dim_dw) {
  HostMergedList m;
  std::vector<int32_t>&mp = m.rowptr, &mc = m.col;
  std::vector<double>& mv = m.val;
  mp.assign((size_t)dw_count + 1, 0);
  for (int64_t r = 0; r < dw_count; r++) {
    const int64_t g = dw_first + r;
    for (int64_t q = dw.rowptr[g]; q < dw.rowptr[g + 1]; q++) {
      mc.push_back(dw.col[q]);
      mv.push_back(dw.val[q]);
    }
    for (int t = 0; t < f.nterms; t++) {
      const uint32_t jd = f.jdw[(size_t)t * dim_dw + g];
      if (jd != 0xFFFFFFFFu) {
        mc.push_back((int32_t)((jd & 0xFFFFFFu) | ((uint32_t)(t + 1) << 24)));
        mv.push_back((jd >> 31) ? -f.coef[t] : f.coef[t]);
      }
    }
    mp[r + 1] = (int32_t)mc.size();
  }
  mc.resize(mc.size() + 8, 0);   // batched list reads run past the last row's end
  mv.resize(mv.size() + 8, 0.0);
  return m;
}

// per-row lists of the tiled sweep: the hops of a row split into those that stay inside its chunk (entry =
// staged row index) and those that leave it (entry = global row), then the applicable factored Hnd terms
HostTileLists build_tile_lists(const HostCsr& dw, int64_t dim_dw, int64_t dw_first, int64_t dw_count,
                               const std::vector<int32_t>& tile_starts, const HostFactored* f) {
  HostTileLists l;
  const bool with_nd = f != nullptr;
  std::vector<HostInt4>& meta = l.meta;
  std::vector<int32_t>&tc = l.col, &lbeg = l.lbeg;
  std::vector<double>& tv = l.val;
  meta.resize((size_t)dw_count);
  tc.reserve((size_t)dw.rowptr[dim_dw] + 8);
  tv.reserve((size_t)dw.rowptr[dim_dw] + 8);
  for (size_t ch = 0; ch + 1 < tile_starts.size(); ch++) {
    const int64_t cs = tile_starts[ch], ce = tile_starts[ch + 1];
    for (int64_t r = cs; r < ce; r++) {
      const int64_t g = dw_first + r;
      HostInt4 m;
      m.x = (int)tc.size();
      m.y = m.z = m.w = 0;
      for (int pass = 0; pass < 2; pass++) {
        for (int64_t q = dw.rowptr[g]; q < dw.rowptr[g + 1]; q++) {
          const int64_t pl = (int64_t)dw.col[q] - dw_first;
          const bool inside = pl >= cs && pl < ce;
          if (inside == (pass == 0)) {
            tc.push_back(inside ? (int32_t)(pl - cs) : dw.col[q]);
            tv.push_back(dw.val[q]);
            (inside ? m.y : m.z)++;
          }
        }
        // whole batches of 4 (the kernel reads int4 / 4 doubles at a time): pad with (own row, weight 0)
        int& cnt = pass == 0 ? m.y : m.z;
        while (cnt % 4) {
          tc.push_back(pass == 0 ? (int32_t)(r - cs) : (int32_t)g);
          tv.push_back(0.0);
          cnt++;
        }
      }
      if (with_nd)
        for (int t = 0; t < f->nterms; t++) {
          const uint32_t jd = f->jdw[(size_t)t * dim_dw + g];
          if (jd != 0xFFFFFFFFu) {
            tc.push_back((int32_t)((jd & 0xFFFFFFu) | ((uint32_t)(t + 1) << 24)));
            tv.push_back((jd >> 31) ? -f->coef[t] : f->coef[t]);
            m.w++;
          }
        }
      while (tc.size() % 4) {  // the next row starts on a batch boundary (entries never read)
        tc.push_back(0);
        tv.push_back(0.0);
      }
      meta[(size_t)r] = m;
    }
  }
  for (size_t ch = 0; ch + 1 < tile_starts.size(); ch++) lbeg.push_back(meta[(size_t)tile_starts[ch]].x);
  lbeg.push_back((int32_t)tc.size());
  l.list_cap = 4;
  for (size_t ch = 0; ch + 1 < lbeg.size(); ch++) l.list_cap = std::max(l.list_cap, lbeg[ch + 1] - lbeg[ch]);
  tc.resize(tc.size() + 8, 0);  // batched list reads run past a row's end
  tv.resize(tv.size() + 8, 0.0);
  l.has_nd = with_nd;
  return l;
}

std::vector<HostInt4> tile_meta_live(const HostTileLists& l, int64_t dw_first) {
  std::vector<HostInt4> meta = l.meta;
  for (size_t r = 0; r < meta.size(); r++) {
    HostInt4& m = meta[r];
    const int ob = m.x + m.y;
    while (m.z % 4 != 1 && m.z > 0 && l.val[(size_t)(ob + m.z - 1)] == 0.0 &&
           l.col[(size_t)(ob + m.z - 1)] == (int32_t)(dw_first + (int64_t)r))
      m.z--;
  }
  return meta;
}

HostBlockLists build_block_lists(const HostCsr& dw, const HostFactored& f, int64_t dim_dw, int shift, int64_t lds_kb) {
  HostBlockLists b;
  // weight table: +/- every hop amplitude and Hnd coefficient, 0.0 at index 0 (padding entries)
  std::vector<double> wtab{0.0};
  auto widx = [&](double w) -> int {
    for (size_t i = 0; i < wtab.size(); i++)
      if (wtab[i] == w && std::signbit(wtab[i]) == std::signbit(w)) return (int)i;
    wtab.push_back(w);
    return (int)wtab.size() - 1;
  };
  // LDS block of the sweep: lds_kb of staged segments, a multiple of 32 rows; the block's list entries are staged
  // next to them
  int64_t R = std::max<int64_t>(32, std::min<int64_t>(lds_kb * 1024 / ((int64_t)8 << shift), 4096) / 32 * 32);
  std::vector<HostInt4> meta((size_t)dim_dw);
  std::vector<uint32_t> ent;
  ent.reserve((size_t)dw.rowptr[dim_dw] + 8 * (size_t)dim_dw);
  bool fits = true;
  for (int64_t g = 0; g < dim_dw && fits; g++) {
    const int64_t cs = g / R * R;  // first row of g's block
    HostInt4 m = {(int)ent.size(), 0, 0, 0};
    for (int pass = 0; pass < 2; pass++) {  // hops inside the block (entry = index in the block), then the others
      int& cnt = pass == 0 ? m.y : m.z;
      for (int64_t q = dw.rowptr[g]; q < dw.rowptr[g + 1]; q++) {
        const int64_t c = dw.col[q];
        const bool inside = c >= cs && c < cs + R;
        if (inside != (pass == 0)) continue;
        ent.push_back((uint32_t)(inside ? c - cs : c) | ((uint32_t)widx(dw.val[q]) << 16));
        cnt++;
      }
      for (; cnt % 4; cnt++) ent.push_back((uint32_t)(pass == 0 ? g - cs : g));  // (own row, weight 0)
    }
    for (int t = 0; t < f.nterms; t++) {
      const uint32_t jd = f.jdw[(size_t)t * dim_dw + g];
      if (jd == 0xFFFFFFFFu) continue;
      ent.push_back((jd & 0xFFFFu) | ((uint32_t)widx((jd >> 31) ? -f.coef[t] : f.coef[t]) << 16) | ((uint32_t)(t + 1) << 24));
      m.w++;
    }
    while (ent.size() % 4) ent.push_back(0);  // the next row starts on a 16-byte boundary
    meta[(size_t)g] = m;
    fits = wtab.size() <= 256;
  }
  std::vector<int32_t> lend;
  int list_cap = 4;
  for (int64_t cs = 0; cs < dim_dw && fits; cs += R) {
    const int64_t last = std::min<int64_t>(cs + R, dim_dw) - 1;
    const HostInt4& ml = meta[(size_t)last];
    const int end = (ml.x + ml.y + ml.z + ml.w + 3) / 4 * 4;
    lend.push_back(end);
    list_cap = std::max(list_cap, end - meta[(size_t)cs].x);
  }
  // the whole block (segments + lists + row meta) must fit a workgroup's LDS
  fits = fits && (size_t)R * ((size_t)8 << shift) + (size_t)list_cap * 4 + (size_t)R * 16 + 8192 <= 150 * 1024;
  if (fits) {
    wtab.resize(256, 0.0);
    ent.resize(ent.size() + 8, 0);
    b.fits = true;
    b.rows = (int)R;
    b.meta = std::move(meta);
    b.ent = std::move(ent);
    b.wtab = std::move(wtab);
    b.lend = std::move(lend);
    b.list_cap = list_cap;
  }
  return b;
}

int factored_col_halo(const HostFactored& f, int64_t dim_up) {
  int halo = 0;
  for (int t = 0; t < f.nterms; t++)
    for (int64_t c = 0; c < dim_up; c++) {
      const uint32_t jt = f.jup[(size_t)t * dim_up + c];
      if (jt != 0xFFFFFFFFu) halo = std::max<int>(halo, (int)std::llabs((int64_t)(jt & 0x7FFFFFFFu) - c));
    }
  return halo;
}

}  // namespace edigpu
