// host_occ.cpp -- host tables of the occupation operators (host_occ.hpp).
#include "host_occ.hpp"

#include <stddef.h>

namespace edigpu {

void occ_patterns_word(const int32_t* map, int64_t n, int norb, uint16_t* out) {
  const uint32_t mask = (1u << norb) - 1u;
  for (int64_t i = 0; i < n; i++) out[i] = (uint16_t)((uint32_t)map[i] & mask);
}

void occ_patterns_state(const int32_t* map, int64_t n, int norb, int ns, uint16_t* out) {
  const uint32_t mask = (1u << norb) - 1u;
  for (int64_t i = 0; i < n; i++) {
    const uint32_t st = (uint32_t)map[i];
    out[i] = (uint16_t)((st & mask) | (((st >> ns) & mask) << norb));
  }
}

void occ_weight_table(const double* w, int norb, double* tab) {
  for (int p = 0; p < kOccMaxPat; p++) {
    double s = 0.0;
    for (int a = 0; a < norb; a++)
      if (p < (1 << norb) && ((p >> a) & 1)) s += w[a];
    tab[p] = s;
  }
}

void occ_sort_rows(const uint8_t* pd, int64_t dim_dw, int nblk, std::vector<int32_t>& order, int32_t* run) {
  const int64_t nrows = dim_dw * nblk;
  for (int p = 0; p <= kOccMaxPat; p++) run[p] = 0;
  for (int64_t r = 0; r < dim_dw; r++) run[pd[r] + 1] += nblk;
  for (int p = 0; p < kOccMaxPat; p++) run[p + 1] += run[p];
  std::vector<int32_t> next(run, run + kOccMaxPat);
  order.assign((size_t)nrows, 0);
  for (int64_t r = 0; r < nrows; r++) order[(size_t)next[pd[r % dim_dw]]++] = (int32_t)r;
}

void occ_shard_view(const uint16_t* pat, int64_t n, bool flat, int nblk, int64_t first, int64_t count, OccShardView& view) {
  view = OccShardView();
  const int64_t lo = first < 0 ? 0 : (first > n ? n : first);
  const int64_t want = count < 0 ? 0 : count;
  const int64_t hi = want > n - lo ? n : lo + want;
  view.first = lo;
  view.count = hi - lo;
  if (flat) {
    view.pu.assign(pat + lo, pat + hi);
    return;
  }
  view.pd.assign(pat + lo, pat + hi);
  occ_sort_rows(view.pd.data(), view.count, nblk, view.order, view.run);
}

int occ_sum_slots(int norb, uint8_t* need_up, uint8_t* need_dw) {
  for (int t = 0; t < kOccSums; t++) need_up[t] = need_dw[t] = 0xFF;
  need_up[0] = need_dw[0] = 0;
  int t = 1;
  const int n2 = 2 * norb;
  for (int x = 0; x < n2; x++)
    for (int y = x; y < n2; y++, t++) {
      uint8_t u = 0, d = 0;
      for (int z : {x, y}) {
        if (z < norb) u |= (uint8_t)(1u << z);
        else d |= (uint8_t)(1u << (z - norb));
      }
      need_up[t] = u;
      need_dw[t] = d;
    }
  return t;
}

void occ_expand_sums(const double* sums, int norb, double* moments, double* norm2) {
  if (norm2) *norm2 = sums[0];
  int t = 1;
  const int n2 = 2 * norb;
  for (int x = 0; x < n2; x++)
    for (int y = x; y < n2; y++, t++) moments[x * n2 + y] = moments[y * n2 + x] = sums[t];
}

}  // namespace edigpu
