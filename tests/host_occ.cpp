// ctypes shim over csrc/host_occ.cpp for tests/test_occupations_host.py (compiled with g++, no HIP).
#include "host_occ.hpp"

#include <cstring>
#include <vector>

using namespace edigpu;

extern "C" {

void ho_patterns_word(const int32_t* map, int64_t n, int norb, uint16_t* out) { occ_patterns_word(map, n, norb, out); }

void ho_patterns_state(const int32_t* map, int64_t n, int norb, int ns, uint16_t* out) {
  occ_patterns_state(map, n, norb, ns, out);
}

void ho_weight_table(const double* w, int norb, double* tab) { occ_weight_table(w, norb, tab); }

// order: dim_dw * nblk entries, run: 33 entries
void ho_sort_rows(const uint8_t* pd, int64_t dim_dw, int nblk, int32_t* order, int32_t* run) {
  std::vector<int32_t> o;
  occ_sort_rows(pd, dim_dw, nblk, o, run);
  if (!o.empty()) std::memcpy(order, o.data(), o.size() * sizeof(int32_t));
}

int ho_sum_slots(int norb, uint8_t* need_up, uint8_t* need_dw) { return occ_sum_slots(norb, need_up, need_dw); }

void ho_expand_sums(const double* sums, int norb, double* moments, double* norm2) {
  occ_expand_sums(sums, norb, moments, norm2);
}

}  // extern "C"
