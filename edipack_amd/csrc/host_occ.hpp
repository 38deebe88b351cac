// host_occ.hpp -- host tables of the occupation operators (edigpu_apply_occ, edigpu_occ_moments).  No HIP in here:
// tests/host_occ.cpp compiles this with g++.
//
// Everything diagonal in the occupation basis needs one thing per state: the impurity occupation pattern, i.e. the low
// norb bits of the map word of each spin (ED_SECTOR.f90:1141-1430 read the same bits through bdecomp).  Normal mode keeps
// one pattern per up index and one per down index; the superc / nonsu2 sectors one per row, up | down << norb.
#pragma once
#include <cstdint>
#include <vector>

namespace edigpu {

constexpr int kOccMaxOrb = 5;                  // == EDIGPU_MAXORB
constexpr int kOccMaxPat = 1 << kOccMaxOrb;    // patterns of one spin
constexpr int kOccSums = 64;                   // slots of one vector's sums: 1 + (2 norb)(2 norb + 1) / 2 <= 56 used

// out[i] = map[i] & (2^norb - 1): the pattern of one spin's word (normal mode: the up or the down map)
void occ_patterns_word(const int32_t* map, int64_t n, int norb, uint16_t* out);
// out[i] = up pattern | down pattern << norb of the state iup + idw 2^ns of a superc / nonsu2 map
void occ_patterns_state(const int32_t* map, int64_t n, int norb, int ns, uint16_t* out);
// tab[p] = sum over the orbitals a in p, ascending, of w[a]; kOccMaxPat entries, those past 2^norb are 0
void occ_weight_table(const double* w, int norb, double* tab);

// Rows of a normal-mode vector (nblk phonon blocks of dim_dw rows, the row's pattern is pd[row % dim_dw]) sorted by
// their down pattern, stable: order[k] = k-th row, run[p] .. run[p + 1] = the positions of pattern p (kOccMaxPat + 1
// entries).  The moments kernel walks a run with one down pattern for every lane.
void occ_sort_rows(const uint8_t* pd, int64_t dim_dw, int nblk, std::vector<int32_t>& order, int32_t* run);

// The tables of a rank's rows [first, first + count) of a sector (edigpu_*_sharded of the occupation operators): the
// range is cut to the sector, a rank past the last row gets empty tables.  Normal mode (flat = false): pat = the down
// patterns pd[n], the view's pd = that slice and order / run = occ_sort_rows of it over nblk blocks of `count` local
// rows -- the up patterns are the sector's own.  Flat: pat = the state patterns, pu = their slice.
struct OccShardView {
  int64_t first = 0, count = 0;  // after the cut
  std::vector<uint16_t> pu;      // flat only
  std::vector<uint8_t> pd;       // normal only
  std::vector<int32_t> order;
  int32_t run[kOccMaxPat + 1] = {0};
};
void occ_shard_view(const uint16_t* pat, int64_t n, bool flat, int nblk, int64_t first, int64_t count, OccShardView& view);

// The sums a vector is reduced to: slot 0 = <v|v>, then the upper triangle (x <= y, row-major) of the 2 norb x 2 norb
// moment matrix, x = a for (a, up) and norb + a for (a, down).  Per slot the up bits and the down bits an element's
// patterns must hold to count (need_up / need_dw, kOccSums entries each; unused slots hold 0xFF).  Returns the slots used.
int occ_sum_slots(int norb, uint8_t* need_up, uint8_t* need_dw);
// sums (kOccSums) -> moments[2 norb][2 norb] (both triangles) and <v|v>
void occ_expand_sums(const double* sums, int norb, double* moments, double* norm2);

}  // namespace edigpu
