// host_twin.hpp -- host side of the ED_TWIN=T reorder (edigpu_twin.hip; kernels_twin.hip): which sector is the twin of a
// sector (get_twin_sector, ED_SECTOR.f90:1824-1843) and the table `order` of twin_sector_order (ED_SECTOR.f90:1747-1776)
// with which es_return_dvector (ED_EIGENSPACE.f90:652-720) makes a twin's vector, v_B[i] = v_A[order[i]]:
// order = argsort(flip(state_A(.))), flip as flip_state_other (:1797-1816).  Plain C++, no HIP: the CPU suite compiles this
// file alone (tests/host_twin.cpp, tests/host_twin_sanitize_main.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace edigpu {

enum TwinMode : int { kTwinNormal = 0, kTwinSuperc = 1, kTwinNonsu2 = 2 };

// The twin (t1, t2) of sector (q1, q2): normal (Nup, Ndw) -> (Ndw, Nup); superc Sz -> -Sz; nonsu2 Ntot -> 2 Ns - Ntot
// (q2 ignored, t2 = 0).  self: the sector is its own twin.  Returns "" or why the sector does not exist.
std::string twin_sector(int mode, int ns, int q1, int q2, int& t1, int& t2, bool& self);

// ed_total_ud = F: (nups, ndws) -> (ndws, nups), norb entries each; self when the two lists are equal
void twin_sector_orbs(int norb, const int* nups, const int* ndws, int* tnups, int* tndws, bool& self);

// order[0:n) of a superc / nonsu2 sector whose map is map[0:n) (ascending states iup + idw 2^ns).  superc: flip swaps
// the two ns-bit halves, so the flipped key is (iup, idw) with iup the major word; the map is sorted by (idw, iup), and
// one STABLE counting pass over iup sorts it by (iup, idw): O(n + 2^ns), no comparison sort.  nonsu2: flip complements
// every bit, which reverses the order: order[i] = n - 1 - i (the device needs no table for it; this is for the tests).
// Returns "" or why the map is not one of such a sector.
std::string twin_order(int mode, const int32_t* map, int64_t n, int ns, std::vector<int32_t>& order);

}  // namespace edigpu
