// host_pairs.hpp -- host tables of the fused two-operator products on normal-mode vectors (edigpu_apply_pairs_normal):
// the seeds of the pair and exciton susceptibilities (ED_NORMAL/ED_CHI_PAIR.f90, ED_CHI_EXCT.f90).  No HIP in here:
// tests/host_pairs.cpp compiles this with g++.
//
// A term is coef * O2 O1, O1 acting first, each O = c (create <= 0) or c^+ (create > 0) of (iorb, ispin).  An operator
// changes the word of its own species only and its sign counts that species only, (-1)^popcount(word & (bit - 1)), as
// apply_op_C / apply_op_CDG do (ED_SECTOR.f90:465-536).  So O2 O1 is a signed partial permutation P_dw (x) P_up of
// V[idw][iup]: per term one table over the destination's up index and one over its down index, each the composition of
// the 0, 1 or 2 operators of that spin.  Entry format (the partner entries of HostFactored): index in the source sector
// in bits 0..30, bit 31 = minus, 0xFFFFFFFF = no preimage.  The basis of a species is the ascending list of the ns-bit
// words of fixed popcount (build_sector, ED_SECTOR.f90:165-373).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace edigpu {

constexpr int kPairsMaxTerms = 8;
constexpr uint32_t kPairsNone = 0xFFFFFFFFu;

struct PairsOp {
  int create, iorb, ispin;  // create > 0: c^+, else c; ispin 0 = up, 1 = down
};
struct PairsTerm {
  double coef;
  PairsOp o1, o2;  // o1 acts first
};

// The sector O2 O1 leads to from (nup, ndw); exists = false when a particle number leaves [0, ns] on the way (the
// reference's getCsector / getCDGsector returning 0): nup, ndw then hold the numbers reached, which need not be valid.
struct PairsDest {
  int nup, ndw;
  bool exists;
};
PairsDest pairs_destination(int nup, int ndw, int ns, const PairsTerm& t);

// number of ns-bit words with n bits set; 0 outside 0 <= n <= ns
int64_t pairs_dim(int ns, int n);
// position of a word in the ascending list of the words of its popcount
int64_t pairs_rank(uint32_t word);

// Table of one species (spin) of one term over the destination's index of that species: tab[j] = preimage of the j-th
// destination word under the term's operators of that spin, n_dst = the species' particle number in the destination.
// Returns true when the term has no operator of that spin: the species is the identity and tab is left empty.
bool pairs_species_table(int ns, int n_dst, const PairsTerm& t, int spin, std::vector<uint32_t>& tab);

// Everything a call needs: tables [nterms][dim_up_dst] and [nterms][dim_dw_dst] (the slots of identity species are not
// read and hold kPairsNone), identity flags as bit masks over the terms.
struct PairsTables {
  int nterms = 0, nup_dst = 0, ndw_dst = 0;
  int64_t dim_up_src = 0, dim_dw_src = 0, dim_up_dst = 0, dim_dw_dst = 0;
  double coef[kPairsMaxTerms] = {0};
  uint32_t id_up = 0, id_dw = 0;
  std::vector<uint32_t> up, dw;
};
// checks only: "" and the common destination, or the reason for refusing (orbital / spin out of range, nterms outside
// 1 .. kPairsMaxTerms, terms that lead to different destinations).  exists = false when some term leaves the Fock space.
std::string pairs_check(int nup, int ndw, int ns, int norb, int nterms, const PairsTerm* terms, PairsDest& dest);
// pairs_check, then the tables; a call whose destination does not exist is refused
std::string pairs_build(int nup, int ndw, int ns, int norb, int nterms, const PairsTerm* terms, PairsTables& out);

}  // namespace edigpu
