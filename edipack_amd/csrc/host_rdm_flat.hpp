// host_rdm_flat.hpp -- host tables of the impurity reduced density matrix of superc / nonsu2 sectors
// (edigpu_imp_rdm_flat).  No HIP in here: tests/host_rdm_flat.cpp compiles this with g++.
//
// rho_imp = Tr_bath |v><v| of imp_rdm_superc (ED_RDM_SUPERC.f90:54-183) and imp_rdm_nonsu2 (ED_RDM_NONSU2.f90:54-188).  A
// state of the sector map is iup + 2^ns idw, iup = Iup + 2^norb Bup, idw = Idw + 2^norb Bdw; the map ascends, so it is idw
// outer, iup inner: the elements of one idw are a contiguous ROW, which lists all up words of one particle number
// nup(popcount(idw)) (nonsu2: Ntot - popcount, superc: Sz + popcount) in ascending order -- a normal-mode up map, with the
// runs of host_rdm.hpp.  The 2^norb rows Idw of one Bdw are consecutive rows; a TILE (Bup, Bdw) is the run of Bup in each of
// them, x = the tile in io = Iup + 2^norb Idw order, and rho += (s x)(s x)^H with s_p = -1 iff popcount(Bup) and
// popcount(Idw_p) are both odd.  A tile lands in ONE block of a block-diagonal matrix: class c = ku + kd (nonsu2) or
// ku - kd + norb (superc), ku / kd the impurity particle numbers, of C(2 norb, c) members.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "host_rdm.hpp"

namespace edigpu {

constexpr int kRdmFlatMaxOrb = 4;         // a block of five orbitals (252 x 252) does not fit the accumulators
constexpr int kRdmFlatRows = 16;          // 2^kRdmFlatMaxOrb rows of a slab
constexpr int kRdmFlatMaxBlock = 70;      // C(8, 4)
constexpr int kRdmFlatClasses = 2 * kRdmFlatMaxOrb + 1;
constexpr int kRdmFlatThreads = 256;      // threads of a workgroup of the tiles kernel
constexpr int kRdmFlatStageElems = 2048;  // elements of a staged slab: the tiles of one chunk of bath words up
constexpr int kRdmFlatAccBytes = 48 << 10;  // accumulators of one workgroup; more classes than fit are split
constexpr uint16_t kRdmFlatNoRun = 0x7fff;  // rel entry of a row that has no run of the tile

struct RdmFlatTables {
  int ns = 0, norb = 0, mode = 0, q = 0;  // mode: 1 superc (q = Sz), 2 nonsu2 (q = Ntot)
  RdmRanks ranks;
  int64_t dim_el = 0;
  int nup_of[33] = {0};                    // up particle number of a row by popcount(idw); -1: the row is absent
  std::vector<int64_t> rowstart;           // [2^ns + 1]
  std::vector<std::vector<int32_t>> run_of;  // [nup][Bup]: start of the run of Bup in a row of nup particles, -1: none
  // packed result: per class the upper triangle (p <= q, row-major) of an n x n block
  int nclass = 0;
  int bn[kRdmFlatClasses] = {0};
  uint8_t member[kRdmFlatClasses][kRdmFlatMaxBlock] = {{0}};  // io of member p: Idw ascending, Iup ascending inside
  int64_t tri_off[kRdmFlatClasses + 1] = {0};
  int64_t ntri = 0;
  // impurity up particle number of a member of class c with kd down particles (may be out of range)
  int ku_of(int c, int kd) const { return mode == 2 ? c - kd : c - norb + kd; }
  int nup_row(int popcount_idw) const { return mode == 2 ? q - popcount_idw : q + popcount_idw; }
};
// "" on success; a message when the arguments are out of range or the map does not have the structure above
std::string rdm_flat_tables(const int32_t* map, int64_t n, int ns, int norb, int mode, int q, RdmFlatTables& t);

// tri (ntri entries of cw doubles) -> dense[D][D]: mirrored (conjugated for cw == 2), 0 outside the blocks
void rdm_flat_place(const RdmFlatTables& t, const double* tri, int cw, double* dense);
double rdm_flat_trace(const RdmFlatTables& t, const double* tri, int cw);

// The specification of the kernel: a plain loop over the tiles of nblk (phonon) blocks of dim_el elements of cw doubles;
// tri must hold ntri * cw zeros.
void rdm_flat_host_reference(const RdmFlatTables& t, int nblk, const double* v, int cw, double* tri);

// ---- what the device walks (kernels_rdm_flat.hip) ----
// A panel: the slabs of one popcount of Bdw x one chunk of bath words up.  Of row Idw (kd = popcount(Idw)) the elements
// [seg[kd], seg[kd] + len[kd]) are staged at soff[Idw]; tile i of the panel (sorted by class, kb[c] .. kb[c + 1]) has its
// run in such a row at rel[rel0 + kd * ntile + i] & 0x7fff of the staged segment, bit 15 = popcount(Bup) is odd.
struct RdmFlatPanel {
  int32_t seg[kRdmFlatMaxOrb + 1], len[kRdmFlatMaxOrb + 1];
  int32_t soff[kRdmFlatRows];
  int32_t kb[kRdmFlatClasses + 1];
  int32_t total, ntile, rel0, bdw0, nbdw, pad;
};
// One workgroup: the slabs j in [j0, j1) of a panel (Bdw = bdw[bdw0 + j % nbdw], phonon block j / nbdw), the packed
// entries [e0, e1) (whole classes).
struct RdmFlatWork {
  int32_t panel, j0, j1, e0, e1, pad;
  int64_t pofs;  // of this workgroup's e1 - e0 partial sums, in entries
};
struct RdmFlatPlan {
  int norb = 0;
  int64_t dim_el = 0;
  int stage_max = 0, ept_max = 0, rel_max = 0;  // sizes of the LDS areas: elements staged, entries per thread, rel words
  int64_t partial_entries = 0;                  // of one vector
  std::vector<int64_t> rowstart;
  std::vector<int32_t> bdw;    // the bath words down, grouped by popcount
  std::vector<uint16_t> rel;
  // per packed entry: c | Idw_p << 4 | rank_p << 8 | Idw_q << 11 | rank_q << 15 | sign parity << 18 | kd_p << 19 | kd_q << 22
  std::vector<uint32_t> ent;
  std::vector<RdmFlatPanel> panels;
  std::vector<RdmFlatWork> work;
  std::vector<RdmGroup> groups;
};
void rdm_flat_plan(const RdmFlatTables& t, int nblk, int cw, int target_wgs, RdmFlatPlan& p);
// The kernels restated on the host, index for index, with every index checked against the sizes of what it reads or
// writes: "" on success, else the first violation.  nel = elements of the vector (nblk * dim_el).
std::string rdm_flat_plan_emulate(const RdmFlatPlan& p, int64_t ntri, int64_t nel, const double* v, int cw, double* tri);

}  // namespace edigpu
