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

// ---- a rank's elements [first, first + count) of the sector (edigpu_imp_rdm_flat_sharded) ----
// The ranges are those of edigpu_shard_plan over the elements: q = ceil(dim_el / world) per rank, rank r starts at
// min(r q, dim_el).  A SLAB is the 2^norb rows of one bath word down: a contiguous range of elements, which a rank
// boundary cuts anywhere.  The rank in whose range a (non-empty) slab STARTS owns it:
//   interior slabs lie wholly inside the range and are walked on the caller's shard in place: `in` is rdm_flat_plan with
//            the bdw lists filtered to them, row starts relative to `first`, block stride `count`; with first = 0, count =
//            dim_el it IS rdm_flat_plan;
//   the head is the elements from `first` up to the first slab start inside the range (the whole range when no slab
//            starts there): elements of a slab an earlier rank owns.  Every rank computes every rank's head, so the halo
//            size H = max_r head(r) < the longest slab is known everywhere; a rank sends its head of every block, padded to H;
//   the tail slab starts inside the range and ends beyond it: its owner copies its own last elements and the heads of the
//            following ranks, in rank order (more than one rank when q < the slab's length), into a buffer of one slab per
//            block, which the tiles kernel walks with the work list `slab`: rdm_flat_plan of that one bath word with row
//            starts relative to the slab, block stride tail_len.
// One table of segments describes a copy, for the halo (pack) and for the slab (fill) alike: len elements to dst of a
// block of the destination from
struct RdmFlatSeg {
  int32_t sel = 0;   // 0: zeros, 1: src of the shard's block, 2: src of rank's halo block
  int32_t rank = 0;
  int64_t src = 0, dst = 0, len = 0;
};
struct RdmFlatShardPlan {
  int world = 1, rank = 0;              // rank: -1 for a range that holds no element
  int64_t first = 0, count = 0, q = 0;  // the range cut to the sector
  int64_t H = 0;                        // elements of a rank's halo (the same on every rank)
  std::vector<int64_t> heads;           // [world]
  int64_t nslab_in = 0;                 // slabs walked in place
  int64_t tail_start = -1, tail_len = 0, tail_own = 0;  // the slab this rank owns across its end: first element relative to
  int32_t tail_bdw = -1;                                // `first`, length, elements held here, bath word; tail_len = 0: none
  std::vector<RdmFlatSeg> pack, fill;   // the halo this rank sends (H elements), the slab (tail_len elements)
  RdmFlatPlan in, slab;                 // work lists of the interior slabs and of the tail slab; their partial sums share
  std::vector<RdmGroup> groups;         // one buffer: per group the workgroups of `in`, then those of `slab`
  int64_t partial_entries = 0;
};
// "" on success; a message when (first, count) is not a rank's range of edigpu_shard_plan for `world` ranks
std::string rdm_flat_shard_plan(const RdmFlatTables& t, int nblk, int cw, int target_wgs, int world, int64_t first,
                                int64_t count, RdmFlatShardPlan& p);
// The segment-copy kernel restated (kernels_rdm_flat.hip rdm_flat_seg_kernel), every index checked: dst[nblk][dlen] (cw
// doubles per element) of one vector from the shard v[nblk][count] (null when count = 0) and the gathered halos
// [world][nblk][H] (null for the pack); a halo element past its rank's head is a violation, and so is a destination
// element written twice or never.
std::string rdm_flat_segs_emulate(const RdmFlatShardPlan& p, const std::vector<RdmFlatSeg>& segs, int64_t dlen, int nblk, int cw,
                                  const double* v, const double* halos, double* dst);
// The two tile launches and the final sums restated as rdm_flat_plan_emulate does: `in` on the shard, `slab` on the
// buffer [nblk][tail_len] (null when tail_len = 0), tri = this rank's packed sums.
std::string rdm_flat_shard_emulate(const RdmFlatShardPlan& p, int64_t ntri, int nblk, const double* v_shard, const double* slab,
                                   int cw, double* tri);
// A whole world on the host: every rank's plan, pack, the all-gather, fill and launches on its shard of v[nblk][dim_el];
// tri = the ranks' sums added in rank order; *H_out = the halo.  Checks on the way that every rank computes the same
// heads, that every non-empty slab has one owner and that every element of the sector is read exactly once.
std::string rdm_flat_world_emulate(const RdmFlatTables& t, int nblk, int cw, int target_wgs, int world, const double* v,
                                   double* tri, int64_t* H_out);

}  // namespace edigpu
