// host_rdm.hpp -- host tables of the impurity reduced density matrix (edigpu_imp_rdm).  No HIP in here:
// tests/host_rdm.cpp and tests/host_rdm_shard.cpp compile this with g++.
//
// rho_imp = Tr_bath |v><v| of a normal-mode (ed_total_ud=T) sector, imp_rdm_normal (ED_RDM_NORMAL.f90:146-209).  A spin
// word is I + 2^norb B (I: impurity pattern, B: bath pattern) and both sector maps ascend, so an index range of one spin
// splits into contiguous RUNS of equal B; a run of impurity particle number k = N_spin - popcount(B) lists the C(norb, k)
// patterns of that number in ascending order.  The vector [dim_dw][dim_up] is therefore tiled into dense Lu x Ld tiles,
// one per (Bup, Bdw), and rho is the sum over tiles of x x^H, x = the flattened tile, which lands in the block (ku, kd)
// of a block-diagonal matrix.  These tables describe the runs, the rank <-> pattern maps, the packed result (the upper
// triangles of the blocks), its placement into the dense 4^norb x 4^norb matrix, and the work list the kernel walks.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace edigpu {

constexpr int kRdmMaxOrb = 5;          // == EDIGPU_MAXORB
constexpr int kRdmMaxRun = 10;         // C(5, 2): the longest run
constexpr int kRdmThreads = 256;       // threads of a workgroup of the tiles kernel
constexpr int kRdmStageElems = 2048;   // elements of a staged slab: the rows of one down run x the columns of one chunk
constexpr int kRdmAccBytes = 48 << 10; // accumulators of one workgroup; a larger down class is split by up class

// rank <-> pattern per particle number: pat_of[k][r] = the r-th pattern (ascending) of k particles on norb orbitals
struct RdmRanks {
  int norb = 0;
  int nk[kRdmMaxOrb + 1] = {0};  // C(norb, k)
  uint8_t pat_of[kRdmMaxOrb + 1][kRdmMaxRun] = {{0}};
  uint8_t rank_of[1 << kRdmMaxOrb] = {0};
};
void rdm_rank_tables(int norb, RdmRanks& r);

// runs of one sector map: start[j] .. start[j + 1] = the indices of run j (nrun + 1 entries), k[j] its particle number
struct RdmRuns {
  std::vector<int32_t> start;
  std::vector<uint8_t> k;
};
// "" on success; a message when the map does not have the structure above (not ascending, a run that is not the
// complete ascending list of its particle number)
std::string rdm_runs(const int32_t* map, int64_t n, int norb, const RdmRanks& rk, RdmRuns& out);

// packed result: per class (ku, kd) the upper triangle (p <= q, row-major) of an n x n block, n = nk[ku] nk[kd], the
// flattened tile index is p = ru + nk[ku] rd.  Classes are laid out kd-major so that one down class is one range.
struct RdmLayout {
  int norb = 0;
  int64_t tri_off[kRdmMaxOrb + 1][kRdmMaxOrb + 1] = {{0}};  // [ku][kd]
  int64_t ntri = 0;
};
void rdm_layout(const RdmRanks& rk, RdmLayout& l);
inline int64_t rdm_tri_index(int n, int p, int q) { return (int64_t)p * n - (int64_t)p * (p - 1) / 2 + (q - p); }
inline int64_t rdm_tri_size(int n) { return (int64_t)n * (n + 1) / 2; }
// tri (ntri entries of cw doubles) -> dense[D][D] (cw doubles each), D = 4^norb, io = Iup + 2^norb Idw: the triangle is
// mirrored (conjugated for cw == 2), everything outside the blocks is 0
void rdm_place(const RdmRanks& rk, const RdmLayout& l, const double* tri, int cw, double* dense);

// The specification of the kernel: a plain loop over the tiles of nblk (phonon) blocks of [dim_dw][dim_up] elements of
// cw doubles (2: interleaved complex), tri[class][p <= q] += x_p conj(x_q); tri must hold ntri * cw zeros.
void rdm_host_reference(const RdmRanks& rk, const RdmLayout& l, const RdmRuns& up, const RdmRuns& dw, int64_t dim_up,
                        int64_t dim_dw, int nblk, const double* v, int cw, double* tri);

// ---- what the device walks (kernels_rdm.hip) ----
// One workgroup: the down runs [j0, j1) of one down class (row of run j: rows[row_list + j % nruns] + (j / nruns) dim_dw),
// the columns [c0, c0 + clen) of one chunk (chunks end on run boundaries), the entries [e0, e1) of the packed result.
// rel[rel0 + kb[ku] .. rel0 + kb[ku + 1]) = the starts, relative to c0, of the chunk's up runs of class ku.
struct RdmWork {
  int32_t row_list, nruns, j0, j1, ld, c0, clen, rel0, e0, e1;
  int32_t kb[kRdmMaxOrb + 2];
  int32_t pad;
  int64_t pofs;  // of this workgroup's e1 - e0 partial sums, in entries
};
// the workgroups that add into the entries [e0, e1): nwg consecutive blocks of e1 - e0 partial sums from pbase
struct RdmGroup {
  int32_t e0, e1, nwg, pad;
  int64_t pbase;
};
struct RdmPlan {
  int stride = 0;             // of a staged row, in elements
  int ld_max = 0, ept_max = 0, rel_max = 0;  // sizes of the LDS areas: rows staged, entries per thread, runs per chunk
  int64_t partial_entries = 0;               // of one vector
  std::vector<int32_t> rows;  // starts of the down runs, grouped by class
  std::vector<uint16_t> rel;
  std::vector<uint32_t> ent;  // per packed entry: ku | ru_p << 4 | rd_p << 8 | ru_q << 12 | rd_q << 16
  std::vector<RdmWork> work;
  std::vector<RdmGroup> groups;
};
// target_wgs: workgroups wanted for one vector (the device's width); cw enters through the accumulators' size only
void rdm_plan(const RdmRanks& rk, const RdmLayout& l, const RdmRuns& up, const RdmRuns& dw, int64_t dim_up, int64_t dim_dw,
              int nblk, int cw, int target_wgs, RdmPlan& p);
// The kernels restated on the host, index for index (staging, per-thread entries, partial sums, final sums), with every
// index checked against the sizes of what it reads or writes: "" on success, else the first violation.
std::string rdm_plan_emulate(const RdmPlan& p, int64_t ntri, int64_t nel, int64_t dim_up, int64_t dim_dw, const double* v,
                             int cw, double* tri);

// ---- a rank's down rows [first, first + count) of the sector (edigpu_imp_rdm_sharded) ----
// The ranges are those of edigpu_shard_plan: q = ceil(dim_dw / world) rows per rank, rank r starts at min(r q, dim_dw).
// A tile needs the whole down run of its bath word, and a rank boundary can cut a run.  The rank in whose range a run
// STARTS owns it:
//   interior runs lie wholly inside the range and are walked on the caller's shard in place (starts relative to `first`,
//            block stride `count`); with first = 0, count = dim_dw they are the runs of the sector and `in` is rdm_plan's;
//   the head is the rows from `first` up to the first run start inside the range (the whole range when no run starts
//            there): rows of a run an earlier rank owns.  Every rank computes every rank's head, so the halo size
//            H = max_r head(r) <= kRdmMaxRun - 1 is known everywhere; a rank sends its head rows of every block, padded to H;
//   the tail run starts inside the range and ends beyond it: its owner copies its own last rows and the head rows of
//            the following ranks, in rank order (more than one rank when q < the run's length), into a slab of one run per
//            block, which the tiles kernel walks with the work list `slab`.
// One table of row sources describes a copy of rows, for the halo (pack) and for the slab alike:
struct RdmRowCopy {
  int32_t nrows = 0;                    // rows of one block of the destination
  int8_t sel[kRdmMaxRun] = {0};         // 0: zeros, 1: row[] of the shard's block, 2: row[] of rank[]'s halo
  int32_t rank[kRdmMaxRun] = {0};
  int32_t row[kRdmMaxRun] = {0};
};
struct RdmShardPlan {
  int world = 1, rank = 0;              // rank: -1 for a range that holds no row
  int64_t first = 0, count = 0, q = 0;  // the range cut to the sector
  int H = 0;                            // rows of a rank's halo (the same on every rank)
  std::vector<int32_t> heads;           // [world]
  int32_t tail_row = 0, tail_own = 0, tail_ld = 0, tail_k = -1;  // the run this rank owns across its end: first row
                                        // relative to `first`, rows held here, length, class; tail_ld = 0: none
  RdmRowCopy pack, fill;                // the halo this rank sends (H rows), the slab (tail_ld rows)
  RdmPlan in, slab;                     // work lists of the interior runs and of the slab; their partial sums share one
  std::vector<RdmGroup> groups;         // buffer: per group the workgroups of `in`, then those of `slab`
  int64_t partial_entries = 0;
};
// "" on success; a message when (first, count) is not a rank's range of edigpu_shard_plan for `world` ranks
std::string rdm_shard_plan(const RdmRanks& rk, const RdmLayout& l, const RdmRuns& up, const RdmRuns& dw, int64_t dim_up,
                           int64_t dim_dw, int nblk, int cw, int target_wgs, int world, int64_t first, int64_t count,
                           RdmShardPlan& p);
// The row-copy kernel restated (kernels_rdm.hip rdm_rows_kernel), every index checked: dst[nblk][t.nrows][rowlen] of one
// vector from the shard v[nblk][count][rowlen] (null when count = 0) and the gathered halos [world][nblk][H][rowlen]
// (null for the pack); a halo row past its rank's head is a violation.
std::string rdm_rows_emulate(const RdmShardPlan& p, const RdmRowCopy& t, int nblk, int64_t rowlen, const double* v,
                             const double* halos, double* dst);
// The two tile launches and the final sums restated on the host as rdm_plan_emulate does: `in` on the shard, `slab`
// on the slab [nblk][tail_ld][dim_up] (null when tail_ld = 0), tri = this rank's packed sums.
std::string rdm_shard_emulate(const RdmShardPlan& p, int64_t ntri, int64_t dim_up, int nblk, const double* v_shard,
                              const double* slab, int cw, double* tri);

}  // namespace edigpu
