// edigpu_internal.hpp -- internal types of the gfx950 H*v engine (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/edigpu.h"
#include "host_build.hpp"
#include "shard_src.hpp"
#include "switches.hpp"

namespace edigpu {

// What a handle is (the values are part of the ABI: edigpu_info hands them out): normal mode (Kronecker), superc / nonsu2
// stored as flat CSR / SELL, the same on the fly, ed_total_ud = F, _CMPLX_NORMAL (H = S + iA over real sub-handles).
enum SectorKind : int { kNormal = 0, kFlat = 1, kDirect = 2, kOrbs = 3, kCmplxNormal = 4 };

// the calling thread's error string (edigpu_last_error) and current device (edigpu_init): edigpu_capi.hip
void set_error(const std::string& msg);
#pragma GCC visibility push(hidden)
bool have_error();
int current_device();
// 0 when a HIP device is usable, else 1 with the message set
int ensure_device(int* count_out = nullptr);
#pragma GCC visibility pop

#define EDIGPU_HIP(call)                                                                     \
  do {                                                                                       \
    hipError_t _e = (call);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      ::edigpu::set_error(std::string(#call) + " failed: " + hipGetErrorString(_e) + " (" +  \
                          __FILE__ + ":" + std::to_string(__LINE__) + ")");                  \
      return 1;                                                                              \
    }                                                                                        \
  } while (0)

// device CSR with 32-bit or 64-bit row pointers (64-bit only when nnz >= 2^31)
struct DevCsr {
  int64_t nrow = 0, nnz = 0;
  int wide = 0;             // 1: rowptr64 used
  int32_t* rowptr32 = nullptr;
  int64_t* rowptr64 = nullptr;
  int32_t* col = nullptr;
  double* val = nullptr;    // nnz (real) or 2*nnz (complex)
  double avg_row = 0.0;
  // SELL-64 image (sliced ELL, 64 rows per slice, entries sorted by column inside a row):
  // entry (slice s, slot k, lane l) at sell_ptr[s]*64 + k*64 + l; padding = own row, value 0
  int sell = 0;
  int64_t nslice = 0;
  int32_t* sell_ptr = nullptr;   // nslice+1, in units of 64 entries
  int32_t* sell_col = nullptr;
  double* sell_val = nullptr;
  // value-dictionary form of the SELL image: 4 B/entry = column (24 bit) | id (8 bit), values in a
  // <= 256-entry table (id 0 = 0.0), diagonal kept apart (one value per row, loc block only)
  int sell_packed = 0;
  uint32_t* sell_pk = nullptr;
  double* sell_dict = nullptr;
  double* sell_diag = nullptr;
};

// ed_total_ud = F ("orbs") sector: kernel argument block (kernels_orbs.hip); all pointers are device memory
constexpr int kOrbsMaxAxes = 2 * EDIGPU_MAXORB;
struct OrbsArgs {
  int naxes = 0;
  int64_t dim = 0;
  int64_t dims[kOrbsMaxAxes] = {0};
  int64_t stride[kOrbsMaxAxes] = {0};
  int off[kOrbsMaxAxes] = {0};        // offset of axis k inside eax / impbit
  int width[kOrbsMaxAxes] = {0};      // ELL width of factor k
  int64_t elloff[kOrbsMaxAxes] = {0};  // offset of factor k inside ell_col / ell_val ([slot][row])
  const int32_t* ell_col = nullptr;
  const double* ell_val = nullptr;
  const double* hd = nullptr;         // explicit diagonal (hand-over) or null: factored tables below
  const double* eax = nullptr;
  const uint8_t* impbit = nullptr;
  const double* xtab = nullptr;
};

// ELL (column-major [slot][row]) image of a small square factor matrix
struct DevEll {
  int64_t nrow = 0, pitch = 0;
  int width = 0;
  int typed = 0;            // packed image with one hop amplitude per slot (coef[k])
  // packed image (preferred): 24-bit column | 7-bit coefficient id | sign; coef[128] table
  uint32_t* pk = nullptr;
  double* coef = nullptr;
  // typed LDS image of a row of at most 4095 columns, beside pk: 16-bit entries (15-bit byte offset | sign << 15), two
  // consecutive slots of a column per word, (width + 1) / 2 * pitch16 words (upload_ell).  Odd nrow: words in column
  // order, pitch16 = pitch; even nrow: in the order in which the rows kernel's threads own the columns
  // (host_pack.hpp: ell16_owned_col), pitch16 = nrow rounded up to 256
  uint32_t* pk16 = nullptr;
  int64_t pitch16 = 0;
  // plain image (fallback when > 127 distinct |values| or nrow >= 2^24)
  int32_t* col = nullptr;   // width*pitch, padding: col=row, val=0
  double* val = nullptr;
};

// Impurity-block image of a whole normal-mode sector on the device (host_ib.hpp; kernels_ib.hip).  Vectors of the
// device-resident Lanczos loops live in the padded panel layout: element (idw, iup) at
// (pos[iup] / 16) * ps + idw * 16 + pos[iup] % 16, ps = dim_dw * 16, len = npanels * ps doubles, padding = zeros.
struct IbDevHalf {  // rows kernel's tables of one half of a split row (host_ib.hpp IbUpHalf)
  int panel0 = 0, npanels = 0, nlist = 0, rimg_len = 0;
  int ucls[5] = {0, 0, 0, 0, 0}, rcb[5] = {0, 0, 0, 0, 0}, rcs[5] = {0, 0, 0, 0, 0};
  uint16_t *ublist = nullptr, *utop = nullptr;
  uint32_t* rmap2 = nullptr;
};

// local-block tables on the same vector layout (host_sb.hpp, kernels_sb.hip; round 4): when present, the product and
// the fused Lanczos step of the impurity-block image run on these
struct DevSb {
  int nb0 = 0, nloc = 0, amode = 0, nbw_up = 0, nbw_dw = 0;
  int rows_nt = 0, rows_nbt = 0, rimg_len = 0, rcs = 0;
  size_t rows_lds = 0, cols_lds = 0;
  uint16_t *urank = nullptr, *ublist = nullptr;
  double* ebw = nullptr;
  int32_t* uslot = nullptr;
  uint32_t* rmap2 = nullptr;
  double *up_vtab = nullptr, *up_tloc = nullptr, *e0 = nullptr;
  uint32_t* up_korb = nullptr;
  int lowbits = 0, nchunks = 0, max_chunk_rows = 0, max_chunk_slots = 0, cols_gs = 8;
  int32_t *chunk_row = nullptr, *chunk_slot = nullptr, *cdesc_off = nullptr;
  uint8_t* cdesc = nullptr;
  double *dw_vtab = nullptr, *dw_tloc = nullptr;
  uint32_t* dw_korb = nullptr;
  uint32_t* nd_dw = nullptr;
  // rows staged in halves (host_sb.hpp SbUpHalf): nhalf = 2; urank then ranks the LOW words, ublist / uslot / rmap2 / ebw of the
  // whole row are absent and rows_lds, rimg_len, rows_nt / rows_nbt serve both halves; the columns kernel of such a sector is
  // the impurity-block one
  int nhalf = 1;
  struct Half {
    int panel0 = 0, npanels = 0;
    uint32_t* ublist32 = nullptr;  // low word | skip | partner position over the top level << 16
    uint8_t* ugap = nullptr;
    int32_t* uslot = nullptr;
    uint32_t* rmap2 = nullptr;
    double* ebw = nullptr;
  } half[2];
};

struct IbDev {
  DevSb* sb = nullptr;
  int nhalf = 1;                 // 2: rows longer than the LDS, staged one half (value of the top bath bit) at a time
  OptInt cols2;                  // Switches::ib_cols2 at set-up: the form of the columns kernel, when set (kernels_ib.hip use_cols2)
  IbDevHalf half[2];
  uint16_t* urank_low = nullptr; // [2^(nb_up - 1)]
  double top_eps = 0.0;          // energy of the top bath level of the up species
  int norb = 0, nb_up = 0, nb_dw = 0, npanels = 0, plen = 0, nlist = 0;
  int ucls[5] = {0, 0, 0, 0, 0};
  int lowbits = 0, nchunks = 0, max_chunk_rows = 0, max_chunk_blocks = 0, nterms = 0, nsub = 1;
  int64_t dim_up = 0, dim_dw = 0, ps = 0, len = 0;
  int rows_nt = 0, rows_nbt = 0;      // rows kernel: threads per workgroup, blocks per thread
  size_t rows_lds = 0, cols_lds = 0;  // dynamic LDS of the two kernels
  uint16_t *urank = nullptr, *ublist = nullptr;  // rows kernel: rank of a bath word inside its class; block list
  uint32_t* rmap2 = nullptr;                     // [plen / 2]: image words of a pair of adjacent positions (lo | hi << 16)
  int rcb[5] = {0, 0, 0, 0, 0}, rcs[5] = {0, 0, 0, 0, 0}, rimg_len = 0;
  double *up_vtab = nullptr, *up_timp = nullptr, *up_ebath = nullptr, *xu = nullptr, *ed = nullptr;
  uint8_t* impd = nullptr;
  int32_t *pos = nullptr, *colof = nullptr;  // column -> position, position -> column (-1: padding)
  int32_t *chunk_row = nullptr, *chunk_blk = nullptr, *dcls = nullptr;
  uint16_t *dblist = nullptr, *dmeta = nullptr;
  double *dw_vtab = nullptr, *dw_timp = nullptr, *ndcoef = nullptr;
  uint8_t *nd_dw = nullptr, *nd_up = nullptr;
  // short rows: the generic LDS row kernel in position order (kernels_normal.hip launch_normal_rows_pos) takes the rows half of
  // the product and of the fused step; Hup as ELL over positions, the diagonal table [impurity pattern of the down word][plen]
  struct PosRows {
    bool on = false;
    DevEll ell;
    double* eux = nullptr;
    int td = 0;  // rows per workgroup
  } pr;
  // bath-bath hops (host_ib.hpp IbSide::pmask, pt): replica / general baths
  int up_np = 0, dw_np = 0;
  uint32_t *up_pmask = nullptr, *dw_pmask = nullptr;
  double *up_pt = nullptr, *dw_pt = nullptr;
};

// Occupation tables of a library-built whole sector (host_occ.hpp; kernels_occ.hip), made and uploaded by the first
// edigpu_apply_occ / edigpu_occ_moments on the handle and kept until edigpu_destroy.  Normal mode: pu[dim_up], the down
// patterns are edigpu_sector::d_impd where the sector has it (pd stays null), order = the rows sorted by down pattern;
// superc / nonsu2: pu[electronic rows] = up | down << norb.
struct OccDev {
  int norb = 0, flat = 0, nblk = 1, ncu = 0;
  int64_t dim_up = 0, dim_dw = 1;
  int64_t first = 0, count = 0;  // shard view (edigpu_sector::occ_shard): the rows it was built for
  uint16_t* pu = nullptr;
  uint8_t* pd = nullptr;
  int32_t* order = nullptr;
  int32_t run[33] = {0};
  double *partial = nullptr, *sums = nullptr;  // edigpu_occ_moments: the waves' partial sums, the vectors' sums
  int64_t partial_cap = 0, sums_cap = 0;       // in doubles
};
void free_occ(edigpu_sector* s);
// The shard view of the same tables (edigpu_sector::occ_shard; host_occ.hpp occ_shard_view): the rows [first, first +
// count) of the sector -- down rows of normal mode, rows of superc / nonsu2 -- with their own down patterns (never
// edigpu_sector::d_impd) and row order, indices local to the shard.  Built by the first sharded call, rebuilt when the
// range changes.  occ_shard_moments leaves the nvec x kOccSums sums of this rank's rows in *sums_dev on the handle's
// stream; occ_shard_apply enqueues the product there.  Neither launches anything for count == 0 (*sums_dev = null).
int occ_shard_moments(edigpu_sector* s, int64_t first, int64_t count, const double* v_dev, int nvec, const double** sums_dev,
                      const std::string& who);
int occ_shard_apply(edigpu_sector* s, int64_t first, int64_t count, const double* src_dev, double* dst_dev, const double* w_up,
                    const double* w_dw, const std::string& who);
// device bytes of the tables above (made lazily, so the sector cache adds them to what it measured at build time)
int64_t occ_table_bytes(const edigpu_sector* s);
// the three refusals the occupation entry points share (ed_total_ud=F, hand-over handle, shard): 1 with the message set
int occ_refuse(const edigpu_sector* s, const std::string& who);
// the first two of them: what the sharded twins refuse as well
int occ_refuse_kind(const edigpu_sector* s, const std::string& who);

// Tables and workspace of edigpu_imp_rdm on a library-built whole normal-mode sector (host_rdm.hpp; kernels_rdm.hip),
// made and uploaded by the first call on the handle and kept until edigpu_destroy.
struct RdmDev;
void free_rdm(edigpu_sector* s);
// device bytes of those tables (made lazily: the sector cache adds them like occ_table_bytes)
int64_t rdm_table_bytes(const edigpu_sector* s);
// The same on the down rows [first, first + count) of the sector, one of `world` ranges of edigpu_shard_plan
// (edigpu_sector::rdm_shard; host_rdm.hpp RdmShardPlan), kept like the occupation tables' shard view and built on every
// rank, rows or not.  A run of down rows a rank boundary cuts belongs to the rank it starts on: every rank sends its first
// H rows (rdm_shard_pack: nvec x nblk x H x DimUp x cw doubles, zero-padded), and rdm_shard_enqueue fills the owner's slab
// (nvec x nblk x tail_ld x DimUp x cw doubles) from the gathered halos, runs the tiles kernel on the shard in place and
// on the slab, and leaves the nvec x ntri x cw packed sums of this rank in *tri_dev, all on the handle's stream.
struct RdmShardDev;
struct RdmShardInfo {
  int H = 0, tail_ld = 0, cw = 1;
  int64_t ntri = 0;
};
// the refusals that need no communicator: ed_total_ud=F, hand-over handle, superc / nonsu2, norb
int rdm_shard_refuse(const edigpu_sector* s, const std::string& who);
int rdm_shard_prepare(edigpu_sector* s, int64_t first, int64_t count, int world, const std::string& who, RdmShardInfo* info);
int rdm_shard_pack(edigpu_sector* s, const double* v_dev, int nvec, double* send_dev);
int rdm_shard_enqueue(edigpu_sector* s, const double* v_dev, int nvec, const double* halos_dev, double* slab_dev,
                      const double** tri_dev);
// the summed packed triangles -> nvec dense matrices and traces, as edigpu_imp_rdm returns them
void rdm_shard_expand(const edigpu_sector* s, const double* tri, int nvec, double* rdm_host, double* norm2_host);

// The same of edigpu_imp_rdm_flat on a library-built whole superc / nonsu2 sector (host_rdm_flat.hpp; kernels_rdm_flat.hip).
struct RdmFlatDev;
void free_rdm_flat(edigpu_sector* s);
// The same on the elements [first, first + count) of the sector, one of `world` ranges of edigpu_shard_plan over the
// electronic dimension (edigpu_sector::rdm_flat_shard; host_rdm_flat.hpp RdmFlatShardPlan), kept like rdm_shard, built on
// every rank, elements or not, and freed by free_rdm_flat.  A slab -- the rows of one bath word down -- that a rank boundary
// cuts belongs to the rank it starts on: every rank sends its first H elements (rdm_flat_shard_pack: nvec x nblk x H x cw
// doubles, zero-padded), and rdm_flat_shard_enqueue fills the owner's slab (nvec x nblk x tail_len x cw doubles) from the
// gathered halos, runs the tiles kernel on the shard in place and on the slab, and leaves the nvec x ntri x cw packed
// sums of this rank in *tri_dev, all on the handle's stream.
struct RdmFlatShardDev;
struct RdmFlatShardInfo {
  int64_t H = 0, nslab_in = 0, tail_start = -1, tail_len = 0, tail_own = 0, ntri = 0;
  int cw = 1;
};
// the refusals that need no communicator: ed_total_ud=F, hand-over handle, normal mode, Jz_basis, Norb = 5
int rdm_flat_shard_refuse(const edigpu_sector* s, const std::string& who);
// the geometry alone, from host tables made for the call: touches no device and keeps nothing
int rdm_flat_shard_info(const edigpu_sector* s, int64_t first, int64_t count, int world, const std::string& who,
                        RdmFlatShardInfo* info);
int rdm_flat_shard_prepare(edigpu_sector* s, int64_t first, int64_t count, int world, const std::string& who,
                           RdmFlatShardInfo* info);
int rdm_flat_shard_pack(edigpu_sector* s, const double* v_dev, int nvec, double* send_dev);
int rdm_flat_shard_enqueue(edigpu_sector* s, const double* v_dev, int nvec, const double* halos_dev, double* slab_dev,
                           const double** tri_dev);
// the summed packed triangles -> nvec dense matrices and traces, as edigpu_imp_rdm_flat returns them
void rdm_flat_shard_expand(const edigpu_sector* s, const double* tri, int nvec, double* rdm_host, double* norm2_host);

// Tables and workspace of edigpu_apply_xph / edigpu_ph_rdm on a library-built whole phonon sector (host_ph.hpp;
// kernels_ph.hip), made and uploaded by the first call on the handle and kept until edigpu_destroy.
struct PhDev;
void free_ph(edigpu_sector* s);
// The same on the rows [first, first + count) of the sector (edigpu_sector::ph_shard; host_ph.hpp ph_shard_plan_*), kept
// like the occupation tables' shard view.  ph_shard_rdm leaves the nvec x ncls x ph_slots x cw sums of this rank's rows in
// *sums_dev (null for count == 0); *ncls, *dimph, *cw describe them.
// occ_refuse_kind, then nph = 0 and -- rdm -- DimPh > kPhMaxDim: the refusals of the phonon entry points but the shard one
int ph_refuse_kind(const edigpu_sector* s, const std::string& who, bool rdm);
int ph_shard_apply(edigpu_sector* s, int64_t first, int64_t count, const double* src_dev, double* dst_dev, const std::string& who);
int ph_shard_rdm(edigpu_sector* s, int64_t first, int64_t count, const double* v_dev, int nvec, const double** sums_dev,
                 const std::string& who);

// Scratch buffer of the partner tables of the one-axis c / c^+ route (edigpu_axisop.hip; host_axisop.hpp,
// kernels_axisop.hip), kept by the DESTINATION handle of a call and grown on demand, until edigpu_destroy.
struct AxisDev;
void free_axisop(edigpu_sector* s);
// true: this pair of handles is not the real, phonon-free, library-built normal-mode pair that apply_op_normal_kernel
// serves; axisop_apply then makes every check and serves phonon, complex (kCmplxNormal) and ed_total_ud=F (kOrbs) pairs.
// cim = null: real coefficients; else complex ones on kCmplxNormal handles (edigpu_apply_cops_normal_z).  Returns after the
// stream has finished.
bool axisop_route(const edigpu_sector* src, const edigpu_sector* dst);
int axisop_apply(edigpu_sector* src, edigpu_sector* dst, const double* v_src, double* v_dst, int nops, const double* cre,
                 const double* cim, const int32_t* create, const int32_t* iorb, const int32_t* ispin, hipStream_t st,
                 const char* who);
// The two halves of axisop_apply for the call on shards (edigpu_shard_seeds.hip): every check of the handles and
// operators with the host tables (no device is touched), and the tables into the destination handle's scratch.
struct AxisTables;
struct AxisArgs;
int axisop_tables(const edigpu_sector* src, const edigpu_sector* dst, int nops, const int32_t* create, const int32_t* iorb,
                  const int32_t* ispin, bool cplx_coef, const char* who, AxisTables& tab);
int axisop_upload(edigpu_sector* dst, const AxisTables& tab, const double* cre, const double* cim, AxisArgs& a, hipStream_t st);
// The same of edigpu_apply_pairs_normal (edigpu_pairs.hip): checks and host tables; upload, launch, wait, free.  win = null:
// no term moves a down electron and the call runs on the rank's `rows` down rows alone, else the window + source form.
struct PairsTables;
int pairs_shard_tables(const edigpu_sector* src, const edigpu_sector* dst, int nterms, const double* coef, const int32_t* create1,
                       const int32_t* iorb1, const int32_t* ispin1, const int32_t* create2, const int32_t* iorb2,
                       const int32_t* ispin2, const std::string& who, PairsTables& tab);
int pairs_shard_call(const edigpu_sector* src, const PairsTables& tab, const ShardWindow* win, int64_t rows, const double* v_src,
                     double* v_dst, hipStream_t st);

// The table `order` of twin_sector_order of a library-built superc sector (host_twin.hpp; kernels_twin.hip), made and
// uploaded by the first edigpu_apply_twin[_sharded] with the handle as SOURCE and kept until edigpu_destroy: n entries,
// the electronic rows of the whole sector (also on a row shard: a rank's window of the destination reads any of them).
struct TwinDev {
  int64_t n = 0;
  int32_t* order = nullptr;
};
void free_twin(edigpu_sector* s);
// device bytes of that table (made lazily: the sector cache adds them like occ_table_bytes)
int64_t twin_table_bytes(const edigpu_sector* s);

// Interleaved workspace of edigpu_apply_multi_dev / edigpu_lanczos_tridiag_batch_dev (edigpu_batch.hip; kernels_multi.hip):
// two buffers of W vectors, the per-column partial sums and scalars.  Allocated by the first batch call on the handle,
// grown when a later call needs more, kept until edigpu_destroy.
struct BatchDev {
  int W = 0;                 // columns the two vector buffers hold
  int64_t len = 0;           // doubles per column (edigpu_sector::ws_len when they were allocated)
  double *P = nullptr, *Q = nullptr;
  double* partial = nullptr;
  int64_t partial_cap = 0;   // in doubles
  double* scal = nullptr;
  size_t scal_cap = 0;       // in doubles
};
void free_batch(edigpu_sector* s);
}  // namespace edigpu

struct edigpu_sector {
  explicit edigpu_sector(const edigpu::Switches& at_creation) : sw(at_creation) {}
  const edigpu::Switches sw;  // the environment the creating C-ABI call saw (switches.hpp): every set-up and launch choice reads it
  edigpu::SectorKind kind = edigpu::kNormal;
  int is_complex = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t dim = 0, nloc = 0, row_first = 0;
  // ---- normal ----
  int64_t dim_up = 0, dim_dw = 0, dw_first = 0, dw_count = 0;
  double* d_hd = nullptr;
  edigpu::DevEll up_ell;
  edigpu::DevCsr dw;          // DimDw rows
  int dw_maxrow = 0;
  edigpu::DevCsr nd;          // local rows, global columns
  int has_nd = 0;
  edigpu::HostCsr h_up, h_dw; // kept for export (tiny)
  int rows_per_block = 1;     // TD of the LDS row-block kernel (0: generic kernel)
  // factored diagonal / non-local block (library-built sectors; see HostFactored)
  int factored = 0;
  int fac_nimp = 0, fac_nterms = 0;
  double* d_eux = nullptr;      // nimp * dim_up
  double* d_ed = nullptr;       // dim_dw
  uint8_t* d_impd = nullptr;    // dim_dw
  double* d_ndcoef = nullptr;   // nterms
  uint32_t* d_jup = nullptr;    // nterms * dim_up
  // kCmplxNormal: H = S + iA as two real normal-mode handles + planar work vectors (6 * dim doubles)
  edigpu_sector* sub_s = nullptr;
  edigpu_sector* sub_a = nullptr;
  // kCmplxNormal, preferred: the same operator as ONE real sector on the doubled up index 2 iup + (re | im)
  // (host_build.cpp: build_normal_doubled); the interleaved complex vectors are its real vectors
  edigpu_sector* sub_d = nullptr;
  double* d_cz = nullptr;
  int panel_mode = 0;           // panel sweep variant (NormalArgs::panel_mode), fixed at set-up
  int tile_nchunks = 0, tile_rows = 0;
  int32_t* d_tile_chunks = nullptr;
  int32_t* d_tile_lbeg = nullptr;
  int tile_list_cap = 0;
  int4* d_tl_meta = nullptr;    // tile form of the panel sweep: per-row lists split by chunk membership
  int32_t* d_tl_col = nullptr;
  double* d_tl_val = nullptr;
  int tl_has_nd = 0;
  // panel-major vector layout of the fused Lanczos loop (NormalArgs::blk_shift): chosen at set-up for large factored
  // whole sectors, 0 = not available; lz_blocked: the current recurrence runs on it
  int blk_shift = 0;
  int blk_tail_balance = 1;     // 0 (Switches::tile_balance off): the padded grid of the tiled sweep (A/B timing, tests)
  int64_t blk_ps = 0, blk_len = 0;
  int4* d_bl_meta = nullptr;
  int blk_rows = 0;             // rows of an LDS block of the blocked sweep
  int blk_list_cap = 0;
  int32_t* d_bl_lend = nullptr;
  uint32_t* d_bl_ent = nullptr;
  double* d_bl_wtab = nullptr;
  bool lz_blocked = false;
  int64_t lz_len = 0;           // doubles per vector of the current recurrence (blk_len, ib->len or ws_len)
  // impurity-block image (large factored whole sectors built from a model; takes precedence over the panel-major image
  // above: lz_blocked then means "the recurrence runs on ib's padded panel layout")
  edigpu::IbDev* ib = nullptr;
  int row_split = 1;  // rows longer than the LDS: number of column parts the row kernel stages them in (SPLIT)
  int col_halo = 0;             // max |partner column - column| over the factored Hnd terms (transposed exchange)
  uint32_t* d_jdw = nullptr;    // nterms * dim_dw
  int32_t* d_mx_rowptr = nullptr;  // per local row: Hdw entries + applicable Hnd terms
  int32_t* d_mx_col = nullptr;
  double* d_mx_val = nullptr;
  // phonon branches (normal mode, whole sectors): vectors hold (nph + 1) electronic blocks of dim_el elements
  int nph = 0;
  int64_t dim_el = 0;
  double w0_ph = 0.0, a_ph = 0.0;
  double* d_gu = nullptr;       // [dim_up]  sum_a g_aa n_a,up
  double* d_gd = nullptr;       // [dim_dw]
  int64_t nd_nnz = 0;           // nnz of the (possibly host-only) CSR image of Hnd
  std::vector<double> h_hd;     // host copies for export when the device holds the factored form;
  edigpu::HostCsr h_nd;         // built on the first export (lazy_export) from the stored model
  bool lazy_export = false;
  edigpu_model model;           // library-built sectors: what edigpu_*_build was given
  int sec_a = 0, sec_b = 0;
  bool jz = false;                 // nonsu2 sector of Jz_basis=T: (Ntot, twoJz) = (sec_a, sec_b)
  bool built_by_library = false;   // made by edigpu_*_build: model, sec_a, sec_b are valid
  bool from_model() const { return built_by_library; }
  bool is_normal_family() const { return kind == edigpu::kNormal || kind == edigpu::kCmplxNormal; }
  bool is_flat_family() const { return kind == edigpu::kFlat || kind == edigpu::kDirect; }  // superc / nonsu2
  bool has_phonons() const { return nph > 0; }
  bool is_whole() const { return nloc == dim; }  // not a row shard
  // ---- flat ----
  edigpu::DevCsr loc, nonloc; // local rows; loc columns are shard-relative, nonloc global
  // ---- orbs (ed_total_ud = F) ----
  edigpu::OrbsArgs orbs;
  std::vector<edigpu::HostCsr> h_orbs_fac;  // kept for export (tiny)
  std::vector<double> h_orbs_hd;            // explicit diagonal when handed over
  std::vector<int> orbs_nups, orbs_ndws;    // library-built (edigpu_orbs_build): the sector's labels, Norb entries each
  // ---- direct (on-the-fly) ----
  int dir_ns = 0, dir_norb = 0, dir_nterms = 0;
  int32_t* d_dir_states = nullptr;
  int32_t* d_dir_offdw = nullptr;
  int32_t* d_dir_rkup = nullptr;
  edigpu::DirectTerm* d_dir_terms = nullptr;
  uint2* d_dir_tests = nullptr;   // (need_set, need_set | need_clear) per term, padded to a multiple of 4
  double* d_dir_dtab = nullptr;
  double* d_dir_xtab = nullptr;
  // ---- occupation operators (lazily built) ----
  edigpu::OccDev* occ = nullptr;
  edigpu::OccDev* occ_shard = nullptr;  // the view of a rank's rows (edigpu_*_sharded)
  // ---- impurity reduced density matrix (lazily built) ----
  edigpu::RdmDev* rdm = nullptr;
  edigpu::RdmShardDev* rdm_shard = nullptr;  // the view of a rank's rows (edigpu_imp_rdm_sharded)
  edigpu::RdmFlatDev* rdm_flat = nullptr;
  edigpu::RdmFlatShardDev* rdm_flat_shard = nullptr;  // the view of a rank's elements (edigpu_imp_rdm_flat_sharded)
  // ---- phonon displacement seed and phonon density matrix (lazily built) ----
  edigpu::PhDev* ph = nullptr;
  edigpu::PhDev* ph_shard = nullptr;    // the view of a rank's rows
  // ---- c / c^+ along one axis: table scratch of calls with this handle as destination (lazily built) ----
  edigpu::AxisDev* axis = nullptr;
  // ---- ED_TWIN=T reorder: the superc order table of calls with this handle as source (lazily built) ----
  edigpu::TwinDev* twin = nullptr;
  // ---- interleaved vectors of the batched product and recurrence (lazily built) ----
  edigpu::BatchDev* batch = nullptr;
  int batch_force_w = 0;         // edigpu_batch_set_width: 2, 4, 8 = the widest group whatever the size (measurement hook)
  // ---- Lanczos workspace (lazily allocated) ----
  int64_t partial_cap = 0;      // doubles in d_partial
  double* d_vin = nullptr;
  double* d_vout = nullptr;
  double* d_tmp = nullptr;
  double* d_partial = nullptr;  // reduction partials
  double* d_scal = nullptr;     // alpha/beta/flags on device
  edigpu::LoopSwitches lz = {};  // the environment at the start of the current recurrence (lanczos_prepare)
  // launch-bound sectors replay the steps of a recurrence from a captured hipGraph (lanczos_run): the executable and
  // what it was captured for
  hipGraphExec_t lz_graph = nullptr;
  int lz_graph_k = 0, lz_graph_nlanc = 0;
  const void* lz_graph_scal = nullptr;
  bool lz_graph_blocked = false, lz_graph_failed = false;
  size_t scal_cap = 0;          // doubles allocated in d_scal
  unsigned int* d_lzcnt = nullptr;  // arrival counter of the in-kernel finalize (lz_finalize.hpp)
  int64_t ws_len = 0;           // in doubles per vector
};

namespace edigpu {

// a handle under construction: edigpu_destroy (device memory, sub-handles with their parent) on every early return
struct SectorDeleter {
  void operator()(edigpu_sector* s) const { edigpu_destroy(s); }
};
using SectorPtr = std::unique_ptr<edigpu_sector, SectorDeleter>;

// ---- what the files of the C-ABI layer share (Source layout) ----
// (these were file-local while the layer was one file: they stay out of the library's dynamic symbols)
#pragma GCC visibility push(hidden)
// edigpu_setup.hip: the device images of a handle
int finish_handle(edigpu_sector* s);
void free_ell(DevEll& e);
void free_csr(DevCsr& d);
void free_ib(IbDev* p);
int setup_normal(edigpu_sector* s, int64_t dim_up, int64_t dim_dw, int64_t dw_first, int64_t dw_count, const double* hd,
                 const HostCsr& up, const HostCsr& dw, const int64_t* nd_rowptr, const int32_t* nd_col, const double* nd_val,
                 HostNormal* built = nullptr);
int setup_flat(edigpu_sector* s, int64_t nrow_local, int64_t ncol_global, int64_t row_first, const int64_t* rowptr,
               const int32_t* col, const double* val, int cplx);
int setup_orbs(edigpu_sector* s, const HostOrbs& ho, const double* hd);
int build_flat_on_device(edigpu_sector* s, const HostDirect& hd);
// edigpu_apply.hip: the product of any handle on stream st (phase: kernels.hpp, launch_normal)
int ensure_workspace(edigpu_sector* s);
int apply_any(edigpu_sector* s, const double* v_local, const double* v_full, double* hv, int phase, hipStream_t st);
int single_shard(const edigpu_sector* s, const char* who);
// edigpu_lanczos.hip: the recurrence on the handle's workspace
int lanczos_step(edigpu_sector* s, int iter, int nlanc, hipStream_t st);
int lanczos_prepare(edigpu_sector* s, int nlanc, double threshold, hipStream_t st);
int lanczos_seed(edigpu_sector* s, const double* src, uint64_t seed, hipStream_t st);
int lanczos_run(edigpu_sector* s, int from, int to, int nlanc, hipStream_t st);
int lanczos_fetch(edigpu_sector* s, const double* v, double* dst, hipStream_t st);
#pragma GCC visibility pop
// edigpu_apply.hip: one electronic block of a superc / nonsu2 phonon handle, phase 1 (own rows) / 2 (gathered block)
int apply_flat_block(edigpu_sector* s, const double* v_local, const double* v_full, double* hv, int phase, hipStream_t st);
// edigpu_lanczos.hip: a flat or on-the-fly sector held whole on this GPU, without phonons, whose product has the fused
// Lanczos epilogue (the sectors whose single-seed step is rotate -> product with partials -> finalize)
bool flat_lanczos_fusable(const edigpu_sector* s);
// edigpu_trl.hip: the thick-restart Lanczos driver, shared by edigpu_lanczos_eigh_multi and its sharded twin
struct TrlOps {
  std::function<int(const double* in, double* out, hipStream_t st)> apply;  // out = H in on this rank's elements
  std::function<int(double* dev, size_t n, hipStream_t st)> allreduce;     // sum over the ranks, in place; empty: one rank
};
int trl_solve(int device, hipStream_t st, int cplx, int64_t n, int64_t len, int64_t nglobal, const TrlOps& ops, int neigen, int ncv,
              double tol, int maxrestart, const double* v0, uint64_t seed_offset, double* evals, double* evecs,
              int* nconv_out, int* nmatvec_out);
// edigpu_ops.hip: apply_Cops on a window of destination units: v_dst_rows = sum_s coef_s O_s v_src for the
// destination's down rows (normal mode) / rows (superc, nonsu2) [first, first + count); v_src_full holds the WHOLE source
// vector in the reference's layout; coef2 = (re, im) per operator (normal mode: real).  gathered (superc / nonsu2 only):
// v_src_full is the all-gather of the ranks' padded chunks instead, shard_src.hpp counted in double2 -- the form phonon row
// shards need.  checked: the caller has made apply_cops_rows_check with the same arguments.  Returns after the stream finished.
int apply_cops_rows(edigpu_sector* src, edigpu_sector* dst, const double* v_src_full, double* v_dst_rows, int64_t first,
                    int64_t count, int nops, const double* coef2, const int32_t* create, const int32_t* iorb,
                    const int32_t* ispin, hipStream_t st, const char* who, const ShardSrc* gathered = nullptr,
                    bool checked = false);
// its checks of the handles and operators alone (no device is touched), every operator before any launch
int apply_cops_rows_check(const edigpu_sector* src, const edigpu_sector* dst, int nops, const double* coef2, const int32_t* create,
                          const int32_t* iorb, const int32_t* ispin, const char* who, const ShardSrc* gathered = nullptr);

}  // namespace edigpu
