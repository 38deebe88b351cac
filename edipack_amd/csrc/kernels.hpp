// kernels.hpp -- launch wrappers of the gfx950 kernels (definitions in kernels_*.hip).
#pragma once
#include "edigpu_internal.hpp"
#include "host_rdm.hpp"
#include "host_rdm_flat.hpp"

namespace edigpu {

// device-resident Lanczos scalars (kernels_lanczos.hip)
enum { SC_ALPHA = 0, SC_BETA = 1, SC_STOP = 2, SC_NDONE = 3, SC_NORM = 4, SC_THR = 5, SC_EXACT = 6, SC_AB = 8 };
constexpr int kRedBlocks = 1024;
constexpr int kMaxPartials = 1 << 16;  // minimum capacity of the per-workgroup partial buffer (edigpu_sector::partial_cap)

// opt a kernel into more than 48 KiB of dynamic LDS, once per (device, kernel, size) instead of on every launch
int ensure_dynamic_lds(const void* kernel, size_t bytes);
// workgroups of a kernel that stay resident on one CU (cached occupancy query; < 1 on error) and the CU count
int resident_blocks(const void* kernel, int threads, size_t dyn_lds);
int device_cu_count();

// ---- normal mode (kernels_normal.hip) ----
// phase: 3 = fused (local+remote, overwrite), 1 = local only (overwrite), 2 = remote only (accumulate)
// v_local : first element of the shard's own rows, v_full : element 0 of the whole vector.
int launch_normal(const edigpu_sector* s, const double* v_local, const double* v_full, double* hv,
                  int phase, hipStream_t st);
// rows_td: Switches::rows_td
int normal_pick_rows_per_block(int64_t dim_up, int64_t dw_count, OptInt rows_td);
// transposed exchange: the row half and the column half of the product on a whole-sector handle
bool normal_transposable(const edigpu_sector* s);
bool normal_transposable_el(const edigpu_sector* s);  // ignoring the phonon blocks
int launch_normal_rows(const edigpu_sector* s, int64_t dw_first, int64_t dw_count, const double* v_rows,
                       double* hv_rows, hipStream_t st);
int launch_normal_cols(const edigpu_sector* s, int64_t col_first, int64_t ncol, int64_t stride, int halo,
                       const double* w, double* hv, hipStream_t st);
// electron-phonon ladder: up[i] += c_up t[i], dn[i] += c_dn t[i] (either target may be NULL); n doubles
int launch_eph_scatter(int64_t n, const double* t, double* up, double c_up, double* dn, double c_dn, hipStream_t st);
// _CMPLX_NORMAL: interleaved complex <-> planar, y = (yr - t1) + i (yi + t2)  (kernels_ops.hip)
int launch_deinterleave(int64_t n, const double* z, double* re, double* im, hipStream_t st);
int launch_combine_interleave(int64_t n, const double* yr, const double* yi, const double* t1, const double* t2,
                              double* z, hipStream_t st);
// row shard <-> all-to-all buffers (kernels_ops.hip)
int launch_transpose_pack(int64_t dim_up, int64_t nrows, int64_t q, int world, int64_t pcol, int halo,
                          const double* v_rows, double* send, hipStream_t st);
int launch_transpose_unpack_add(int64_t dim_up, int64_t nrows, int64_t q, int world, int64_t pcol, int halo,
                                const double* recv, double* hv_rows, hipStream_t st);
// fused Lanczos step (normal, single shard): P = Lanczos vector, Q = work vector, see kernels_normal.hip
bool normal_lanczos_fusable(const edigpu_sector* s);
// nlanc / finalized: when the sweep finalizes the step in its last workgroup (*finalized = true) no finalize kernel must follow
// X / in_x: the impurity-block image writes the new Lanczos vector of a later step to X instead of P (*in_x = true: the
// caller swaps its P and X buffers); other images ignore them
int launch_normal_lanczos(const edigpu_sector* s, double* P, double* Q, const double* scal,
                          double* partial, int64_t partial_cap, bool first, bool lazy_axpy, hipStream_t st, int* npartial,
                          int nlanc = 0, bool* finalized = nullptr, double* X = nullptr, bool* in_x = nullptr);
// alpha = sum(partial[0:np]), beta = sqrt(sum(partial[np:2np]) - alpha^2) with an exact fallback pass
int lz_finalize_alpha_beta(const double* P, const double* Q, int64_t n, double* partial, int np,
                           double* scal, int iter, int nlanc, hipStream_t st);
int lz_finalize_alpha(const double* partial, int np, double* scal, int iter, int nlanc, hipStream_t st);

// ---- flat CSR (kernels_csr.hip) ----
// y[0:nrow] (=|+=) A x ; T = double (cplx=0) or (re,im) pairs (cplx=1)
int launch_csr(const DevCsr& a, int cplx, const double* x, double* y, int accumulate,
               hipStream_t st);
int launch_zero(double* y, int64_t n, hipStream_t st);

// ---- direct / on-the-fly (kernels_direct.hip): hv[local rows] = H v_full ----
// sig: device scalar the <Q|Q> partial is accumulated about (the previous alpha, scal + SC_ALPHA; see k_finalize_ab)
// cap: capacity of `partial` in doubles, checked BEFORE anything is enqueued (2 partials per workgroup)
int launch_direct_lanczos(const edigpu_sector* s, const double* v_full, double* q, double* partial, int64_t cap, int* np,
                          const double* sig, hipStream_t st);
bool csr_lanczos_fusable(const DevCsr& a);
int launch_csr_lanczos(const DevCsr& a, int cplx, const double* x, double* y, double* partial, int64_t cap, int* np,
                       const double* sig, hipStream_t st);
// (P, Q) <- ((Q - alpha*P)/beta, -beta*P): rotate with the pending axpy of the fused step folded in
int lz_rotate_lazy(double* P, double* Q, int64_t n, const double* scal, hipStream_t st);
int lz_next_vector(const double* P, const double* Q, double* X, int64_t n, const double* scal, bool lazy, hipStream_t st);
int launch_direct(const edigpu_sector* s, const double* v_full, double* hv, hipStream_t st);

// ---- W = 2, 4 or 8 interleaved vectors per sweep over a flat sector (kernels_multi.hip) ----
// layout: element (row, column j) at Xi[row * W + j] (double, or double2 when cplx); g <= W vectors of nrow elements in
// the natural layout, one after another; the columns past g are written as zeros
int launch_interleave_multi(int W, int cplx, int64_t nrow, int g, const double* src, double* dst, hipStream_t st);
int launch_deinterleave_multi(int W, int cplx, int64_t nrow, int g, const double* src, double* dst, hipStream_t st);
// Yi = H Xi (lz = false), or Yi += H Xi with the per-column partials [3 * W][*np] of <P|Q>, sum (Q - sg_j P)^2, <P|P>
// (lz = true; sg_j = scal[j * sstride + SC_ALPHA]); cap: doubles in `partial`, checked before anything is enqueued
int launch_csr_multi(const DevCsr& a, int cplx, int W, const double* Xi, double* Yi, bool lz, double* partial, int64_t cap,
                     int* np, const double* scal, int64_t sstride, hipStream_t st);
int launch_direct_multi(const edigpu_sector* s, int W, const double* Xi, double* Yi, bool lz, double* partial, int64_t cap,
                        int* np, const double* scal, int64_t sstride, hipStream_t st);
// the vector kernels of W recurrences in lock-step: column j keeps its SC_* scalars at scal + j * sstride; a column whose
// stop flag is set is held at exactly zero
int lz_norm_begin_multi(int W, int cplx, int64_t nrow, double* P, double* partial, int64_t cap, double* scal,
                        int64_t sstride, hipStream_t st);
int lz_rotate_lazy_multi(int W, int cplx, int64_t nrow, double* P, double* Q, const double* scal, int64_t sstride,
                         hipStream_t st);
int lz_finalize_ab_multi(int W, int cplx, int64_t nrow, const double* P, const double* Q, const double* partial, int np,
                         double* scal, int64_t sstride, int nlanc, hipStream_t st);

// ---- Lanczos vector kernels (kernels_lanczos.hip); n counts doubles ----
int lz_norm_begin(double* vin, int64_t n, double* partial, double* scal, hipStream_t st);
int lz_rotate(double* vin, double* vout, int64_t n, const double* scal, hipStream_t st);
int lz_alpha(const double* vin, double* vout, const double* tmp, int64_t n, double* partial,
             double* scal, int iter, int nlanc, hipStream_t st);
int lz_beta(const double* vin, double* vout, int64_t n, double* partial, double* scal, int iter,
            int nlanc, hipStream_t st);
int lz_axpy_coef(double* acc, const double* vin, int64_t n, double coef, const double* scal,
                 int iter, hipStream_t st);
int lz_add_dot3(const double* P, double* Q, const double* tmp, int64_t n, const double* scal, double* partial, int* np,
                hipStream_t st);
int lz_fill_random(double* v, int64_t n, uint64_t seed, hipStream_t st);
// natural layout (idw * DimUp + iup) <-> panel-major layout of the Lanczos loop (normal_args.hpp: blk_shift); the
// padding columns of the last panel are written as zeros
int vec_to_blocked(const double* src, double* dst, int64_t dim_up, int64_t dim_dw, int shift, hipStream_t st);
int vec_from_blocked(const double* src, double* dst, int64_t dim_up, int64_t dim_dw, int shift, hipStream_t st);
int launch_normal_blocked(const edigpu_sector* s, const double* v, double* hv, hipStream_t st);
// impurity-block image (kernels_ib.hip): layout conversion, plain product and fused Lanczos step on its vectors
int vec_to_ib(const IbDev* ib, const double* src, double* dst, hipStream_t st);
int vec_from_ib(const IbDev* ib, const double* src, double* dst, hipStream_t st);
int launch_ib(const edigpu_sector* s, const double* v, double* hv, hipStream_t st);
int launch_ib_lanczos(const edigpu_sector* s, const double* P, double* Q, double* X, const double* scal, double* partial,
                      int64_t partial_cap, bool first, bool lazy_axpy, hipStream_t st, int* npartial);
// local-block kernels on the same layout (kernels_sb.hip, round 4); launch_ib / launch_ib_lanczos take them when IbDev::sb is set
int launch_sb(const edigpu_sector* s, const double* v, double* hv, hipStream_t st);
// generic LDS row kernel on the padded panel layout in position order (kernels_normal.hip; IbDev::pr)
int launch_normal_rows_pos(const edigpu_sector* s, const double* P, double* Q, double* X, int what, const double* scal, hipStream_t st);
int launch_sb_lanczos(const edigpu_sector* s, const double* P, double* Q, double* X, const double* scal, double* partial,
                      int64_t partial_cap, bool first, bool lazy_axpy, hipStream_t st, int* npartial);
// row shards on the padded panel layout (kernels_sb.hip): see there for the shard form of the layout
bool sb_shardable(const edigpu_sector* s);
int sb_shard_panels(const edigpu_sector* s, int world);
int sb_shard_to_panels(const edigpu_sector* s, const double* rows, double* dst, int64_t count, int64_t q, int world, hipStream_t st);
int sb_shard_from_panels_add(const edigpu_sector* s, const double* a, const double* b, double* rows, int64_t count, int64_t q, hipStream_t st);
int launch_sb_rows_shard(const edigpu_sector* s, int64_t row0, int64_t count, int64_t q, const double* v, double* hv, hipStream_t st);
int launch_sb_cols_shard(const edigpu_sector* s, int p0, int np, int64_t q, int npmax, int world, const double* v, double* out,
                         hipStream_t st);
int sb_nb0(int norb);
int sb_cols_waves(int cw);  // cw: Switches::sb_cw, as for sb_cols_gs (host_sb.hpp)
size_t sb_rows_lds(int nbw, int rimg_len, bool top = false);
// one half of the rows kernel's product on a sector whose rows are staged in halves (h = 0 / 1: top walked level empty /
// occupied); scal: the recurrence's scalars (stop flag) or null
int launch_sb_rows_half(const edigpu_sector* s, int h, const double* v, double* hv, const double* scal, hipStream_t st);
size_t sb_cols_lds(int nbw, int nloc, int max_chunk_rows, int max_chunk_slots, int gs);
bool sb_rows_config(int norb, int slots, int plen, int cs, int force_nt, int force_nbt, int* nt_out, int* nbt_out);
size_t ib_rows_lds_bytes(int nb, int rimg_len);
size_t ib_cols_lds_bytes(int nb, int max_chunk_rows, int max_chunk_blocks);
bool ib_rows_config(int norb, int nb, int nlist, int plen, int rimg_len, int force_nt, int* nt_out, int* nbt_out, bool split = false);
int measure_membw(int64_t bytes, double out[3]);
// stand-alone vector kernels with explicit device scalars (sharded loop)
int vec_rotate(int64_t n, double* vin, double* vout, const double* beta2, hipStream_t st);
int vec_add_dot(int64_t n, const double* vin, double* vout, const double* tmp, double* out, double* work, hipStream_t st);
int vec_axpy_nrm2(int64_t n, const double* vin, double* vout, const double* alpha, double* out, double* work, hipStream_t st);
int vec_scale(int64_t n, double* v, const double* nrm2, hipStream_t st);
// one-reduction recurrence on any sharded vector: (v, w) <- ((w - alpha v)/beta, -beta v) from ab = (<v|w>, <w|w>),
// and w += tmp with this rank's (<v|w>, <w|w>) (work: kRedBlocks doubles)
int vec_rotate_lazy(int64_t n, double* vin, double* vout, const double* ab, hipStream_t st);
int vec_add_dot2(int64_t n, const double* vin, double* vout, const double* tmp, double* out2, double* work,
                 hipStream_t st);
// fused vector updates of the transposed-exchange Lanczos step (work: kRedBlocks doubles)
int vec_rotate_pack(int first, int64_t dim_up, int64_t nrows, int64_t q, int world, int64_t pcol, int halo,
                    double* vin, double* vout, const double* ab, double* send, hipStream_t st);
int vec_unpack_add_dot2(int64_t dim_up, int64_t nrows, int64_t q, int64_t pcol, int halo, const double* vin,
                        double* vout, const double* tmp, const double* back, double* out2, double* work,
                        hipStream_t st);

// ---- one-reduction recurrence on shards (kernels_shard.hip); t / tprev: the reduced sums of the two previous steps ----
// (null where there is none), work: 3 * kRedBlocks doubles, sums: where this rank's three sums of the step land
#pragma GCC visibility push(hidden)
// (v, w) <- ((w - alpha v) / beta, -beta v), nothing on the first step; send != null: the new v also goes into the
// all-to-all send buffer of the column-block exchange.  n counts doubles
int shard_rotate3(bool first, int64_t n, int64_t dim_up, int64_t q, int world, int64_t pcol, int halo, double* vin, double* vout,
                  const double* t, const double* tprev, double* send, hipStream_t st);
// w += tmp (+ back through the exchange's index map when back != null), then the three sums
int shard_add_dot3(int64_t n, int64_t dim_up, int64_t q, int64_t pcol, int halo, const double* vin, double* vout,
                   const double* tmp, const double* back, const double* tprev, double* work, double* sums, hipStream_t st);
// the same two on vectors that share the padded panel layout element by element; n2 counts pairs of doubles
int shard_panel_rotate(int64_t n2, double* x, const double* v, const double* t, const double* tprev, hipStream_t st);
int shard_panel_add_dot(int64_t n2, const double* x, double* vdst, const double* rowhalf, const double* colhalf,
                        const double* t, const double* tprev, double* work, double* sums, hipStream_t st);
#pragma GCC visibility pop

// ---- thick-restart Lanczos multi-vector kernels (kernels_trl.hip) ----
// h_dev (2 doubles per basis vector: re, im) = Q^H w, then w -= Q h; n counts complex or real elements
int trl_orthogonalize(int cplx, int64_t n, int nvec, const double* Q, int64_t ldq, double* w, double* h_dev,
                      double* partial, hipStream_t st, const int* skip = nullptr);
int trl_dots(int cplx, int64_t n, int ndot, const double* Q, int64_t ldq, const double* w, double* h_dev,
             double* partial, hipStream_t st, const int* skip = nullptr);
int trl_subtract(int cplx, int64_t n, int nvec, const double* Q, int64_t ldq, const double* h_dev, double* w,
                 hipStream_t st, const int* skip = nullptr);
// after the first sweep (nvec coefficients + <w|w> in h_dev): skip <- 1 when at least eta2 of |w|^2 is left (no second
// pass); hf_dev <- the coefficients with those below thr * |w_new| set to exactly zero (all kept when skip = 0)
int trl_decide(const double* h_dev, int nvec, double eta2, double thr2, double* hf_dev, int* skip, hipStream_t st);
int trl_norm2(int cplx, int64_t n, const double* w, double* h_dev, double* partial, hipStream_t st);
// coefficients (nvec pairs + <w|w>) below sqrt(thr2) * |w| -> exact zeros, in place
int trl_filter(double* h_dev, int nvec, double thr2, hipStream_t st);
int trl_partial_doubles(void);
int trl_rotate_basis(int64_t len, int m, int k, const double* Q, int64_t ldq, const double* Y_dev, int ldy,
                     double* out, int64_t ldo, hipStream_t st);
int trl_scale(int64_t len, double* v, double f, hipStream_t st);

// ---- c / c^+ between normal-mode sectors (kernels_ops.hip) ----
int launch_apply_op_normal(int64_t dst_dimup, int64_t dst_dimdw, int64_t src_dimup, int spin_down,
                           const uint32_t* part, const double* src, double* dst, hipStream_t st, double coef = 1.0,
                           int accumulate = 0);

int launch_phonon(const edigpu_sector* s, const double* v, double* hv, hipStream_t st);
// the same pass on a shard of down rows [dw_first, dw_first + dw_count) of a normal-mode sector: (Nph + 1) blocks of
// dw_count * DimUp elements (the layout of spMatVec_mpi_normal_main); density couplings only
int launch_phonon_rows(const edigpu_sector* s, int64_t dw_first, int64_t dw_count, const double* v, double* hv,
                       hipStream_t st);
int launch_apply_op_flat(int64_t ndst, int ns, uint32_t bit, int create, const int32_t* dst_states,
                         const int32_t* src_offdw, const int32_t* src_rkup, const double* src, double* dst,
                         hipStream_t st, double cre = 1.0, double cim = 0.0, int accumulate = 0, int nblk = 1,
                         int64_t nsrc = 0,  // nblk > 1: phonon blocks of ndst (destination) / nsrc (source) elements
                         const ShardSrc* gathered = nullptr);  // src = the all-gathered shards, counted in double2 (nsrc unused)

// ---- ed_total_ud = F sectors (kernels_orbs.hip) ----
int launch_orbs(const edigpu_sector* s, const double* v, double* hv, hipStream_t st);

// ---- on-device construction of the stored flat image (kernels_build.hip) ----
struct BuildArgs {
  int64_t nrow, row_first;  // local rows, first global row
  int64_t lo, hi;           // column window of the loc block (global indices)
  int ns, norb, nterms;
  const int32_t* states;
  const int32_t* off_dw;
  const int32_t* rk_up;
  const DirectTerm* terms;
  const uint8_t* vid;  // [2 * nterms]: dictionary id of +coef for (term, forward / reverse); id ^ 1 = -coef
  const double* dtab;
  const double* xtab;
};
// widths per 64-row slice of the loc / non-local block; totals = {entries loc, entries non-local,
// longest row loc, longest row non-local}
int launch_build_count(const BuildArgs& a, int32_t* width_loc, int32_t* width_non, unsigned long long* totals,
                       hipStream_t st);
int launch_build_fill(const BuildArgs& a, int which, int maxlen, const int32_t* sptr, uint32_t* pk, double* diag,
                      hipStream_t st);

// ---- occupation operators (kernels_occ.hip; tables: host_occ.hpp) ----
// what the kernels read of a sector: normal mode the vector is nblk (phonon) blocks of dim_dw rows of dim_up elements,
// pu[iup] / pd[idw] the patterns; flat (superc / nonsu2): nblk blocks of dim_up rows, pu[row] = up | down << norb
struct OccTables {
  int norb = 0, flat = 0, cplx = 0, nblk = 1;
  int64_t dim_up = 0, dim_dw = 1;
  const uint16_t* pu = nullptr;
  const uint8_t* pd = nullptr;
  const int32_t* order = nullptr;  // normal mode: rows sorted by down pattern (occ_sort_rows)
};
struct OccWeights {  // occ_weight_table of w_up, w_dw
  double wu[32], wd[32];
};
struct OccSlots {    // occ_sum_slots
  uint8_t need_up[64], need_dw[64];
  int nslots;
};
struct OccRuns {     // occ_sort_rows
  int32_t run[33];
};
// v_dst(i) = (wu[up pattern of i] + wd[down pattern of i]) v_src(i); enqueued on st, no synchronisation
int launch_apply_occ(const OccTables& t, const OccWeights& w, const double* src, double* dst, hipStream_t st);
// waves (= partial sums per vector) launch_occ_moments wants for this sector on a device of ncu compute units
int occ_moment_waves(const OccTables& t, int ncu);
// sums[k][64] (slots of occ_sum_slots) of nvec consecutive vectors; partial: nvec * nwaves * 64 doubles
int launch_occ_moments(const OccTables& t, const OccSlots& sl, const OccRuns& rn, const double* v, int nvec, int nwaves,
                       double* partial, double* sums, hipStream_t st);

// ---- phonon operators (kernels_ph.hip; tables and work list: host_ph.hpp) ----
struct PhUnit;
// what the kernels read of a phonon sector: dimph blocks of dim_el elements (interleaved complex when cplx); the Gram
// kernel's element of (sorted row r, sorted column j) is rorder[r] * dim_cols + corder[j]
struct PhTables {
  int cplx = 0, dimph = 0, nunits = 0, ncls = 0;
  int64_t dim_el = 0, dim_cols = 0;
  const double* sq = nullptr;  // ph_sqrt_table: dimph + 1 entries
  const int32_t *rorder = nullptr, *corder = nullptr, *ubeg = nullptr;
  const PhUnit* units = nullptr;
};
// dst(i_el, n) = sq[n+1] src(i_el, n+1) + sq[n] src(i_el, n-1); enqueued on st, no synchronisation; dst must not overlap src
int launch_apply_xph(const PhTables& t, const double* src, double* dst, hipStream_t st);
// sums[ncls][ph_slots(dimph) (* 2)] of one vector; partial: nunits * ph_slots(dimph) (* 2) doubles
int launch_ph_rdm(const PhTables& t, const double* v, double* partial, double* sums, hipStream_t st);

// ---- fused two-operator products on normal-mode vectors (kernels_pairs.hip; tables: host_pairs.hpp) ----
// the device copies of a PairsTables: pu[nterms][du_dst], pd[nterms][dd_dst]; a vector is nblk (phonon) blocks of dd rows
// of du elements; bit t of id_up / id_dw: term t leaves that species alone and its table is not read
struct PairsArgs {
  int nterms = 0, nblk = 1;
  uint32_t id_up = 0, id_dw = 0;
  int64_t du_src = 0, dd_src = 0, du_dst = 0, dd_dst = 0;
  double coef[8] = {0};
  const uint32_t* pu = nullptr;
  const uint32_t* pd = nullptr;
};
// dst[p][jdw][jup] = sum_t coef_t s_t src[p][pd_t(jdw)][pu_t(jup)], acc = 0 then acc = fma(coef_t, +-x_t, acc) for t
// ascending; every element of dst is written once; enqueued on st, no synchronisation; dst must not overlap src
int launch_apply_pairs(const PairsArgs& a, const double* src, double* dst, hipStream_t st);
// the window + source form (shard_src.hpp ShardWindow): dst = the down rows [w.j_first, w.j_first + w.j_count) of every block,
// src = the all-gathered shards (w.s.unit_len = du_src); the same arithmetic in the same order, element by element
int launch_apply_pairs_window(const PairsArgs& a, const ShardWindow& w, const double* src, double* dst, hipStream_t st);

// ---- c / c^+ along one axis of a vector [O][A][I] (kernels_axisop.hip; tables: host_axisop.hpp) ----
// the device copy of an AxisTables (part[nterms][a_dst]) and the coefficients; I in doubles
struct AxisArgs {
  int nterms = 0;
  int64_t I = 0, a_src = 0, a_dst = 0, O = 0;
  double cre[8] = {0}, cim[8] = {0};
  const uint32_t* part = nullptr;
};
// dst[o][j][i] = sum_t coef_t s_t(j) src[o][part_t(j)][i] in the order stated in kernels_axisop.hip; cplx_coef: elements
// are double2 and the coefficients complex (I even), else cim is not read; every element of dst is written once; enqueued
// on st, no synchronisation; dst must not overlap src
int launch_apply_axisop(const AxisArgs& a, int cplx_coef, const double* src, double* dst, hipStream_t st);
// the window + source form (shard_src.hpp ShardWindow): dst = the indices [w.j_first, w.j_first + w.j_count) of axis A in every
// o, src = the all-gathered shards (a.O = w.s.nblk, w.s.unit_len = a.I, in doubles); the same arithmetic, element by element
int launch_apply_axisop_window(const AxisArgs& a, const ShardWindow& w, int cplx_coef, const double* src, double* dst,
                               hipStream_t st);

// ---- the ED_TWIN=T reorder: a twin sector's vectors from the stored sector's (kernels_twin.hip; host_twin.hpp) ----
// Elements are doubles, or (cplx) double2; src and dst may be 8-byte aligned only (16-byte accesses where they allow).
// Enqueued on st, no synchronisation; dst must not overlap src; every element of dst is written once.
// normal mode: nvec vectors [nblk][R][C] (C fastest) -> [nblk][C][R]
int launch_twin_transpose(int cplx, int64_t R, int64_t C, int nblk, int nvec, const void* src, void* dst, hipStream_t st);
// superc / nonsu2: dst[b n + i] = src[b n + order[i]], b over the nvec * nblk blocks; order == null: src[b n + n - 1 - i]
int launch_twin_gather(int cplx, int64_t n, int nblk, int nvec, const int32_t* order, const void* src, void* dst, hipStream_t st);
// The window + source forms (shard_src.hpp ShardWindow): dst = the rows [w.j_first, w.j_first + w.j_count) of the
// destination (its down rows = the source's up columns; rows of superc / nonsu2) as [nvec][nblk][j_count][..]; src = the
// all-gather of the ranks' parts, each nvec vectors of vstride = q unit_len nblk elements (w.s counted in elements, w.s.chunk
// = nvec vstride, w.s.units = R / n, w.s.unit_len = C / 1)
int launch_twin_transpose_window(int cplx, int64_t R, int64_t C, int nvec, const ShardWindow& w, int64_t vstride, const void* src,
                                 void* dst, hipStream_t st);
int launch_twin_gather_window(int cplx, int64_t n, int nvec, const ShardWindow& w, int64_t vstride, const int32_t* order,
                              const void* src, void* dst, hipStream_t st);

// ---- impurity reduced density matrix (kernels_rdm.hip; tables and work list: host_rdm.hpp) ----
struct RdmArgs {  // the device copies of an RdmPlan
  int cw = 1, stride = 0, ld_max = 0, ept_max = 0, rel_max = 0;
  int64_t dim_up = 0, dim_dw = 0;
  const int32_t* rows = nullptr;
  const uint16_t* rel = nullptr;
  const uint32_t* ent = nullptr;
  const RdmWork* work = nullptr;
};
// dynamic LDS of the tiles kernel: staged slab, accumulators, the chunk's run starts
size_t rdm_lds_bytes(const RdmArgs& a);
// out[k][ntri cw] (ostride doubles apart) = the packed triangles of nvec vectors vstride doubles apart; partial: nvec
// blocks of pstride doubles; groups: host array.  Enqueued on st, no synchronisation.
int launch_imp_rdm(const RdmArgs& a, int nwork, const RdmGroup* groups, int ngroups, const double* v, int64_t vstride,
                   int nvec, double* partial, int64_t pstride, double* out, int64_t ostride, hipStream_t st);
// The same of a rank's down rows (edigpu_imp_rdm_sharded; host_rdm.hpp RdmShardPlan): the work list of `in` on the
// shards v, that of `slab` (nslab workgroups, 0: none) on the boundary slabs, their partial sums in one buffer of nvec
// blocks of pstride doubles; the final sums run over the groups of both.
int launch_imp_rdm_shard(const RdmArgs& in, int nin, const double* v, int64_t vstride, const RdmArgs& slab, int nslab,
                         const double* vslab, int64_t sstride, const RdmGroup* groups, int ngroups, int nvec, double* partial,
                         int64_t pstride, double* out, int64_t ostride, hipStream_t st);
// dst[nvec][nblk][t.nrows][rowlen] <- the rows t names: of the shards v (vstride doubles apart, nblk blocks of `count`
// rows of rowlen doubles), of the gathered halos [world][nvec][nblk][H][rowlen], or zeros.  The halo a rank sends
// (RdmShardPlan::pack, halos = null) and the slab of its tail run (RdmShardPlan::fill).
int launch_rdm_rows(const RdmRowCopy& t, int nblk, int rowlen, int nvec, const double* v, int64_t vstride, int64_t count,
                    const double* halos, int H, double* dst, hipStream_t st);

// ---- the same of superc / nonsu2 vectors (kernels_rdm_flat.hip; tables and work list: host_rdm_flat.hpp) ----
struct RdmFlatArgs {  // the device copies of an RdmFlatPlan
  int cw = 1, norb = 0, stage_max = 0, ept_max = 0, rel_max = 0;
  int64_t dim_el = 0;
  const int64_t* rowstart = nullptr;
  const int32_t* bdw = nullptr;
  const uint16_t* rel = nullptr;
  const uint32_t* ent = nullptr;
  const RdmFlatPanel* panels = nullptr;
  const RdmFlatWork* work = nullptr;
};
// dynamic LDS of the tiles kernel: staged slab, accumulators, the panel's run starts
size_t rdm_flat_lds_bytes(const RdmFlatArgs& a);
// as launch_imp_rdm
int launch_imp_rdm_flat(const RdmFlatArgs& a, int nwork, const RdmGroup* groups, int ngroups, const double* v, int64_t vstride,
                        int nvec, double* partial, int64_t pstride, double* out, int64_t ostride, hipStream_t st);
// The same of a rank's elements (edigpu_imp_rdm_flat_sharded; host_rdm_flat.hpp RdmFlatShardPlan), as launch_imp_rdm_shard:
// the work list of `in` on the shards v, that of `slab` (nslab workgroups, 0: none) on the tail slabs, their partial sums in
// one buffer; the final sums run over the groups of both.
int launch_imp_rdm_flat_shard(const RdmFlatArgs& in, int nin, const double* v, int64_t vstride, const RdmFlatArgs& slab, int nslab,
                              const double* vslab, int64_t sstride, const RdmGroup* groups, int ngroups, int nvec, double* partial,
                              int64_t pstride, double* out, int64_t ostride, hipStream_t st);
// dst[nvec][nblk][dlen] (cw doubles per element) <- the nseg segments of the device table segs (the longest of maxlen
// elements): of the shards v (vstride doubles apart, nblk blocks of `count` elements), of the gathered halos
// [world][nvec][nblk][H], or zeros.  The halo a rank sends (RdmFlatShardPlan::pack, halos = null) and its tail slab (fill).
int launch_rdm_flat_segs(const RdmFlatSeg* segs, int nseg, int64_t maxlen, int nblk, int cw, int nvec, const double* v,
                         int64_t vstride, int64_t count, const double* halos, int64_t H, double* dst, int64_t dlen, hipStream_t st);

}  // namespace edigpu
