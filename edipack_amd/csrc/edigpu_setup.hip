// edigpu_setup.hip -- device images of a sector: uploads of the host images (host_pack.hpp, host_ib.hpp, host_sb.hpp), the
// setup_* routine of each kind of handle, the stored flat image generated on the device.  Called by the entry points
// that create handles (edigpu_build.hip); freed by edigpu_destroy (edigpu_capi.hip).
#include <algorithm>
#include <cstddef>
#include <memory>

#include "dev_mem.hpp"
#include "host_ib.hpp"
#include "host_pack.hpp"
#include "host_sb.hpp"
#include "kernels.hpp"

namespace edigpu {

// the row meta of host_pack.hpp as the device reads it
static const int4* as_int4(const std::vector<HostInt4>& v) {
  static_assert(sizeof(HostInt4) == sizeof(int4) && offsetof(HostInt4, x) == offsetof(int4, x) &&
                    offsetof(HostInt4, y) == offsetof(int4, y) && offsetof(HostInt4, z) == offsetof(int4, z) &&
                    offsetof(HostInt4, w) == offsetof(int4, w),
                "HostInt4 is uploaded as int4");
  return reinterpret_cast<const int4*>(v.data());
}

// upload a CSR given with int64 row pointers; columns optionally shifted
static int upload_csr(DevCsr& d, int64_t nrow, const int64_t* rowptr, const int32_t* col,
                      const double* val, int cplx) {
  d = DevCsr();
  d.nrow = nrow;
  d.nnz = rowptr ? rowptr[nrow] : 0;
  d.avg_row = nrow > 0 ? (double)d.nnz / (double)nrow : 0.0;
  if (nrow == 0) return 0;
  if (d.nnz >= ((int64_t)1 << 31)) {
    d.wide = 1;
    if (dev_upload(&d.rowptr64, rowptr, (size_t)nrow + 1)) return 1;
  } else {
    std::vector<int32_t> rp((size_t)nrow + 1);
    for (int64_t i = 0; i <= nrow; i++) rp[i] = (int32_t)rowptr[i];
    if (dev_upload(&d.rowptr32, rp.data(), rp.size())) return 1;
  }
  // 8 zero entries behind the last row: the panel sweep reads a row's list in batches of 8 (kernels_panel.hip)
  std::vector<int32_t> cpad(col, col + d.nnz);
  cpad.resize((size_t)d.nnz + 8, 0);
  std::vector<double> vpad(val, val + (size_t)d.nnz * (cplx ? 2 : 1));
  vpad.resize(vpad.size() + 8, 0.0);
  if (dev_upload(&d.col, cpad.data(), cpad.size())) return 1;
  if (dev_upload(&d.val, vpad.data(), vpad.size())) return 1;
  return 0;
}

void free_ell(DevEll& e) { dev_free_all(e.pk, e.pk16, e.coef, e.col, e.val); }

void free_csr(DevCsr& d) {
  dev_free_all(d.sell_ptr, d.sell_pk, d.sell_dict, d.sell_diag, d.sell_col, d.sell_val, d.rowptr32, d.rowptr64, d.col, d.val);
}

// device copies of the images of host_pack.hpp
static int upload_ell(DevEll& e, const HostCsr& a, bool lds, const Switches& sw) {
  e = DevEll();
  const HostEll h = encode_ell(a, lds, !sw.ell_untyped, sw.ell16);
  e.nrow = h.nrow;
  e.pitch = h.pitch;
  e.width = h.width;
  e.typed = h.typed;
  // one 16-bit image per sector: in ownership order where the rows kernel owns column pairs (even nrow)
  const std::vector<uint32_t>& h16 = h.pk16o.empty() ? h.pk16 : h.pk16o;
  e.pitch16 = h.pk16o.empty() ? h.pitch : h.pitch16o;
  return dev_upload(&e.pk, h.pk.data(), h.pk.size()) || dev_upload(&e.coef, h.coef.data(), h.coef.size()) ||
         dev_upload(&e.pk16, h16.data(), h16.size()) || dev_upload(&e.col, h.col.data(), h.col.size()) ||
         dev_upload(&e.val, h.val.data(), h.val.size());
}

static int upload_sell(DevCsr& d, int64_t nrow, int64_t ncol, const int64_t* rowptr, const int32_t* col,
                       const double* val, int cplx, bool is_loc, const Switches& sw, double max_pad = 1.6) {
  if (sw.csr_nosell) return 0;
  const HostSell h = encode_sell(nrow, ncol, rowptr, col, val, cplx, is_loc, max_pad, !sw.csr_unpacked);
  if (!h.built) return 0;
  d.sell = 1;
  d.nslice = h.nslice;
  d.sell_packed = h.packed ? 1 : 0;
  return dev_upload(&d.sell_ptr, h.ptr.data(), h.ptr.size()) || dev_upload(&d.sell_pk, h.pk.data(), h.pk.size()) ||
         dev_upload(&d.sell_dict, h.dict.data(), h.dict.size()) || dev_upload(&d.sell_diag, h.diag.data(), h.diag.size()) ||
         dev_upload(&d.sell_col, h.col.data(), h.col.size()) || dev_upload(&d.sell_val, h.val.data(), h.val.size());
}

int finish_handle(edigpu_sector* s) {
  EDIGPU_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  return 0;
}

static void free_sb(DevSb* q) {
  if (!q) return;
  dev_free(q->urank); dev_free(q->ublist); dev_free(q->uslot); dev_free(q->rmap2); dev_free(q->up_vtab); dev_free(q->up_tloc);
  dev_free(q->e0); dev_free(q->ebw); dev_free(q->up_korb); dev_free(q->chunk_row); dev_free(q->chunk_slot); dev_free(q->cdesc_off);
  dev_free(q->cdesc); dev_free(q->dw_vtab); dev_free(q->dw_tloc); dev_free(q->dw_korb); dev_free(q->nd_dw);
  for (DevSb::Half& h : q->half) {
    dev_free(h.ublist32); dev_free(h.ugap); dev_free(h.uslot); dev_free(h.rmap2); dev_free(h.ebw);
  }
  delete q;
}

void free_ib(IbDev* p) {
  if (!p) return;
  free_sb(p->sb);
  p->sb = nullptr;
  dev_free(p->urank); dev_free(p->rmap2); dev_free(p->ublist); dev_free(p->up_vtab); dev_free(p->up_timp); dev_free(p->up_ebath);
  dev_free(p->xu); dev_free(p->ed); dev_free(p->impd); dev_free(p->pos); dev_free(p->colof); dev_free(p->chunk_row);
  dev_free(p->chunk_blk); dev_free(p->dcls); dev_free(p->dblist); dev_free(p->dmeta); dev_free(p->dw_vtab);
  dev_free(p->dw_timp); dev_free(p->ndcoef); dev_free(p->nd_dw); dev_free(p->nd_up);
  dev_free(p->up_pmask); dev_free(p->dw_pmask); dev_free(p->up_pt); dev_free(p->dw_pt);
  free_ell(p->pr.ell);
  dev_free(p->pr.eux);
  dev_free(p->urank_low);
  for (IbDevHalf& h : p->half) {
    dev_free(h.ublist); dev_free(h.utop); dev_free(h.rmap2);
  }
}

// Local-block tables (host_sb.hpp, kernels_sb.hip) on the layout of the impurity-block image d: when the sector is of that
// form and a geometry of the kernels fits, the product and the fused step of the device-resident loops run on them
// (Switches::sb off: keep the round-3 impurity-block kernels).
static int setup_sb(IbDev* d, const HostNormal& hn, const HostIb& h, const Switches& sw) {
  if (!sw.sb) return 0;
  const bool verbose = sw.sb_verbose;
  const int chunk_rows = sw.ib_rows;
  auto skip = [&](const std::string& why) {
    if (verbose) fprintf(stderr, "edigpu: no local-block tables: %s\n", why.c_str());
    return 0;
  };
  const bool split = h.nhalf == 2;  // rows staged in halves: the local-block ROWS kernel per half, the impurity-block columns kernel
  if (split) {
    // Opt-in (Switches::sb_split): measured at Ns = 17 the local-block rows kernel on half rows takes 3.30 + 3.15 ms against
    // 2.77 + 2.58 ms for the round-3 kernel (kernels_sb_impl.hpp, TOP) -- the gathers of the hop over the top level cost it
    // more than the cheaper walk gains.  Kept, tested (CPU shim and GPU), off.
    if (!sw.sb_split) return skip("rows staged in halves (EDIGPU_SB_SPLIT=1 takes the local-block rows kernel)");
  }
  const int nb0 = sb_nb0(h.norb);
  if (nb0 < 1 || hn.ns - h.norb - nb0 < 2) return skip("too few bath levels");
  const int slots = sb_rows_slots(hn, nb0, split);
  if (slots < 1) return skip("not of the local-block form");
  const int plen_rows = split ? std::max(h.half[0].npanels, h.half[1].npanels) * kIbPanel : h.npanels * kIbPanel;
  HostSb t;
  const int gs = sb_cols_gs(sw.sb_cw), waves = sb_cols_waves(sw.sb_cw);
  build_sb(hn, h, nb0, chunk_rows, 64 * slots, 1, waves, t, gs, sw.sb_amode);  // (the class stride of the row image: needed to choose the geometry)
  if (!t.valid) return skip(t.why);
  int nt = 0, nbt = 0;
  if (!sb_rows_config(h.norb, slots, plen_rows, t.rcs, sw.sb_nt, sw.sb_nbt, &nt, &nbt)) return skip("no geometry of the rows kernel fits");
  if (split && nbt > 4) return skip("rows staged in halves: more than 4 blocks per thread");
  build_sb(hn, h, nb0, chunk_rows, nt, nbt, waves, t, gs, sw.sb_amode);
  if (!t.valid) return skip(t.why);
  if (split && t.amode != 0) return skip("rows staged in halves: all-orbital walk only");
  std::unique_ptr<DevSb, void (*)(DevSb*)> q(new DevSb(), free_sb);
  q->nb0 = t.nb0;
  q->nloc = t.nloc;
  q->amode = t.amode;
  q->nbw_up = t.up.nbw;
  q->nbw_dw = t.dw.nbw;
  q->rows_nt = nt;
  q->rows_nbt = nbt;
  q->rimg_len = t.rimg_len;
  q->rcs = t.rcs;
  q->rows_lds = split ? sb_rows_lds(t.up.nbw - 1, t.rimg_len, true) : sb_rows_lds(t.up.nbw, t.rimg_len);
  q->nhalf = t.nhalf;
  q->lowbits = t.lowbits;
  q->nchunks = (int)t.chunk_row.size() - 1;
  q->max_chunk_rows = t.max_chunk_rows;
  q->max_chunk_slots = t.max_chunk_slots;
  q->cols_gs = t.cols_gs;
  q->cols_lds = sb_cols_lds(t.dw.nbw, t.nloc, t.max_chunk_rows, t.max_chunk_slots, t.cols_gs);
  if (q->rows_lds > 158 * 1024 || q->cols_lds > 158 * 1024) return skip("tables larger than the LDS");
  std::vector<uint32_t> rmap2(t.rmap.size() / 2);
  for (size_t i = 0; i < rmap2.size(); i++) rmap2[i] = (uint32_t)t.rmap[2 * i] | ((uint32_t)t.rmap[2 * i + 1] << 16);
  if (split) {
    for (int hh = 0; hh < 2; hh++) {
      const SbUpHalf& hf = t.half[hh];
      DevSb::Half& dh = q->half[hh];
      dh.panel0 = hf.panel0;
      dh.npanels = hf.npanels;
      std::vector<uint32_t> ub(hf.ublist.size()), rm(hf.rmap.size() / 2);
      for (size_t i = 0; i < ub.size(); i++) ub[i] = (uint32_t)hf.ublist[i] | ((uint32_t)hf.utop[i] << 16);
      for (size_t i = 0; i < rm.size(); i++) rm[i] = (uint32_t)hf.rmap[2 * i] | ((uint32_t)hf.rmap[2 * i + 1] << 16);
      if (dev_upload(&dh.ublist32, ub.data(), ub.size()) || dev_upload(&dh.ugap, hf.ugap.data(), hf.ugap.size()) ||
          dev_upload(&dh.uslot, hf.uslot.data(), hf.uslot.size()) || dev_upload(&dh.rmap2, rm.data(), rm.size()) ||
          dev_upload(&dh.ebw, hf.ebw.data(), hf.ebw.size()))
        return 1;
    }
  }
  if (dev_upload(&q->urank, t.urank.data(), t.urank.size()) ||
      (!split && (dev_upload(&q->ublist, t.ublist.data(), t.ublist.size()) ||
                  dev_upload(&q->uslot, t.uslot.data(), t.uslot.size()) || dev_upload(&q->rmap2, rmap2.data(), rmap2.size()))) ||
      dev_upload(&q->up_vtab, t.up.vtab.data(), t.up.vtab.size()) || dev_upload(&q->up_tloc, t.up.tloc.data(), t.up.tloc.size()) ||
      dev_upload(&q->e0, t.e0.data(), t.e0.size()) || dev_upload(&q->ebw, t.ebw.data(), t.ebw.size()) || dev_upload(&q->up_korb, t.up.korb.data(), t.up.korb.size()) ||
      dev_upload(&q->chunk_row, t.chunk_row.data(), t.chunk_row.size()) ||
      dev_upload(&q->chunk_slot, t.chunk_slot.data(), t.chunk_slot.size()) ||
      dev_upload(&q->cdesc_off, t.cdesc_off.data(), t.cdesc_off.size()) || dev_upload(&q->cdesc, t.cdesc.data(), t.cdesc.size()) ||
      dev_upload(&q->dw_vtab, t.dw.vtab.data(), t.dw.vtab.size()) || dev_upload(&q->dw_tloc, t.dw.tloc.data(), t.dw.tloc.size()) ||
      dev_upload(&q->dw_korb, t.dw.korb.data(), t.dw.korb.size()) || dev_upload(&q->nd_dw, t.nd_dw.data(), t.nd_dw.size()))
    return 1;
  if (verbose)
    fprintf(stderr, "edigpu: local-block tables: nb0 %d amode %d rows %d x %d cs %d (%d slots, %zu B LDS) cols low %d chunks %d (%zu B LDS)\n", t.nb0, t.amode,
            nt, nbt, t.rcs, slots, q->rows_lds, t.lowbits, q->nchunks, q->cols_lds);
  d->sb = q.release();
  return 0;
}

// Short rows (IbDev::PosRows): Hup and the diagonal table in POSITION order for the generic LDS row kernel, which then
// works on the padded panel layout beside the local-block columns kernel.  Built on request (Switches::posrows) when the
// sector has local-block tables with whole rows; for rows shorter than Switches::ib_min_row_bytes() the block image is then built for it.
static int setup_pos_rows(edigpu_sector* s, const HostNormal& hn, const HostIb& h) {
  IbDev* d = s->ib;
  if (!d || !d->sb || d->sb->nhalf != 1 || !s->factored || !hn.fac.valid) return 0;
  // Opt-in.  Measured on config 2: the plain product gains (0.110 against 0.119 ms: 0.43 against 0.40
  // of the peak) but the fused Lanczos step loses (0.166 against 0.158 ms per step, 6020 against 6350 it/s): on 16-column
  // panels a row is 215 pieces 439 KB apart, and the fused row kernel's five streams of them take 100-120 us where the
  // 128-column panels of the default loop (27 pieces per row) take 81.
  if (!s->sw.posrows) return 0;
  const int plen = d->plen;
  const int td = normal_pick_rows_per_block(plen, hn.dim_dw, s->sw.rows_td);
  if (td < 1) return 0;
  const HostCsr& up = s->h_up;
  HostCsr pu;
  pu.nrow = pu.ncol = plen;
  pu.rowptr.assign((size_t)plen + 1, 0);
  std::vector<int32_t> colof((size_t)plen, -1);
  for (int64_t i = 0; i < hn.dim_up; i++) colof[(size_t)h.pos[(size_t)i]] = (int32_t)i;
  for (int p = 0; p < plen; p++) {
    const int32_t i = colof[(size_t)p];
    pu.rowptr[(size_t)p + 1] = pu.rowptr[(size_t)p] + (i < 0 ? 0 : up.rowptr[(size_t)i + 1] - up.rowptr[(size_t)i]);
  }
  pu.col.resize((size_t)pu.rowptr[(size_t)plen]);
  pu.val.resize(pu.col.size());
  for (int p = 0; p < plen; p++) {
    const int32_t i = colof[(size_t)p];
    if (i < 0) continue;
    int64_t at = pu.rowptr[(size_t)p];
    for (int64_t q = up.rowptr[(size_t)i]; q < up.rowptr[(size_t)i + 1]; q++, at++) {
      pu.col[(size_t)at] = h.pos[(size_t)up.col[(size_t)q]];
      pu.val[(size_t)at] = up.val[(size_t)q];
    }
  }
  if (upload_ell(d->pr.ell, pu, true, s->sw)) return 1;
  if (!d->pr.ell.pk || !d->pr.ell.typed) {  // the fast path of the row kernel only
    free_ell(d->pr.ell);
    d->pr.ell = DevEll();
    return 0;
  }
  const size_t nimp = hn.fac.eux.size() / (size_t)hn.dim_up;
  std::vector<double> ex(nimp * (size_t)plen, 0.0);
  for (size_t c = 0; c < nimp; c++)
    for (int64_t i = 0; i < hn.dim_up; i++) ex[c * (size_t)plen + (size_t)h.pos[(size_t)i]] = hn.fac.eux[c * (size_t)hn.dim_up + (size_t)i];
  if (dev_upload(&d->pr.eux, ex.data(), ex.size())) return 1;
  d->pr.td = td;
  d->pr.on = true;
  if (s->sw.sb_verbose) fprintf(stderr, "edigpu: rows half on the generic row kernel in position order (plen %d, %d rows per workgroup, ELL width %d)\n", plen, td, d->pr.ell.width);
  return 0;
}

// device copy of the impurity-block image; leaves s->ib null (and returns 0) when the sector is not of that form
static int setup_ib(edigpu_sector* s, const HostNormal& hn) {
  const Switches& sw = s->sw;
  HostIb h;
  // Rows whose image does not fit the LDS beside the tables are staged one half at a time (host_ib.hpp IbUpHalf);
  // Switches::ib_split forces that form on any sector (tests) or leaves such sectors to the generic kernels.
  const int lds_budget = !sw.ib_split ? 156 * 1024 : *sw.ib_split != 0 ? -1 : 0;
  build_ib(hn, sw.ib_rows, h, lds_budget);
  if (!h.valid) {
    if (sw.ib_verbose) fprintf(stderr, "edigpu: no impurity-block image: %s\n", h.why.c_str());
    return 0;
  }
  int nt = 0, nbt = 0;
  const int plen = h.npanels * kIbPanel;
  size_t rows_lds = 0;
  if (h.nhalf == 2) {
    const IbUpHalf &a = h.half[0], &b = h.half[1];
    const int rimg = std::max(a.rimg_len, b.rimg_len);
    if (!ib_rows_config(h.norb, h.up.nb - 1, (int)std::max(a.ublist.size(), b.ublist.size()),
                        std::max(a.npanels, b.npanels) * kIbPanel, rimg, sw.ib_nt, &nt, &nbt, true))
      return 0;
    rows_lds = ib_rows_lds_bytes(h.up.nb - 1, rimg);
  } else {
    if (!ib_rows_config(h.norb, h.up.nb, (int)h.ublist.size(), plen, h.rimg_len, sw.ib_nt, &nt, &nbt)) return 0;
    rows_lds = ib_rows_lds_bytes(h.up.nb, h.rimg_len);
  }
  int mcb = 8;
  for (size_t c = 0; c + 1 < h.chunk_blk.size(); c++) mcb = std::max(mcb, h.chunk_blk[c + 1] - h.chunk_blk[c]);
  std::unique_ptr<IbDev> d(new IbDev());
  d->norb = h.norb;
  d->nb_up = h.up.nb;
  d->nb_dw = h.dw.nb;
  d->npanels = h.npanels;
  d->plen = plen;
  d->nlist = (int)h.ublist.size();
  for (int i = 0; i < 5; i++) d->ucls[i] = h.ucls[std::min(i, h.norb + 1)];
  d->lowbits = h.lowbits;
  d->nchunks = (int)h.chunk_row.size() - 1;
  d->max_chunk_rows = h.max_chunk_rows;
  d->max_chunk_blocks = mcb;
  // workgroups per chunk of the columns kernel.  Two per chunk make one panel's tasks cover the 64 workgroup slots of an
  // XCD, so that a single panel is in flight per L2 -- measured SLOWER (Ns = 16: 2.79 against 2.42 ms per product,
  // Ns = 15: 0.69 against 0.64): staging the chunk twice costs more than the gathers that then hit the L2 save.
  d->nsub = sw.ib_nsub;
  d->cols2 = sw.ib_cols2;
  d->nterms = h.nterms;
  d->dim_up = hn.dim_up;
  d->dim_dw = hn.dim_dw;
  d->ps = hn.dim_dw * kIbPanel;
  d->ps += (int64_t)sw.ib_pspad / 2 * 2;  // doubles between two panels (tuning)
  d->len = (int64_t)h.npanels * d->ps;
  d->rows_nt = nt;
  d->rows_nbt = nbt;
  d->rows_lds = rows_lds;
  for (int i = 0; i < 5; i++) {
    d->rcb[i] = h.rcb[i];
    d->rcs[i] = h.rcs[i];
  }
  d->rimg_len = h.rimg_len;
  std::vector<uint32_t> rmap2((size_t)plen / 2);
  for (size_t i = 0; i < rmap2.size(); i++) rmap2[i] = (uint32_t)h.rmap[2 * i] | ((uint32_t)h.rmap[2 * i + 1] << 16);
  d->cols_lds = ib_cols_lds_bytes(h.dw.nb, h.max_chunk_rows, mcb);
  if (d->cols_lds > 158 * 1024) return 0;
  std::vector<int32_t> colof((size_t)plen, -1);
  for (int64_t i = 0; i < hn.dim_up; i++) colof[(size_t)h.pos[(size_t)i]] = (int32_t)i;
  IbDev* p = d.get();
  if (dev_upload(&p->urank, h.urank.data(), h.urank.size()) || dev_upload(&p->rmap2, rmap2.data(), rmap2.size()) ||
      dev_upload(&p->ublist, h.ublist.data(), h.ublist.size()) ||
      dev_upload(&p->up_vtab, h.up.vtab.data(), h.up.vtab.size()) || dev_upload(&p->up_timp, h.up.timp.data(), h.up.timp.size()) ||
      dev_upload(&p->up_ebath, h.up.ebath.data(), h.up.ebath.size()) || dev_upload(&p->xu, h.xu.data(), h.xu.size()) ||
      dev_upload(&p->ed, h.ed.data(), h.ed.size()) || dev_upload(&p->impd, h.impd.data(), h.impd.size()) ||
      dev_upload(&p->pos, h.pos.data(), h.pos.size()) || dev_upload(&p->colof, colof.data(), colof.size()) ||
      dev_upload(&p->chunk_row, h.chunk_row.data(), h.chunk_row.size()) ||
      dev_upload(&p->chunk_blk, h.chunk_blk.data(), h.chunk_blk.size()) || dev_upload(&p->dcls, h.dcls.data(), h.dcls.size()) ||
      dev_upload(&p->dblist, h.dblist.data(), h.dblist.size()) || dev_upload(&p->dmeta, h.dmeta.data(), h.dmeta.size()) ||
      dev_upload(&p->dw_vtab, h.dw.vtab.data(), h.dw.vtab.size()) || dev_upload(&p->dw_timp, h.dw.timp.data(), h.dw.timp.size()) ||
      dev_upload(&p->nd_dw, h.nd_dw.data(), h.nd_dw.size()) || dev_upload(&p->nd_up, h.nd_up.data(), h.nd_up.size())) {
    free_ib(p);
    return 1;
  }
  p->up_np = (int)h.up.pmask.size();
  p->dw_np = (int)h.dw.pmask.size();
  if ((p->up_np > 0 && (dev_upload(&p->up_pmask, h.up.pmask.data(), h.up.pmask.size()) || dev_upload(&p->up_pt, h.up.pt.data(), h.up.pt.size()))) ||
      (p->dw_np > 0 && (dev_upload(&p->dw_pmask, h.dw.pmask.data(), h.dw.pmask.size()) || dev_upload(&p->dw_pt, h.dw.pt.data(), h.dw.pt.size())))) {
    free_ib(p);
    return 1;
  }
  if (h.nterms > 0 && dev_upload(&p->ndcoef, h.ndcoef.data(), h.ndcoef.size())) {
    free_ib(p);
    return 1;
  }
  p->nhalf = h.nhalf;
  if (h.nhalf == 2) {
    p->top_eps = h.up.vtab[(size_t)(h.up.nb - 1) * 4 + 3];
    int rc = dev_upload(&p->urank_low, h.urank_low.data(), h.urank_low.size());
    for (int k = 0; k < 2 && !rc; k++) {
      const IbUpHalf& src = h.half[k];
      IbDevHalf& dst = p->half[k];
      dst.panel0 = src.panel0;
      dst.npanels = src.npanels;
      dst.nlist = (int)src.ublist.size();
      dst.rimg_len = src.rimg_len;
      for (int i = 0; i < 5; i++) {
        dst.ucls[i] = src.ucls[std::min(i, h.norb + 1)];
        dst.rcb[i] = src.rcb[i];
        dst.rcs[i] = src.rcs[i];
      }
      std::vector<uint32_t> m2((size_t)src.npanels * kIbPanel / 2);
      for (size_t i = 0; i < m2.size(); i++) m2[i] = (uint32_t)src.rmap[2 * i] | ((uint32_t)src.rmap[2 * i + 1] << 16);
      rc = dev_upload(&dst.ublist, src.ublist.data(), src.ublist.size()) || dev_upload(&dst.utop, src.utop.data(), src.utop.size()) ||
           dev_upload(&dst.rmap2, m2.data(), m2.size());
    }
    if (rc) {
      free_ib(p);
      return 1;
    }
  }
  s->ib = d.release();
  if (setup_sb(s->ib, hn, h, sw)) return 1;
  return setup_pos_rows(s, hn, h);
}

int setup_normal(edigpu_sector* s, int64_t dim_up, int64_t dim_dw, int64_t dw_first,
                 int64_t dw_count, const double* hd, const HostCsr& up, const HostCsr& dw,
                 const int64_t* nd_rowptr, const int32_t* nd_col, const double* nd_val,
                 HostNormal* built) {
  s->kind = kNormal;
  s->is_complex = 0;
  s->device = current_device();
  s->dim_up = dim_up;
  s->dim_dw = dim_dw;
  s->dw_first = dw_first;
  s->dw_count = dw_count;
  s->dim = dim_up * dim_dw;
  s->nloc = dim_up * dw_count;
  s->row_first = dw_first * dim_up;
  s->h_up = up;
  s->h_dw = dw;
  std::vector<int32_t> tile_starts;  // row chunks of the LDS-tiled panel sweep (empty: not planned)
  const Switches& sw = s->sw;
  s->rows_per_block = normal_pick_rows_per_block(dim_up, dw_count, sw.rows_td);
  // Rows longer than the LDS (rows_per_block == 0): staged in column parts when the typed LDS image exists
  // (normal_rows_kernel SPLIT); Switches::row_split forces it on any sector (tests) or switches it off.
  {
    int parts = 0;
    if (sw.row_split) {
      parts = *sw.row_split;
      if (parts > 1) s->rows_per_block = 0;
    } else if (s->rows_per_block == 0) {
      parts = (int)(((dim_up + 2) * 8 + 140 * 1024 - 1) / (140 * 1024));
    }
    if (s->rows_per_block == 0 && parts > 1 && dim_up >= 4 * parts) {
      if (upload_ell(s->up_ell, up, true, sw)) return 1;
      if (s->up_ell.typed && s->up_ell.pk) {
        s->row_split = parts;
      } else {
        free_ell(s->up_ell);
        s->up_ell = DevEll();
      }
    }
  }
  if (s->row_split == 1 && upload_ell(s->up_ell, up, s->rows_per_block != 0, sw)) return 1;
  if (upload_csr(s->dw, dim_dw, dw.rowptr.data(), dw.col.data(), dw.val.data(), 0)) return 1;
  for (int64_t i = 0; i < dim_dw; i++)
    s->dw_maxrow = std::max<int>(s->dw_maxrow, (int)(dw.rowptr[i + 1] - dw.rowptr[i]));
  {
    // panel sweep variant (kernels_panel.hip).  Measured: cache-resident sectors are 13 % SLOWER with the two-column
    // panels (fewer, fatter waves), hence the size gate Switches::panel_vec2_min (tests force the large-sector kernels on
    // small sectors).  Switches::tile_rows sets the chunk length (KiB of LDS per workgroup), at most kTileMaxRows of
    // kernels_panel.hip: 4 rows per wave (their results live in registers), 16 waves.
    if (sw.panel_vec2 && dim_up >= 2 && dim_up * dw_count >= sw.panel_vec2_min) s->panel_mode = 1;
    if (s->panel_mode == 1 && sw.panel_tile && dw_count > 0 && dim_dw < ((int64_t)1 << 24)) {
      plan_tile_chunks(dw, dw_first, dw_count, sw.tile_rows, tile_starts, s->tile_rows);
      s->tile_nchunks = (int)tile_starts.size() - 1;
      if (dev_upload(&s->d_tile_chunks, tile_starts.data(), tile_starts.size())) return 1;
      s->panel_mode = 2;
    }
  }
  s->has_nd = nd_rowptr != nullptr && nd_rowptr[s->nloc] > 0;
  s->nd_nnz = s->has_nd ? nd_rowptr[s->nloc] : 0;
  if (built && !nd_rowptr) {  // factored-only build: no explicit arrays were made
    s->has_nd = built->has_nd && built->nd_nnz > 0;
    s->nd_nnz = s->has_nd ? built->nd_nnz : 0;
  }
  // library-built sectors keep the diagonal and Hnd in factored form on the device (the explicit
  // arrays stay on the host for export); Switches::normal_explicit forces the explicit image.
  if (built && built->fac.valid && built->fac.nterms <= 16 && !sw.normal_explicit) {
    const HostFactored& f = built->fac;
    s->factored = 1;
    s->fac_nimp = f.nimp;
    s->fac_nterms = f.nterms;
    if (dev_upload(&s->d_eux, f.eux.data(), f.eux.size())) return 1;
    if (dev_upload(&s->d_ed, f.ed.data(), f.ed.size())) return 1;
    if (dev_upload(&s->d_impd, f.impd.data(), f.impd.size())) return 1;
    if (f.nterms > 0) {
      if (dev_upload(&s->d_ndcoef, f.coef.data(), f.coef.size())) return 1;
      if (dev_upload(&s->d_jup, f.jup.data(), f.jup.size())) return 1;
      s->col_halo = factored_col_halo(f, dim_up);
      if (dev_upload(&s->d_jdw, f.jdw.data(), f.jdw.size())) return 1;
      // merged per-local-row list for the panel kernel: Hdw entries (tag 0) + applicable Hnd terms
      if (dim_dw < ((int64_t)1 << 24) && f.nterms < 127) {
        const HostMergedList m = merge_dw_lists(dw, f, dw_first, dw_count, dim_dw);
        if (dev_upload(&s->d_mx_rowptr, m.rowptr.data(), m.rowptr.size()) || dev_upload(&s->d_mx_col, m.col.data(), m.col.size()) ||
            dev_upload(&s->d_mx_val, m.val.data(), m.val.size()))
          return 1;
      }
    }
    s->h_hd = std::move(built->hd);
    s->h_nd = std::move(built->nd);
  } else {
    if (dev_upload(&s->d_hd, hd, (size_t)s->nloc)) return 1;
    if (s->has_nd && upload_csr(s->nd, s->nloc, nd_rowptr, nd_col, nd_val, 0)) return 1;
    // Hnd as its own SELL pass after the panel sweep (global columns): keeps the row kernel free of the CSR
    // row pointers and lets the Lanczos step stay fused (the dot partials move to this last pass)
    if (s->has_nd && !sw.nd_in_rows &&
        upload_sell(s->nd, s->nloc, dim_up * dim_dw, nd_rowptr, nd_col, nd_val, 0, false, sw, 16.0))
      return 1;
  }
  if (s->panel_mode == 2) {
    // per-row lists of the tiled sweep, with the factored Hnd terms when the merged list above exists
    const HostFactored* f = (s->factored && built) ? &built->fac : nullptr;
    const bool with_nd = f && f->nterms > 0 && s->d_mx_rowptr != nullptr;
    const HostTileLists l = build_tile_lists(dw, dim_dw, dw_first, dw_count, tile_starts, with_nd ? f : nullptr);
    s->tile_list_cap = l.list_cap;
    const std::vector<HostInt4> meta = tile_meta_live(l, dw_first);  // the kernel gathers the live outside entries only
    if (dev_upload(&s->d_tile_lbeg, l.lbeg.data(), l.lbeg.size()) || dev_upload(&s->d_tl_meta, as_int4(meta), meta.size()) ||
        dev_upload(&s->d_tl_col, l.col.data(), l.col.size()) || dev_upload(&s->d_tl_val, l.val.data(), l.val.size()))
      return 1;
    s->tl_has_nd = l.has_nd ? 1 : 0;
  }
  // Impurity-block image (host_ib.hpp, kernels_ib.hip): whole sectors built from a model whose hops connect impurity
  // levels with single bath levels (normal / hybrid baths), <= 3 orbitals.  The device-resident Lanczos loops then run
  // on its padded 16-column panel layout and its two kernels.  Measured (r3): 0.61 against 0.85 ms per product at
  // Ns = 15, 2.4 against 3.3 ms at Ns = 16, but 0.18 against 0.13 ms on config 2, whose 27 KB rows leave the generic
  // row kernel four workgroups per CU -- so the default takes it for rows of more than Switches::ib_min_row_bytes()
  // (40 KB) in sectors of at least Switches::ib_min elements (tests force it on small ones with 0, which also lifts the
  // row gate).
  if (s->factored && built && built->norb > 0 && dw_first == 0 && dw_count == dim_dw) {
    const int64_t min_rows = sw.ib_min;
    // Replica / general baths (hops between the bath levels of a replica, host_ib.hpp IbSide::pmask): the image and its
    // kernels hold them as pair hops of whole blocks -- tested, golden-pinned -- but every lane runs through every pair
    // (half of them idle), which costs as much as the walk over the levels: measured on the 3-orbital x 4-replica sector
    // of Ns = 15 the product takes 1.16 ms on the blocks against 0.81 ms on the generic kernels.  So the default keeps
    // such sectors on the generic kernels; Switches::ib_pairs (or ib_min == 0, the tests) takes the image.
    bool pairs = false;
    for (int sp = 0; sp < 2 && !pairs; sp++) {
      const std::vector<double>& a = built->ob_a[sp];
      const int ns = built->ns;
      if ((int)a.size() == ns * ns)
        for (int p = built->norb; p < ns && !pairs; p++)
          for (int q = p + 1; q < ns; q++)
            if (a[(size_t)p * ns + q] != 0.0) {
              pairs = true;
              break;
            }
    }
    const bool pairs_ok = !pairs || min_rows == 0 || sw.ib_pairs;
    // Rows below ib_min_row_bytes(): the block ROWS kernels lose to the generic LDS row kernel there; the image is still built
    // when that kernel can take the rows half on the image's layout (setup_pos_rows), and dropped again when it cannot.
    const bool short_rows = dim_up * 8 < sw.ib_min_row_bytes();
    if (sw.ib && pairs_ok && s->nloc >= min_rows && (!short_rows || sw.posrows) && !sw.lanczos_unfused && setup_ib(s, *built))
      return 1;
    if (s->ib && short_rows && !s->ib->pr.on) {
      free_ib(s->ib);
      delete s->ib;
      s->ib = nullptr;
    }
  }
  // Panel-major vector layout for the device-resident Lanczos loop (normal_args.hpp): large
  // factored whole sectors whose rows fit the LDS row kernel.  Default: 128-column panels (1 KiB line-aligned segments)
  // swept by the LDS-tiled kernel -- measured 6 % (config 2), 14 % (Ns = 15) and 8 % (Ns = 16) faster per product than
  // the same kernel on the natural layout, whose segments start at arbitrary 8-byte offsets.  Panels of 16 / 32 / 64
  // columns (Switches::blocked_w) take the narrow-panel sweep (normal_dw_blk_kernel: panels that stay in one L2, fetch
  // traffic 1.1-1.9x of V + result instead of 1.8-5x, but bound by the L2's gather throughput and 10-60 % slower: an
  // experiment that is kept, tested, off).
  if (!s->ib && s->factored && built && dw_first == 0 && dw_count == dim_dw && s->rows_per_block >= 1 && s->row_split == 1 &&
      dim_dw <= 65535 && dim_up >= 64) {
    const bool on = sw.blocked;
    const int64_t min_rows = sw.blocked_min;
    const int shift = sw.blocked_shift();
    const HostFactored& f = built->fac;
    if (on && shift == 7 && s->nloc >= min_rows && s->panel_mode == 2 && (f.nterms == 0 || s->tl_has_nd)) {
      // 128-column panels: the tiled sweep and its lists as they are, on line-aligned contiguous panels
      s->blk_shift = 7;
      s->blk_tail_balance = sw.tile_balance;
      s->blk_rows = s->tile_rows;
      s->blk_ps = dim_dw << 7;
      s->blk_len = ((dim_up + 127) >> 7) * s->blk_ps;
    } else if (on && shift && shift < 7 && s->nloc >= min_rows && f.nterms <= 16) {
      // narrow panels: lists over LDS blocks of Switches::blocked_lds_kb KiB of staged segments
      const HostBlockLists b = build_block_lists(dw, f, dim_dw, shift, sw.blocked_lds_kb);
      if (b.fits) {
        s->blk_list_cap = b.list_cap;
        if (dev_upload(&s->d_bl_lend, b.lend.data(), b.lend.size()) || dev_upload(&s->d_bl_meta, as_int4(b.meta), b.meta.size()) ||
            dev_upload(&s->d_bl_ent, b.ent.data(), b.ent.size()) || dev_upload(&s->d_bl_wtab, b.wtab.data(), b.wtab.size()))
          return 1;
        s->blk_shift = shift;
        s->blk_rows = b.rows;
        s->blk_ps = dim_dw << shift;
        s->blk_len = ((dim_up + ((int64_t)1 << shift) - 1) >> shift) * s->blk_ps;
      }
    }
  }
  return finish_handle(s);
}

// split a local-row CSR with global columns into shard-local and non-local blocks
int setup_flat(edigpu_sector* s, int64_t nrow_local, int64_t ncol_global, int64_t row_first,
               const int64_t* rowptr, const int32_t* col, const double* val, int cplx) {
  s->kind = kFlat;
  s->is_complex = cplx;
  s->device = current_device();
  s->dim = ncol_global;
  s->nloc = nrow_local;
  s->row_first = row_first;
  const int w = cplx ? 2 : 1;
  const int64_t lo = row_first, hi = row_first + nrow_local;
  std::vector<int64_t> rpl((size_t)nrow_local + 1, 0), rpn((size_t)nrow_local + 1, 0);
  for (int64_t i = 0; i < nrow_local; i++) {
    int64_t nl = 0;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; k++)
      if (col[k] >= lo && col[k] < hi) nl++;
    rpl[i + 1] = rpl[i] + nl;
    rpn[i + 1] = rpn[i] + (rowptr[i + 1] - rowptr[i] - nl);
  }
  std::vector<int32_t> cl((size_t)rpl[nrow_local]), cn((size_t)rpn[nrow_local]);
  std::vector<double> vl((size_t)rpl[nrow_local] * w), vn((size_t)rpn[nrow_local] * w);
  for (int64_t i = 0; i < nrow_local; i++) {
    int64_t pl = rpl[i], pn = rpn[i];
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; k++) {
      if (col[k] >= lo && col[k] < hi) {
        cl[pl] = (int32_t)(col[k] - lo);
        for (int q = 0; q < w; q++) vl[pl * w + q] = val[k * w + q];
        pl++;
      } else {
        cn[pn] = col[k];
        for (int q = 0; q < w; q++) vn[pn * w + q] = val[k * w + q];
        pn++;
      }
    }
  }
  if (upload_csr(s->loc, nrow_local, rpl.data(), cl.data(), vl.data(), cplx)) return 1;
  if (upload_csr(s->nonloc, nrow_local, rpn.data(), cn.data(), vn.data(), cplx)) return 1;
  if (upload_sell(s->loc, nrow_local, nrow_local, rpl.data(), cl.data(), vl.data(), cplx, true, s->sw)) return 1;
  if (upload_sell(s->nonloc, nrow_local, ncol_global, rpn.data(), cn.data(), vn.data(), cplx, false, s->sw)) return 1;
  return finish_handle(s);
}

// ed_total_ud = F sector: factor matrices as ELL ([slot][row] per axis, padding col = own row, val = 0),
// diagonal explicit (hd != null) or as per-axis tables + impurity table
int setup_orbs(edigpu_sector* s, const HostOrbs& ho, const double* hd) {
  s->kind = kOrbs;
  s->is_complex = 0;
  s->device = current_device();
  s->dim = s->nloc = ho.dim;
  s->row_first = 0;
  OrbsArgs& a = s->orbs;
  a = OrbsArgs();
  a.naxes = ho.naxes;
  a.dim = ho.dim;
  std::vector<int32_t> ecol;
  std::vector<double> eval, eax;
  std::vector<uint8_t> imp;
  int64_t stride = 1;
  for (int k = 0; k < ho.naxes; k++) {
    const int64_t d = ho.dims[k];
    a.dims[k] = d;
    a.stride[k] = stride;
    stride *= d;
    const HostCsr& f = ho.fac[k];
    int w = 0;
    for (int64_t i = 0; i < d; i++) w = std::max<int>(w, (int)(f.rowptr[i + 1] - f.rowptr[i]));
    a.width[k] = w;
    a.elloff[k] = (int64_t)ecol.size();
    const size_t base = ecol.size();
    ecol.resize(base + (size_t)w * d);
    eval.resize(base + (size_t)w * d, 0.0);
    for (int sl = 0; sl < w; sl++)
      for (int64_t i = 0; i < d; i++) ecol[base + (size_t)sl * d + i] = (int32_t)i;
    for (int64_t i = 0; i < d; i++) {
      int sl = 0;
      for (int64_t q = f.rowptr[i]; q < f.rowptr[i + 1]; q++, sl++) {
        ecol[base + (size_t)sl * d + i] = f.col[q];
        eval[base + (size_t)sl * d + i] = f.val[q];
      }
    }
    a.off[k] = (int)eax.size();
    if (!hd) {
      eax.insert(eax.end(), ho.eax[k].begin(), ho.eax[k].end());
      imp.insert(imp.end(), ho.impbit[k].begin(), ho.impbit[k].end());
    }
  }
  if (ecol.empty()) {  // no off-diagonal element at all: keep valid pointers
    ecol.push_back(0);
    eval.push_back(0.0);
  }
  int32_t* dcol = nullptr;
  double *dval = nullptr, *dhd = nullptr, *deax = nullptr, *dx = nullptr;
  uint8_t* dimp = nullptr;
  if (dev_upload(&dcol, ecol.data(), ecol.size())) return 1;
  a.ell_col = dcol;
  if (dev_upload(&dval, eval.data(), eval.size())) return 1;
  a.ell_val = dval;
  if (hd) {
    if (dev_upload(&dhd, hd, (size_t)ho.dim)) return 1;
    a.hd = dhd;
  } else {
    if (dev_upload(&deax, eax.data(), eax.size())) return 1;
    a.eax = deax;
    if (dev_upload(&dimp, imp.data(), imp.size())) return 1;
    a.impbit = dimp;
    if (dev_upload(&dx, ho.xtab.data(), ho.xtab.size())) return 1;
    a.xtab = dx;
  }
  s->h_orbs_fac = ho.fac;
  return finish_handle(s);
}

// Stored flat image generated on the device from the on-the-fly description (kernels_build.hip).
// Returns 0 = built, 2 = not applicable (caller falls back to the host CSR builder), 1 = error.
int build_flat_on_device(edigpu_sector* s, const HostDirect& hd) {
  const int nterms = (int)hd.terms.size();
  const int64_t nrow = hd.row_count;
  if (nrow == 0 || hd.dim >= ((int64_t)1 << 24)) return 2;  // 24-bit columns in the packed words
  // ---- value dictionary: ids (2j, 2j+1) = (+v_j, -v_j), j >= 1; ids 0, 1 = 0.0 (padding) ----
  std::vector<double> dict(4, 0.0);
  std::vector<uint8_t> vid((size_t)2 * std::max(nterms, 1), 0);
  auto id_of = [&](double re, double im) -> int {
    const size_t n = dict.size() / 2;
    for (size_t k = 2; k < n; k++)
      if (dict[2 * k] == re && dict[2 * k + 1] == im) return (int)k;
    if (n + 2 > 256) return -1;
    dict.push_back(re);
    dict.push_back(im);
    dict.push_back(-re);
    dict.push_back(-im);
    return (int)n;
  };
  for (int t = 0; t < nterms; t++) {
    const DirectTerm& tm = hd.terms[t];
    const int f = id_of(tm.cre, tm.cim);
    const int r = tm.pair ? id_of(tm.c2re, tm.c2im) : f;
    if (f < 0 || r < 0) return 2;
    vid[2 * t] = (uint8_t)f;
    vid[2 * t + 1] = (uint8_t)r;
  }
  dict.resize(512, 0.0);
  // ---- temporaries on the device (the direct image + work arrays) ----
  struct Tmp {
    int32_t *states = nullptr, *offdw = nullptr, *rkup = nullptr, *wl = nullptr, *wn = nullptr;
    DirectTerm* terms = nullptr;
    uint8_t* vid = nullptr;
    double *dtab = nullptr, *xtab = nullptr;
    unsigned long long* totals = nullptr;
    ~Tmp() { dev_free_all(states, offdw, rkup, wl, wn, terms, vid, dtab, xtab, totals); }
  } t;
  const int64_t nslice = (nrow + 63) / 64;
  int rc = dev_upload(&t.states, hd.states.data(), hd.states.size());
  rc |= dev_upload(&t.offdw, hd.off_dw.data(), hd.off_dw.size());
  rc |= dev_upload(&t.rkup, hd.rk_up.data(), hd.rk_up.size());
  if (nterms) rc |= dev_upload(&t.terms, hd.terms.data(), hd.terms.size());
  rc |= dev_upload(&t.vid, vid.data(), vid.size());
  rc |= dev_upload(&t.dtab, hd.dtab.data(), hd.dtab.size());
  rc |= dev_upload(&t.xtab, hd.xtab.data(), hd.xtab.size());
  if (rc) return 1;
  EDIGPU_HIP(hipMalloc((void**)&t.wl, (size_t)nslice * sizeof(int32_t)));
  EDIGPU_HIP(hipMalloc((void**)&t.wn, (size_t)nslice * sizeof(int32_t)));
  EDIGPU_HIP(hipMalloc((void**)&t.totals, 4 * sizeof(unsigned long long)));
  EDIGPU_HIP(hipMemset(t.totals, 0, 4 * sizeof(unsigned long long)));
  BuildArgs a;
  a.nrow = nrow;
  a.row_first = hd.row_first;
  a.lo = hd.row_first;
  a.hi = hd.row_first + nrow;
  a.ns = hd.ns;
  a.norb = hd.norb;
  a.nterms = nterms;
  a.states = t.states;
  a.off_dw = t.offdw;
  a.rk_up = t.rkup;
  a.terms = t.terms;
  a.vid = t.vid;
  a.dtab = t.dtab;
  a.xtab = t.xtab;
  if (launch_build_count(a, t.wl, t.wn, t.totals, nullptr)) return 1;
  std::vector<int32_t> wl((size_t)nslice), wn((size_t)nslice);
  unsigned long long tot[4];
  EDIGPU_HIP(hipMemcpy(wl.data(), t.wl, wl.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  EDIGPU_HIP(hipMemcpy(wn.data(), t.wn, wn.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  EDIGPU_HIP(hipMemcpy(tot, t.totals, sizeof(tot), hipMemcpyDeviceToHost));
  const int maxl = (int)(tot[2] & 0xFFFFFFFFull), maxn = (int)(tot[3] & 0xFFFFFFFFull);
  if (maxl > 160 || maxn > 160) return 2;  // rows too long for the LDS sort buffers
  auto finish = [&](DevCsr& d, const std::vector<int32_t>& w, int64_t nent, int maxlen, int which) -> int {
    d = DevCsr();
    d.nrow = nrow;
    d.nnz = nent + (which == 0 ? nrow : 0);  // the loc block also holds the diagonal
    d.avg_row = (double)d.nnz / (double)nrow;
    if (nent == 0 && which == 1) return 0;   // no non-local block on a single shard
    std::vector<int32_t> sp((size_t)nslice + 1, 0);
    int64_t acc = 0;
    for (int64_t k = 0; k < nslice; k++) {
      acc += w[k];
      if (acc >= ((int64_t)1 << 31) / 64) return 2;
      sp[k + 1] = (int32_t)acc;
    }
    if (nent > 0 && (double)acc * 64.0 > 1.6 * (double)nent) return 2;  // too ragged for SELL
    d.sell = 1;
    d.sell_packed = 1;
    d.nslice = nslice;
    if (dev_upload(&d.sell_ptr, sp.data(), sp.size())) return 1;
    if (dev_upload(&d.sell_dict, dict.data(), dict.size())) return 1;
    EDIGPU_HIP(hipMalloc((void**)&d.sell_pk, (size_t)std::max<int64_t>(acc, 1) * 64 * sizeof(uint32_t)));
    if (which == 0) EDIGPU_HIP(hipMalloc((void**)&d.sell_diag, (size_t)nrow * 2 * sizeof(double)));
    return launch_build_fill(a, which, maxlen, d.sell_ptr, d.sell_pk, d.sell_diag, nullptr);
  };
  int r0 = finish(s->loc, wl, (int64_t)tot[0], maxl, 0);
  if (r0) return r0;
  int r1 = finish(s->nonloc, wn, (int64_t)tot[1], maxn, 1);
  if (r1) return r1;
  EDIGPU_HIP(hipDeviceSynchronize());
  return 0;
}

}  // namespace edigpu
