// Test-only shim: the image encoders of the generic kernels (csrc/host_pack.cpp) behind a C interface, so that
// tests/test_host_pack.py can decode every image the way its kernel does and compare it with the CSR it was made from.
// An encoder call keeps its result here; the getters copy the vectors out.  Compiled with g++; never part of the product.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "host_build.hpp"
#include "host_pack.hpp"
#include "switches.cpp"  // (compiled into this shim: it samples the environment at every call, like the C-ABI builders)
using namespace edigpu;

namespace {

std::string g_err;
HostNormal g_hn;
HostEll g_ell;
HostSell g_sell;
HostMergedList g_mx;
HostTileLists g_tl;
HostBlockLists g_bl;

HostCsr make_csr(int64_t nrow, const int64_t* rowptr, const int32_t* col, const double* val) {
  HostCsr a;
  a.nrow = a.ncol = nrow;
  a.rowptr.assign(rowptr, rowptr + nrow + 1);
  a.col.assign(col, col + rowptr[nrow]);
  a.val.assign(val, val + rowptr[nrow]);
  return a;
}

HostFactored make_fac(int64_t dim_dw, int nterms, const double* coef, const uint32_t* jdw) {
  HostFactored f;
  f.valid = true;
  f.nterms = nterms;
  if (nterms > 0) {
    f.coef.assign(coef, coef + nterms);
    f.jdw.assign(jdw, jdw + (size_t)nterms * dim_dw);
  }
  return f;
}

template <class T>
void copy_out(T* dst, const std::vector<T>& v) {
  if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(T));
}

}  // namespace

extern "C" {

const char* hp_error() { return g_err.c_str(); }

// the sector (nup, ndw) of a model; dims: dim_up, dim_dw, nnz(Hup), nnz(Hdw), Hnd terms
int hp_build_normal(const edigpu_model* m, int nup, int ndw, int64_t* dims) {
  g_hn = HostNormal();
  g_err = build_normal(*m, nup, ndw, 0, -1, g_hn, false, !Switches::sample().nd_no_merge);
  if (!g_err.empty()) return 1;
  dims[0] = g_hn.dim_up;
  dims[1] = g_hn.dim_dw;
  dims[2] = g_hn.up.nnz();
  dims[3] = g_hn.dw.nnz();
  dims[4] = g_hn.fac.valid ? g_hn.fac.nterms : -1;
  return 0;
}
void hp_get_csr(int which, int64_t* rowptr, int32_t* col, double* val) {
  const HostCsr& a = which ? g_hn.dw : g_hn.up;
  copy_out(rowptr, a.rowptr);
  copy_out(col, a.col);
  copy_out(val, a.val);
}
void hp_get_fac(double* coef, uint32_t* jdw, uint32_t* jup) {
  copy_out(coef, g_hn.fac.coef);
  copy_out(jdw, g_hn.fac.jdw);
  copy_out(jup, g_hn.fac.jup);
}

// info: nrow, pitch, width, typed, then the lengths of pk, coef, pk16, col, val
void hp_ell(int64_t nrow, const int64_t* rowptr, const int32_t* col, const double* val, int lds, int allow_typed,
            int allow_16, int64_t* info) {
  g_ell = encode_ell(make_csr(nrow, rowptr, col, val), lds != 0, allow_typed != 0, allow_16 != 0);
  const int64_t v[9] = {g_ell.nrow, g_ell.pitch, g_ell.width, g_ell.typed, (int64_t)g_ell.pk.size(), (int64_t)g_ell.coef.size(),
                        (int64_t)g_ell.pk16.size(), (int64_t)g_ell.col.size(), (int64_t)g_ell.val.size()};
  std::memcpy(info, v, sizeof(v));
}
void hp_ell_get(uint32_t* pk, double* coef, uint32_t* pk16, int32_t* col, double* val) {
  copy_out(pk, g_ell.pk);
  copy_out(coef, g_ell.coef);
  copy_out(pk16, g_ell.pk16);
  copy_out(col, g_ell.col);
  copy_out(val, g_ell.val);
}

// info: built, nslice, packed, then the lengths of ptr, pk, dict, diag, col, val
void hp_sell(int64_t nrow, int64_t ncol, const int64_t* rowptr, const int32_t* col, const double* val, int cplx, int is_loc,
             double max_pad, int allow_packed, int64_t* info) {
  g_sell = encode_sell(nrow, ncol, rowptr, col, val, cplx, is_loc != 0, max_pad, allow_packed != 0);
  const int64_t v[9] = {g_sell.built, g_sell.nslice, g_sell.packed, (int64_t)g_sell.ptr.size(), (int64_t)g_sell.pk.size(),
                        (int64_t)g_sell.dict.size(), (int64_t)g_sell.diag.size(), (int64_t)g_sell.col.size(),
                        (int64_t)g_sell.val.size()};
  std::memcpy(info, v, sizeof(v));
}
void hp_sell_get(int32_t* ptr, uint32_t* pk, double* dict, double* diag, int32_t* col, double* val) {
  copy_out(ptr, g_sell.ptr);
  copy_out(pk, g_sell.pk);
  copy_out(dict, g_sell.dict);
  copy_out(diag, g_sell.diag);
  copy_out(col, g_sell.col);
  copy_out(val, g_sell.val);
}

// starts: room for dw_count + 1 entries; returns how many were written
int hp_chunks(int64_t dim_dw, const int64_t* rowptr, const int32_t* col, const double* val, int64_t dw_first, int64_t dw_count,
              int rmax, int32_t* starts, int* longest) {
  std::vector<int32_t> st;
  plan_tile_chunks(make_csr(dim_dw, rowptr, col, val), dw_first, dw_count, rmax, st, *longest);
  copy_out(starts, st);
  return (int)st.size();
}

// info: lengths of rowptr, col, val
void hp_merged(int64_t dim_dw, const int64_t* rowptr, const int32_t* col, const double* val, int nterms, const double* coef,
               const uint32_t* jdw, int64_t dw_first, int64_t dw_count, int64_t* info) {
  g_mx = merge_dw_lists(make_csr(dim_dw, rowptr, col, val), make_fac(dim_dw, nterms, coef, jdw), dw_first, dw_count, dim_dw);
  info[0] = (int64_t)g_mx.rowptr.size();
  info[1] = (int64_t)g_mx.col.size();
  info[2] = (int64_t)g_mx.val.size();
}
void hp_merged_get(int32_t* rowptr, int32_t* col, double* val) {
  copy_out(rowptr, g_mx.rowptr);
  copy_out(col, g_mx.col);
  copy_out(val, g_mx.val);
}

// with_nd == 0: no factored terms (the encoder gets a null pointer).  info: lengths of meta (rows), col, val, lbeg, then
// list_cap, has_nd
void hp_tile(int64_t dim_dw, const int64_t* rowptr, const int32_t* col, const double* val, int with_nd, int nterms,
             const double* coef, const uint32_t* jdw, int64_t dw_first, int64_t dw_count, const int32_t* starts, int nstarts,
             int64_t* info) {
  const HostFactored f = make_fac(dim_dw, nterms, coef, jdw);
  g_tl = build_tile_lists(make_csr(dim_dw, rowptr, col, val), dim_dw, dw_first, dw_count,
                          std::vector<int32_t>(starts, starts + nstarts), with_nd ? &f : nullptr);
  const int64_t v[6] = {(int64_t)g_tl.meta.size(), (int64_t)g_tl.col.size(), (int64_t)g_tl.val.size(), (int64_t)g_tl.lbeg.size(),
                        g_tl.list_cap, g_tl.has_nd};
  std::memcpy(info, v, sizeof(v));
}
void hp_tile_get(int32_t* meta, int32_t* col, double* val, int32_t* lbeg) {
  static_assert(sizeof(HostInt4) == 4 * sizeof(int32_t), "meta is copied out as 4 int32 per row");
  if (meta && !g_tl.meta.empty()) std::memcpy(meta, g_tl.meta.data(), g_tl.meta.size() * sizeof(HostInt4));
  copy_out(col, g_tl.col);
  copy_out(val, g_tl.val);
  copy_out(lbeg, g_tl.lbeg);
}

// info: fits, rows, list_cap, then the lengths of meta (rows), ent, wtab, lend
void hp_block(int64_t dim_dw, const int64_t* rowptr, const int32_t* col, const double* val, int nterms, const double* coef,
              const uint32_t* jdw, int shift, int64_t lds_kb, int64_t* info) {
  g_bl = build_block_lists(make_csr(dim_dw, rowptr, col, val), make_fac(dim_dw, nterms, coef, jdw), dim_dw, shift, lds_kb);
  const int64_t v[7] = {g_bl.fits, g_bl.rows, g_bl.list_cap, (int64_t)g_bl.meta.size(), (int64_t)g_bl.ent.size(),
                        (int64_t)g_bl.wtab.size(), (int64_t)g_bl.lend.size()};
  std::memcpy(info, v, sizeof(v));
}
void hp_block_get(int32_t* meta, uint32_t* ent, double* wtab, int32_t* lend) {
  if (meta && !g_bl.meta.empty()) std::memcpy(meta, g_bl.meta.data(), g_bl.meta.size() * sizeof(HostInt4));
  copy_out(ent, g_bl.ent);
  copy_out(wtab, g_bl.wtab);
  copy_out(lend, g_bl.lend);
}

int hp_col_halo(int64_t dim_up, int nterms, const uint32_t* jup) {
  HostFactored f;
  f.nterms = nterms;
  f.jup.assign(jup, jup + (size_t)nterms * dim_up);
  return factored_col_halo(f, dim_up);
}

}  // extern "C"
