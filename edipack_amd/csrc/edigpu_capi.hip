// edigpu_capi.hip -- the core of the C ABI declared in include/edigpu.h: the calling thread's error string and current
// device, the queries on a handle and on a model's sectors, raw device memory, edigpu_destroy.  The other jobs of the
// ABI have a file each (Source layout).
// There is no CPU compute path: without a usable HIP device every entry point fails.
#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>

#include "dev_mem.hpp"
#include "host_ib.hpp"
#include "kernels.hpp"

namespace edigpu {

static thread_local std::string g_err;
static thread_local int g_device = 0;
void set_error(const std::string& msg) { g_err = msg; }

bool have_error() { return !g_err.empty(); }
int current_device() { return g_device; }

int ensure_device(int* count_out) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    set_error(std::string("edigpu: no usable HIP device (") +
              (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
              "); this library has no CPU fallback");
    if (count_out) *count_out = 0;
    return 1;
  }
  if (count_out) *count_out = n;
  return 0;
}

int ensure_dynamic_lds(const void* kernel, size_t bytes) {
  if (bytes <= 48 * 1024) return 0;
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> done;
  int dev = 0;
  EDIGPU_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  size_t& have = done[{dev, kernel}];
  if (have >= bytes) return 0;
  EDIGPU_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  have = bytes;
  return 0;
}

int device_cu_count() {
  static thread_local int cached_dev = -1, cached = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (dev != cached_dev) {
    hipDeviceProp_t pr;
    cached = (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
    cached_dev = dev;
  }
  return cached;
}

int resident_blocks(const void* kernel, int threads, size_t dyn_lds) {
  static std::mutex mu;
  static std::map<std::tuple<int, const void*, int, size_t>, int> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    set_error("resident_blocks: hipGetDevice failed");
    return -1;
  }
  std::lock_guard<std::mutex> lk(mu);
  auto key = std::make_tuple(dev, kernel, threads, dyn_lds);
  auto it = done.find(key);
  if (it != done.end()) return it->second;
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, dyn_lds) != hipSuccess || n < 1) {
    set_error("resident_blocks: occupancy query failed (kernel does not fit a CU?)");
    return -1;
  }
  done[key] = n;
  return n;
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

const char* edigpu_last_error(void) { return g_err.c_str(); }

int edigpu_version(void) { return 100; }
int64_t edigpu_model_sizeof(void) { return (int64_t)sizeof(edigpu_model); }

int edigpu_device_count(int* count) {
  int n = 0;
  int rc = ensure_device(&n);
  if (count) *count = n;
  return rc;
}

int edigpu_init(int device) {
  int n = 0;
  if (ensure_device(&n)) return 1;
  if (device < 0 || device >= n) {
    set_error("edigpu_init: device index out of range");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(device));
  g_device = device;
  return 0;
}

int edigpu_sector_dim(const edigpu_model* model, int q1, int q2, int64_t* dim) {
  if (!model || !dim) {
    set_error("edigpu_sector_dim: NULL argument");
    return 1;
  }
  std::string e = sector_dim(*model, q1, q2, *dim);
  if (!e.empty()) {
    set_error(e);
    return 1;
  }
  return 0;
}

int edigpu_sector_map(const edigpu_model* model, int q1, int q2, int which, int32_t* map, int64_t* n) {
  if (!model || !n) {
    set_error("edigpu_sector_map: NULL argument");
    return 1;
  }
  std::vector<int32_t> st;
  std::string e = sector_map(*model, q1, q2, which, st);
  if (!e.empty()) {
    set_error(e);
    return 1;
  }
  if (map) {
    if (*n < (int64_t)st.size()) {
      set_error("edigpu_sector_map: output buffer too small");
      return 1;
    }
    std::copy(st.begin(), st.end(), map);
  }
  *n = (int64_t)st.size();
  return 0;
}

int edigpu_sector_map_jz(const edigpu_model* model, int ntot, int twojz, int32_t* map, int64_t* n) {
  if (!model || !n) {
    set_error("edigpu_sector_map_jz: NULL argument");
    return 1;
  }
  std::vector<int32_t> st;
  std::string e = sector_map_jz(*model, ntot, twojz, st);
  if (!e.empty()) {
    set_error(e);
    return 1;
  }
  if (map) {
    if (*n < (int64_t)st.size()) {
      set_error("edigpu_sector_map_jz: output buffer too small");
      return 1;
    }
    std::copy(st.begin(), st.end(), map);
  }
  *n = (int64_t)st.size();
  return 0;
}

int edigpu_image_info(edigpu_handle s, int32_t image[6]) {
  if (!s || !image || s->kind != kNormal) {
    set_error("edigpu_image_info: not a normal-mode handle");
    return 1;
  }
  image[0] = s->factored;
  image[1] = s->factored ? s->fac_nterms : 0;
  image[2] = s->factored ? s->fac_nimp : 0;
  image[3] = s->panel_mode;
  image[4] = s->ib ? kIbPanel : (s->blk_shift ? (1 << s->blk_shift) : 0);
  image[5] = s->ib ? (s->ib->sb ? (s->ib->sb->nhalf == 2 ? 4 : (s->ib->pr.on ? 5 : 3)) : s->ib->nhalf) : 0;  // 1: impurity-block image, 2: with rows staged in halves, 3: local-block tables, 4: local-block rows kernel on half rows, 5: local-block columns kernel + generic row kernel in position order (short rows)
  return 0;
}

int edigpu_info(edigpu_handle s, int64_t info[10]) {
  if (!s || !info) {
    set_error("edigpu_info: NULL argument");
    return 1;
  }
  info[0] = s->dim;
  info[1] = s->nloc;
  info[2] = s->row_first;
  info[3] = s->is_complex;
  info[4] = s->kind;
  info[5] = s->dim_up;
  info[6] = s->dim_dw;
  if (s->kind == kNormal) {
    info[7] = s->h_up.nnz() + s->h_dw.nnz();
    info[8] = s->nd_nnz;
  } else if (s->kind == kCmplxNormal) {
    info[7] = s->sub_s->h_up.nnz() + s->sub_s->h_dw.nnz();  // pattern of Hup / Hdw (A shares it or is a subset)
    info[8] = s->sub_s->nd_nnz;
  } else if (s->kind == kDirect) {
    info[7] = s->dir_nterms;
    info[8] = 0;
  } else if (s->kind == kOrbs) {
    info[7] = 0;
    for (const HostCsr& f : s->h_orbs_fac) info[7] += f.nnz();
    info[8] = s->orbs.naxes;
  } else {
    info[7] = s->loc.nnz;
    info[8] = s->nonloc.nnz;
  }
  info[9] = s->device;
  return 0;
}

int edigpu_algorithmic_bytes(edigpu_handle s, double* bytes_hv, double* bytes_step) {
  if (!s) {
    set_error("edigpu_algorithmic_bytes: NULL handle");
    return 1;
  }
  // reference storage format, every array read once, v read once, Hv written once
  double b = 0.0;
  const double sz = s->is_complex ? 16.0 : 8.0;
  if (s->kind == kCmplxNormal) {
    // the reference's complex(8) normal-mode arrays: same pattern as the real build, 16-byte values and vectors
    const edigpu_sector* r = s->sub_s;
    const double n = (double)s->nloc;
    b = 3.0 * sz * n;
    if (r->has_nd) b += (sz + 4.0) * (double)r->nd_nnz + 4.0 * (n + 1.0);
    b += (sz + 4.0) * (double)(r->h_up.nnz() + r->h_dw.nnz()) + 4.0 * (double)(r->dim_up + r->dim_dw + 2);
  } else if (s->kind == kNormal) {
    const double n = (double)s->nloc;
    b = 3.0 * sz * n;
    if (s->has_nd) b += (sz + 4.0) * (double)s->nd_nnz + 4.0 * (n + 1.0);
    b += (sz + 4.0) * (double)(s->h_up.nnz() + s->h_dw.nnz()) + 4.0 * (double)(s->dim_up + s->dim_dw + 2);
  } else if (s->kind == kOrbs) {
    // orbs: diagonal + 2 vectors + the small factor matrices
    b = 3.0 * sz * (double)s->nloc;
    for (const HostCsr& f : s->h_orbs_fac) b += (sz + 4.0) * (double)f.nnz() + 4.0 * (double)(f.nrow + 1);
  } else if (s->kind == kDirect) {
    // direct: 2 vectors + the sector map (B = 2*s*Dim + 4*DimEl)
    b = 2.0 * sz * (double)s->nloc + 4.0 * (double)s->nloc;
  } else {
    const double n = (double)s->nloc;
    b = (sz + 4.0) * (double)(s->loc.nnz + s->nonloc.nnz) + 4.0 * (n + 1.0) + 2.0 * sz * n;
  }
  if (bytes_hv) *bytes_hv = b;
  if (bytes_step) *bytes_step = b + 3.0 * sz * (double)s->nloc;
  return 0;
}

int edigpu_dev_alloc(int64_t bytes, void** dev_ptr) {
  if (!dev_ptr || bytes < 0) {
    set_error("edigpu_dev_alloc: bad argument");
    return 1;
  }
  if (ensure_device()) return 1;
  EDIGPU_HIP(hipSetDevice(g_device));
  *dev_ptr = nullptr;
  EDIGPU_HIP(hipMalloc(dev_ptr, (size_t)std::max<int64_t>(bytes, 8)));
  return 0;
}

int edigpu_dev_free(void* dev_ptr) {
  if (dev_ptr) EDIGPU_HIP(hipFree(dev_ptr));
  return 0;
}

int edigpu_dev_upload(void* dst_dev, const void* src_host, int64_t bytes) {
  if (bytes < 0 || (bytes > 0 && (!dst_dev || !src_host))) {
    set_error("edigpu_dev_upload: bad argument");
    return 1;
  }
  if (bytes > 0) EDIGPU_HIP(hipMemcpy(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice));
  return 0;
}

int edigpu_dev_download(void* dst_host, const void* src_dev, int64_t bytes) {
  if (bytes < 0 || (bytes > 0 && (!dst_host || !src_dev))) {
    set_error("edigpu_dev_download: bad argument");
    return 1;
  }
  if (bytes > 0) EDIGPU_HIP(hipMemcpy(dst_host, src_dev, (size_t)bytes, hipMemcpyDeviceToHost));
  return 0;
}

int edigpu_destroy(edigpu_handle s) {
  if (!s) return 0;
  (void)hipSetDevice(s->device);
  if (s->stream) {
    (void)hipStreamSynchronize(s->stream);
    (void)hipStreamDestroy(s->stream);
  }
  if (s->sub_s) edigpu_destroy(s->sub_s);
  if (s->sub_a) edigpu_destroy(s->sub_a);
  if (s->sub_d) edigpu_destroy(s->sub_d);
  dev_free_all(s->d_cz, s->d_hd, s->d_gu, s->d_gd, s->d_mx_rowptr, s->d_tile_chunks, s->d_tile_lbeg);
  if (s->lz_graph) (void)hipGraphExecDestroy(s->lz_graph);
  dev_free_all(s->d_lzcnt, s->d_bl_meta, s->d_bl_lend, s->d_bl_ent, s->d_bl_wtab);
  if (s->ib) {
    free_ib(s->ib);
    delete s->ib;
    s->ib = nullptr;
  }
  dev_free_all(s->d_tl_meta, s->d_tl_col, s->d_tl_val, s->d_mx_col, s->d_mx_val);
  dev_free_all(s->d_eux, s->d_ed, s->d_impd, s->d_ndcoef, s->d_jup, s->d_jdw);
  free_ell(s->up_ell);
  free_csr(s->dw);
  free_csr(s->nd);
  free_csr(s->loc);
  free_csr(s->nonloc);
  dev_free_all(s->orbs.ell_col, s->orbs.ell_val, s->orbs.hd, s->orbs.eax, s->orbs.impbit, s->orbs.xtab);
  s->orbs = OrbsArgs();
  dev_free_all(s->d_dir_states, s->d_dir_offdw, s->d_dir_rkup, s->d_dir_terms, s->d_dir_tests, s->d_dir_dtab, s->d_dir_xtab);
  free_occ(s);
  free_rdm(s);
  free_rdm_flat(s);
  free_ph(s);
  free_axisop(s);
  free_twin(s);
  free_batch(s);
  dev_free_all(s->d_vin, s->d_vout, s->d_tmp, s->d_partial, s->d_scal);
  delete s;
  return 0;
}

}  // extern "C"
