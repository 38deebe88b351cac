// image_hooks.hip -- test hooks of the host images and of the finalize kernel: the task map of the tiled column sweep
// (tile_map.hpp), the 16-bit row images (host_pack.hpp), one call of lz_finalize_alpha_beta on host buffers.
#include <algorithm>
#include <climits>

#include "../dev_mem.hpp"
#include "../host_pack.hpp"
#include "../kernels.hpp"
#include "../tile_map.hpp"

using namespace edigpu;

extern "C" {

int edigpu_tile_task_map(int32_t npanels, int32_t blocks_per_panel, int32_t balanced, int32_t* grid, int32_t* np,
                         int32_t* panel, int32_t* chunk, int32_t* pos) {
  if (npanels < 1 || blocks_per_panel < 1 || !grid || !np ||
      ((int64_t)npanels + 7) / 8 * 8 * (int64_t)blocks_per_panel > INT32_MAX) {
    set_error("edigpu_tile_task_map: bad argument");
    return 1;
  }
  const TileMap m = plan_tile_map(npanels, blocks_per_panel, balanced != 0);
  *grid = m.grid;
  *np = m.np;
  for (int wg = 0; wg < m.grid; wg++) {
    int pn, ch, ps;
    if (!tile_task_of(m, npanels, blocks_per_panel, wg, pn, ch, ps)) pn = -1;
    if (panel) panel[wg] = pn;
    if (chunk) chunk[wg] = ch;
    if (pos) pos[wg] = ps;
  }
  return 0;
}

int edigpu_ell16_images(int64_t nrow, const int64_t* rowptr, const int32_t* col, const double* val, int64_t* info,
                        uint32_t* pk16, uint32_t* pk16o, int64_t* owned_col) {
  if (nrow < 1 || !rowptr || !info || (rowptr[nrow] > 0 && (!col || !val))) {
    set_error("edigpu_ell16_images: bad argument");
    return 1;
  }
  HostCsr a;
  a.nrow = a.ncol = nrow;
  a.rowptr.assign(rowptr, rowptr + nrow + 1);
  a.col.assign(col, col + rowptr[nrow]);
  a.val.assign(val, val + rowptr[nrow]);
  const HostEll h = encode_ell(a, true, true, true);
  info[0] = h.width;
  info[1] = h.pitch;
  info[2] = h.pitch16o;
  info[3] = (int64_t)h.pk16.size();
  info[4] = (int64_t)h.pk16o.size();
  if (pk16) std::copy(h.pk16.begin(), h.pk16.end(), pk16);
  if (pk16o) std::copy(h.pk16o.begin(), h.pk16o.end(), pk16o);
  if (owned_col)
    for (int64_t pos = 0; pos < h.pitch16o; pos++) owned_col[pos] = ell16_owned_col(pos);
  return 0;
}

int edigpu_finalize_ab(int32_t np, const double* partial, int64_t n, const double* P, const double* Q, int32_t nscal,
                       double* scal, int32_t iter, int32_t nlanc) {
  if (np < 1 || np > kMaxPartials || !partial || n < 1 || !P || !Q || !scal || nlanc < 1 || iter >= nlanc ||
      nscal < SC_AB + 2 * nlanc) {
    set_error("edigpu_finalize_ab: bad argument");
    return 1;
  }
  if (ensure_device()) return 1;
  EDIGPU_HIP(hipSetDevice(current_device()));
  double *d_part = nullptr, *d_p = nullptr, *d_q = nullptr, *d_scal = nullptr;
  int rc = dev_upload(&d_part, partial, (size_t)3 * np) || dev_upload(&d_p, P, (size_t)n) ||
           dev_upload(&d_q, Q, (size_t)n) || dev_upload(&d_scal, scal, (size_t)nscal);
  if (!rc) rc = lz_finalize_alpha_beta(d_p, d_q, n, d_part, np, d_scal, iter, nlanc, nullptr);
  if (!rc && hipDeviceSynchronize() != hipSuccess) {
    set_error("edigpu_finalize_ab: the kernel failed");
    rc = 1;
  }
  if (!rc && hipMemcpy(scal, d_scal, (size_t)nscal * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
    set_error("edigpu_finalize_ab: download failed");
    rc = 1;
  }
  dev_free_all(d_part, d_p, d_q, d_scal);
  return rc;
}

}  // extern "C"
