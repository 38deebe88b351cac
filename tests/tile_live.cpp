// Test-only shim of tests/test_tile_gathers.py: the row meta the tiled sweep reads on the device (csrc/host_pack.cpp:
// tile_meta_live), computed from tile lists handed over as plain arrays.  Compiled with g++; never part of the product.
#include <cstdint>
#include <vector>

#include "host_build.hpp"
#include "host_pack.hpp"
using namespace edigpu;

// meta: nrow x 4 (as build_tile_lists gives it); out: nrow x 4
extern "C" void tl_meta_live(int64_t nrow, const int32_t* meta, int64_t nent, const int32_t* col, const double* val,
                             int64_t dw_first, int32_t* out) {
  HostTileLists l;
  l.meta.resize((size_t)nrow);
  for (int64_t r = 0; r < nrow; r++) l.meta[(size_t)r] = HostInt4{meta[4 * r], meta[4 * r + 1], meta[4 * r + 2], meta[4 * r + 3]};
  l.col.assign(col, col + nent);
  l.val.assign(val, val + nent);
  const std::vector<HostInt4> m = tile_meta_live(l, dw_first);
  for (int64_t r = 0; r < nrow; r++) {
    out[4 * r] = m[(size_t)r].x;
    out[4 * r + 1] = m[(size_t)r].y;
    out[4 * r + 2] = m[(size_t)r].z;
    out[4 * r + 3] = m[(size_t)r].w;
  }
}
