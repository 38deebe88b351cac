// host_pack.hpp -- host-side encoders of the packed tables the generic kernels read: the ELL images of a factor
// matrix (normal_rows_kernel), the SELL-64 image of a CSR block (sell_rows_kernel) and the per-row lists of the panel
// sweeps (normal_dw_*_kernel).  Plain C++17: host data and explicit options in, vectors and scalars out.  The switches
// that choose among the images, and the uploads, belong to the C-ABI source; an empty vector means "not built".
#pragma once
#include <cstdint>
#include <vector>

#include "host_build.hpp"

namespace edigpu {

struct HostInt4 {  // the device's int4
  int32_t x, y, z, w;
};

// ELL (column-major [slot][row]) images of a small square factor matrix: the fields of DevEll
struct HostEll {
  int64_t nrow = 0, pitch = 0;
  int width = 0;
  int typed = 0;
  std::vector<uint32_t> pk;
  std::vector<double> coef;
  std::vector<uint32_t> pk16;
  // even nrow: the words of pk16 in the order in which the rows kernel's threads own the columns, (width + 1) / 2
  // * pitch16o words -- the image such a sector's kernel reads; pk16 (column order) is what an odd nrow reads
  std::vector<uint32_t> pk16o;
  int64_t pitch16o = 0;
  std::vector<int32_t> col;
  std::vector<double> val;
};
// Ownership order of the 16-bit image (normal_rows_kernel, LINES): a pass of the kernel covers 2048 columns with 512
// threads; lane l of wave w owns the column pairs {2l, 2l + 1} of the pass's blocks 2w and 2w + 1 of 128 columns, so
// that a wave's 16-byte-per-lane vector accesses are whole 1 KiB pieces.  The word at position 4 t + e of a pass
// belongs to the e-th column thread t = 64 w + l owns; this is the column of position pos (it may lie past the row).
inline int64_t ell16_owned_col(int64_t pos) {
  const int64_t pass = pos >> 11, t = (pos & 2047) >> 2, e = pos & 3;
  return (pass << 11) + ((2 * (t >> 6) + (e >> 1)) << 7) + 2 * (t & 63) + (e & 1);
}
// lds: the sector's row kernel stages V rows in LDS; the packed layouts then hold byte offsets into
// the staged row instead of columns, and dead typed slots name its zero slot (index nrow).
HostEll encode_ell(const HostCsr& a, bool lds, bool allow_typed, bool allow_16);

// SELL-64 image of a CSR block: the sell_* fields of DevCsr; built == false: keep the CSR kernel
struct HostSell {
  bool built = false;
  int64_t nslice = 0;
  bool packed = false;
  std::vector<int32_t> ptr;
  std::vector<uint32_t> pk;
  std::vector<double> dict, diag;
  std::vector<int32_t> col;
  std::vector<double> val;
};
HostSell encode_sell(int64_t nrow, int64_t ncol, const int64_t* rowptr, const int32_t* col, const double* val, int cplx,
                     bool is_loc, double max_pad, bool allow_packed);

void plan_tile_chunks(const HostCsr& dw, int64_t dw_first, int64_t dw_count, int rmax, std::vector<int32_t>& starts,
                      int& longest);

// merged per-local-row list for the panel kernel: Hdw entries (tag 0) + applicable Hnd terms
struct HostMergedList {
  std::vector<int32_t> rowptr, col;
  std::vector<double> val;
};
HostMergedList merge_dw_lists(const HostCsr& dw, const HostFactored& f, int64_t dw_first, int64_t dw_count, int64_t dim_dw);

// per-row lists of the tiled sweep; f: the factored Hnd terms to append, or null
struct HostTileLists {
  std::vector<HostInt4> meta;  // per local row: first entry, entries inside the chunk, outside, Hnd terms
  std::vector<int32_t> col;
  std::vector<double> val;
  std::vector<int32_t> lbeg;   // first entry of every chunk, then the end of the last
  int list_cap = 4;            // entries of the longest chunk
  bool has_nd = false;
};
HostTileLists build_tile_lists(const HostCsr& dw, int64_t dim_dw, int64_t dw_first, int64_t dw_count,
                               const std::vector<int32_t>& tile_starts, const HostFactored* f);
// the row meta as the kernel reads it: the count of hops leaving the chunk WITHOUT the padding of its last batch (the
// trailing entries that name the row itself, which no live outside entry can: a row lies inside its own chunk)
std::vector<HostInt4> tile_meta_live(const HostTileLists& l, int64_t dw_first);

// per-row lists of the narrow-panel sweep with their weight table; fits == false: no blocked layout
struct HostBlockLists {
  bool fits = false;
  int rows = 0;                // rows of an LDS block
  std::vector<HostInt4> meta;
  std::vector<uint32_t> ent;
  std::vector<double> wtab;
  std::vector<int32_t> lend;   // end of every block's entries
  int list_cap = 4;
};
HostBlockLists build_block_lists(const HostCsr& dw, const HostFactored& f, int64_t dim_dw, int shift, int64_t lds_kb);

// max |partner column - column| over the factored Hnd terms
int factored_col_halo(const HostFactored& f, int64_t dim_up);

}  // namespace edigpu
