// switches.hpp -- every EDIGPU_* environment switch of the library: one table, read at one of two moments.
//
// Set-up: Switches::sample() at the top of every C-ABI call that creates a sector handle; the snapshot stays with the
//         handle (edigpu_sector::sw, sub-handles inherit it) and CommSwitches::sample() with a communicator.  Whatever
//         chooses an image, a layout, a geometry or a launch shape reads that snapshot.
// Loop:   LoopSwitches::sample() where a recurrence or a solve is prepared; kept for that run.
// Nothing reads the environment inside a step or a launcher, and nothing is cached per process.  Host-only C++17.
//
// A new switch is one more row in one of the three lists below and one more row in DESIGN.md, "Environment switches".
#pragma once
#include <cstdint>
#include <limits>
#include <optional>

namespace edigpu {

// how the text of a variable becomes a value
enum class SwitchRule {
  Present,           // on when the variable exists, whatever it holds ("" and "0" included)
  FirstIsOne,        // on when its first character is '1'
  OnUnlessZero,      // on when unset; off when atoi gives 0 ("0", "abc", "")
  OffUnlessNonzero,  // off when unset; on when atoi gives something else than 0
  Int,               // atoi, clamped to [lo, hi]; the default when unset
  Int64,             // atoll, clamped to [lo, hi]; the default when unset
  IntOrUnset,        // atoi; no value when unset: the reader derives the default (the row's text says from what)
  Int64OrUnset,      // atoll; likewise
  DoubleOrUnset,     // atof; likewise
};
enum class SwitchMoment { SetUp, Comm, Loop };

struct SwitchRow {
  const char* name;
  SwitchRule rule;
  int64_t dflt, lo, hi;  // Int / Int64 only
  SwitchMoment moment;
  const char* what;
};
// the whole table: the set-up rows, then the communicator's, then the loop's
const SwitchRow* switch_table(int* nrows);

constexpr int64_t kSwAny = std::numeric_limits<int64_t>::max();  // hi = kSwAny, lo = -kSwAny: no clamp
using OptInt = std::optional<int>;
using OptInt64 = std::optional<int64_t>;
using OptDouble = std::optional<double>;

// X(field, type, name, rule, default, lo, hi, what it does)
#define EDIGPU_SETUP_SWITCHES(X)                                                                                                            \
  /* images of the generic kernels */                                                                                                       \
  X(ell16, bool, "EDIGPU_ELL16", OnUnlessZero, 1, 0, 1, "0: no 16-bit LDS image of Hup beside the packed one")                              \
  X(ell_untyped, bool, "EDIGPU_ELL_UNTYPED", Present, 0, 0, 1, "Hup as plain ELL (column, value), not the packed typed image")            \
  X(csr_nosell, bool, "EDIGPU_CSR_NOSELL", Present, 0, 0, 1, "stored sectors stay CSR: no SELL-64 image")                                  \
  X(csr_unpacked, bool, "EDIGPU_CSR_UNPACKED", Present, 0, 0, 1, "SELL-64 image with explicit values, not the value dictionary")          \
  X(normal_explicit, bool, "EDIGPU_NORMAL_EXPLICIT", FirstIsOne, 0, 0, 1, "normal mode: explicit diagonal and Hnd, not the factored tables") \
  X(handover_factor, bool, "EDIGPU_HANDOVER_FACTOR", OnUnlessZero, 1, 0, 1, "0: handed-over arrays are not searched for the factored form") \
  X(nd_in_rows, bool, "EDIGPU_ND_IN_ROWS", FirstIsOne, 0, 0, 1, "explicit Hnd as CSR inside the row kernel, not as its own SELL pass")     \
  X(nd_no_merge, bool, "EDIGPU_ND_NO_MERGE", Present, 0, 0, 1, "factored Hnd terms of equal partner maps are not merged")                  \
  X(cmplx_fourproducts, bool, "EDIGPU_CMPLX_FOURPRODUCTS", FirstIsOne, 0, 0, 1, "complex normal mode as four real products, not the doubled real sector") \
  X(flat_hostbuild, bool, "EDIGPU_FLAT_HOSTBUILD", FirstIsOne, 0, 0, 1, "stored superc / nonsu2 image built on the host, not on the device") \
  X(direct_nosort, bool, "EDIGPU_DIRECT_NOSORT", Present, 0, 0, 1, "on-the-fly terms keep the builder's order")                            \
  X(direct_termorder, bool, "EDIGPU_DIRECT_TERMORDER", Present, 0, 0, 1, "on-the-fly kernel walks all terms, no per-workgroup compaction") \
  X(direct_wgs, int, "EDIGPU_DIRECT_WGS", Int, 2, -kSwAny, kSwAny, "on-the-fly kernel: persistent workgroups per CU")                      \
  /* generic normal-mode kernels: rows, panel sweep, panel-major loop */                                                                    \
  X(rows_td, OptInt, "EDIGPU_ROWS_TD", IntOrUnset, 0, 0, 0, "rows per workgroup of the LDS row kernel (1, 2, 4, 8); unset: from the row length") \
  X(row_split, OptInt, "EDIGPU_ROW_SPLIT", IntOrUnset, 0, 0, 0, "column parts long rows are staged in (0: never); unset: as many as the LDS needs") \
  X(panel_vec2, bool, "EDIGPU_PANEL_VEC2", OnUnlessZero, 1, 0, 1, "0: no two-column panel sweep")                                          \
  X(panel_vec2_min, int64_t, "EDIGPU_PANEL_VEC2_MIN", Int64, (int64_t)1 << 21, -kSwAny, kSwAny, "smallest sector (rows) of the two-column and tiled sweeps") \
  X(panel_tile, bool, "EDIGPU_PANEL_TILE", OnUnlessZero, 1, 0, 1, "0: no LDS-tiled panel sweep")                                           \
  X(tile_rows, int, "EDIGPU_TILE_ROWS", Int, 32, 8, 64, "rows of a chunk of the tiled sweep")                                               \
  X(tile_balance, bool, "EDIGPU_TILE_BALANCE", OnUnlessZero, 1, 0, 1, "0: padded grid of the tiled sweep, last panel group not spread over the XCDs") \
  X(tile_persist, bool, "EDIGPU_TILE_PERSIST", OffUnlessNonzero, 0, 0, 1, "tiled sweep as a persistent grid")                              \
  X(panel_w, OptInt, "EDIGPU_PANEL_W", IntOrUnset, 0, 0, 0, "widest panel (columns); unset or out of range: 64, two-column sweep 128")      \
  X(panel_bpp, OptInt, "EDIGPU_PANEL_BPP", IntOrUnset, 0, 0, 0, "workgroups per panel; unset: 128, two-column sweep 256")                   \
  X(blocked, bool, "EDIGPU_BLOCKED", OnUnlessZero, 1, 0, 1, "0: the Lanczos loop keeps the natural vector layout")                         \
  X(blocked_min, int64_t, "EDIGPU_BLOCKED_MIN", Int64, (int64_t)1 << 21, -kSwAny, kSwAny, "smallest sector (rows) of the panel-major loop") \
  X(blocked_w, int, "EDIGPU_BLOCKED_W", Int, 128, -kSwAny, kSwAny, "panel width of that loop: 128 (tiled sweep), 64 / 32 / 16 (narrow-panel sweep); else none") \
  X(blocked_lds_kb, int64_t, "EDIGPU_BLOCKED_LDS_KB", Int64, 32, -kSwAny, kSwAny, "KiB of staged segments per block of the narrow-panel sweep") \
  X(blocked_wgs, int, "EDIGPU_BLOCKED_WGS", Int, 8, -kSwAny, kSwAny, "narrow-panel sweep: workgroups per CU (1 .. 8, else 8)")             \
  /* impurity-block image */                                                                                                                \
  X(ib, bool, "EDIGPU_IB", OnUnlessZero, 1, 0, 1, "0: no impurity-block image")                                                            \
  X(ib_min, int64_t, "EDIGPU_IB_MIN", Int64, (int64_t)1 << 21, -kSwAny, kSwAny, "smallest sector (elements) that gets it; 0 also lifts the row and pair gates") \
  X(ib_minrow, OptInt64, "EDIGPU_IB_MINROW", Int64OrUnset, 0, 0, 0, "shortest row (bytes) on its rows kernels; unset: 40960, or 0 when EDIGPU_IB_MIN=0") \
  X(ib_rows, int, "EDIGPU_IB_ROWS", Int, 480, 4, 480, "rows of a staged chunk of its columns kernel")                                       \
  X(ib_pairs, bool, "EDIGPU_IB_PAIRS", FirstIsOne, 0, 0, 1, "replica / general baths take the image too")                                  \
  X(ib_split, OptInt, "EDIGPU_IB_SPLIT", IntOrUnset, 0, 0, 0, "rows staged in halves: non-zero always, 0 never; unset: rows longer than the LDS") \
  X(ib_nsub, int, "EDIGPU_IB_NSUB", Int, 1, 1, 8, "workgroups per chunk of the columns kernel")                                            \
  X(ib_pspad, int, "EDIGPU_IB_PSPAD", Int, 0, 0, kSwAny, "doubles between two panels (rounded down to even)")                              \
  X(ib_nt, int, "EDIGPU_IB_NT", Int, 0, -kSwAny, kSwAny, "threads per workgroup of the rows kernel; 0: the best that fits")                \
  X(ib_cols2, OptInt, "EDIGPU_IB_COLS2", IntOrUnset, 0, 0, 0, "pipelined columns kernel: non-zero on, 0 off; unset: panels above 2 MiB")   \
  X(ib_verbose, bool, "EDIGPU_IB_VERBOSE", Present, 0, 0, 1, "say on stderr why a sector gets no image")                                   \
  X(posrows, bool, "EDIGPU_POSROWS", OffUnlessNonzero, 0, 0, 1, "short rows: the generic LDS row kernel in position order beside the block columns kernel") \
  /* local-block tables on that image */                                                                                                    \
  X(sb, bool, "EDIGPU_SB", OnUnlessZero, 1, 0, 1, "0: the impurity-block kernels, no local-block tables")                                  \
  X(sb_split, bool, "EDIGPU_SB_SPLIT", OffUnlessNonzero, 0, 0, 1, "local-block rows kernel on rows staged in halves")                      \
  X(sb_amode, bool, "EDIGPU_SB_AMODE", OffUnlessNonzero, 0, 0, 1, "per-orbital walk where the bath allows it")                             \
  X(sb_cw, int, "EDIGPU_SB_CW", Int, 0, -kSwAny, kSwAny, "columns kernel: 1 = one column per lane, 512 threads; else two, 256 threads")    \
  X(sb_nt, int, "EDIGPU_SB_NT", Int, 0, -kSwAny, kSwAny, "threads per workgroup of the rows kernel; 0: the first geometry that fits")      \
  X(sb_nbt, int, "EDIGPU_SB_NBT", Int, 0, -kSwAny, kSwAny, "blocks per thread of the rows kernel; 0: likewise")                            \
  X(sb_stamp, bool, "EDIGPU_SB_STAMP", Present, 0, 0, 1, "print cycle stamps of the rows kernel per launch")                               \
  X(sb_verbose, bool, "EDIGPU_SB_VERBOSE", Present, 0, 0, 1, "say on stderr which tables a sector gets, or why none")                      \
  /* shape of the Lanczos step */                                                                                                           \
  X(lanczos_unfused, bool, "EDIGPU_LANCZOS_UNFUSED", Present, 0, 0, 1, "literal recurrence: product, then the vector kernels")             \
  X(lanczos_inkernel_finalize, bool, "EDIGPU_LANCZOS_INKERNEL_FINALIZE", OffUnlessNonzero, 0, 0, 1, "the sweep's last workgroup finalizes the step") \
  X(lanczos_graph, bool, "EDIGPU_LANCZOS_GRAPH", OffUnlessNonzero, 0, 0, 1, "later steps of a small sector replayed from a captured graph") \
  X(lanczos_graph_max, int64_t, "EDIGPU_LANCZOS_GRAPH_MAX", Int64, (int64_t)1 << 21, -kSwAny, kSwAny, "largest sector (rows) that uses the graph")

#define EDIGPU_COMM_SWITCHES(X)                                                                                                      \
  X(force_collectives, bool, "EDIGPU_FORCE_COLLECTIVES", Present, 0, 0, 1, "a world of one still issues its collectives (rehearsal)") \
  X(comm_two_streams, bool, "EDIGPU_COMM_TWO_STREAMS", Present, 0, 0, 1, "collectives on the caller's stream, not the communicator's own")

#define EDIGPU_LOOP_SWITCHES(X)                                                                                                              \
  X(lanczos_exactbeta, bool, "EDIGPU_LANCZOS_EXACTBETA", Present, 0, 0, 1, "two-reduction recurrence: beta from its own axpy + norm pass")   \
  X(sb_step, int, "EDIGPU_SB_STEP", Int, 1, -kSwAny, kSwAny, "Lanczos step on local-block tables: 0 impurity-block kernels, 2 semi-fused, else fused") \
  X(eigh_twopass, bool, "EDIGPU_EIGH_TWOPASS", Present, 0, 0, 1, "edigpu_lanczos_eigh regenerates the Lanczos vectors for the Ritz vector") \
  X(trl_onepass, bool, "EDIGPU_TRL_ONEPASS", Present, 0, 0, 1, "thick-restart solver: second Gram-Schmidt pass only when the first removed much") \
  X(trl_full, bool, "EDIGPU_TRL_FULL", Present, 0, 0, 1, "thick-restart solver: full CGS2 on every step, no selective skip")               \
  X(trl_thr, OptDouble, "EDIGPU_TRL_THR", DoubleOrUnset, 0, 0, 0, "coefficients below this times |w| stay in w; unset: 1e-3 * tol")        \
  X(trl_debug, bool, "EDIGPU_TRL_DEBUG", Present, 0, 0, 1, "print every restart on stderr")                                                \
  X(shard_panel_loop, bool, "EDIGPU_SHARD_PANEL_LOOP", OnUnlessZero, 1, 0, 1, "0: sharded recurrence on the rows layout, converted around every product") \
  X(shard_generic, bool, "EDIGPU_SHARD_GENERIC", Present, 0, 0, 1, "shards never take the column-block exchange of the local-block tables")

#define EDIGPU_SWITCH_FIELD(field, type, name, rule, dflt, lo, hi, what) type field;

// set-up snapshot of a sector handle
struct Switches {
  EDIGPU_SETUP_SWITCHES(EDIGPU_SWITCH_FIELD)
  static Switches sample();
  int64_t ib_min_row_bytes() const { return ib_minrow.value_or(ib_min == 0 ? 0 : 40 * 1024); }
  // log2 of the panel width of the panel-major loop; 0: a width no sweep is built for
  int blocked_shift() const { return blocked_w == 128 ? 7 : blocked_w == 64 ? 6 : blocked_w == 32 ? 5 : blocked_w == 16 ? 4 : 0; }
};

// set-up snapshot of a communicator
struct CommSwitches {
  EDIGPU_COMM_SWITCHES(EDIGPU_SWITCH_FIELD)
  static CommSwitches sample();
};

// one recurrence or solve
struct LoopSwitches {
  EDIGPU_LOOP_SWITCHES(EDIGPU_SWITCH_FIELD)
  static LoopSwitches sample();
};

}  // namespace edigpu
