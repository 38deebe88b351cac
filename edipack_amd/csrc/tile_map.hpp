// tile_map.hpp -- which (panel, chunk) task a workgroup of the tiled column sweep takes on 128-column panels of the
// panel-major layout (kernels_panel.hip: launch_dw_blocked_tiles, normal_dw_tile_kernel<.., BLK = true>).
//
// Workgroups are placed on the eight XCDs round-robin (blockIdx & 7; another placement only costs speed), and a panel
// (DimDw segments of 1 KiB) is meant to stay in the L2 of the XCD that sweeps it.  Whole groups of eight panels
// therefore give one panel to each XCD: workgroup wg takes panel (slot / blocks_per_panel) * 8 + x and chunk
// slot % blocks_per_panel with x = wg & 7, slot = wg >> 3.  Mapped the same way, the t = npanels % 8 panels of a last,
// partly filled group keep t XCDs busy while 8 - t have nothing to run.  Instead their t * blocks_per_panel tasks,
// ordered by (panel, chunk), are cut into eight contiguous ranges, one per XCD (XCD x takes q tasks, one more when
// x < r): a tail panel enters two or three L2s instead of one, every XCD finishes at the same time, and no workgroup
// is launched without a task.
//
// The three sums of a task (fused Lanczos step) go to the position the task has in the padded grid of the unbalanced
// mapping, ((panel / 8) * blocks_per_panel + chunk) * 8 + panel % 8 of np = ceil(npanels / 8) * blocks_per_panel * 8:
// the finalize adds the same numbers in the same order under either mapping.
#pragma once

#if defined(__HIPCC__)
#define EDIGPU_TILE_HD __host__ __device__
#else
#define EDIGPU_TILE_HD
#endif

namespace edigpu {

struct TileMap {
  int grid;        // workgroups to launch
  int np;          // positions per sum in the partial buffer
  int wg_tail;     // first workgroup of the balanced tail (== grid: there is none)
  int panel_tail;  // first panel of the tail
  int q, r;        // tail tasks of XCD x: q + (x < r)
};

// balance = false: the padded grid (workgroups of the last group whose panel does not exist leave at once)
inline TileMap plan_tile_map(int npanels, int blocks_per_panel, bool balance) {
  TileMap m;
  const int t = npanels % 8;
  m.np = (npanels + 7) / 8 * blocks_per_panel * 8;
  m.grid = m.wg_tail = m.np;
  m.panel_tail = npanels;
  m.q = m.r = 0;
  if (balance && t != 0) {
    m.panel_tail = npanels - t;
    m.wg_tail = m.panel_tail * blocks_per_panel;  // whole groups: 8 * blocks_per_panel workgroups each
    m.q = t * blocks_per_panel / 8;
    m.r = t * blocks_per_panel % 8;
    m.grid = m.wg_tail + t * blocks_per_panel;
  }
  return m;
}

// task of workgroup wg < m.grid and the position of its sums; false: a workgroup of the padding (no task)
EDIGPU_TILE_HD inline bool tile_task_of(const TileMap& m, int npanels, int blocks_per_panel, int wg, int& panel, int& chunk,
                                        int& pos) {
  const int x = wg & 7;
  if (wg >= m.wg_tail) {
    const int i = x * m.q + (x < m.r ? x : m.r) + ((wg - m.wg_tail) >> 3);
    panel = m.panel_tail + i / blocks_per_panel;
    chunk = i % blocks_per_panel;
    pos = ((panel >> 3) * blocks_per_panel + chunk) * 8 + (panel & 7);
    return true;
  }
  panel = ((wg >> 3) / blocks_per_panel) * 8 + x;
  chunk = (wg >> 3) % blocks_per_panel;
  pos = wg;
  return panel < npanels;
}

}  // namespace edigpu
