"""The tiled column sweep on 128-column panels of the panel-major layout: the tasks of a partly filled last group of
eight panels are spread over all eight XCDs (csrc/tile_map.hpp) instead of keeping one XCD per panel busy.

Only the task -> workgroup mapping differs from the padded grid (EDIGPU_TILE_BALANCE=0, read at set-up: each switch
value builds its own handle): every task computes what it computed and its three sums land where they landed, so H*v
and the Lanczos coefficients are the same bit for bit, and both match the oracle.
"""
import ctypes as C

import numpy as np
import pytest

from tests.common import make_models, rel_err

TOL = 1e-12  # test_gpu_parity.TOL (test_normal_apply_matches_oracle)

CASES = [
    # npanels, bath, norb, nbath, (nup, ndw), jxp, EDIGPU_TILE_ROWS
    (1, "normal", 2, 3, (4, 2), 0.25, None),     # DimUp = 70: fewer panels than XCDs, Hnd terms
    (4, "normal", 1, 10, (5, 2), 0.0, None),     # DimUp = 462: fewer panels than XCDs
    (7, "normal", 2, 5, (5, 2), 0.0, None),      # DimUp = 792
    (8, "normal", 2, 5, (6, 2), 0.25, None),     # DimUp = 924: no tail, the mapping is the padded grid's; Hnd terms
    (11, "normal", 1, 12, (5, 2), 0.0, None),    # DimUp = 1287: tail of 3 (3 * chunks is no multiple of 8 below 8 chunks)
    (11, "hybrid", 3, 10, (5, 2), 0.25, 8),      # the same tail with Hnd terms and short chunks: ranges that cross panels
    (14, "hybrid", 2, 11, (6, 2), 0.25, None),   # DimUp = 1716: tail of 6, Hnd terms
    (14, "normal", 1, 12, (6, 3), 0.0, 8),       # tail of 6, DimDw = 286 in short chunks
]


def _skip_if_switched():
    import os
    if os.environ.get("EDIGPU_NORMAL_EXPLICIT") or os.environ.get("EDIGPU_LANCZOS_UNFUSED") or os.environ.get("EDIGPU_ROW_SPLIT") \
            or os.environ.get("EDIGPU_PANEL_VEC2") == "0" or os.environ.get("EDIGPU_PANEL_TILE") == "0" \
            or os.environ.get("EDIGPU_LANCZOS_INKERNEL_FINALIZE"):
        pytest.skip("needs the factored image, the fused step, whole rows in the LDS and the tiled sweep")


def _build(monkeypatch, pm, sec, balance):
    from edipack_amd.hamiltonian import SectorHamiltonian
    if balance:
        monkeypatch.delenv("EDIGPU_TILE_BALANCE", raising=False)
    else:
        monkeypatch.setenv("EDIGPU_TILE_BALANCE", "0")
    h = SectorHamiltonian.normal_from_model(pm, *sec)
    assert h.image_info()[4] == 128  # panel-major, 128-column panels: the tiled sweep
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("npanels,bath,norb,nbath,sec,jxp,tile_rows", CASES)
def test_balanced_tail_matches_padded_grid_and_oracle(gpu, monkeypatch, npanels, bath, norb, nbath, sec, jxp, tile_rows):
    """(a) H*v through the product of the panel-major loop against the oracle, (b) the same bit for bit with either
    mapping, (c) alpha and beta of 12 fused Lanczos steps bit for bit with either mapping (and against the oracle)."""
    _skip_if_switched()
    from oracle import oracle as O
    om, pm = make_models("normal", bath, norb, nbath, seed=83, jxp=jxp)
    ho = O.HNormal(om, *sec)
    assert (ho.dimup + 127) // 128 == npanels
    monkeypatch.setenv("EDIGPU_IB", "0")  # the generic panel-major loop, forced on a small sector (test_gpu_ell16)
    monkeypatch.setenv("EDIGPU_BLOCKED", "1")
    monkeypatch.setenv("EDIGPU_BLOCKED_MIN", "0")
    monkeypatch.setenv("EDIGPU_BLOCKED_W", "128")
    monkeypatch.setenv("EDIGPU_PANEL_VEC2_MIN", "0")
    if tile_rows:
        monkeypatch.setenv("EDIGPU_TILE_ROWS", str(tile_rows))
    hb = _build(monkeypatch, pm, sec, True)
    hp = _build(monkeypatch, pm, sec, False)
    assert (hb.image_info()[1] > 0) == (jxp != 0.0)
    rng = np.random.default_rng(79)
    for _ in range(2):
        v = rng.standard_normal(ho.dim)
        yb, yp = hb.apply_loop(v), hp.apply_loop(v)
        assert np.array_equal(yb, yp)
        assert rel_err(yb, ho.matvec(v)) < TOL
    v = rng.standard_normal(ho.dim)
    n = 12
    ao, bo, _ = ho.lanc_tridiag(v, n)
    ab, bb, nb = hb.lanczos_tridiag(v, n)
    ap, bp, npd = hp.lanczos_tridiag(v, n)
    assert nb == npd == n
    assert np.array_equal(ab, ap) and np.array_equal(bb, bp)
    assert rel_err(ab, ao) < 1e-10 and rel_err(bb, bo) < 1e-10  # as test_lanczos_tridiag_matches_oracle
    hb.destroy()
    hp.destroy()


def _task_map(npanels, bpp, balanced):
    from edipack_amd import capi
    L = capi.lib()
    cap = (npanels + 7) // 8 * 8 * bpp
    grid, np_ = C.c_int32(), C.c_int32()
    panel, chunk, pos = (np.full(cap, -7, dtype=np.int32) for _ in range(3))
    assert L.edigpu_tile_task_map(npanels, bpp, int(balanced), C.byref(grid), C.byref(np_), capi.pi32(panel),
                                  capi.pi32(chunk), capi.pi32(pos)) == 0
    assert np_.value == cap and grid.value <= cap
    return grid.value, panel[:grid.value], chunk[:grid.value], pos[:grid.value]


@pytest.mark.usefixtures("built")
def test_task_map_covers_every_task_once():
    """Host only: the launcher's mapping (the function the kernel calls) gives every (panel, chunk) to exactly one
    workgroup, launches none without a task, keeps whole groups of eight panels on one XCD each, cuts the tail into
    eight contiguous near-equal ranges, and places every task's sums where the padded grid places them."""
    for npanels in range(1, 41):
        for bpp in (1, 2, 3, 5, 8, 13, 86, 131):
            t, ntasks = npanels % 8, npanels * bpp
            # the padded grid: one position per (group, chunk, XCD); workgroup = position
            gp, panel_p, chunk_p, pos_p = _task_map(npanels, bpp, False)
            assert gp == (npanels + 7) // 8 * 8 * bpp
            assert np.array_equal(pos_p, np.arange(gp))
            live = panel_p >= 0
            assert live.sum() == ntasks and (panel_p[live] < npanels).all()
            where = {(int(p), int(c)): int(w) for w, (p, c) in enumerate(zip(panel_p, chunk_p)) if p >= 0}
            assert len(where) == ntasks
            for (p, c), w in where.items():
                assert w == ((p // 8) * bpp + c) * 8 + p % 8
            # the balanced grid
            g, panel, chunk, pos = _task_map(npanels, bpp, True)
            assert g == ntasks                                    # no workgroup without a task
            assert (panel >= 0).all() and (panel < npanels).all() and (chunk >= 0).all() and (chunk < bpp).all()
            assert len(set(zip(panel.tolist(), chunk.tolist()))) == ntasks  # every task exactly once
            assert all(where[(int(p), int(c))] == int(s) for p, c, s in zip(panel, chunk, pos))  # sums where they were
            full = (npanels - t) * bpp
            assert np.array_equal(panel[:full], panel_p[:full]) and np.array_equal(chunk[:full], chunk_p[:full])
            assert (panel[:full] % 8 == np.arange(full) % 8).all()  # whole groups: panel p on XCD p % 8
            if t == 0:
                assert g == gp
                continue
            # tail: XCD x (workgroups = x mod 8, in launch order) walks one contiguous range of the (panel, chunk) list
            order = (panel[full:].astype(np.int64) - (npanels - t)) * bpp + chunk[full:]
            ranges = [order[x::8] for x in range(8)]
            lens = [len(r) for r in ranges]
            assert max(lens) - min(lens) <= 1 and sum(lens) == t * bpp
            nxt = 0
            for r in ranges:
                assert np.array_equal(r, np.arange(nxt, nxt + len(r)))
                nxt += len(r)
    from edipack_amd import capi
    assert capi.lib().edigpu_tile_task_map(0, 4, 1, None, None, None, None, None) != 0
