"""What the tiled column sweep (kernels_panel.hip: normal_dw_tile_kernel) relies on since it gathers the live entries
of a row's outside list only and reads a staged Hnd partner row from its LDS tile: in the lists of build_tile_lists
(through the shim of test_host_pack.py, whose format test stays the reference for the rest)
  * the zero-weight entries of an outside list are exactly its trailing ones, fewer than four, and name the row itself;
  * no live outside entry names the row itself (a row lies inside its own chunk), so the padding is recognisable;
  * the row meta the device gets (host_pack.cpp: tile_meta_live, through tests/tile_live.cpp) is the format's meta with
    the outside count replaced by the live count.
The case must contain what can go wrong in the kernel, and the test asserts that it does: live counts of every residue
mod 4 (0: no partial batch; 1-3: the three straight-line paths), a row without outside hops, and Hnd partner rows
both inside their row's chunk (read from the tile) and outside it (the chunk cut separates the pair: global read)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_host_pack import I32, I64, F64, ROOT, plan, ptr, sector44, shim  # noqa: F401  (fixtures)


@pytest.fixture(scope="module")
def live_shim(shim, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tile_live") / "tile_live.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           "-o", so, os.path.join(ROOT, "tests", "tile_live.cpp"), os.path.join(csrc, "host_pack.cpp")])
    lib = C.CDLL(so)
    lib.tl_meta_live.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return lib


def tile_lists(lib, dw, coef, jdw, with_nd, first, count, starts):
    info = np.zeros(6, I64)
    lib.hp_tile(dw.nrow, *dw.args(), int(with_nd), len(coef), ptr(coef), ptr(jdw), first, count, ptr(starts), len(starts), ptr(info))
    meta, col, val, lbeg = np.zeros((info[0], 4), I32), np.zeros(info[1], I32), np.zeros(info[2], F64), np.zeros(info[3], I32)
    lib.hp_tile_get(ptr(meta), ptr(col), ptr(val), ptr(lbeg))
    return meta, col, val


CASES = [(rmax, first, count) for rmax in (8, 32) for first, count in ((0, None), (5, 40))] + [("pairs", 0, None)]


@pytest.mark.parametrize("rmax,first,count", CASES)
@pytest.mark.parametrize("with_nd", [False, True])
def test_outside_padding_is_trailing_and_names_the_row(shim, live_shim, sector44, rmax, first, count, with_nd):
    """rmax 8 / 32: the planner's chunks.  "pairs": a hand-made partition (any partition is a valid plan) that cuts
    between the two rows of every second Hnd pair, because the planner's own cuts separate none of the 40 partners of
    this sector -- nor any of the 1848 of config 2 (scripts/tile_gather_counts.py)."""
    _, dw, coef, jdw, _ = sector44
    count = dw.nrow if count is None else count
    if rmax == "pairs":
        between = [g for g in range(1, dw.nrow) if jdw[g] != 0xFFFFFFFF and (int(jdw[g]) & 0xFFFFFF) == g - 1]
        starts = np.array([0] + between[::2] + [dw.nrow], I32)
    else:
        starts = plan(shim, dw, first, count, rmax)
    meta, col, val = tile_lists(shim, dw, coef, jdw, with_nd, first, count, starts)
    live = np.zeros_like(meta)
    live_shim.tl_meta_live(count, ptr(meta), col.size, ptr(col), ptr(val), first, ptr(live))
    residues, no_outside, partners_in, partners_out = set(), 0, 0, 0
    for ch in range(len(starts) - 1):
        cs, ce = int(starts[ch]), int(starts[ch + 1])
        for r in range(cs, ce):
            g = first + r
            x, y, z, nnd = (int(v) for v in meta[r])
            oc, ov = col[x + y:x + y + z], val[x + y:x + y + z]
            nlive = int(np.count_nonzero(ov))
            assert z == (nlive + 3) // 4 * 4                          # fewer than four padding entries
            assert (ov[:nlive] != 0).all() and (ov[nlive:] == 0).all()  # ... and they are the trailing ones
            assert (oc[nlive:] == g).all()                            # padding names the row itself
            assert (oc[:nlive] != g).all()                            # which no live entry does
            assert live[r].tolist() == [x, y, nlive, nnd]             # what the device reads
            residues.add(nlive % 4)
            no_outside += nlive == 0
            for q in range(x + y + z, x + y + z + nnd):
                prow = int(col[q]) & 0xFFFFFF
                if first + cs <= prow < first + ce:
                    partners_in += 1
                else:
                    partners_out += 1
    print(f"rmax={rmax} first={first} count={count} nd={with_nd}: chunks={len(starts) - 1} residues={sorted(residues)} "
          f"rows without outside hops={no_outside} partners inside={partners_in} outside={partners_out}")
    if first == 0:   # the whole sector; the shard (5, 40) checks the lists of a dw_first != 0 caller
        assert residues == {0, 1, 2, 3}
        assert no_outside > 0
    assert (partners_in > 0) == with_nd
    assert (partners_out > 0) == (with_nd and rmax == "pairs")
