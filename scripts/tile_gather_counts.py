#!/usr/bin/env python3
"""Host only: what the tiled column sweep (normal_dw_tile_kernel) asks the L2 for, counted on the library's own lists
of a workload (plan_tile_chunks + build_tile_lists through the test shim tests/host_pack.cpp, compiled with g++).

    python scripts/tile_gather_counts.py [--workload cfg2] [--rmax 32]

Per down row: hops that leave the row's chunk as the format pads them (whole batches of four) and live (what the
kernel gathers), Hnd partner rows inside / outside the chunk, dependent L2 round trips (batches + partner loads)."""
import argparse
import collections
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2")
    ap.add_argument("--rmax", type=int, default=32)
    a = ap.parse_args()
    from edipack_amd.synthetic import WORKLOADS, synthetic_model
    from tests.test_host_pack import F64, I32, I64, U32, Csr, plan, ptr
    w = WORKLOADS[a.workload]
    assert w.ed_mode == "normal"
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "host_pack.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                               "-o", so, os.path.join(ROOT, "tests", "host_pack.cpp"), os.path.join(csrc, "host_pack.cpp"),
                               os.path.join(csrc, "host_build.cpp")])
        lib = C.CDLL(so)
    VP, L, I = C.c_void_p, C.c_int64, C.c_int
    lib.hp_error.restype = C.c_char_p
    lib.hp_build_normal.argtypes = [VP, I, I, VP]
    lib.hp_get_csr.argtypes = [I, VP, VP, VP]
    lib.hp_get_fac.argtypes = [VP, VP, VP]
    lib.hp_chunks.argtypes = [L, VP, VP, VP, L, L, I, VP, VP]
    lib.hp_tile.argtypes = [L, VP, VP, VP, I, I, VP, VP, L, L, VP, I, VP]
    lib.hp_tile_get.argtypes = [VP] * 4
    m = synthetic_model(w).to_c()
    dims = np.zeros(5, I64)
    assert lib.hp_build_normal(C.addressof(m), *w.sector, ptr(dims)) == 0, lib.hp_error().decode()
    du, dd, _, nd, nt = (int(x) for x in dims)
    rp, col, val = np.zeros(dd + 1, I64), np.zeros(nd, I32), np.zeros(nd, F64)
    lib.hp_get_csr(1, ptr(rp), ptr(col), ptr(val))
    dw = Csr.from_arrays(rp, col, val)
    coef, jdw, jup = np.zeros(max(nt, 0), F64), np.zeros(max(nt, 0) * dd, U32), np.zeros(max(nt, 0) * du, U32)
    lib.hp_get_fac(ptr(coef), ptr(jdw), ptr(jup))
    starts = plan(lib, dw, 0, dd, a.rmax)
    info = np.zeros(6, I64)
    lib.hp_tile(dd, *dw.args(), int(nt > 0), len(coef), ptr(coef), ptr(jdw), 0, dd, ptr(starts), len(starts), ptr(info))
    meta, tcol, tval, lbeg = np.zeros((info[0], 4), I32), np.zeros(info[1], I32), np.zeros(info[2], F64), np.zeros(info[3], I32)
    lib.hp_tile_get(ptr(meta), ptr(tcol), ptr(tval), ptr(lbeg))
    padded = live = pin = pout = batches = live_batches = 0
    hist = collections.Counter()
    for ch in range(len(starts) - 1):
        cs, ce = int(starts[ch]), int(starts[ch + 1])
        for r in range(cs, ce):
            x, y, z, nnd = (int(v) for v in meta[r])
            oc = tcol[x + y:x + y + z]
            nl = z
            while nl % 4 != 1 and nl > 0 and oc[nl - 1] == r and tval[x + y + nl - 1] == 0.0:
                nl -= 1
            padded += z
            live += nl
            hist[nl] += 1
            batches += z // 4
            for q in range(x + y + z, x + y + z + nnd):
                p = int(tcol[q]) & 0xFFFFFF
                if cs <= p < ce:
                    pin += 1
                else:
                    pout += 1
    sizes = np.diff(starts)
    nhop = int(rp[-1])
    print(f"{a.workload}: DimUp={du} ({(du + 127) // 128} panels of 128 columns) DimDw={dd} Hnd terms={nt} rmax={a.rmax}")
    print(f"chunks: {len(sizes)} of {sizes.min()}-{sizes.max()} rows, mean {sizes.mean():.1f}; "
          f"sizes {dict(sorted(collections.Counter(sizes.tolist()).items()))}")
    print(f"hops per row: {nhop / dd:.2f}")
    print(f"hops leaving the chunk per row: padded {padded / dd:.2f}, live {live / dd:.2f}")
    print(f"live outside hops per row -> rows: {dict(sorted(hist.items()))}")
    print(f"Hnd partner rows per row: {(pin + pout) / dd:.2f}; inside the chunk {pin} of {pin + pout} "
          f"({100.0 * pin / max(1, pin + pout):.1f} %), outside {pout / dd:.3f} per row")
    before, after = (padded + pin + pout) / dd, (live + pout) / dd
    print(f"1 KiB L2 gathers per row: before {before:.2f}, now {after:.2f} ({100.0 * (after / before - 1.0):+.0f} %)")
    print(f"dependent L2 round trips per row (batches + partner loads): before {batches / dd:.2f} + {(pin + pout) / dd:.2f}, "
          f"now {batches / dd:.2f} + {pout / dd:.2f}")
    npan = (du + 127) // 128
    print(f"128-byte L2 requests removed per product: {(before - after) * dd * npan * 8 / 1e6:.2f} M "
          f"({before - after:.2f} gathers x {dd} rows x {npan} panels x 8)")


if __name__ == "__main__":
    main()
