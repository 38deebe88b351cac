#!/usr/bin/env python
"""Times the ED_TWIN=T reorder on the device (edigpu_apply_twin) against two yardsticks taken in the same process, writes
profiles/twin.json and prints the table of DESIGN.md section 6.

Sectors:
  cfg2     normal mode, config 2 (Ns = 14): (7, 6) -> (6, 7), DimUp = 3432 != DimDw = 3003
  ns16     normal mode, the 3-orbital hybrid model at Ns = 16: (8, 7) -> (7, 8), 12870 x 11440
  superc   config 4 at Ns = 12: Sz = 1 -> -1 (the table gather)
  nonsu2   config 5 (Ns = 13, on the fly): Ntot = 13, its own twin (the reversal)

Per sector, one vector:
  twin_ms   edigpu_time_twin: the median of `--steps` runs after `--warmup`, each between two HIP events
  copy_ms   the ceiling: a device copy of a buffer of the vector's size at the copy figure of edigpu_membw
            (bytes read + written per second) measured on that size
  host_ms   what a host does today: edigpu_dev_download + the numpy reorder + edigpu_dev_upload, wall clock, the same
            number of runs
and the ratios twin / copy and host / twin.  The result is compared with numpy before timing (bit for bit).

    python scripts/time_twin.py [--steps 21] [--warmup 3] [--sectors cfg2,ns16,superc,nonsu2] [--out profiles/twin.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sectors", default="cfg2,ns16,superc,nonsu2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twin.json"))
    args = ap.parse_args()
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian as H, sector_map, twin_sector
    from edipack_amd.synthetic import WORKLOADS, synthetic_model
    if capi.device_count() < 1:
        raise SystemExit("time_twin.py: no HIP device (there is nothing to time on a CPU)")
    capi.init(0)
    L = capi.lib()
    plan = {"cfg2": ("cfg2", 0, (7, 6)), "ns16": ("cfg3_ns16", 0, (8, 7)), "superc": ("cfg4_ns12", 1, 1), "nonsu2": ("cfg5", 2, 13)}
    out = {"script": "scripts/time_twin.py", "kernel_source_hash": capi.kernel_source_hash(), "steps": args.steps,
           "warmup": args.warmup, "sectors": []}
    for key in args.sectors.split(","):
        wname, mode, sec = plan[key]
        w = WORKLOADS[wname]
        pm = synthetic_model(w)
        if mode == 0:
            t1, t2, self_twin = twin_sector(pm, 0, *sec)
            a = H.normal_from_model(pm, *sec)
            b = a if self_twin else H.normal_from_model(pm, t1, t2)
            order = None
            twin_label = [t1, t2]
        else:
            t1, _, self_twin = twin_sector(pm, mode, sec)
            build = H.direct_from_model if w.direct else H.flat_from_model
            a = build(pm, sec)
            b = a if self_twin else build(pm, t1)
            ns = pm.ns
            if mode == 1:
                s = sector_map(pm, sec).astype(np.int64)
                order = np.argsort(((s & ((1 << ns) - 1)) << ns) | (s >> ns), kind="stable")
            else:
                order = np.arange(a.dim - 1, -1, -1)
            twin_label = [t1]
        dt = torch.complex128 if a.is_complex else torch.float64
        nbytes = a.dim * (16 if a.is_complex else 8)
        gen = torch.Generator(device="cuda").manual_seed(1234)
        x = torch.randn(a.dim * (2 if a.is_complex else 1), dtype=torch.float64, device="cuda", generator=gen)
        x = torch.view_as_complex(x.view(-1, 2)) if a.is_complex else x
        y = torch.zeros(a.dim, dtype=dt, device="cuda")

        def host_reorder(v):
            if order is None:
                return np.ascontiguousarray(v.reshape(a.dim_dw, a.dim_up).T).reshape(-1)
            return v[order]

        a.twin_to(b, x.data_ptr(), y.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        xh = x.cpu().numpy()
        equal = bool(np.array_equal(y.cpu().numpy().view(np.float64), host_reorder(xh).view(np.float64)))
        twin_ms = a.time_twin(b, x.data_ptr(), y.data_ptr(), args.warmup, args.steps)
        copy_gbs = capi.membw(nbytes)[1]
        copy_ms = 2.0 * nbytes / (copy_gbs * 1e9) * 1e3
        hv = np.empty(a.dim, dtype=np.complex128 if a.is_complex else np.float64)
        ts = []
        for k in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            capi.check(L.edigpu_dev_download(hv.ctypes.data_as(C.c_void_p), x.data_ptr(), nbytes), "edigpu_dev_download")
            r = host_reorder(hv)
            capi.check(L.edigpu_dev_upload(y.data_ptr(), r.ctypes.data_as(C.c_void_p), nbytes), "edigpu_dev_upload")
            ts.append((time.perf_counter() - t0) * 1e3)
        host_ms = float(np.median(ts[args.warmup:]))
        out["sectors"].append({"name": key, "workload": wname, "mode": ("normal", "superc", "nonsu2")[mode],
                               "sector": list(sec) if mode == 0 else [sec], "twin": twin_label, "self_twin": bool(self_twin),
                               "dim": a.dim, "dim_up": a.dim_up, "dim_dw": a.dim_dw, "complex": bool(a.is_complex),
                               "vector_bytes": nbytes, "bit_equal_numpy": equal, "twin_ms": twin_ms,
                               "twin_GBs_read_plus_written": 2.0 * nbytes / (twin_ms * 1e-3) / 1e9, "membw_copy_GBs": copy_gbs,
                               "copy_ms": copy_ms, "host_roundtrip_ms": host_ms, "twin_over_copy": twin_ms / copy_ms,
                               "host_over_twin": host_ms / twin_ms})
        if b is not a:
            b.destroy()
        a.destroy()
        del x, y
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print("| sector | elements | MB | twin ms | copy ms (GB/s) | twin / copy | host round trip ms | host / twin |")
    print("|---|---|---|---|---|---|---|---|")
    for s in out["sectors"]:
        print(f"| {s['name']} {s['sector']} -> {s['twin']} | {s['dim']} | {s['vector_bytes'] / 1e6:.0f} | {s['twin_ms']:.4f} | "
              f"{s['copy_ms']:.4f} ({s['membw_copy_GBs']:.0f}) | {s['twin_over_copy']:.2f} | {s['host_roundtrip_ms']:.1f} | "
              f"{s['host_over_twin']:.0f} |")
    assert all(s["bit_equal_numpy"] for s in out["sectors"])


if __name__ == "__main__":
    main()
