#!/usr/bin/env python
"""Times edigpu_occ_moments and edigpu_apply_occ on three sectors and prints ONE JSON line (profiles/occupations.json):

  cfg2        normal mode, Ns=14 (7,7), 94 MB per vector (inside the 256 MiB Infinity Cache)
  cfg3_ns16   normal mode, Ns=16 (8,8), 1.33 GB per vector: the HBM-resident sector of bench.py
  cfg5        nonsu2 on the fly, 10.4 M rows, complex, 166 MB per vector

Per sector, in this one process: the kernels' medians over >= 20 runs between HIP events after a warm-up
(edigpu_time_occ), the streaming ceilings of edigpu_membw on buffers of the vector's size -- read (gbs3[0]) for
occ_moments, copy (gbs3[1]) for apply_occ -- and what a host has to do without these entry points: edigpu_dev_download of
the vector plus the numpy evaluation of tests/observables.py::dens_docc on it (wall clock, once).

    python scripts/time_occupations.py [--workloads cfg2,cfg3_ns16,cfg5] [--steps 21]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_baseline(h, model, sector, v_ptr):
    """seconds of (download, numpy dens/docc) for the vector at v_ptr"""
    from edipack_amd import capi
    from edipack_amd.hamiltonian import sector_map
    from tests import observables as ob
    v = np.empty(h.dim, dtype=h.dtype)
    t0 = time.perf_counter()
    capi.check(capi.lib().edigpu_dev_download(v.ctypes.data_as(C.c_void_p), C.c_void_p(v_ptr), v.nbytes), "edigpu_dev_download")
    t1 = time.perf_counter()
    om = SimpleNamespace(ed_mode=model.ed_mode, norb=model.norb, ns=model.ns)
    if model.ed_mode == "normal":
        mu, md = sector_map(model, sector[0], sector[1], 0), sector_map(model, sector[0], sector[1], 1)
        ho = SimpleNamespace(dim=h.dim, dimup=mu.size, mapup=mu.astype(np.int64), mapdw=md.astype(np.int64))
    else:
        ho = SimpleNamespace(dim=h.dim, map=sector_map(model, sector).astype(np.int64))
    t2 = time.perf_counter()
    dens, docc = ob.dens_docc(om, [(sector, ho, v)])
    t3 = time.perf_counter()
    return t1 - t0, t3 - t2, dens, docc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg2,cfg3_ns16,cfg5")
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from edipack_amd import capi
    from edipack_amd.observables import from_moments
    from edipack_amd.synthetic import WORKLOADS, build_workload, synthetic_model
    if capi.device_count() < 1:
        raise SystemExit("time_occupations.py: no HIP device (there is nothing to time on a CPU)")
    capi.init(0)
    out = {"script": "scripts/time_occupations.py", "kernel_source_hash": capi.kernel_source_hash(),
           "steps": args.steps, "warmup": args.warmup, "sectors": []}
    for name in args.workloads.split(","):
        w = WORKLOADS[name]
        model = synthetic_model(w)
        h = build_workload(w)
        wd = 2 if h.is_complex else 1
        gen = torch.Generator(device="cuda").manual_seed(1234)
        v = torch.randn(h.dim * wd, dtype=torch.float64, device="cuda", generator=gen)
        torch.cuda.synchronize()
        nbytes = h.dim * wd * 8
        M, n2 = h.occ_moments(v.data_ptr())           # first call: builds the tables; the result checks the baseline
        t_down, t_numpy, dens, docc = host_baseline(h, model, w.sector, v.data_ptr())
        o = from_moments(M[0], model.norb, norm2=n2[0])
        agree = float(max(np.max(np.abs(o.dens - dens / n2[0])), np.max(np.abs(o.docc - docc / n2[0]))))
        ms_mom, ms_app = h.time_occ(v.data_ptr(), args.warmup, args.steps)
        del v
        torch.cuda.empty_cache()
        read, copy, _ = capi.membw(max(nbytes, 1 << 20))
        gbs_mom, gbs_app = nbytes / (ms_mom * 1e-3) / 1e9, 2 * nbytes / (ms_app * 1e-3) / 1e9
        out["sectors"].append({
            "workload": name, "note": w.note, "dim": h.dim, "complex": h.is_complex, "norb": model.norb,
            "vector_bytes": nbytes,
            "occ_moments": {"ms": ms_mom, "GBs": gbs_mom, "ceiling_read_GBs": read, "frac_of_ceiling": gbs_mom / read},
            "apply_occ": {"ms": ms_app, "GBs": gbs_app, "ceiling_copy_GBs": copy, "frac_of_ceiling": gbs_app / copy},
            "host_baseline": {"download_ms": t_down * 1e3, "numpy_dens_docc_ms": t_numpy * 1e3,
                              "total_over_occ_moments": (t_down + t_numpy) * 1e3 / ms_mom,
                              "max_abs_diff_dens_docc": agree}})
        h.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
