#!/usr/bin/env python
"""Times edigpu_imp_rdm on two normal-mode sectors, or edigpu_imp_rdm_flat on two superc / nonsu2 sectors, and prints ONE
JSON line (profiles/rdm.json holds the sectors of both):

  cfg2        Ns=14 (7,7), two orbitals, 94 MB per vector (inside the 256 MiB Infinity Cache)
  cfg3_ns16   Ns=16 (8,8), three orbitals, 1.33 GB per vector: the HBM-resident sector of bench.py
  cfg5        nonsu2 on the fly, Ns=13, N=13, three orbitals, complex, 166 MB per vector
  superc_ns13 superc on the fly, Ns=13, Sz=0, two orbitals, the same size

Per sector, in this one process: the median of the imp_rdm kernels over >= 20 runs between HIP events after a warm-up
(edigpu_time_rdm), the occ_moments median on the same vector (edigpu_time_occ: the same single pass over v), the read
ceiling of edigpu_membw on a buffer of the vector's size, and what a host has to do without this entry point:
edigpu_dev_download of the vector plus the numpy restatement of imp_rdm_normal (tests/test_rdm_host.py::numpy_rdm) on
it (wall clock, once); for the flat sectors the restatement is tests/rdm_flat_cases.py::numpy_rdm_flat.

    python scripts/time_rdm.py [--workloads cfg2,cfg3_ns16 | cfg5,superc_ns13] [--steps 21]

--sharded times edigpu_imp_rdm_sharded instead (the flat workloads: edigpu_imp_rdm_flat_sharded): a world of ONE rank on
the RCCL communicator with its collectives forced (EDIGPU_FORCE_COLLECTIVES=1), the vector passed as a device pointer,
against edigpu_imp_rdm (edigpu_imp_rdm_flat) on the same vector -- both as whole calls by the wall clock (kernels, the
download of the packed result, its placement), medians of --steps calls after --warmup.  A one-GPU rehearsal of the
calls, not a scaling measurement: the line goes into profiles/rdm.json under "sharded_rehearsal" (the flat workloads:
"flat_sharded_rehearsal").
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


def host_baseline(h, model, sector, v_ptr):
    """seconds of (download, numpy rho) for the vector at v_ptr, and rho"""
    from edipack_amd import capi
    from edipack_amd.hamiltonian import sector_map
    from tests.test_rdm_host import numpy_rdm
    flat = model.ed_mode != "normal"
    if flat:
        from tests.rdm_flat_cases import numpy_rdm_flat
    v = np.empty(h.dim, dtype=h.dtype)
    t0 = time.perf_counter()
    capi.check(capi.lib().edigpu_dev_download(v.ctypes.data_as(C.c_void_p), C.c_void_p(v_ptr), v.nbytes), "edigpu_dev_download")
    t1 = time.perf_counter()
    if flat:
        mp = sector_map(model, sector)
        t2 = time.perf_counter()
        rho = numpy_rdm_flat(mp, model.ns, model.norb, v)
        return t1 - t0, time.perf_counter() - t2, rho
    mu, md = sector_map(model, sector[0], sector[1], 0), sector_map(model, sector[0], sector[1], 1)
    t2 = time.perf_counter()
    rho = numpy_rdm(mu, md, model.norb, v)
    t3 = time.perf_counter()
    return t1 - t0, t3 - t2, rho


def wall_median_ms(call, warmup, steps):
    ts = []
    for k in range(warmup + steps):
        t0 = time.perf_counter()
        call()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def sharded_rehearsal(args):
    os.environ["EDIGPU_FORCE_COLLECTIVES"] = "1"          # read when the communicator is made
    import torch
    from edipack_amd import capi
    from edipack_amd.sharding import LibraryComm
    from edipack_amd.synthetic import WORKLOADS, Workload, build_workload
    workloads = dict(WORKLOADS)
    workloads["superc_ns13"] = SUPERC_NS13(Workload)
    capi.init(0)
    comm = LibraryComm(0, 1, unique_id=LibraryComm.unique_id())
    out = {"script": "scripts/time_rdm.py --sharded", "kernel_source_hash": capi.kernel_source_hash(), "steps": args.steps,
           "warmup": args.warmup, "world": 1, "collectives": "forced (RCCL)", "sectors": []}
    for name in args.workloads.split(","):
        w = workloads[name]
        flat = w.ed_mode != "normal"
        h = build_workload(w)
        one, sharded, kernels = (h.imp_rdm_flat, comm.imp_rdm_flat, h.time_rdm_flat) if flat else (h.imp_rdm, comm.imp_rdm, h.time_rdm)
        gen = torch.Generator(device="cuda").manual_seed(1234)
        v = torch.randn(h.dim * (2 if h.is_complex else 1), dtype=torch.float64, device="cuda", generator=gen)
        torch.cuda.synchronize()
        rho, n2 = one(v.data_ptr())
        rho_s, n2_s = sharded(h, v.data_ptr())
        ms_one = wall_median_ms(lambda: one(v.data_ptr()), args.warmup, args.steps)
        ms_sh = wall_median_ms(lambda: sharded(h, v.data_ptr()), args.warmup, args.steps)
        ms_kernels = kernels(v.data_ptr(), args.warmup, args.steps)
        out["sectors"].append({"workload": name, "entry": "edigpu_imp_rdm_flat_sharded" if flat else "edigpu_imp_rdm_sharded",
                               "note": w.note, "dim": h.dim, "norb": h.norb,
                               "imp_rdm_call_ms": ms_one, "imp_rdm_sharded_call_ms": ms_sh, "ratio": ms_sh / ms_one,
                               "imp_rdm_kernels_ms": ms_kernels,
                               "same_bits": bool(np.array_equal(rho, rho_s) and np.array_equal(n2, n2_s))})
        h.destroy()
        del v
        torch.cuda.empty_cache()
    comm.destroy()
    print(json.dumps(out))


def SUPERC_NS13(Workload):
    return Workload("superc_ns13", 4, "superc", "hybrid", 2, 11, 0, "Ns=13, Sz=0, Dim=10 400 600, direct", True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg2,cfg3_ns16")
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sharded", action="store_true", help="one-rank rehearsal of edigpu_imp_rdm[_flat]_sharded against edigpu_imp_rdm[_flat]")
    args = ap.parse_args()
    if args.sharded:
        return sharded_rehearsal(args)
    import torch
    from edipack_amd import capi
    from edipack_amd.synthetic import WORKLOADS, Workload, build_workload, synthetic_model
    workloads = dict(WORKLOADS)
    workloads["superc_ns13"] = SUPERC_NS13(Workload)
    if capi.device_count() < 1:
        raise SystemExit("time_rdm.py: no HIP device (there is nothing to time on a CPU)")
    capi.init(0)
    out = {"script": "scripts/time_rdm.py", "kernel_source_hash": capi.kernel_source_hash(),
           "steps": args.steps, "warmup": args.warmup, "sectors": []}
    for name in args.workloads.split(","):
        w = workloads[name]
        model = synthetic_model(w)
        h = build_workload(w)
        flat = w.ed_mode != "normal"
        width = 2 if h.is_complex else 1
        gen = torch.Generator(device="cuda").manual_seed(1234)
        v = torch.randn(h.dim * width, dtype=torch.float64, device="cuda", generator=gen)
        torch.cuda.synchronize()
        nbytes = h.dim * 8 * width
        rdm, time_rdm = (h.imp_rdm_flat, h.time_rdm_flat) if flat else (h.imp_rdm, h.time_rdm)
        rho, n2 = rdm(v.data_ptr())                   # first call: builds the tables; the result checks the baseline
        t_down, t_numpy, rho_host = host_baseline(h, model, w.sector, v.data_ptr())
        agree = float(np.max(np.abs(rho[0] - rho_host)) / n2[0])
        ms_rdm = time_rdm(v.data_ptr(), args.warmup, args.steps)
        ms_mom, _ = h.time_occ(v.data_ptr(), args.warmup, args.steps)   # overwrites v
        del v
        torch.cuda.empty_cache()
        read, _, _ = capi.membw(max(nbytes, 1 << 20))
        gbs_rdm, gbs_mom = nbytes / (ms_rdm * 1e-3) / 1e9, nbytes / (ms_mom * 1e-3) / 1e9
        out["sectors"].append({
            "workload": name, "entry": "edigpu_imp_rdm_flat" if flat else "edigpu_imp_rdm", "note": w.note, "dim": h.dim, "norb": model.norb, "vector_bytes": nbytes,
            "imp_rdm": {"ms": ms_rdm, "GBs": gbs_rdm, "ceiling_read_GBs": read, "frac_of_ceiling": gbs_rdm / read,
                        "rate_over_occ_moments": ms_mom / ms_rdm},
            "occ_moments": {"ms": ms_mom, "GBs": gbs_mom, "frac_of_ceiling": gbs_mom / read},
            "host_baseline": {"download_ms": t_down * 1e3, "numpy_rdm_ms": t_numpy * 1e3,
                              "total_over_imp_rdm": (t_down + t_numpy) * 1e3 / ms_rdm,
                              "max_abs_diff_rho_over_norm2": agree}})
        h.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
