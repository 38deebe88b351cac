#!/usr/bin/env python
"""Times edigpu_ph_rdm and edigpu_apply_xph on phonon sectors and prints ONE JSON line (profiles/phonons.json).

A case is norb:nbath:nup:ndw:nph of the normal / normal family of tests/common.py::make_models.  The defaults:

  3:3:6:6:7   924^2 electronic states, DimPh 8: 54.6 MB per vector (inside the 256 MiB Infinity Cache)
  3:4:7:7:1   6435^2 electronic states, DimPh 2: 662 MB per vector, HBM resident

Per case, in this one process: the kernels' medians over >= 20 runs between HIP events after a warm-up (edigpu_time_ph),
the streaming ceilings of edigpu_membw on buffers of the vector's size -- read (gbs3[0]) for ph_rdm, copy (gbs3[1]) for
apply_xph, which reads and writes the vector once -- and the occ_moments median of edigpu_time_occ on the same handle
and vector (the same single pass over v, 56 sums instead of 3^norb DimPh (DimPh + 1) / 2).

    python scripts/time_phonons.py [--cases 3:3:6:6:7,3:4:7:7:1] [--steps 21]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="3:3:6:6:7,3:4:7:7:1")
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian
    from edipack_amd.observables import from_ph_rdm
    from tests.common import make_models
    if capi.device_count() < 1:
        raise SystemExit("time_phonons.py: no HIP device (there is nothing to time on a CPU)")
    capi.init(0)
    out = {"script": "scripts/time_phonons.py", "kernel_source_hash": capi.kernel_source_hash(),
           "steps": args.steps, "warmup": args.warmup, "sectors": []}
    for case in args.cases.split(","):
        norb, nbath, nup, ndw, nph = (int(x) for x in case.split(":"))
        _, pm = make_models("normal", "normal", norb, nbath, seed=11)
        pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = nph, 0.8, 0.0, np.diag(np.linspace(0.3, 0.5, norb))
        h = SectorHamiltonian.normal_from_model(pm, nup, ndw)
        gen = torch.Generator(device="cuda").manual_seed(1234)
        v = torch.randn(h.dim, dtype=torch.float64, device="cuda", generator=gen)
        w = torch.empty_like(v)
        torch.cuda.synchronize()
        nbytes = h.dim * 8
        rho, n2 = h.ph_rdm(v.data_ptr())                # first call: builds the tables
        o = from_ph_rdm(rho[0], norm2=n2[0])
        ms_rdm, ms_xph = h.time_ph(v.data_ptr(), w.data_ptr(), args.warmup, args.steps)
        M, on2 = h.occ_moments(v.data_ptr())
        ms_mom, _ = h.time_occ(w.data_ptr(), args.warmup, args.steps)   # on the seed: the same size, v stays intact
        del v, w
        torch.cuda.empty_cache()
        read, copy, _ = capi.membw(max(nbytes, 1 << 20))
        gbs_rdm, gbs_xph = nbytes / (ms_rdm * 1e-3) / 1e9, 2 * nbytes / (ms_xph * 1e-3) / 1e9
        out["sectors"].append({
            "case": case, "dim_el": h.dim // (nph + 1), "dimph": nph + 1, "dim": h.dim, "norb": norb, "vector_bytes": nbytes,
            "ph_rdm": {"ms": ms_rdm, "bytes_per_ms": nbytes / ms_rdm, "GBs": gbs_rdm, "ceiling_read_GBs": read,
                       "frac_of_ceiling": gbs_rdm / read, "over_occ_moments": ms_rdm / ms_mom},
            "apply_xph": {"ms": ms_xph, "bytes_per_ms": 2 * nbytes / ms_xph, "GBs": gbs_xph, "ceiling_copy_GBs": copy,
                          "frac_of_ceiling": gbs_xph / copy, "over_occ_moments": ms_xph / ms_mom},
            "occ_moments_ms": ms_mom,
            "checks": {"prob_ph_sum": float(o.prob_ph.sum()), "norm2_rel_diff_occ_moments": float(abs(on2[0] - n2[0]) / n2[0])}})
        h.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
