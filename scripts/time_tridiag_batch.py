#!/usr/bin/env python
"""Times the Green's-function phase of one target sector both ways and prints ONE JSON line (profiles/tridiag_batch.json):

  singles  nseed calls of edigpu_lanczos_tridiag_dev, one seed after another
  batch    one call of edigpu_lanczos_tridiag_batch_dev on the same seeds

by default on the stored config-4 sector (cfg4_ns12: superc, Ns=12, Sz=0, 2 704 156 rows, 43 MB per vector, 1.15 GB of matrix) and
the on-the-fly config-5 sector (cfg5: nonsu2, Ns=13, N=13, 10 400 600 rows, 166 MB per vector) of BASELINE.json, nlanc
steps, nseed in {2, 4, 8}; the smaller sectors cfg4 (184 756 rows), cfg5_ns11 (705 432), cfg4_ns8 (12 870) and cfg5_ns9
(48 620) show where the wider groups stop paying.  A leg is timed as wall clock around the calls (each returns after its stream has finished),
repeated `--repeats` times after one untimed run; reported: median, minimum and maximum in ms, and the median per seed
and step in us -- the figure the keep rule of DESIGN.md 4.10 compares.

--force-width times nseed = 2, 4, 8 as ONE group of that width (edigpu_batch_set_width) whatever the sector's default, which
on a large sector is pairs of seeds: the rows of DESIGN.md 6 that the default route no longer takes.  cfg4_ns6 (924 rows)
and cfg5_ns7 (3 432) are the smallest sectors of the table.

--singles-only runs the first leg alone and needs nothing this script's commit added, so the same file times a checkout
of the parent commit: that leg is the reference time.

    python scripts/time_tridiag_batch.py [--workloads cfg4_ns12,cfg5] [--nlanc 100] [--repeats 5] [--force-width] [--singles-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats):
    fn()  # untimed: allocations, first-launch set-up
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg4_ns12,cfg5")
    ap.add_argument("--nlanc", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nseeds", default="2,4,8")
    ap.add_argument("--singles-only", action="store_true")
    ap.add_argument("--force-width", action="store_true",
                    help="time nseed = 2, 4, 8 at width 2, 4, 8 whatever the sector's default (edigpu_batch_set_width)")
    args = ap.parse_args()
    import torch
    from edipack_amd import capi
    from edipack_amd.synthetic import WORKLOADS, Workload, build_workload
    workloads = dict(WORKLOADS)
    # small sectors of the same two structures: where the widths that lose on the large ones are kept
    workloads["cfg4_ns8"] = Workload("cfg4_ns8", 4, "superc", "hybrid", 2, 6, 0, "Ns=8, Sz=0, Dim=12 870")
    workloads["cfg5_ns9"] = Workload("cfg5_ns9", 5, "nonsu2", "hybrid", 3, 6, 9, "Ns=9, N=9, Dim=48 620, direct", True)
    workloads["cfg4_ns6"] = Workload("cfg4_ns6", 4, "superc", "hybrid", 2, 4, 0, "Ns=6, Sz=0, Dim=924")
    workloads["cfg5_ns7"] = Workload("cfg5_ns7", 5, "nonsu2", "hybrid", 3, 4, 7, "Ns=7, N=7, Dim=3 432, direct", True)
    if capi.device_count() < 1:
        raise SystemExit("time_tridiag_batch.py: no HIP device (there is nothing to time on a CPU)")
    capi.init(0)
    out = {"script": "scripts/time_tridiag_batch.py", "nlanc": args.nlanc, "repeats": args.repeats,
           "singles_only": bool(args.singles_only), "force_width": bool(args.force_width), "sectors": []}
    if hasattr(capi, "kernel_source_hash"):
        out["kernel_source_hash"] = capi.kernel_source_hash()
    nseeds = [int(x) for x in args.nseeds.split(",")]
    for name in args.workloads.split(","):
        w = workloads[name]
        h = build_workload(w)
        width = 2 if h.is_complex else 1
        gen = torch.Generator(device="cuda").manual_seed(1234)
        seeds = torch.randn(max(nseeds), h.dim * width, dtype=torch.float64, device="cuda", generator=gen)
        torch.cuda.synchronize()
        rec = {"workload": name, "kind": "direct" if w.direct else "stored", "rows": int(h.dim),
               "vector_MB": h.dim * 8 * width / 1e6, "runs": []}
        for n in nseeds:
            def singles():
                return [h.lanczos_tridiag_dev(seeds[j].data_ptr(), args.nlanc) for j in range(n)]
            r = {"nseed": n, "singles": timed(singles, args.repeats)}
            r["singles"]["us_per_seed_step"] = r["singles"]["median_ms"] * 1e3 / (n * args.nlanc)
            if not args.singles_only:
                if args.force_width:
                    h.batch_set_width(2 if n <= 2 else 4 if n <= 4 else 8)

                def batch():
                    return h.lanczos_tridiag_batch_dev(seeds.data_ptr(), n, args.nlanc)
                r["batch"] = timed(batch, args.repeats)
                r["batch"]["us_per_seed_step"] = r["batch"]["median_ms"] * 1e3 / (n * args.nlanc)
                one, all_ = singles(), batch()
                r["route"] = int(all_[4])
                r["niter_equal"] = bool(all(int(all_[2][j]) == one[j][2] for j in range(n)))
                r["max_rel_diff_alpha15"] = float(max(
                    np.max(np.abs(all_[0][j][:15] - one[j][0][:15])) / np.max(np.abs(one[j][0][:15])) for j in range(n)))
                r["speedup"] = r["singles"]["median_ms"] / r["batch"]["median_ms"]
            rec["runs"].append(r)
        out["sectors"].append(rec)
        h.destroy()
        del seeds
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
