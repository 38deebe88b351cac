#!/usr/bin/env python
"""Times c / c^+ along one axis (kernels_axisop.hip through edigpu_apply_op_normal) and prints ONE JSON line
(profiles/axisop.json).

Cases, each with the up and the down operator of orbital 0 (ed_total_ud=F: every axis), annihilation:
  - the config-2 sector of bench.py (synthetic.WORKLOADS["cfg2"]: Ns = 14, (7, 7), 11.8 M elements) with nph = 0 -- the
    route that keeps apply_op_normal_kernel -- and with nph = 4 (five blocks, 59 M elements);
  - its complex twin (edigpu_normal_build_z, 23.6 M doubles);
  - an ed_total_ud=F sector of comparable size: two chains of 8 levels, nups = (4, 4), ndws = (4, 3), 19.2 M elements.
Per case edigpu_time_apply_op gives the median of the whole call as a caller pays it and of the kernel alone.  Two
comparisons come from the same run: the existing kernel on one electronic block times the number of blocks (what the
phonon sector costs block by block through nph = 0 handles), and the copy rate of edigpu_membw at the bytes the kernel
moves (it stores every destination element once and loads the live half of them).  The cases alternate over `--rounds`
rounds in this one process; over the rounds the median.

    python scripts/time_axisop.py [--steps 21] [--warmup 3] [--rounds 3]

--sharded times edigpu_apply_cops_sharded instead (profiles/axisop.json, key sharded_rehearsal): a world of ONE rank on the
RCCL communicator with the collectives forced (EDIGPU_FORCE_COLLECTIVES=1, so the all-gather is a real RCCL call), c up and
c down of orbital 0 on the config-2 sector with nph = 4, device vectors, against edigpu_apply_cops_normal on the same
vectors; both calls return after the device has finished and are timed on the host clock.  A rehearsal of the call's fixed
costs on one GPU, not a scaling figure.
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sharded(args):
    import time
    os.environ["EDIGPU_FORCE_COLLECTIVES"] = "1"
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian as H
    from edipack_amd.sharding import LibraryComm
    from edipack_amd.synthetic import WORKLOADS, synthetic_model
    if capi.device_count() < 1:
        raise SystemExit("time_axisop.py: no HIP device (there is nothing to time on a CPU)")
    capi.init(0)
    w = WORKLOADS["cfg2"]
    nup, ndw = w.sector
    nph = 4
    pm = synthetic_model(w)
    pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = nph, 0.8, 0.0, np.diag(np.linspace(0.3, 0.5, w.norb))
    comm = LibraryComm(0, 1, unique_id=LibraryComm.unique_id())
    src = H.normal_from_model(pm, nup, ndw)
    gen = torch.Generator(device="cuda").manual_seed(1234)
    v = torch.randn(src.dim, dtype=torch.float64, device="cuda", generator=gen)

    def median_ms(fn):
        ms = []
        for k in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms[args.warmup:]))

    out = {"script": "scripts/time_axisop.py --sharded", "kernel_source_hash": capi.kernel_source_hash(), "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds, "world": 1, "forced_collectives": True, "nph": nph,
           "source_sector": [nup, ndw], "doubles_src": src.dim, "cases": []}
    for spin, dest in ((0, (nup - 1, ndw)), (1, (nup, ndw - 1))):
        dst = H.normal_from_model(pm, *dest)
        one = torch.empty(dst.dim, dtype=torch.float64, device="cuda")
        sh = torch.empty(dst.dim, dtype=torch.float64, device="cuda")
        ops = [(1.0, False, 0, spin)]
        single = lambda: src.apply_cops_to(dst, v.data_ptr(), one.data_ptr(), [1.0], [False], [0], [spin])      # noqa: E731
        shard = lambda: comm.apply_cops(src, dst, v.data_ptr(), dst.dim, ops, out=sh.data_ptr())               # noqa: E731
        single(), shard()
        torch.cuda.synchronize()
        equal = bool(torch.equal(one.view(torch.int64), sh.view(torch.int64)))
        rounds = [{"single_call_ms": median_ms(single), "sharded_call_ms": median_ms(shard)} for _ in range(args.rounds)]
        med = {k: float(np.median([r[k] for r in rounds])) for k in rounds[0]}
        route, contributed = comm.apply_cops_info(src, dst, ops)
        out["cases"].append({"name": f"c {'down' if spin else 'up'} of orbital 0", "route": route, "allgather_doubles": contributed,
                             "doubles_dst": dst.dim, **med, "ratio": med["sharded_call_ms"] / med["single_call_ms"],
                             "bit_equal": equal, "per_round": rounds})
        dst.destroy()
    src.destroy()
    comm.destroy()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sharded", action="store_true", help="one-rank rehearsal of edigpu_apply_cops_sharded against edigpu_apply_cops_normal")
    args = ap.parse_args()
    if args.sharded:
        return sharded(args)
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian as H
    from edipack_amd.synthetic import WORKLOADS, synthetic_model
    if capi.device_count() < 1:
        raise SystemExit("time_axisop.py: no HIP device (there is nothing to time on a CPU)")
    capi.init(0)
    w = WORKLOADS["cfg2"]
    nup, ndw = w.sector
    nph = 4
    pm = synthetic_model(w)
    pmp = synthetic_model(w)
    pmp.nph, pmp.w0_ph, pmp.a_ph, pmp.g_ph = nph, 0.8, 0.0, np.diag(np.linspace(0.3, 0.5, w.norb))
    po = synthetic_model(dataclasses.replace(w, nbath=7))
    po.jx = po.jp = 0.0                                   # what ed_total_ud=F requires (impHloc is zero already)
    nups, ndws = (4, 4), (4, 3)

    cases = []   # (name, what it is compared with, source handle, destination handle, iorb, ispin)

    handles = {}

    def add(name, base, family, build, src_key, dst_key, iorb, ispin):
        for key in (src_key, dst_key):
            if (family, key) not in handles:
                handles[(family, key)] = build(*key)
        cases.append({"name": name, "base": base, "src": handles[(family, src_key)], "dst": handles[(family, dst_key)],
                      "iorb": iorb, "ispin": ispin})

    for label, model, build in (("cfg2 nph=0 (existing kernel)", pm, H.normal_from_model), (f"cfg2 nph={nph}", pmp, H.normal_from_model),
                                ("cfg2 complex", pm, H.normal_cmplx_from_model)):
        for spin, dest in ((0, (nup - 1, ndw)), (1, (nup, ndw - 1))):
            add(f"{label}, {'down' if spin else 'up'} operator", f"cfg2 nph=0 (existing kernel), {'down' if spin else 'up'} operator", label,
                lambda a, b, model=model, build=build: build(model, a, b), (nup, ndw), dest, 0, spin)
    for axis in range(4):
        occ = [list(nups), list(ndws)]
        occ[axis // 2][axis % 2] -= 1
        add(f"ed_total_ud=F (4 4 | 4 3), axis {axis}", None, "orbs", lambda u, d: H.orbs_from_model(po, u, d), (nups, ndws),
            (tuple(occ[0]), tuple(occ[1])), axis % 2, axis // 2)
    gen = torch.Generator(device="cuda").manual_seed(1234)
    for c in cases:
        wd = 2 if c["src"].is_complex else 1
        c["v"] = torch.randn(c["src"].dim * wd, dtype=torch.float64, device="cuda", generator=gen)
        c["out"] = torch.empty(c["dst"].dim * wd, dtype=torch.float64, device="cuda")
        c["doubles_dst"] = c["dst"].dim * wd
        c["rounds"] = []
    for _ in range(args.rounds):
        for c in cases:
            call_ms, kernel_ms = c["src"].time_apply_op(c["dst"], c["v"].data_ptr(), c["out"].data_ptr(), c["iorb"], c["ispin"],
                                                        False, args.warmup, args.steps)
            c["rounds"].append({"call_ms": call_ms, "kernel_ms": kernel_ms})
    out = {"script": "scripts/time_axisop.py", "kernel_source_hash": capi.kernel_source_hash(), "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds, "cases": []}
    med = {c["name"]: {k: float(np.median([r[k] for r in c["rounds"]])) for k in ("call_ms", "kernel_ms")} for c in cases}
    for c in cases:
        m = med[c["name"]]
        nel = c["doubles_dst"]
        # c on a level empties it: half the destination words have a preimage (exactly for the half-filled species)
        moved = 8.0 * nel * 1.5
        copy_gbs = capi.membw(int(max(moved, 1 << 26)))[1]
        rec = {"name": c["name"], "doubles_dst": nel, **m, "kernel_ns_per_double": m["kernel_ms"] * 1e6 / nel,
               "kernel_GBs": moved / (m["kernel_ms"] * 1e-3) / 1e9, "membw_copy_GBs": copy_gbs,
               "kernel_spread": [min(r["kernel_ms"] for r in c["rounds"]), max(r["kernel_ms"] for r in c["rounds"])],
               "per_round": c["rounds"]}
        if c["base"] and c["base"] != c["name"]:
            b = med[c["base"]]
            base_nel = next(x["doubles_dst"] for x in cases if x["name"] == c["base"])
            rec["existing_kernel_times_blocks_ms"] = b["kernel_ms"] * nel / base_nel
            rec["kernel_over_existing_per_double"] = (m["kernel_ms"] / nel) / (b["kernel_ms"] / base_nel)
        out["cases"].append(rec)
    for h in handles.values():
        h.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
