#!/usr/bin/env python
"""Times the fused two-operator seeds (edigpu_apply_pairs_normal) against the chain they replace and prints ONE JSON line
(profiles/pairs.json).

On the config-2 sector of bench.py (synthetic.WORKLOADS["cfg2"]: Ns = 14, (7, 7), 3432^2 = 11.8 M elements, 94 MB per
vector), for a 1-term seed (pair, lesser, diagonal: c_{0,up} c_{0,dw}|v>) and a 2-term seed (pair, lesser, mixed: the same
of orbitals 0 and 1 added), both into the sector (6, 6):

  (a) edigpu_time_pairs: the median of the whole call as a caller pays it (host tables, upload, kernel, wait, free)
      between two HIP events, and the median of the kernel alone;
  (b) the yardstick, made only of entry points that existed before the fused pass: edigpu_apply_op_normal through the
      built intermediate sector (7, 6) -- one pair of calls per term -- and, for the second term, a torch add of the two
      results, between two torch events on the stream the calls are given.

(a) and (b) alternate over `--rounds` rounds in this one process; per round the medians over `--steps` runs after
`--warmup`, and over the rounds the median of those.  The two results are compared on the same input before timing
(bit patterns after adding +0.0: the chain writes -0.0 where a sign meets an empty intermediate element).

    python scripts/time_pairs.py [--steps 21] [--warmup 3] [--rounds 3]

--sharded times edigpu_apply_pairs_sharded instead (profiles/pairs.json, key sharded_rehearsal): a world of ONE rank on the
RCCL communicator with the collectives forced (EDIGPU_FORCE_COLLECTIVES=1), the 1-term pair seed on the config-2 sector
with nph = 4, device vectors, against edigpu_apply_pairs_normal on the same vectors; both calls return after the device has
finished and are timed on the host clock.  A rehearsal of the call's fixed costs on one GPU, not a scaling figure.
"""
import argparse
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
    from edipack_amd.hamiltonian import SectorHamiltonian, pairs_sector
    from edipack_amd.observables import pair_chi_seeds
    from edipack_amd.sharding import LibraryComm
    from edipack_amd.synthetic import WORKLOADS, synthetic_model
    if capi.device_count() < 1:
        raise SystemExit("time_pairs.py: no HIP device (there is nothing to time on a CPU)")
    capi.init(0)
    w = WORKLOADS[args.workload]
    nph = 4
    pm = synthetic_model(w)
    pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = nph, 0.8, 0.0, np.diag(np.linspace(0.3, 0.5, w.norb))
    nup, ndw = w.sector
    terms = pair_chi_seeds(0, 0)[0][0]
    dest = pairs_sector(pm, nup, ndw, terms)
    comm = LibraryComm(0, 1, unique_id=LibraryComm.unique_id())
    src = SectorHamiltonian.normal_from_model(pm, nup, ndw)
    dst = SectorHamiltonian.normal_from_model(pm, dest[0], dest[1])
    gen = torch.Generator(device="cuda").manual_seed(1234)
    v = torch.randn(src.dim, dtype=torch.float64, device="cuda", generator=gen)
    one = torch.empty(dst.dim, dtype=torch.float64, device="cuda")
    sh = torch.empty(dst.dim, dtype=torch.float64, device="cuda")

    def median_ms(fn):
        ms = []
        for k in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms[args.warmup:]))

    single = lambda: src.apply_pairs_to(dst, v.data_ptr(), one.data_ptr(), terms)                               # noqa: E731
    shard = lambda: comm.apply_pairs(src, dst, v.data_ptr(), dst.dim, terms, out=sh.data_ptr())                # noqa: E731
    single(), shard()
    torch.cuda.synchronize()
    equal = bool(torch.equal(one.view(torch.int64), sh.view(torch.int64)))
    rounds = [{"single_call_ms": median_ms(single), "sharded_call_ms": median_ms(shard)} for _ in range(args.rounds)]
    med = {k: float(np.median([r[k] for r in rounds])) for k in rounds[0]}
    route, contributed = comm.apply_pairs_info(src, dst, terms)
    print(json.dumps({"script": "scripts/time_pairs.py --sharded", "kernel_source_hash": capi.kernel_source_hash(),
                      "workload": w.name, "nph": nph, "world": 1, "forced_collectives": True, "steps": args.steps,
                      "warmup": args.warmup, "rounds": args.rounds, "source_sector": [nup, ndw], "destination_sector": list(dest[:2]),
                      "doubles_src": src.dim, "doubles_dst": dst.dim, "seed": "pair lesser diag (1 term)", "route": route,
                      "allgather_doubles": contributed, **med, "ratio": med["sharded_call_ms"] / med["single_call_ms"],
                      "bit_equal": equal, "per_round": rounds}))
    src.destroy(), dst.destroy()
    comm.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2")
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sharded", action="store_true", help="one-rank rehearsal of edigpu_apply_pairs_sharded against edigpu_apply_pairs_normal")
    args = ap.parse_args()
    if args.sharded:
        return sharded(args)
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian, pairs_sector
    from edipack_amd.observables import pair_chi_seeds
    from edipack_amd.synthetic import WORKLOADS, synthetic_model
    if capi.device_count() < 1:
        raise SystemExit("time_pairs.py: no HIP device (there is nothing to time on a CPU)")
    capi.init(0)
    w = WORKLOADS[args.workload]
    pm = synthetic_model(w)
    nup, ndw = w.sector
    seeds = [("pair lesser diag (1 term)", pair_chi_seeds(0, 0)[0][0]), ("pair lesser mix (2 terms)", pair_chi_seeds(0, 1)[0][0])]
    dest = pairs_sector(pm, nup, ndw, seeds[0][1])
    assert dest[2] and pairs_sector(pm, nup, ndw, seeds[1][1]) == dest
    h_src = SectorHamiltonian.normal_from_model(pm, nup, ndw)
    h_mid = SectorHamiltonian.normal_from_model(pm, nup, ndw - 1)          # after c_{a,dw}
    h_dst = SectorHamiltonian.normal_from_model(pm, dest[0], dest[1])
    gen = torch.Generator(device="cuda").manual_seed(1234)
    v = torch.randn(h_src.dim, dtype=torch.float64, device="cuda", generator=gen)
    tmp = torch.empty(h_mid.dim, dtype=torch.float64, device="cuda")
    fused = torch.empty(h_dst.dim, dtype=torch.float64, device="cuda")
    va, vb = torch.empty_like(fused), torch.empty_like(fused)
    st = torch.cuda.current_stream().cuda_stream

    def chain(terms):
        """the seed the old way; the result is va"""
        for k, (coef, o1, o2) in enumerate(terms):
            out = va if k == 0 else vb
            h_src.apply_op_to(h_mid, v.data_ptr(), tmp.data_ptr(), o1[1], o1[2], bool(o1[0]), st)
            h_mid.apply_op_to(h_dst, tmp.data_ptr(), out.data_ptr(), o2[1], o2[2], bool(o2[0]), st)
            if k > 0:
                va.add_(vb, alpha=coef)
        return va

    def time_chain(terms):
        ms = []
        for k in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            chain(terms)
            e1.record()
            e1.synchronize()
            if k >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    out = {"script": "scripts/time_pairs.py", "kernel_source_hash": capi.kernel_source_hash(), "workload": w.name,
           "source_sector": [nup, ndw], "intermediate_sector": [nup, ndw - 1], "destination_sector": list(dest[:2]),
           "dim_src": h_src.dim, "dim_dst": h_dst.dim, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "seeds": []}
    for name, terms in seeds:
        assert all(t[0] == 1.0 for t in terms)
        h_src.apply_pairs_to(h_dst, v.data_ptr(), fused.data_ptr(), terms, st)
        ref = chain(terms)
        torch.cuda.synchronize()
        equal = bool(torch.equal((fused + 0.0).view(torch.int64), (ref + 0.0).view(torch.int64)))
        rounds = []
        for _ in range(args.rounds):
            call_ms, kernel_ms = h_src.time_pairs(h_dst, v.data_ptr(), fused.data_ptr(), terms, args.warmup, args.steps)
            rounds.append({"fused_call_ms": call_ms, "fused_kernel_ms": kernel_ms, "chain_ms": time_chain(terms)})
        med = {k: float(np.median([r[k] for r in rounds])) for k in rounds[0]}
        written = 8.0 * h_dst.dim                     # every destination element is stored once; the reads depend on the term
        out["seeds"].append({"name": name, "nterms": len(terms), **med, "fused_call_over_chain": med["fused_call_ms"] / med["chain_ms"],
                             "fused_kernel_store_GBs": written / (med["fused_kernel_ms"] * 1e-3) / 1e9,
                             "bit_equal_mod_zero_sign": equal, "per_round": rounds})
    for h in (h_src, h_mid, h_dst):
        h.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
