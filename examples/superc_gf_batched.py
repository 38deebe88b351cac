#!/usr/bin/env python3
"""The Sz+1 half of the Nambu Green's function of a two-orbital superconducting impurity, every seed of the target
sector tridiagonalised in ONE call.

What EDIpack does in lanc_build_gf_superc_Gdiag / _Fmix (ED_SUPERC/ED_GF_SUPERC.f90:130-198, 287-361) for the channels
that lead from the ground state's sector Sz to Sz+1, with the hot path on the GPU:

  1. the ground state of every Sz sector by thick-restart Lanczos (edigpu_lanczos_eigh_multi); the vector stays in HBM
  2. the four seeds of every orbital a -- c^+_{a,up}, c_{a,dw}, c^+_{a,up} + c_{a,dw}, c^+_{a,up} + i c_{a,dw} applied to
     the ground state -- are written device-to-device into consecutive vectors of one buffer (edigpu_apply_cops_flat)
  3. one edigpu_lanczos_tridiag_batch_dev call tridiagonalises all 4 Norb seeds in lock-step: one sweep over H per step
     serves a whole group of seeds; only alpha, beta and the seed norms reach the host
  4. poles and weights of each small tridiagonal matrix give G_aa, barG_aa and the auxiliary functions of F_aa on i w_n

The same seeds are then run one by one through edigpu_lanczos_tridiag_dev for comparison.

Run on a machine with an MI355X:   python examples/superc_gf_batched.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import ImpurityModel, SectorHamiltonian

    capi.init(0)
    norb, nbath = 2, 6
    rng = np.random.default_rng(1)
    hloc = np.zeros((1, 1, norb, norb), complex)
    hloc[0, 0] = np.diag([0.25, -0.25])
    model = ImpurityModel(ed_mode="superc", bath_type="hybrid", norb=norb, nbath=nbath, nspin=1, hfmode=True, xmu=0.0,
                          uloc=np.array([2.0, 2.0]), ust=1.5, jh=0.25, jx=0.25, jp=0.25, hloc=hloc,
                          be=rng.uniform(-2, 2, (1, 1, nbath)), bv=rng.uniform(0.2, 0.6, (1, norb, nbath)),
                          bd=rng.uniform(-0.1, 0.1, (1, 1, nbath)))
    ns = model.ns

    # 1. ground state over the Sz sectors
    best = None
    for sz in range(-ns, ns + 1):
        h = SectorHamiltonian.flat_from_model(model, sz)
        ev, vec, _, _ = h.lanczos_eigh_multi(1, tol=1e-12)
        h.destroy()
        if best is None or ev[0] < best[0]:
            best = (ev[0], sz, vec[0].copy())
    e0, sz, gs = best
    print(f"ground state: E0 = {e0:.10f} in Sz = {sz}")

    # 2. every seed of Sz+1 into one buffer
    src = SectorHamiltonian.flat_from_model(model, sz)
    dst = SectorHamiltonian.flat_from_model(model, sz + 1)
    up, dw = 0, 1
    chans = []
    for a in range(norb):
        chans += [(f"c+_{a}up", [(1.0, True, a, up)]), (f"c_{a}dw", [(1.0, False, a, dw)]),
                  (f"c+_{a}up + c_{a}dw", [(1.0, True, a, up), (1.0, False, a, dw)]),
                  (f"c+_{a}up + i c_{a}dw", [(1.0, True, a, up), (1j, False, a, dw)])]
    vd = torch.from_numpy(gs).cuda()
    seeds = torch.zeros(len(chans), dst.dim, dtype=torch.complex128, device="cuda")
    for k, (_, ops) in enumerate(chans):
        src.apply_cops_flat_to(dst, vd.data_ptr(), seeds[k].data_ptr(), [o[0] for o in ops], [o[1] for o in ops],
                               [o[2] for o in ops], [o[3] for o in ops])
    torch.cuda.synchronize()

    # 3. one call for all of them, then one by one
    nl = min(dst.dim, 100)
    dst.lanczos_tridiag_batch_dev(seeds.data_ptr(), len(chans), nl)  # (first call: allocates the interleaved buffers)
    t0 = time.perf_counter()
    a, b, niter, norm2, route = dst.lanczos_tridiag_batch_dev(seeds.data_ptr(), len(chans), nl)
    t1 = time.perf_counter()
    one = [dst.lanczos_tridiag_dev(seeds[k].data_ptr(), nl) for k in range(len(chans))]
    t2 = time.perf_counter()
    print(f"target sector Sz = {sz + 1}: {dst.dim} rows, {len(chans)} seeds, {nl} steps; route {route}: "
          f"{(t1 - t0) * 1e3:.2f} ms in one call, {(t2 - t1) * 1e3:.2f} ms one by one")

    # 4. the pole sums on the first Matsubara frequencies
    beta, nw = 50.0, 8
    z = 1j * np.pi / beta * (2 * np.arange(nw) + 1)

    def pole_sum(al, bl, n2):
        t = np.diag(al) + np.diag(bl[1:], 1) + np.diag(bl[1:], -1)
        ev, y = np.linalg.eigh(t)
        return np.sum((n2 * y[0] ** 2)[None, :] / (z[:, None] - (ev - e0)[None, :]), axis=1)

    for k, (name, _) in enumerate(chans):
        if norm2[k] == 0.0:
            print(f"{name:>20s}: annihilates the ground state")
            continue
        g, g1 = pole_sum(a[k], b[k], norm2[k]), pole_sum(one[k][0], one[k][1], one[k][3])
        print(f"{name:>20s}: niter {niter[k]}, norm2 {norm2[k]:.6f}, G(i w_0) = {g[0]:.8f}, "
              f"max |batch - single| = {np.max(np.abs(g - g1)):.1e}")
    src.destroy()
    dst.destroy()


if __name__ == "__main__":
    main()
