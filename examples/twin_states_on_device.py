#!/usr/bin/env python3
"""ED_TWIN=T without a host copy: the state of a twin sector made on the device from the state of the stored sector.

With ed_twin=T EDIpack diagonalises only one sector of each pair (Nup, Ndw) / (Ndw, Nup) and keeps the partner as a
vector-less twin state; es_return_dvector (ED_EIGENSPACE.f90:652-720) makes its vector on demand by the reorder
vector(i) = twin%dvec(Order(i)).  Here, for a spin-symmetric two-orbital model:

  1. the lowest state of (Nup, Ndw) = (4, 3) is found on the device and stays there (edigpu_lanczos_eigh_multi)
  2. its twin, the lowest state of (3, 4), is made by SectorHamiltonian.twin_to (edigpu_apply_twin): a transpose of the
     DimDw x DimUp array, no solve of (3, 4) and no download
  3. c^+_{a,up} on the source (-> sector (5, 3)) and c^+_{a,dw} on the twin (-> sector (3, 5)) seed two
     tridiagonalisations (edigpu_apply_op_normal, edigpu_lanczos_tridiag_dev)
  4. the particle part of G_dw from the twin equals that of G_up from the source, as the spin symmetry demands

Run on a machine with an MI355X:   python examples/twin_states_on_device.py
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import ImpurityModel, SectorHamiltonian, twin_sector

    capi.init(0)
    norb, nbath = 2, 3
    rng = np.random.default_rng(1)
    hloc = np.zeros((1, 1, norb, norb), complex)
    hloc[0, 0] = np.diag([0.25, -0.25])
    model = ImpurityModel(ed_mode="normal", bath_type="normal", norb=norb, nbath=nbath, nspin=1, hfmode=True, xmu=0.0,
                          uloc=np.array([2.0, 2.0]), ust=1.5, jh=0.25, jx=0.25, jp=0.25, hloc=hloc,
                          be=rng.uniform(-2, 2, (1, norb, nbath)), bv=rng.uniform(0.2, 0.6, (1, norb, nbath)))
    nup, ndw = 4, 3
    tup, tdw, self_twin = twin_sector(model, 0, nup, ndw)
    print(f"sector ({nup}, {ndw}); its twin ({tup}, {tdw}); self-twin: {self_twin}")

    # 1. the lowest state of the stored sector, on the device
    src = SectorHamiltonian.normal_from_model(model, nup, ndw)
    v_a = torch.empty(src.dim, dtype=torch.float64, device="cuda")
    e, nconv, nmv = np.zeros(1), C.c_int(0), C.c_int(0)
    capi.check(capi.lib().edigpu_lanczos_eigh_multi(src._h, 1, 0, 1e-13, 300, None, capi.pd(e), C.c_void_p(v_a.data_ptr()),
                                                    C.byref(nconv), C.byref(nmv)), "edigpu_lanczos_eigh_multi")
    print(f"E0({nup}, {ndw}) = {e[0]:.10f} ({nmv.value} products)")

    # 2. the twin state, on the device
    twin = SectorHamiltonian.normal_from_model(model, tup, tdw)
    v_b = torch.empty(twin.dim, dtype=torch.float64, device="cuda")
    src.twin_to(twin, v_a.data_ptr(), v_b.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    hv = torch.empty_like(v_b)
    twin.apply_dev(v_b.data_ptr(), hv.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    print(f"|H_twin v_twin - E0 v_twin| = {torch.linalg.norm(hv - e[0] * v_b).item():.2e}")

    # 3., 4. the particle part of G_up from the source and of G_dw from the twin
    beta, nw = 50.0, 8
    z = 1j * np.pi / beta * (2 * np.arange(nw) + 1)
    for a in range(norb):
        g = {}
        for name, h, vec, spin, dest in (("up, from the source", src, v_a, 0, (nup + 1, ndw)),
                                         ("dw, from the twin", twin, v_b, 1, (tup, tdw + 1))):
            dst = SectorHamiltonian.normal_from_model(model, *dest)
            seed = torch.empty(dst.dim, dtype=torch.float64, device="cuda")
            h.apply_op_to(dst, vec.data_ptr(), seed.data_ptr(), a, spin, True)
            nl = min(dst.dim, 200)
            al, bl, _, norm2 = dst.lanczos_tridiag_dev(seed.data_ptr(), nl)
            dst.destroy()
            t = np.diag(al[:nl]) + np.diag(bl[1:nl], 1) + np.diag(bl[1:nl], -1)
            ev, y = np.linalg.eigh(t)
            g[name] = np.sum((norm2 * y[0] ** 2)[None, :] / (z[:, None] - (ev - e[0])[None, :]), axis=1)
            print(f"orbital {a}, G_{name}: norm2 = {norm2:.12f}, G(i w_0) = {g[name][0]:.10f}")
        up, dw = g["up, from the source"], g["dw, from the twin"]
        print(f"orbital {a}: max |G_dw(twin) - G_up(source)| = {np.max(np.abs(dw - up)):.2e}")
    src.destroy(), twin.destroy()


if __name__ == "__main__":
    main()
