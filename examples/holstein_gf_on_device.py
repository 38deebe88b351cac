#!/usr/bin/env python3
"""Zero-temperature electron Green's function of a one-orbital Anderson-Holstein impurity, device-resident.

The electronic counterpart of examples/phonon_gf_on_device.py: what EDIpack does for ed_mode=normal with phonons between
`ed_solve` and `ed_get_gimp` (ED_NORMAL/ED_GF_NORMAL.f90:131-177, 363-427; apply_op_C / apply_op_CDG with their iph loop,
ED_SECTOR.f90:465-839), with the hot path on the GPU:

  1. the ground state of every (Nup, Ndw) phonon sector by thick-restart Lanczos (edigpu_lanczos_eigh_multi); the
     eigenvector of the lowest one stays in HBM
  2. c^+ / c in every phonon block, device to device (edigpu_apply_op_normal on phonon sectors: kernels_axisop.hip)
  3. the neighbouring sector is tridiagonalised from that seed (edigpu_lanczos_tridiag_dev)
  4. poles and weights from the small tridiagonal matrix give G(i w)

Only alpha, beta and the seed norm reach the host.

Run on a machine with an MI355X:   python examples/holstein_gf_on_device.py
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import ImpurityModel, SectorHamiltonian

    capi.init(0)
    nbath, nph = 5, 8
    rng = np.random.default_rng(1)
    model = ImpurityModel(ed_mode="normal", bath_type="normal", norb=1, nbath=nbath, nspin=1, hfmode=True, xmu=0.0,
                          uloc=np.array([2.0]), hloc=np.zeros((1, 1, 1, 1), complex),
                          be=rng.uniform(-2, 2, (1, 1, nbath)), bv=rng.uniform(0.2, 0.6, (1, 1, nbath)),
                          nph=nph, w0_ph=0.5, a_ph=0.0, g_ph=np.array([[0.4]]))
    ns = model.ns

    # 1. the lowest state of every sector; the eigenvector of the winner is computed again into device memory
    best = None
    for nup in range(ns + 1):
        for ndw in range(ns + 1):
            h = SectorHamiltonian.normal_from_model(model, nup, ndw)
            ev, _, _, _ = h.lanczos_eigh_multi(1, tol=1e-12, want_vectors=False)
            if best is None or ev[0] < best[0]:
                best = (float(ev[0]), (nup, ndw))
            h.destroy()
    e0, (nup, ndw) = best
    src = SectorHamiltonian.normal_from_model(model, nup, ndw)
    gs = torch.empty(src.dim, dtype=torch.float64, device="cuda")
    ev, nc, nmv = np.zeros(1), C.c_int(0), C.c_int(0)
    capi.check(capi.lib().edigpu_lanczos_eigh_multi(src._h, 1, 0, 1e-12, 300, None, capi.pd(ev), C.c_void_p(gs.data_ptr()),
                                                    C.byref(nc), C.byref(nmv)), "edigpu_lanczos_eigh_multi")
    print(f"ground state: E = {e0:.10f} in sector ({nup}, {ndw}), {nph + 1} phonon blocks of {src.dim // (nph + 1)} states")

    # 2.-4. G(i w_n) of the impurity, spin up, on the first Matsubara frequencies
    beta, nw = 50.0, 8
    z = 1j * np.pi / beta * (2 * np.arange(nw) + 1)
    g = np.zeros(nw, complex)
    for create, sign in ((True, 1), (False, -1)):
        n2 = nup + (1 if create else -1)
        if not 0 <= n2 <= ns:
            continue
        dst = SectorHamiltonian.normal_from_model(model, n2, ndw)
        seed = torch.empty(dst.dim, dtype=torch.float64, device="cuda")
        src.apply_op_to(dst, gs.data_ptr(), seed.data_ptr(), 0, 0, create)
        nl = min(dst.dim, 200)
        al, bl, nit, norm2 = dst.lanczos_tridiag_dev(seed.data_ptr(), nl)
        dst.destroy()
        if norm2 == 0.0:
            continue
        t = np.diag(al[:nit]) + np.diag(bl[1:nit], 1) + np.diag(bl[1:nit], -1)
        et, y = np.linalg.eigh(t)
        g += np.sum((norm2 * y[0] ** 2)[None, :] / (z[:, None] - sign * (et - e0)[None, :]), axis=1)
        print(f"  {'c^+' if create else 'c  '}|gs>: |seed|^2 = {norm2:.6f}, {nit} Lanczos steps")
    src.destroy()
    print("G(i w_0..2) =", np.array2string(g[:3], precision=6))


if __name__ == "__main__":
    main()
