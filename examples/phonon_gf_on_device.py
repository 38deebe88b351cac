#!/usr/bin/env python3
"""Phonon Green's function and phonon observables of a one-orbital Holstein impurity, device-resident.

What EDIpack does for a phonon run between `ed_solve` and `ed_get_dph` (lanc_build_gf_phonon_main,
ED_NORMAL/ED_GF_NORMAL.f90:278-345; the phonon lines of ED_NORMAL/ED_OBSERVABLES_NORMAL.f90:182-214), with the vectors in
HBM from start to end:

  1. every (Nup,Ndw) sector with its Nph + 1 phonon blocks is built on the device and its lowest state is found
     (edigpu_lanczos_eigh_multi); the eigenvector stays on the device
  2. the seed (b + b+)|gs> is made next to it (edigpu_apply_xph) and the SAME sector is tridiagonalised from it
     (edigpu_lanczos_tridiag_dev); only alpha / beta and the seed norm reach the host
  3. poles and weights of the small tridiagonal matrix give D(i nu_n) (edipack_amd.observables.phonon_gf)
  4. one reduction of the eigenvector (edigpu_ph_rdm) gives the phonon density matrix per impurity occupation class:
     prob_ph, dens_ph, <X>, <X^2> and the displacement distribution P(x) come off 3 * DimPh^2 numbers

Run on a machine with an MI355X:   python examples/phonon_gf_on_device.py
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
    from edipack_amd.observables import from_ph_rdm, phonon_gf, phonon_pdf

    capi.init(0)
    norb, nbath, nph = 1, 3, 8
    rng = np.random.default_rng(1)
    model = ImpurityModel(ed_mode="normal", bath_type="normal", norb=norb, nbath=nbath, nspin=1, hfmode=True, xmu=0.0,
                          uloc=np.array([1.0]), hloc=np.zeros((1, 1, 1, 1), complex),
                          be=rng.uniform(-1, 1, (1, norb, nbath)), bv=rng.uniform(0.2, 0.5, (1, norb, nbath)),
                          nph=nph, w0_ph=0.5, a_ph=0.0, g_ph=np.array([[0.4]]))
    ns = model.ns

    # 1. ground state: the lowest state of every sector, left on the device
    best = None
    for nup in range(ns + 1):
        for ndw in range(ns + 1):
            h = SectorHamiltonian.normal_from_model(model, nup, ndw)
            vec = torch.empty(h.dim, dtype=torch.float64, device="cuda")
            ev, nc, nmv = np.zeros(1), C.c_int(0), C.c_int(0)
            capi.check(capi.lib().edigpu_lanczos_eigh_multi(h._h, 1, 0, 1e-13, 300, None, capi.pd(ev),
                                                            C.c_void_p(vec.data_ptr()), C.byref(nc), C.byref(nmv)),
                       "edigpu_lanczos_eigh_multi")
            if best is None or ev[0] < best[0]:
                if best is not None:
                    best[2].destroy()
                best = (float(ev[0]), (nup, ndw), h, vec)
            else:
                h.destroy()
    e0, sec, h, vec = best
    print(f"ground-state energy {e0:.10f} in sector {sec}, dim {h.dim} = {h.dim // (nph + 1)} x {nph + 1} phonon blocks")

    # 2. seed and tridiagonalisation of the same sector
    seed = torch.empty_like(vec)
    h.apply_xph(vec.data_ptr(), seed.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    alanc, blanc, nit, norm2 = h.lanczos_tridiag_dev(seed.data_ptr(), min(100, h.dim))

    # 3. D(i nu_n) on the first bosonic Matsubara frequencies
    beta = 50.0
    nu = 2.0 * np.pi * np.arange(8) / beta
    D = phonon_gf(alanc[:nit], blanc[:nit], norm2, e0, 1j * nu, beta=beta)
    for n, d in zip(nu, D):
        print(f"  nu = {n:8.5f}   D = {d.real:+.10f}")

    # 4. phonon observables from one reduction
    rho, n2 = h.ph_rdm(vec.data_ptr())
    o = from_ph_rdm(rho[0], norm2=n2[0])
    print(f"prob_ph = {np.array2string(o.prob_ph, precision=6)}")
    print(f"dens_ph = {o.dens_ph:.8f}   <X> = {o.x_ph:+.8f}   <X^2> = {o.x2_ph:.8f}")
    print(f"weight of the impurity occupations 0, 1, 2: {np.array2string(o.prob_class, precision=6)}")
    x, pdf, part = phonon_pdf(rho[0], -5.0, 5.0, 11, norm2=n2[0])
    for xi, p, pp in zip(x, pdf, part):
        print(f"  x = {xi:+.3f}   P(x) = {p:.6f}   by occupation {np.array2string(pp, precision=6)}")
    # <seed|seed> = <(b + b+)^2> in the truncated space: 2 <X^2> minus the cut step above the top level
    print(f"<seed|seed> = {norm2:.10f}   2 <X^2> - (Nph + 1) prob_ph[Nph] = {2 * o.x2_ph - (nph + 1) * o.prob_ph[nph]:.10f}")
    h.destroy()


if __name__ == "__main__":
    main()
