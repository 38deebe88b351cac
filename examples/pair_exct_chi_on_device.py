#!/usr/bin/env python3
"""Pair and exciton susceptibilities of a two-orbital impurity, device-resident.

What EDIpack does between `ed_solve` and `ed_get_pairchi` / `ed_get_exctchi` (lanc_ed_build_pairChi_diag,
ED_NORMAL/ED_CHI_PAIR.f90:98-161; lanc_ed_build_exctChi_tripletXY, ED_NORMAL/ED_CHI_EXCT.f90:151-241), with the vectors in
HBM from start to end and no intermediate sector:

  1. every (Nup,Ndw) sector is built on the device and its lowest state is found (edigpu_lanczos_eigh_multi); the
     eigenvector stays on the device
  2. per channel, the seed O2 O1|gs> is made in ONE pass straight into the target sector (edigpu_apply_pairs_normal):
     c_up c_dw|gs> and c+_dw c+_up|gs> for the pair channel, c+_{a,dw} c_{b,up}|gs> and its three siblings for the
     triplet-XY exciton
  3. the target sector is tridiagonalised from the seed (edigpu_lanczos_tridiag_dev); only alpha / beta and the seed norm
     reach the host
  4. poles and weights of the small tridiagonal matrix give the channel's share of chi(i nu_n)
     (edipack_amd.observables.chi_channel)

Run on a machine with an MI355X:   python examples/pair_exct_chi_on_device.py
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import ImpurityModel, SectorHamiltonian, pairs_sector
    from edipack_amd.observables import chi_channel, exct_chi_seeds, pair_chi_seeds

    capi.init(0)
    norb, nbath = 2, 2
    rng = np.random.default_rng(3)
    hloc = np.zeros((1, 1, norb, norb), complex)
    hloc[0, 0] = np.array([[0.2, 0.15], [0.15, -0.2]])
    model = ImpurityModel(ed_mode="normal", bath_type="normal", norb=norb, nbath=nbath, nspin=1, hfmode=True, xmu=0.0,
                          uloc=np.array([2.0, 2.0]), ust=1.5, jh=0.25, jx=0.25, jp=0.25, hloc=hloc,
                          be=rng.uniform(-1.5, 1.5, (1, norb, nbath)), bv=rng.uniform(0.2, 0.5, (1, norb, nbath)))
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
    print(f"ground-state energy {e0:.10f} in sector {sec}, dim {h.dim}")

    beta = 50.0
    nu = 2.0 * np.pi * np.arange(8) / beta

    def chi_of(channels):
        """sum over the channels of one susceptibility: seed -> tridiagonalisation -> poles and weights"""
        chi = np.zeros(nu.size, complex)
        for ichan, (terms, isign) in enumerate(channels, start=1):
            nu_t, nd_t, exists = pairs_sector(model, *sec, terms)
            if not exists:                      # getCsector / getCDGsector = 0: the reference skips the channel
                continue
            target = h if (nu_t, nd_t) == sec else SectorHamiltonian.normal_from_model(model, nu_t, nd_t)
            seed = torch.empty(target.dim, dtype=torch.float64, device="cuda")
            h.apply_pairs_to(target, vec.data_ptr(), seed.data_ptr(), terms, torch.cuda.current_stream().cuda_stream)
            alanc, blanc, nit, norm2 = target.lanczos_tridiag_dev(seed.data_ptr(), min(100, target.dim))
            if norm2 > 0.0:
                chi += chi_channel(alanc[:nit], blanc[:nit], norm2, e0, isign, ichan, 1j * nu, beta)
            print(f"    channel {ichan}: target sector ({nu_t}, {nd_t}), dim {target.dim}, <seed|seed> = {norm2:.10f}, "
                  f"{nit} Lanczos steps")
            if target is not h:
                target.destroy()
        return chi

    # 2.-4. one pair channel pair and the triplet-XY exciton
    print("chi_pair(1,1): seeds c_up c_dw|gs>, c+_dw c+_up|gs> of orbital 1")
    chi_pair = chi_of(pair_chi_seeds(0, 0))
    for n, c in zip(nu, chi_pair):
        print(f"  nu = {n:8.5f}   chi_pair = {c.real:+.10f}")
    print("chi_exct triplet-XY (1,2): seeds c+_{1,dw} c_{2,up}|gs> and its three siblings")
    chi_xy = chi_of(exct_chi_seeds(2, 0, 1))
    for n, c in zip(nu, chi_xy):
        print(f"  nu = {n:8.5f}   chi_exct_XY = {c.real:+.10f}")
    h.destroy()


if __name__ == "__main__":
    main()
