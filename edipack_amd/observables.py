"""Ground-state observables from occupation moments.

``SectorHamiltonian.occ_moments`` (edigpu_occ_moments) reduces a device vector to

    M[x, y] = sum_i |v_i|^2 n_x(i) n_y(i),   x = a for (a, up), norb + a for (a, down),

and everything the observables loop of the reference (ED_NORMAL/ED_OBSERVABLES_NORMAL.f90:120-185 and its superc /
nonsu2 sisters) accumulates from the occupations of a state is a linear combination of those numbers: with
U = M[:n, :n] (up-up), D = M[n:, n:] (down-down), X = M[:n, n:] (up-down)

    dens    = diag U + diag D            dens_up = diag U,  dens_dw = diag D
    docc    = diag X                     magz    = diag U - diag D
    sz2     = (U + D - X - X^T) / 4      n2      = U + D + X + X^T
    s2tot   = sum sz2                    (imp.check[0])
    dust    = sum_{a<b} X_ab + X_ba      dund    = sum_{a<b} U_ab + D_ab      (doubles.check[0:2])

``SectorHamiltonian.imp_rdm`` (edigpu_imp_rdm) gives the other family, the impurity reduced density matrix
rho = Tr_bath |v><v| in the ordering io = Iup + 2^norb Idw (imp_rdm_normal, ED_NORMAL/ED_RDM_NORMAL.f90): rdm_average
normalises and averages it as that routine's loop over the states does, rdm_occupations reads its diagonal,
entanglement_entropy its spectrum.  ``SectorHamiltonian.imp_rdm_flat`` (edigpu_imp_rdm_flat) is the same of superc /
nonsu2 vectors (imp_rdm_superc, imp_rdm_nonsu2) in the basis |Iup Idw>; its blocks couple different (N_up, N_dw), and
rdm_anomalous / rdm_magx read the anomalous amplitudes and the transverse magnetisation off it.

``SectorHamiltonian.ph_rdm`` (edigpu_ph_rdm) gives the phonon side: rho[c, n, m] = sum over the electronic states of
impurity occupation class c of v(i_el, n) conj v(i_el, m).  from_ph_rdm reads prob_ph, dens_ph, X_ph, X2_ph off it
(ED_OBSERVABLES_NORMAL.f90:184-199), phonon_pdf the displacement distribution of prob_distr_ph (:1235-1298), and
phonon_gf turns the tridiagonalisation seeded with ``apply_xph`` into D(z) (ED_GF_NORMAL.f90:434-483, 616-690).

``SectorHamiltonian.apply_pairs_to`` (edigpu_apply_pairs_normal) makes the seeds of the pair and exciton susceptibilities
in one pass; pair_chi_seeds / exct_chi_seeds write their operator products as the reference's loops do
(ED_NORMAL/ED_CHI_PAIR.f90, ED_CHI_EXCT.f90) and chi_channel turns a seed's tridiagonalisation into its channel's share of
chi(z).

Pure numpy: O(norb^2) numbers per vector (16^norb for the density matrix, 3^norb DimPh^2 for the phonon one) reach the
host."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class OccObservables:
    dens: np.ndarray
    dens_up: np.ndarray
    dens_dw: np.ndarray
    docc: np.ndarray
    magz: np.ndarray
    sz2: np.ndarray
    n2: np.ndarray
    s2tot: float
    dust: float
    dund: float


def from_moments(M, norb: int, norm2=None) -> OccObservables:
    """Observables of one state, M[2 norb, 2 norb], or the average over a manifold of states, M[k, 2 norb, 2 norb].
    norm2 (a scalar, or k of them): <v|v> of each vector as occ_moments returns it; None = the moments are already those
    of normalised vectors."""
    M = np.asarray(M, dtype=np.float64)
    n = int(norb)
    if M.shape[-2:] != (2 * n, 2 * n) or M.ndim not in (2, 3):
        raise ValueError(f"from_moments: expected [..., {2 * n}, {2 * n}] moments, got {M.shape}")
    if norm2 is not None:
        M = M / np.asarray(norm2, dtype=np.float64).reshape(M.shape[:-2] + (1, 1))
    if M.ndim == 3:
        M = M.mean(axis=0)
    U, D, X = M[:n, :n], M[n:, n:], M[:n, n:]
    up, dw = np.diag(U).copy(), np.diag(D).copy()
    sz2 = 0.25 * (U + D - X - X.T)
    n2 = U + D + X + X.T
    off = np.triu(np.ones((n, n), dtype=bool), 1)
    return OccObservables(dens=up + dw, dens_up=up, dens_dw=dw, docc=np.diag(X).copy(), magz=up - dw, sz2=sz2, n2=n2,
                          s2tot=float(sz2.sum()), dust=float((X + X.T)[off].sum()), dund=float((U + D)[off].sum()))


def rdm_average(rhos, norm2, weights=None) -> np.ndarray:
    """rho of a manifold: rhos[k, D, D] as imp_rdm returns them, each divided by norm2[k], then averaged -- equal weights
    (the degenerate ground states of imp_rdm_normal at zero temperature) or `weights` (Boltzmann weights; they are
    normalised to sum 1)."""
    rhos = np.asarray(rhos)
    if rhos.ndim == 2:
        rhos = rhos[None]
    n2 = np.atleast_1d(np.asarray(norm2, dtype=np.float64))
    if rhos.ndim != 3 or rhos.shape[1] != rhos.shape[2] or n2.shape != (rhos.shape[0],):
        raise ValueError(f"rdm_average: expected rhos[k, D, D] and k norms, got {rhos.shape} and {n2.shape}")
    w = np.full(n2.size, 1.0 / n2.size) if weights is None else np.asarray(weights, dtype=np.float64) / np.sum(weights)
    if w.shape != n2.shape:
        raise ValueError("rdm_average: one weight per state")
    return np.tensordot(w / n2, rhos, axes=(0, 0))


def rdm_occupations(rho, norb: int):
    """(dens_up, dens_dw, docc) per orbital from the diagonal of rho[D, D], D = 4^norb, io = Iup + 2^norb Idw."""
    n = int(norb)
    rho = np.asarray(rho)
    if rho.shape != (4 ** n, 4 ** n):
        raise ValueError(f"rdm_occupations: expected [{4 ** n}, {4 ** n}], got {rho.shape}")
    p = np.real(np.diag(rho))
    io = np.arange(4 ** n)
    up = np.array([(io >> a) & 1 for a in range(n)], dtype=np.float64)
    dw = np.array([(io >> (n + a)) & 1 for a in range(n)], dtype=np.float64)
    return up @ p, dw @ p, (up * dw) @ p


def _impurity_annihilators(norb: int):
    """c_l of the 2 norb impurity levels (up 0 .. norb-1, then down 0 .. norb-1) in the 4^norb occupation space, bit l of
    the state index = level l, with the Jordan-Wigner sign (-1)^(occupied levels below l)."""
    n = int(norb)
    D = 4 ** n
    io = np.arange(D)
    ops = []
    for l in range(2 * n):
        sel = io[(io >> l) & 1 == 1]
        below = np.zeros(sel.size, dtype=np.int64)
        for m in range(l):
            below += (sel >> m) & 1
        c = np.zeros((D, D))
        c[sel ^ (1 << l), sel] = 1.0 - 2.0 * (below & 1)
        ops.append(c)
    return ops


def _rdm_checked(rho, norb: int, who: str):
    n = int(norb)
    rho = np.asarray(rho)
    if rho.shape != (4 ** n, 4 ** n):
        raise ValueError(f"{who}: expected [{4 ** n}, {4 ** n}], got {rho.shape}")
    return n, rho


def rdm_anomalous(rho, norb: int) -> np.ndarray:
    """phi[a, b] = <c_{b,up} c_{a,dw}> = tr(rho c_{b,up} c_{a,dw}) of the (normalised) rho[D, D] of imp_rdm_flat; complex.
    The real part is phisc of the superc observables (ED_OBSERVABLES_SUPERC.f90)."""
    n, rho = _rdm_checked(rho, norb, "rdm_anomalous")
    c = _impurity_annihilators(n)
    return np.array([[np.trace(rho @ (c[b] @ c[n + a])) for b in range(n)] for a in range(n)], dtype=np.complex128)


def rdm_magx(rho, norb: int) -> np.ndarray:
    """magX[a] = 2 Re <c+_{a,up} c_{a,dw}> = 2 Re tr(rho c+_{a,up} c_{a,dw}) of the (normalised) rho[D, D] of imp_rdm_flat
    (ED_OBSERVABLES_NONSU2.f90)."""
    n, rho = _rdm_checked(rho, norb, "rdm_magx")
    c = _impurity_annihilators(n)
    return np.array([2.0 * np.real(np.trace(rho @ (c[a].T @ c[n + a]))) for a in range(n)])


def entanglement_entropy(rho) -> float:
    """-sum p ln p over the eigenvalues p > 1e-300 of the (normalised, Hermitian) rho."""
    p = np.linalg.eigvalsh(np.asarray(rho))
    p = p[p > 1e-300]
    return float(-np.sum(p * np.log(p)))


@dataclass
class PhononObservables:
    prob_ph: np.ndarray     # [DimPh] probability of n phonons
    dens_ph: float          # <b+ b>
    x_ph: float             # <X>, X = (b + b+) / sqrt(2)
    x2_ph: float            # <X^2>
    prob_class: np.ndarray  # [3^norb] weight of the impurity occupation class c = sum_a nt_a 3^a


def _ph_rdm_average(rho, norm2, who: str) -> np.ndarray:
    """rho[C, D, D] of one state or the average of rho[k, C, D, D] over a manifold, each divided by its norm2 (None: the
    vectors were normalised), as from_moments forms it"""
    rho = np.asarray(rho)
    if rho.ndim not in (3, 4) or rho.shape[-1] != rho.shape[-2]:
        raise ValueError(f"{who}: expected rho[..., classes, DimPh, DimPh], got {rho.shape}")
    if norm2 is not None:
        rho = rho / np.asarray(norm2, dtype=np.float64).reshape(rho.shape[:-3] + (1, 1, 1))
    return rho.mean(axis=0) if rho.ndim == 4 else rho


def from_ph_rdm(rho, norm2=None) -> PhononObservables:
    """prob_ph, dens_ph, X_ph, X2_ph of ED_OBSERVABLES_NORMAL.f90:184-199 from the phonon density matrix of ph_rdm,
    rho[C, D, D] or a manifold rho[k, C, D, D] with norm2 as ph_rdm returns it.  On R = sum_c rho[c]:
    prob_ph[n] = R_nn, dens_ph = sum n R_nn, X_ph = sqrt(2) sum_n sqrt(n+1) Re R[n, n+1],
    X2_ph = 1/2 sum (2n+1) R_nn + sum_n sqrt((n+1)(n+2)) Re R[n, n+2]   (v conj v throughout)."""
    rho = _ph_rdm_average(rho, norm2, "from_ph_rdm")
    R = rho.sum(axis=0)
    d = R.shape[0]
    n = np.arange(d, dtype=np.float64)
    p = np.real(np.diag(R)).copy()
    x = np.sqrt(2.0) * float(np.sum(np.sqrt(n[:-1] + 1.0) * np.real(np.diag(R, 1))))
    x2 = 0.5 * float(np.sum((2.0 * n + 1.0) * p))
    if d > 2:
        x2 += float(np.sum(np.sqrt((n[:-2] + 1.0) * (n[:-2] + 2.0)) * np.real(np.diag(R, 2))))
    return PhononObservables(prob_ph=p, dens_ph=float(np.sum(n * p)), x_ph=x, x2_ph=x2,
                             prob_class=np.real(np.trace(rho, axis1=1, axis2=2)).copy())


def hermite_functions(x, dimph: int) -> np.ndarray:
    """psi[i, n], n = 0 .. dimph - 1: the harmonic-oscillator eigenfunctions at the positions x[i], by the recurrence and
    with the constant of Hermite (ED_OBSERVABLES_NORMAL.f90:1282-1298)."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    den = 1.331335373062335   # pi^(1/4)
    psi = np.zeros((x.size, int(dimph)))
    psi[:, 0] = np.exp(-0.5 * x * x) / den
    if dimph > 1:
        psi[:, 1] = np.exp(-0.5 * x * x) * np.sqrt(2.0) * x / den
    for i in range(2, int(dimph)):
        psi[:, i] = 2 * x * psi[:, i - 1] / np.sqrt(float(2 * i)) - psi[:, i - 2] * np.sqrt(float(i - 1) / float(i))
    return psi


def phonon_pdf(rho, xmin: float, xmax: float, lpos: int, norm2=None):
    """(x[lpos], pdf_ph[lpos], pdf_part[lpos, 3^norb]) of prob_distr_ph (ED_OBSERVABLES_NORMAL.f90:1235-1280) on its grid
    x_i = xmin + i (xmax - xmin) / lpos: pdf_part[i, c] = sum_nm psi_n(x_i) psi_m(x_i) rho[c, n, m], pdf_ph = sum_c."""
    rho = _ph_rdm_average(rho, norm2, "phonon_pdf")
    x = xmin + np.arange(int(lpos)) * ((xmax - xmin) / float(lpos))
    psi = hermite_functions(x, rho.shape[-1])
    part = np.real(np.einsum("in,cnm,im->ic", psi, rho, psi))
    return x, part.sum(axis=1), part


def phonon_gf(alanc, blanc, norm2: float, e_state: float, z, zeta: float = 1.0, beta: float | None = None) -> np.ndarray:
    """D(z) of one state from the tridiagonalisation seeded with (b + b+)|state> (apply_xph, lanczos_tridiag_dev).
    add_to_lanczos_phonon (ED_GF_NORMAL.f90:434-483): poles dE_j = E_j - e_state, weights norm2 Z(1,j)^2 / zeta of the
    tridiagonal matrix's eigenpairs.  get_impD_normal (ED_GF_NORMAL.f90:616-690) sums them in the bosonic form: only the
    poles dE > 0 count, each with its mirror image,
        D(z) = sum_j w_j (1 - exp(-beta dE_j)) (1 / (z - dE_j) - 1 / (z + dE_j)),
    which on the Matsubara axis is the reference's -w (1 - exp(-beta dE)) 2 dE / (nu^2 + dE^2) (:676-677); a pole with
    |beta dE| < 1e-8 adds -w beta at z = 0 only (:655-661).  beta = None is zero temperature: the factor is 1 and a
    zero-energy pole adds nothing."""
    a = np.asarray(alanc, dtype=np.float64)
    b = np.asarray(blanc, dtype=np.float64)
    t = np.diag(a) + np.diag(b[1:], 1) + np.diag(b[1:], -1)
    e, zv = np.linalg.eigh(t)
    w = float(norm2) * zv[0, :] ** 2 / float(zeta)
    de = e - float(e_state)
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    out = np.zeros(z.shape, dtype=np.complex128)
    for wj, dj in zip(w, de):
        if abs(dj) < (1e-8 / beta if beta is not None else 1e-10):
            if beta is not None:
                out[np.abs(z) < 1e-10] -= wj * beta
        elif dj > 0:
            f = 1.0 if beta is None else 1.0 - np.exp(-beta * dj)
            out += wj * f * (1.0 / (z - dj) - 1.0 / (z + dj))
    return out


# ---- pair and exciton susceptibilities (ED_NORMAL/ED_CHI_PAIR.f90, ED_CHI_EXCT.f90; real build) ----------------------
# A term is (coef, O1, O2), O1 acting first, O = (create, iorb, ispin): create 1 = c^+, 0 = c; iorb 0-based; ispin 0 = up,
# 1 = down -- what SectorHamiltonian.apply_pairs_to takes.  A channel is (terms, isign), channels in the reference's order
# (ichan = 1, 2, ...: odd = lesser, even = greater).  A term whose sector does not exist (hamiltonian.pairs_sector) is to
# be left out of the call, and a channel left with no term skipped, as the reference does when getCsector /
# getCDGsector return 0.
_UP, _DW = 0, 1


def pair_chi_seeds(iorb: int, jorb: int):
    """The two channels of chi_pair(iorb, jorb): lanc_ed_build_pairChi_diag for jorb == iorb (ED_CHI_PAIR.f90:129-153),
    lanc_ed_build_pairChi_mix otherwise (:204-241; the channels 3, 4 of the _CMPLX_NORMAL build are not wanted)."""
    orbs = (iorb,) if iorb == jorb else (iorb, jorb)
    lesser = [(1.0, (0, a, _DW), (0, a, _UP)) for a in orbs]     # C_a,dw|gs> = |tmp>, C_a,up|tmp>; va + vb
    greater = [(1.0, (1, a, _UP), (1, a, _DW)) for a in orbs]    # C^+_a,up|gs> = |tmp>, C^+_a,dw|tmp>; va + vb
    return [(lesser, +1), (greater, -1)]


def exct_chi_seeds(indx: int, iorb: int, jorb: int):
    """The channels of chi_exct(indx, iorb, jorb), indx as the reference counts it: 1 singlet, 2 triplet-XY, 3 triplet-Z.
    Singlet and triplet-Z (auxiliary_vvinit_manipulation, ED_CHI_EXCT.f90:513-592): two channels, vup + comb_sign vdw
    with the orbitals swapped in the greater one; triplet-XY (:178-235): four channels of one term each."""
    if indx == 2:
        return [([(1.0, (0, jorb, _UP), (1, iorb, _DW))], +1),   # C_b,up|gs>, C^+_a,dw|tmp>: first lesser
                ([(1.0, (0, iorb, _DW), (1, jorb, _UP))], -1),   # C_a,dw|gs>, C^+_b,up|tmp>: first greater
                ([(1.0, (0, jorb, _DW), (1, iorb, _UP))], +1),   # C_b,dw|gs>, C^+_a,up|tmp>: second lesser
                ([(1.0, (0, iorb, _UP), (1, jorb, _DW))], -1)]   # C_a,up|gs>, C^+_b,dw|tmp>: second greater
    if indx not in (1, 3):
        raise ValueError("exct_chi_seeds: indx is 1 (singlet), 2 (triplet-XY) or 3 (triplet-Z)")
    comb_sign = 1.0 if indx == 1 else -1.0
    out = []
    for a, b, isign in ((iorb, jorb, +1), (jorb, iorb, -1)):
        out.append(([(1.0, (0, b, _UP), (1, a, _UP)),            # vup  = C^+_a,up C_b,up|gs>
                     (comb_sign, (0, b, _DW), (1, a, _DW))],     # vdw  = C^+_a,dw C_b,dw|gs>
                    isign))
    return out


def chi_channel(alanc, blanc, norm2: float, e_state: float, isign: int, ichan: int, z, beta: float | None,
                zeta: float = 1.0, mirror: bool = False, axis: str = "m"):
    """The share of one channel of one state in chi(z), from the tridiagonalisation of the channel's seed
    (apply_pairs_to, lanczos_tridiag_dev).  add_to_lanczos_pairChi / add_to_lanczos_exctChi (ED_CHI_PAIR.f90:302-368):
    weights peso_j = norm2 Z(1,j)^2 / zeta, poles de_j = isign (E_j - e_state) of the tridiagonal matrix's eigenpairs (a
    state's Boltzmann factor is the caller's).  get_Chiab (ED_CHI_PAIR.f90:431-508) sums them: a pole with
    |beta de| < 1e-8 adds 0.5 peso beta at z = 0 only (axis "r": at Re z = 0); otherwise only the poles with
    merge(de, -de, mod(ichan, 2) == 1) > 0 count,
        lesser  (ichan odd):   - peso (1 - exp(-beta de)) / (z - de)
        greater (ichan even):  + peso (1 - exp(+beta de)) / (z - de).
    ichan counts from 1.  mirror=True returns (chi, chi_mirror), chi_mirror the share in chi(jorb, iorb) of
    ED_CHI_EXCT.f90:475-485: the same with (z - de) -> (z + de) and the opposite sign, the zero pole unchanged.
    beta = None is zero temperature: the thermal factors are 1 and a zero-energy pole (|de| < 1e-10) adds nothing.
    The imaginary-time axis is not served."""
    if axis not in ("m", "r"):
        raise ValueError("chi_channel: axis is 'm' or 'r'")
    a = np.asarray(alanc, dtype=np.float64)
    b = np.asarray(blanc, dtype=np.float64)
    t = np.diag(a) + np.diag(b[1:], 1) + np.diag(b[1:], -1)
    e, zv = np.linalg.eigh(t)
    w = float(norm2) * zv[0, :] ** 2 / float(zeta)
    de = int(isign) * (e - float(e_state))
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    at_zero = (np.abs(z) if axis == "m" else np.abs(z.real)) < 1e-10
    lesser = int(ichan) % 2 == 1
    out = np.zeros(z.shape, dtype=np.complex128)
    mir = np.zeros(z.shape, dtype=np.complex128)
    for wj, dj in zip(w, de):
        if (abs(beta * dj) < 1e-8) if beta is not None else (abs(dj) < 1e-10):
            if beta is not None:
                out[at_zero] += 0.5 * wj * beta
                mir[at_zero] += 0.5 * wj * beta
        elif (dj if lesser else -dj) > 0:
            if lesser:
                f = wj * (1.0 if beta is None else 1.0 - np.exp(-beta * dj))
                out -= f / (z - dj)
                mir += f / (z + dj)
            else:
                f = wj * (1.0 if beta is None else 1.0 - np.exp(beta * dj))
                out += f / (z - dj)
                mir -= f / (z + dj)
    return (out, mir) if mirror else out
