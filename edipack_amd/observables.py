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

Pure numpy: O(norb^2) numbers per vector (16^norb for the density matrix) reach the host."""
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
