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

Pure numpy: O(norb^2) numbers per vector reach the host."""
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
