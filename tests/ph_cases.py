"""Shared helpers of the phonon-operator tests (tests/test_gpu_phonons.py, tests/test_ph_host.py): impurity occupation
classes from the sector maps, and numpy restatements of the phonon density matrix and of the displacement seed."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53


def ternary_class(nt) -> np.ndarray:
    """class = sum_a nt[a] 3^a of the occupations nt[norb, n] (the reference's val - 1)"""
    nt = np.asarray(nt, dtype=np.int64)
    return (nt * (3 ** np.arange(nt.shape[0]))[:, None]).sum(axis=0)


def normal_classes(pm, nup, ndw) -> np.ndarray:
    """class of every electronic index i_el = iup + idw DimUp of the normal-mode sector"""
    from edipack_amd.hamiltonian import sector_map
    mu, md = sector_map(pm, nup, ndw, 0), sector_map(pm, nup, ndw, 1)
    nt = np.array([np.tile((mu >> a) & 1, md.size) + np.repeat((md >> a) & 1, mu.size) for a in range(pm.norb)])
    return ternary_class(nt)


def flat_classes(pm, mp) -> np.ndarray:
    """class of every row of a superc / nonsu2 sector map"""
    return ternary_class(np.array([((mp >> a) & 1) + ((mp >> (pm.ns + a)) & 1) for a in range(pm.norb)]))


def class_occupations(norb: int) -> np.ndarray:
    """nt[a, c] = occupation of orbital a in class c"""
    c = np.arange(3 ** norb)
    return np.array([(c // 3 ** a) % 3 for a in range(norb)])


def ref_ph_rdm(cls, v, dimph: int, ncls: int) -> np.ndarray:
    """rho[c, n, m] = sum_{i_el in c} v(i_el, n) conj v(i_el, m), summed in extended precision"""
    cplx = np.iscomplexobj(v)
    V = v.reshape(dimph, -1).astype(np.clongdouble if cplx else np.longdouble)
    rho = np.zeros((ncls, dimph, dimph), dtype=V.dtype)
    for c in np.unique(cls):
        Vc = V[:, cls == c]
        rho[c] = (Vc[:, None, :] * np.conj(Vc)[None, :, :]).sum(axis=2)
    return rho


def ref_xph(v, dimph: int) -> np.ndarray:
    """(b + b+) v exactly as the kernel writes it, per component: sqrt(n+1) v[n+1] + sqrt(n) v[n-1], one product in the
    edge blocks"""
    V = np.ascontiguousarray(v).view(np.float64).reshape(dimph, -1)
    out = np.empty_like(V)
    for n in range(dimph):
        if n == 0:
            out[n] = np.sqrt(n + 1.) * V[n + 1]
        elif n == dimph - 1:
            out[n] = np.sqrt(float(n)) * V[n - 1]
        else:
            out[n] = np.sqrt(n + 1.) * V[n + 1] + np.sqrt(float(n)) * V[n - 1]
    return out.reshape(-1).view(v.dtype)


def random_vector(dim: int, cplx: bool, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(dim)
    return v + 1j * rng.standard_normal(dim) if cplx else v


def set_phonons(pm, nph: int, general: bool = False):
    """the phonon parameters test_phonon_sector_sums_over_the_phonon_blocks uses; general: a non-diagonal g_ph"""
    g = np.diag(np.linspace(0.3, 0.5, pm.norb)) if pm.norb > 1 else np.array([[0.3]])
    if general:
        g = g + 0.1 * (np.ones((pm.norb, pm.norb)) - np.eye(pm.norb))
    pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = nph, 0.8, 0.0, g
    return pm
