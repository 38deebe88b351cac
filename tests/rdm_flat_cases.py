"""Shared by tests/test_rdm_flat_host.py and tests/test_gpu_rdm_flat.py: the sector list of edigpu_imp_rdm_flat and the
numpy restatement of imp_rdm_superc (ED_RDM_SUPERC.f90:54-183) / imp_rdm_nonsu2 (ED_RDM_NONSU2.f90:54-188).

The tolerance of every comparison is derived, not measured: the signs are +-1, an entry is a sum of at most dim products
x_p conj(x_q), and sum |x_p| |x_q| <= norm2, so ANY summation order stays within 4 dim u norm2, u = 2^-53."""
import numpy as np

from tests.common import make_models

U = 2.0 ** -53
MODE = {"superc": 1, "nonsu2": 2}

# mode, bath, norb, nbath, sector (Sz / Ntot), seed of make_models
SECTORS = [
    ("nonsu2", "hybrid", 2, 2, 4, 13),
    ("nonsu2", "normal", 2, 2, 6, 13),    # 924
    ("nonsu2", "normal", 2, 2, 0, 13),    # dim 1
    ("nonsu2", "normal", 2, 2, 12, 13),   # dim 1
    ("nonsu2", "normal", 2, 2, 1, 13),    # 12: one impurity class only
    ("nonsu2", "normal", 1, 4, 5, 13),    # 252: a 2 x 2 spin-flip block, everything else diagonal
    ("nonsu2", "hybrid", 3, 3, 6, 13),    # 924: blocks of 20
    ("nonsu2", "hybrid", 4, 2, 6, 13),    # 924: blocks of 70, the classes split between workgroups
    ("superc", "hybrid", 2, 3, 0, 12),    # 252
    ("superc", "hybrid", 2, 3, 5, 12),    # extreme Sz: dim 1
    ("superc", "hybrid", 2, 3, -5, 12),   # extreme Sz: dim 1
    ("superc", "normal", 2, 2, 0, 12),    # 924
    ("superc", "normal", 2, 2, 1, 12),    # 792
]


def _popcount(x):
    x = np.asarray(x, np.int64)
    c = np.zeros(x.shape, np.int64)
    for k in range(32):
        c += (x >> k) & 1
    return c


def flat_model(mode, bath, norb, nbath, seed):
    return make_models(mode, bath, norb, nbath, seed=seed)[1]


def flat_map(pm, sec):
    from edipack_amd.hamiltonian import sector_map
    return sector_map(pm, sec)


def numpy_rdm_flat(mp, ns, norb, v, nblk=1, dtype=None, sign=True):
    """The two reference routines restated: the elements of v[nblk, dim_el] grouped by their bath words (Bup, Bdw) (and
    phonon block) into the columns of A[io, tile], io = Iup + 2^norb Idw, each times sgn = -1 where popcount(Bup) and
    popcount(Idw) are both odd (signI of the reference); then rho = A A^H, so rho[io, jo] carries signI signJ.  Nothing
    is assumed about the order of the map.  dtype: np.longdouble / np.clongdouble for the extended-precision reference;
    sign=False drops sgn (what a kernel without the sign would return)."""
    mp = np.asarray(mp, np.int64)
    mask, D = (1 << norb) - 1, 4 ** norb
    V = np.asarray(v).reshape(nblk, mp.size)
    if dtype is not None:
        V = V.astype(dtype)
    iup, idw = mp & ((1 << ns) - 1), mp >> ns
    io = (iup & mask) + ((idw & mask) << norb)
    bup, bdw = iup >> norb, idw >> norb
    tiles, t = np.unique(bup + (bdw << (ns - norb)), return_inverse=True)
    t = t.reshape(-1)
    sgn = np.where((_popcount(bup) & 1) & (_popcount(idw & mask) & 1), -1.0, 1.0) if sign else np.ones(mp.size)
    rho = np.zeros((D, D), V.dtype)
    step = max(1, (1 << 16) // D)          # tiles of one slice of A
    order = np.argsort(t, kind="stable")
    io, t, sgn = io[order], t[order], sgn[order]
    cut = np.searchsorted(t, np.arange(0, tiles.size + step, step))
    for k in range(nblk):
        x = V[k][order] * sgn
        for j, t0 in enumerate(range(0, tiles.size, step)):
            sel = slice(cut[j], cut[j + 1])
            A = np.zeros((D, min(step, tiles.size - t0)), V.dtype)
            A[io[sel], t[sel] - t0] = x[sel]
            rho += A @ A.conj().T
    return rho


def ref_rdm_flat(mp, ns, norb, v, nblk=1, sign=True):
    """(rho, norm2) in extended precision, rounded to double"""
    cplx = np.iscomplexobj(v)
    r = numpy_rdm_flat(mp, ns, norb, v, nblk, dtype=np.clongdouble if cplx else np.longdouble, sign=sign)
    n2 = float(np.sum(v.real.astype(np.longdouble) ** 2 + v.imag.astype(np.longdouble) ** 2))
    return r.astype(np.complex128 if cplx else np.float64), n2


def random_vector(dim, cplx, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(dim)
    return v + 1j * rng.standard_normal(dim) if cplx else v


def blocks_mask(mode, norb, ns=None):
    """mask[io, jo]: True where rho may be non-zero: equal ku + kd (nonsu2) or equal ku - kd (superc)"""
    io = np.arange(4 ** norb)
    ku, kd = _popcount(io & ((1 << norb) - 1)), _popcount(io >> norb)
    c = ku + kd if mode == "nonsu2" else ku - kd
    return c[:, None] == c[None, :]
