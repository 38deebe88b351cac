"""GPU tests of the phonon operators on device vectors: edigpu_apply_xph (the seed (b + b+)|v> of the phonon Green's
function) and edigpu_ph_rdm (the phonon reduced density matrix per impurity occupation class).

References are numpy on the host from the sector maps, summed in extended precision (tests/ph_cases.py).  Tolerances are
derived, not measured: an entry of rho is a sum of at most dim_el products, each rounded once, so in ANY summation order
its error is at most (dim_el + 1) u sum |v_n| |v_m| <= (dim_el + 1) u norm2, u = 2^-53; the tests allow 2 dim_el u norm2
for real vectors and 4 dim_el u norm2 for complex ones (a complex product is two products and a sum).  The seed is two
products and one sum, uncontracted, with square roots from the host's sqrt: it must be bit-equal to the numpy expression.

The Jz-basis builders refuse nph > 0 ("phonon sectors are not built in the Jz basis"), and so does edigpu_normal_build_z:
there is no Jz case and no complex normal-mode case; the complex paths run on the superc / nonsu2 sectors."""
import ctypes as C

import numpy as np
import pytest

from tests.common import make_models
from tests.ph_cases import (U, class_occupations, flat_classes, normal_classes, random_vector, ref_ph_rdm, ref_xph,
                            set_phonons)

pytestmark = pytest.mark.gpu

GUARD = 3.25


def _handles():
    from edipack_amd.hamiltonian import SectorHamiltonian
    return SectorHamiltonian


def _buffers(h, v, odd=False):
    """one device buffer | guard | src | guard | dst (filled with 7.0) | guard |; odd: src starts 8 bytes past a 16-byte
    boundary.  Returns (buffer, src view, dst view, list of guard slices)."""
    import torch
    w = h.dim * (2 if h.is_complex else 1)
    g = 3 if odd else 2
    buf = torch.full((3 * g + 2 * w,), GUARD, dtype=torch.float64, device="cuda")
    src, dst = buf[g:g + w], buf[2 * g + w:2 * g + 2 * w]
    assert src.data_ptr() % 16 == (8 if odd else 0)
    src.copy_(torch.from_numpy(np.ascontiguousarray(v).view(np.float64)))
    dst.fill_(7.0)
    guards = [buf[:g], buf[g + w:2 * g + w], buf[2 * g + 2 * w:]]
    return buf, src, dst, guards


def check_sector(h, cls, seed, odd=False):
    """every assertion of this file that needs one handle and the classes of its electronic states"""
    import torch
    norb, dimph = h.norb, h.nph + 1
    ncls, dim_el = 3 ** norb, cls.size
    assert h.dim == dim_el * dimph
    cplx = h.is_complex
    v = random_vector(h.dim, cplx, seed)
    buf, src, dst, guards = _buffers(h, v, odd)
    # ---- density matrix: tolerance, Hermiticity, trace, determinism
    rho, n2 = h.ph_rdm(src.data_ptr())
    ref = ref_ph_rdm(cls, v, dimph, ncls)
    n2r = float(np.sum(np.abs(v.astype(np.clongdouble if cplx else np.longdouble)) ** 2))
    tol = (4 if cplx else 2) * dim_el * U * n2r
    err = float(np.max(np.abs(rho[0] - ref)))
    print(f"ph_rdm dim_el={dim_el} DimPh={dimph} max|drho|={err:.3e} |dnorm2|={abs(n2[0] - n2r):.3e} tol={tol:.3e}")
    assert rho.shape == (1, ncls, dimph, dimph) and rho.dtype == (np.complex128 if cplx else np.float64)
    assert err <= tol
    assert all(np.array_equal(rho[0, c], rho[0, c].conj().T) for c in range(ncls))
    assert abs(n2[0] - n2r) <= tol
    assert abs(n2[0] - np.real(np.trace(rho[0], axis1=1, axis2=2)).sum()) <= tol
    rho2, n22 = h.ph_rdm(src.data_ptr())
    assert np.array_equal(rho, rho2) and np.array_equal(n2, n22)
    # ---- sum_c rho[c] diagonal = prob_ph
    from edipack_amd.observables import from_ph_rdm
    V = v.reshape(dimph, dim_el)
    prob = np.sum(np.abs(V.astype(np.clongdouble if cplx else np.longdouble)) ** 2, axis=1)
    assert np.max(np.abs(from_ph_rdm(rho[0]).prob_ph - prob)) <= tol
    # ---- class weights against the merged moments kernel: dens, docc, n2 diagonal
    M, on2 = h.occ_moments(src.data_ptr())
    tol_occ = 2 * h.dim * U * n2r
    P = np.real(np.trace(rho[0], axis1=1, axis2=2))
    nt = class_occupations(norb)
    for a in range(norb):
        Uaa, Daa, Xaa = M[0, a, a], M[0, norb + a, norb + a], M[0, a, norb + a]
        assert abs(np.sum(nt[a] * P) - (Uaa + Daa)) <= tol + tol_occ
        assert abs(np.sum(P[nt[a] == 2]) - Xaa) <= tol + tol_occ
        assert abs(np.sum(nt[a] ** 2 * P) - (Uaa + Daa + 2 * Xaa)) <= tol + tol_occ
    assert abs(on2[0] - n2[0]) <= tol + tol_occ
    # ---- seed: bit-equal, nothing of the fill left, source and guards untouched
    h.apply_xph(src.data_ptr(), dst.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.array_equal(out.view(v.dtype), ref_xph(v, dimph))
    assert not np.any(out == 7.0)
    assert np.array_equal(src.cpu().numpy().view(v.dtype), v)
    assert all(bool((g == GUARD).all().item()) for g in guards)
    return v, rho[0], n2[0], out.view(v.dtype)


NORMAL_CASES = [
    # bath, norb, nbath, (nup, ndw), nph, general g_ph
    ("normal", 2, 2, (3, 3), 3, False),    # 20 x 20, baseline
    ("normal", 2, 2, (3, 3), 1, False),    # DimPh 2: no (n, n+2) term, both blocks are edges
    ("normal", 2, 2, (1, 4), 2, False),    # rows of 6: shorter than a wave
    ("normal", 2, 2, (0, 0), 3, False),    # dim_el 1, one class populated
    ("normal", 2, 2, (6, 6), 3, False),
    ("normal", 2, 2, (2, 2), 2, False),    # 15 x 15 odd: the 8-byte paths (odd block stride, unaligned destination)
    ("normal", 3, 3, (6, 6), 1, False),    # 924^2: several partials per class, blocks split over workgroups
    ("normal", 3, 3, (1, 6), 2, False),    # many short rows
    ("normal", 3, 3, (6, 1), 2, False),    # few long rows
    ("hybrid", 5, 3, (4, 4), 2, False),    # 243 classes, largest tables
    ("normal", 2, 2, (3, 3), 15, False),   # DimPh 16: largest all-register form
    ("normal", 2, 2, (3, 3), 16, False),   # DimPh 17: first past it, 8 x 8 tiles
    ("normal", 2, 2, (3, 3), 31, False),   # DimPh 32: the cap
    ("normal", 2, 2, (3, 3), 2, True),     # general-coupling handle
]


@pytest.mark.parametrize("bath,norb,nbath,sec,nph,general", NORMAL_CASES)
def test_normal_sectors(gpu, bath, norb, nbath, sec, nph, general):
    _, pm = make_models("normal", bath, norb, nbath, seed=11)
    set_phonons(pm, nph, general)
    h = _handles().normal_from_model(pm, *sec)
    check_sector(h, normal_classes(pm, *sec), seed=sum(sec) + nph)
    h.destroy()


def _flat_handle(mode, form):
    from edipack_amd.hamiltonian import sector_map
    H = _handles()
    if mode == "superc":
        _, pm = make_models("superc", "hybrid", 2, 3, seed=12)
        set_phonons(pm, 2)
        sec = 0
    else:
        _, pm = make_models("nonsu2", "normal", 1, 4, seed=13)
        set_phonons(pm, 3)
        sec = 5
    h = (H.flat_from_model if form == "stored" else H.direct_from_model)(pm, sec)
    return h, flat_classes(pm, sector_map(pm, sec))


@pytest.mark.parametrize("form", ["stored", "direct"])
@pytest.mark.parametrize("mode", ["superc", "nonsu2"])
def test_flat_sectors(gpu, mode, form):
    h, cls = _flat_handle(mode, form)
    assert mode != "nonsu2" or cls.size == 252
    check_sector(h, cls, seed=70)
    h.destroy()


def test_flat_vector_at_an_odd_offset(gpu):
    """an interleaved complex vector 8 bytes past a 16-byte boundary takes the kernels' two-load paths"""
    h, cls = _flat_handle("superc", "direct")
    check_sector(h, cls, seed=71, odd=True)
    h.destroy()


def test_several_vectors_equal_single_calls_bit_for_bit(gpu):
    import torch
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    for sec in ((3, 3), (2, 2)):     # (2, 2): dim_el 225, the second vector starts at an odd element
        set_phonons(pm, 2)
        h = _handles().normal_from_model(pm, *sec)
        cls = normal_classes(pm, *sec)
        vs = np.stack([random_vector(h.dim, False, 20 + k) for k in range(3)])
        vd = torch.from_numpy(vs).cuda()
        rho, n2 = h.ph_rdm(vd.data_ptr(), 3)
        assert rho.shape == (3, 9, 3, 3)
        for k in range(3):
            rk, nk = h.ph_rdm(vd[k].data_ptr())
            assert np.array_equal(rho[k], rk[0]) and n2[k] == nk[0]
            assert np.max(np.abs(rho[k] - ref_ph_rdm(cls, vs[k], 3, 9))) <= 2 * cls.size * U * float(vs[k] @ vs[k])
        h.destroy()


def test_seed_norm_is_x2_of_the_density_matrix(gpu):
    """<seed|seed> = <v| (b + b+)^2 |v> in the truncated space.  There <n|(b + b+)^2|n> = 2n + 1 except on the top level,
    where the step to Nph + 1 is cut: Nph instead of 2 Nph + 1.  The reference's X2_ph counts 2n + 1 on every level, so
    <seed|seed> = 2 x2 - (Nph + 1) R[Nph, Nph], x2 and R not normalised.
    Tolerance 2 dim u norm2 (Nph + 1) * 4, four units of 2 dim u norm2 (Nph + 1):
    1. the errors of the R_nn together are at most (dim_el + 1) u norm2 (the bound of one sum over the whole vector) and
       carry weights 2n + 1 <= 2 (Nph + 1);
    2. the errors of the R[n, n+2] are at most (dim_el + 1) u sum_i |v(i, n)| |v(i, n+2)|, together at most
       (dim_el + 1) u norm2, with weights 2 sqrt((n+1)(n+2)) <= 2 (Nph + 1);
    3. the host's sums over the classes and levels in double: a few dozen roundings of terms <= 2 (Nph + 1) norm2;
    4. the seed's own rounding (two products and a sum per element: relative 3 u, so 6 u on its square) against
       <seed|seed> <= 2 (Nph + 1) norm2.  dim = dim_el (Nph + 1) exceeds dim_el + 1 and the small counts of 3 and 4."""
    import torch
    from edipack_amd.observables import from_ph_rdm
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    set_phonons(pm, 3)
    h = _handles().normal_from_model(pm, 3, 3)
    v, rho, n2, seed = check_sector(h, normal_classes(pm, 3, 3), seed=81)
    o = from_ph_rdm(rho)
    R = rho.sum(axis=0)
    ss = float(np.sum(seed.astype(np.longdouble) ** 2))
    want = 2 * o.x2_ph - (h.nph + 1) * R[h.nph, h.nph]
    tol = 2 * h.dim * U * n2 * (h.nph + 1) * 4
    print(f"<seed|seed>={ss!r} 2 x2 - (Nph+1) R_top={want!r} diff={abs(ss - want):.3e} tol={tol:.3e}")
    assert abs(ss - want) <= tol
    h.destroy()


def test_phonon_gf_chain_without_a_host_copy(gpu):
    """eigenvector -> (b + b+) seed -> tridiagonalisation, all on the device (lanc_build_gf_phonon_main,
    ED_GF_NORMAL.f90:278-345); alpha, beta, niter bit-equal to the host-seeded entry point on the numpy-made seed"""
    import torch
    from edipack_amd import capi
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    set_phonons(pm, 3)
    h = _handles().normal_from_model(pm, 3, 3)
    evec = torch.empty(h.dim, dtype=torch.float64, device="cuda")
    ev, nc, nmv = np.zeros(1), C.c_int(0), C.c_int(0)
    capi.check(capi.lib().edigpu_lanczos_eigh_multi(h._h, 1, 0, 1e-13, 300, None, capi.pd(ev), C.c_void_p(evec.data_ptr()),
                                                    C.byref(nc), C.byref(nmv)), "edigpu_lanczos_eigh_multi")
    seed = torch.empty_like(evec)
    h.apply_xph(evec.data_ptr(), seed.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    a1, b1, n1, nrm2 = h.lanczos_tridiag_dev(seed.data_ptr(), 30)
    # for checking only: the vector on the host
    ref = ref_xph(evec.cpu().numpy(), h.nph + 1)
    assert np.array_equal(seed.cpu().numpy(), ref)
    a0, b0, n0 = h.lanczos_tridiag(ref, 30)
    assert n0 == n1 and np.array_equal(a0, a1) and np.array_equal(b0, b1)
    assert abs(nrm2 - ref @ ref) < 1e-12 * max(1.0, ref @ ref)
    h.destroy()


def test_phonon_gf_end_to_end(gpu):
    """D(i nu_n) of a one-orbital Holstein impurity from the device chain against the dense spectral sum"""
    import torch
    from edipack_amd import capi
    from edipack_amd.observables import phonon_gf
    _, pm = make_models("normal", "normal", 1, 2, seed=11)
    set_phonons(pm, 3)
    h = _handles().normal_from_model(pm, 1, 1)
    dim, dimph = h.dim, h.nph + 1
    assert dim == 36
    eye = np.eye(dim)
    Hd = np.stack([h.apply(eye[:, k].copy()) for k in range(dim)], axis=1)
    assert np.max(np.abs(Hd - Hd.T)) < 1e-13
    e, x = np.linalg.eigh(Hd)
    assert e[1] - e[0] > 1e-6
    evec = torch.empty(dim, dtype=torch.float64, device="cuda")
    ev, nc, nmv = np.zeros(1), C.c_int(0), C.c_int(0)
    capi.check(capi.lib().edigpu_lanczos_eigh_multi(h._h, 1, 0, 1e-13, 300, None, capi.pd(ev), C.c_void_p(evec.data_ptr()),
                                                    C.byref(nc), C.byref(nmv)), "edigpu_lanczos_eigh_multi")
    assert abs(ev[0] - e[0]) < 1e-10
    seed = torch.empty_like(evec)
    h.apply_xph(evec.data_ptr(), seed.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    al, bl, nit, nrm2 = h.lanczos_tridiag_dev(seed.data_ptr(), dim)
    beta = 50.0
    z = 1j * 2.0 * np.pi * np.arange(8) / beta    # the reference's formula is regular at nu = 0: it stays in
    D = phonon_gf(al[:nit], bl[:nit], nrm2, ev[0], z, beta=beta)
    # dense: weights |<j|b + b+|0>|^2, poles E_j - E_0, the same bosonic sum (get_impD_normal, ED_GF_NORMAL.f90:641-686)
    xs = ref_xph(x[:, 0].copy(), dimph)
    wj, dj = (x.T @ xs) ** 2, e - e[0]
    Dd = np.zeros(z.size, complex)
    for w_, d_ in zip(wj, dj):
        if abs(beta * d_) < 1e-8:
            Dd[np.abs(z) < 1e-10] -= w_ * beta
        elif d_ > 0:
            Dd += w_ * (1.0 - np.exp(-beta * d_)) * (1.0 / (z - d_) - 1.0 / (z + d_))
    err = np.max(np.abs(D - Dd)) / np.max(np.abs(Dd))
    print(f"phonon_gf niter={nit} max|D|={np.max(np.abs(Dd)):.6e} rel err={err:.3e}")
    assert err < 1e-9
    h.destroy()


def test_refusals(gpu):
    import torch
    from edipack_amd import capi
    from oracle import oracle as O
    H = _handles()
    buf = torch.zeros(8192, dtype=torch.float64, device="cuda")
    a, b = buf.data_ptr(), buf.data_ptr() + 4096 * 8

    def both_refuse(h, match):
        with pytest.raises(capi.EdigpuError, match="edigpu_apply_xph: .*" + match):
            h.apply_xph(a, b)
        with pytest.raises(capi.EdigpuError, match="edigpu_ph_rdm: .*" + match):
            h.ph_rdm(a)
        h.destroy()

    om, pm = make_models("normal", "normal", 2, 2, seed=11, jxp=0.0)
    hl = np.zeros_like(om.hloc)
    for k in range(2):
        hl[0, 0, k, k] = om.hloc[0, 0, k, k].real
    pm.hloc = hl                                             # what ed_total_ud=F requires
    both_refuse(H.orbs_from_model(pm, (2, 1), (1, 2)), "ed_total_ud=F sectors are not supported")
    ho = O.HNormal(om, 3, 3)
    both_refuse(H.normal_from_arrays(ho.dimup, ho.dimdw, ho.hd, ho.up, ho.dw, ho.nd), "must be built from a model")
    _, ps = make_models("superc", "hybrid", 2, 3, seed=12)
    both_refuse(H.flat_from_model(ps, 0, row_first=1, row_count=10), "must hold the whole sector")
    _, pn = make_models("normal", "normal", 2, 2, seed=11)
    both_refuse(H.normal_from_model(pn, 3, 3, dw_first=2, dw_count=5), "must hold the whole sector")
    both_refuse(H.normal_from_model(pn, 3, 3), "the handle has no phonons")
    both_refuse(H.flat_from_model(ps, 0), "the handle has no phonons")
    # overlap: the destination starts inside the source
    set_phonons(pn, 2)
    h = H.normal_from_model(pn, 2, 2)
    for dst in (a, a + 8, a + 8 * (h.dim - 1)):
        with pytest.raises(capi.EdigpuError, match="edigpu_apply_xph: .*must not overlap"):
            h.apply_xph(a, dst)
    with pytest.raises(capi.EdigpuError, match="edigpu_apply_xph: .*must not overlap"):
        h.apply_xph(a + 8 * (h.dim - 1), a)
    h.destroy()
    # DimPh = 33: the density matrix is refused, the seed is not
    set_phonons(pn, 32)
    h = H.normal_from_model(pn, 1, 4)
    assert h.dim == 33 * 90 and 2 * h.dim <= 8192
    with pytest.raises(capi.EdigpuError, match="edigpu_ph_rdm: DimPh = 33 exceeds the limit of 32"):
        h.ph_rdm(a)
    v = random_vector(h.dim, False, 5)
    buf[:h.dim].copy_(torch.from_numpy(v))
    h.apply_xph(a, a + 8 * h.dim)
    torch.cuda.synchronize()
    assert np.array_equal(buf[h.dim:2 * h.dim].cpu().numpy(), ref_xph(v, 33))
    h.destroy()
