"""GPU tests of edigpu_imp_rdm: the impurity reduced density matrix rho = Tr_bath |v><v| of device vectors of normal-mode
sectors (imp_rdm_normal, ED_RDM_NORMAL.f90:146-209).

The reference is the numpy restatement of tests/test_rdm_host.py in extended precision.  The tolerance is derived, not
measured: an entry is a sum of at most dim products x_p conj(x_q), and sum |x_p| |x_q| <= norm2, so ANY summation order
stays within (dim + 2) u norm2 of the exact value, u = 2^-53; the tests allow 4 dim u norm2."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.common import make_models
from tests.test_rdm_host import SECTORS, numpy_rdm, random_vector, sector_maps

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _handles():
    from edipack_amd.hamiltonian import SectorHamiltonian
    return SectorHamiltonian


def ref_rdm(mu, md, norb, v, nblk=1):
    """(rho, norm2) in extended precision, rounded to double"""
    cplx = np.iscomplexobj(v)
    r = numpy_rdm(mu, md, norb, v, nblk, dtype=np.clongdouble if cplx else np.longdouble)
    n2 = float(np.sum(v.real.astype(np.longdouble) ** 2 + v.imag.astype(np.longdouble) ** 2))
    return r.astype(np.complex128 if cplx else np.float64), n2


def occupation_weights(norb):
    """bits[x, io]: occupation of orbital x (a up, norb + a down) in the impurity state io = Iup + 2^norb Idw"""
    io = np.arange(4 ** norb)
    return np.array([(io >> x) & 1 for x in range(2 * norb)], dtype=np.float64)


def check_sector(h, mu, md, norb, seed, nblk=1):
    """every assertion of this file that needs one handle and its maps"""
    import torch
    dim = mu.size * md.size * nblk
    assert h.dim == dim and h.norb == norb
    v = random_vector(dim, h.is_complex, seed)
    vd = torch.from_numpy(v).cuda()
    rho, n2 = h.imp_rdm(vd.data_ptr())
    ref, n2r = ref_rdm(mu, md, norb, v, nblk)
    tol = 4 * dim * U * n2r
    D = 4 ** norb
    assert rho.shape == (1, D, D) and rho.dtype == (np.complex128 if h.is_complex else np.float64)
    print(f"imp_rdm dim={dim} max|drho|={np.max(np.abs(rho[0] - ref)):.3e} |trace-norm2|={abs(np.trace(rho[0]).real - n2r):.3e} "
          f"|dnorm2|={abs(n2[0] - n2r):.3e} tol={tol:.3e}")
    assert np.max(np.abs(rho[0] - ref)) <= tol
    assert np.array_equal(rho[0], rho[0].conj().T)                      # exactly Hermitian
    assert abs(np.trace(rho[0]).real - n2r) <= tol and abs(n2[0] - n2r) <= tol
    rho2, n22 = h.imp_rdm(vd.data_ptr())
    assert np.array_equal(rho, rho2) and np.array_equal(n2, n22)        # fixed summation order
    # the diagonal holds the occupation moments: M[x, y] = sum_io rho[io, io] n_x(io) n_y(io)
    M, mn2 = h.occ_moments(vd.data_ptr())
    bits = occupation_weights(norb)
    Mr = (bits * np.real(np.diag(rho[0]))[None, :]) @ bits.T
    assert np.max(np.abs(Mr - M[0])) <= tol + 2 * dim * U * n2r
    assert np.array_equal(vd.cpu().numpy(), v)
    return v, rho[0]


CASES = SECTORS + [
    ("normal", 3, 3, (1, 6)),   # 12 x 924: many short rows
    ("normal", 3, 3, (6, 6)),   # 924^2: two chunks of columns, several workgroups per chunk, rows split between them
]


@pytest.mark.parametrize("bath,norb,nbath,sec", CASES)
def test_normal_sectors(gpu, bath, norb, nbath, sec):
    _, pm = make_models("normal", bath, norb, nbath, seed=11)
    h = _handles().normal_from_model(pm, *sec)
    mu, md = sector_maps(pm, sec)
    _, rho = check_sector(h, mu, md, norb, seed=sum(sec) + 3)
    if norb == 1:
        assert np.count_nonzero(rho - np.diag(np.diag(rho))) == 0
    h.destroy()


def test_several_vectors_equal_single_calls_bit_for_bit(gpu):
    import torch
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    for sec in ((3, 3), (2, 2)):     # (2, 2): dim 225, the second vector starts at an odd element
        h = _handles().normal_from_model(pm, *sec)
        mu, md = sector_maps(pm, sec)
        vs = np.stack([random_vector(h.dim, False, 20 + k) for k in range(3)])
        vd = torch.from_numpy(vs).cuda()
        rho, n2 = h.imp_rdm(vd.data_ptr(), 3)
        for k in range(3):
            rk, nk = h.imp_rdm(vd[k].data_ptr())
            assert np.array_equal(rho[k], rk[0]) and n2[k] == nk[0]
            ref, n2r = ref_rdm(mu, md, 2, vs[k])
            assert np.max(np.abs(rho[k] - ref)) <= 4 * h.dim * U * n2r
        h.destroy()


def test_vectors_at_odd_offsets(gpu):
    """8-byte aligned vectors, real and complex; the buffer around them is left alone"""
    import torch
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    mu, md = sector_maps(pm, (3, 2))
    for cplx in (False, True):
        h = _handles().normal_cmplx_from_model(pm, 3, 2) if cplx else _handles().normal_from_model(pm, 3, 2)
        v = random_vector(h.dim, cplx, 31)
        w = h.dim * (2 if cplx else 1)
        buf = torch.zeros(w + 2, dtype=torch.float64, device="cuda")
        src = buf[1:1 + w]
        assert src.data_ptr() % 16 == 8
        src.copy_(torch.from_numpy(v.view(np.float64)))
        rho, n2 = h.imp_rdm(src.data_ptr())
        ref, n2r = ref_rdm(mu, md, 2, v)
        tol = 4 * h.dim * U * n2r
        assert np.max(np.abs(rho[0] - ref)) <= tol and abs(n2[0] - n2r) <= tol
        assert np.array_equal(rho[0], rho[0].conj().T)
        assert buf[0].item() == 0.0 and buf[-1].item() == 0.0
        assert np.array_equal(src.cpu().numpy().view(v.dtype), v)
        h.destroy()


def test_complex_normal_sector(gpu):
    """a complex vector whose rho has an imaginary part: rho^T in place of rho (a swapped conjugate) fails"""
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    h = _handles().normal_cmplx_from_model(pm, 3, 2)
    assert h.is_complex
    mu, md = sector_maps(pm, (3, 2))
    v, rho = check_sector(h, mu, md, 2, seed=43)
    ref, n2r = ref_rdm(mu, md, 2, v)
    assert np.max(np.abs(ref.imag)) > 1e3 * 4 * h.dim * U * n2r
    assert np.max(np.abs(rho.T - ref)) > 1e3 * 4 * h.dim * U * n2r
    h.destroy()


def test_phonon_sector_traces_the_phonon_blocks(gpu):
    import torch
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    mu, md = sector_maps(pm, (3, 3))
    pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = 3, 0.8, 0.0, np.diag((0.3, 0.5))
    h = _handles().normal_from_model(pm, 3, 3)
    assert h.dim == 4 * 400
    v, rho = check_sector(h, mu, md, 2, seed=41, nblk=4)
    # the sum over the blocks, each taken as a vector of the electronic sector
    he = _handles().normal_from_model(make_models("normal", "normal", 2, 2, seed=11)[1], 3, 3)
    vd = torch.from_numpy(v).cuda()
    parts, _ = he.imp_rdm(vd.data_ptr(), 4)
    n2 = float(np.vdot(v, v).real)
    assert np.max(np.abs(parts.sum(axis=0) - rho)) <= 2 * 4 * h.dim * U * n2
    he.destroy()
    h.destroy()


def test_golden_rdm_from_a_device_eigenvector(gpu):
    """rdm.check of the reference's NORMAL_NORMAL directory from the lowest eigenvector of sector (3, 3), which never
    leaves the device, at the tolerance test_golden_observables_from_device_vectors uses"""
    import torch
    from edipack_amd import capi
    from edipack_amd.observables import entanglement_entropy, rdm_average, rdm_occupations
    from oracle import oracle as O
    from tests.test_oracle_golden import GOLD, _from_dir, golden_models
    g = GOLD["NORMAL_NORMAL"]
    inp, par = _from_dir("NORMAL_NORMAL")
    pm_par = {k: v for k, v in par.items() if k not in ("ed_hw_bath", "deltasc")}
    om, pm = golden_models(inp["ED_MODE"], inp["BATH_TYPE"], int(inp["NORB"]), int(inp["NBATH"]), pm_par)
    O.to_struct(om)
    h = _handles().normal_from_model(pm, 3, 3)
    e, nc, nmv = np.zeros(1), C.c_int(0), C.c_int(0)
    evec = torch.empty(h.dim, dtype=torch.float64, device="cuda")
    capi.check(capi.lib().edigpu_lanczos_eigh_multi(h._h, 1, 0, 1e-13, 300, None, capi.pd(e), C.c_void_p(evec.data_ptr()),
                                                    C.byref(nc), C.byref(nmv)), "edigpu_lanczos_eigh_multi")
    assert abs(e[0] - g["evals"][0]) < 1e-9
    rhos, n2 = h.imp_rdm(evec.data_ptr())
    rho = rdm_average(rhos, n2)
    gold = np.array(g["rdm"]).reshape(16, 16, 2)
    assert np.max(np.abs(gold[..., 1])) == 0.0
    print(f"max |rho - rdm.check| = {np.max(np.abs(rho - gold[..., 0])):.3e}")
    assert np.max(np.abs(rho - gold[..., 0])) < 1e-8
    up, dw, docc = rdm_occupations(rho, om.norb)
    assert np.max(np.abs(up + dw - np.array(g["dens"]))) < 1e-8 and np.max(np.abs(docc - np.array(g["docc"]))) < 1e-8
    ev = np.linalg.eigvalsh(gold[..., 0])
    assert abs(entanglement_entropy(rho) - float(-np.sum(ev[ev > 1e-300] * np.log(ev[ev > 1e-300])))) < 1e-6
    h.destroy()


def test_refusals(gpu):
    import torch
    from edipack_amd import capi
    from oracle import oracle as O
    H = _handles()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")

    def refuses(h, match):
        with pytest.raises(capi.EdigpuError, match=match):
            h.imp_rdm(buf.data_ptr())
        with pytest.raises(capi.EdigpuError, match=match):
            h.time_rdm(buf.data_ptr(), 0, 1)
        h.destroy()

    _, ps = make_models("superc", "hybrid", 2, 3, seed=12)
    refuses(H.flat_from_model(ps, 0), "only ed_mode=normal sectors are supported")
    refuses(H.direct_from_model(ps, 0), "only ed_mode=normal sectors are supported")
    om, pm = make_models("normal", "normal", 2, 2, seed=11, jxp=0.0)
    hl = np.zeros_like(om.hloc)
    for a in range(2):
        hl[0, 0, a, a] = om.hloc[0, 0, a, a].real
    pm.hloc = hl                                             # what ed_total_ud=F requires
    refuses(H.orbs_from_model(pm, (2, 1), (1, 2)), "ed_total_ud=F sectors are not supported")
    ho = O.HNormal(om, 3, 3)
    refuses(H.normal_from_arrays(ho.dimup, ho.dimdw, ho.hd, ho.up, ho.dw, ho.nd), "must be built from a model")
    _, pn = make_models("normal", "normal", 2, 2, seed=11)
    refuses(H.normal_from_model(pn, 3, 3, dw_first=2, dw_count=5), "must hold the whole sector")
    assert math.isfinite(buf.sum().item())
