"""GPU tests of edigpu_imp_rdm_flat: the impurity reduced density matrix rho = Tr_bath |v><v| of device vectors of superc /
nonsu2 sectors (imp_rdm_superc, ED_RDM_SUPERC.f90:54-183; imp_rdm_nonsu2, ED_RDM_NONSU2.f90:54-188).

The reference is the numpy restatement of tests/rdm_flat_cases.py in extended precision.  The tolerance is derived, not
measured: the signs are +-1, an entry is a sum of at most dim products x_p conj(x_q), and sum |x_p| |x_q| <= norm2, so ANY
summation order stays within 4 dim u norm2 of the exact value, u = 2^-53."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.common import make_jz_models, make_models
from tests.rdm_flat_cases import SECTORS, U, blocks_mask, flat_map, flat_model, random_vector, ref_rdm_flat

pytestmark = pytest.mark.gpu


def _handles():
    from edipack_amd.hamiltonian import SectorHamiltonian
    return SectorHamiltonian


def occupation_weights(norb):
    """bits[x, io]: occupation of orbital x (a up, norb + a down) in the impurity state io = Iup + 2^norb Idw"""
    io = np.arange(4 ** norb)
    return np.array([(io >> x) & 1 for x in range(2 * norb)], dtype=np.float64)


def check_sector(h, mp, ns, norb, mode, seed, nblk=1):
    """every assertion of this file that needs one handle and its map"""
    import torch
    dim = mp.size * nblk
    assert h.dim == dim and h.norb == norb
    v = random_vector(dim, h.is_complex, seed)
    vd = torch.from_numpy(v).cuda()
    rho, n2 = h.imp_rdm_flat(vd.data_ptr())
    ref, n2r = ref_rdm_flat(mp, ns, norb, v, nblk)
    tol = 4 * dim * U * n2r
    D = 4 ** norb
    assert rho.shape == (1, D, D) and rho.dtype == (np.complex128 if h.is_complex else np.float64)
    print(f"imp_rdm_flat dim={dim} max|drho|={np.max(np.abs(rho[0] - ref)):.3e} "
          f"|trace-norm2|={abs(np.trace(rho[0]).real - n2r):.3e} |dnorm2|={abs(n2[0] - n2r):.3e} tol={tol:.3e}")
    assert np.max(np.abs(rho[0] - ref)) <= tol
    assert np.array_equal(rho[0], rho[0].conj().T)                      # exactly Hermitian
    assert np.count_nonzero(rho[0][~blocks_mask(mode, norb)]) == 0
    assert abs(np.trace(rho[0]).real - n2r) <= tol and abs(n2[0] - n2r) <= tol
    rho2, n22 = h.imp_rdm_flat(vd.data_ptr())
    assert np.array_equal(rho, rho2) and np.array_equal(n2, n22)        # fixed summation order
    # the diagonal holds the occupation moments: M[x, y] = sum_io rho[io, io] n_x(io) n_y(io)
    M, _ = h.occ_moments(vd.data_ptr())
    bits = occupation_weights(norb)
    Mr = (bits * np.real(np.diag(rho[0]))[None, :]) @ bits.T
    assert np.max(np.abs(Mr - M[0])) <= tol + 2 * dim * U * n2r
    assert np.array_equal(vd.cpu().numpy(), v)
    return v, rho[0]


@pytest.mark.parametrize("mode,bath,norb,nbath,sec,seed", SECTORS)
def test_flat_sectors(gpu, mode, bath, norb, nbath, sec, seed):
    pm = flat_model(mode, bath, norb, nbath, seed)
    h = _handles().flat_from_model(pm, sec)
    mp = flat_map(pm, sec)
    _, rho = check_sector(h, mp, pm.ns, norb, mode, seed=sec + 30)
    if norb == 1:       # only |up> and |dw> of the one orbital are coupled
        off = rho - np.diag(np.diag(rho))
        assert np.count_nonzero(off) == np.count_nonzero(off[[1, 2], [2, 1]])
    h.destroy()


@pytest.mark.parametrize("mode,bath,norb,nbath,sec,seed", [SECTORS[0], SECTORS[8], SECTORS[12]])
def test_stored_and_on_the_fly_handles_return_the_same_bits(gpu, mode, bath, norb, nbath, sec, seed):
    import torch
    pm = flat_model(mode, bath, norb, nbath, seed)
    hs, hd = _handles().flat_from_model(pm, sec), _handles().direct_from_model(pm, sec)
    assert hs.is_complex == hd.is_complex
    vd = torch.from_numpy(random_vector(hs.dim, hs.is_complex, 17)).cuda()
    (rs, ns_), (rd, nd_) = hs.imp_rdm_flat(vd.data_ptr()), hd.imp_rdm_flat(vd.data_ptr())
    assert np.array_equal(rs, rd) and np.array_equal(ns_, nd_) and np.count_nonzero(rs) > 0
    hs.destroy()
    hd.destroy()


def test_several_workgroups_and_slabs_on_the_fly(gpu):
    """nonsu2, three orbitals, Ns = 9, N = 9: 48 620 states, many workgroups per panel"""
    pm = flat_model("nonsu2", "normal", 3, 2, 13)
    h = _handles().direct_from_model(pm, 9)
    mp = flat_map(pm, 9)
    assert mp.size == 48620
    check_sector(h, mp, pm.ns, 3, "nonsu2", seed=9)
    h.destroy()


def test_rows_longer_than_the_staged_chunk(gpu):
    """nonsu2, hybrid bath, two orbitals, Ns = 11, N = 11 on an on-the-fly handle (nothing stored): a chunk stages the
    tiles of 2048 / 6 = 341 bath words up and this sector has 512 of them, so every slab is staged in two parts (rows
    of up to C(11, 5) = 462 elements, 705 432 states)"""
    pm = flat_model("nonsu2", "hybrid", 2, 9, 13)
    assert pm.ns == 11
    h = _handles().direct_from_model(pm, 11)
    mp = flat_map(pm, 11)
    assert mp.size == math.comb(22, 11)
    check_sector(h, mp, 11, 2, "nonsu2", seed=21)
    h.destroy()


def test_several_vectors_equal_single_calls_bit_for_bit(gpu):
    import torch
    # superc Sz = 3: dim 45, nonsu2 N = 4: dim 495 -- the second vector starts at an odd element
    for mode, bath, nbath, sec, seed, dim in (("superc", "hybrid", 3, 3, 12, 45), ("nonsu2", "normal", 2, 4, 13, 495)):
        pm = flat_model(mode, bath, 2, nbath, seed)
        h = _handles().flat_from_model(pm, sec)
        assert h.dim == dim
        mp = flat_map(pm, sec)
        vs = np.stack([random_vector(h.dim, h.is_complex, 20 + k) for k in range(3)])
        vd = torch.from_numpy(vs).cuda()
        rho, n2 = h.imp_rdm_flat(vd.data_ptr(), 3)
        for k in range(3):
            rk, nk = h.imp_rdm_flat(vd[k].data_ptr())
            assert np.array_equal(rho[k], rk[0]) and n2[k] == nk[0]
            ref, n2r = ref_rdm_flat(mp, pm.ns, 2, vs[k])
            assert np.max(np.abs(rho[k] - ref)) <= 4 * h.dim * U * n2r
        h.destroy()


def test_vectors_at_odd_offsets(gpu):
    """8-byte aligned vectors, real (superc) and complex (nonsu2); the buffer around them is left alone"""
    import torch
    for mode, bath, nbath, sec, seed in (("superc", "hybrid", 3, 1, 12), ("nonsu2", "normal", 2, 5, 13)):
        pm = flat_model(mode, bath, 2, nbath, seed)
        h = _handles().flat_from_model(pm, sec)
        mp = flat_map(pm, sec)
        v = random_vector(h.dim, h.is_complex, 31)
        w = h.dim * (2 if h.is_complex else 1)
        buf = torch.zeros(w + 2, dtype=torch.float64, device="cuda")
        src = buf[1:1 + w]
        assert src.data_ptr() % 16 == 8
        src.copy_(torch.from_numpy(v.view(np.float64)))
        rho, n2 = h.imp_rdm_flat(src.data_ptr())
        ref, n2r = ref_rdm_flat(mp, pm.ns, 2, v)
        tol = 4 * h.dim * U * n2r
        assert np.max(np.abs(rho[0] - ref)) <= tol and abs(n2[0] - n2r) <= tol
        assert np.array_equal(rho[0], rho[0].conj().T)
        assert buf[0].item() == 0.0 and buf[-1].item() == 0.0
        assert np.array_equal(src.cpu().numpy().view(v.dtype), v)
        h.destroy()


def test_complex_vector_and_the_sign(gpu):
    """a complex vector whose rho has an imaginary part: rho^T in place of rho (a swapped conjugate) fails; and the
    restatement without the fermionic sign is far from the one with it, so a kernel that drops the sign fails"""
    pm = flat_model("nonsu2", "normal", 2, 2, 13)
    h = _handles().flat_from_model(pm, 6)
    assert h.is_complex
    mp = flat_map(pm, 6)
    v, rho = check_sector(h, mp, pm.ns, 2, "nonsu2", seed=43)
    ref, n2r = ref_rdm_flat(mp, pm.ns, 2, v)
    tol = 4 * h.dim * U * n2r
    assert np.max(np.abs(ref.imag)) > 1e3 * tol
    assert np.max(np.abs(rho.T - ref)) > 1e3 * tol
    nosign, _ = ref_rdm_flat(mp, pm.ns, 2, v, sign=False)
    assert np.max(np.abs(nosign - ref)) > 1e3 * tol
    assert np.max(np.abs(rho - nosign)) > 1e3 * tol and np.max(np.abs(rho - ref)) <= tol
    h.destroy()


def test_phonon_sector_traces_the_phonon_blocks(gpu):
    import torch
    ps = flat_model("superc", "hybrid", 2, 3, 12)
    mp = flat_map(ps, 0)
    ps.nph, ps.w0_ph, ps.a_ph, ps.g_ph = 3, 0.8, 0.0, np.diag((0.3, 0.5))
    h = _handles().flat_from_model(ps, 0)
    assert h.dim == 4 * 252
    v, rho = check_sector(h, mp, ps.ns, 2, "superc", seed=41, nblk=4)
    # the sum over the blocks, each taken as a vector of the electronic sector
    he = _handles().flat_from_model(flat_model("superc", "hybrid", 2, 3, 12), 0)
    assert he.is_complex == h.is_complex
    vd = torch.from_numpy(v).cuda()
    parts, _ = he.imp_rdm_flat(vd.data_ptr(), 4)
    n2 = float(np.vdot(v, v).real)
    assert np.max(np.abs(parts.sum(axis=0) - rho)) <= 2 * 4 * h.dim * U * n2
    he.destroy()
    h.destroy()


def _golden_ground_state(name, sec):
    """(om, fixture, handle, device eigenvector) of the lowest state of sector sec of a fixture directory"""
    import torch
    from edipack_amd import capi
    from oracle import oracle as O
    from tests.common import replica_golden_models
    from tests.test_oracle_golden import GOLD, REPLICA_DIRS, _from_dir, golden_models
    g = GOLD[name]
    if name in REPLICA_DIRS:
        om, pm = replica_golden_models(g["input"])
    else:
        inp, par = _from_dir(name)
        pm_par = {k: v for k, v in par.items() if k not in ("ed_hw_bath", "deltasc")}
        om, pm = golden_models(inp["ED_MODE"], inp["BATH_TYPE"], int(inp["NORB"]), int(inp["NBATH"]), pm_par)
    O.to_struct(om)
    h = _handles().flat_from_model(pm, sec)
    w = 2 if h.is_complex else 1
    e, nc, nmv = np.zeros(1), C.c_int(0), C.c_int(0)
    evec = torch.empty(h.dim * w, dtype=torch.float64, device="cuda")
    capi.check(capi.lib().edigpu_lanczos_eigh_multi(h._h, 1, 0, 1e-13, 300, None, capi.pd(e), C.c_void_p(evec.data_ptr()),
                                                    C.byref(nc), C.byref(nmv)), "edigpu_lanczos_eigh_multi")
    assert abs(e[0] - g["evals"][0]) < 1e-9     # the ground state of the fixture lies in this sector, alone
    return om, g, h, evec


def test_golden_magx_from_a_device_eigenvector(gpu):
    """dens, docc and magX of the reference's NORMAL_NONSU2 directory from rho of the ground state (sector N = 6), which
    never leaves the device: the sign and the basis order are the reference's, independent of the restatement"""
    from edipack_amd.observables import rdm_average, rdm_magx, rdm_occupations
    om, g, h, evec = _golden_ground_state("NORMAL_NONSU2", 6)
    rhos, n2 = h.imp_rdm_flat(evec.data_ptr())
    rho = rdm_average(rhos, n2)
    up, dw, docc = rdm_occupations(rho, om.norb)
    mx = rdm_magx(rho, om.norb)
    print(f"max |dens - check| = {np.max(np.abs(up + dw - np.array(g['dens']))):.3e} "
          f"|docc| {np.max(np.abs(docc - np.array(g['docc']))):.3e} |magX| {np.max(np.abs(mx - np.array(g['magX']))):.3e}")
    assert np.max(np.abs(up + dw - np.array(g["dens"]))) < 1e-8 and np.max(np.abs(docc - np.array(g["docc"]))) < 1e-8
    assert np.max(np.abs(np.array(g["magX"]))) > 1e-2 and np.max(np.abs(mx - np.array(g["magX"]))) < 1e-8
    h.destroy()


def test_golden_phisc_from_a_device_eigenvector(gpu):
    """dens, docc and phisc (the signed real part, tests/observables.py::phisc) of the reference's GENERAL_SUPERC
    directory from rho of the ground state (sector Sz = 0)"""
    from edipack_amd.observables import rdm_anomalous, rdm_average, rdm_occupations
    om, g, h, evec = _golden_ground_state("GENERAL_SUPERC", 0)
    rhos, n2 = h.imp_rdm_flat(evec.data_ptr())
    rho = rdm_average(rhos, n2)
    up, dw, docc = rdm_occupations(rho, om.norb)
    phi = rdm_anomalous(rho, om.norb).flatten(order="F")      # Fortran element order, as the fixture
    print(f"max |dens - check| = {np.max(np.abs(up + dw - np.array(g['dens']))):.3e} "
          f"|docc| {np.max(np.abs(docc - np.array(g['docc']))):.3e} |phisc| {np.max(np.abs(phi.real - np.array(g['phisc']))):.3e}")
    assert np.max(np.abs(up + dw - np.array(g["dens"]))) < 1e-8 and np.max(np.abs(docc - np.array(g["docc"]))) < 1e-8
    assert np.max(np.abs(np.array(g["phisc"]))) > 1e-2
    assert np.max(np.abs(phi.real - np.array(g["phisc"]))) < 1e-8 and np.max(np.abs(phi.imag)) < 1e-8
    h.destroy()


def test_refusals(gpu):
    import torch
    from edipack_amd import capi
    H = _handles()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")

    def refuses(h, match):
        with pytest.raises(capi.EdigpuError, match=match):
            h.imp_rdm_flat(buf.data_ptr())
        with pytest.raises(capi.EdigpuError, match=match):
            h.time_rdm_flat(buf.data_ptr(), 0, 1)
        h.destroy()

    _, pn = make_models("normal", "normal", 2, 2, seed=11)
    refuses(H.normal_from_model(pn, 3, 3), "edigpu_(imp|time)_rdm_flat: normal-mode sectors are not served here, use edigpu_imp_rdm")
    _, pj = make_jz_models(1)
    refuses(H.flat_jz_from_model(pj, 3, 1), "edigpu_(imp|time)_rdm_flat: Jz_basis sectors are not supported")
    refuses(H.direct_jz_from_model(pj, 3, 1), "edigpu_(imp|time)_rdm_flat: Jz_basis sectors are not supported")
    p5 = flat_model("nonsu2", "hybrid", 5, 1, 13)
    refuses(H.flat_from_model(p5, 2), "edigpu_(imp|time)_rdm_flat: Norb = 5 is not supported")
    ps = flat_model("superc", "hybrid", 2, 3, 12)
    refuses(H.flat_from_model(ps, 0, row_first=2, row_count=5), "edigpu_(imp|time)_rdm_flat: the handle must hold the whole sector")
    refuses(H.direct_from_model(ps, 0, row_first=2, row_count=5), "edigpu_(imp|time)_rdm_flat: the handle must hold the whole sector")
    assert math.isfinite(buf.sum().item())
