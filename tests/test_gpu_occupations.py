"""GPU tests of the occupation operators on device vectors: edigpu_apply_occ (apply_op_N / apply_op_Sz seeds) and
edigpu_occ_moments (the sums behind dens, docc, magz, sz2, n2, s2tot).

References are numpy on the host from the sector maps, summed in extended precision.  Tolerances are derived, not
measured: a moment is a sum of dim non-negative terms |v_i|^2 n_x n_y <= |v_i|^2, each rounded once when squared, so ANY
summation order stays within (dim + 1) u norm2 of the exact value, u = 2^-53; the tests allow 2 dim u norm2.
The N_a and Sz_a weights (0, 1, 2, +-0.5) and their sums are exact in binary, so those products must be bit-equal."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.common import make_jz_models, make_models

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _handles():
    from edipack_amd.hamiltonian import SectorHamiltonian
    return SectorHamiltonian


def normal_bits(pm, nup, ndw, nblk=1):
    """nu, nd [norb, dim * nblk] of the vector layout i = iup + idw DimUp (+ iph dim_el)"""
    from edipack_amd.hamiltonian import sector_map
    mu, md = sector_map(pm, nup, ndw, 0), sector_map(pm, nup, ndw, 1)
    nu = np.array([np.tile((mu >> a) & 1, md.size * nblk) for a in range(pm.norb)])
    nd = np.array([np.tile(np.repeat((md >> a) & 1, mu.size), nblk) for a in range(pm.norb)])
    return nu, nd


def flat_bits(pm, mp, nblk=1):
    ns = pm.ns
    nu = np.array([np.tile((mp >> a) & 1, nblk) for a in range(pm.norb)])
    nd = np.array([np.tile((mp >> (ns + a)) & 1, nblk) for a in range(pm.norb)])
    return nu, nd


def ref_moments(nu, nd, v):
    """(M, norm2) in extended precision"""
    p = v.real.astype(np.longdouble) ** 2 + v.imag.astype(np.longdouble) ** 2
    bits = np.concatenate([nu, nd], axis=0).astype(np.longdouble)
    return ((bits * p[None, :]) @ bits.T).astype(np.float64), float(p.sum())


def random_vector(dim, cplx, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(dim)
    return v + 1j * rng.standard_normal(dim) if cplx else v


def check_sector(h, nu, nd, seed, inplace=False):
    """every assertion of this file that needs one handle and its occupations"""
    import torch
    norb, dim = nu.shape[0], nu.shape[1]
    assert h.dim == dim and h.norb == norb
    v = random_vector(dim, h.is_complex, seed)
    vd = torch.from_numpy(v).cuda()
    # ---- moments: tolerance, symmetry, determinism
    M, n2 = h.occ_moments(vd.data_ptr())
    Mr, n2r = ref_moments(nu, nd, v)
    tol = 2 * dim * U * n2r
    print(f"occ_moments dim={dim} max|dM|={np.max(np.abs(M[0] - Mr)):.3e} |dnorm2|={abs(n2[0] - n2r):.3e} tol={tol:.3e}")
    assert M.shape == (1, 2 * norb, 2 * norb)
    assert np.max(np.abs(M[0] - Mr)) <= tol and abs(n2[0] - n2r) <= tol
    assert np.array_equal(M[0], M[0].T)
    M2, n22 = h.occ_moments(vd.data_ptr())
    assert np.array_equal(M, M2) and np.array_equal(n2, n22)
    # ---- apply: N_a and Sz_a bit-equal, the source untouched out of place
    st = torch.cuda.current_stream().cuda_stream
    for a in range(norb):
        out = torch.full_like(vd, 7.0)
        h.apply_n(vd.data_ptr(), out.data_ptr(), a, st)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), (nu[a] + nd[a]).astype(np.float64) * v)
        h.apply_sz(vd.data_ptr(), out.data_ptr(), a, st)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ((nu[a] - nd[a]) * 0.5) * v)
    assert np.array_equal(vd.cpu().numpy(), v)
    # ---- random weights: two rounded table sums, their sum, the product: 4 u sum|w| |v_i| covers them
    rng = np.random.default_rng(seed + 1)
    wu, wd = rng.standard_normal(norb), rng.standard_normal(norb)
    exact = (wu.astype(np.longdouble) @ nu + wd.astype(np.longdouble) @ nd) * v
    dst = vd.clone() if inplace else torch.empty_like(vd)
    h.apply_occ(dst.data_ptr() if inplace else vd.data_ptr(), dst.data_ptr(), wu, wd, st)
    torch.cuda.synchronize()
    bound = 4 * U * (np.abs(wu).sum() + np.abs(wd).sum()) * np.abs(v)
    assert np.all(np.abs(dst.cpu().numpy() - exact) <= bound)
    if not inplace:
        assert np.array_equal(vd.cpu().numpy(), v)


NORMAL_CASES = [
    # bath, norb, nbath, (nup, ndw), in place
    ("normal", 2, 2, (3, 3), False),   # 20 x 20
    ("normal", 2, 2, (1, 4), True),    # DimUp 6 x DimDw 15: rows shorter than a wave
    ("normal", 2, 2, (0, 0), False),   # dim 1, nothing occupied
    ("normal", 2, 2, (6, 6), False),   # dim 1, everything occupied
    ("normal", 2, 2, (5, 0), False),
    ("normal", 2, 2, (2, 2), False),   # 15 x 15: odd dimension
    ("normal", 3, 3, (6, 1), False),   # 924 x 12: long rows
    ("normal", 3, 3, (1, 6), False),   # 12 x 924: many short rows
    ("normal", 3, 3, (6, 6), False),   # 924^2: every workgroup walks several runs, rows split between workgroups
    ("hybrid", 5, 3, (4, 4), False),   # 70 x 70, five orbitals: the largest tables (32 bins, 56 sums)
]


@pytest.mark.parametrize("bath,norb,nbath,sec,inplace", NORMAL_CASES)
def test_normal_sectors(gpu, bath, norb, nbath, sec, inplace):
    _, pm = make_models("normal", bath, norb, nbath, seed=11)
    h = _handles().normal_from_model(pm, *sec)
    check_sector(h, *normal_bits(pm, *sec), seed=sum(sec) + 3, inplace=inplace)
    h.destroy()


def test_several_vectors_equal_single_calls_bit_for_bit(gpu):
    import torch
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    for sec in ((3, 3), (2, 2)):     # (2, 2): dim 225, the second vector starts at an odd element
        h = _handles().normal_from_model(pm, *sec)
        vs = np.stack([random_vector(h.dim, False, 20 + k) for k in range(3)])
        vd = torch.from_numpy(vs).cuda()
        M, n2 = h.occ_moments(vd.data_ptr(), 3)
        nu, nd = normal_bits(pm, *sec)
        for k in range(3):
            Mk, nk = h.occ_moments(vd[k].data_ptr())
            assert np.array_equal(M[k], Mk[0]) and n2[k] == nk[0]
            Mr, n2r = ref_moments(nu, nd, vs[k])
            assert np.max(np.abs(M[k] - Mr)) <= 2 * h.dim * U * n2r
        h.destroy()


def test_vectors_at_odd_offsets(gpu):
    """8-byte aligned vectors take the kernels' scalar paths: real and complex, apply and moments"""
    import torch
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    st = torch.cuda.current_stream().cuda_stream
    for cplx in (False, True):
        h = _handles().normal_cmplx_from_model(pm, 3, 2) if cplx else _handles().normal_from_model(pm, 3, 2)
        nu, nd = normal_bits(pm, 3, 2)
        v = random_vector(h.dim, cplx, 31)
        w = h.dim * (2 if cplx else 1)
        buf = torch.zeros(2 * w + 2, dtype=torch.float64, device="cuda")
        src, dst = buf[1:1 + w], buf[w + 1:2 * w + 1]
        assert src.data_ptr() % 16 == 8
        src.copy_(torch.from_numpy(v.view(np.float64)))
        M, n2 = h.occ_moments(src.data_ptr())
        Mr, n2r = ref_moments(nu, nd, v)
        assert np.max(np.abs(M[0] - Mr)) <= 2 * h.dim * U * n2r and abs(n2[0] - n2r) <= 2 * h.dim * U * n2r
        h.apply_n(src.data_ptr(), dst.data_ptr(), 1, st)
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy().view(v.dtype), (nu[1] + nd[1]).astype(np.float64) * v)
        assert buf[0].item() == 0.0 and buf[-1].item() == 0.0
        h.destroy()


def test_phonon_sector_sums_over_the_phonon_blocks(gpu):
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = 3, 0.8, 0.0, np.diag((0.3, 0.5))
    h = _handles().normal_from_model(pm, 3, 3)
    assert h.dim == 4 * 400
    check_sector(h, *normal_bits(pm, 3, 3, nblk=4), seed=41)
    h.destroy()


def test_complex_normal_sector(gpu):
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    h = _handles().normal_cmplx_from_model(pm, 3, 2)
    assert h.is_complex
    check_sector(h, *normal_bits(pm, 3, 2), seed=43)
    h.destroy()


@pytest.mark.parametrize("form", ["stored", "direct"])
def test_flat_sectors(gpu, form):
    from edipack_amd.hamiltonian import sector_map, sector_map_jz
    H = _handles()
    _, ps = make_models("superc", "hybrid", 2, 3, seed=12)
    build = H.flat_from_model if form == "stored" else H.direct_from_model
    for sz in range(-ps.ns, ps.ns + 1):          # every Sz, +-Ns have dim 1
        h = build(ps, sz)
        check_sector(h, *flat_bits(ps, sector_map(ps, sz)), seed=50 + sz, inplace=(sz == 1))
        h.destroy()
    _, pn = make_models("nonsu2", "normal", 1, 4, seed=13)
    h = build(pn, 5)
    assert h.dim == 252
    check_sector(h, *flat_bits(pn, sector_map(pn, 5)), seed=61)
    h.destroy()
    _, pj = make_jz_models(1)
    hj = (H.flat_jz_from_model if form == "stored" else H.direct_jz_from_model)(pj, 3, 1)
    check_sector(hj, *flat_bits(pj, sector_map_jz(pj, 3, 1)), seed=62)
    hj.destroy()


@pytest.mark.parametrize("form", ["stored", "direct"])
def test_flat_phonon_sector(gpu, form):
    from edipack_amd.hamiltonian import sector_map
    H = _handles()
    _, ps = make_models("superc", "hybrid", 2, 3, seed=12)
    ps.nph, ps.w0_ph, ps.a_ph, ps.g_ph = 2, 0.8, 0.0, np.diag((0.3, 0.5))
    h = (H.flat_from_model if form == "stored" else H.direct_from_model)(ps, 0)
    mp = sector_map(ps, 0)
    assert h.dim == 3 * mp.size
    check_sector(h, *flat_bits(ps, mp, nblk=3), seed=63)
    h.destroy()


def test_chi_spin_chain_without_a_host_copy(gpu):
    """eigenvector -> Sz_a seed -> tridiagonalisation, all on the device (ED_CHI_SPIN.f90:121-170)"""
    import torch
    from edipack_amd import capi
    from edipack_amd.observables import from_moments
    from oracle import oracle as O
    om, pm = make_models("normal", "normal", 2, 2, seed=11)
    h = _handles().normal_from_model(pm, 3, 3)
    dim, nl = h.dim, 20
    evec = torch.empty(dim, dtype=torch.float64, device="cuda")
    ev, nc, nmv = np.zeros(1), C.c_int(0), C.c_int(0)
    capi.check(capi.lib().edigpu_lanczos_eigh_multi(h._h, 1, 0, 1e-13, 300, None, capi.pd(ev), C.c_void_p(evec.data_ptr()),
                                                    C.byref(nc), C.byref(nmv)), "edigpu_lanczos_eigh_multi")
    seed = torch.empty_like(evec)
    h.apply_sz(evec.data_ptr(), seed.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    al, bl, _, norm2 = h.lanczos_tridiag_dev(seed.data_ptr(), nl)
    M, vn2 = h.occ_moments(evec.data_ptr())
    sz2_00 = from_moments(M[0], 2).sz2[0, 0]            # not normalised, as the seed is not
    # sz2[0,0] = (U00 + D00 - 2 X00) / 4: four moment errors / 4, plus the recurrence's own sum of dim squares of a
    # vector of norm <= 1/2: together under the bound of one moment
    print(f"norm2={norm2!r} sz2[0,0]={sz2_00!r} diff={abs(norm2 - sz2_00):.3e}")
    assert abs(norm2 - sz2_00) <= 2 * dim * U * vn2[0]
    # for checking only: the vector on the host
    x = evec.cpu().numpy()
    nu, nd = normal_bits(pm, 3, 3)
    s = 0.5 * (nu[0] - nd[0]) * x
    assert np.array_equal(seed.cpu().numpy(), s)
    hd = O.HNormal(om, 3, 3).dense()
    assert abs(al[0] - (s @ hd @ s) / (s @ s)) < 1e-10
    a2, b2, _ = h.lanczos_tridiag(s, nl)
    assert np.max(np.abs(al - a2)) <= 1e-12 * np.max(np.abs(a2)) and np.max(np.abs(bl - b2)) <= 1e-12 * np.max(np.abs(b2))
    h.destroy()


@pytest.mark.parametrize("name", ["NORMAL_NORMAL", "REPLICA_NORMAL", "GENERAL_SUPERC", "NORMAL_NONSU2"])
def test_golden_observables_from_device_vectors(gpu, name):
    """dens, docc, imp[0], doubles[0:2] of the reference's fixtures from occ_moments of eigenvectors that never leave the
    device (the directories without a near-degenerate ground state, at the tolerance
    test_golden_observables_from_gpu_eigenvectors uses for them)."""
    import torch
    from edipack_amd import capi
    from edipack_amd.observables import from_moments
    from oracle import oracle as O
    from tests.common import replica_golden_models
    from tests.test_oracle_golden import GOLD, REPLICA_DIRS, _from_dir, golden_models
    H = _handles()
    g = GOLD[name]
    if name in REPLICA_DIRS:
        om, pm = replica_golden_models(g["input"])
    else:
        inp, par = _from_dir(name)
        pm_par = {k: v for k, v in par.items() if k not in ("ed_hw_bath", "deltasc")}
        om, pm = golden_models(inp["ED_MODE"], inp["BATH_TYPE"], int(inp["NORB"]), int(inp["NBATH"]), pm_par)
    O.to_struct(om)
    found = []   # (energies, device vectors [k, dim], handle)
    for sec in O.sectors(om):
        h = H.normal_from_model(pm, *sec) if om.ed_mode == "normal" else H.flat_from_model(pm, sec)
        if h.dim == 0:
            h.destroy()
            continue
        w = 2 if h.is_complex else 1
        if h.dim <= 8:   # the reference diagonalises small sectors densely: columns of H from H*v, vectors uploaded
            eye = np.eye(h.dim, dtype=h.dtype)
            e, x = np.linalg.eigh(np.stack([h.apply(eye[:, k].copy()) for k in range(h.dim)], axis=1))
            vecs = torch.from_numpy(np.ascontiguousarray(x.T).view(np.float64)).cuda()
        else:
            k = min(4, h.dim)
            e, nc, nmv = np.zeros(k), C.c_int(0), C.c_int(0)
            vecs = torch.empty((k, h.dim * w), dtype=torch.float64, device="cuda")
            capi.check(capi.lib().edigpu_lanczos_eigh_multi(h._h, k, 0, 1e-13, 300, None, capi.pd(e),
                                                            C.c_void_p(vecs.data_ptr()), C.byref(nc), C.byref(nmv)),
                       "edigpu_lanczos_eigh_multi")
        found.append((e, vecs, h))
    e0 = min(e[0] for e, _, _ in found)
    assert abs(e0 - g["evals"][0]) < 1e-9
    Ms, norms = [], []
    for e, vecs, h in found:
        for k in range(len(e)):
            if e[k] - e0 <= 1e-9:
                M, n2 = h.occ_moments(vecs[k].data_ptr())
                Ms.append(M[0])
                norms.append(n2[0])
        h.destroy()
    o = from_moments(np.stack(Ms), om.norb, norm2=norms)
    tol = 1e-8
    assert np.max(np.abs(o.dens - np.array(g["dens"]))) < tol and np.max(np.abs(o.docc - np.array(g["docc"]))) < tol
    assert abs(o.s2tot - g["imp"][0]) < tol
    assert abs(o.dust - g["doubles"][0]) < tol and abs(o.dund - g["doubles"][1]) < tol


def test_refusals(gpu):
    import torch
    from edipack_amd import capi
    from oracle import oracle as O
    H = _handles()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    w = np.ones(2)

    def both_refuse(h, match):
        with pytest.raises(capi.EdigpuError, match=match):
            h.apply_occ(buf.data_ptr(), buf.data_ptr(), w, w)
        with pytest.raises(capi.EdigpuError, match=match):
            h.occ_moments(buf.data_ptr())
        h.destroy()

    om, pm = make_models("normal", "normal", 2, 2, seed=11, jxp=0.0)
    hl = np.zeros_like(om.hloc)
    for a in range(2):
        hl[0, 0, a, a] = om.hloc[0, 0, a, a].real
    pm.hloc = hl                                             # what ed_total_ud=F requires
    both_refuse(H.orbs_from_model(pm, (2, 1), (1, 2)), "ed_total_ud=F sectors are not supported")
    ho = O.HNormal(om, 3, 3)
    both_refuse(H.normal_from_arrays(ho.dimup, ho.dimdw, ho.hd, ho.up, ho.dw, ho.nd), "must be built from a model")
    _, ps = make_models("superc", "hybrid", 2, 3, seed=12)
    both_refuse(H.flat_from_model(ps, 0, row_first=1, row_count=10), "must hold the whole sector")
    _, pn = make_models("normal", "normal", 2, 2, seed=11)
    both_refuse(H.normal_from_model(pn, 3, 3, dw_first=2, dw_count=5), "must hold the whole sector")
    assert math.isfinite(buf.sum().item())
