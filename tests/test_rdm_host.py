"""CPU tests of the impurity reduced density matrix (edigpu_imp_rdm): the numpy restatement of imp_rdm_normal on the
reference's rdm.check fixture, the host tables and the kernel's work list of csrc/host_rdm.cpp through tests/host_rdm.cpp,
the formulas of edipack_amd/observables.py, and the error paths that need no device."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from edipack_amd import capi
from edipack_amd.observables import entanglement_entropy, rdm_average, rdm_occupations
from tests.common import make_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, L, I = C.c_void_p, C.c_int64, C.c_int

# bath, norb, nbath, sector: the shapes the host reference, the work list and the kernel are all checked on
SECTORS = [
    ("normal", 2, 2, (3, 3)),   # the fixture's sector
    ("normal", 2, 2, (1, 4)),   # short rows
    ("normal", 2, 2, (0, 0)),   # dim 1
    ("normal", 2, 2, (6, 6)),   # dim 1
    ("normal", 1, 4, (2, 3)),   # all runs of length 1: rho is diagonal
    ("normal", 3, 3, (6, 1)),   # long rows
    ("hybrid", 4, 3, (3, 4)),   # runs of up to 6
    ("hybrid", 5, 3, (4, 4)),   # runs of 10, 100 x 100 blocks, D = 1024
]


def _popcount(x):
    return np.array([bin(int(k)).count("1") for k in np.ravel(x)]).reshape(np.shape(x))


def numpy_rdm(mu, md, norb, v, nblk=1, dtype=None):
    """imp_rdm_normal (ED_RDM_NORMAL.f90:146-209) restated: the elements of v[nblk, DimDw, DimUp] grouped by their bath
    words (Bup, Bdw) (and phonon block) into the columns of A[io, tile], io = Iup + 2^norb Idw; then rho = A A^H.  A is
    built class by class (impurity particle numbers (ku, kd): its rows outside a class are zero), which assumes nothing
    about the order of the maps.  dtype: np.longdouble / np.clongdouble for the extended-precision reference."""
    mu, md = np.asarray(mu, np.int64), np.asarray(md, np.int64)
    mask, D = (1 << norb) - 1, 4 ** norb
    V = np.asarray(v).reshape(nblk, md.size, mu.size)
    if dtype is not None:
        V = V.astype(dtype)
    iu, bu, idw, bd = mu & mask, mu >> norb, md & mask, md >> norb
    ku, kd = _popcount(iu), _popcount(idw)
    rho = np.zeros((D, D), V.dtype)
    for a in np.unique(ku):
        for b in np.unique(kd):
            cu, cd = np.nonzero(ku == a)[0], np.nonzero(kd == b)[0]
            io = (idw[cd][:, None] << norb) + iu[cu][None, :]
            rows, r = np.unique(io, return_inverse=True)
            r = r.reshape(io.shape)
            tu, td = np.unique(bu[cu], return_inverse=True)[1], np.unique(bd[cd], return_inverse=True)[1]
            nt = (td.max() + 1) * (tu.max() + 1)
            t = td[:, None] * (tu.max() + 1) + tu[None, :]
            A = np.zeros((rows.size, nblk * nt), V.dtype)
            for k in range(nblk):
                A[r, k * nt + t] = V[k][np.ix_(cd, cu)]
            rho[np.ix_(rows, rows)] = A @ A.conj().T
    return rho


def sector_maps(pm, sec):
    from edipack_amd.hamiltonian import sector_map
    return sector_map(pm, sec[0], sec[1], 0), sector_map(pm, sec[0], sec[1], 1)


def random_vector(dim, cplx, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(dim)
    return v + 1j * rng.standard_normal(dim) if cplx else v


def _fixture_rho():
    from tests import observables as ob
    from tests.test_oracle_golden import _golden_model
    om, g = _golden_model("NORMAL_NORMAL")
    _, states = ob.ground_manifold(om)
    assert len(states) == 1 and tuple(states[0][0]) == (3, 3)
    sec, h, v = states[0]
    rho = numpy_rdm(h.mapup, h.mapdw, om.norb, v) / np.vdot(v, v).real
    gold = np.array(g["rdm"]).reshape(16, 16, 2)
    return om, g, rho, gold[..., 0] + 1j * gold[..., 1]


def test_numpy_restatement_reproduces_reference_fixture():
    """rdm.check of NORMAL_NORMAL from the oracle's dense ground state, to the tolerance tests/test_oracle_golden.py uses
    for that directory"""
    _, _, rho, gold = _fixture_rho()
    print(f"max |rho - rdm.check| = {np.max(np.abs(rho - gold)):.3e}")
    assert np.max(np.abs(rho - gold)) < 1e-9
    assert abs(np.trace(rho) - 1.0) < 1e-12


def test_rdm_occupations_reproduce_dens_and_docc_of_the_fixture():
    om, g, rho, _ = _fixture_rho()
    up, dw, docc = rdm_occupations(rho, om.norb)
    assert np.max(np.abs(up + dw - np.array(g["dens"]))) < 1e-9
    assert np.max(np.abs(docc - np.array(g["docc"]))) < 1e-9


def test_observables_of_a_density_matrix_against_their_definitions():
    rng = np.random.default_rng(3)
    norb, D = 2, 16
    xs = rng.standard_normal((3, D, 5)) + 1j * rng.standard_normal((3, D, 5))
    rhos = np.stack([x @ x.conj().T for x in xs])
    n2 = np.array([np.trace(r).real for r in rhos])
    # average: equal weights, Boltzmann weights (normalised inside), a single matrix
    avg = rdm_average(rhos, n2)
    assert np.allclose(avg, sum(r / n for r, n in zip(rhos, n2)) / 3, atol=1e-14) and abs(np.trace(avg) - 1) < 1e-13
    w = np.array([3.0, 1.0, 0.5])
    assert np.allclose(rdm_average(rhos, n2, w), sum(wk * r / n for wk, r, n in zip(w / w.sum(), rhos, n2)), atol=1e-14)
    assert np.allclose(rdm_average(rhos[0], n2[0]), rhos[0] / n2[0], atol=1e-15)
    with pytest.raises(ValueError):
        rdm_average(rhos, n2[:2])
    # occupations: bit a of io is orbital a up, bit norb + a is orbital a down
    p = np.real(np.diag(avg))
    up, dw, docc = rdm_occupations(avg, norb)
    for a in range(norb):
        assert abs(up[a] - sum(p[io] for io in range(D) if (io >> a) & 1)) < 1e-14
        assert abs(dw[a] - sum(p[io] for io in range(D) if (io >> (norb + a)) & 1)) < 1e-14
        assert abs(docc[a] - sum(p[io] for io in range(D) if (io >> a) & 1 and (io >> (norb + a)) & 1)) < 1e-14
    with pytest.raises(ValueError):
        rdm_occupations(avg, 3)
    # entropy: -sum p ln p; a pure state has none, the maximally mixed state ln D, zero eigenvalues are skipped
    ev = np.linalg.eigvalsh(avg)
    assert abs(entanglement_entropy(avg) - float(-np.sum(ev[ev > 0] * np.log(ev[ev > 0])))) < 1e-12
    x = xs[0][:, :1]
    assert abs(entanglement_entropy(x @ x.conj().T / np.vdot(x, x).real)) < 1e-12
    assert abs(entanglement_entropy(np.eye(D) / D) - math.log(D)) < 1e-12
    assert abs(entanglement_entropy(np.diag([0.5, 0.5, 0.0, 0.0])) - math.log(2)) < 1e-14


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_rdm") / "host_rdm.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", so,
                           os.path.join(ROOT, "tests", "host_rdm.cpp"), os.path.join(csrc, "host_rdm.cpp")])
    lib = C.CDLL(so)
    lib.hr_ranks.argtypes = [I, VP, VP, VP]
    lib.hr_runs.argtypes = [VP, L, I, VP, VP, C.c_char_p]
    lib.hr_runs.restype = L
    lib.hr_ntri.argtypes = [I]
    lib.hr_ntri.restype = L
    lib.hr_dense.argtypes = [VP, L, VP, L, I, I, VP, I, I, I, VP, VP, C.c_char_p]
    return lib


def shim_dense(shim, mu, md, norb, v, nblk=1, which=0, target_wgs=2048):
    cplx = np.iscomplexobj(v)
    v = np.ascontiguousarray(v)
    D = 4 ** norb
    rho = np.full((D, D), np.nan, dtype=v.dtype)
    info, msg = np.zeros(4, np.int64), C.create_string_buffer(256)
    rc = shim.hr_dense(mu.ctypes.data, mu.size, md.ctypes.data, md.size, norb, nblk, v.ctypes.data, 2 if cplx else 1, which,
                       target_wgs, rho.ctypes.data, info.ctypes.data, msg)
    assert rc == 0, msg.value.decode()
    return rho, info


@pytest.mark.parametrize("norb", [1, 2, 3, 4, 5])
def test_rank_tables_and_packed_size(shim, norb):
    nk, pat_of, rank_of = np.zeros(6, np.int32), np.zeros((6, 10), np.uint8), np.zeros(32, np.uint8)
    shim.hr_ranks(norb, nk.ctypes.data, pat_of.ctypes.data, rank_of.ctypes.data)
    for k in range(norb + 1):
        pats = [p for p in range(2 ** norb) if bin(p).count("1") == k]
        assert nk[k] == math.comb(norb, k) == len(pats)
        assert list(pat_of[k, :nk[k]]) == pats and all(rank_of[p] == r for r, p in enumerate(pats))
    # the upper triangles of the blocks: (nonzero entries C(2 norb, norb)^2 + the diagonal 4^norb) / 2
    assert shim.hr_ntri(norb) == (math.comb(2 * norb, norb) ** 2 + 4 ** norb) // 2


@pytest.mark.parametrize("bath,norb,nbath,sec", SECTORS)
def test_runs_cover_the_maps(built, shim, bath, norb, nbath, sec):
    _, pm = make_models("normal", bath, norb, nbath, seed=11)
    mask = 2 ** norb - 1
    for mp in sector_maps(pm, sec):
        start, k, msg = np.zeros(mp.size + 1, np.int32), np.zeros(mp.size, np.uint8), C.create_string_buffer(256)
        n = shim.hr_runs(mp.ctypes.data, mp.size, norb, start.ctypes.data, k.ctypes.data, msg)
        assert n > 0, msg.value.decode()
        assert start[0] == 0 and start[n] == mp.size and np.all(np.diff(start[:n + 1]) > 0)
        for j in range(n):
            run = mp[start[j]:start[j + 1]]
            assert run.size == math.comb(norb, int(k[j]))
            assert np.all(run >> norb == run[0] >> norb) and np.all(_popcount(run & mask) == k[j])
            assert np.all(np.diff(run & mask) > 0)
        bath_words = mp[start[:n]] >> norb
        assert np.all(np.diff(bath_words) > 0)          # one run per bath word


def test_runs_refuse_a_map_without_the_structure(shim):
    msg = C.create_string_buffer(256)
    start, k = np.zeros(8, np.int32), np.zeros(8, np.uint8)
    for bad in ([1, 2, 4, 6], [2, 1], [1, 5, 9, 9]):    # a run that misses a pattern, descending, repeated
        mp = np.array(bad, np.int32)
        assert shim.hr_runs(mp.ctypes.data, mp.size, 2, start.ctypes.data, k.ctypes.data, msg) == -1
        assert msg.value


@pytest.mark.parametrize("bath,norb,nbath,sec", SECTORS)
@pytest.mark.parametrize("cplx", [False, True])
def test_host_reference_and_work_list_equal_the_restatement(built, shim, bath, norb, nbath, sec, cplx):
    """rdm_host_reference (the kernel's specification) and the kernel's work list walked on the host with every index
    checked (rdm_plan_emulate), at two device widths, against numpy: sums of dim products, |x_p x_q| summing to at most
    norm2, so 4 dim u norm2 covers any order (the bound of tests/test_gpu_rdm.py)."""
    _, pm = make_models("normal", bath, norb, nbath, seed=11)
    mu, md = sector_maps(pm, sec)
    v = random_vector(mu.size * md.size, cplx, seed=sum(sec) + norb)
    ref = numpy_rdm(mu, md, norb, v)
    tol = 4 * v.size * 2.0 ** -53 * np.vdot(v, v).real
    rho, _ = shim_dense(shim, mu, md, norb, v)
    assert np.max(np.abs(rho - ref)) <= tol and np.array_equal(rho, rho.conj().T)
    if norb == 1:
        assert np.count_nonzero(rho - np.diag(np.diag(rho))) == 0
    for wgs in (2048, 3):
        plan, info = shim_dense(shim, mu, md, norb, v, which=1, target_wgs=wgs)
        assert np.max(np.abs(plan - ref)) <= tol and np.array_equal(plan, plan.conj().T)
        assert info[0] >= info[1] >= 1 and info[3] * 8 <= 150 * 1024


def test_work_list_splits_rows_chunks_and_phonon_blocks(built, shim):
    """a sector wide enough for several chunks and several workgroups per chunk; three phonon blocks"""
    _, pm = make_models("normal", "normal", 3, 3, seed=11)
    mu, md = sector_maps(pm, (6, 5))                     # 924 columns (two chunks of 682) x 792 rows
    v = random_vector(mu.size * md.size, False, seed=5)
    ref = numpy_rdm(mu, md, 3, v)
    plan, info = shim_dense(shim, mu, md, 3, v, which=1, target_wgs=2048)
    assert info[0] > 8 * info[1]
    assert np.max(np.abs(plan - ref)) <= 4 * v.size * 2.0 ** -53 * np.vdot(v, v).real
    _, p2 = make_models("normal", "normal", 2, 2, seed=11)
    mu, md = sector_maps(p2, (3, 3))
    v = random_vector(3 * mu.size * md.size, True, seed=6)
    ref = numpy_rdm(mu, md, 2, v, nblk=3)
    assert np.allclose(ref, sum(numpy_rdm(mu, md, 2, v.reshape(3, -1)[k]) for k in range(3)), atol=1e-12)
    for which in (0, 1):
        rho, _ = shim_dense(shim, mu, md, 2, v, nblk=3, which=which, target_wgs=64)
        assert np.max(np.abs(rho - ref)) <= 4 * v.size * 2.0 ** -53 * np.vdot(v, v).real


def test_null_arguments_are_refused_with_a_message(built):
    lib = capi.lib()
    buf = np.zeros(16)
    assert lib.edigpu_imp_rdm(None, None, 1, capi.pd(buf), None) != 0
    assert "edigpu_imp_rdm" in capi.last_error() and "NULL" in capi.last_error()
    assert lib.edigpu_time_rdm(None, None, 0, 1, capi.pd(buf)) != 0
    assert "edigpu_time_rdm" in capi.last_error()
