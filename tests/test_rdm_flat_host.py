"""CPU tests of the impurity reduced density matrix of superc / nonsu2 sectors (edigpu_imp_rdm_flat): the host tables and
the kernel's work list of csrc/host_rdm_flat.cpp through tests/host_rdm_flat.cpp against the numpy restatement of
tests/rdm_flat_cases.py, the refusal of maps without the structure, the same code as a stand-alone program under the
address and undefined-behaviour sanitizers, the helpers of edipack_amd/observables.py, and the error paths that need no
device."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from edipack_amd import capi
from edipack_amd.observables import rdm_anomalous, rdm_magx
from tests.rdm_flat_cases import MODE, SECTORS, U, blocks_mask, flat_map, flat_model, numpy_rdm_flat, random_vector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edipack_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "host_rdm_flat.cpp"), os.path.join(CSRC, "host_rdm_flat.cpp"),
           os.path.join(CSRC, "host_rdm.cpp")]
VP, L, I = C.c_void_p, C.c_int64, C.c_int


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_rdm_flat") / "host_rdm_flat.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", so] + SOURCES)
    lib = C.CDLL(so)
    lib.hrf_tables.argtypes = [VP, L, I, I, I, I, VP, C.c_char_p]
    lib.hrf_dense.argtypes = [VP, L, I, I, I, I, I, VP, I, I, I, VP, VP, C.c_char_p]
    return lib


def shim_dense(shim, mp, ns, norb, mode, q, v, nblk=1, which=0, target_wgs=2048):
    cplx = np.iscomplexobj(v)
    v = np.ascontiguousarray(v)
    D = 4 ** norb
    rho = np.full((D, D), np.nan, dtype=v.dtype)
    info, msg = np.zeros(5, np.int64), C.create_string_buffer(256)
    rc = shim.hrf_dense(mp.ctypes.data, mp.size, ns, norb, MODE[mode], q, nblk, v.ctypes.data, 2 if cplx else 1, which,
                        target_wgs, rho.ctypes.data, info.ctypes.data, msg)
    assert rc == 0, msg.value.decode()
    return rho, info


@pytest.mark.parametrize("mode,bath,norb,nbath,sec,seed", SECTORS)
@pytest.mark.parametrize("cplx", [False, True])
def test_host_reference_and_work_list_equal_the_restatement(built, shim, mode, bath, norb, nbath, sec, seed, cplx):
    """rdm_flat_host_reference (the kernel's specification) and the kernel's work list walked on the host with every
    index checked (rdm_flat_plan_emulate), at two device widths, against numpy within 4 dim u norm2; place gives an
    exactly Hermitian matrix with zeros outside the blocks."""
    pm = flat_model(mode, bath, norb, nbath, seed)
    mp = flat_map(pm, sec)
    v = random_vector(mp.size, cplx, seed=sec + norb + 40)
    ref = numpy_rdm_flat(mp, pm.ns, norb, v)
    tol = 4 * v.size * U * np.vdot(v, v).real
    outside = ~blocks_mask(mode, norb)
    info = np.zeros(3, np.int64)
    assert shim.hrf_tables(mp.ctypes.data, mp.size, pm.ns, norb, MODE[mode], sec, info.ctypes.data, C.create_string_buffer(256)) == 0
    assert info[1] == 2 * norb + 1 and info[2] == math.comb(2 * norb, norb)
    assert info[0] == sum(math.comb(2 * norb, c) * (math.comb(2 * norb, c) + 1) // 2 for c in range(2 * norb + 1))
    rho, _ = shim_dense(shim, mp, pm.ns, norb, mode, sec, v)
    assert np.max(np.abs(rho - ref)) <= tol and np.array_equal(rho, rho.conj().T) and np.count_nonzero(rho[outside]) == 0
    for wgs in (2048, 3):
        plan, info = shim_dense(shim, mp, pm.ns, norb, mode, sec, v, which=1, target_wgs=wgs)
        assert np.max(np.abs(plan - ref)) <= tol and np.array_equal(plan, plan.conj().T)
        assert np.count_nonzero(plan[outside]) == 0
        assert info[0] >= info[1] >= 1 and info[3] * 8 <= 150 * 1024
    if norb == 4:
        assert info[1] >= 2                     # the classes of four orbitals do not fit one workgroup's accumulators


def test_work_list_splits_slabs_chunks_and_phonon_blocks(built, shim):
    """a sector with more bath words up than one chunk stages: at two orbitals a chunk is 2048 / 6 = 341 bath words, and
    hybrid Norb = 2, Ns = 11 has 512 of them, so every popcount of Bdw has two panels; then three phonon blocks"""
    pm = flat_model("nonsu2", "hybrid", 2, 9, 13)
    assert pm.ns == 11
    mp = flat_map(pm, 11)
    assert mp.size == math.comb(22, 11)
    v = random_vector(mp.size, False, seed=5)
    ref = numpy_rdm_flat(mp, 11, 2, v)
    plan, info = shim_dense(shim, mp, 11, 2, "nonsu2", 11, v, which=1, target_wgs=2048)
    assert info[4] > 10 and info[0] > 8 * info[1]        # two chunks for each popcount of Bdw, many workgroups
    assert np.max(np.abs(plan - ref)) <= 4 * v.size * U * np.vdot(v, v).real
    ps = flat_model("superc", "hybrid", 2, 3, 12)
    mp = flat_map(ps, 0)
    v = random_vector(3 * mp.size, True, seed=6)
    ref = numpy_rdm_flat(mp, ps.ns, 2, v, nblk=3)
    assert np.allclose(ref, sum(numpy_rdm_flat(mp, ps.ns, 2, v.reshape(3, -1)[k]) for k in range(3)), atol=1e-12)
    for which in (0, 1):
        rho, _ = shim_dense(shim, mp, ps.ns, 2, "superc", 0, v, nblk=3, which=which, target_wgs=64)
        assert np.max(np.abs(rho - ref)) <= 4 * v.size * U * np.vdot(v, v).real


def test_maps_without_the_structure_are_refused(built, shim):
    pm = flat_model("nonsu2", "normal", 2, 2, 13)
    mp = flat_map(pm, 6)
    info, msg = np.zeros(3, np.int64), C.create_string_buffer(256)

    def tables(m, q=6, mode=2, norb=2):
        m = np.ascontiguousarray(m, np.int32)
        msg.value = b""
        return shim.hrf_tables(m.ctypes.data, m.size, pm.ns, norb, mode, q, info.ctypes.data, msg)

    assert tables(mp) == 0
    swapped = mp.copy()
    swapped[[100, 101]] = swapped[[101, 100]]
    assert tables(swapped) == 1 and msg.value
    assert tables(np.delete(mp, 300)) == 1 and msg.value
    assert tables(mp, q=5) == 1 and msg.value            # the map of another sector
    assert tables(mp, mode=1) == 1 and msg.value
    assert tables(mp, mode=0) == 1 and msg.value
    assert tables(mp, norb=5) == 1 and msg.value


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """host code only: the glue with its own main, built with -fsanitize=address,undefined and run as a program"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "host_rdm_flat_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DHRF_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe] + SOURCES)
    args = []
    for mode, bath, norb, nbath, sec, seed in SECTORS:
        args += [flat_model(mode, bath, norb, nbath, seed).ns, norb, MODE[mode], sec]
    args += [9, 3, 2, 9, 7, 2, 1, 0]
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("ok ") == len(args) // 4 and "FAIL" not in out.stdout


def test_anomalous_and_magx_against_their_definitions():
    """tr(rho O) on a pure state of the impurity space against <psi|O|psi> written out with explicit fermionic signs"""
    rng = np.random.default_rng(4)
    norb, D = 2, 16
    psi = rng.standard_normal(D) + 1j * rng.standard_normal(D)
    psi /= np.linalg.norm(psi)
    rho = np.outer(psi, psi.conj())

    def c(level, state):          # (sign, new state) or None
        if not (state >> level) & 1:
            return None
        return (-1.0) ** bin(state & ((1 << level) - 1)).count("1"), state ^ (1 << level)

    def cdag(level, state):
        if (state >> level) & 1:
            return None
        return (-1.0) ** bin(state & ((1 << level) - 1)).count("1"), state | (1 << level)

    phi, mx = rdm_anomalous(rho, norb), rdm_magx(rho, norb)
    assert phi.shape == (norb, norb) and mx.shape == (norb,)
    for a in range(norb):
        for b in range(norb):
            s = 0.0
            for i in range(D):    # <c_{b up} c_{a dw}>
                r1 = c(norb + a, i)
                r2 = c(b, r1[1]) if r1 else None
                if r2:
                    s += np.conj(psi[r2[1]]) * r1[0] * r2[0] * psi[i]
            assert abs(phi[a, b] - s) < 1e-14
        s = 0.0
        for i in range(D):        # <c+_{a up} c_{a dw}>
            r1 = c(norb + a, i)
            r2 = cdag(a, r1[1]) if r1 else None
            if r2:
                s += np.conj(psi[r2[1]]) * r1[0] * r2[0] * psi[i]
        assert abs(mx[a] - 2 * s.real) < 1e-14
    with pytest.raises(ValueError):
        rdm_anomalous(rho, 3)
    with pytest.raises(ValueError):
        rdm_magx(rho, 1)


def test_null_arguments_are_refused_with_a_message(built):
    lib = capi.lib()
    buf = np.zeros(16)
    assert lib.edigpu_imp_rdm_flat(None, None, 1, capi.pd(buf), None) != 0
    assert "edigpu_imp_rdm_flat" in capi.last_error() and "NULL" in capi.last_error()
    assert lib.edigpu_time_rdm_flat(None, None, 0, 1, capi.pd(buf)) != 0
    assert "edigpu_time_rdm_flat" in capi.last_error()
