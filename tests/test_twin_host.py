"""CPU tests of the host side of the ED_TWIN=T reorder (csrc/host_twin.cpp through tests/host_twin.cpp, g++, no HIP): the
order table against a numpy restatement of twin_sector_order written from the Fortran (ED_SECTOR.f90:1747-1816: flip
every state of the sector map -- superc swaps the two Ns-bit halves, nonsu2 complements the 2 Ns bits --, then argsort),
the twin of every sector of the three modes (get_twin_sector, :1824-1843) through the host function and through
edigpu_twin_sector, the per-orbital form, and the same builder as a stand-alone program under ASan + UBSan."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from edipack_amd.hamiltonian import sector_map, twin_sector
from tests.common import make_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, I = C.c_void_p, C.c_int
NORMAL, SUPERC, NONSU2 = 0, 1, 2


def flip_states(mode, ns, states):
    """flip_state_other on an array of states iup + idw 2^Ns"""
    s = np.asarray(states, np.int64)
    low = (1 << ns) - 1
    if mode == SUPERC:
        return ((s & low) << ns) | (s >> ns)
    return ~s & ((1 << (2 * ns)) - 1)


def twin_order_ref(mode, ns, states):
    """twin_sector_order: Order = the permutation that sorts the flipped states (they are distinct: any sort does)"""
    return np.argsort(flip_states(mode, ns, states), kind="stable").astype(np.int32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_twin") / "host_twin.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", so,
                           os.path.join(ROOT, "tests", "host_twin.cpp"), os.path.join(csrc, "host_twin.cpp")])
    lib = C.CDLL(so)
    lib.ht_twin_sector.argtypes = [I, I, I, I, VP, C.c_char_p]
    lib.ht_twin_sector_orbs.argtypes = [I, VP, VP, VP]
    lib.ht_twin_order.argtypes = [I, VP, C.c_int64, I, VP, C.c_char_p]
    return lib


def _order(lib, mode, states, ns):
    m = np.ascontiguousarray(states, np.int32)
    out, err = np.full(max(m.size, 1), -7, np.int32), C.create_string_buffer(256)
    if lib.ht_twin_order(mode, m.ctypes.data, m.size, ns, out.ctypes.data, err):
        return err.value.decode(), None
    return "", out[:m.size]


def _twin(lib, mode, ns, q1, q2=0):
    out, err = np.zeros(3, np.int32), C.create_string_buffer(256)
    if lib.ht_twin_sector(mode, ns, q1, q2, out.ctypes.data, err):
        return err.value.decode(), None
    return "", (int(out[0]), int(out[1]), bool(out[2]))


@pytest.mark.parametrize("nbath", [1, 2])
@pytest.mark.parametrize("ed_mode,mode", [("superc", SUPERC), ("nonsu2", NONSU2)])
def test_order_of_every_sector(shim, built, ed_mode, mode, nbath):
    """Norb = 2, Nbath = 1 and 2 (Ns = 4, 6): the table of every sector against argsort(flip(map)), and what it is for:
    the flipped state order[i] of the source is state i of the twin sector"""
    _, pm = make_models(ed_mode, "normal", 2, nbath, seed=3)
    ns = pm.ns
    assert ns == 2 * (1 + nbath)
    sectors = range(-ns, ns + 1) if mode == SUPERC else range(0, 2 * ns + 1)
    total = 0
    for q in sectors:
        states = sector_map(pm, q)
        why, order = _order(shim, mode, states, ns)
        assert why == "", (q, why)
        ref = twin_order_ref(mode, ns, states)
        assert order.dtype == np.int32 and np.array_equal(order, ref), q
        tq = -q if mode == SUPERC else 2 * ns - q
        assert np.array_equal(flip_states(mode, ns, states)[order], sector_map(pm, tq).astype(np.int64)), q
        if mode == NONSU2:
            assert np.array_equal(order, np.arange(states.size - 1, -1, -1))
        total += states.size
    assert total == 4 ** ns      # every state of the Fock space is in one sector


def test_order_refusals(shim):
    ns = 3
    states = np.array([x for x in range(1 << (2 * ns)) if bin(x & 7).count("1") == bin(x >> 3).count("1")], np.int32)
    assert _order(shim, SUPERC, states, ns)[0] == ""
    assert "mode must be" in _order(shim, NORMAL, states, ns)[0]
    assert "Ns out of range" in _order(shim, SUPERC, states, 0)[0]
    assert "Ns out of range" in _order(shim, SUPERC, states, 16)[0]
    assert "not ascending" in _order(shim, SUPERC, states[::-1], ns)[0]
    assert "not ascending" in _order(shim, SUPERC, states, 2)[0]          # states past 2^(2 Ns)
    assert "not ascending" in _order(shim, NONSU2, np.array([3, 3], np.int32), ns)[0]


def test_twin_of_every_sector(shim, built):
    """the host function and edigpu_twin_sector, every sector of the three modes, self-twins included"""
    for ed_mode, mode, nbath in (("normal", NORMAL, 1), ("normal", NORMAL, 2), ("superc", SUPERC, 1), ("superc", SUPERC, 2),
                                 ("nonsu2", NONSU2, 1), ("nonsu2", NONSU2, 2)):
        _, pm = make_models(ed_mode, "normal", 2, nbath, seed=3)
        ns = pm.ns
        if mode == NORMAL:
            cases = [((a, b), (b, a, a == b)) for a, b in itertools.product(range(ns + 1), repeat=2)]
        elif mode == SUPERC:
            cases = [((sz, 0), (-sz, 0, sz == 0)) for sz in range(-ns, ns + 1)]
        else:
            cases = [((n, 0), (2 * ns - n, 0, n == ns)) for n in range(2 * ns + 1)]
        nself = 0
        for (q1, q2), want in cases:
            assert _twin(shim, mode, ns, q1, q2) == ("", want)
            assert twin_sector(pm, mode, q1, q2) == want
            # the twin of the twin is the sector
            assert twin_sector(pm, mode, want[0], want[1])[:2] == (q1, q2)
            nself += want[2]
        assert nself == (ns + 1 if mode == NORMAL else 1)


def test_twin_sector_refusals(shim, built):
    from edipack_amd import capi
    _, pm = make_models("normal", "normal", 2, 1, seed=3)
    ns = pm.ns
    for mode, q1, q2, msg in ((NORMAL, ns + 1, 0, "(Nup, Ndw) out of range"), (NORMAL, 0, -1, "(Nup, Ndw) out of range"),
                              (SUPERC, ns + 1, 0, "Sz out of range"), (SUPERC, -ns - 1, 0, "Sz out of range"),
                              (NONSU2, 2 * ns + 1, 0, "Ntot out of range"), (NONSU2, -1, 0, "Ntot out of range"),
                              (3, 0, 0, "mode must be"), (-1, 0, 0, "mode must be")):
        assert msg in _twin(shim, mode, ns, q1, q2)[0]
        with pytest.raises(capi.EdigpuError, match="edigpu_twin_sector.*" + msg.replace("(", r"\(").replace(")", r"\)")):
            twin_sector(pm, mode, q1, q2)
    assert "Ns out of range" in _twin(shim, NORMAL, 0, 0, 0)[0]
    assert capi.lib().edigpu_twin_sector(None, 0, 0, 0, None, None, None) != 0 and "NULL argument" in capi.last_error()


def test_twin_per_orbital(shim):
    """ed_total_ud = F: (nups, ndws) -> (ndws, nups)"""
    for norb in (1, 2, 3):
        for nups in itertools.product(range(3), repeat=norb):
            for ndws in itertools.product(range(3), repeat=norb):
                u, d, out = np.array(nups, np.int32), np.array(ndws, np.int32), np.zeros(2 * norb, np.int32)
                self_twin = shim.ht_twin_sector_orbs(norb, u.ctypes.data, d.ctypes.data, out.ctypes.data)
                assert tuple(out[:norb]) == ndws and tuple(out[norb:]) == nups and bool(self_twin) == (nups == ndws)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_twin_under_asan_ubsan(tmp_path):
    """a stand-alone program, nothing loaded into Python"""
    exe = str(tmp_path / "host_twin_sanitize")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=c++17", "-I", csrc,
           "-o", exe, os.path.join(ROOT, "tests", "host_twin_sanitize_main.cpp"), os.path.join(csrc, "host_twin.cpp")]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "0 failures" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
