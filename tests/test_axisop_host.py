"""CPU tests of the one-axis c / c^+ operators (kernels_axisop.hip): the host tables of csrc/host_axisop.cpp through
tests/host_axisop.cpp against a forward numpy restatement (tests/axisop_cases.py: loop over the source states, flip the
bit, apply the sign, rank in the destination), and the (I, A, O) triple of every case against the sector dimensions.
Models: Ns = 4 (ed_total_ud=T, every operator, orbital, spin and sector, real and complex, with and without phonon blocks)
and chains of 1 + Nbath = 4 and 5 levels (ed_total_ud=F, every sector of one and two orbitals)."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from edipack_amd.hamiltonian import sector_map
from tests.axisop_cases import NONE, comb_words, forward_table, orbs_shape
from tests.common import make_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, I = C.c_void_p, C.c_int


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_axisop") / "host_axisop.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", so,
                           os.path.join(ROOT, "tests", "host_axisop.cpp"), os.path.join(csrc, "host_axisop.cpp"),
                           os.path.join(csrc, "host_pairs.cpp")])
    lib = C.CDLL(so)
    lib.ha_build_normal.argtypes = [I, I, I, I, I, I, I, VP, VP, VP, VP, C.c_char_p]
    lib.ha_build_orbs.argtypes = [I, I, VP, VP, I, VP, VP, VP, VP, C.c_char_p]
    return lib


def _ops(ops):
    return np.array([(1 if c else -1, a, s) for c, a, s in ops], dtype=np.int32).reshape(-1)


def _normal(lib, nup, ndw, ns, norb, nblk, cplx, ops):
    o, dest, shape, err = _ops(ops), np.zeros(2, np.int32), np.zeros(5, np.int64), C.create_string_buffer(256)
    if lib.ha_build_normal(nup, ndw, ns, norb, nblk, int(cplx), len(ops), o.ctypes.data, dest.ctypes.data, shape.ctypes.data, None, err):
        return err.value.decode(), None, None, None
    part = np.zeros(max(int(shape[4]), 1), np.uint32)
    assert lib.ha_build_normal(nup, ndw, ns, norb, nblk, int(cplx), len(ops), o.ctypes.data, dest.ctypes.data, shape.ctypes.data,
                               part.ctypes.data, err) == 0
    return "", tuple(int(x) for x in dest), tuple(int(x) for x in shape[:4]), part[:int(shape[4])].reshape(len(ops), -1)


def _orbs(lib, norb, nbath, nups, ndws, ops):
    o, dest, shape, err = _ops(ops), np.zeros(2 * norb, np.int32), np.zeros(5, np.int64), C.create_string_buffer(256)
    u, d = np.array(nups, np.int32), np.array(ndws, np.int32)
    if lib.ha_build_orbs(norb, nbath, u.ctypes.data, d.ctypes.data, len(ops), o.ctypes.data, dest.ctypes.data, shape.ctypes.data, None, err):
        return err.value.decode(), None, None, None
    part = np.zeros(max(int(shape[4]), 1), np.uint32)
    assert lib.ha_build_orbs(norb, nbath, u.ctypes.data, d.ctypes.data, len(ops), o.ctypes.data, dest.ctypes.data, shape.ctypes.data,
                             part.ctypes.data, err) == 0
    return ("", (tuple(int(x) for x in dest[:norb]), tuple(int(x) for x in dest[norb:])), tuple(int(x) for x in shape[:4]),
            part[:int(shape[4])].reshape(len(ops), -1))


def test_normal_tables_every_operator_every_sector(shim, built):
    """Ns = 4, norb = 2: index, sign and "none" exactly; (I, A, O) against the sector dimensions, real / complex vectors,
    one and three phonon blocks"""
    _, pm = make_models("normal", "normal", 2, 1, seed=11)
    ns = pm.ns
    assert ns == 4
    maps = {n: sector_map(pm, n, 0, 0).astype(np.int64) for n in range(ns + 1)}
    for n in range(ns + 1):
        assert np.array_equal(maps[n], comb_words(ns, n))
    checked = refused = 0
    for create, iorb, ispin in itertools.product((0, 1), (0, 1), (0, 1)):
        for nup, ndw in itertools.product(range(ns + 1), repeat=2):
            n_src = nup if ispin == 0 else ndw
            n_dst = n_src + (1 if create else -1)
            for nblk, cplx in ((1, False), (3, False), (1, True)):
                why, dest, shape, part = _normal(shim, nup, ndw, ns, 2, nblk, cplx, [(create, iorb, ispin)])
                if not 0 <= n_dst <= ns:
                    assert "leaves the Fock space" in why
                    refused += 1
                    continue
                assert why == "" and dest == ((n_dst, ndw) if ispin == 0 else (nup, n_dst))
                du, dd, w = maps[nup].size, maps[ndw].size, 2 if cplx else 1
                want = (w, du, maps[n_dst].size, dd * nblk) if ispin == 0 else (w * du, dd, maps[n_dst].size, nblk)
                assert shape == want, (create, iorb, ispin, nup, ndw, nblk, cplx)
                # the triple describes the whole vectors
                assert shape[0] * shape[1] * shape[3] == w * du * dd * nblk
                ref = forward_table(maps[n_src], maps[n_dst], iorb, bool(create), counted=True)
                assert part.shape == (1, maps[n_dst].size) and np.array_equal(part[0], ref)
                checked += 1
    assert checked == 3 * 8 * 20 and refused == 3 * 8 * 5


def test_normal_tables_several_terms_and_refusals(shim, built):
    ns = 4
    w = {n: comb_words(ns, n) for n in range(ns + 1)}
    ops = [(0, 0, 1), (0, 1, 1)]
    why, dest, shape, part = _normal(shim, 2, 3, ns, 2, 2, False, ops)
    assert why == "" and dest == (2, 2) and shape == (6, 4, 6, 2) and part.shape == (2, 6)
    for t, (c, a, s) in enumerate(ops):
        assert np.array_equal(part[t], forward_table(w[3], w[2], a, bool(c), True))
    why, _, shape, part = _normal(shim, 2, 2, ns, 2, 1, False, [(1, 0, 0)] * 8)
    assert why == "" and part.shape == (8, 4)
    for n in (0, 9):
        assert "nops must be 1 .. 8" in _normal(shim, 2, 2, ns, 2, 1, False, [(1, 0, 0)] * n)[0]
    assert "different destination sectors" in _normal(shim, 2, 2, ns, 2, 1, False, [(1, 0, 0), (1, 0, 1)])[0]
    assert "different destination sectors" in _normal(shim, 2, 2, ns, 2, 1, False, [(1, 0, 0), (0, 1, 0)])[0]
    for bad in ((1, 2, 0), (1, -1, 0), (1, 0, 2), (1, 0, -1)):
        assert "orbital / spin out of range" in _normal(shim, 2, 2, ns, 2, 1, False, [bad])[0]
    assert "out of range" in _normal(shim, 5, 2, ns, 2, 1, False, [(1, 0, 0)])[0]
    assert "out of range" in _normal(shim, 2, 2, ns, 2, 0, False, [(1, 0, 0)])[0]


@pytest.mark.parametrize("norb,nbath", [(1, 3), (2, 3), (1, 4), (2, 4)])
def test_orbs_tables_every_operator_every_sector(shim, norb, nbath):
    """chains of 1 + Nbath = 4 and 5 levels: the impurity is bit 0 of its chain word, so no entry carries a sign"""
    nlev = 1 + nbath
    words = {n: comb_words(nlev, n) for n in range(nlev + 1)}
    checked = refused = 0
    step = 1 if norb == 1 else 2      # two orbitals: every second occupation of the spectator axes keeps the sweep short
    for nups in itertools.product(range(0, nlev + 1, 1), repeat=norb):
        for ndws in itertools.product(range(0, nlev + 1, step), repeat=norb):
            dims = [words[n].size for n in nups + ndws]
            for create, iorb, ispin in itertools.product((0, 1), range(norb), (0, 1)):
                why, dest, shape, part = _orbs(shim, norb, nbath, nups, ndws, [(create, iorb, ispin)])
                n_src = (nups, ndws)[ispin][iorb]
                n_dst = n_src + (1 if create else -1)
                if not 0 <= n_dst <= nlev:
                    assert "leaves the Fock space" in why
                    refused += 1
                    continue
                want = [list(nups), list(ndws)]
                want[ispin][iorb] = n_dst
                assert why == "" and dest == (tuple(want[0]), tuple(want[1]))
                axis = iorb + ispin * norb
                i, a, o = orbs_shape(dims, axis)
                assert shape == (i, a, words[n_dst].size, o), (nups, ndws, create, iorb, ispin)
                assert i * a * o == int(np.prod(dims))
                ref = forward_table(words[n_src], words[n_dst], 0, bool(create), counted=False)
                assert np.array_equal(part[0], ref)
                live = part[0] != NONE
                assert not np.any(part[0][live] >> np.uint32(31)) and live.sum() == (words[n_dst] & 1 == create).sum()
                checked += 1
    assert checked > 30 and refused > 0


def test_orbs_tables_several_terms_and_refusals(shim):
    why, dest, shape, part = _orbs(shim, 2, 3, (2, 1), (1, 2), [(0, 1, 1)] * 3)
    assert why == "" and dest == ((2, 1), (1, 1)) and shape == (6 * 4 * 4, 6, 4, 1) and part.shape == (3, 4)
    assert np.array_equal(part[0], part[1]) and np.array_equal(part[0], part[2])
    assert "different destination sectors" in _orbs(shim, 2, 3, (2, 1), (1, 2), [(0, 1, 1), (0, 0, 1)])[0]
    assert "different destination sectors" in _orbs(shim, 2, 3, (2, 1), (1, 2), [(0, 1, 1), (1, 1, 1)])[0]
    assert "nops must be 1 .. 8" in _orbs(shim, 2, 3, (2, 1), (1, 2), [(0, 1, 1)] * 9)[0]
    assert "orbital / spin out of range" in _orbs(shim, 2, 3, (2, 1), (1, 2), [(0, 2, 1)])[0]
    assert "out of range" in _orbs(shim, 2, 3, (5, 1), (1, 2), [(0, 1, 1)])[0]
