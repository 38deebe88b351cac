"""CPU tests of the fused two-operator products (edigpu_apply_pairs_normal): the host tables of csrc/host_pairs.cpp
through tests/host_pairs.cpp against a state-by-state numpy restatement (tests/pairs_cases.py), the destination rules, the
seed lists and chi_channel of edipack_amd/observables.py, and the entry point that needs no device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from edipack_amd import capi
from edipack_amd.hamiltonian import pairs_sector, sector_map
from edipack_amd.observables import chi_channel, exct_chi_seeds, pair_chi_seeds
from tests.common import make_models
from tests.pairs_cases import NONE, ORDERED_PAIRS2, destination, get_chiab, species_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, L, I = C.c_void_p, C.c_int64, C.c_int


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_pairs") / "host_pairs.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", so,
                           os.path.join(ROOT, "tests", "host_pairs.cpp"), os.path.join(csrc, "host_pairs.cpp")])
    lib = C.CDLL(so)
    lib.hp_dim.restype = L
    lib.hp_dim.argtypes = [I, I]
    lib.hp_rank.restype = L
    lib.hp_rank.argtypes = [C.c_uint32]
    lib.hp_destination.argtypes = [I, I, I, VP, VP]
    lib.hp_species_table.argtypes = [I, I, VP, I, VP]
    lib.hp_build.argtypes = [I, I, I, I, I, VP, VP, VP, VP, VP, VP, C.c_char_p]
    lib.hp_check.argtypes = [I, I, I, I, I, VP, VP, C.c_char_p]
    return lib


@pytest.fixture(scope="module")
def model4(built):
    """norb = 2, ns = 4"""
    _, pm = make_models("normal", "normal", 2, 1, seed=11)
    assert pm.ns == 4
    return pm


def _ops(term):
    return np.array([(1 if o[0] else -1) if f == 0 else o[f] for o in term[1:] for f in range(3)], dtype=np.int32)


def _table(lib, ns, n_dst, term, spin):
    tab = np.full(max(int(lib.hp_dim(ns, n_dst)), 1), 12345, dtype=np.uint32)
    ops = _ops(term)
    ident = lib.hp_species_table(ns, n_dst, ops.ctypes.data, spin, tab.ctypes.data)
    return None if ident else tab[:int(lib.hp_dim(ns, n_dst))]


def _build(lib, nup, ndw, ns, norb, terms):
    n = len(terms)
    ops = np.concatenate([_ops(t) for t in terms]) if n else np.zeros(6, np.int32)
    coef = np.array([t[0] for t in terms] + [0.0], dtype=np.float64)
    info, cout = np.zeros(8, np.int64), np.zeros(max(n, 1))
    err = C.create_string_buffer(256)
    if lib.hp_build(nup, ndw, ns, norb, n, coef.ctypes.data, ops.ctypes.data, info.ctypes.data, cout.ctypes.data, None, None, err):
        return err.value.decode(), None
    up, dw = np.zeros(max(n * info[4], 1), np.uint32), np.zeros(max(n * info[5], 1), np.uint32)
    assert lib.hp_build(nup, ndw, ns, norb, n, coef.ctypes.data, ops.ctypes.data, info.ctypes.data, cout.ctypes.data,
                        up.ctypes.data, dw.ctypes.data, err) == 0
    return "", (info, cout, up[:n * info[4]].reshape(n, -1), dw[:n * info[5]].reshape(n, -1))


def test_rank_is_the_position_in_the_sector_map(shim, model4):
    for n in range(5):
        m = sector_map(model4, n, 0, 0)
        assert shim.hp_dim(4, n) == m.size
        assert [shim.hp_rank(int(w)) for w in m] == list(range(m.size))
    assert shim.hp_dim(4, -1) == 0 and shim.hp_dim(4, 5) == 0 and shim.hp_dim(30, 15) == 155117520


def test_tables_against_numpy_every_ordered_pair_every_sector(shim, model4):
    """index, sign and "none" exactly, for all 64 ordered operator pairs on all 25 sectors of norb = 2, ns = 4"""
    ns = 4
    maps = {n: sector_map(model4, n, 0, 0) for n in range(ns + 1)}   # the up and the down map are the same list
    checked = skipped = 0
    for o1, o2 in ORDERED_PAIRS2:
        term = (1.0, o1, o2)
        for nup in range(ns + 1):
            for ndw in range(ns + 1):
                nu, nd, ok = destination(nup, ndw, ns, term)
                out = np.zeros(3, np.int32)
                shim.hp_destination(nup, ndw, ns, _ops(term).ctypes.data, out.ctypes.data)
                assert (int(out[0]), int(out[1]), bool(out[2])) == (nu, nd, ok)
                if not ok:
                    skipped += 1
                    continue
                for spin, (ns_, nd_) in ((0, (nup, nu)), (1, (ndw, nd))):
                    ref = species_table(maps[ns_], maps[nd_], term, spin)
                    got = _table(shim, ns, nd_, term, spin)
                    assert (ref is None) == (got is None), (term, nup, ndw, spin)
                    if ref is not None:
                        assert np.array_equal(ref, got), (term, nup, ndw, spin)
                        checked += 1
    assert checked > 1500 and skipped > 0


def test_destination_rules_at_the_edges(shim, model4):
    ns = 4
    c_up_c_dw = (1.0, (0, 0, 1), (0, 0, 0))          # C_dw first, then C_up
    cd_dw_cd_up = (1.0, (1, 0, 0), (1, 0, 1))        # C^+_up first, then C^+_dw
    for n in range(ns + 1):
        assert destination(0, n, ns, c_up_c_dw)[2] is False and pairs_sector(model4, 0, n, [c_up_c_dw])[2] is False
        assert destination(ns, n, ns, cd_dw_cd_up)[2] is False and pairs_sector(model4, ns, n, [cd_dw_cd_up])[2] is False
    assert pairs_sector(model4, 2, 2, [c_up_c_dw]) == (1, 1, True)
    assert pairs_sector(model4, 2, 2, [cd_dw_cd_up]) == (3, 3, True)
    assert pairs_sector(model4, 1, 0, [c_up_c_dw]) == (0, -1, False)
    # c^+ c on an empty species: the number leaves the range on the way, though it comes back
    assert pairs_sector(model4, 0, 2, [(1.0, (0, 0, 0), (1, 1, 0))]) == (0, 2, False)
    assert pairs_sector(model4, 1, 2, [(1.0, (0, 0, 0), (1, 1, 0))]) == (1, 2, True)
    # several terms: one common destination, exists only when every term exists
    assert pairs_sector(model4, 2, 2, exct_chi_seeds(1, 0, 1)[0][0]) == (2, 2, True)
    assert pairs_sector(model4, 0, 2, exct_chi_seeds(1, 0, 1)[0][0]) == (0, 2, False)


def test_validation(shim, model4):
    ok = (1.0, (0, 0, 1), (0, 0, 0))
    for bad in ((1.0, (0, 2, 1), (0, 0, 0)), (1.0, (0, 0, 1), (0, -1, 0)), (1.0, (0, 0, 2), (0, 0, 0)), (1.0, (0, 0, 1), (0, 0, -1))):
        why, _ = _build(shim, 2, 2, 4, 2, [bad])
        assert "orbital / spin out of range" in why
        with pytest.raises(capi.EdigpuError, match="edigpu_pairs_sector: orbital / spin out of range"):
            pairs_sector(model4, 2, 2, [bad])
    why, _ = _build(shim, 2, 2, 4, 2, [ok, (1.0, (1, 0, 0), (1, 0, 1))])
    assert "different destination sectors" in why
    with pytest.raises(capi.EdigpuError, match="edigpu_pairs_sector: the terms lead to different destination sectors"):
        pairs_sector(model4, 2, 2, [ok, (1.0, (1, 0, 0), (1, 0, 1))])
    for n in (0, 9):
        why, _ = _build(shim, 2, 2, 4, 2, [ok] * n)
        assert "nterms must be 1 .. 8" in why
        with pytest.raises(capi.EdigpuError, match="edigpu_pairs_sector: nterms must be 1 .. 8"):
            pairs_sector(model4, 2, 2, [ok] * n)
    why, t = _build(shim, 2, 2, 4, 2, [ok] * 8)
    assert why == "" and t[2].shape == (8, 4) and t[3].shape == (8, 4)
    why, _ = _build(shim, 0, 2, 4, 2, [ok])
    assert "leaves the Fock space" in why


def test_same_level_cc_gives_an_all_none_table(shim, model4):
    for create in (0, 1):
        for spin in (0, 1):
            term = (1.0, (create, 1, spin), (create, 1, spin))
            for n_dst in range(5):                      # any particle number: a level cannot be emptied or filled twice
                tab = _table(shim, 4, n_dst, term, spin)
                assert tab is not None and tab.size == shim.hp_dim(4, n_dst) and np.all(tab == NONE)
            assert _table(shim, 4, 2, term, 1 - spin) is None
    why, t = _build(shim, 2, 2, 4, 2, [(1.0, (0, 0, 0), (0, 0, 0))])
    assert why == "" and t[0][0] == 0 and np.all(t[2] == NONE) and t[0][6] == 0 and t[0][7] == 1   # up: none; down: identity


def test_number_operator_is_the_partial_identity(shim, model4):
    for a in (0, 1):
        for spin in (0, 1):
            for n in range(5):
                m = sector_map(model4, n, 0, 0)
                tab = _table(shim, 4, n, (1.0, (0, a, spin), (1, a, spin)), spin)
                occ = ((m >> a) & 1).astype(bool)
                assert np.array_equal(tab[occ], np.arange(m.size, dtype=np.uint32)[occ])    # plus sign: the two signs cancel
                assert np.all(tab[~occ] == NONE)


def test_swapping_two_same_spin_operators_flips_every_sign(shim, model4):
    ops = [(c, a, 0) for c in (0, 1) for a in (0, 1)]
    n_live = 0
    for o1 in ops:
        for o2 in ops:
            if o1[1] == o2[1]:
                continue                                  # the same level: the operators do not simply anticommute
            for n in range(5):
                nd = n + sum(1 if o[0] else -1 for o in (o1, o2))
                if not 0 <= nd <= 4 or not 0 <= n + (1 if o1[0] else -1) <= 4 or not 0 <= n + (1 if o2[0] else -1) <= 4:
                    continue
                t12, t21 = _table(shim, 4, nd, (1.0, o1, o2), 0), _table(shim, 4, nd, (1.0, o2, o1), 0)
                live = t12 != NONE
                assert np.array_equal(live, t21 != NONE)
                assert np.array_equal(t12[live] ^ np.uint32(0x80000000), t21[live])
                n_live += int(live.sum())
    assert n_live > 0


def test_pair_and_exciton_seed_lists():
    UP, DW = 0, 1
    assert pair_chi_seeds(0, 0) == [([(1.0, (0, 0, DW), (0, 0, UP))], +1), ([(1.0, (1, 0, UP), (1, 0, DW))], -1)]
    assert pair_chi_seeds(0, 1) == [
        ([(1.0, (0, 0, DW), (0, 0, UP)), (1.0, (0, 1, DW), (0, 1, UP))], +1),
        ([(1.0, (1, 0, UP), (1, 0, DW)), (1.0, (1, 1, UP), (1, 1, DW))], -1)]
    assert exct_chi_seeds(1, 0, 1) == [
        ([(1.0, (0, 1, UP), (1, 0, UP)), (1.0, (0, 1, DW), (1, 0, DW))], +1),
        ([(1.0, (0, 0, UP), (1, 1, UP)), (1.0, (0, 0, DW), (1, 1, DW))], -1)]
    assert exct_chi_seeds(3, 0, 1) == [
        ([(1.0, (0, 1, UP), (1, 0, UP)), (-1.0, (0, 1, DW), (1, 0, DW))], +1),
        ([(1.0, (0, 0, UP), (1, 1, UP)), (-1.0, (0, 0, DW), (1, 1, DW))], -1)]
    assert exct_chi_seeds(2, 0, 1) == [
        ([(1.0, (0, 1, UP), (1, 0, DW))], +1),
        ([(1.0, (0, 0, DW), (1, 1, UP))], -1),
        ([(1.0, (0, 1, DW), (1, 0, UP))], +1),
        ([(1.0, (0, 0, UP), (1, 1, DW))], -1)]
    with pytest.raises(ValueError):
        exct_chi_seeds(4, 0, 1)


@pytest.mark.parametrize("axis", ["m", "r"])
def test_chi_channel_against_get_chiab(axis):
    rng = np.random.default_rng(5)
    beta = 7.0
    z = 1j * 2.0 * np.pi * np.arange(6) / beta if axis == "m" else np.concatenate([[0.01j], np.linspace(-3, 3, 6) + 0.01j])
    for trial in range(6):
        n = 5 + trial
        a, b = rng.standard_normal(n), np.abs(rng.standard_normal(n)) + 0.1
        e, zv = np.linalg.eigh(np.diag(a) + np.diag(b[1:], 1) + np.diag(b[1:], -1))
        # trial 0, 1: a pole forced to zero (e_state = an eigenvalue of the tridiagonal matrix)
        e_state = float(e[2]) if trial < 2 else float(e[0]) - 0.3 + 0.5 * trial
        norm2, zeta = 0.7 + trial, 1.3
        for ichan, isign in ((1, +1), (2, -1), (3, +1), (4, -1)):
            peso, de = norm2 * zv[0] ** 2 / zeta, isign * (e - e_state)
            ref, refm = get_chiab(peso, de, ichan, z, beta, axis)
            got, gotm = chi_channel(a, b, norm2, e_state, isign, ichan, z, beta, zeta=zeta, mirror=True, axis=axis)
            scale = max(np.max(np.abs(ref)), np.max(np.abs(refm)), 1.0)
            assert np.max(np.abs(got - ref)) < 1e-12 * scale and np.max(np.abs(gotm - refm)) < 1e-12 * scale
            assert np.array_equal(chi_channel(a, b, norm2, e_state, isign, ichan, z, beta, zeta=zeta, axis=axis), got)
            if trial < 2:
                assert np.min(np.abs(beta * de)) < 1e-8 and np.max(np.abs(ref)) > 0
            # zero temperature: the thermal factors are 1, the poles on the other side and the zero pole drop out
            got0 = chi_channel(a, b, norm2, e_state, isign, ichan, z, None, zeta=zeta, axis=axis)
            keep = (de if ichan % 2 == 1 else -de) > 1e-10
            ref0 = sum((-p if ichan % 2 == 1 else p) / (z - d) for p, d in zip(peso[keep], de[keep])) + 0 * z
            assert np.max(np.abs(got0 - ref0)) < 1e-12 * max(np.max(np.abs(ref0)), 1.0)


def test_chi_channel_rejects_the_time_axis():
    with pytest.raises(ValueError):
        chi_channel([0.0], [0.0], 1.0, 0.0, 1, 1, [0.0], 1.0, axis="t")


def test_pairs_sector_needs_no_device(built):
    _, pm = make_models("normal", "hybrid", 5, 3, seed=11)
    assert pairs_sector(pm, 4, 4, pair_chi_seeds(0, 4)[0][0]) == (3, 3, True)
    assert pairs_sector(pm, 4, 4, exct_chi_seeds(2, 0, 4)[0][0]) == (3, 5, True)
    _, ps = make_models("superc", "hybrid", 2, 3, seed=12)
    with pytest.raises(capi.EdigpuError, match="edigpu_pairs_sector: only ed_mode=normal"):
        pairs_sector(ps, 1, 1, pair_chi_seeds(0, 0)[0][0])
