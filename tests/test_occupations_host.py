"""CPU tests of the occupation operators (edigpu_apply_occ / edigpu_occ_moments): the observables formulas of
edipack_amd/observables.py on the reference's fixtures, the host tables of csrc/host_occ.cpp through tests/host_occ.cpp,
and the error paths that need no device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from edipack_amd import capi
from edipack_amd.hamiltonian import sector_map, sector_map_jz
from edipack_amd.observables import from_moments
from tests.common import make_jz_models, make_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, L, I = C.c_void_p, C.c_int64, C.c_int


def numpy_moments(nu, nd, v):
    """M[x, y] = sum_i |v_i|^2 n_x(i) n_y(i) from the occupation arrays nu, nd [norb, dim] of tests/observables.py"""
    bits = np.concatenate([nu, nd], axis=0)
    return (bits * (np.abs(v) ** 2)[None, :]) @ bits.T


@pytest.mark.parametrize("name", ["NORMAL_NORMAL", "HYBRID_NORMAL", "REPLICA_NORMAL", "GENERAL_SUPERC", "NORMAL_NONSU2",
                                  "REPLICA_NONSU2"])
def test_from_moments_reproduces_reference_fixture(name):
    """dens.check, docc.check, imp.check[0] (s2tot) and doubles.check[0:2] (Dust, Dund) from the moments of the oracle's
    dense ground states, to the tolerance tests/test_oracle_golden.py uses."""
    from tests import observables as ob
    from tests.test_oracle_golden import _golden_model
    om, g = _golden_model(name)
    _, states = ob.ground_manifold(om)
    M = np.stack([numpy_moments(*ob._occupations(om, sec, h), v) for sec, h, v in states])
    o = from_moments(M, om.norb, norm2=[float(np.vdot(v, v).real) for _, _, v in states])
    tol = 1e-9
    assert np.max(np.abs(o.dens - np.array(g["dens"]))) < tol
    assert np.max(np.abs(o.docc - np.array(g["docc"]))) < tol
    assert abs(o.s2tot - g["imp"][0]) < tol
    assert abs(o.dust - g["doubles"][0]) < tol and abs(o.dund - g["doubles"][1]) < tol
    # the parts the fixtures do not hold, against their definitions
    assert np.allclose(o.dens_up + o.dens_dw, o.dens, atol=1e-15) and np.allclose(o.dens_up - o.dens_dw, o.magz, atol=1e-15)
    assert np.allclose(np.diag(o.n2), o.dens + 2 * o.docc, atol=1e-13)
    assert np.allclose(np.diag(o.sz2), 0.25 * (o.dens - 2 * o.docc), atol=1e-13)


def test_from_moments_rejects_wrong_shape():
    with pytest.raises(ValueError):
        from_moments(np.zeros((4, 4)), 3)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_occ") / "host_occ.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", so,
                           os.path.join(ROOT, "tests", "host_occ.cpp"), os.path.join(csrc, "host_occ.cpp")])
    lib = C.CDLL(so)
    lib.ho_patterns_word.argtypes = [VP, L, I, VP]
    lib.ho_patterns_state.argtypes = [VP, L, I, I, VP]
    lib.ho_weight_table.argtypes = [VP, I, VP]
    lib.ho_sort_rows.argtypes = [VP, L, I, VP, VP]
    lib.ho_sum_slots.argtypes = [I, VP, VP]
    lib.ho_expand_sums.argtypes = [VP, I, VP, VP]
    return lib


def _word_patterns(shim, mp, norb):
    out = np.zeros(mp.size, np.uint16)
    shim.ho_patterns_word(mp.ctypes.data, mp.size, norb, out.ctypes.data)
    return out


def _state_patterns(shim, mp, norb, ns):
    out = np.zeros(mp.size, np.uint16)
    shim.ho_patterns_state(mp.ctypes.data, mp.size, norb, ns, out.ctypes.data)
    return out


def test_patterns_are_the_low_bits_of_the_map_words(shim):
    from oracle import oracle as O
    nsec = 0
    for mode, bath, norb, nbath in (("normal", "normal", 2, 2), ("normal", "hybrid", 3, 3), ("superc", "hybrid", 2, 3),
                                    ("nonsu2", "normal", 1, 4)):
        om, pm = make_models(mode, bath, norb, nbath, seed=1)
        mask = 2 ** norb - 1
        for sec in O.sectors(om):
            nsec += 1
            if mode == "normal":
                for which in (0, 1):
                    mp = sector_map(pm, sec[0], sec[1], which)
                    assert np.array_equal(_word_patterns(shim, mp, norb), mp & mask), (mode, sec, which)
            else:
                mp = sector_map(pm, sec)
                p = _state_patterns(shim, mp, norb, om.ns)
                assert np.array_equal(p & mask, mp & mask), (mode, sec)
                assert np.array_equal(p >> norb, (mp >> om.ns) & mask), (mode, sec)
    assert nsec > 60
    om, pm = make_jz_models(1)
    mp = sector_map_jz(pm, 3, 1)
    assert mp.size > 1
    p = _state_patterns(shim, mp, 3, om.ns)
    assert np.array_equal(p & 7, mp & 7) and np.array_equal(p >> 3, (mp >> om.ns) & 7)


@pytest.mark.parametrize("norb", [1, 2, 3, 5])
def test_weight_table_is_the_direct_sum(shim, norb):
    w = np.random.default_rng(norb).standard_normal(norb)
    tab = np.full(32, np.nan)
    shim.ho_weight_table(w.ctypes.data, norb, tab.ctypes.data)
    for p in range(32):
        s = 0.0
        for a in range(norb):
            if p < 2 ** norb and (p >> a) & 1:
                s += w[a]
        assert tab[p] == s, (p, tab[p], s)
    # N_a and S^z_a weights and their sums are exact
    for a in range(norb):
        for wu, wd in ((1.0, 1.0), (0.5, -0.5)):
            e = np.zeros(norb)
            e[a] = 1.0
            tu, td = np.zeros(32), np.zeros(32)
            shim.ho_weight_table((wu * e).ctypes.data, norb, tu.ctypes.data)
            shim.ho_weight_table((wd * e).ctypes.data, norb, td.ctypes.data)
            assert all(tu[p] == wu * ((p >> a) & 1) and td[p] == wd * ((p >> a) & 1) for p in range(2 ** norb))


@pytest.mark.parametrize("nblk", [1, 3])
def test_sorted_rows_and_sum_slots_give_the_moments(shim, nblk):
    """The reduction of the normal-mode kernel restated in numpy from the host tables alone -- rows taken in the sorted
    order, one bin per (run, up pattern), every slot gathering the bins that hold its bits -- equals the direct moments."""
    _, pm = make_models("normal", "hybrid", 3, 3, seed=2)
    norb, npat = 3, 8
    mu, md = sector_map(pm, 3, 2, 0), sector_map(pm, 3, 2, 1)
    pu, pd = _word_patterns(shim, mu, norb), _word_patterns(shim, md, norb).astype(np.uint8)
    order, run = np.zeros(md.size * nblk, np.int32), np.zeros(33, np.int32)
    shim.ho_sort_rows(pd.ctypes.data, md.size, nblk, order.ctypes.data, run.ctypes.data)
    assert np.array_equal(np.sort(order), np.arange(md.size * nblk)) and run[0] == 0 and run[npat] == order.size
    assert np.all(run[npat:] == order.size)
    for p in range(npat):
        rows = order[run[p]:run[p + 1]]
        assert np.all(pd[rows % md.size] == p) and np.all(np.diff(rows) > 0)
    need_up, need_dw = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    nslots = shim.ho_sum_slots(norb, need_up.ctypes.data, need_dw.ctypes.data)
    assert nslots == 1 + (2 * norb) * (2 * norb + 1) // 2
    assert np.all(need_up[nslots:] == 0xFF) and np.all(need_dw[nslots:] == 0xFF)
    v = np.random.default_rng(5).standard_normal((md.size * nblk, mu.size))
    sums = np.zeros(64)
    for p in range(npat):
        rows = order[run[p]:run[p + 1]]
        bins = np.array([np.sum(v[rows][:, pu == q] ** 2) for q in range(npat)])
        for t in range(nslots):
            if (p & need_dw[t]) == need_dw[t]:
                sums[t] += sum(bins[q] for q in range(npat) if (q & need_up[t]) == need_up[t])
    M, n2 = np.zeros((2 * norb, 2 * norb)), C.c_double(0.0)
    shim.ho_expand_sums(sums.ctypes.data, norb, M.ctypes.data, C.byref(n2))
    nu = np.array([np.tile((mu >> a) & 1, md.size * nblk) for a in range(norb)], float)
    nd = np.array([np.repeat((np.tile(md, nblk) >> a) & 1, mu.size) for a in range(norb)], float)
    ref = numpy_moments(nu, nd, v.reshape(-1))
    assert abs(n2.value - np.sum(v ** 2)) < 1e-12 * np.sum(v ** 2)
    assert np.max(np.abs(M - ref)) < 1e-12 * np.sum(v ** 2) and np.array_equal(M, M.T)


def test_null_handle_is_refused_with_a_message(built):
    lib = capi.lib()
    w = np.zeros(5)
    buf = np.zeros(100)
    assert lib.edigpu_apply_occ(None, None, None, capi.pd(w), capi.pd(w), None) != 0
    assert "edigpu_apply_occ" in capi.last_error() and "NULL" in capi.last_error()
    assert lib.edigpu_occ_moments(None, None, 1, capi.pd(buf), capi.pd(w)) != 0
    assert "edigpu_occ_moments" in capi.last_error() and "NULL" in capi.last_error()
