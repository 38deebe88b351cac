"""CPU tests of the phonon operators (edigpu_apply_xph / edigpu_ph_rdm): the host tables of csrc/host_ph.cpp through
tests/host_ph.cpp, the numpy observables of edipack_amd/observables.py against loop-by-loop restatements of the
reference's lines, and the error paths that need no device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from edipack_amd import capi
from edipack_amd.observables import from_ph_rdm, hermite_functions, phonon_gf, phonon_pdf
from tests.ph_cases import U, ref_ph_rdm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, L, I = C.c_void_p, C.c_int64, C.c_int


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_ph") / "host_ph.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", so,
                           os.path.join(ROOT, "tests", "host_ph.cpp"), os.path.join(csrc, "host_ph.cpp"),
                           os.path.join(csrc, "host_occ.cpp")])
    lib = C.CDLL(so)
    lib.hp_class_word.argtypes = [I, VP]
    lib.hp_class_rows.argtypes = [VP, L, I, VP]
    lib.hp_sqrt_table.argtypes = [I, VP]
    lib.hp_sort_keys.argtypes = [VP, L, I, VP, VP]
    lib.hp_plan_normal.argtypes = [VP, L, VP, L, I, L, VP, VP, VP, I, VP]
    lib.hp_plan_flat.argtypes = [VP, L, I, L, VP, VP, VP, I, VP]
    lib.hp_expand_slots.argtypes = [VP, I, I, VP]
    lib.hp_expand_slots.restype = C.c_double
    return lib


def _ternary(p, norb):
    """class of the spin-word pattern p, counted digit by digit"""
    c = 0
    for a in range(norb):
        if (p >> a) & 1:
            c += 3 ** a
    return c


@pytest.mark.parametrize("norb", [1, 2, 3, 4, 5])
def test_class_tables_are_the_ternary_count(shim, norb):
    assert shim.hp_num_classes(norb) == 3 ** norb
    cls = np.zeros(2 ** norb, np.uint16)
    shim.hp_class_word(norb, cls.ctypes.data)
    assert [int(x) for x in cls] == [_ternary(p, norb) for p in range(2 ** norb)]
    pat = np.arange(4 ** norb, dtype=np.uint16)                 # every up | down << norb
    out = np.zeros(pat.size, np.uint8)
    shim.hp_class_rows(pat.ctypes.data, pat.size, norb, out.ctypes.data)
    for p in range(4 ** norb):
        up, dw = p & (2 ** norb - 1), p >> norb
        nt = [((up >> a) & 1) + ((dw >> a) & 1) for a in range(norb)]
        assert out[p] == sum(nt[a] * 3 ** a for a in range(norb)) == _ternary(up, norb) + _ternary(dw, norb)
    assert out.max() == 3 ** norb - 1


@pytest.mark.parametrize("dimph", [2, 17, 32])
def test_sqrt_table(shim, dimph):
    sq = np.full(dimph + 1, np.nan)
    shim.hp_sqrt_table(dimph, sq.ctypes.data)
    assert np.array_equal(sq, np.sqrt(np.arange(dimph + 1, dtype=np.float64)))


def test_sort_keys_is_a_stable_permutation(shim):
    key = np.random.default_rng(3).integers(0, 243, 5000).astype(np.uint8)
    order, run = np.zeros(key.size, np.int32), np.zeros(244, np.int32)
    shim.hp_sort_keys(key.ctypes.data, key.size, 243, order.ctypes.data, run.ctypes.data)
    assert np.array_equal(order, np.argsort(key, kind="stable"))
    assert run[0] == 0 and run[-1] == key.size and np.array_equal(np.diff(run), np.bincount(key, minlength=243))


def _plan(shim, norb, target, pu=None, pd=None, pat=None):
    ncls, cap = 3 ** norb, 20000
    ubeg, units = np.zeros(ncls + 1, np.int32), np.zeros((cap, 6), np.int32)
    if pat is None:
        rorder, corder = np.zeros(pd.size, np.int32), np.zeros(pu.size, np.int32)
        n = shim.hp_plan_normal(pu.ctypes.data, pu.size, pd.ctypes.data, pd.size, norb, target, rorder.ctypes.data,
                                corder.ctypes.data, units.ctypes.data, cap, ubeg.ctypes.data)
    else:
        rorder, corder = np.zeros(1, np.int32), np.zeros(pat.size, np.int32)
        n = shim.hp_plan_flat(pat.ctypes.data, pat.size, norb, target, rorder.ctypes.data, corder.ctypes.data,
                              units.ctypes.data, cap, ubeg.ctypes.data)
    assert n >= 0
    return rorder, corder, units[:n], ubeg


def _walk(rorder, corder, units, dim_cols):
    """(electronic index, class, unit) of every element the kernel visits, in its order"""
    els, cl = [], []
    for (r0, c0, ncols, cls, p0, p1) in units:
        p = np.arange(p0, p1)
        els.append(rorder[r0 + p // ncols].astype(np.int64) * dim_cols + corder[c0 + p % ncols])
        cl.append(np.full(p.size, cls))
    return np.concatenate(els), np.concatenate(cl)


@pytest.mark.parametrize("norb,dim_up,dim_dw,target", [(1, 7, 5, 4), (2, 37, 23, 16), (3, 130, 61, 64), (5, 200, 90, 50),
                                                       (2, 1, 1, 2048), (2, 64, 64, 100000)])
def test_normal_plan_covers_every_element_once_with_one_class_per_unit(shim, norb, dim_up, dim_dw, target):
    rng = np.random.default_rng(norb + dim_up)
    pu = rng.integers(0, 2 ** norb, dim_up).astype(np.uint16)
    pd = rng.integers(0, 2 ** norb, dim_dw).astype(np.uint16)
    rorder, corder, units, ubeg = _plan(shim, norb, target, pu=pu, pd=pd)
    assert np.array_equal(np.sort(rorder), np.arange(dim_dw)) and np.array_equal(np.sort(corder), np.arange(dim_up))
    els, cl = _walk(rorder, corder, units, dim_up)
    assert np.array_equal(np.sort(els), np.arange(dim_up * dim_dw))          # a permutation of the electronic indices
    want = np.array([_ternary(int(pu[e % dim_up]), norb) + _ternary(int(pd[e // dim_up]), norb) for e in els])
    assert np.array_equal(cl, want)                                          # one class per unit, the right one
    assert np.all(np.diff(units[:, 3]) >= 0) and ubeg[0] == 0 and ubeg[-1] == len(units)
    assert np.array_equal(np.diff(ubeg), np.bincount(units[:, 3], minlength=3 ** norb))
    assert np.all(units[:, 5] - units[:, 4] <= max(target, 1) + 1) and np.all(units[:, 5] > units[:, 4])
    # the kernel's sums restated from the plan alone: partial Gram matrices per unit, added per class in unit order
    dimph = 3
    v = rng.standard_normal((dimph, dim_up * dim_dw))
    rho = np.zeros((3 ** norb, dimph, dimph))
    for (r0, c0, ncols, cls, p0, p1) in units:
        p = np.arange(p0, p1)
        e = rorder[r0 + p // ncols].astype(np.int64) * dim_up + corder[c0 + p % ncols]
        rho[cls] += v[:, e] @ v[:, e].T
    ref = ref_ph_rdm(want[np.argsort(els)], v.reshape(-1), dimph, 3 ** norb)
    assert np.max(np.abs(rho - ref)) <= 2 * dim_up * dim_dw * U * np.sum(v ** 2)


@pytest.mark.parametrize("norb,dim_el,target", [(1, 11, 3), (2, 252, 16), (5, 3000, 40)])
def test_flat_plan_covers_every_row_once_with_one_class_per_unit(shim, norb, dim_el, target):
    pat = np.random.default_rng(dim_el).integers(0, 4 ** norb, dim_el).astype(np.uint16)
    rorder, corder, units, ubeg = _plan(shim, norb, target, pat=pat)
    assert np.array_equal(rorder, [0]) and np.array_equal(np.sort(corder), np.arange(dim_el))
    els, cl = _walk(rorder, corder, units, dim_el)
    assert np.array_equal(np.sort(els), np.arange(dim_el))
    mask = 2 ** norb - 1
    assert np.array_equal(cl, [_ternary(int(pat[e]) & mask, norb) + _ternary(int(pat[e]) >> norb, norb) for e in els])
    assert np.all(np.diff(units[:, 3]) >= 0) and np.array_equal(np.diff(ubeg), np.bincount(units[:, 3], minlength=3 ** norb))
    for c in range(3 ** norb):      # stable: the rows of a class in ascending order
        assert np.all(np.diff(els[cl == c]) > 0)


@pytest.mark.parametrize("dimph", [2, 5, 32])
@pytest.mark.parametrize("cw", [1, 2])
def test_slot_expansion_is_exactly_hermitian(shim, dimph, cw):
    ns = shim.hp_slots(dimph)
    assert ns == dimph * (dimph + 1) // 2
    assert sorted(shim.hp_slot(dimph, n, m) for n in range(dimph) for m in range(n, dimph)) == list(range(ns))
    slots = np.random.default_rng(dimph).standard_normal(ns * cw)
    rho = np.full(dimph * dimph * cw, np.nan)
    tr = shim.hp_expand_slots(slots.ctypes.data, dimph, cw, rho.ctypes.data)
    R = rho.view(np.complex128 if cw == 2 else np.float64).reshape(dimph, dimph)
    assert np.array_equal(R, R.conj().T) and np.all(np.imag(np.diag(R)) == 0)
    for n in range(dimph):
        for m in range(n, dimph):
            s = slots[shim.hp_slot(dimph, n, m) * cw:][:cw]
            assert R[n, m].real == s[0] and (cw == 1 or n == m or R[n, m].imag == s[1])
    assert tr == sum(slots[shim.hp_slot(dimph, n, n) * cw] for n in range(dimph))


def _reference_hermite(x, dimph):
    """Hermite, ED_OBSERVABLES_NORMAL.f90:1282-1298"""
    psi = np.zeros(dimph)
    den = 1.331335373062335
    psi[0] = np.exp(-0.5 * x * x) / den
    psi[1] = np.exp(-0.5 * x * x) * np.sqrt(2.0) * x / den
    for i in range(2, dimph):
        psi[i] = 2 * x * psi[i - 1] / np.sqrt(float(2 * i)) - psi[i - 2] * np.sqrt(float(i - 1) / float(i))
    return psi


def _reference_loop(v, cls, dim_el, dimph, ncls, xmin, xmax, lpos, conj=False):
    """the observables loop, ED_OBSERVABLES_NORMAL.f90:182-214, and prob_distr_ph, :1235-1280, index by index (0-based),
    with peso = 1; conj: v(i) conjg(v(j)) and the real part, our definition for complex vectors"""
    prob, dens, xph, x2 = np.zeros(dimph), 0.0, 0.0, 0.0
    pdf, part = np.zeros(lpos), np.zeros((lpos, ncls))
    pr = (lambda a, b: (a * np.conj(b)).real) if conj else (lambda a, b: a * b)
    for i in range(dim_el * dimph):
        iph, i_el = i // dim_el, i % dim_el
        w = abs(v[i]) ** 2
        prob[iph] += w
        dens += iph * w
        if iph < dimph - 1:
            xph += np.sqrt(2.0 * (iph + 1)) * pr(v[i], v[i_el + (iph + 1) * dim_el])
        x2 += 0.5 * (1 + 2 * iph) * w
        if iph < dimph - 2:
            x2 += np.sqrt(float((iph + 1) * (iph + 2))) * pr(v[i], v[i_el + (iph + 2) * dim_el])
        if dimph > 1 and iph == 0:
            dx = (xmax - xmin) / float(lpos)
            for k in range(lpos):
                psi = _reference_hermite(xmin + k * dx, dimph)
                for a in range(dimph):
                    for b in range(dimph):
                        t = psi[a] * psi[b] * pr(v[i_el + a * dim_el], v[i_el + b * dim_el])
                        pdf[k] += t
                        part[k, cls[i_el]] += t
    return prob, dens, xph, x2, pdf, part


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("dimph", [2, 3, 5])
def test_observables_against_the_reference_loops(dimph, cplx):
    """Each side adds at most dim_el DimPh^2 (<= 925) terms bounded by norm2 max psi^2: the tolerance is
    2 dim_el DimPh^2 u norm2 max(1, max psi^2).  Complex vectors: v conj v against its own restatement."""
    norb, dim_el, ncls = 2, 37, 9
    rng = np.random.default_rng(dimph)
    cls = rng.integers(0, ncls, dim_el)
    v = rng.standard_normal(dim_el * dimph)
    if cplx:
        v = v + 1j * rng.standard_normal(dim_el * dimph)
    V = v.reshape(dimph, dim_el)
    rho = np.zeros((ncls, dimph, dimph), dtype=v.dtype)
    for c in range(ncls):
        rho[c] = V[:, cls == c] @ V[:, cls == c].conj().T
    xmin, xmax, lpos = -3.0, 3.5, 13
    prob, dens, xph, x2, pdf, part = _reference_loop(v, cls, dim_el, dimph, ncls, xmin, xmax, lpos, conj=cplx)
    o = from_ph_rdm(rho)
    x, pdf_ph, pdf_part = phonon_pdf(rho, xmin, xmax, lpos)
    psi = hermite_functions(x, dimph)
    assert np.array_equal(x, xmin + np.arange(lpos) * ((xmax - xmin) / lpos)) and psi.shape == (lpos, dimph)
    assert all(np.allclose(psi[k], _reference_hermite(x[k], dimph), rtol=1e-13, atol=1e-300) for k in range(lpos))
    norm2 = float(np.sum(np.abs(v) ** 2))
    tol = 2 * dim_el * dimph ** 2 * U * norm2 * max(1.0, float(np.max(psi ** 2)))
    assert np.max(np.abs(o.prob_ph - prob)) <= tol and abs(o.dens_ph - dens) <= tol
    assert abs(o.x_ph - xph) <= tol and abs(o.x2_ph - x2) <= tol
    assert np.max(np.abs(o.prob_class - np.bincount(cls, (np.abs(V) ** 2).sum(axis=0), minlength=ncls))) <= tol
    assert np.max(np.abs(pdf_ph - pdf)) <= tol and np.max(np.abs(pdf_part - part)) <= tol
    # a manifold of two states, each divided by its norm, as from_moments averages
    o2 = from_ph_rdm(np.stack([rho, 4.0 * rho]), norm2=[norm2, 4.0 * norm2])
    assert abs(o2.x2_ph - x2 / norm2) <= tol / norm2 and abs(o2.prob_ph.sum() - 1.0) <= tol / norm2


def test_from_ph_rdm_rejects_wrong_shape():
    with pytest.raises(ValueError):
        from_ph_rdm(np.zeros((4, 4)))
    with pytest.raises(ValueError):
        phonon_pdf(np.zeros((9, 3, 2)), -1.0, 1.0, 4)


def test_phonon_gf_is_the_dense_resolvent_of_the_tridiagonal_matrix():
    """every pole above the state: D(z) = norm2 / zeta [ (z - (T - E))^-1 - (z + (T - E))^-1 ]_00"""
    rng = np.random.default_rng(12)
    n = 12
    a, b = rng.standard_normal(n), np.concatenate([[0.0], rng.uniform(0.2, 1.0, n - 1)])
    T = np.diag(a) + np.diag(b[1:], 1) + np.diag(b[1:], -1)
    e_state = np.linalg.eigvalsh(T)[0] - 0.3
    norm2, zeta = 1.7, 2.5
    z = np.concatenate([1j * 2 * np.pi * np.arange(8) / 50.0, np.linspace(-3, 3, 7) + 0.05j])
    D = phonon_gf(a, b, norm2, e_state, z, zeta=zeta)
    A = T - e_state * np.eye(n)
    ref = np.array([np.linalg.inv(zz * np.eye(n) - A)[0, 0] - np.linalg.inv(zz * np.eye(n) + A)[0, 0] for zz in z])
    ref *= norm2 / zeta
    assert np.max(np.abs(D - ref)) <= 1e-12 * np.max(np.abs(ref))
    # finite temperature: the Matsubara form of get_impD_normal (ED_GF_NORMAL.f90:676-677) pole by pole
    beta = 50.0
    e, zv = np.linalg.eigh(T)
    nu = 2 * np.pi * np.arange(8) / beta
    want = sum(-(norm2 * zv[0, j] ** 2 / zeta) * (1 - np.exp(-beta * (e[j] - e_state))) * 2 * (e[j] - e_state) /
               (nu ** 2 + (e[j] - e_state) ** 2) for j in range(n))
    got = phonon_gf(a, b, norm2, e_state, 1j * nu, zeta=zeta, beta=beta)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def test_null_handle_is_refused_with_a_message(built):
    lib = capi.lib()
    buf = np.zeros(16)
    assert lib.edigpu_apply_xph(None, None, None, None) != 0
    assert "edigpu_apply_xph" in capi.last_error() and "NULL" in capi.last_error()
    assert lib.edigpu_ph_rdm(None, None, 1, capi.pd(buf), capi.pd(buf)) != 0
    assert "edigpu_ph_rdm" in capi.last_error() and "NULL" in capi.last_error()
    assert lib.edigpu_time_ph(None, None, None, 0, 1, capi.pd(buf)) != 0
    assert "edigpu_time_ph" in capi.last_error()
