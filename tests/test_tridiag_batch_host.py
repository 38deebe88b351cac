"""edigpu_apply_multi_dev / edigpu_lanczos_tridiag_batch_dev reject bad arguments with "bad argument" before any device
work: no GPU needed.  The handle and the pointers of the cases that test a count are dummies that are never read."""
import ctypes as C

import numpy as np
import pytest

from edipack_amd import capi


@pytest.fixture()
def dummies():
    buf = np.zeros(64)
    out = np.zeros(64)
    return C.c_void_p(buf.ctypes.data), C.c_void_p(out.ctypes.data), buf, out


def _bad(rc):
    assert rc != 0
    assert "bad argument" in capi.last_error()


def test_apply_multi_rejects_bad_arguments(built, dummies):
    L = capi.lib()
    x, y, _, _ = dummies
    fake = x  # never dereferenced: the counts and pointers are checked first
    _bad(L.edigpu_apply_multi_dev(None, 2, x, y, None))
    assert "edigpu_apply_multi_dev" in capi.last_error()
    _bad(L.edigpu_apply_multi_dev(fake, 0, x, y, None))
    _bad(L.edigpu_apply_multi_dev(fake, -3, x, y, None))
    _bad(L.edigpu_apply_multi_dev(fake, 2, None, y, None))
    _bad(L.edigpu_apply_multi_dev(fake, 2, x, None, None))


def test_tridiag_batch_rejects_bad_arguments(built, dummies):
    L = capi.lib()
    x, _, _, _ = dummies
    fake = x
    a, b = np.zeros(8), np.zeros(8)
    nd = (C.c_int * 2)()
    n2 = np.zeros(2)
    route = C.c_int(7)
    args = dict(h=fake, nseed=2, vin=x, nlanc=4, a=capi.pd(a), b=capi.pd(b), nd=nd, n2=capi.pd(n2))

    def call(**kw):
        p = dict(args, **kw)
        return L.edigpu_lanczos_tridiag_batch_dev(p["h"], p["nseed"], p["vin"], p["nlanc"], p["a"], p["b"], 1e-12, p["nd"],
                                                  p["n2"], C.byref(route))

    _bad(call(h=None))
    assert "edigpu_lanczos_tridiag_batch_dev" in capi.last_error()
    _bad(call(nseed=0))
    _bad(call(nseed=-1))
    _bad(call(nlanc=0))
    _bad(call(nlanc=-5))
    _bad(call(vin=None))
    _bad(call(a=None))
    _bad(call(b=None))
    assert not a.any() and not b.any() and route.value == 7  # nothing was written


def test_batch_set_width_rejects_bad_arguments(built, dummies):
    L = capi.lib()
    fake = dummies[0]  # only a valid width would touch the handle
    _bad(L.edigpu_batch_set_width(None, 2))
    for w in (-1, 1, 3, 5, 16):
        _bad(L.edigpu_batch_set_width(fake, w))


def test_python_class_has_the_batch_methods(built):
    from edipack_amd.hamiltonian import SectorHamiltonian
    assert callable(SectorHamiltonian.apply_multi_dev) and callable(SectorHamiltonian.lanczos_tridiag_batch_dev)
    assert {"edigpu_apply_multi_dev", "edigpu_lanczos_tridiag_batch_dev"} <= set(capi.SIGNATURES)
