"""CPU tests of the two dense eigensolvers behind every eigenvalue the library returns (csrc/host_dense.cpp, through
tests/host_dense.cpp): tql2 on the Lanczos tridiagonal matrix (edigpu_lanczos_eigh) and jacobi_eigh on the projection of
the thick-restart solver (trl_solve), against numpy.linalg.eigh (LAPACK) on the same matrix.

Every measure is in the max norm: the residual |A Z - Z L|, the orthogonality defect |Z^T Z - 1| and the difference of
the sorted eigenvalues to LAPACK's.  A measure passes when it is at most FACTOR * max(what LAPACK attains in the same
measure on the same matrix, n eps |A|), |A| = the largest |element| of A (LAPACK's eigenvalue difference to itself is 0:
that measure is held to the second term alone)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, I = C.c_void_p, C.c_int
EPS = np.finfo(np.float64).eps

# Worst ratio measure / max(LAPACK's, n eps |A|) over the cases below, measured once with the routines as they were
# moved out of the C-ABI source; the factor is the next power of two above it.
TQL2_FACTOR = 2.0      # worst observed: 1.04 (orthogonality, random_n3)
JACOBI_FACTOR = 4.0    # worst observed: 2.32 (eigenvalues, random_n40)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_dense") / "host_dense.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", so,
                           os.path.join(ROOT, "tests", "host_dense.cpp"), os.path.join(csrc, "host_dense.cpp")])
    lib = C.CDLL(so)
    lib.hd_tql2.argtypes = [I, VP, VP, VP]
    lib.hd_tql2.restype = I
    lib.hd_jacobi_eigh.argtypes = [I, VP, VP, VP]
    lib.hd_jacobi_eigh.restype = None
    return lib


def _ptr(a):
    return a.ctypes.data_as(VP)


def measures(A, lam, Z):
    """(residual, orthogonality defect) of eigenvalues lam and eigenvectors in the columns of Z"""
    n = A.shape[0]
    return float(np.max(np.abs(A @ Z - Z * lam[None, :]))), float(np.max(np.abs(Z.T @ Z - np.eye(n))))


def ratios(A, lam, Z):
    """the three measures over their allowance (module docstring); the eigenvalues in the order given"""
    n = A.shape[0]
    lam_ref, Z_ref = np.linalg.eigh(A)
    floor = n * EPS * float(np.max(np.abs(A)))
    res, orth = measures(A, lam, Z)
    res_ref, orth_ref = measures(A, lam_ref, Z_ref)
    dlam = float(np.max(np.abs(np.sort(lam) - lam_ref)))

    def over(x, allowance):
        return 0.0 if x == 0.0 else x / allowance

    out = {"residual": over(res, max(res_ref, floor)), "orthogonality": over(orth, max(orth_ref, floor)),
           "eigenvalues": over(dlam, floor)}
    print(f"n={n} |A|={np.max(np.abs(A)):.3e} residual {res:.3e} (LAPACK {res_ref:.3e}) orthogonality {orth:.3e} "
          f"(LAPACK {orth_ref:.3e}) eigenvalues {dlam:.3e} floor {floor:.3e} ratios {out}")
    return out


# ---- tql2 ----

def _tridiag_random(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), rng.standard_normal(max(n - 1, 0))


def _tql2_cases():
    cases = {f"random_n{n}": _tridiag_random(n, 100 + n) for n in (1, 2, 3, 20, 128)}  # 128: the cap of m in trl_solve
    d, e = _tridiag_random(20, 7)
    e[9] = 0.0
    cases["splits_in_the_middle"] = (d, e)
    # 2 x 2 blocks [[2, 1], [1, 2]]: the eigenvalues 1 and 3, six times each
    cases["repeated_eigenvalues"] = (np.full(12, 2.0), np.array([1.0, 0.0] * 5 + [1.0]))
    # Wilkinson's W21+: pairs of eigenvalues that agree to rounding without any zero off-diagonal
    cases["wilkinson_21"] = (np.abs(np.arange(-10, 11)).astype(float), np.ones(20))
    g = np.logspace(0, -8, 20)
    cases["graded_1_to_1e-8"] = (g, 0.1 * np.sqrt(g[:-1] * g[1:]))
    cases["e_all_zero"] = (np.array([3.0, -1.0, 2.0, 2.0, 0.5]), np.zeros(4))
    return cases


TQL2_CASES = _tql2_cases()


def run_tql2(lib, d, e):
    """eigenvalues (in tql2's order) and the matrix with eigenvector j in column j, read from z as documented"""
    n = len(d)
    dd = np.array(d, dtype=np.float64)
    ee = np.zeros(n)
    ee[1:] = e  # e[0] unused
    z = np.zeros(n * n)
    assert lib.hd_tql2(n, _ptr(dd), _ptr(ee), _ptr(z)) == 0
    return dd, z.reshape((n, n), order="F")  # column-major


def _tridiag_dense(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


@pytest.mark.parametrize("name", sorted(TQL2_CASES))
def test_tql2_against_lapack(shim, name):
    d, e = TQL2_CASES[name]
    lam, Z = run_tql2(shim, d, e)
    for what, r in ratios(_tridiag_dense(d, e), lam, Z).items():
        assert r <= TQL2_FACTOR, (name, what, r)


def test_tql2_eigenvectors_are_the_columns_of_column_major_z(shim):
    """edigpu_lanczos_eigh reads eigenvector j as z[j * n + k]: the other reading of z is no decomposition"""
    d, e = TQL2_CASES["random_n20"]
    A = _tridiag_dense(d, e)
    lam, Z = run_tql2(shim, d, e)
    assert ratios(A, lam, Z)["residual"] <= TQL2_FACTOR
    assert measures(A, lam, Z.T)[0] > 1e-3


# ---- jacobi_eigh ----

def _sym_random(n, seed):
    a = np.random.default_rng(seed).standard_normal((n, n))
    return 0.5 * (a + a.T)


def _jacobi_cases():
    cases = {f"random_n{n}": _sym_random(n, 200 + n) for n in (1, 2, 5, 40)}
    cases["diagonal_unsorted"] = np.diag([3.0, -1.0, 2.0, 0.5, 2.5])  # leaves the sweeps at once; the sort still runs
    q, _ = np.linalg.qr(np.random.default_rng(11).standard_normal((5, 5)))
    a = (q * np.array([1.0, 2.0, 2.0, 3.0, 5.0])[None, :]) @ q.T
    cases["degenerate_pair"] = 0.5 * (a + a.T)
    return cases


JACOBI_CASES = _jacobi_cases()


def run_jacobi(lib, A):
    """eigenvalues and the matrix with eigenvector j in column j, read from z as documented (row-major)"""
    n = A.shape[0]
    a = np.ascontiguousarray(A, dtype=np.float64).copy()
    w, z = np.zeros(n), np.zeros(n * n)
    lib.hd_jacobi_eigh(n, _ptr(a), _ptr(w), _ptr(z))
    return w, z.reshape((n, n))


@pytest.mark.parametrize("name", sorted(JACOBI_CASES))
def test_jacobi_eigh_against_lapack(shim, name):
    A = JACOBI_CASES[name]
    lam, Z = run_jacobi(shim, A)
    assert np.all(np.diff(lam) >= 0.0), "jacobi_eigh promises ascending eigenvalues"
    for what, r in ratios(A, lam, Z).items():
        assert r <= JACOBI_FACTOR, (name, what, r)


def test_jacobi_eigenvectors_are_the_columns_of_row_major_z(shim):
    """trl_solve reads component k of Ritz vector i as Y[k * m + i]: the other reading of z is no decomposition"""
    A = JACOBI_CASES["random_n5"]
    lam, Z = run_jacobi(shim, A)
    assert ratios(A, lam, Z)["residual"] <= JACOBI_FACTOR
    assert measures(A, lam, Z.T)[0] > 1e-3
