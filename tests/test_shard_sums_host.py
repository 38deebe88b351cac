"""CPU test of the one definition of alpha / beta of the one-reduction Lanczos recurrence from its three sums
(csrc/lanczos_sums.hpp, through tests/shard_sums_host.cpp): the function the shard kernels (csrc/kernels_shard.hip), the
in-kernel finalize (csrc/lz_finalize.hpp) and the host loop of sharded_tridiag (csrc/edigpu_shard.hip) share, compiled
as plain C++ with g++ and compared with the same identity evaluated in long double.

The formula is a fixed sequence of double operations (no contraction into fused multiply-adds), so its error on given
inputs is reproducible.  MEASURED below is the relative error the host copy of the formula had on each case before it
was moved into the shared header (beta^2, beta; in units of eps = 2^-52); a case passes when its error is at most 4 x
that figure, with a floor of 4 eps."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, VP = C.c_double, C.c_void_p
EPS = float(np.finfo(np.float64).eps)

# name -> (alpha = <v|w>, qq = sum (w - sg v)^2, vv = <v|v>, sg = the previous alpha; 0 on the first step)
CASES = {
    "first_step_unit_seed": (0.3, 1.7, 1.0, 0.0),
    "first_step_unnormalised": (0.9, 3.1, 2.0, 0.0),
    "generic_step": (0.25, 2.2, 1.0, -0.4),
    "norm_off_by_1e-10": (-1.3, 5.0, 1.0000000001, 0.7),
    "alpha_equals_shift": (0.7, 0.81, 1.0, 0.7),
    # a spectrum far from zero: alpha ~ sg ~ 1e6, beta ~ 1, <v|v> one ulp above 1
    "far_spectrum": (1.0e6 + 0.37, 1.0625, 1.0 + EPS, 1.0e6 + 0.12),
    "far_spectrum_negative": (-1.0e6 - 0.41, 0.9 + 0.2809, 1.0 - EPS / 2, -1.0e6 + 0.12),
}
# relative error of (beta^2, beta) in eps, measured once with the host formula of sharded_tridiag as it stood.  The two
# far-spectrum cases: sg * <v|v> is rounded at 1e6 (half an ulp = 6e-11) and multiplied by 2 d ~ 1, i.e. ~1e-11 of beta^2 ~ 1
MEASURED = {
    "first_step_unit_seed": (0.38, 0.48),
    "first_step_unnormalised": (0.0, 0.03),
    "generic_step": (0.17, 0.42),
    "norm_off_by_1e-10": (0.0, 0.0),
    "alpha_equals_shift": (0.0, 0.04),
    "far_spectrum": (24319.94, 12159.97),
    "far_spectrum_negative": (28643.43, 14321.67),
}
# w = alpha v exactly, so beta^2 = 0; qq one ulp short of d^2 <v|v> makes the difference negative: beta = 0, not NaN
NEGATIVE = (0.5, 0.0625 * (1.0 - EPS), 1.0, 0.25)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("shard_sums") / "shard_sums_host.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    # (-ffp-contract=off: as the library is built)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", csrc, "-o", so,
                           os.path.join(ROOT, "tests", "shard_sums_host.cpp")])
    lib = C.CDLL(so)
    lib.ss_ab_from_sums.argtypes = [VP, VP, VP, VP]
    lib.ss_ab_from_sums.restype = None
    for name, nargs in (("ss_beta2_from_sums", 4), ("ss_beta_from_beta2", 1), ("ss_ref_beta2", 4), ("ss_relerr_beta2", 5),
                        ("ss_relerr_beta", 5)):
        getattr(lib, name).argtypes = [D] * nargs
        getattr(lib, name).restype = D
    return lib


def ab_from_sums(lib, alpha, qq, vv, sg, first):
    """(alpha, beta) as the kernels get them: t = this step's sums, tprev = the previous step's (null on the first)"""
    t = np.array([alpha, qq, vv])
    tprev = np.array([sg, 0.0, 0.0])
    out = np.zeros(2)
    lib.ss_ab_from_sums(t.ctypes.data_as(VP), None if first else tprev.ctypes.data_as(VP), out.ctypes.data_as(VP),
                        out[1:].ctypes.data_as(VP))
    return float(out[0]), float(out[1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_beta_against_long_double(shim, name):
    alpha, qq, vv, sg = CASES[name]
    b2 = shim.ss_beta2_from_sums(alpha, qq, vv, sg)
    a, b = ab_from_sums(shim, alpha, qq, vv, sg, first=name.startswith("first_step"))
    assert a == alpha
    assert b == shim.ss_beta_from_beta2(b2) == np.sqrt(b2), "ab_from_sums is the two pieces the host loop uses"
    err2 = shim.ss_relerr_beta2(b2, alpha, qq, vv, sg) / EPS
    err = shim.ss_relerr_beta(b, alpha, qq, vv, sg) / EPS
    print(f"{name}: beta^2 = {b2!r} beta = {b!r} relative error {err2:.3f} eps, {err:.3f} eps (measured "
          f"{MEASURED[name][0]}, {MEASURED[name][1]})")
    assert err2 <= max(4.0 * MEASURED[name][0], 4.0), (name, err2)
    assert err <= max(4.0 * MEASURED[name][1], 4.0), (name, err)


def test_first_step_ignores_the_previous_sums(shim):
    """tprev = null means sg = 0, whatever a stale slot would hold"""
    alpha, qq, vv, _ = CASES["first_step_unit_seed"]
    assert ab_from_sums(shim, alpha, qq, vv, 123.0, first=True) == ab_from_sums(shim, alpha, qq, vv, 0.0, first=False)


def test_negative_beta2_from_rounding_gives_beta_zero(shim):
    alpha, qq, vv, sg = NEGATIVE
    b2 = shim.ss_beta2_from_sums(alpha, qq, vv, sg)
    assert b2 < 0.0 and shim.ss_ref_beta2(alpha, qq, vv, sg) < 0.0, "the case is meant to be negative"
    a, b = ab_from_sums(shim, alpha, qq, vv, sg, first=False)
    assert a == alpha
    assert b == 0.0 and not np.signbit(b)
