"""The edigpu_trl_* test hooks (csrc/hooks/trl_hooks.hip) check their arguments before they touch the device: negative
sizes, buffers shorter than what the launcher reads or writes, an h below 2 * 16 * ceil(ndot / 16) doubles and ldq < len
with more than one column are refused with a message, not by a crash.  CPU only; and the hook source adds no kernel, so
it stays outside the sources capi.kernel_source_hash() covers."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from edipack_amd import capi

Q = np.ones(64)
W = np.ones(16)
H = np.zeros(80)


def dots(cplx=0, n=5, ndot=2, ncol=2, ldq=5, qlen=10, wlen=5, w_col=-1, hlen=32, skip=-1, w=W):
    return capi.lib().edigpu_trl_dots(cplx, n, ndot, capi.pd(Q), ncol, ldq, qlen, capi.pd(w) if w is not None else None, wlen,
                                      w_col, capi.pd(H), hlen, skip)


def subtract(cplx=0, n=5, nvec=2, ncol=2, ldq=5, qlen=10, hlen=4, wlen=5, skip=-1):
    return capi.lib().edigpu_trl_subtract(cplx, n, nvec, capi.pd(Q), ncol, ldq, qlen, capi.pd(H), hlen, capi.pd(W), wlen, skip)


def rotate(ln=5, m=2, k=2, ldq=5, qlen=10, ldy=2, ylen=4, ldo=5, olen=10):
    return capi.lib().edigpu_trl_rotate(ln, m, k, capi.pd(Q), ldq, qlen, capi.pd(W), ldy, ylen, capi.pd(H), ldo, olen)


def decide(hlen=6, nvec=2, hflen=4, skip=True):
    s = C.c_int32(0)
    return capi.lib().edigpu_trl_decide(capi.pd(H), hlen, nvec, 0.5, 1e-6, capi.pd(H), hflen, C.byref(s) if skip else None)


REFUSED = [
    (lambda: dots(n=-1), "negative or zero size"),
    (lambda: dots(n=0), "negative or zero size"),
    (lambda: dots(ndot=0), "negative or zero size"),
    (lambda: dots(qlen=-1), "negative or zero size"),
    (lambda: dots(ldq=-5), "negative or zero size"),
    (lambda: dots(ldq=4), "leading dimension below the vector length"),
    (lambda: dots(cplx=1, ldq=9, qlen=20, wlen=10), "leading dimension below the vector length"),
    (lambda: dots(qlen=9), "matrix buffer too short"),
    (lambda: dots(ndot=3, hlen=32), "more dots than columns"),
    (lambda: dots(hlen=31), "2 * 16 * ceil(ndot / 16)"),
    (lambda: dots(ndot=17, ncol=17, ldq=1, n=1, qlen=17, hlen=63), "2 * 16 * ceil(ndot / 16)"),
    (lambda: dots(hlen=-1), "2 * 16 * ceil(ndot / 16)"),
    (lambda: dots(wlen=4), "w shorter than the vector length"),
    (lambda: dots(w=None), "w shorter than the vector length"),
    (lambda: dots(w_col=2), "w_col is not a column of Q"),
    (lambda: dots(skip=2), "skip is -1, 0 or 1"),
    (lambda: capi.lib().edigpu_trl_norm2(0, 5, capi.pd(W), 4, capi.pd(H), 32), "w shorter than the vector length"),
    (lambda: capi.lib().edigpu_trl_norm2(1, 5, capi.pd(W), 9, capi.pd(H), 32), "w shorter than the vector length"),
    (lambda: capi.lib().edigpu_trl_norm2(0, 5, capi.pd(W), 5, capi.pd(H), 31), "h needs 2 * 16 doubles"),
    (lambda: capi.lib().edigpu_trl_norm2(0, -5, capi.pd(W), 5, capi.pd(H), 32), "negative or zero size"),
    (lambda: subtract(n=-1), "negative or zero size"),
    (lambda: subtract(ldq=4), "leading dimension below the vector length"),
    (lambda: subtract(qlen=9), "matrix buffer too short"),
    (lambda: subtract(nvec=3), "more coefficients than columns"),
    (lambda: subtract(hlen=3), "h needs 2 * nvec doubles"),
    (lambda: subtract(wlen=4), "w shorter than the vector length"),
    (lambda: subtract(skip=-2), "skip is -1, 0 or 1"),
    (lambda: decide(nvec=0), "negative or zero size"),
    (lambda: decide(hlen=5), "h needs 2 * nvec + 2 doubles"),
    (lambda: decide(hflen=3), "hf needs 2 * nvec doubles"),
    (lambda: decide(skip=False), "null skip"),
    (lambda: capi.lib().edigpu_trl_filter(capi.pd(H), 5, 2, 1e-6), "h needs 2 * nvec + 2 doubles"),
    (lambda: capi.lib().edigpu_trl_filter(capi.pd(H), 6, -2, 1e-6), "negative or zero size"),
    (lambda: rotate(ln=0), "negative or zero size"),
    (lambda: rotate(m=-1), "negative or zero size"),
    (lambda: rotate(ldq=4), "leading dimension below the vector length"),
    (lambda: rotate(ldo=4), "leading dimension below the vector length"),
    (lambda: rotate(qlen=9), "matrix buffer too short"),
    (lambda: rotate(olen=9), "matrix buffer too short"),
    (lambda: rotate(ldy=1), "Y needs (m - 1) * ldy + k doubles"),
    (lambda: rotate(ylen=3), "Y needs (m - 1) * ldy + k doubles"),
    (lambda: capi.lib().edigpu_trl_scale(0, capi.pd(W), 5, 2.0), "negative or zero size"),
    (lambda: capi.lib().edigpu_trl_scale(5, capi.pd(W), 4, 2.0), "v shorter than the vector length"),
    (lambda: capi.lib().edigpu_trl_scale(5, None, 5, 2.0), "v shorter than the vector length"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_bad_arguments_are_refused_with_a_message(built, k):
    call, message = REFUSED[k]
    capi.lib().edigpu_info(None, None)           # leaves another message behind
    assert call() != 0
    assert "edigpu_trl_" in capi.last_error() and message in capi.last_error()


def test_good_arguments_reach_the_device_check(built):
    """the same calls with nothing wrong get as far as the device: without one they fail for that reason alone"""
    if capi.device_count() > 0:
        assert dots() == 0 and subtract() == 0 and rotate() == 0 and decide() == 0
    else:
        for call in (dots, subtract, rotate, decide):
            assert call() != 0 and "no usable HIP device" in capi.last_error()


def test_hook_source_is_outside_the_kernel_source_hash(built):
    """a test hook that adds no kernel must not invalidate the stamp of profiles/pmc_traffic.json"""
    csrc = os.path.join(capi.HERE, "csrc")
    hashed = glob.glob(os.path.join(csrc, "*.h*")) + glob.glob(os.path.join(csrc, "*.cpp"))
    assert hashed and os.path.exists(os.path.join(csrc, "hooks", "trl_hooks.hip"))
    assert not any("trl_hooks" in os.path.basename(f) for f in hashed)
    for f in hashed:
        assert "edigpu_trl_" not in open(f).read(), f
