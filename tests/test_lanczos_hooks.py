"""The edigpu_lzk_* test hooks (csrc/hooks/lanczos_hooks.hip) check their arguments before they touch the device: null
buffers, buffers shorter than what the launcher reads or writes, a width other than 2 / 4 / 8, more vectors than columns,
scalar blocks that overlap, an exchange geometry that does not hold the shard -- all refused with a message, not by a
crash.  CPU only; and the hook source adds no kernel, so it stays outside the sources capi.kernel_source_hash() covers."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from edipack_amd import capi

V = np.ones(4096)
S = np.zeros(64)


def _b(a, n):
    return (capi.pd(a) if a is not None else None, n)


def norm_begin(n=5, v=V, vlen=5, plen=1, slen=8):
    return capi.lib().edigpu_lzk_norm_begin(n, *_b(v, vlen), *_b(V, plen), *_b(S, slen))


def rotate(lazy=0, n=5, vinlen=5, vout=V, voutlen=5, slen=8):
    return capi.lib().edigpu_lzk_rotate(lazy, n, *_b(V, vinlen), *_b(vout, voutlen), *_b(S, slen))


def next_vector(n=5, plen=5, qlen=5, xlen=5, slen=8):
    return capi.lib().edigpu_lzk_next_vector(1, n, *_b(V, plen), *_b(V, qlen), *_b(V, xlen), *_b(S, slen))


def alpha(n=5, vinlen=5, voutlen=5, tmplen=5, plen=1, slen=20, it=0, nlanc=6):
    return capi.lib().edigpu_lzk_alpha(n, *_b(V, vinlen), *_b(V, voutlen), *_b(V, tmplen), *_b(V, plen), *_b(S, slen), it, nlanc)


def beta(n=5, vinlen=5, voutlen=5, plen=1, slen=20, it=0, nlanc=6):
    return capi.lib().edigpu_lzk_beta(n, *_b(V, vinlen), *_b(V, voutlen), *_b(V, plen), *_b(S, slen), it, nlanc)


def add_dot3(n=600, plen=600, qlen=600, tmplen=600, slen=8, partlen=9, np_=True):
    cnt = C.c_int32(0)
    return capi.lib().edigpu_lzk_add_dot3(n, *_b(V, plen), *_b(V, qlen), *_b(V, tmplen), *_b(S, slen), *_b(V, partlen),
                                          C.byref(cnt) if np_ else None)


def axpy(n=5, acclen=5, vinlen=5, slen=8):
    return capi.lib().edigpu_lzk_axpy(n, *_b(V, acclen), *_b(V, vinlen), 0.5, *_b(S, slen), 0)


def blocked(to=1, du=10, dd=3, shift=2, srclen=30, dstlen=36):
    return capi.lib().edigpu_lzk_blocked(to, du, dd, shift, *_b(V, srclen), *_b(V, dstlen))


T3 = np.array([0.5, 2.3125, 1.0])


def shard_rotate3(first=0, n=30, du=10, q=4, world=2, pcol=5, halo=1, vinlen=30, voutlen=30, t=T3, send=V, sendlen=56):
    return capi.lib().edigpu_lzk_shard_rotate3(first, n, du, q, world, pcol, halo, *_b(V, vinlen), *_b(V, voutlen),
                                               capi.pd(t) if t is not None else None, None, *_b(send, sendlen))


def shard_add_dot3(n=30, du=10, q=4, world=2, pcol=5, halo=1, vinlen=30, voutlen=30, tmplen=30, back=V, backlen=56,
                   worklen=3072, sumslen=3):
    return capi.lib().edigpu_lzk_shard_add_dot3(n, du, q, world, pcol, halo, *_b(V, vinlen), *_b(V, voutlen), *_b(V, tmplen),
                                                *_b(back, backlen), None, *_b(V, worklen), *_b(S, sumslen))


def panel_rotate(n2=5, xlen=10, vlen=10, t=T3):
    return capi.lib().edigpu_lzk_panel_rotate(n2, *_b(V, xlen), *_b(V, vlen), capi.pd(t) if t is not None else None, None)


def panel_add_dot(n2=5, xlen=10, vdstlen=10, rowlen=10, collen=10, t=None, tprev=None, worklen=3072, sumslen=3):
    return capi.lib().edigpu_lzk_panel_add_dot(n2, *_b(V, xlen), *_b(V, vdstlen), *_b(V, rowlen), *_b(V, collen),
                                               capi.pd(t) if t is not None else None,
                                               capi.pd(tprev) if tprev is not None else None, *_b(V, worklen), *_b(S, sumslen))


def interleave(to=1, W=4, cplx=0, nrow=5, g=3, srclen=15, dstlen=20):
    return capi.lib().edigpu_lzk_interleave(to, W, cplx, nrow, g, *_b(V, srclen), *_b(V, dstlen))


def norm_begin_multi(W=4, cplx=0, nrow=5, plen=20, partlen=4, slen=38, sstride=10):
    return capi.lib().edigpu_lzk_norm_begin_multi(W, cplx, nrow, *_b(V, plen), *_b(V, partlen), *_b(S, slen), sstride)


def rotate_lazy_multi(W=4, cplx=0, nrow=5, plen=20, qlen=20, slen=38, sstride=10):
    return capi.lib().edigpu_lzk_rotate_lazy_multi(W, cplx, nrow, *_b(V, plen), *_b(V, qlen), *_b(S, slen), sstride)


def finalize_ab_multi(W=2, cplx=0, nrow=5, plen=10, qlen=10, partlen=18, np_=3, scal=S, slen=42, sstride=22, nlanc=6):
    return capi.lib().edigpu_lzk_finalize_ab_multi(W, cplx, nrow, *_b(V, plen), *_b(V, qlen), *_b(V, partlen), np_, *_b(scal, slen),
                                                   sstride, nlanc)


NEG = S.copy()
NEG[22 + 3] = -1.0        # SC_NDONE of the second column

REFUSED = [
    (lambda: norm_begin(n=0), "negative or zero size"),
    (lambda: norm_begin(vlen=4), "v shorter than the vector length"),
    (lambda: norm_begin(v=None), "v shorter than the vector length"),
    (lambda: norm_begin(n=600, vlen=600, plen=2), "partial needs min(ceil(n / 256), 1024)"),
    (lambda: norm_begin(slen=7), "scal needs 8 doubles"),
    (lambda: rotate(n=-1), "negative or zero size"),
    (lambda: rotate(vinlen=4), "vin shorter than the vector length"),
    (lambda: rotate(lazy=1, voutlen=4), "vout shorter than the vector length"),
    (lambda: rotate(vout=None), "vout shorter than the vector length"),
    (lambda: rotate(slen=7), "scal needs 8 doubles"),
    (lambda: next_vector(n=0), "negative or zero size"),
    (lambda: next_vector(plen=4), "P shorter than the vector length"),
    (lambda: next_vector(qlen=4), "Q shorter than the vector length"),
    (lambda: next_vector(xlen=4), "X shorter than the vector length"),
    (lambda: next_vector(slen=0), "scal needs 8 doubles"),
    (lambda: alpha(nlanc=0), "negative or zero size"),
    (lambda: alpha(it=6), "iter is not a step below nlanc"),
    (lambda: alpha(it=-1), "iter is not a step below nlanc"),
    (lambda: alpha(vinlen=4), "vin shorter than the vector length"),
    (lambda: alpha(voutlen=4), "vout shorter than the vector length"),
    (lambda: alpha(tmplen=4), "tmp shorter than the vector length"),
    (lambda: alpha(plen=0), "partial needs min(ceil(n / 256), 1024)"),
    (lambda: alpha(slen=19), "scal needs 8 + 2 * nlanc doubles"),
    (lambda: beta(n=0), "negative or zero size"),
    (lambda: beta(it=6), "iter is not a step below nlanc"),
    (lambda: beta(vinlen=4), "vin shorter than the vector length"),
    (lambda: beta(voutlen=4), "vout shorter than the vector length"),
    (lambda: beta(plen=0), "partial needs min(ceil(n / 256), 1024)"),
    (lambda: beta(slen=19), "scal needs 8 + 2 * nlanc doubles"),
    (lambda: add_dot3(n=0), "negative or zero size"),
    (lambda: add_dot3(plen=599), "P shorter than the vector length"),
    (lambda: add_dot3(qlen=599), "Q shorter than the vector length"),
    (lambda: add_dot3(tmplen=599), "tmp shorter than the vector length"),
    (lambda: add_dot3(slen=7), "scal needs 8 doubles"),
    (lambda: add_dot3(partlen=8), "partial needs 3 * min(ceil(n / 256), 1024)"),
    (lambda: add_dot3(np_=False), "null np"),
    (lambda: axpy(n=0), "negative or zero size"),
    (lambda: axpy(acclen=4), "acc shorter than the vector length"),
    (lambda: axpy(vinlen=4), "vin shorter than the vector length"),
    (lambda: axpy(slen=7), "scal needs 8 doubles"),
    (lambda: blocked(du=0), "negative or zero size"),
    (lambda: blocked(dd=-1), "negative or zero size"),
    (lambda: blocked(shift=-1), "shift out of range"),
    (lambda: blocked(shift=17), "shift out of range"),
    (lambda: blocked(srclen=29), "src shorter than its layout"),
    (lambda: blocked(dstlen=35), "dst shorter than its layout"),
    (lambda: blocked(to=0, srclen=35, dstlen=30), "src shorter than its layout"),
    (lambda: blocked(to=0, srclen=36, dstlen=29), "dst shorter than its layout"),
    (lambda: shard_rotate3(n=0), "negative or zero size"),
    (lambda: shard_rotate3(vinlen=29), "vin shorter than the vector length"),
    (lambda: shard_rotate3(voutlen=29), "vout shorter than the vector length"),
    (lambda: shard_rotate3(t=None), "a later step needs the sums t"),
    (lambda: shard_rotate3(du=0), "negative or zero size"),
    (lambda: shard_rotate3(halo=-1), "negative or zero size"),
    (lambda: shard_rotate3(du=7), "n is not a whole number of rows"),
    (lambda: shard_rotate3(q=2), "nrows > q"),
    (lambda: shard_rotate3(pcol=4), "pcol * world < dim_up"),
    (lambda: shard_rotate3(sendlen=55), "send needs world * q * (pcol + 2 * halo)"),
    (lambda: shard_add_dot3(n=0), "negative or zero size"),
    (lambda: shard_add_dot3(vinlen=29), "vin shorter than the vector length"),
    (lambda: shard_add_dot3(voutlen=29), "vout shorter than the vector length"),
    (lambda: shard_add_dot3(tmplen=29), "tmp shorter than the vector length"),
    (lambda: shard_add_dot3(q=2), "nrows > q"),
    (lambda: shard_add_dot3(world=1), "pcol * world < dim_up"),
    (lambda: shard_add_dot3(backlen=55), "back needs world * q * (pcol + 2 * halo)"),
    (lambda: shard_add_dot3(worklen=3071), "work needs 3 * 1024 doubles"),
    (lambda: shard_add_dot3(sumslen=2), "sums needs 3 doubles"),
    (lambda: panel_rotate(n2=0), "negative or zero size"),
    (lambda: panel_rotate(xlen=9), "x shorter than 2 * n2 doubles"),
    (lambda: panel_rotate(vlen=9), "v shorter than 2 * n2 doubles"),
    (lambda: panel_rotate(t=None), "null sums t"),
    (lambda: panel_add_dot(n2=0), "negative or zero size"),
    (lambda: panel_add_dot(xlen=9), "x shorter than 2 * n2 doubles"),
    (lambda: panel_add_dot(vdstlen=9), "vdst shorter than 2 * n2 doubles"),
    (lambda: panel_add_dot(rowlen=9), "rowhalf shorter than 2 * n2 doubles"),
    (lambda: panel_add_dot(collen=9), "colhalf shorter than 2 * n2 doubles"),
    (lambda: panel_add_dot(tprev=T3), "tprev without t"),
    (lambda: panel_add_dot(worklen=3071), "work needs 3 * 1024 doubles"),
    (lambda: panel_add_dot(sumslen=2), "sums needs 3 doubles"),
    (lambda: interleave(W=3), "width must be 2, 4 or 8"),
    (lambda: interleave(W=16), "width must be 2, 4 or 8"),
    (lambda: interleave(nrow=0), "negative or zero size"),
    (lambda: interleave(g=5), "g > W"),
    (lambda: interleave(g=-1), "g > W"),
    (lambda: interleave(srclen=14), "src shorter than its layout"),
    (lambda: interleave(dstlen=19), "dst shorter than its layout"),
    (lambda: interleave(cplx=1, srclen=29, dstlen=40), "src shorter than its layout"),
    (lambda: interleave(to=0, srclen=19, dstlen=15), "src shorter than its layout"),
    (lambda: interleave(to=0, srclen=20, dstlen=14), "dst shorter than its layout"),
    (lambda: norm_begin_multi(W=1), "width must be 2, 4 or 8"),
    (lambda: norm_begin_multi(nrow=0), "negative or zero size"),
    (lambda: norm_begin_multi(plen=19), "P shorter than W interleaved columns"),
    (lambda: norm_begin_multi(cplx=1, plen=39), "P shorter than W interleaved columns"),
    (lambda: norm_begin_multi(partlen=3), "partial needs W * min(ceil(len / 256), 1024)"),
    (lambda: norm_begin_multi(sstride=7), "sstride smaller than the scalar block"),
    (lambda: norm_begin_multi(slen=37), "scal shorter than W blocks at sstride"),
    (lambda: rotate_lazy_multi(W=6), "width must be 2, 4 or 8"),
    (lambda: rotate_lazy_multi(nrow=-3), "negative or zero size"),
    (lambda: rotate_lazy_multi(plen=19), "P shorter than W interleaved columns"),
    (lambda: rotate_lazy_multi(qlen=19), "Q shorter than W interleaved columns"),
    (lambda: rotate_lazy_multi(sstride=0), "sstride smaller than the scalar block"),
    (lambda: rotate_lazy_multi(slen=37), "scal shorter than W blocks at sstride"),
    (lambda: finalize_ab_multi(W=0), "width must be 2, 4 or 8"),
    (lambda: finalize_ab_multi(np_=0), "negative or zero size"),
    (lambda: finalize_ab_multi(nlanc=0), "negative or zero size"),
    (lambda: finalize_ab_multi(plen=9), "P shorter than W interleaved columns"),
    (lambda: finalize_ab_multi(qlen=9), "Q shorter than W interleaved columns"),
    (lambda: finalize_ab_multi(partlen=17), "partial needs 3 * W * np doubles"),
    (lambda: finalize_ab_multi(sstride=19), "sstride smaller than the scalar block"),
    (lambda: finalize_ab_multi(slen=41), "scal shorter than W blocks at sstride"),
    (lambda: finalize_ab_multi(scal=NEG), "a column's step count is negative"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_bad_arguments_are_refused_with_a_message(built, k):
    call, message = REFUSED[k]
    capi.lib().edigpu_info(None, None)           # leaves another message behind
    assert call() != 0
    assert "edigpu_lzk_" in capi.last_error() and message in capi.last_error()


GOOD = (norm_begin, rotate, next_vector, alpha, beta, add_dot3, axpy, blocked, shard_rotate3, shard_add_dot3, panel_rotate,
        panel_add_dot, interleave, norm_begin_multi, rotate_lazy_multi, finalize_ab_multi,
        lambda: shard_rotate3(first=1, t=None, send=None, sendlen=0), lambda: shard_add_dot3(back=None, backlen=0),
        lambda: panel_add_dot(t=T3, tprev=T3), lambda: blocked(to=0, srclen=36, dstlen=30),
        lambda: interleave(to=0, srclen=20, dstlen=15))


def test_good_arguments_reach_the_device_check(built):
    """the same calls with nothing wrong get as far as the device: without one they fail for that reason alone"""
    for call in GOOD:
        if capi.device_count() > 0:
            assert call() == 0, capi.last_error()
        else:
            assert call() != 0 and "no usable HIP device" in capi.last_error()


def test_hook_source_is_outside_the_kernel_source_hash(built):
    """test hooks that add no kernel must not invalidate the stamp of profiles/pmc_traffic.json: neither the hook source
    nor the header the hook files share lies among the hashed sources, and none of those names a hook"""
    csrc = os.path.join(capi.HERE, "csrc")
    hashed = glob.glob(os.path.join(csrc, "*.h*")) + glob.glob(os.path.join(csrc, "*.cpp"))
    assert hashed
    for name in ("lanczos_hooks.hip", "hook_util.hpp"):
        assert os.path.exists(os.path.join(csrc, "hooks", name))
        assert not any(os.path.basename(f) == name for f in hashed)
    assert "__global__" not in open(os.path.join(csrc, "hooks", "lanczos_hooks.hip")).read()
    for f in hashed:
        assert "edigpu_lzk_" not in open(f).read(), f
