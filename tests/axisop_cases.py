"""Shared helpers of the one-axis c / c^+ tests (tests/test_axisop_host.py, tests/test_gpu_axisop.py): forward numpy
restatements on the sector maps.  A partner table is made the way the reference applies the operator: loop over the source
states, flip the bit, apply the sign, rank in the destination."""
from __future__ import annotations

import numpy as np

NONE = np.uint32(0xFFFFFFFF)
U = 2.0 ** -53


def comb_words(nlev: int, n: int) -> np.ndarray:
    """the ascending nlev-bit words with n bits set: the basis of a species (ed_total_ud=T) or of a chain (ed_total_ud=F)"""
    return np.array([w for w in range(1 << nlev) if bin(w).count("1") == n], dtype=np.int64)


def forward_table(src_words, dst_words, level: int, create: bool, counted: bool) -> np.ndarray:
    """part[j] = source index | minus << 31 of destination word j, NONE without a preimage"""
    rank = {int(w): j for j, w in enumerate(dst_words)}
    part = np.full(len(dst_words), NONE, dtype=np.uint32)
    bit = 1 << level
    for i, w in enumerate(src_words):
        w = int(w)
        if bool(w & bit) == bool(create):
            continue                      # c on an empty level, c^+ on a full one
        minus = counted and (bin(w & (bit - 1)).count("1") & 1)
        part[rank[w ^ bit]] = np.uint32(i | (0x80000000 if minus else 0))
    return part


def signed_gather(part: np.ndarray, src3: np.ndarray) -> np.ndarray:
    """x[o][j][i] = +-src3[o][part[j]][i], 0.0 without a preimage (src3: [O][A_src][I])"""
    live = part != NONE
    idx = (part & np.uint32(0x7FFFFFFF)).astype(np.int64)
    x = np.zeros((src3.shape[0], part.size, src3.shape[2]), dtype=src3.dtype)
    x[:, live, :] = src3[:, idx[live], :]
    x[:, live & ((part >> np.uint32(31)) == 1), :] *= -1.0
    return x


def orbs_shape(dims, axis: int):
    """(I, A, O) of axis `axis` of an ed_total_ud=F sector with the per-axis dimensions dims (axis 0 fastest)"""
    i = int(np.prod(dims[:axis], dtype=np.int64))
    o = int(np.prod(dims[axis + 1:], dtype=np.int64))
    return i, int(dims[axis]), o


def fma(c: float, x: np.ndarray, acc: np.ndarray) -> np.ndarray:
    """round(c * x + acc) with ONE rounding, element by element: math.fma where Python has it, else exact rationals
    (Fraction -> float rounds to nearest even, as the hardware does)"""
    import math
    if abs(c) == 1.0:
        return c * x + acc                 # the product is exact: one rounding as it stands
    out = np.array(acc, dtype=np.float64, copy=True)
    xf, of = np.ascontiguousarray(x).reshape(-1), out.reshape(-1)
    todo = np.nonzero(xf != 0.0)[0]        # c * 0 + acc = acc (up to the sign of a zero)
    if hasattr(math, "fma"):
        for k in todo:
            of[k] = math.fma(c, float(xf[k]), float(of[k]))
    else:
        from fractions import Fraction
        fc = Fraction(c)
        for k in todo:
            of[k] = float(fc * Fraction(float(xf[k])) + Fraction(float(of[k])))
    return out


def real_chain(coefs, xs):
    """acc = coef_0 x_0, then acc = fma(coef_t, x_t, acc), t ascending: the arithmetic kernels_axisop.hip states"""
    acc = float(coefs[0]) * xs[0]
    for c, x in zip(coefs[1:], xs[1:]):
        acc = fma(float(c), x, acc)
    return acc


def cplx_chain(coefs, xs):
    """y_t = (cre x.re - cim x.im, cre x.im + cim x.re), every product and every sum rounded; acc = y_0, then
    acc = y_t + acc per component: the arithmetic of apply_op_flat_kernel"""
    acc = None
    for c, x in zip(coefs, xs):
        c = complex(c)
        y = np.empty(x.shape, dtype=np.complex128)
        y.real = c.real * x.real - c.imag * x.imag
        y.imag = c.real * x.imag + c.imag * x.real
        if acc is None:
            acc = y
        else:
            nxt = np.empty_like(y)
            nxt.real = y.real + acc.real
            nxt.imag = y.imag + acc.imag
            acc = nxt
    return acc
