"""Case tables, hook wrappers and NumPy references of tests/test_gpu_trl_kernels.py: the multi-vector kernels of the
thick-restart eigensolver (csrc/kernels_trl.hip) driven one launcher at a time through the edigpu_trl_* test hooks.

Where the grid-stride loops change behaviour (1024 workgroups of 256 threads; real vectors are walked in pairs):
  * the loop of trl_mdot / trl_maxpy / trl_rotate / trl_scale wraps above 524 288 real or 262 144 complex elements,
  * trl_msum adds more than one partial per thread above 256 workgroups (131 072 real, 65 536 complex elements),
  * a second group of columns starts at the 17th basis vector.
"""
import ctypes as C

import numpy as np

EPS = 2.0 ** -53
GROUP = 16                     # kTrlNC: basis vectors per launch
SENT = 12345.678               # sentinel of buffers a launcher writes next to (finite: arithmetic on it would show)

REAL_N = (1, 2, 3, 511, 512, 513, 131073, 524288, 524289, 1100001)
CPLX_N = (1, 2, 255, 256, 257, 65537, 262144, 262145, 600001)
SMALL_MAX = 513
SMALL_COLS = (1, 2, 15, 16, 17, 32, 33, 129)
LARGE_COLS = (17,)             # a second group with nc = 1


def column_counts(n):
    return SMALL_COLS if n <= SMALL_MAX else LARGE_COLS


def vector_cases():
    """(cplx, n, pad): ldq = len + pad.  pad = 0 is the solver's case (odd real n: every other column starts 8 bytes off a
    16-byte boundary); pad = 3 for the sizes up to 513 and for 524 289."""
    out = []
    for cplx, shapes in ((0, REAL_N), (1, CPLX_N)):
        for n in shapes:
            out.append((cplx, n, 0))
            if n <= SMALL_MAX or n == 524289:
                out.append((cplx, n, 3))
    return out


SPIKES = (0, 1, 510, 511, 512, -2, -1, 524287, 524288)


def spike_positions(n):
    pos = []
    for i in SPIKES:
        i = n + i if i < 0 else i
        if 0 <= i < n and i not in pos:
            pos.append(i)
    return pos


ROTATE_M = (2, 20, 128)
ROTATE_K = (1, 16, 17, 64)
ROTATE_LEN = (1, 2, 3, 513)
ROTATE_LARGE = (524289, 20, 17)   # len, m, k
SCALE_LEN = (1, 2, 3, 513, 524289)


def rotate_cases():
    """(len, m, k, ldo - len)"""
    out = []
    for ln in ROTATE_LEN:
        for m in ROTATE_M:
            for k in ROTATE_K:
                out.append((ln, m, k, 0))
                if ln % 2:
                    out.append((ln, m, k, 1))
    ln, m, k = ROTATE_LARGE
    return out + [(ln, m, k, 0), (ln, m, k, 1)]


def dots_slots(ndot):
    """doubles trl_dots writes: all 2 * GROUP slots of every group of columns"""
    return 2 * GROUP * ((ndot + GROUP - 1) // GROUP)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- buffers ---------------------------------------------------------------------------------------------------------
def make_q(cols, ldq, tail=5):
    """cols (ncol, len) -> flat buffer with column c at c * ldq; the gaps and the tail hold NaN: Q is only read, and a read
    outside a column poisons the result"""
    ncol, ln = cols.shape
    buf = np.full((ncol - 1) * ldq + ln + tail, np.nan)
    for c in range(ncol):
        buf[c * ldq:c * ldq + ln] = cols[c]
    return buf


def with_tail(v, tail=5, fill=SENT):
    return np.concatenate([np.asarray(v, dtype=np.float64), np.full(tail, fill)])


def as_doubles(z):
    """complex vector(s) -> interleaved doubles along the last axis"""
    z = np.ascontiguousarray(z)
    return z.view(np.float64) if np.iscomplexobj(z) else z


def random_vectors(rng, cplx, shape):
    if cplx:
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return rng.standard_normal(shape)


# ---- hook wrappers -----------------------------------------------------------------------------------------------------
def _capi():
    from edipack_amd import capi
    return capi


def hook_dots(cplx, n, ndot, qbuf, ncol, ldq, w, w_col, h, skip=-1):
    capi = _capi()
    h = h.copy()
    wp, wl = (capi.pd(w), len(w)) if w is not None else (None, 0)
    capi.check(capi.lib().edigpu_trl_dots(cplx, n, ndot, capi.pd(qbuf), ncol, ldq, len(qbuf), wp, wl, w_col, capi.pd(h), len(h),
                                          skip), "edigpu_trl_dots")
    return h


def hook_norm2(cplx, n, w, h):
    capi = _capi()
    h = h.copy()
    capi.check(capi.lib().edigpu_trl_norm2(cplx, n, capi.pd(w), len(w), capi.pd(h), len(h)), "edigpu_trl_norm2")
    return h


def hook_subtract(cplx, n, nvec, qbuf, ncol, ldq, h, w, skip=-1):
    capi = _capi()
    w = w.copy()
    capi.check(capi.lib().edigpu_trl_subtract(cplx, n, nvec, capi.pd(qbuf), ncol, ldq, len(qbuf), capi.pd(h), len(h), capi.pd(w),
                                              len(w), skip), "edigpu_trl_subtract")
    return w


def hook_decide(h, nvec, eta2, thr2, hf, skip_in=-7):
    capi = _capi()
    hf = hf.copy()
    s = C.c_int32(skip_in)
    capi.check(capi.lib().edigpu_trl_decide(capi.pd(h), len(h), nvec, eta2, thr2, capi.pd(hf), len(hf), C.byref(s)),
               "edigpu_trl_decide")
    return hf, s.value


def hook_filter(h, nvec, thr2):
    capi = _capi()
    h = h.copy()
    capi.check(capi.lib().edigpu_trl_filter(capi.pd(h), len(h), nvec, thr2), "edigpu_trl_filter")
    return h


def hook_rotate(ln, m, k, qbuf, ldq, y, ldy, out, ldo):
    """y: a flat view that starts at the first coefficient (the view's own length is handed over)"""
    capi = _capi()
    out = out.copy()
    capi.check(capi.lib().edigpu_trl_rotate(ln, m, k, capi.pd(qbuf), ldq, len(qbuf), capi.pd(y), ldy, len(y), capi.pd(out), ldo,
                                            len(out)), "edigpu_trl_rotate")
    return out


def hook_scale(ln, v, f):
    capi = _capi()
    v = v.copy()
    capi.check(capi.lib().edigpu_trl_scale(ln, capi.pd(v), len(v), f), "edigpu_trl_scale")
    return v


# ---- references ------------------------------------------------------------------------------------------------------
def ref_dots(q, w):
    """<q_c|w> in long double -> (re, im, sum_i |q_i| |w_i|) per column; q (ncol, n), w (n,), real or complex"""
    ld = np.longdouble
    if np.iscomplexobj(q):
        qr, qi, wr, wi = q.real.astype(ld), q.imag.astype(ld), w.real.astype(ld), w.imag.astype(ld)
        re = (qr * wr + qi * wi).sum(axis=1)
        im = (qr * wi - qi * wr).sum(axis=1)
    else:
        re = (q.astype(ld) * w.astype(ld)).sum(axis=1)
        im = np.zeros(len(q), dtype=ld)
    mag = (np.abs(q).astype(ld) * np.abs(w).astype(ld)).sum(axis=1)
    return re, im, mag


def ref_subtract(q, h, w):
    """the kernel's arithmetic in float64 (no contraction): columns in ascending order, zero coefficients skipped.
    q (nvec, n), h 2 * nvec doubles (re, im), w (n,)"""
    if np.iscomplexobj(q):
        xr, xi = w.real.copy(), w.imag.copy()
        for c in range(len(q)):
            hr, hi = h[2 * c], h[2 * c + 1]
            if hr != 0.0 or hi != 0.0:
                qr, qi = q[c].real, q[c].imag
                xr, xi = xr - (hr * qr - hi * qi), xi - (hr * qi + hi * qr)
        x = np.empty(len(xr), dtype=np.complex128)
        x.real, x.imag = xr, xi
        return x
    x = w.copy()
    for c in range(len(q)):
        hr = h[2 * c]
        if hr != 0.0:
            x = x - hr * q[c]
    return x


def ref_rotate(q, y):
    """out_c = sum_j y[j, c] q_j in long double and sum_j |y_jc| |q_ji|; q (m, len), y (m, k)"""
    m, ln = q.shape
    k = y.shape[1]
    ref = np.empty((k, ln), dtype=np.longdouble)
    mag = np.empty((k, ln), dtype=np.longdouble)
    yl = y.astype(np.longdouble)
    step = 8192                                   # long-double products in pieces that stay in the cache
    for s in range(0, ln, step):
        ql = q[:, s:s + step].astype(np.longdouble)
        ref[:, s:s + step] = yl.T @ ql
        mag[:, s:s + step] = np.abs(yl).T @ np.abs(ql)
    return ref, mag


def ref_decide(h, nvec, eta2, thr2):
    """trl_decide_kernel with Python floats -> (hf[0 : 2 nvec], skip)"""
    h = [float(x) for x in h]
    hh = 0.0
    for c in range(nvec):
        hh += h[2 * c] * h[2 * c] + h[2 * c + 1] * h[2 * c + 1]
    ww = h[2 * nvec]
    enough = ww - hh >= eta2 * ww
    cut = thr2 * (ww - hh) if enough else -1.0
    hf = []
    for c in range(nvec):
        a, b = h[2 * c], h[2 * c + 1]
        keep = c >= nvec - 2 or a * a + b * b > cut
        hf += [a if keep else 0.0, b if keep else 0.0]
    return np.array(hf), int(enough)


def ref_filter(h, nvec, thr2):
    """trl_filter_kernel with Python floats -> the whole of h afterwards"""
    out = [float(x) for x in h]
    cut = thr2 * out[2 * nvec]
    for c in range(nvec):
        a, b = out[2 * c], out[2 * c + 1]
        if not (a * a + b * b > cut):
            out[2 * c] = out[2 * c + 1] = 0.0
    out[2 * nvec] = out[2 * nvec + 1] = 0.0
    return np.array(out)


# ---- the block-diagonal matrix of the end-to-end case ----------------------------------------------------------------
OUTLIERS = (-6.0, -4.5, -3.5, -2.75, -2.0)
SOLVER_BLOCKS = {0: 174763, 1: 87382}   # real: n = 524 289 (odd, one pair past the grid); complex: n = 262 146


class BlockMatrix:
    """Symmetric / Hermitian 3 x 3 blocks B = (G + G^H) / 2 + 5 I (seed 1), entry [0, 0] of five blocks replaced by
    OUTLIERS, conjugated with a random permutation of the indices.  NumPy knows its spectrum block by block."""

    def __init__(self, cplx, nblocks):
        rng = np.random.default_rng(1)
        g = rng.standard_normal((nblocks, 3, 3))
        if cplx:
            g = (g + 1j * rng.standard_normal((nblocks, 3, 3))) / np.sqrt(2.0)
        b = (g + np.conj(np.swapaxes(g, 1, 2))) / 2 + 5.0 * np.eye(3)
        chosen = (np.arange(len(OUTLIERS)) * 2 + 1) * nblocks // (2 * len(OUTLIERS))
        for blk, val in zip(chosen, OUTLIERS):
            b[blk, 0, 0] = val
        self.blocks = b
        self.n = 3 * nblocks
        self.perm = rng.permutation(self.n)
        self.evals = np.sort(np.linalg.eigvalsh(b).ravel())

    def csr(self):
        p = self.perm.reshape(-1, 3)
        rows = np.repeat(p, 3, axis=1).ravel()            # entry (b, r, c) -> row p[b, r]
        cols = np.tile(p, (1, 3)).ravel()                 #                 -> column p[b, c]
        vals = self.blocks.ravel()
        order = np.lexsort((cols, rows))
        rowptr = np.arange(self.n + 1, dtype=np.int64) * 3
        return rowptr, cols[order].astype(np.int32), np.ascontiguousarray(vals[order])

    def matvec(self, x):
        """H x for x (k, n), from the blocks"""
        y = x[:, self.perm].reshape(len(x), -1, 3)
        hy = np.einsum("brc,kbc->kbr", self.blocks, y).reshape(len(x), -1)
        out = np.empty_like(hy)
        out[:, self.perm] = hy
        return out
