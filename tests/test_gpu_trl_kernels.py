"""The multi-vector kernels of the thick-restart eigensolver (csrc/kernels_trl.hip), one launcher at a time through the
edigpu_trl_* test hooks, and the solver end to end at a size where every one of their loops wraps.

The solver hides small kernel errors (its second Gram-Schmidt pass and the next restart repair a slightly non-orthogonal
basis), so each launcher is compared here with a plain NumPy restatement: long double with a bound that follows from the
summation depth where the kernel's order of additions is its own business, float64 bit for bit where the arithmetic is
fixed (no contraction: -ffp-contract=off).  Every buffer travels whole, so sentinels around the payload show every
write; Q is only read, so its gaps hold NaN and a read outside a column poisons the result.  Shapes: tests/trl_cases.py.
"""
import functools

import numpy as np
import pytest

from tests import trl_cases as T
from tests.trl_cases import EPS, SENT

pytestmark = pytest.mark.gpu


def _id(case):
    return "-".join(str(x) for x in case)


def _len(cplx, n):
    return 2 * n if cplx else n


def _nan_h(ndot, extra=7):
    return np.full(T.dots_slots(ndot) + extra, np.nan)


def check_h_layout(h, cplx, ndot):
    """what trl_dots leaves around the ndot sums: exact zeros up to the end of the last group, the sentinel beyond"""
    end = T.dots_slots(ndot)
    assert np.all(T.bits(h[2 * ndot:end]) == 0), "slots of the last group beyond its columns are +0.0"
    assert np.all(np.isnan(h[end:])), "nothing is written beyond 2 * 16 * ceil(ndot / 16) slots"
    if not cplx:
        assert np.all(T.bits(h[1:2 * ndot:2]) == 0), "real: the imaginary slots are +0.0"


# ---- dots ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.vector_cases(), ids=_id)
def test_dots_against_long_double(gpu, case):
    cplx, n, pad = case
    ln = _len(cplx, n)
    ldq = ln + pad
    rng = np.random.default_rng(1000 * n + 10 * pad + cplx)
    ncmax = max(T.column_counts(n))
    q = T.random_vectors(rng, cplx, (ncmax, n))
    w = T.random_vectors(rng, cplx, n)
    re, im, mag = T.ref_dots(q, w)
    wbuf = T.with_tail(T.as_doubles(w), fill=np.nan)
    for ncol in T.column_counts(n):
        qbuf = T.make_q(T.as_doubles(q[:ncol]), ldq)
        h0 = _nan_h(ncol)
        h = T.hook_dots(cplx, n, ncol, qbuf, ncol, ldq, wbuf, -1, h0)
        bound = 64 * EPS * mag[:ncol]
        err_re = np.abs(h[0:2 * ncol:2].astype(np.longdouble) - re[:ncol])
        err_im = np.abs(h[1:2 * ncol:2].astype(np.longdouble) - im[:ncol])
        print(f"dots cplx={cplx} n={n} ldq-len={pad} ncol={ncol}: max err/bound re {float(np.max(err_re / bound)):.3f} "
              f"im {float(np.max(err_im / bound)):.3f}")
        assert np.all(err_re <= bound), (ncol, np.argmax(err_re / bound))
        assert np.all(err_im <= bound), (ncol, np.argmax(err_im / bound))
        check_h_layout(h, cplx, ncol)
        # a set skip flag: nothing is written; a clear one: the same numbers as with no flag
        assert T.same_bits(T.hook_dots(cplx, n, ncol, qbuf, ncol, ldq, wbuf, -1, h0, skip=1), h0)
        assert T.same_bits(T.hook_dots(cplx, n, ncol, qbuf, ncol, ldq, wbuf, -1, h0, skip=0), h)


@pytest.mark.parametrize("case", T.vector_cases(), ids=_id)
def test_dots_with_w_as_a_column_of_q(gpu, case):
    """the solver's <w|w> column: trl_dots(..., j + 2, Q, ..., w = q(j + 1)) -- bit for bit what a separate w gives"""
    cplx, n, pad = case
    ln = _len(cplx, n)
    ldq = ln + pad
    rng = np.random.default_rng(2000 * n + 10 * pad + cplx)
    ncmax = max(T.column_counts(n))
    q = T.random_vectors(rng, cplx, (ncmax, n))
    for ncol in T.column_counts(n):
        qbuf = T.make_q(T.as_doubles(q[:ncol]), ldq)
        h0 = _nan_h(ncol)
        h_col = T.hook_dots(cplx, n, ncol, qbuf, ncol, ldq, None, ncol - 1, h0)
        h_sep = T.hook_dots(cplx, n, ncol, qbuf, ncol, ldq, T.with_tail(T.as_doubles(q[ncol - 1]), fill=np.nan), -1, h0)
        assert T.same_bits(h_col, h_sep), ncol
        check_h_layout(h_col, cplx, ncol)
        re, im, mag = T.ref_dots(q[ncol - 1:ncol], q[ncol - 1])
        assert abs(np.longdouble(h_col[2 * ncol - 2]) - re[0]) <= 64 * EPS * mag[0]
        assert h_col[2 * ncol - 1] == 0.0        # <w|w>: q.x w.y - q.y w.x cancels exactly


@pytest.mark.parametrize("case", [c for c in T.vector_cases() if c[2] == 0], ids=_id)
def test_norm2(gpu, case):
    cplx, n, _ = case
    rng = np.random.default_rng(3000 * n + cplx)
    w = T.random_vectors(rng, cplx, n)
    re, _, mag = T.ref_dots(w[None, :], w)
    h = T.hook_norm2(cplx, n, T.with_tail(T.as_doubles(w), fill=np.nan), _nan_h(1))
    assert abs(np.longdouble(h[0]) - re[0]) <= 64 * EPS * mag[0]
    assert T.bits(h[1:2])[0] == 0                # complex too: exactly zero
    check_h_layout(h, cplx, 1)


@pytest.mark.parametrize("case", [c for c in T.vector_cases() if c[2] == 0], ids=_id)
def test_dots_pick_out_single_elements(gpu, case):
    """w = e_i, Q[c, i] = 1 + c + i / 2^20: every sum has one non-zero term and must equal it bit for bit (conjugated
    for complex vectors) -- the first and last elements, the ends of a workgroup's and of the grid's first trip"""
    cplx, n, _ = case
    ln = _len(cplx, n)
    ncol = max(T.column_counts(n))
    val = 1.0 + np.arange(ncol)[:, None] + np.arange(n)[None, :] / 2.0 ** 20
    q = val + 1j * (val - 0.5) if cplx else val
    qbuf = T.make_q(T.as_doubles(q), ln)
    for i in T.spike_positions(n):
        w = np.zeros(n, dtype=q.dtype)
        w[i] = 1.0
        h = T.hook_dots(cplx, n, ncol, qbuf, ncol, ln, T.with_tail(T.as_doubles(w), fill=np.nan), -1, _nan_h(ncol))
        assert np.array_equal(h[0:2 * ncol:2], val[:, i]), i
        if cplx:
            assert np.array_equal(h[1:2 * ncol:2], -(val[:, i] - 0.5)), i
        check_h_layout(h, cplx, ncol)


# ---- subtract --------------------------------------------------------------------------------------------------------
def _coefficients(rng, cplx, ncol):
    h = rng.standard_normal(2 * ncol)
    if not cplx:
        h[1::2] = 0.0
    return h


@pytest.mark.parametrize("case", T.vector_cases(), ids=_id)
def test_subtract_bit_for_bit(gpu, case):
    cplx, n, pad = case
    ln = _len(cplx, n)
    ldq = ln + pad
    rng = np.random.default_rng(4000 * n + 10 * pad + cplx)
    ncmax = max(T.column_counts(n))
    q = T.random_vectors(rng, cplx, (ncmax, n))
    w = T.random_vectors(rng, cplx, n)
    wbuf = T.with_tail(T.as_doubles(w))
    for ncol in T.column_counts(n):
        qbuf = T.make_q(T.as_doubles(q[:ncol]), ldq)
        h = np.concatenate([_coefficients(rng, cplx, ncol), np.full(3, np.nan)])
        got = T.hook_subtract(cplx, n, ncol, qbuf, ncol, ldq, h, wbuf)
        want = T.with_tail(T.as_doubles(T.ref_subtract(q[:ncol], h, w)))
        assert T.same_bits(got[ln:], want[ln:]), "the sentinels after w[len - 1] are untouched"
        assert T.same_bits(got, want), (ncol, np.flatnonzero(T.bits(got) != T.bits(want))[:4])
        # a set skip flag: w stays as it is; a clear one changes nothing
        assert T.same_bits(T.hook_subtract(cplx, n, ncol, qbuf, ncol, ldq, h, wbuf, skip=1), wbuf)
        assert T.same_bits(T.hook_subtract(cplx, n, ncol, qbuf, ncol, ldq, h, wbuf, skip=0), want)


@pytest.mark.parametrize("case", T.vector_cases(), ids=_id)
def test_subtract_does_not_read_vectors_of_zero_coefficient(gpu, case):
    cplx, n, pad = case
    ln = _len(cplx, n)
    ldq = ln + pad
    rng = np.random.default_rng(5000 * n + 10 * pad + cplx)
    ncmax = max(T.column_counts(n))
    q = T.random_vectors(rng, cplx, (ncmax, n))
    w = T.random_vectors(rng, cplx, n)
    wbuf = T.with_tail(T.as_doubles(w))
    for ncol in T.column_counts(n):
        h = _coefficients(rng, cplx, ncol)
        zero = rng.random(ncol) < 0.5
        zero[16:32] = True                       # a whole group of zeros (where there is a second group)
        zero[0] = ncol > 1                       # the first vector of the first group
        h[np.repeat(zero, 2)] = 0.0
        qn = q[:ncol].copy()
        qn[zero] = np.nan
        qbuf = T.make_q(T.as_doubles(qn), ldq)
        got = T.hook_subtract(cplx, n, ncol, qbuf, ncol, ldq, h, wbuf)
        assert np.all(np.isfinite(got)), ncol
        assert T.same_bits(got, T.with_tail(T.as_doubles(T.ref_subtract(q[:ncol], h, w)))), ncol
        # every coefficient zero: every group returns before it touches w
        qbuf = T.make_q(np.full((ncol, ln), np.nan), ldq)
        assert T.same_bits(T.hook_subtract(cplx, n, ncol, qbuf, ncol, ldq, np.zeros(2 * ncol), wbuf), wbuf), ncol


# ---- rotate ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _rotate_problem(ln, m, k):
    """Q, the coefficient buffer, and the long-double reference: shared by the cases that differ in ldo only"""
    rng = np.random.default_rng(6000 * ln + 100 * m + 10 * k)
    q = rng.standard_normal((m, ln))
    off = 13                                     # Y starts inside its first row: columns off + c cross a group of 16
    ldy = off + k + 3
    ybuf = rng.standard_normal(m * ldy)
    y = np.array([ybuf[off + j * ldy:off + j * ldy + k] for j in range(m)])
    ref, mag = T.ref_rotate(q, y)
    for a in (q, ybuf, ref, mag):
        a.setflags(write=False)
    return q, ybuf, off, ldy, ref, mag


@pytest.mark.parametrize("case", T.rotate_cases(), ids=_id)
def test_rotate_basis(gpu, case):
    ln, m, k, opad = case
    ldo = ln + opad
    q, ybuf, off, ldy, ref, mag = _rotate_problem(ln, m, k)
    out0 = SENT + np.arange((k - 1) * ldo + ln + 6, dtype=np.float64)
    out = T.hook_rotate(ln, m, k, T.make_q(q, ln), ln, ybuf[off:], ldy, out0, ldo)
    payload = np.zeros(len(out0), dtype=bool)
    for c in range(k):
        payload[c * ldo:c * ldo + ln] = True
    assert T.same_bits(out[~payload], out0[~payload]), "only the k * len payload is written"
    got = np.array([out[c * ldo:c * ldo + ln] for c in range(k)])
    err = np.abs(got.astype(np.longdouble) - ref)
    bound = (m + 1) * EPS * mag
    print(f"rotate len={ln} m={m} k={k} ldo-len={opad}: max err/bound {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound), np.unravel_index(np.argmax(err / bound), err.shape)


# ---- scale -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", T.SCALE_LEN)
def test_scale(gpu, ln):
    rng = np.random.default_rng(7000 + ln)
    v = rng.standard_normal(ln)
    f = 1.0 / 3.7
    got = T.hook_scale(ln, T.with_tail(v), f)
    assert T.same_bits(got, T.with_tail(v * f))


# ---- decide / filter -------------------------------------------------------------------------------------------------
def _decide(h, nvec, eta2, thr2):
    hbuf = np.concatenate([h, np.full(4, np.nan)])
    hf0 = SENT + np.arange(2 * nvec + 5, dtype=np.float64)
    hf, skip = T.hook_decide(hbuf, nvec, eta2, thr2, hf0)
    want, want_skip = T.ref_decide(hbuf, nvec, eta2, thr2)
    assert skip == want_skip
    assert T.same_bits(hf[:2 * nvec], want)
    assert T.same_bits(hf[2 * nvec:], hf0[2 * nvec:])
    return hf[:2 * nvec], skip


@pytest.mark.parametrize("nvec", [1, 2, 3, 17, 40])
def test_decide_at_the_twice_is_enough_threshold(gpu, nvec):
    """ww - hh just above, at and just below eta2 * ww (eta2 = 1/2: ww = 2 hh is the boundary, exact in binary)"""
    rng = np.random.default_rng(8000 + nvec)
    coef = rng.standard_normal(2 * nvec)
    hh = 0.0
    for c in range(nvec):
        a, b = float(coef[2 * c]), float(coef[2 * c + 1])
        hh += a * a + b * b
    skips = []
    for ww in (np.nextafter(2 * hh, np.inf), 2 * hh, np.nextafter(2 * hh, 0.0)):
        hf, skip = _decide(np.concatenate([coef, [ww, 0.0]]), nvec, 0.5, 1e-6)
        skips.append(skip)
        if not skip:
            assert T.same_bits(hf, coef)         # a second pass follows: nothing is filtered
    assert skips == [1, 1, 0]


def test_decide_filters_at_the_cut(gpu):
    """dyadic numbers, so that hh, ww - hh = 16 and the cut thr2 * 16 = 2^-6 are exact: |h_0|^2 is exactly the cut (dropped:
    kept means above), |h_1|^2 one term above (kept), |h_2|^2 below (dropped), the last two are kept whatever they are"""
    coef = np.array([2.0 ** -3, 0.0, 2.0 ** -3, 2.0 ** -10, 2.0 ** -5, 0.0, 2.0 ** -12, 0.0, 1.0, 0.5])
    hh = float(np.sum(coef * coef))
    thr2 = 2.0 ** -10
    hf, skip = _decide(np.concatenate([coef, [hh + 16.0, 0.0]]), 5, 0.5, thr2)
    assert (hh + 16.0) - hh == 16.0 and skip == 1
    want = coef.copy()
    want[[0, 1, 4, 5]] = 0.0
    assert T.same_bits(hf, want)
    # one and two vectors: always kept, though far below the cut
    for nvec in (1, 2):
        tiny = np.array([2.0 ** -30, 2.0 ** -31, 2.0 ** -32, 2.0 ** -33])[:2 * nvec]
        hf, skip = _decide(np.concatenate([tiny, [16.0, 0.0]]), nvec, 0.5, thr2)
        assert skip == 1 and T.same_bits(hf, tiny)


@pytest.mark.parametrize("nvec", [1, 2, 5, 40])
def test_filter(gpu, nvec):
    """trl_filter has no kept pair: whatever is not above thr2 * <w|w> goes, and the <w|w> slot is cleared"""
    rng = np.random.default_rng(9000 + nvec)
    coef = rng.standard_normal(2 * nvec) * 10.0 ** rng.integers(-8, 1, 2 * nvec)
    coef[0], coef[1] = 2.0 ** -3, 0.0            # exactly at the cut 2^-10 * 16: dropped
    if nvec > 1:
        coef[2], coef[3] = 2.0 ** -3, 2.0 ** -10  # above: kept
    h = np.concatenate([coef, [16.0, 3.0], np.full(4, np.nan)])
    got = T.hook_filter(h, nvec, 2.0 ** -10)
    want = T.ref_filter(h[:2 * nvec + 2], nvec, 2.0 ** -10)
    assert T.same_bits(got[:2 * nvec + 2], want)
    assert np.all(np.isnan(got[2 * nvec + 2:]))
    assert got[0] == 0.0 and got[2 * nvec] == 0.0 and got[2 * nvec + 1] == 0.0
    if nvec > 1:
        assert got[2] == 2.0 ** -3 and got[3] == 2.0 ** -10


# ---- the solver at a size where every kernel wraps ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def block_problem(gpu):
    from edipack_amd.hamiltonian import SectorHamiltonian
    made = {}

    def get(cplx):
        if cplx not in made:
            bm = T.BlockMatrix(cplx, T.SOLVER_BLOCKS[cplx])
            made[cplx] = (bm, SectorHamiltonian.csr_from_arrays(*bm.csr()))
        return made[cplx]
    yield get
    for _, h in made.values():
        h.destroy()


def check_solver(bm, h, label):
    ev, x, nconv, nmv = h.lanczos_eigh_multi(4, ncv=20, tol=1e-12)
    print(f"trl_solve {label} n={bm.n}: nconv={nconv} products={nmv} evals={ev}")
    ref = bm.evals[:4]
    assert ref[3] < bm.evals[4] - 0.5            # the four wanted values are separated from the rest
    assert nconv == 4
    scale = np.maximum(1.0, np.abs(ref))
    assert np.all(np.abs(ev - ref) <= 1e-10 * scale), ev - ref
    gram = x.conj() @ x.T
    assert np.max(np.abs(gram - np.eye(4))) < 1e-10
    res = np.linalg.norm(bm.matvec(x) - ev[:, None] * x, axis=1)
    print(f"  |x^H x - 1| {np.max(np.abs(gram - np.eye(4))):.2e} residuals {res}")
    assert np.all(res < 1e-9 * scale), res


@pytest.mark.parametrize("cplx", [0, 1], ids=["real-524289", "complex-262146"])
def test_solver_on_a_known_spectrum(block_problem, monkeypatch, cplx):
    """524 289 real elements (odd: ldq = n puts every other basis vector 8 bytes off a 16-byte boundary, and the grid's
    second trip holds the one last pair and the tail element), 262 146 complex ones; the default, selective branch"""
    monkeypatch.delenv("EDIGPU_TRL_FULL", raising=False)
    monkeypatch.delenv("EDIGPU_TRL_ONEPASS", raising=False)
    bm, h = block_problem(cplx)
    assert h.nloc == bm.n == (524289, 262146)[cplx]
    check_solver(bm, h, "complex" if cplx else "real")


@pytest.mark.parametrize("switch", ["EDIGPU_TRL_FULL", "EDIGPU_TRL_ONEPASS"])
def test_solver_other_orthogonalisation_branches(block_problem, monkeypatch, switch):
    """full CGS2 on every step, and the branch of trl_decide and the skip flag: the switches are read when the solver starts"""
    monkeypatch.delenv("EDIGPU_TRL_FULL", raising=False)
    monkeypatch.delenv("EDIGPU_TRL_ONEPASS", raising=False)
    monkeypatch.setenv(switch, "1")
    bm, h = block_problem(0)
    check_solver(bm, h, switch)
