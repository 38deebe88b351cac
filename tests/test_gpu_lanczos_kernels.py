"""The vector kernels of the three-term recurrence, one launcher at a time: the single-seed kernels outside the fused
path (csrc/kernels_lanczos.hip), the sharded recurrence (csrc/kernels_shard.hip) and the batched one
(csrc/kernels_multi.hip) through the edigpu_lzk_* test hooks, the public edigpu_vec_* / edigpu_transpose_* functions on
torch tensors.

End-to-end runs compare a dozen coefficients to 1e-10 and cannot tell a damaged element from rounding, so each launcher
is held to a plain NumPy restatement (tests/lanczos_cases.py, checked on the CPU by tests/test_lanczos_cases_host.py):
  * elementwise results bit for bit where the scalar is given (float64 in the kernel's own sequence of operations; the
    library is built with -ffp-contract=off), to 4 ulp where the kernel takes a square root on the device, and bit for
    bit again where that root is exact;
  * sums bit for bit against the restated order of additions (per-workgroup partials and totals), within
    64 EPS sum |terms| of a long-double sum (the ratio is printed), and exactly in the pick-out cases;
  * layouts against index formulas, the send / back buffers also against the library's exchange maps;
  * every written buffer is followed by NaN that must survive, every read-only buffer by NaN that would poison a sum;
  * a set stop flag leaves every buffer and scalar bit-identical;
  * each column of the batched kernels equals the single-seed launcher run on that column alone, bit for bit.
Lengths: the edges of the grid-stride loops as written in the launchers (tests/lanczos_cases.py).
"""
import numpy as np
import pytest

from tests import lanczos_cases as L
from tests.lanczos_cases import (NLANC, NSCAL, NT, RED, SC_AB, SC_ALPHA, SC_BETA, SC_NDONE, SC_NORM, SC_STOP, SC_THR, TAIL, guard,
                                 nans, same_bits, scalars, tail_intact)

pytestmark = pytest.mark.gpu

T_RANDOM = np.array([0.3, 1.7, 0.9])         # beta^2 = 1.7 - 2 * 0.1 * (0.3 - 0.2 * 0.9) + 0.01 * 0.9: no exact root
TPREV_RANDOM = np.array([0.2, 5.0, 1.1])


def report(kernel, n, value, terms):
    """the long-double bound of a sum: asserted, and printed as error / bound"""
    r = L.bound_ratio(value, terms)
    print(f"RATIO {kernel} n={n} err/bound={r:.4f}")
    assert r <= 1.0, (kernel, n, r)


def within_4_ulp(a, b):
    return bool(np.all(L.ulp_diff(a, b) <= 4))


def values(n):
    """distinct, exactly representable, none zero"""
    return 1.0 + np.arange(n, dtype=np.float64) / 2.0 ** 21


# ---- kernels_lanczos.hip ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", L.REDUCE_LENGTHS + L.EW_N)
def test_norm_begin(gpu, n):
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n)
    nb = L.red_blocks(n)
    scal0 = scalars(alpha=0.3, beta=0.7, stop=1.0, ndone=3.0, norm=9.0)      # mode 0 starts a recurrence: stop is reset
    vo, part, scal = L.hook_norm_begin(n, guard(v), nans(nb), scal0)
    tot, want_part = L.device_sum(v * v, nb)
    assert same_bits(part[:nb], want_part) and tail_intact(part, nb)
    report("k_sumsq+k_finalize(0)", n, tot, v * v)
    nrm = scal[SC_NORM]
    assert L.ulp_diff(nrm, np.sqrt(tot))[0] <= 4
    want = scal0.copy()
    want[SC_NORM], want[SC_STOP], want[SC_NDONE] = nrm, 0.0, 0.0
    assert same_bits(scal, want)
    assert same_bits(vo[:n], v * (1.0 / nrm)) and tail_intact(vo, n)
    # an exact root: |v|^2 = 25 (9 when n = 1)
    e = np.zeros(n)
    e[0], e[-1] = 3.0, (4.0 if n > 1 else 3.0)
    vo, _, scal = L.hook_norm_begin(n, guard(e), nans(nb), scal0)
    assert scal[SC_NORM] == (5.0 if n > 1 else 3.0)
    assert same_bits(vo[:n], e * (1.0 / scal[SC_NORM]))
    # pick-outs: one non-zero element, one non-zero partial that is its square
    for i in L.spike_positions(n, nb):
        e = np.zeros(n)
        e[i] = 1.0 + i / 2.0 ** 21
        _, part, _ = L.hook_norm_begin(n, guard(e), nans(nb), scal0)
        want_part = np.zeros(nb)
        want_part[(i // NT) % nb] = e[i] * e[i]
        assert same_bits(part[:nb], want_part), i
    # a zero vector: the recurrence never starts, and no 1 / 0 reaches the vector
    vo, _, scal = L.hook_norm_begin(n, guard(np.zeros(n)), nans(nb), scalars(alpha=0.3, ndone=3.0, norm=9.0))
    assert scal[SC_STOP] == 1.0 and scal[SC_NORM] == 0.0 and scal[SC_NDONE] == 0.0
    assert same_bits(vo, guard(np.zeros(n)))


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("n", L.ELEMENTWISE_LENGTHS)
def test_rotate(gpu, n, lazy):
    rng = np.random.default_rng(10 * n + lazy)
    p, q = rng.standard_normal(n), rng.standard_normal(n)
    a, b = 0.3, 0.7
    scal = scalars(alpha=a, beta=b)
    po, qo = L.hook_rotate(lazy, n, guard(p), guard(q), scal)
    wp, wq = L.ref_rotate_lazy(p, q, a, b) if lazy else L.ref_rotate(p, q, b)
    assert same_bits(po[:n], wp) and same_bits(qo[:n], wq) and tail_intact(po, n) and tail_intact(qo, n)
    po, qo = L.hook_rotate(lazy, n, guard(p), guard(q), scalars(alpha=a, beta=b, stop=1.0))
    assert same_bits(po, guard(p)) and same_bits(qo, guard(q))


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("n", L.ELEMENTWISE_LENGTHS)
def test_next_vector(gpu, n, lazy):
    rng = np.random.default_rng(20 * n + lazy)
    p, q = rng.standard_normal(n), rng.standard_normal(n)
    a, b = 0.3, 0.7
    x = L.hook_next_vector(lazy, n, guard(p), guard(q), nans(n), scalars(alpha=a, beta=b))
    ib = 1.0 / b
    assert same_bits(x[:n], (q - (a if lazy else 0.0) * p) * ib) and tail_intact(x, n)
    x = L.hook_next_vector(lazy, n, guard(p), guard(q), nans(n), scalars(alpha=a, beta=b, stop=1.0))
    assert np.all(np.isnan(x))


@pytest.mark.parametrize("n", L.REDUCE_LENGTHS)
def test_alpha(gpu, n):
    rng = np.random.default_rng(30 * n)
    vin, vout, tmp = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    nb = L.red_blocks(n)
    it = 2
    scal0 = scalars(alpha=0.3, beta=0.7, ndone=2.0, norm=1.25)
    wo, part, scal = L.hook_alpha(n, guard(vin), guard(vout), guard(tmp), nans(nb), scal0, it)
    w = vout + tmp
    tot, want_part = L.device_sum(vin * w, nb)
    assert same_bits(wo[:n], w) and tail_intact(wo, n)
    assert same_bits(part[:nb], want_part) and tail_intact(part, nb)
    report("k_alpha+k_finalize(1)", n, tot, vin * w)
    want = scal0.copy()
    want[SC_ALPHA] = want[SC_AB + it] = tot
    want[SC_NDONE] = it + 1.0
    assert same_bits(scal, want)
    for i in L.spike_positions(n, nb):
        e = np.zeros(n)
        e[i] = 1.0
        _, _, scal = L.hook_alpha(n, guard(e), guard(values(n)), guard(np.zeros(n)), nans(nb), scal0, it)
        assert scal[SC_ALPHA] == values(n)[i], i
    stop0 = scalars(alpha=0.3, beta=0.7, stop=1.0, ndone=2.0)
    wo, part, scal = L.hook_alpha(n, guard(vin), guard(vout), guard(tmp), nans(nb), stop0, it)
    assert same_bits(wo, guard(vout)) and np.all(np.isnan(part)) and same_bits(scal, stop0)


@pytest.mark.parametrize("n", L.REDUCE_LENGTHS)
def test_beta(gpu, n):
    rng = np.random.default_rng(40 * n)
    vin, vout = rng.standard_normal(n), rng.standard_normal(n)
    nb = L.red_blocks(n)
    a = 0.3
    w = vout - a * vin
    tot, want_part = L.device_sum(w * w, nb)
    for it in (2, NLANC - 1):
        scal0 = scalars(alpha=a, beta=0.7, ndone=it + 1.0, norm=1.25)
        wo, part, scal = L.hook_beta(n, guard(vin), guard(vout), nans(nb), scal0, it)
        assert same_bits(wo[:n], w) and tail_intact(wo, n)
        assert same_bits(part[:nb], want_part) and tail_intact(part, nb)
        b = scal[SC_BETA]
        assert L.ulp_diff(b, np.sqrt(tot))[0] <= 4
        want = scal0.copy()
        want[SC_BETA] = b
        if it + 1 < NLANC:
            want[SC_AB + NLANC + it + 1] = b            # it + 1 == nlanc records no beta
        assert same_bits(scal, want)
    report("k_beta+k_finalize(2)", n, tot, w * w)
    # an exact root: vout = (3, 0 ..., 4), vin = 0
    e = np.zeros(n)
    e[0], e[-1] = 3.0, (4.0 if n > 1 else 3.0)
    _, _, scal = L.hook_beta(n, guard(np.zeros(n)), guard(e), nans(nb), scalars(alpha=a), 0)
    assert scal[SC_BETA] == (5.0 if n > 1 else 3.0) and scal[SC_AB + NLANC + 1] == scal[SC_BETA] and scal[SC_STOP] == 0.0
    # beta below the threshold ends the recurrence and records no beta
    thr0 = scalars(alpha=a, thr=1e6)
    _, _, scal = L.hook_beta(n, guard(vin), guard(vout), nans(nb), thr0, 0)
    assert scal[SC_STOP] == 1.0 and L.ulp_diff(scal[SC_BETA], np.sqrt(tot))[0] <= 4 and np.isnan(scal[SC_AB + NLANC + 1])
    # an exact zero ends it at threshold 0
    _, _, scal = L.hook_beta(n, guard(np.zeros(n)), guard(np.zeros(n)), nans(nb), scalars(alpha=a, thr=0.0), 0)
    assert scal[SC_STOP] == 1.0 and scal[SC_BETA] == 0.0 and np.isnan(scal[SC_AB + NLANC + 1])
    stop0 = scalars(alpha=a, beta=0.7, stop=1.0)
    wo, part, scal = L.hook_beta(n, guard(vin), guard(vout), nans(nb), stop0, 0)
    assert same_bits(wo, guard(vout)) and np.all(np.isnan(part)) and same_bits(scal, stop0)


@pytest.mark.parametrize("n", L.REDUCE_LENGTHS)
def test_add_dot3(gpu, n):
    rng = np.random.default_rng(50 * n)
    p, q, tmp = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    nb = L.red_blocks(n)
    sg = 0.3
    qo, part, cnt = L.hook_add_dot3(n, guard(p), guard(q), guard(tmp), scalars(alpha=sg), nans(3 * nb))
    w = q + tmp
    assert cnt == nb and same_bits(qo[:n], w) and tail_intact(qo, n) and tail_intact(part, 3 * nb)
    for k, terms in enumerate(L.three_terms(p, w, sg)):
        assert same_bits(part[k * nb:(k + 1) * nb], L.block_partials(terms, nb)), k
        report(f"k_add_dot3[{k}]", n, L.strided_tree_sum(part[k * nb:(k + 1) * nb]), terms)
    for i in L.spike_positions(n, nb):
        e = np.zeros(n)
        e[i] = 1.0
        _, part, _ = L.hook_add_dot3(n, guard(e), guard(values(n)), guard(np.zeros(n)), scalars(alpha=0.0), nans(3 * nb))
        assert L.strided_tree_sum(part[:nb]) == values(n)[i] and L.strided_tree_sum(part[2 * nb:3 * nb]) == 1.0, i
    # stopped: the partials are written as zeros (the finalize that follows returns at once), Q is left alone
    qo, part, cnt = L.hook_add_dot3(n, guard(p), guard(q), guard(tmp), scalars(alpha=sg, stop=1.0), nans(3 * nb))
    assert cnt == nb and same_bits(qo, guard(q)) and same_bits(part, guard(np.zeros(3 * nb)))


@pytest.mark.parametrize("n", L.ELEMENTWISE_LENGTHS)
def test_axpy_coef(gpu, n):
    rng = np.random.default_rng(60 * n)
    acc, vin = rng.standard_normal(n), rng.standard_normal(n)
    scal = scalars(ndone=3.0)
    out = L.hook_axpy(n, guard(acc), guard(vin), 0.37, scal, 2)              # iter < SC_NDONE: added
    assert same_bits(out[:n], acc + 0.37 * vin) and tail_intact(out, n)
    for it in (3, 4):                                                         # iter >= SC_NDONE: skipped
        assert same_bits(L.hook_axpy(n, guard(acc), guard(vin), 0.37, scal, it), guard(acc))


@pytest.mark.parametrize("shift", [2, 5, 7])
def test_blocked_layout(gpu, shift):
    for du, dd, sh in L.BLOCKED_CASES:
        if sh != shift:
            continue
        src = 1.0 + np.arange(du * dd, dtype=np.float64)
        blen = L.blocked_len(du, dd, sh)
        blk = L.hook_blocked(1, du, dd, sh, guard(src), nans(blen))
        assert same_bits(blk[:blen], L.to_blocked(src, du, dd, sh)), (du, dd)     # the padding is exactly +0.0
        assert tail_intact(blk, blen)
        poisoned = L.to_blocked(src, du, dd, sh)
        poisoned[poisoned == 0.0] = np.nan                                        # the way back never reads the padding
        nat = L.hook_blocked(0, du, dd, sh, guard(poisoned), nans(du * dd))
        assert same_bits(nat[:du * dd], src) and tail_intact(nat, du * dd), (du, dd)


# ---- kernels_shard.hip --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", L.ELEMENTWISE_LENGTHS)
def test_shard_rotate3_without_exchange(gpu, n):
    rng = np.random.default_rng(70 * n)
    v, w = rng.standard_normal(n), rng.standard_normal(n)
    for t, tprev, exact in ((L.EXACT_T, L.EXACT_TPREV, True), (T_RANDOM, TPREV_RANDOM, False), (T_RANDOM, None, False)):
        a, b, _ = L.ab_from_sums(t, tprev)
        vo, wo, _ = L.hook_shard_rotate3(0, n, None, guard(v), guard(w), t, tprev, None)
        wv, ww = L.ref_rotate_lazy(v, w, a, b)
        assert tail_intact(vo, n) and tail_intact(wo, n)
        if exact:
            assert same_bits(vo[:n], wv) and same_bits(wo[:n], ww)
        else:
            assert within_4_ulp(vo[:n], wv) and within_4_ulp(wo[:n], ww)
    # the first step without a send buffer touches nothing
    vo, wo, _ = L.hook_shard_rotate3(1, n, None, guard(v), guard(w), None, None, None)
    assert same_bits(vo, guard(v)) and same_bits(wo, guard(w))


@pytest.mark.parametrize("geom", L.EXCHANGE_SMALL + (L.EXCHANGE_RED, L.EXCHANGE_EW), ids=str)
def test_shard_rotate3_packs_the_send_buffer(gpu, geom):
    world, du, nrows, q, halo = geom
    pcol = L.pcol_of(world, du)
    n, nsend = nrows * du, world * q * (pcol + 2 * halo)
    rng = np.random.default_rng(du + nrows)
    v, w = rng.standard_normal(q * du), rng.standard_normal(q * du)
    src = L.library_send_map(du, nrows, q, world, pcol, halo)
    # first step: only packs
    vo, wo, send = L.hook_shard_rotate3(1, n, geom, guard(v), guard(w), None, None, nans(nsend))
    assert same_bits(vo, guard(v)) and same_bits(wo, guard(w))
    assert same_bits(send[:nsend], L.pack(v, du, nrows, q, world, pcol, halo, np.full(nsend, np.nan)))
    assert same_bits(send[:nsend], np.where(src >= 0, v[np.maximum(src, 0)], np.nan)) and tail_intact(send, nsend)
    # a later step: rotate, and the new v in every block that holds its column; rows past nrows are left alone
    a, b, _ = L.ab_from_sums(L.EXACT_T, L.EXACT_TPREV)
    vo, wo, send = L.hook_shard_rotate3(0, n, geom, guard(v), guard(w), L.EXACT_T, L.EXACT_TPREV, nans(nsend))
    wv, ww = L.ref_rotate_lazy(v[:n], w[:n], a, b)
    assert same_bits(vo[:n], wv) and same_bits(wo[:n], ww)
    assert same_bits(vo[n:], guard(v)[n:]) and same_bits(wo[n:], guard(w)[n:])
    assert same_bits(send[:nsend], np.where(src >= 0, vo[np.maximum(src, 0)], np.nan)) and tail_intact(send, nsend)
    assert np.isnan(send[:nsend]).sum() == (src < 0).sum()       # positions no column maps to keep their sentinel


def check_three_sums(kernel, n, nb, work, sums, terms3):
    """work: three planes RED apart, nb partials each, the rest untouched; sums: their totals"""
    assert len(work) == 3 * RED + TAIL and tail_intact(sums, 3)
    for k, terms in enumerate(terms3):
        plane = work[k * RED:(k + 1) * RED]
        assert same_bits(plane[:nb], L.block_partials(terms, nb)), (kernel, k)
        assert np.all(np.isnan(plane[nb:])), (kernel, k)
        assert sums[k] == L.strided_tree_sum(plane[:nb]), (kernel, k)
        report(f"{kernel}[{k}]", n, sums[k], terms)
    assert tail_intact(work, 3 * RED)


@pytest.mark.parametrize("n", L.REDUCE_LENGTHS)
def test_shard_add_dot3_without_exchange(gpu, n):
    rng = np.random.default_rng(80 * n)
    v, w, tmp = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    nb = L.red_blocks(n)
    for tprev in (None, TPREV_RANDOM):
        sg = tprev[0] if tprev is not None else 0.0
        wo, work, sums = L.hook_shard_add_dot3(n, None, guard(v), guard(w), guard(tmp), None, tprev, nans(3 * RED), nans(3))
        assert same_bits(wo[:n], w + tmp) and tail_intact(wo, n)
        check_three_sums("ks_add_dot3+ks_sum3", n, nb, work, sums, L.three_terms(v, w + tmp, sg))
    for i in L.spike_positions(n, nb):
        e = np.zeros(n)
        e[i] = 1.0
        _, _, sums = L.hook_shard_add_dot3(n, None, guard(e), guard(values(n)), guard(np.zeros(n)), None, None, nans(3 * RED), nans(3))
        assert sums[0] == values(n)[i] and sums[2] == 1.0, i


@pytest.mark.parametrize("geom", L.EXCHANGE_SMALL + (L.EXCHANGE_RED,), ids=str)
def test_shard_add_dot3_unpacks_the_way_back(gpu, geom):
    world, du, nrows, q, halo = geom
    pcol = L.pcol_of(world, du)
    n, nback = nrows * du, world * q * (pcol + 2 * halo)
    rng = np.random.default_rng(du + 7 * nrows)
    v, w, tmp = rng.standard_normal(q * du), rng.standard_normal(q * du), rng.standard_normal(q * du)
    slots = L.library_back_map(du, nrows, q, world, pcol, halo)
    assert np.array_equal(slots, L.back_slots(du, nrows, q, pcol, halo))
    back = np.full(nback, np.nan)              # only the slots the kernel must read are finite
    back[slots] = rng.standard_normal(n)
    wo, work, sums = L.hook_shard_add_dot3(n, geom, guard(v), guard(w), guard(tmp), guard(back), TPREV_RANDOM, nans(3 * RED), nans(3))
    wn = (w[:n] + tmp[:n]) + back[slots]
    assert same_bits(wo[:n], wn) and same_bits(wo[n:], guard(w)[n:])
    check_three_sums("ks_add_dot3(back)+ks_sum3", n, L.red_blocks(n), work, sums, L.three_terms(v[:n], wn, TPREV_RANDOM[0]))


@pytest.mark.parametrize("n2", L.SMALL_N + L.EW_N)
def test_shard_panel_rotate(gpu, n2):
    rng = np.random.default_rng(90 * n2)
    x, v = rng.standard_normal(2 * n2), rng.standard_normal(2 * n2)
    for t, tprev, exact in ((L.EXACT_T, L.EXACT_TPREV, True), (T_RANDOM, TPREV_RANDOM, False), (T_RANDOM, None, False)):
        a, b, _ = L.ab_from_sums(t, tprev)
        xo = L.hook_panel_rotate(n2, guard(x), guard(v), t, tprev)
        want = (x - a * v) * (1.0 / b)
        assert tail_intact(xo, 2 * n2)
        assert same_bits(xo[:2 * n2], want) if exact else within_4_ulp(xo[:2 * n2], want)


@pytest.mark.parametrize("n2", L.REDUCE_LENGTHS)
def test_shard_panel_add_dot(gpu, n2):
    rng = np.random.default_rng(100 * n2)
    n = 2 * n2
    x, p, r, c = (rng.standard_normal(n) for _ in range(4))
    nb = L.red_blocks(n2)
    # first step: vdst = rowhalf + colhalf, and vdst is not read (it holds NaN); the sums are about 0
    wo, work, sums = L.hook_panel_add_dot(n2, guard(x), nans(n), guard(r), guard(c), None, None, nans(3 * RED), nans(3))
    assert same_bits(wo[:n], r + c) and tail_intact(wo, n)
    check_three_sums("ks_panel_add_dot(first)+ks_sum3", n2, nb, work, sums, L.three_terms_pairs(x, r + c, 0.0))
    # later steps: w = rowhalf + colhalf - beta v over v, the sums about alpha
    for t, tprev, exact in ((L.EXACT_T, L.EXACT_TPREV, True), (T_RANDOM, None, False)):
        sg, b, _ = L.ab_from_sums(t, tprev)
        wo, work, sums = L.hook_panel_add_dot(n2, guard(x), guard(p), guard(r), guard(c), t, tprev, nans(3 * RED), nans(3))
        want = (r + c) - b * p
        assert tail_intact(wo, n)
        if exact:
            assert same_bits(wo[:n], want)
        else:
            # a beta within 4 ulp of ours: the product b p moves by at most 5 * 2^-52 |b p| (4 ulp of beta, two
            # roundings), and the subtraction rounds once more -- an absolute bound, since the difference may cancel
            assert np.all(np.abs(wo[:n] - want) <= 5 * 2.0 ** -52 * np.abs(b * p) + 2.0 ** -52 * np.abs(want))
        # the sums are those of the w the kernel stored
        check_three_sums("ks_panel_add_dot+ks_sum3", n2, nb, work, sums, L.three_terms_pairs(x, wo[:n], sg))
    for i in L.spike_positions(n2, nb):
        e = np.zeros(n)
        e[2 * i + 1] = 1.0
        _, _, sums = L.hook_panel_add_dot(n2, guard(e), nans(n), guard(values(n)), guard(np.zeros(n)), None, None, nans(3 * RED), nans(3))
        assert sums[0] == values(n)[2 * i + 1] and sums[2] == 1.0, i


# ---- kernels_multi.hip --------------------------------------------------------------------------------------------------
def multi_rows(W, EL, elems=False):
    return (L.mu_rows_below(W, EL), L.mu_rows_second_trip_elems(W) if elems else L.mu_rows_second_trip_chunks(W, EL))


@pytest.mark.parametrize("W,EL", L.WIDTHS)
def test_interleave_and_back(gpu, W, EL):
    for n in multi_rows(W, EL, elems=True):
        for g in ((W - 1, W, 0) if n < 10000 else (W - 1,)):
            src = 1.0 + np.arange(g * n * EL, dtype=np.float64)
            xi = L.hook_interleave(1, W, EL, n, g, guard(src), nans(W * n * EL))
            assert same_bits(xi[:W * n * EL], L.interleave(src, n, W, EL, g)), (n, g)     # columns g .. W-1 are +0.0
            assert tail_intact(xi, W * n * EL)
            full = 1.0 + np.arange(W * n * EL, dtype=np.float64)
            nat = L.hook_interleave(0, W, EL, n, g, guard(full), nans(W * n * EL))
            assert same_bits(nat, L.deinterleave(full, n, W, EL, g, nans(W * n * EL))), (n, g)  # vectors g .. W-1 untouched


def scal_blocks(W, sstride, **cols):
    """W scalar blocks sstride apart, NaN in the gaps and the tail; cols: per-column lists"""
    s = np.full((W - 1) * sstride + NSCAL + TAIL, np.nan)
    for j in range(W):
        kw = {k: v[j] for k, v in cols.items()}
        s[j * sstride:j * sstride + NSCAL] = scalars(**kw)[:NSCAL]
    return s


def block_of(scal, j, sstride):
    return guard(scal[j * sstride:j * sstride + NSCAL])


@pytest.mark.parametrize("W,EL", L.WIDTHS)
def test_norm_begin_multi_equals_the_single_seed_norm(gpu, W, EL):
    sstride = NSCAL + 3
    for n in multi_rows(W, EL):
        rng = np.random.default_rng(1000 * W + 10 * EL + (n > 10000))
        n1 = n * EL
        nb = L.red_blocks(n1)
        seeds = rng.standard_normal((W, n1)) * (1.0 + np.arange(W))[:, None]
        seeds[W - 1] = 0.0                                                       # a zero seed: the column never starts
        P = L.interleave(seeds.ravel(), n, W, EL, W)
        scal0 = scal_blocks(W, sstride, alpha=[0.1 * j for j in range(W)], ndone=[3.0] * W, norm=[9.0 + j for j in range(W)])
        Po, part, scal = L.hook_norm_begin_multi(W, EL, n, guard(P), nans(W * nb), scal0, sstride)
        assert tail_intact(Po, W * n1) and tail_intact(part, W * nb)
        want_scal = scal0.copy()
        for j in range(W):
            vo, p1, s1 = L.hook_norm_begin(n1, guard(seeds[j]), nans(nb), block_of(scal0, j, sstride))
            assert same_bits(part[j * nb:(j + 1) * nb], p1[:nb]), (n, j)          # bit for bit the single-seed kernels
            assert same_bits(L.column(Po, n, W, EL, j), vo[:n1]), (n, j)
            want_scal[j * sstride:j * sstride + NSCAL] = s1[:NSCAL]
            assert same_bits(part[j * nb:(j + 1) * nb], L.block_partials(seeds[j] * seeds[j], nb)), (n, j)
        assert same_bits(scal, want_scal), n                                      # gaps and tail untouched
        assert scal[(W - 1) * sstride + SC_STOP] == 1.0 and scal[SC_STOP] == 0.0
        assert same_bits(L.column(Po, n, W, EL, W - 1), np.zeros(n1))
        # a stopped column that held something is written as exact zeros: a NaN seed has no norm
        if n < 10000:
            seeds[0, 0] = np.nan
            Po, _, scal = L.hook_norm_begin_multi(W, EL, n, guard(L.interleave(seeds.ravel(), n, W, EL, W)), nans(W * nb), scal0, sstride)
            assert scal[SC_STOP] == 1.0 and same_bits(L.column(Po, n, W, EL, 0), np.zeros(n1))
            assert np.all(np.isfinite(Po[:W * n1]))
            if W > 2:                                   # its neighbour is unaffected
                assert scal[sstride + SC_STOP] == 0.0 and np.count_nonzero(L.column(Po, n, W, EL, 1)) == n1


@pytest.mark.parametrize("W,EL", L.WIDTHS)
def test_rotate_lazy_multi_equals_the_single_seed_rotate(gpu, W, EL):
    sstride = NSCAL + 3
    for n in multi_rows(W, EL):
        rng = np.random.default_rng(2000 * W + 10 * EL + (n > 10000))
        n1 = n * EL
        pc, qc = rng.standard_normal((W, n1)), rng.standard_normal((W, n1))
        alphas = [0.3 + 0.11 * j for j in range(W)]
        betas = [0.7 + 0.13 * j for j in range(W)]
        stops = [1.0 if j == 1 else 0.0 for j in range(W)]                       # column 1 has ended
        scal = scal_blocks(W, sstride, alpha=alphas, beta=betas, stop=stops)
        P, Q = L.interleave(pc.ravel(), n, W, EL, W), L.interleave(qc.ravel(), n, W, EL, W)
        Po, Qo = L.hook_rotate_lazy_multi(W, EL, n, guard(P), guard(Q), scal, sstride)
        assert tail_intact(Po, W * n1) and tail_intact(Qo, W * n1)
        for j in range(W):
            cp, cq = L.column(Po, n, W, EL, j), L.column(Qo, n, W, EL, j)
            if stops[j]:
                assert same_bits(cp, np.zeros(n1)) and same_bits(cq, np.zeros(n1)), (n, j)     # exact zeros
                continue
            wp, wq = L.ref_rotate_lazy(pc[j], qc[j], alphas[j], betas[j])
            assert same_bits(cp, wp) and same_bits(cq, wq), (n, j)
            sp, sq = L.hook_rotate(1, n1, guard(pc[j]), guard(qc[j]), block_of(scal, j, sstride))
            assert same_bits(cp, sp[:n1]) and same_bits(cq, sq[:n1]), (n, j)      # bit for bit k_rotate_lazy


def finalize_case(rng, W, EL, n, npart, roles, sstride):
    """per-column partials at (3 j + t) * np + i, vectors and scalar blocks for the roles 'diff' (difference form),
    'sweep' (fallback sweep, built as test_fallback_sweep of tests/test_gpu_finalize.py), 'stopped' and 'done'"""
    n1 = n * EL
    pc, qc = rng.standard_normal((W, n1)), rng.standard_normal((W, n1))
    partial = np.zeros(3 * W * npart)
    sgs = [0.3 + 0.05 * j for j in range(W)]
    for j, role in enumerate(roles):
        a = (0.2 + 0.1 * j + 0.3 * rng.standard_normal(npart)) / npart
        q = (1.0 + rng.random(npart)) / npart
        v = (0.9 + 0.2 * rng.random(npart)) / npart
        if role == "sweep":
            v[:] = 0.0
            v[0] = 1.0
            d = L.strided_tree_sum(a) - sgs[j]
            q[:] = 0.0
            q[0] = d * d * (1.0 + 1e-5)
        partial[(3 * j) * npart:(3 * j + 3) * npart] = np.concatenate([a, q, v])
    scal = scal_blocks(W, sstride, alpha=sgs, beta=[0.7 + 0.1 * j for j in range(W)],
                       stop=[1.0 if r == "stopped" else 0.0 for r in roles],
                       ndone=[float(NLANC) if r == "done" else float(j % (NLANC - 1)) for j, r in enumerate(roles)],
                       norm=[1.25] * W)
    return pc, qc, partial, scal


@pytest.mark.parametrize("npart", L.NP_CASES)
@pytest.mark.parametrize("W,EL", L.WIDTHS)
def test_finalize_ab_multi_equals_the_single_seed_finalize(gpu, W, EL, npart):
    sstride = NSCAL + 3
    n = 777
    n1 = n * EL
    plans = [["sweep", "diff", "stopped", "done", "diff", "sweep", "diff", "diff"][:W]]
    if W == 2:
        plans.append(["stopped", "done"])
    for k, roles in enumerate(plans):
        rng = np.random.default_rng(3000 * W + 100 * EL + npart + k)
        pc, qc, partial, scal0 = finalize_case(rng, W, EL, n, npart, roles, sstride)
        P, Q = L.interleave(pc.ravel(), n, W, EL, W), L.interleave(qc.ravel(), n, W, EL, W)
        scal = L.hook_finalize_ab_multi(W, EL, n, guard(P), guard(Q), guard(partial), npart, scal0, sstride)
        want = scal0.copy()
        for j, role in enumerate(roles):
            if role in ("stopped", "done"):
                continue                       # a stopped column, and one with SC_NDONE >= nlanc, are not written
            pj = partial[(3 * j) * npart:(3 * j + 3) * npart]
            alpha, qq, vv = (L.strided_tree_sum(pj[t * npart:(t + 1) * npart]) for t in range(3))
            swept = L.beta2_from_sums(alpha, qq, vv, scal0[j * sstride + SC_ALPHA]) < 1e-3 * qq
            assert swept == (role == "sweep"), (j, role)
            # the single-seed kernel on the de-interleaved column, the step index from the device
            s1 = L.hook_finalize_ab(npart, pj.copy(), pc[j], qc[j], scal0[j * sstride:j * sstride + NSCAL].copy(), -1)
            want[j * sstride:j * sstride + NSCAL] = s1
            assert s1[SC_ALPHA] == alpha and s1[SC_NDONE] == scal0[j * sstride + SC_NDONE] + 1.0
            if swept:
                w = qc[j] - alpha * pc[j]
                assert L.ulp_diff(s1[SC_BETA], np.sqrt(L.strided_tree_sum(w * w)))[0] <= 4
        assert same_bits(scal, want), roles        # bit for bit, neighbours, gaps and tail included


# ---- edigpu_vec_* and the fused exchange forms on torch tensors ---------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.cpu().numpy()


def vec_lib():
    import torch
    from edipack_amd import capi
    lib = capi.lib()
    nwork = lib.edigpu_vec_work_doubles()
    assert nwork == RED
    return capi, lib, torch.cuda.current_stream().cuda_stream, nwork


@pytest.mark.parametrize("n", (0,) + L.ELEMENTWISE_LENGTHS)
def test_vec_rotate_scale_rotate_lazy(gpu, n):
    capi, lib, st, _ = vec_lib()
    rng = np.random.default_rng(110 * n + 1)
    p, q = rng.standard_normal(n), rng.standard_normal(n)
    for b2, exact in ((2.25, True), (1.7, False)):
        ok = same_bits if exact else within_4_ulp
        b = np.sqrt(b2)
        a, c, s = dev(guard(p)), dev(guard(q)), dev(np.array([b2, np.nan]))
        capi.check(lib.edigpu_vec_rotate(n, a.data_ptr(), c.data_ptr(), s.data_ptr(), st), "edigpu_vec_rotate")
        wp, wq = L.ref_rotate(p, q, b)
        assert ok(host(a)[:n], wp) and ok(host(c)[:n], wq) and tail_intact(host(a), n) and tail_intact(host(c), n)
        a = dev(guard(p))
        capi.check(lib.edigpu_vec_scale(n, a.data_ptr(), s.data_ptr(), st), "edigpu_vec_scale")
        assert ok(host(a)[:n], p * (1.0 / b)) and tail_intact(host(a), n)
        alpha = 0.5                                  # 0.25 + 2.25 and 2.5 - 0.25 are exact: beta^2 = 2.25 again
        a, c, ab = dev(guard(p)), dev(guard(q)), dev(np.array([alpha, alpha * alpha + b2, np.nan]))
        b_dev = np.sqrt((alpha * alpha + b2) - alpha * alpha)
        assert not exact or b_dev == 1.5
        capi.check(lib.edigpu_vec_rotate_lazy(n, a.data_ptr(), c.data_ptr(), ab.data_ptr(), st), "edigpu_vec_rotate_lazy")
        wp, wq = L.ref_rotate_lazy(p, q, alpha, b_dev)
        assert ok(host(a)[:n], wp) and ok(host(c)[:n], wq) and tail_intact(host(a), n) and tail_intact(host(c), n)


def run_vec_sum(name, n, vin, vout, third, nout):
    """edigpu_vec_add_dot / axpy_nrm2 / add_dot2: (vout, work, out) after the call; work holds exactly
    edigpu_vec_work_doubles() doubles followed by NaN"""
    capi, lib, st, nwork = vec_lib()
    a, c, t = dev(guard(vin)), dev(guard(vout)), dev(guard(third))
    work, out = dev(nans(nwork)), dev(nans(nout))
    capi.check(getattr(lib, name)(n, a.data_ptr(), c.data_ptr(), t.data_ptr(), out.data_ptr(), work.data_ptr(), st), name)
    return host(c), host(work), host(out)


@pytest.mark.parametrize("n", (0,) + L.REDUCE_LENGTHS)
def test_vec_add_dot_and_axpy_nrm2(gpu, n):
    rng = np.random.default_rng(120 * n + 1)
    vin, vout, tmp = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    nb = L.red_blocks(max(n, 1))
    wo, work, out = run_vec_sum("edigpu_vec_add_dot", n, vin, vout, tmp, 1)
    w = vout + tmp
    tot, part = L.device_sum(vin * w, nb)
    assert same_bits(wo[:n], w) and tail_intact(wo, n) and tail_intact(out, 1)
    assert same_bits(work[:nb], part) and np.all(np.isnan(work[nb:])) and out[0] == tot
    report("kv_add_dot+kv_sum", n, out[0], vin * w)
    alpha = 0.37
    wo, work, out = run_vec_sum("edigpu_vec_axpy_nrm2", n, vin, vout, np.array([alpha]), 1)
    w = vout - alpha * vin
    tot, part = L.device_sum(w * w, nb)
    assert same_bits(wo[:n], w) and tail_intact(wo, n) and tail_intact(out, 1)
    assert same_bits(work[:nb], part) and np.all(np.isnan(work[nb:])) and out[0] == tot
    report("kv_axpy_nrm2+kv_sum", n, out[0], w * w)
    if n == 0:
        assert out[0] == 0.0
    for i in L.spike_positions(n, nb):
        e = np.zeros(n)
        e[i] = 1.0
        _, _, out = run_vec_sum("edigpu_vec_add_dot", n, e, values(n), np.zeros(n), 1)
        assert out[0] == values(n)[i], i


@pytest.mark.parametrize("n", (0,) + L.SMALL_N + L.RED2_N + (262145,))
def test_vec_add_dot2(gpu, n):
    rng = np.random.default_rng(130 * n + 1)
    vin, vout, tmp = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    nb = L.red_blocks(max(n, 1), RED // 2)
    wo, work, out = run_vec_sum("edigpu_vec_add_dot2", n, vin, vout, tmp, 2)
    w = vout + tmp
    assert same_bits(wo[:n], w) and tail_intact(wo, n) and tail_intact(out, 2) and tail_intact(work, RED)
    for k, terms in enumerate((vin * w, w * w)):
        plane = work[k * (RED // 2):(k + 1) * (RED // 2)]
        assert same_bits(plane[:nb], L.block_partials(terms, nb)) and np.all(np.isnan(plane[nb:])), k
        assert out[k] == L.strided_tree_sum(plane[:nb]), k
        report(f"kv_add_dot2+kv_sum2[{k}]", n, out[k], terms)
    if n == 0:
        assert out[0] == 0.0 and out[1] == 0.0
    for i in L.spike_positions(n, nb):
        e = np.zeros(n)
        e[i] = 1.0
        _, _, out = run_vec_sum("edigpu_vec_add_dot2", n, e, values(n), np.zeros(n), 2)
        assert out[0] == values(n)[i], i


@pytest.mark.parametrize("geom", L.EXCHANGE_SMALL + (L.EXCHANGE_RED, L.EXCHANGE_EW), ids=str)
def test_transposed_rotate_pack_and_unpack_add_dot2(gpu, geom):
    capi, lib, st, nwork = vec_lib()
    world, du, nrows, q, halo = geom
    pcol = L.pcol_of(world, du)
    n, nx = nrows * du, world * q * (pcol + 2 * halo)
    rng = np.random.default_rng(du + 13 * nrows)
    v, w, tmp = rng.standard_normal(q * du), rng.standard_normal(q * du), rng.standard_normal(q * du)
    src = L.library_send_map(du, nrows, q, world, pcol, halo)
    alpha, b2 = 0.5, 2.25
    ab = dev(np.array([alpha, 2.5, np.nan]))          # beta^2 = 2.5 - 0.25 = 2.25 exactly
    for first in (1, 0):
        a, c, send = dev(guard(v)), dev(guard(w)), dev(nans(nx))
        capi.check(lib.edigpu_transpose_rotate_pack(first, du, nrows, q, world, pcol, halo, a.data_ptr(), c.data_ptr(), ab.data_ptr(),
                                                    send.data_ptr(), st), "edigpu_transpose_rotate_pack")
        vo, wo, so = host(a), host(c), host(send)
        if first:
            assert same_bits(vo, guard(v)) and same_bits(wo, guard(w))
        else:
            wv, ww = L.ref_rotate_lazy(v[:n], w[:n], alpha, np.sqrt(b2))
            assert same_bits(vo[:n], wv) and same_bits(wo[:n], ww)
            assert same_bits(vo[n:], guard(v)[n:]) and same_bits(wo[n:], guard(w)[n:])
        assert same_bits(so[:nx], np.where(src >= 0, vo[np.maximum(src, 0)], np.nan)) and tail_intact(so, nx)
    slots = L.back_slots(du, nrows, q, pcol, halo)
    back = np.full(nx, np.nan)
    back[slots] = rng.standard_normal(n)
    a, c, t, bk = dev(guard(v)), dev(guard(w)), dev(guard(tmp)), dev(guard(back))
    work, out = dev(nans(nwork)), dev(nans(2))
    capi.check(lib.edigpu_transpose_unpack_add_dot2(du, nrows, q, world, pcol, halo, a.data_ptr(), c.data_ptr(), t.data_ptr(),
                                                    bk.data_ptr(), out.data_ptr(), work.data_ptr(), st), "edigpu_transpose_unpack_add_dot2")
    wo, wk, o2 = host(c), host(work), host(out)
    wn = (w[:n] + tmp[:n]) + back[slots]
    nb = L.red_blocks(n, RED // 2)
    assert same_bits(wo[:n], wn) and same_bits(wo[n:], guard(w)[n:]) and tail_intact(o2, 2) and tail_intact(wk, RED)
    for k, terms in enumerate((v[:n] * wn, wn * wn)):
        plane = wk[k * (RED // 2):(k + 1) * (RED // 2)]
        assert same_bits(plane[:nb], L.block_partials(terms, nb)) and np.all(np.isnan(plane[nb:])), k
        assert o2[k] == L.strided_tree_sum(plane[:nb]), k
        report(f"kv_unpack_add_dot2+kv_sum2[{k}]", n, o2[k], terms)
