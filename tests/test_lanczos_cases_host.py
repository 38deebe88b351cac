"""The NumPy references of tests/lanczos_cases.py checked on the CPU, before any kernel is held to them: the restated
orders of summation agree with a long-double sum within the stated bound on every length of the case tables, the layout
restatements round-trip, and the restated send / back layouts agree with the library's own exchange maps
(edigpu_exchange_send_map / edigpu_exchange_back_map, host functions)."""
import numpy as np
import pytest

from tests import lanczos_cases as L


@pytest.mark.parametrize("n", L.REDUCE_LENGTHS + L.RED2_N + L.EW_N)
def test_restated_summation_is_within_the_bound(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    for cap in (L.RED, L.RED // 2):
        nb = L.red_blocks(n, cap)
        for terms in (x * x, x * rng.standard_normal(n)):      # one sign, and cancelling
            tot, part = L.device_sum(terms, nb)
            assert part.shape == (nb,)
            assert L.bound_ratio(tot, terms) <= 1.0
            # each workgroup's partial is the sum of its own elements
            per = nb * L.NT
            own = terms[:L.NT] if n <= per else np.concatenate([terms[k:k + L.NT] for k in range(0, n, per)])
            assert L.bound_ratio(part[0], own) <= 1.0


def test_restated_summation_on_exact_data():
    """integers: every order gives the same sum, so the bookkeeping of the restatement (trips, lanes, waves) is exact"""
    for n in (1, 65, 257, 262145, 524289):
        x = np.arange(n, dtype=np.float64) % 7.0 - 3.0
        for nb in (L.red_blocks(n), L.red_blocks(n, 512)):
            tot, part = L.device_sum(x, nb)
            assert tot == x.sum() == part.sum()
    for npart in L.NP_CASES:
        x = np.arange(npart, dtype=np.float64) % 5.0
        assert L.strided_tree_sum(x) == x.sum()


def test_pick_out_terms_survive_the_restated_sum():
    n = 262145
    nb = L.red_blocks(n)
    for i in L.spike_positions(n, nb):
        x = np.zeros(n)
        x[i] = 1.0 + i / 2.0 ** 20
        assert L.device_sum(x, nb)[0] == x[i]
    assert L.spike_positions(n, nb) == [0, 255, 256, 262143, 262144]


def test_exact_sums_give_an_exact_beta():
    a, b, b2 = L.ab_from_sums(L.EXACT_T, L.EXACT_TPREV)
    assert (a, b, b2) == (0.5, 1.5, 2.25)
    a, b, b2 = L.ab_from_sums(L.sums_for(0.75, 2.25), None)
    assert a == 0.75 and b == 1.5


@pytest.mark.parametrize("case", L.BLOCKED_CASES, ids=str)
def test_blocked_layout_round_trips(case):
    du, dd, sh = case
    src = 1.0 + np.arange(du * dd, dtype=np.float64)
    blk = L.to_blocked(src, du, dd, sh)
    assert len(blk) == L.blocked_len(du, dd, sh) and len(blk) % (dd << sh) == 0
    assert np.count_nonzero(blk) == du * dd                      # the padding, and only the padding, is zero
    assert np.array_equal(L.from_blocked(blk, du, dd, sh), src)
    # element (row, col) sits in panel col >> sh at (row << sh) + (col & mask)
    row, col = dd - 1, du - 1
    assert blk[(col >> sh) * (dd << sh) + (row << sh) + (col & ((1 << sh) - 1))] == src[row * du + col]


@pytest.mark.parametrize("W,EL", L.WIDTHS)
def test_interleave_round_trips(W, EL):
    n = L.mu_rows_below(W, EL)
    for g in (W, W - 1, 1):
        src = 1.0 + np.arange(g * n * EL, dtype=np.float64)
        xi = L.interleave(src, n, W, EL, g)
        assert np.count_nonzero(xi) == g * n * EL
        for j in range(W):
            want = src[j * n * EL:(j + 1) * n * EL] if j < g else np.zeros(n * EL)
            assert np.array_equal(L.column(xi, n, W, EL, j), want)
        dst = np.full(W * n * EL, -7.0)
        back = L.deinterleave(xi, n, W, EL, g, dst)
        assert np.array_equal(back[:g * n * EL], src) and np.all(back[g * n * EL:] == -7.0)


def test_second_trip_row_counts():
    assert L.mu_rows_second_trip_chunks(8, 2) == 131073 and L.mu_rows_second_trip_chunks(2, 1) == 1048577
    for W, EL in L.WIDTHS:
        assert (L.mu_rows_second_trip_chunks(W, EL) - 1) * W * EL // 2 == L.EW * L.NT
        assert (L.mu_rows_second_trip_elems(W) - 1) * W == L.EW * L.NT
        assert L.mu_rows_below(W, EL) * W * EL // 2 < L.EW * L.NT and L.mu_rows_below(W, EL) * W > L.NT


@pytest.mark.parametrize("geom", L.EXCHANGE_SMALL + (L.EXCHANGE_RED,), ids=str)
def test_send_and_back_layouts_agree_with_the_exchange_maps(built, geom):
    world, du, nrows, q, halo = geom
    pcol = L.pcol_of(world, du)
    src = L.library_send_map(du, nrows, q, world, pcol, halo)
    x = 1.0 + np.arange(q * du, dtype=np.float64)
    send = L.pack(x, du, nrows, q, world, pcol, halo, np.full(len(src), np.nan))
    want = np.where(src >= 0, x[np.maximum(src, 0)], np.nan)
    assert L.same_bits(send, want)
    slots, elems = L.send_slots(du, nrows, q, world, pcol, halo)
    assert len(np.unique(slots)) == len(slots) and set(elems) == set(range(nrows * du))
    assert np.array_equal(L.back_slots(du, nrows, q, pcol, halo), L.library_back_map(du, nrows, q, world, pcol, halo))
    # a halo column lands in every block that holds it; (7, 10, 3, 3, 3): blocks of 2 columns, narrower than the halo
    if geom == (7, 10, 3, 3, 3):
        assert np.max(np.bincount(elems)) > 2
