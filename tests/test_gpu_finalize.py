"""k_finalize_ab (csrc/kernels_lanczos.hip, csrc/lz_finalize.hpp): alpha and beta of a fused Lanczos step from the
per-workgroup partial sums, by one workgroup of 1024 threads.

However the kernel schedules its loads, the sums themselves are fixed: thread t adds the partials t, t + 1024, ... in
that order, then the pairwise tree with offsets 512 ... 1.  That summation is restated here in NumPy: alpha must be
equal bit for bit, beta to 4 ulp (its expression may contract into fma).  Driven through the test hook
edigpu_finalize_ab, and through a short recurrence for the form that takes the step index from the device.
"""
import numpy as np
import pytest

from tests.common import make_models, rel_err

pytestmark = pytest.mark.gpu

NT = 1024
SC_ALPHA, SC_BETA, SC_STOP, SC_NDONE, SC_NORM, SC_THR, SC_EXACT, SC_AB = 0, 1, 2, 3, 4, 5, 6, 8
NLANC = 6


def strided_tree_sum(x):
    """thread t of 1024 adds x[t], x[t + 1024], ... in that order to 0.0; then the pairwise tree, offsets 512 ... 1"""
    s = np.zeros(NT)
    for j in range(0, len(x), NT):
        part = x[j:j + NT]
        s[:len(part)] = s[:len(part)] + part
    off = NT // 2
    while off > 0:
        s[:off] = s[:off] + s[off:2 * off]
        off //= 2
    return s[0]


def expected(partial, npart, sg, P, Q):
    """alpha, beta^2 as the kernel computes them, and whether it swept the vectors for beta^2"""
    alpha, qq, vv = (strided_tree_sum(partial[k * npart:(k + 1) * npart]) for k in range(3))
    d = alpha - sg
    b2 = qq - 2.0 * d * (alpha - sg * vv) + d * d * vv
    swept = b2 < 1e-3 * qq
    if swept:
        w = Q - alpha * P
        b2 = strided_tree_sum(w * w)
    return alpha, b2, swept


def finalize(partial, npart, P, Q, scal, it):
    from edipack_amd import capi
    out = scal.copy()
    capi.check(capi.lib().edigpu_finalize_ab(npart, capi.pd(partial), len(P), capi.pd(P), capi.pd(Q), len(out), capi.pd(out),
                                             it, NLANC), "edigpu_finalize_ab")
    return out


def ulp_diff(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def make_case(rng, npart):
    """partials of a plausible step: <P|Q> = alpha ~ 0.2 from pieces of either sign, sum (Q - sg P)^2 ~ 1.5 and
    <P|P> ~ 1 from positive ones (beta^2 ~ 1.5 - (alpha - sg)^2: far from the fallback)"""
    partial = np.concatenate([(0.2 + 0.3 * rng.standard_normal(npart)) / npart, (1.0 + rng.random(npart)) / npart,
                              (0.9 + 0.2 * rng.random(npart)) / npart])
    n = 5000
    P, Q = rng.standard_normal(n), rng.standard_normal(n)
    scal = np.zeros(SC_AB + 2 * NLANC)
    scal[SC_ALPHA] = 0.3       # the previous alpha
    scal[SC_BETA] = 0.7
    scal[SC_NORM] = 1.25
    scal[SC_THR] = 1e-12
    scal[SC_EXACT] = 1.0
    return partial, P, Q, scal


def check_step(out, scal, partial, npart, P, Q, it, want_swept):
    alpha, b2, swept = expected(partial, npart, scal[SC_ALPHA], P, Q)
    assert swept == want_swept
    beta = np.sqrt(max(b2, 0.0))
    assert out[SC_ALPHA] == alpha and out[SC_AB + it] == alpha            # bit for bit
    assert ulp_diff(out[SC_BETA], beta) <= 4
    assert out[SC_NDONE] == it + 1 and out[SC_EXACT] == 0.0 and out[SC_STOP] == 0.0
    assert out[SC_NORM] == scal[SC_NORM] and out[SC_THR] == scal[SC_THR]
    want = scal.copy()
    for k in (SC_ALPHA, SC_BETA, SC_NDONE, SC_EXACT, SC_AB + it):
        want[k] = out[k]
    if it + 1 < NLANC:
        assert out[SC_AB + NLANC + it + 1] == out[SC_BETA]
        want[SC_AB + NLANC + it + 1] = out[SC_BETA]
    assert np.array_equal(out, want)                                      # nothing else is written


@pytest.mark.parametrize("npart", [1, 3, 1023, 1024, 1025, 3591, 4097])
def test_alpha_beta_from_partials(gpu, npart):
    """fewer partials than threads, a partly filled trip of the strided loop, and more than four trips (4097)"""
    rng = np.random.default_rng(npart)
    partial, P, Q, scal = make_case(rng, npart)
    for it in (2, NLANC - 1):
        out = finalize(partial, npart, P, Q, scal, it)
        check_step(out, scal, partial, npart, P, Q, it, False)


def test_step_index_from_the_device(gpu):
    """iter < 0: the step is scal[SC_NDONE]"""
    rng = np.random.default_rng(5)
    partial, P, Q, scal = make_case(rng, 3591)
    scal[SC_NDONE] = 3.0
    out = finalize(partial, 3591, P, Q, scal, -1)
    check_step(out, scal, partial, 3591, P, Q, 3, False)


@pytest.mark.parametrize("npart", [3, 3591])
def test_fallback_sweep(gpu, npart):
    """beta^2 from the difference form loses its digits (b2 < 1e-3 qq): the workgroup sweeps |Q - alpha P|^2 itself."""
    rng = np.random.default_rng(100 + npart)
    partial, P, Q, scal = make_case(rng, npart)
    # <P|P> = 1 and d = alpha - sg: b2 = qq - d^2; choose qq just above d^2
    partial[2 * npart:] = 0.0
    partial[2 * npart] = 1.0
    alpha = strided_tree_sum(partial[:npart])
    d = alpha - scal[SC_ALPHA]
    partial[npart:2 * npart] = 0.0
    partial[npart] = d * d * (1.0 + 1e-5)
    out = finalize(partial, npart, P, Q, scal, 1)
    check_step(out, scal, partial, npart, P, Q, 1, True)


def test_breakdown_sets_stop_and_a_stopped_recurrence_is_left_alone(gpu):
    rng = np.random.default_rng(9)
    npart = 1025
    partial, P, Q, scal = make_case(rng, npart)
    scal[SC_THR] = 1e3                    # beta lies below it
    out = finalize(partial, npart, P, Q, scal, 2)
    alpha, b2, swept = expected(partial, npart, scal[SC_ALPHA], P, Q)
    assert not swept and out[SC_ALPHA] == alpha and out[SC_AB + 2] == alpha
    assert ulp_diff(out[SC_BETA], np.sqrt(b2)) <= 4 and out[SC_BETA] < 1e3
    assert out[SC_STOP] == 1.0 and out[SC_NDONE] == 3.0
    assert out[SC_AB + NLANC + 3] == 0.0  # no beta is recorded for a step that ends the recurrence
    # the next step's launch finds the recurrence ended: scal stays as it is, for either form of the step index
    for it in (3, -1):
        again = finalize(rng.standard_normal(3 * npart), npart, P, Q, out, it)
        assert np.array_equal(again, out)
    # an exact zero ends it whatever the threshold is
    scal[SC_THR] = 0.0
    zero = np.zeros(3 * npart)
    out = finalize(zero, npart, P, Q * 0.0, scal * 0.0, 0)
    assert out[SC_STOP] == 1.0 and out[SC_BETA] == 0.0


def test_graph_replay_matches_the_plain_loop(gpu, monkeypatch):
    """EDIGPU_LANCZOS_GRAPH=1 (read at set-up): the later steps of a small sector are replayed from a captured graph whose
    finalize takes the step index from the device; same kernels, same coefficients."""
    from edipack_amd.hamiltonian import SectorHamiltonian
    from oracle import oracle as O
    om, pm = make_models("normal", "normal", 2, 3, seed=31)
    sec = (4, 4)
    ho = O.HNormal(om, *sec)
    v = np.random.default_rng(3).standard_normal(ho.dim)
    n = 40
    ao, bo, _ = ho.lanc_tridiag(v, n)
    monkeypatch.delenv("EDIGPU_LANCZOS_GRAPH", raising=False)
    hp = SectorHamiltonian.normal_from_model(pm, *sec)
    monkeypatch.setenv("EDIGPU_LANCZOS_GRAPH", "1")
    hg = SectorHamiltonian.normal_from_model(pm, *sec)
    a0, b0, n0 = hp.lanczos_tridiag(v, n)
    a1, b1, n1 = hg.lanczos_tridiag(v, n)
    assert n0 == n1 == n
    assert np.array_equal(a0, a1) and np.array_equal(b0, b1)
    assert rel_err(a1[:15], ao[:15]) < 1e-10 and rel_err(b1[:15], bo[:15]) < 1e-10
    hp.destroy()
    hg.destroy()
