"""normal_rows_kernel on rows of 2049 to 4095 columns, where it runs code that shorter rows leave dead: byte offsets with
bits 12 to 14 set beside the sign bit in the 16-bit hop table, the second column pass (c0 = NT * kE = 2048), and both
passes of the keep-P variant of the fused step (one row per workgroup on the 16-bit image).  Real Ns = 14 sectors
against the oracle, synthetic operators at the exact size boundaries against a long-double restatement, and the
short-row pairing (the same kernel in position order) at config 2's row length.  tests/test_host_pack.py shows on the
CPU that the sectors and operators of tests/rows_long_cases.py have the 16-bit image exactly where this file assumes it.
"""
import functools

import numpy as np
import pytest

from tests.common import make_models, rel_err
from tests.rows_long_cases import MODEL_SEED, POS_CASES, SECTORS, SYNTH_DIMUP, synth_matvec, synth_operator
from tests.test_gpu_ell16 import TOL, _build, _layout_env, _oracle, _skip_if_switched

pytestmark = pytest.mark.gpu

NLANC = 40


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def _sector(case):
    """oracle sector, model, two vectors with their oracle products, a Lanczos seed with the oracle's coefficients:
    computed once per sector, shared by every case on it"""
    bath, norb, nbath, sec = case
    om, pm = make_models("normal", bath, norb, nbath, seed=MODEL_SEED)
    ho = _oracle().HNormal(om, *sec)
    rng = np.random.default_rng(77)
    vs = _frozen(rng.standard_normal(ho.dim), rng.standard_normal(ho.dim))
    refs = _frozen(*[ho.matvec(v) for v in vs])
    v, = _frozen(rng.standard_normal(ho.dim))
    ao, bo, no = ho.lanc_tridiag(v, NLANC)
    assert no == NLANC and np.abs(bo[1:]).min() > 1e-3 * np.abs(bo).max()    # no breakdown near
    return ho, pm, vs, refs, v, _frozen(ao, bo)


def _lanczos_both(monkeypatch, h16, h32, v):
    """the fused step with the pending axpy, then EDIGPU_LANCZOS_EXACTBETA=1: bitwise equal on the two images"""
    out = []
    for exact in (False, True):
        if exact:
            monkeypatch.setenv("EDIGPU_LANCZOS_EXACTBETA", "1")
        else:
            monkeypatch.delenv("EDIGPU_LANCZOS_EXACTBETA", raising=False)
        a16, b16, n16 = h16.lanczos_tridiag(v, NLANC)
        a32, b32, n32 = h32.lanczos_tridiag(v, NLANC)
        assert n16 == n32 == NLANC
        assert np.array_equal(a16, a32) and np.array_equal(b16, b32)
        out.append((a16, b16))
    return out


# ---- 1. real sectors against the oracle ----------------------------------------------------------------------------------
# (no td = 8: normal_pick_rows_per_block ignores an override whose rows exceed 150 KiB; td = 4 on 14 down rows leaves a
# last workgroup with 2 live rows)
@pytest.mark.parametrize("td", [1, 2, 4])
@pytest.mark.parametrize("layout", ["natural", "panel"])
@pytest.mark.parametrize("image", ["library", "handover"])
@pytest.mark.parametrize("case", SECTORS, ids=lambda c: "%s-%d-%d-%d_%d" % (c[0], c[1], c[2], *c[3]))
def test_long_rows_ell16_matches_ell32_and_oracle(gpu, monkeypatch, case, image, layout, td):
    """The assertions of test_ell16_matches_ell32_and_oracle on rows of 3003 and 3432 columns; the fused run at td = 1 is
    the keep-P variant with both passes live."""
    _skip_if_switched()
    ho, pm, vs, refs, v, (ao, bo) = _sector(case)
    monkeypatch.setenv("EDIGPU_ROWS_TD", str(td))
    _layout_env(monkeypatch, layout)
    h16 = _build(monkeypatch, ho, pm, case[3], image, True)
    h32 = _build(monkeypatch, ho, pm, case[3], image, False)
    if image == "library":
        assert h16.image_info()[4] == h32.image_info()[4] == (128 if layout == "panel" else 0)
    for x, ref in zip(vs, refs):
        y16, y32 = h16.apply(x), h32.apply(x)
        assert np.array_equal(y16, y32)
        assert rel_err(y16, ref) < TOL
    for a16, b16 in _lanczos_both(monkeypatch, h16, h32, v):
        # as test_lanczos_tridiag_matches_oracle: the first steps agree to rounding
        assert rel_err(a16[:15], ao[:15]) < 1e-10 and rel_err(b16[:15], bo[:15]) < 1e-10
    h16.destroy()
    h32.destroy()


@pytest.mark.parametrize("td", [1, 4])
def test_long_rows_down_row_shards(gpu, monkeypatch, td):
    """Three shards of the 14 down rows (4, 1 and 9 rows, cut as in test_down_sweep_variants_match_oracle) in the
    two-phase form: the row tail (fewer live rows than td) and dw_first != 0 on the 16-bit image and on the 32-bit one."""
    import torch
    _skip_if_switched()
    case = SECTORS[0]
    ho, pm, vs, refs, _, _ = _sector(case)
    monkeypatch.setenv("EDIGPU_ROWS_TD", str(td))
    _layout_env(monkeypatch, "natural")
    vd = torch.from_numpy(vs[0]).cuda()
    cuts = [0, ho.dimdw // 3, ho.dimdw // 3 + 1, ho.dimdw]
    for ell16 in (True, False):
        out = []
        for first, last in zip(cuts[:-1], cuts[1:]):
            hs = _build(monkeypatch, ho, pm, case[3], "library", ell16, dw_first=first, dw_count=last - first)
            hv = torch.empty(hs.nloc, dtype=torch.float64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            hs.apply_local_dev(vd[hs.row_first:].data_ptr(), hv.data_ptr(), st)
            hs.apply_remote_dev(vd.data_ptr(), hv.data_ptr(), st)
            torch.cuda.synchronize()
            out.append(hv.cpu().numpy())
            hs.destroy()
        assert rel_err(np.concatenate(out), refs[0]) < TOL, ell16


# ---- 3. synthetic operators at the size boundaries, by hand-over -----------------------------------------------------------
def _lanczos_numpy(matvec, v, n):
    """the literal recurrence: q <- H p - beta p_old; alpha = <p|q>; q <- q - alpha p; beta = |q|; p_old, p <- p, q / beta"""
    a, b = np.zeros(n), np.zeros(n)
    p, q, beta = v / np.sqrt(v @ v), np.zeros_like(v), 0.0
    for k in range(n):
        if k:
            p, q = q / beta, -beta * p
            b[k] = beta
        q = q + matvec(p)
        a[k] = p @ q
        q = q - a[k] * p
        beta = np.sqrt(q @ q)
    return a, b


@functools.lru_cache(maxsize=None)
def _synthetic(n):
    op = synth_operator(n)
    rng = np.random.default_rng(9000 + n)
    vs = _frozen(rng.standard_normal(op.dim), np.ones(op.dim))
    # reference in long double, rounded to double.  An output element is a chain of K = 1 + 6 + 5 fused multiply-adds of
    # exactly stored amplitudes: any order stays within (K + 1) u (|H||v|)_i of the exact value, the rounded reference
    # within u (|H||v|)_i: the bound asserted is 2 (K + 2) u (|Hd||v| + |Hup||v| + |Hdw||v|)_i, u = 2^-53.
    K = 1 + 6 + op.dimdw
    refs = []
    for x in vs:
        y, mag = synth_matvec(op, x, np.longdouble)
        refs.append(_frozen(y.astype(np.float64), (2 * (K + 2) * 2.0 ** -53 * mag).astype(np.float64)))
    v, = _frozen(rng.standard_normal(op.dim))
    ar, br = _lanczos_numpy(lambda x: synth_matvec(op, x)[0], v, NLANC)
    return op, vs, refs, v, _frozen(ar, br)


@pytest.mark.parametrize("td", [1, 2, 4])
@pytest.mark.parametrize("n", SYNTH_DIMUP)
def test_synthetic_rows_at_the_size_boundaries(gpu, monkeypatch, n, td):
    """DimUp at 2048 / 2049 / 2050 (the second keep-P pass empty, one column, one double2), 4094 / 4095 (the largest
    offsets the 16-bit entry holds) and 4096 / 4097 (32-bit image only, where the 16 / 32 comparison is trivially true:
    test_host_pack shows the 16-bit image absent there).  No Hnd: the explicit image is fusable, td = 1 keeps P."""
    _skip_if_switched()
    assert np.finfo(np.longdouble).eps < 2.0 ** -60     # the reference is more precise than the kernel
    op, vs, refs, v, (ar, br) = _synthetic(n)
    assert np.abs(br[1:]).min() > 1e-3 * np.abs(br).max()    # the coefficient comparison means nothing near a breakdown
    monkeypatch.setenv("EDIGPU_ROWS_TD", str(td))
    _layout_env(monkeypatch, "natural")
    h16 = _build(monkeypatch, op, None, None, "handover", True)
    h32 = _build(monkeypatch, op, None, None, "handover", False)
    for x, (ref, bound) in zip(vs, refs):
        y16, y32 = h16.apply(x), h32.apply(x)
        assert np.array_equal(y16, y32)
        excess = np.abs(y16 - ref) - bound
        assert (excess <= 0).all(), (int(np.argmax(excess)), float(excess.max()))
    for a16, b16 in _lanczos_both(monkeypatch, h16, h32, v):
        # two independent recurrences (test_lanczos_tridiag_matches_oracle)
        assert rel_err(a16[:15], ar[:15]) < 1e-10 and rel_err(b16[:15], br[:15]) < 1e-10
    h16.destroy()
    h32.destroy()


# ---- 4. the short-row pairing at config 2's row length ---------------------------------------------------------------------
@pytest.mark.parametrize("case,rows", POS_CASES, ids=lambda c: c if isinstance(c, int) else "%s-%d-%d-%d_%d" % (c[0], c[1], c[2], *c[3]))
def test_position_order_rows_past_the_first_column_pass(gpu, monkeypatch, case, rows):
    """test_local_block_kernels_match_oracle with cw = 0 on rows of 3432 columns: the padded row is longer than 2048
    positions, so the rows kernel in position order (image kind 5) runs its second column pass."""
    import os
    from edipack_amd.hamiltonian import SectorHamiltonian
    from tests.test_gpu_parity import _cf
    if os.environ.get("EDIGPU_NORMAL_EXPLICIT") or os.environ.get("EDIGPU_LANCZOS_UNFUSED") or os.environ.get("EDIGPU_ROW_SPLIT") \
            or os.environ.get("EDIGPU_IB_SPLIT") == "1" or os.environ.get("EDIGPU_SB") == "0":
        pytest.skip("needs the whole-row impurity-block image and the local-block tables")
    ho, pm, vs, refs, v, (ao, bo) = _sector(case)
    assert ho.dimup == 3432
    monkeypatch.setenv("EDIGPU_IB", "1")
    monkeypatch.setenv("EDIGPU_IB_MIN", "0")
    monkeypatch.setenv("EDIGPU_IB_ROWS", str(rows))
    monkeypatch.setenv("EDIGPU_POSROWS", "1")
    monkeypatch.setenv("EDIGPU_SB_CW", "2")
    hb = SectorHamiltonian.normal_from_model(pm, *case[3])
    assert hb.image_info()[5] == 5 and hb.image_info()[4] == 16
    for x, ref in zip(vs, refs):
        assert rel_err(hb.apply(x), ref) < TOL
    for step in ("1", "0"):                                      # fused step on the local-block kernels / default pairing
        monkeypatch.setenv("EDIGPU_SB_STEP", step)
        ab, bb, nb = hb.lanczos_tridiag(v, NLANC)
        assert nb == NLANC
        assert rel_err(ab[:15], ao[:15]) < 1e-10 and rel_err(bb[:15], bo[:15]) < 1e-10
        for z in (40.0 + 0.1j, 25.0j):
            assert abs(_cf(ab, bb, z) - _cf(ao, bo, z)) / abs(_cf(ao, bo, z)) < 1e-10
    monkeypatch.setenv("EDIGPU_SB_STEP", "1")
    monkeypatch.setenv("EDIGPU_LANCZOS_EXACTBETA", "1")          # the literal two-reduction recurrence, no lazy axpy
    ae, be, _ = hb.lanczos_tridiag(v, NLANC)
    assert rel_err(ae[:15], ao[:15]) < 1e-10 and rel_err(be[:15], bo[:15]) < 1e-10
    hb.destroy()
