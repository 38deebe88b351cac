"""CPU tests of the shard views behind the observables on sharded vectors (edigpu_occ_moments_sharded and its kin): the
tables of a rank's rows [first, first + count) made by occ_shard_view (csrc/host_occ.cpp) and ph_shard_plan_normal / _flat
(csrc/host_ph.cpp), through tests/host_shard_view.cpp, and the error paths that need no device.

The ranks' ranges are those of edigpu_shard_plan: q = ceil(n / world) rows per rank, rank r starts at min(r q, n).  The
views are asked for the uncut range (r q, q), so the cut to the sector is part of what is tested."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from edipack_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, L, I = C.c_void_p, C.c_int64, C.c_int
NORB, NPAT = 3, 8
DIMS_DW = [1, 8, 15, 56, 70]
WORLDS = [1, 2, 3, 5, 10]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_shard_view") / "host_shard_view.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", so,
                           os.path.join(ROOT, "tests", "host_shard_view.cpp"), os.path.join(csrc, "host_occ.cpp"),
                           os.path.join(csrc, "host_ph.cpp")])
    lib = C.CDLL(so)
    lib.hsv_occ_view.restype = L
    lib.hsv_occ_view.argtypes = [VP, L, I, I, L, L, VP, VP, VP, VP, VP]
    lib.hsv_ph_plan_normal.argtypes = [VP, L, VP, L, L, L, I, L, VP, VP, VP, VP, I, VP]
    lib.hsv_ph_plan_flat.argtypes = [VP, L, L, L, I, L, VP, VP, VP, VP, I, VP]
    return lib


def _patterns(n, seed, bits=NORB):
    return np.random.default_rng(seed).integers(0, 2 ** bits, size=n).astype(np.uint16)


def _occ_view(shim, pat, flat, nblk, first, count):
    n = pat.size
    rng, run = np.zeros(4, np.int64), np.full(33, -1, np.int32)
    pu, pd, order = np.zeros(n, np.uint16), np.zeros(n, np.uint8), np.full(n * nblk, -1, np.int32)
    m = shim.hsv_occ_view(pat.ctypes.data, n, int(flat), nblk, first, count, rng.ctypes.data, pu.ctypes.data, pd.ctypes.data,
                          order.ctypes.data, run.ctypes.data)
    return rng, pu[:rng[2]], pd[:rng[3]], order[:m], run


@pytest.mark.parametrize("nblk", [1, 4])
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("dim_dw", DIMS_DW)
def test_normal_views_name_every_row_of_every_block_once(shim, dim_dw, nblk, world):
    pd = _patterns(dim_dw, 100 + dim_dw)
    q = -(-dim_dw // world)
    seen = np.zeros((nblk, dim_dw), int)
    for r in range(world):
        first, count = min(r * q, dim_dw), max(0, min(q, dim_dw - min(r * q, dim_dw)))
        rng, pu, pdl, order, run = _occ_view(shim, pd, False, nblk, r * q, q)
        assert (rng[0], rng[1]) == (first, count) and pu.size == 0
        assert np.array_equal(pdl, pd[first:first + count].astype(np.uint8))
        if count == 0:                                      # a rank past the last row: empty tables
            assert order.size == 0 and not run.any()
            continue
        # every local row of every block exactly once
        assert np.array_equal(np.sort(order), np.arange(count * nblk))
        np.add.at(seen, (order // count, first + order % count), 1)
        # runs sorted by down pattern, stable, with the right lengths
        assert run[0] == 0 and np.all(run[NPAT:] == order.size) and np.all(np.diff(run) >= 0)
        for p in range(NPAT):
            rows = order[run[p]:run[p + 1]]
            assert rows.size == nblk * int(np.sum(pdl == p))
            assert np.all(pdl[rows % count] == p) and np.all(np.diff(rows) > 0)
    assert np.all(seen == 1)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("n", DIMS_DW)
def test_flat_views_are_the_slices_of_the_state_patterns(shim, n, world):
    pat = _patterns(n, 200 + n, bits=2 * NORB)
    q = -(-n // world)
    got = []
    for r in range(world):
        rng, pu, pdl, order, run = _occ_view(shim, pat, True, 4, r * q, q)
        first = min(r * q, n)
        assert rng[0] == first and rng[1] == pu.size == max(0, min(q, n - first))
        assert pdl.size == 0 and order.size == 0 and not run.any()
        got.append(pu)
    assert np.array_equal(np.concatenate(got), pat)


def _class_word(p):
    return sum(((p >> a) & 1) * 3 ** a for a in range(NORB))


def _plan(shim, normal, pu, pd, first, count, target):
    dims = np.zeros(3, np.int64)
    nrow, ncol = (pd.size, pu.size) if normal else (1, pu.size)
    cap = 4 * NPAT * NPAT + (nrow * ncol) // max(target, 1) + 64
    rorder, corder = np.full(max(nrow, 1), -1, np.int32), np.full(max(ncol, 1), -1, np.int32)
    units, ubeg = np.zeros((cap, 6), np.int32), np.zeros(3 ** NORB + 1, np.int32)
    if normal:
        rc = shim.hsv_ph_plan_normal(pu.ctypes.data, pu.size, pd.ctypes.data, pd.size, first, count, NORB, target,
                                     dims.ctypes.data, rorder.ctypes.data, corder.ctypes.data, units.ctypes.data, cap,
                                     ubeg.ctypes.data)
    else:
        rc = shim.hsv_ph_plan_flat(pu.ctypes.data, pu.size, first, count, NORB, target, dims.ctypes.data,
                                   rorder.ctypes.data, corder.ctypes.data, units.ctypes.data, cap, ubeg.ctypes.data)
    assert rc == 0
    return dims, rorder, corder, units[:dims[2]], ubeg


def _unit_elements(u, rorder, corder, dim_cols):
    r0, c0, ncols, cls, p0, p1 = (int(x) for x in u)
    p = np.arange(p0, p1)
    return rorder[r0 + p // ncols].astype(np.int64) * dim_cols + corder[c0 + p % ncols], cls


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("dim_dw", DIMS_DW)
def test_normal_phonon_plans_cover_the_shards_by_class(shim, dim_dw, world):
    """every element (local row, column) of a rank's block in exactly one unit, of the class of its two patterns; the
    units sorted by class with ubeg delimiting them; the ranks together hold every row of the sector"""
    dim_up = 20
    pu, pd = _patterns(dim_up, 7), _patterns(dim_dw, 300 + dim_dw)
    q = -(-dim_dw // world)
    rows = 0
    for r in range(world):
        first, count = min(r * q, dim_dw), max(0, min(q, dim_dw - min(r * q, dim_dw)))
        dims, rorder, corder, units, ubeg = _plan(shim, True, pu, pd, r * q, q, target=64)
        assert (dims[0], dims[1]) == (count, dim_up)
        rows += count
        if count == 0:
            assert units.shape[0] == 0 and not ubeg.any()
            continue
        seen = np.zeros(count * dim_up, int)
        for k, u in enumerate(units):
            e, cls = _unit_elements(u, rorder, corder, dim_up)
            seen[e] += 1
            want = np.array([_class_word(int(pu[i % dim_up])) + _class_word(int(pd[first + i // dim_up])) for i in e])
            assert np.all(want == cls) and ubeg[cls] <= k < ubeg[cls + 1]
        assert np.all(seen == 1) and np.all(np.diff(units[:, 3]) >= 0) and ubeg[-1] == units.shape[0]
    assert rows == dim_dw


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("n", DIMS_DW)
def test_flat_phonon_plans_cover_the_shards_by_class(shim, n, world):
    pat = _patterns(n, 400 + n, bits=2 * NORB)
    q = -(-n // world)
    for r in range(world):
        first, count = min(r * q, n), max(0, min(q, n - min(r * q, n)))
        dims, rorder, corder, units, ubeg = _plan(shim, False, pat, None, r * q, q, target=16)
        assert (dims[0], dims[1]) == (1, count)
        seen = np.zeros(count, int)
        for k, u in enumerate(units):
            e, cls = _unit_elements(u, rorder, corder, count)
            seen[e] += 1
            want = np.array([_class_word(int(pat[first + i]) & 7) + _class_word(int(pat[first + i]) >> NORB) for i in e])
            assert np.all(want == cls) and ubeg[cls] <= k < ubeg[cls + 1]
        assert np.all(seen == 1) and ubeg[-1] == units.shape[0]


def test_null_arguments_are_refused_with_a_message(built):
    lib = capi.lib()
    w, buf = np.zeros(5), np.zeros(100)
    assert lib.edigpu_occ_moments_sharded(None, None, None, 1, capi.pd(buf), capi.pd(w)) != 0
    assert "edigpu_occ_moments_sharded" in capi.last_error() and "NULL" in capi.last_error()
    assert lib.edigpu_apply_occ_sharded(None, None, None, None, capi.pd(w), capi.pd(w)) != 0
    assert "edigpu_apply_occ_sharded" in capi.last_error() and "NULL" in capi.last_error()
    assert lib.edigpu_apply_xph_sharded(None, None, None, None) != 0
    assert "edigpu_apply_xph_sharded" in capi.last_error() and "NULL" in capi.last_error()
    assert lib.edigpu_ph_rdm_sharded(None, None, None, 1, capi.pd(buf), capi.pd(w)) != 0
    assert "edigpu_ph_rdm_sharded" in capi.last_error() and "NULL" in capi.last_error()
