"""The rows kernel's column ownership on the 16-bit image of an even row (csrc/kernels_normal.hip, LINES): a thread owns
two column pairs 128 columns apart, so that every vector access of a wave is one contiguous 1 KiB piece, and the image
is stored in that ownership order (csrc/host_pack.hpp: ell16_owned_col).

Same slots, same order, same fma chains as the 32-bit image with four adjacent columns per thread: H*v and the Lanczos
coefficients must be equal bit for bit (EDIGPU_ELL16=0 builds the 32-bit handle), and match the oracle.  The shapes
reach every way a pass of 2048 columns can be filled; the host-only test decodes the reordered image.
"""
import ctypes as C

import numpy as np
import pytest

from tests.common import make_models, rel_err

TOL = 1e-12  # tests/test_gpu_ell16.py

SHAPES = [
    # bath, norb, nbath, (nup, ndw), DimUp, rows per workgroup
    ("normal", 2, 3, (4, 2), 70, (1, 8)),       # less than one block of 128: the second pair of every lane is empty
    ("normal", 2, 4, (5, 5), 252, (1, 2, 4, 8)),  # the last block partly filled
    ("normal", 2, 5, (6, 2), 924, (1, 2)),      # 7 * 128 + 28: odd number of blocks, wave 3's second block partly filled
    ("normal", 2, 6, (7, 1), 3432, (1,)),       # second pass, second register set of the kept P, last block 104 columns
    ("normal", 2, 5, (4, 2), 495, (1, 4)),      # odd: the scalar path and the column-order image, untouched
    ("hybrid", 2, 8, (5, 2), 252, (1, 2)),      # Hnd terms (jxp != 0) of the sweep behind the new P
]
CASES = [(b, no, nb, sec, du, td) for b, no, nb, sec, du, tds in SHAPES for td in tds]


def _oracle():
    from oracle import oracle as O
    return O


def _layout_env(monkeypatch, layout):
    monkeypatch.setenv("EDIGPU_IB", "0")  # the generic rows kernel
    if layout == "panel":
        monkeypatch.setenv("EDIGPU_BLOCKED", "1")
        monkeypatch.setenv("EDIGPU_BLOCKED_MIN", "0")
        monkeypatch.setenv("EDIGPU_BLOCKED_W", "128")
        monkeypatch.setenv("EDIGPU_PANEL_VEC2_MIN", "0")
    else:
        monkeypatch.setenv("EDIGPU_BLOCKED", "0")


def _build(monkeypatch, pm, sec, ell16):
    from edipack_amd.hamiltonian import SectorHamiltonian
    if ell16:
        monkeypatch.delenv("EDIGPU_ELL16", raising=False)
    else:
        monkeypatch.setenv("EDIGPU_ELL16", "0")
    return SectorHamiltonian.normal_from_model(pm, *sec)


def _skip_if_switched():
    import os
    if os.environ.get("EDIGPU_NORMAL_EXPLICIT") or os.environ.get("EDIGPU_LANCZOS_UNFUSED") or os.environ.get("EDIGPU_ROW_SPLIT") \
            or os.environ.get("EDIGPU_ELL_UNTYPED"):
        pytest.skip("needs the typed LDS image, the fused step and whole rows in the LDS")


_REF = {}


def _reference(bath, norb, nbath, sec):
    """oracle handle, vectors, products and coefficients of a shape: computed once, shared, left unchanged"""
    key = (bath, norb, nbath, sec)
    if key not in _REF:
        O = _oracle()
        om, pm = make_models("normal", bath, norb, nbath, seed=31)
        ho = O.HNormal(om, *sec)
        rng = np.random.default_rng(77)
        vs = [rng.standard_normal(ho.dim) for _ in range(3)]
        ys = [ho.matvec(v) for v in vs[:2]]
        ao, bo, _ = ho.lanc_tridiag(vs[2], 40)
        for x in vs + ys + [ao, bo]:
            x.setflags(write=False)
        _REF[key] = (ho, pm, vs, ys, ao, bo)
    return _REF[key]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["natural", "panel"])
@pytest.mark.parametrize("bath,norb,nbath,sec,dimup,td", CASES)
def test_lines_match_ell32_and_oracle(gpu, monkeypatch, bath, norb, nbath, sec, dimup, td, layout):
    _skip_if_switched()
    ho, pm, vs, ys, ao, bo = _reference(bath, norb, nbath, sec)
    assert ho.dimup == dimup
    monkeypatch.setenv("EDIGPU_ROWS_TD", str(td))
    _layout_env(monkeypatch, layout)
    h16 = _build(monkeypatch, pm, sec, True)
    h32 = _build(monkeypatch, pm, sec, False)
    if bath == "hybrid":
        assert h16.image_info()[1] > 0   # factored Hnd terms (jxp = 0.25)
    assert h16.image_info()[4] == h32.image_info()[4] == (128 if layout == "panel" else 0)
    for v, ref in zip(vs, ys):
        y16, y32 = h16.apply(v), h32.apply(v)
        assert np.array_equal(y16, y32)
        assert rel_err(y16, ref) < TOL
        l16, l32 = h16.apply_loop(v), h32.apply_loop(v)
        assert np.array_equal(l16, l32)
        assert rel_err(l16, ref) < TOL
    n = 40
    for exact in (False, True):
        if exact:
            monkeypatch.setenv("EDIGPU_LANCZOS_EXACTBETA", "1")
        else:
            monkeypatch.delenv("EDIGPU_LANCZOS_EXACTBETA", raising=False)
        a16, b16, n16 = h16.lanczos_tridiag(vs[2], n)
        a32, b32, n32 = h32.lanczos_tridiag(vs[2], n)
        assert n16 == n32 == n
        assert np.array_equal(a16, a32) and np.array_equal(b16, b32)
        assert rel_err(a16[:15], ao[:15]) < 1e-10 and rel_err(b16[:15], bo[:15]) < 1e-10
    h16.destroy()
    h32.destroy()


# ---------------------------------------------------------------- the encoder (host only) ----------------------------------------------------------------

def _owned_col(pos):
    """the kernel's ownership map, restated: 512 threads, 2048 columns per pass; lane l of wave w owns the pairs
    {2l, 2l + 1} of the blocks 2w and 2w + 1 of the pass; position 4 t + e = the e-th column of thread t = 64 w + l"""
    ps, rem = divmod(pos, 2048)
    t, e = divmod(rem, 4)
    w, l = divmod(t, 64)
    return ps * 2048 + (2 * w + e // 2) * 128 + 2 * l + e % 2


def _random_typed_ell(rng, n, width):
    """rows of at most `width` entries, entry k of a row with the amplitude of hop type k: a typed image of that width"""
    amps = 0.1 + np.arange(width) * 0.37
    rows = []
    for i in range(n):
        keep = rng.random(width) < 0.7
        if i == 0:
            keep[:] = True   # one full row fixes the width
        cols = rng.integers(0, n, width)
        rows.append([(int(cols[k]), float(amps[k]) * (-1.0 if rng.random() < 0.5 else 1.0)) for k in range(width) if keep[k]])
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([c for r in rows for c, _ in r], np.int32)
    val = np.array([v for r in rows for _, v in r], np.float64)
    return rowptr, col, val


@pytest.mark.usefixtures("built")
@pytest.mark.parametrize("n", [70, 128, 129, 2048, 2049, 4094])
@pytest.mark.parametrize("width", [1, 2, 11, 12])
def test_ownership_order_image_is_the_column_order_image_permuted(n, width):
    from edipack_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(1000 * width + n)
    rowptr, col, val = _random_typed_ell(rng, n, width)
    info = np.zeros(5, np.int64)
    assert L.edigpu_ell16_images(n, capi.pi64(rowptr), capi.pi32(col), capi.pd(val), capi.pi64(info), None, None, None) == 0
    w, pitch, pitch_o, n16, n16o = (int(x) for x in info)
    npair = (width + 1) // 2
    assert w == width and pitch == (n + 63) // 64 * 64 and n16 == npair * pitch
    if n % 2:
        assert pitch_o == 0 and n16o == 0    # odd rows keep the column order (the scalar path)
        return
    assert pitch_o == (n + 255) // 256 * 256 and n16o == npair * pitch_o
    pk16, pk16o, owned = np.zeros(n16, np.uint32), np.zeros(n16o, np.uint32), np.zeros(pitch_o, np.int64)
    assert L.edigpu_ell16_images(n, capi.pi64(rowptr), capi.pi32(col), capi.pd(val), capi.pi64(info),
                                 pk16.ctypes.data_as(C.c_void_p), pk16o.ctypes.data_as(C.c_void_p), capi.pi64(owned)) == 0
    pk16, pk16o = pk16.reshape(npair, pitch), pk16o.reshape(npair, pitch_o)
    # the permutation is the kernel's ownership map ...
    want = np.array([_owned_col(p) for p in range(pitch_o)])
    assert np.array_equal(owned, want)
    live = want < n
    # ... every column stands at exactly one position, and its words are those of the column-order image
    assert np.array_equal(np.sort(want[live]), np.arange(n))
    assert np.array_equal(pk16o[:, live], pk16[:, want[live]])
    # every thread that owns a column of the row finds its four words inside the pitch
    first = np.array([_owned_col(4 * t) for t in range(pitch_o // 4 + 512)])
    assert (4 * np.nonzero(first < n)[0] + 3 < pitch_o).all()
    # positions of columns past the row, dead slots and the pad slot of an odd width name the zero slot
    dead = n * 8
    assert dead <= 0x7FFF
    assert (pk16o[:, ~live] == (dead | dead << 16)).all()
    if width % 2:
        assert ((pk16o[-1] >> 16) == dead).all()
    nnz_rows = np.diff(rowptr)
    lo, hi = pk16o & 0x7FFF, (pk16o >> 16) & 0x7FFF
    n_live = int(((lo != dead).sum() + (hi != dead).sum()))
    assert n_live == int(nnz_rows.sum())
    assert ((lo % 8 == 0) & (lo <= dead) & (hi % 8 == 0) & (hi <= dead)).all()
