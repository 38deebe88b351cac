"""The 16-bit typed image of Hup (rows of at most 4095 columns) against the 32-bit one and the oracle.

The rows kernel reads the same slots in the same order from either image, so H*v and the Lanczos coefficients are
the same bit for bit; EDIGPU_ELL16=0 (read at set-up: every (image, switch) pair builds its own handle) keeps a
qualifying sector on the 32-bit image.
"""
import numpy as np
import pytest

from tests.common import make_models, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-12  # test_gpu_parity.TOL (test_normal_apply_matches_oracle)

SECTORS = [
    # bath, norb, nbath, (nup, ndw)
    ("normal", 2, 4, (5, 5)),   # Ns = 10: DimUp = 252 (even), Dim = 63 504
    ("normal", 2, 5, (4, 2)),   # Ns = 12: DimUp = 495 (odd: the scalar access path), DimDw = 66
]


def _oracle():
    from oracle import oracle as O
    return O


def _layout_env(monkeypatch, layout):
    monkeypatch.setenv("EDIGPU_IB", "0")  # the generic rows kernel is what this file is about
    if layout == "panel":   # 128-column panels swept by the tiled kernel, forced on a small sector
        monkeypatch.setenv("EDIGPU_BLOCKED", "1")
        monkeypatch.setenv("EDIGPU_BLOCKED_MIN", "0")
        monkeypatch.setenv("EDIGPU_BLOCKED_W", "128")
        monkeypatch.setenv("EDIGPU_PANEL_VEC2_MIN", "0")
    else:
        monkeypatch.setenv("EDIGPU_BLOCKED", "0")


def _build(monkeypatch, ho, pm, sec, image, ell16, **shard):
    """shard: dw_first / dw_count of a library-built handle that owns a slice of the down rows"""
    from edipack_amd.hamiltonian import SectorHamiltonian
    if ell16:
        monkeypatch.delenv("EDIGPU_ELL16", raising=False)
    else:
        monkeypatch.setenv("EDIGPU_ELL16", "0")
    if image == "library":
        return SectorHamiltonian.normal_from_model(pm, *sec, **shard)
    return SectorHamiltonian.normal_from_arrays(ho.dimup, ho.dimdw, ho.hd, ho.up, ho.dw, ho.nd if ho.has_nd else None)


def _skip_if_switched():
    import os
    if os.environ.get("EDIGPU_NORMAL_EXPLICIT") or os.environ.get("EDIGPU_LANCZOS_UNFUSED") or os.environ.get("EDIGPU_ROW_SPLIT") \
            or os.environ.get("EDIGPU_ELL_UNTYPED"):
        pytest.skip("needs the typed LDS image, the fused step and whole rows in the LDS")


@pytest.mark.parametrize("td", [1, 2, 4, 8])
@pytest.mark.parametrize("layout", ["natural", "panel"])
@pytest.mark.parametrize("image", ["library", "handover"])
@pytest.mark.parametrize("bath,norb,nbath,sec", SECTORS)
def test_ell16_matches_ell32_and_oracle(gpu, monkeypatch, bath, norb, nbath, sec, image, layout, td):
    """(a) H*v and (b) the Lanczos coefficients (fused step with the pending axpy, and EDIGPU_LANCZOS_EXACTBETA=1)
    with the 16-bit image equal those with the 32-bit image bit for bit, and match the oracle."""
    _skip_if_switched()
    O = _oracle()
    om, pm = make_models("normal", bath, norb, nbath, seed=31)
    ho = O.HNormal(om, *sec)
    monkeypatch.setenv("EDIGPU_ROWS_TD", str(td))
    _layout_env(monkeypatch, layout)
    h16 = _build(monkeypatch, ho, pm, sec, image, True)
    h32 = _build(monkeypatch, ho, pm, sec, image, False)
    if image == "library":
        assert h16.image_info()[4] == h32.image_info()[4] == (128 if layout == "panel" else 0)
    rng = np.random.default_rng(77)
    for _ in range(2):
        v = rng.standard_normal(ho.dim)
        y16, y32 = h16.apply(v), h32.apply(v)
        assert np.array_equal(y16, y32)
        assert rel_err(y16, ho.matvec(v)) < TOL
    v = rng.standard_normal(ho.dim)
    n = 40
    ao, bo, _ = ho.lanc_tridiag(v, n)
    for exact in (False, True):
        if exact:
            monkeypatch.setenv("EDIGPU_LANCZOS_EXACTBETA", "1")
        else:
            monkeypatch.delenv("EDIGPU_LANCZOS_EXACTBETA", raising=False)
        a16, b16, n16 = h16.lanczos_tridiag(v, n)
        a32, b32, n32 = h32.lanczos_tridiag(v, n)
        assert n16 == n32 == n
        assert np.array_equal(a16, a32) and np.array_equal(b16, b32)
        # as test_lanczos_tridiag_matches_oracle: the first steps agree to rounding
        assert rel_err(a16[:15], ao[:15]) < 1e-10 and rel_err(b16[:15], bo[:15]) < 1e-10
    h16.destroy()
    h32.destroy()


def test_long_rows_keep_the_32bit_image(gpu, monkeypatch):
    """(c) DimUp = C(15, 7) = 6435 > 4095: no 16-bit image is built, the switch changes nothing."""
    _skip_if_switched()
    O = _oracle()
    om, pm = make_models("normal", "normal", 3, 4, seed=32)
    sec = (7, 1)
    ho = O.HNormal(om, *sec)
    assert ho.dimup == 6435
    _layout_env(monkeypatch, "natural")
    ha = _build(monkeypatch, ho, pm, sec, "library", True)
    hb = _build(monkeypatch, ho, pm, sec, "library", False)
    v = np.random.default_rng(78).standard_normal(ho.dim)
    ya, yb = ha.apply(v), hb.apply(v)
    assert np.array_equal(ya, yb)
    assert rel_err(ya, ho.matvec(v)) < TOL
    n = 30
    ao, bo, _ = ho.lanc_tridiag(v, n)
    aa, ba, _ = ha.lanczos_tridiag(v, n)
    ab, bb, _ = hb.lanczos_tridiag(v, n)
    assert np.array_equal(aa, ab) and np.array_equal(ba, bb)
    assert rel_err(aa[:15], ao[:15]) < 1e-10 and rel_err(ba[:15], bo[:15]) < 1e-10
    ha.destroy()
    hb.destroy()
