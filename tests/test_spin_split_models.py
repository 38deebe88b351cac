"""tests.common.make_models(..., spin_split=True): the down species gets one-body data of its own (Nspin = 2; bath
levels, hybridisations, the spin-diagonal impHloc block, the replica matrices of the down species), drawn from a second
generator so that the default call keeps every value.  The oracle's matrix of such a model is Hermitian and is not the
matrix of the spin-symmetric model: the guard of tests/test_host_builders.py that a switch does something."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.common import make_models

NORMAL = [("normal", 2, 2, (3, 2)), ("hybrid", 3, 3, (3, 3)), ("normal", 1, 4, (2, 3)), ("replica", 2, 2, (3, 3)),
          ("general", 2, 3, (4, 3))]
FLAT = [("normal", 2, 2, 5), ("hybrid", 2, 3, 4), ("replica", 2, 2, 5), ("general", 2, 2, 5)]


def _arrays(m):
    a = {k: np.asarray(getattr(m, k)) for k in ("be", "bv", "bu", "hloc", "hb", "vr", "vg")
         if getattr(m, k, None) is not None}
    if "bv" not in a:          # the oracle's replica / general models: vg[nspin * norb, nbath]
        a["bv"] = a["vg"].reshape(-1, m.norb, m.nbath)
    return a


@pytest.mark.parametrize("bath,norb,nbath,sec", NORMAL)
def test_normal_mode_split_keeps_the_up_species(bath, norb, nbath, sec):
    om0, pm0 = make_models("normal", bath, norb, nbath, seed=3)
    om, pm = make_models("normal", bath, norb, nbath, seed=3, spin_split=True)
    assert (om0.nspin, om.nspin, pm.nspin) == (1, 2, 2)
    for m0, m in ((om0, om), (pm0, pm)):
        a0, a = _arrays(m0), _arrays(m)
        assert a.keys() == a0.keys()
        assert np.array_equal(a["hloc"][0, 0], a0["hloc"][0, 0]) and a["hloc"].shape == (2, 2, norb, norb)
        assert not a["hloc"][0, 1].any() and not a["hloc"][1, 0].any()          # no spin mixing in normal mode
        assert np.array_equal(a["hloc"][1, 1], a["hloc"][1, 1].T) and not np.array_equal(a["hloc"][1, 1], a["hloc"][0, 0])
        assert np.array_equal(a["bv"][0], a0["bv"][0])
        if bath in ("normal", "hybrid"):
            assert np.array_equal(a["be"][0], a0["be"][0])
            assert not np.array_equal(a["be"][1], a["be"][0]) and not np.array_equal(a["bv"][1], a["bv"][0])
        else:
            assert a["hb"].shape == (2, 2, norb, norb, nbath) and np.array_equal(a["hb"][0, 0], a0["hb"][0, 0])
            assert not a["hb"][0, 1].any() and not a["hb"][1, 0].any()
            assert not np.array_equal(a["hb"][1, 1], a["hb"][0, 0])
            assert np.array_equal(a["hb"][1, 1], a["hb"][1, 1].transpose(1, 0, 2))
            # replica: one amplitude per bath element for both species; general: the down species has its own
            assert np.array_equal(a["bv"][1], a["bv"][0]) == (bath == "replica")
    ref = O.HNormal(om, *sec).dense()
    assert np.abs(ref - ref.T).max() < 1e-14
    assert np.abs(ref - O.HNormal(om0, *sec).dense()).max() > 1e-3       # the switch does something


@pytest.mark.parametrize("bath,norb,nbath,sec", FLAT)
def test_nonsu2_split_keeps_the_up_species(bath, norb, nbath, sec):
    om0, pm0 = make_models("nonsu2", bath, norb, nbath, seed=5)
    om, pm = make_models("nonsu2", bath, norb, nbath, seed=5, spin_split=True)
    for m0, m in ((om0, om), (pm0, pm)):
        a0, a = _arrays(m0), _arrays(m)
        assert np.array_equal(a["hloc"], a0["hloc"])
        if bath in ("normal", "hybrid"):
            assert np.array_equal(a["be"][0], a0["be"][0]) and np.array_equal(a["bv"][0], a0["bv"][0])
            assert np.array_equal(a["bu"], a0["bu"])
            assert not np.array_equal(a["be"][1], a["be"][0]) and not np.array_equal(a["bv"][1], a["bv"][0])
        else:                                   # both spin blocks of the replica matrices are drawn already
            assert all(np.array_equal(a[k], a0[k]) for k in a0)
    if bath in ("normal", "hybrid"):
        ref = O.HFlat(om, sec).dense()
        assert np.abs(ref - ref.conj().T).max() < 1e-14
        assert np.abs(ref - O.HFlat(om0, sec).dense()).max() > 1e-3


def test_default_call_is_unchanged():
    """spin_split=False draws what the function drew before the switch existed: the generator's own stream, restated."""
    for mode, bath, norb, nbath, seed in (("normal", "normal", 2, 3, 7), ("normal", "hybrid", 3, 5, 71),
                                          ("nonsu2", "hybrid", 2, 3, 11), ("superc", "normal", 2, 2, 13)):
        rng = np.random.default_rng(20260630 + seed)
        nspin = 2 if mode == "nonsu2" else 1
        nfoo = 1 if bath == "hybrid" else norb
        be = rng.uniform(-2, 2, (nspin, nfoo, nbath))
        bv = rng.uniform(0.1, 0.6, (nspin, norb, nbath))
        bd = rng.uniform(-0.1, 0.1, (nspin, nfoo, nbath)) if mode == "superc" else None
        bu = rng.uniform(0.0, 0.3, (nspin, norb, nbath)) if mode == "nonsu2" else None
        if nspin == 2:
            be[1], bv[1] = be[0], bv[0]
        om, pm = make_models(mode, bath, norb, nbath, seed=seed)
        for m in (om, pm):
            assert np.array_equal(m.be, be) and np.array_equal(m.bv, bv)
            assert bd is None or np.array_equal(m.bd, bd)
            assert bu is None or np.array_equal(m.bu, bu)
        if mode == "normal":
            a = rng.standard_normal((norb, norb))
            assert np.array_equal(om.hloc[0, 0], 0.3 * (a + a.T)) and om.hloc.shape == (1, 1, norb, norb)


def test_zero_dw_and_refusals():
    _, pm = make_models("normal", "normal", 2, 3, seed=41, spin_split=True, zero_dw=(1, 2))
    _, p0 = make_models("normal", "normal", 2, 3, seed=41, spin_split=True)
    assert pm.bv[1, 1, 2] == 0.0 and p0.bv[1, 1, 2] != 0.0 and pm.bv[0, 1, 2] == p0.bv[0, 1, 2] != 0.0
    z = pm.bv.copy()
    z[1, 1, 2] = p0.bv[1, 1, 2]
    assert np.array_equal(z, p0.bv)
    with pytest.raises(ValueError):
        make_models("superc", "normal", 2, 2, spin_split=True)
    with pytest.raises(ValueError):
        make_models("normal", "normal", 2, 2, zero_dw=(0, 0))
