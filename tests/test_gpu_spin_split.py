"""Spin-resolved one-body data (Nspin = 2) through every kernel family, against the CPU oracle.

The models of the other GPU tests give both spin species the same bath levels, hybridisations and impHloc block, so a
kernel, an argument struct or an upload that read the up species' table for the down species would pass them all.  Here
make_models(..., spin_split=True) draws the down species' numbers on their own (tests/test_spin_split_models.py), and
the sectors include nup == ndw, where a swapped table has the right length and only the numbers show it.

Most tests run the body of the test they mirror (tests/test_gpu_parity.py, tests/test_gpu_tile_gathers.py) on such a
model: the `split` fixture hands those modules a make_models that sets spin_split=True and records what it made, so the
assertions, tolerances, image_info() checks and skips are the mirrored test's own, line for line.  The last part pins
the reference's antiferromagnet fixture (test/src/INEQ_NORMAL_NORMAL) from GPU eigenvectors."""
import os

import numpy as np
import pytest

import tests.test_gpu_parity as P
import tests.test_gpu_tile_gathers as TG
from tests.common import afm_site_models, csr_to_dense, make_models, rel_err
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu


def _is_split(pm):
    """the down species' one-body data differs from the up species' in every family the model has"""
    hl = np.asarray(pm.hloc)
    if pm.nspin != 2:
        return False
    if pm.ed_mode == "normal" and (np.array_equal(hl[1, 1], hl[0, 0]) or hl[0, 1].any() or hl[1, 0].any()):
        return False
    if pm.hb is not None:
        return not np.array_equal(np.asarray(pm.hb)[1, 1], np.asarray(pm.hb)[0, 0])
    return not np.array_equal(pm.be[1], pm.be[0]) and not np.array_equal(pm.bv[1], pm.bv[0])


def _split_models(*a, **k):
    k.setdefault("spin_split", True)
    om, pm = make_models(*a, **k)
    assert _is_split(pm) and om.nspin == 2
    return om, pm


@pytest.fixture
def split(monkeypatch):
    """tests.test_gpu_parity / test_gpu_tile_gathers build their models with spin_split=True for the length of a test;
    the list returned holds every model pair they made."""
    made = []

    def mm(*a, **k):
        made.append(_split_models(*a, **k))
        return made[-1]

    monkeypatch.setattr(P, "make_models", mm)
    monkeypatch.setattr(TG, "make_models", mm)
    return made


# --------------------------------------------------------------------------------------------
# a. generic kernels: factored and explicit image, hand-over, untyped / 32-bit ELL
# --------------------------------------------------------------------------------------------
GENERIC_CASES = [
    ("normal", 2, 2, (3, 3)),
    ("hybrid", 3, 5, (4, 4)),
    ("normal", 2, 3, (4, 3)),
    ("normal", 2, 3, (8, 0)),      # DimUp = 1: only the down species' tables are walked
    ("replica", 2, 2, (3, 3)),
    ("general", 3, 2, (4, 5)),
]


def _check_generic(hg, ho):
    """export_normal() against the oracle's arrays (test_normal_builder_matches_oracle), two products
    (test_normal_apply_matches_oracle) and a 20-step tridiagonalisation (test_lanczos_tridiag_matches_oracle's bound)."""
    assert (hg.dim_up, hg.dim_dw, hg.dim) == (ho.dimup, ho.dimdw, ho.dim)
    hd, up, dw, nd = hg.export_normal()
    assert rel_err(hd, ho.hd) < 1e-13
    assert np.allclose(csr_to_dense(*up, ho.dimup), csr_to_dense(*ho.up, ho.dimup), rtol=0, atol=1e-14)
    assert np.allclose(csr_to_dense(*dw, ho.dimdw), csr_to_dense(*ho.dw, ho.dimdw), rtol=0, atol=1e-14)
    if ho.has_nd and ho.dim <= 4000:
        assert np.allclose(csr_to_dense(*nd, ho.dim), csr_to_dense(*ho.nd, ho.dim), rtol=0, atol=1e-14)
    rng = np.random.default_rng(12345)
    for _ in range(2):
        v = rng.standard_normal(ho.dim)
        assert rel_err(hg.apply(v), ho.matvec(v)) < TOL
    n = min(20, ho.dim)
    k = min(15, n)
    ao, bo, _ = ho.lanc_tridiag(v, n)
    ag, bg, _ = hg.lanczos_tridiag(v, n)
    assert rel_err(ag[:k], ao[:k]) < 1e-10 and rel_err(bg[:k], bo[:k]) < 1e-10


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("bath,norb,nbath,sec", GENERIC_CASES)
def test_generic_kernels_spin_split(gpu, monkeypatch, bath, norb, nbath, sec, explicit):
    from oracle import oracle as O
    from edipack_amd.hamiltonian import SectorHamiltonian
    if explicit:
        monkeypatch.setenv("EDIGPU_NORMAL_EXPLICIT", "1")
    om, pm = _split_models("normal", bath, norb, nbath, seed=3)
    ho = O.HNormal(om, *sec)
    if sec[0] == sec[1]:      # equal table lengths on both sides, different numbers
        assert not np.allclose(csr_to_dense(*ho.up, ho.dimup), csr_to_dense(*ho.dw, ho.dimdw), rtol=0, atol=1e-3)
    hg = SectorHamiltonian.normal_from_model(pm, *sec)
    assert hg.image_info()[0] == int(not os.environ.get("EDIGPU_NORMAL_EXPLICIT"))
    _check_generic(hg, ho)
    hg.destroy()


@pytest.mark.parametrize("factor", [True, False])
def test_handover_arrays_spin_split(gpu, monkeypatch, split, factor):
    """test_normal_create_from_reference_arrays on the oracle's arrays of a spin-split model (EDIGPU_HANDOVER_FACTOR 1, 0)."""
    P.test_normal_create_from_reference_arrays(gpu, monkeypatch, factor)
    assert len(split) == 1


@pytest.mark.parametrize("switch", ["EDIGPU_ELL_UNTYPED=1", "EDIGPU_ELL16=0"])
def test_ell_variants_spin_split(gpu, monkeypatch, switch):
    """The (column, value) ELL image and the 32-bit typed image of H up / H dw (read at set-up), nup == ndw."""
    from oracle import oracle as O
    from edipack_amd.hamiltonian import SectorHamiltonian
    monkeypatch.setenv(*switch.split("="))
    om, pm = _split_models("normal", "hybrid", 3, 5, seed=3)
    ho = O.HNormal(om, 4, 4)
    hg = SectorHamiltonian.normal_from_model(pm, 4, 4)
    assert hg.image_info()[0] == int(not os.environ.get("EDIGPU_NORMAL_EXPLICIT"))
    _check_generic(hg, ho)
    hg.destroy()


# --------------------------------------------------------------------------------------------
# b. impurity-block image, whole rows and rows staged in halves
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [480, 24])
@pytest.mark.parametrize("bath,norb,nbath,sec", [
    ("normal", 2, 3, (4, 4)),
    ("hybrid", 3, 5, (4, 3)),
    ("normal", 1, 8, (4, 5)),
    ("hybrid", 3, 5, (1, 6)),
    ("replica", 2, 3, (4, 4)),
    ("general", 3, 2, (5, 4)),
])
def test_impurity_block_image_spin_split(gpu, monkeypatch, split, rows, bath, norb, nbath, sec):
    P.test_impurity_block_image_matches_oracle(gpu, monkeypatch, rows, bath, norb, nbath, sec, {})
    assert len(split) == 1


@pytest.mark.parametrize("rows", [480, 12])
@pytest.mark.parametrize("bath,norb,nbath,sec", [
    ("hybrid", 3, 5, (4, 3)),
    ("normal", 1, 8, (4, 5)),
    ("hybrid", 2, 7, (5, 4)),
])
@pytest.mark.parametrize("local_blocks", [0, 1])
def test_impurity_block_split_rows_spin_split(gpu, monkeypatch, split, local_blocks, rows, bath, norb, nbath, sec):
    P.test_impurity_block_split_rows_match_oracle(gpu, monkeypatch, local_blocks, rows, bath, norb, nbath, sec, {})
    assert len(split) == 1


# --------------------------------------------------------------------------------------------
# c. local-block kernels (both EDIGPU_SB_STEP values and EDIGPU_LANCZOS_EXACTBETA=1 inside the mirrored body)
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cw", [2, 1, 0])
@pytest.mark.parametrize("bath,norb,nbath,sec", [
    ("normal", 2, 3, (4, 4)),
    ("hybrid", 3, 5, (4, 3)),
    ("hybrid", 3, 6, (4, 5)),
    ("normal", 1, 8, (4, 5)),
])
def test_local_block_kernels_spin_split(gpu, monkeypatch, split, cw, bath, norb, nbath, sec):
    P.test_local_block_kernels_match_oracle(gpu, monkeypatch, cw, 24, bath, norb, nbath, sec, {})
    assert len(split) == 1


def test_local_block_kernels_down_hop_missing(gpu, monkeypatch, split):
    """cw = 1 sets EDIGPU_SB_AMODE=1 (the per-orbital walk); the down species has one walked level without a hop
    (v[1, 1, 2] = 0), so its korb mask is not the up species'."""
    P.test_local_block_kernels_match_oracle(gpu, monkeypatch, 1, 24, "normal", 2, 3, (4, 4), dict(zero_dw=(1, 2)))
    assert len(split) == 1 and split[0][1].bv[1, 1, 2] == 0.0 and split[0][1].bv[0, 1, 2] != 0.0


# --------------------------------------------------------------------------------------------
# d. panel-major loop and tiled column sweep
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [16, 64, 128])
@pytest.mark.parametrize("bath,norb,nbath,sec,jxp", [
    ("normal", 2, 3, (4, 4), 0.25),
    ("hybrid", 3, 5, (4, 3), 0.25),
    ("normal", 2, 4, (5, 5), 0.0),
])
def test_panel_major_lanczos_spin_split(gpu, monkeypatch, split, w, bath, norb, nbath, sec, jxp):
    P.test_panel_major_lanczos_matches_oracle(gpu, monkeypatch, w, bath, norb, nbath, sec, jxp)
    assert len(split) == 1


@pytest.mark.parametrize("tile_rows", [8, None])
@pytest.mark.parametrize("bath,norb,nbath,sec", [("normal", 2, 3, (4, 4)), ("hybrid", 3, 5, (4, 3))])
def test_tiled_sweep_spin_split(gpu, monkeypatch, split, bath, norb, nbath, sec, tile_rows):
    """The tiled sweep merges the H dw entries with the Hnd terms: the down species' numbers inside the merged lists."""
    TG.test_tiled_sweep_matches_oracle(gpu, monkeypatch, bath, norb, nbath, sec, 0.25, tile_rows)
    assert len(split) == 1


# --------------------------------------------------------------------------------------------
# e. two-phase entry points, emulated transposed exchange
# --------------------------------------------------------------------------------------------
def test_two_phase_spin_split(gpu, split):
    P.test_normal_two_phase_equals_fused(gpu)
    assert len(split) == 1


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("bath,norb,nbath,sec", [("normal", 2, 3, (4, 4)), ("hybrid", 3, 3, (3, 2))])
def test_transposed_exchange_spin_split(gpu, split, bath, norb, nbath, sec, world):
    P.test_transposed_exchange_emulated(gpu, bath, norb, nbath, sec, 0.25, world)
    assert len(split) == 1


# --------------------------------------------------------------------------------------------
# f. complex normal mode, phonons, ed_total_ud = F
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["doubled", "fourproducts"])
def test_cmplx_normal_spin_split(gpu, monkeypatch, split, form):
    P.test_cmplx_normal_matches_oracle(gpu, monkeypatch, "hybrid", 3, 3, (3, 3), form)
    assert len(split) == 1 and np.abs(np.asarray(split[0][1].hloc)[1, 1].imag).max() > 0.0


def test_phonon_branches_spin_split(gpu, split):
    P.test_phonon_branches_match_oracle(gpu, "hybrid", 3, 3, (3, 3), 2, (0.2, 0.1, 0.4), 0.0)
    assert len(split) == 1


@pytest.mark.parametrize("norb,nbath,nups,ndws", [(2, 2, (1, 2), (2, 1)), (3, 2, (1, 1, 2), (2, 1, 1))])
def test_orbs_apply_spin_split(gpu, norb, nbath, nups, ndws):
    """test_orbs_apply_matches_oracle with both species' diagonal impHloc kept (its _orbs_models keeps the up block only)."""
    from oracle import oracle as O
    from edipack_amd.hamiltonian import SectorHamiltonian
    om, pm = _split_models("normal", "normal", norb, nbath, seed=31, jxp=0.0)
    hl = np.zeros_like(om.hloc)
    for s in range(2):
        hl[s, s] = np.diag(np.diag(om.hloc[s, s].real))
    om.hloc = pm.hloc = hl
    assert not np.array_equal(hl[1, 1], hl[0, 0])
    ho = O.HOrbs(om, nups, ndws)
    hg = SectorHamiltonian.orbs_from_model(pm, nups, ndws)
    assert hg.dim == ho.dim
    v = np.random.default_rng(5).standard_normal(ho.dim)
    ref = ho.matvec(v)
    assert rel_err(hg.apply(v), ref) < TOL
    ha = SectorHamiltonian.orbs_from_arrays(ho.dims, ho.hd, ho.fac)
    assert rel_err(ha.apply(v), ref) < TOL
    hg.destroy()
    ha.destroy()


# --------------------------------------------------------------------------------------------
# g. nonsu2 with spin-dependent e, v: stored (device-built), on the fly, host-built
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["stored", "direct", "hostbuild"])
@pytest.mark.parametrize("bath,norb,nbath,sec", [("normal", 2, 2, 5), ("hybrid", 2, 3, 4), ("hybrid", 3, 2, 5)])
def test_flat_forms_spin_split(gpu, monkeypatch, form, bath, norb, nbath, sec):
    """test_flat_builder_and_apply_match_oracle in the three forms (the on-the-fly handle has no CSR to export: its
    product and recurrence are checked instead, as test_direct_matches_oracle_stored does)."""
    from oracle import oracle as O
    from edipack_amd.hamiltonian import SectorHamiltonian
    om, pm = _split_models("nonsu2", bath, norb, nbath, seed=11)
    ho = O.HFlat(om, sec)
    if form == "hostbuild":
        monkeypatch.setenv("EDIGPU_FLAT_HOSTBUILD", "1")
    hg = (SectorHamiltonian.direct_from_model if form == "direct" else SectorHamiltonian.flat_from_model)(pm, sec)
    assert hg.dim == ho.dim and hg.is_complex
    dense_ref = ho.dense()
    assert np.allclose(dense_ref, dense_ref.conj().T, atol=1e-14)
    if form != "direct":
        rp, col, val = hg.export_csr()
        assert np.allclose(csr_to_dense(rp, col, val, ho.dim), dense_ref, rtol=0, atol=1e-14)
    rng = np.random.default_rng(4)
    v = rng.standard_normal(ho.dim) + 1j * rng.standard_normal(ho.dim)
    assert rel_err(hg.apply(v), ho.matvec(v)) < TOL
    ao, bo, _ = ho.lanc_tridiag(v, 20)
    ag, bg, _ = hg.lanczos_tridiag(v, 20)
    assert rel_err(ag[:15], ao[:15]) < 1e-10 and rel_err(bg[:15], bo[:15]) < 1e-10
    hg.destroy()


def test_flat_device_built_midsize_spin_split(gpu, monkeypatch, split):
    P.test_flat_device_built_midsize(gpu, "nonsu2", "hybrid", 3, 5, 8, monkeypatch)
    assert len(split) == 1


def test_phonon_flat_direct_spin_split(gpu, monkeypatch, split):
    P.test_phonon_branches_flat_match_oracle(gpu, monkeypatch, "direct", "nonsu2", "hybrid", 3, 2, 5, 2, (0.2, 0.1, 0.4), 0.0)
    assert len(split) == 1


# --------------------------------------------------------------------------------------------
# h. seeds and observables on a polarised state
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bath,norb,nbath,sec,seed", [("hybrid", 3, 3, (3, 3), 43), ("normal", 2, 3, (4, 4), 43)])
def test_observables_of_a_polarised_ground_state(gpu, bath, norb, nbath, sec, seed):
    """<n_up>, <n_dw>, <n_up n_dw> per orbital from occ_moments of the GPU ground state against the dense ground state of
    the oracle's H (1e-9), on a state whose species differ by more than 1e-2 on some orbital; one c_up and one c_dw seed
    from that state against the host restatement (tests/gf_normal.py, 1e-12)."""
    import torch
    from oracle import oracle as O
    from edipack_amd.hamiltonian import SectorHamiltonian
    from tests.gf_normal import apply_c_dw, apply_c_up
    om, pm = _split_models("normal", bath, norb, nbath, seed=seed)
    ho = O.HNormal(om, *sec)
    w, vecs = np.linalg.eigh(ho.dense())
    assert w[1] - w[0] > 1e-3                                     # a ground state of its own: the vector is defined
    p = vecs[:, 0] ** 2
    iup, idw = np.arange(ho.dim) % ho.dimup, np.arange(ho.dim) // ho.dimup
    nu = np.array([(ho.mapup[iup] >> a) & 1 for a in range(norb)], dtype=float)
    nd = np.array([(ho.mapdw[idw] >> a) & 1 for a in range(norb)], dtype=float)
    n_up, n_dw, docc = nu @ p, nd @ p, (nu * nd) @ p
    assert np.max(np.abs(n_up - n_dw)) > 1e-2                     # polarised: the species can be told apart
    hg = SectorHamiltonian.normal_from_model(pm, *sec)
    e, x, _ = hg.lanczos_eigh(nitermax=min(400, ho.dim), tol=1e-14, v0=np.random.default_rng(3).standard_normal(ho.dim))
    assert abs(e - w[0]) < 1e-9 * max(1.0, abs(w[0]))
    xd = torch.from_numpy(x).cuda()
    m, nrm = hg.occ_moments(xd.data_ptr())
    m = m[0] / nrm[0]
    d = np.diag(m)
    print(f"occupation errors: up {np.max(np.abs(d[:norb] - n_up)):.2e} dw {np.max(np.abs(d[norb:2 * norb] - n_dw)):.2e}")
    assert np.max(np.abs(d[:norb] - n_up)) < 1e-9 and np.max(np.abs(d[norb:2 * norb] - n_dw)) < 1e-9
    assert np.max(np.abs(np.array([m[a, norb + a] for a in range(norb)]) - docc)) < 1e-9
    for ispin, restate in ((0, apply_c_up), (1, apply_c_dw)):
        sec2 = (sec[0] - 1, sec[1]) if ispin == 0 else (sec[0], sec[1] - 1)
        ho2 = O.HNormal(om, *sec2)
        h2 = SectorHamiltonian.normal_from_model(pm, *sec2)
        out = torch.full((h2.dim,), 7.0, dtype=torch.float64, device="cuda")
        hg.apply_cops_to(h2, xd.data_ptr(), out.data_ptr(), (1.0,), [False], (norb - 1,), [ispin])
        ref = restate(ho, ho2, x, norb - 1, False)
        assert ref @ ref > 1e-3 and np.max(np.abs(out.cpu().numpy() - ref)) < 1e-12
        h2.destroy()
    hg.destroy()


# --------------------------------------------------------------------------------------------
# the reference's antiferromagnet fixture (test/src/INEQ_NORMAL_NORMAL; tests/test_oracle_golden.py has the CPU twin)
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site", [0, 1])
def test_golden_afm_fixture_from_gpu_eigenvectors(gpu, site):
    """dens, docc, energy, doubles (absolute 1e-9, ASSERTING.f90:74-80) from the GPU eigenvector of the GPU-built (4, 4)
    sector (4900 states) -- its four neighbours are diagonalised as well and lie above it -- and Sigma_momenta (1e-10
    relative, as test_golden_sigma_momenta_through_gpu_tridiag) with every tridiagonalisation on the GPU."""
    from oracle import oracle as O
    from edipack_amd.hamiltonian import SectorHamiltonian
    from tests import observables as ob
    from tests.gf_normal import sigma_momenta_normal
    from tests.test_oracle_golden import GOLD
    g = GOLD["INEQ_NORMAL_NORMAL"]
    om, pm = afm_site_models(g["input"], site)
    assert not np.array_equal(pm.be[1], pm.be[0])
    found = {}
    for sec in ((4, 4), (3, 4), (5, 4), (4, 3), (4, 5)):      # no twin shortcut: (3, 4) and (4, 3) differ here
        hg = SectorHamiltonian.normal_from_model(pm, *sec)
        found[sec] = hg.lanczos_eigh_multi(2, tol=1e-13)[:2]
        hg.destroy()
    w, v = found[(4, 4)]
    assert w[1] - w[0] > 1e-6 and all(found[s][0][0] - w[0] > 1e-6 for s in found if s != (4, 4))
    assert abs(found[(3, 4)][0][0] - found[(4, 3)][0][0]) > 1e-3
    e0, h = w[0], O.HNormal(om, 4, 4)
    states = [((4, 4), h, v[0])]
    dens, docc = ob.dens_docc(om, states)
    up, dw = ob._densities(om, states)
    assert abs(up[0] - dw[0]) > 0.1                             # magnetised
    doubles, energy, _ = ob.doubles_energy_imp(om, states, e0)
    print(f"afm site {site}: dens {abs(dens[0] - g['dens'][site]):.2e} docc {abs(docc[0] - g['docc'][site]):.2e} "
          f"energy {np.max(np.abs(energy - np.array(g['energy']).reshape(2, 4)[site])):.2e}")
    assert abs(dens[0] - g["dens"][site]) < 1e-9 and abs(docc[0] - g["docc"][site]) < 1e-9
    assert np.max(np.abs(energy - np.array(g["energy"]).reshape(2, 4)[site])) < 1e-9
    assert np.max(np.abs(doubles - np.array(g["doubles"]).reshape(2, 4)[site])) < 1e-9

    def tridiag(s, vec, nl):
        hs = SectorHamiltonian.normal_from_model(pm, *s)
        a, b, _ = hs.lanczos_tridiag(vec, nl)
        hs.destroy()
        return a, b

    m = sigma_momenta_normal(om, tridiag, beta=g["input"]["BETA"], ngfiter=int(g["input"]["LANC_NGFITER"]),
                             states=[((4, 4), h, e0, v[0])])
    gold = np.array(g["Sigma_momenta"]).reshape(2, 4)[site]
    print(f"afm site {site}: Sigma_momenta rel err {np.max(np.abs(m[0] - gold) / np.abs(gold)):.2e}")
    assert np.max(np.abs(m[0] - gold) / np.abs(gold)) < 1e-10
