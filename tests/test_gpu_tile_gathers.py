"""The tiled column sweep (kernels_panel.hip: normal_dw_tile_kernel) gathers the LIVE entries of a row's outside list
only -- full batches of four, then one straight-line path per live count of the last batch -- and reads an Hnd partner
row that lies inside the chunk from the staged tile instead of from global memory.  Every live entry enters the same
sum in the same order as before, so nothing is to be seen but against the oracle: the product of the panel-major loop
(BLK), twelve fused Lanczos steps (ALPHA) and the boundary product on the natural layout (EDGE where DimUp is odd), on
small sectors forced onto the tiled sweep as in test_gpu_tile_balance.py.

The planner's own cuts do not separate an Hnd pair in these small sectors (tests/test_tile_gathers.py counts them), so
the partner row outside the chunk -- the path that keeps the global read -- is met where a shard boundary separates a
pair: test_shard_boundary_separates_a_pair."""
import itertools

import numpy as np
import pytest

from tests.common import make_models, rel_err
from tests.test_gpu_tile_balance import _skip_if_switched

TOL = 1e-12  # test_gpu_parity.TOL (test_normal_apply_matches_oracle)

CASES = [
    # bath, norb, nbath, (nup, ndw), jxp, EDIGPU_TILE_ROWS
    ("normal", 2, 3, (4, 4), 0.25, 8),       # DimUp = DimDw = 70: one panel, 11 chunks
    ("normal", 2, 3, (4, 4), 0.25, None),    # the same in 3 chunks
    ("normal", 2, 5, (6, 3), 0.25, 8),       # DimUp = 924 = 8 panels: Hnd partner columns in neighbouring panels; DimDw = 220
    ("hybrid", 3, 10, (5, 2), 0.25, 8),      # DimUp = 1287 (odd: EDGE), 11 panels: several merged terms
    ("normal", 2, 3, (4, 4), 0.0, 8),        # no Hnd terms (DO_ND = false)
]


def _force_tiled(monkeypatch, tile_rows):
    monkeypatch.setenv("EDIGPU_IB", "0")  # the generic panel-major loop, forced on a small sector (test_gpu_ell16)
    monkeypatch.setenv("EDIGPU_BLOCKED", "1")
    monkeypatch.setenv("EDIGPU_BLOCKED_MIN", "0")
    monkeypatch.setenv("EDIGPU_BLOCKED_W", "128")
    monkeypatch.setenv("EDIGPU_PANEL_VEC2_MIN", "0")
    if tile_rows:
        monkeypatch.setenv("EDIGPU_TILE_ROWS", str(tile_rows))
    else:
        monkeypatch.delenv("EDIGPU_TILE_ROWS", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("bath,norb,nbath,sec,jxp,tile_rows", CASES)
def test_tiled_sweep_matches_oracle(gpu, monkeypatch, bath, norb, nbath, sec, jxp, tile_rows):
    _skip_if_switched()
    from oracle import oracle as O
    from edipack_amd.hamiltonian import SectorHamiltonian
    om, pm = make_models("normal", bath, norb, nbath, seed=83, jxp=jxp)
    ho = O.HNormal(om, *sec)
    _force_tiled(monkeypatch, tile_rows)
    h = SectorHamiltonian.normal_from_model(pm, *sec)
    assert h.image_info()[4] == 128  # panel-major, 128-column panels: the tiled sweep
    assert (h.image_info()[1] > 0) == (jxp != 0.0)
    rng = np.random.default_rng(97)
    for _ in range(2):
        v = rng.standard_normal(ho.dim)
        ref = ho.matvec(v)
        e_loop, e_nat = rel_err(h.apply_loop(v), ref), rel_err(h.apply(v), ref)
        print(f"H*v rel err: panel-major loop {e_loop:.2e}, natural layout {e_nat:.2e}")
        assert e_loop < TOL
        assert e_nat < TOL  # the boundary product: natural layout
    v = rng.standard_normal(ho.dim)
    n = 12
    ao, bo, _ = ho.lanc_tridiag(v, n)
    a, b, nd = h.lanczos_tridiag(v, n)
    print(f"lanczos rel err: alpha {rel_err(a, ao):.2e}, beta {rel_err(b, bo):.2e}")
    assert nd == n
    assert rel_err(a, ao) < 1e-10 and rel_err(b, bo) < 1e-10  # as test_lanczos_tridiag_matches_oracle
    h.destroy()


@pytest.mark.gpu
def test_shard_boundary_separates_a_pair(gpu, monkeypatch):
    """Two down-row shards of the (4, 4) sector cut between the two rows of an Hnd pair (down words that differ in
    the two impurity bits only, adjacent in the sorted basis): the partner row of either lies outside every chunk of
    its shard, all other pairs inside."""
    _skip_if_switched()
    import torch
    from oracle import oracle as O
    from edipack_amd.hamiltonian import SectorHamiltonian
    om, pm = make_models("normal", "normal", 2, 3, seed=83, jxp=0.25)
    sec = (4, 4)
    ho = O.HNormal(om, *sec)
    words = sorted(sum(1 << b for b in c) for c in itertools.combinations(range(om.ns), sec[1]))
    assert len(words) == ho.dimdw
    cuts = [k for k in range(1, len(words)) if words[k - 1] & 3 == 1 and words[k] & 3 == 2 and words[k - 1] >> 2 == words[k] >> 2]
    cut = cuts[len(cuts) // 2]
    _force_tiled(monkeypatch, 8)
    monkeypatch.setenv("EDIGPU_BLOCKED", "0")  # shards keep the natural layout
    v = np.random.default_rng(101).standard_normal(ho.dim)
    ref = ho.matvec(v)
    vd = torch.from_numpy(v).cuda()
    out = []
    for first, cnt in ((0, cut), (cut, ho.dimdw - cut)):
        hs = SectorHamiltonian.normal_from_model(pm, *sec, dw_first=first, dw_count=cnt)
        assert hs.image_info()[1] > 0 and hs.image_info()[3] == 2  # Hnd terms, the tiled variant of the panel sweep
        hv = torch.empty(hs.nloc, dtype=torch.float64, device="cuda")
        hs.apply_dev(vd.data_ptr(), hv.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out.append(hv.cpu().numpy())
        hs.destroy()
    err = rel_err(np.concatenate(out), ref)
    print(f"sharded H*v rel err {err:.2e} (cut at down row {cut})")
    assert err < TOL
