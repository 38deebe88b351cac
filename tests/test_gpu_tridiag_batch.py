"""Several vectors per sweep over H on superc / nonsu2 sectors: edigpu_apply_multi_dev against single products and
edigpu_lanczos_tridiag_batch_dev against single edigpu_lanczos_tridiag_dev calls, whose results define it.

Cases (rows): S superc hybrid 2+3 sector 0 (252: one workgroup, the last SELL slice holds 60 rows), N the same shape
in nonsu2 (sector 5), L nonsu2 normal 1+6 sector 7 (3432: 54 slices = 14 workgroups of 4, the last half empty, last
slice 40 rows, more than one workgroup of the on-the-fly kernel); each stored and on the fly.

Bounds: a product column against the single product 1e-13 (existing tests hold two routes of one product to 1e-14, the
oracle to 1e-12); the recurrence as test_lanczos_tridiag_matches_oracle: first 15 coefficients and the continued
fraction away from the spectrum 1e-10, norm2 1e-12, step counts equal."""
import numpy as np
import pytest

from tests.common import make_models, rel_err

pytestmark = pytest.mark.gpu

CASES = {
    "S": ("superc", "hybrid", 2, 3, 0, 252),
    "N": ("nonsu2", "hybrid", 2, 3, 5, 252),
    "L": ("nonsu2", "normal", 1, 6, 7, 3432),
}
NLANC = 60
ZS = (40.0 + 0.1j, -40.0 + 0.1j, 25.0j)


def _cf(alpha, beta, z):
    """continued fraction <v|(z-H)^-1|v> from the tridiagonal (what the GF builder consumes)."""
    g = 0.0
    for k in range(len(alpha) - 1, -1, -1):
        b2 = beta[k + 1] ** 2 if k + 1 < len(alpha) else 0.0
        g = 1.0 / (z - alpha[k] - b2 * g)
    return g


@pytest.fixture(scope="module")
def sectors(gpu):
    """(oracle sector, {form: handle}) per case, built once"""
    from oracle import oracle as O
    from edipack_amd.hamiltonian import SectorHamiltonian
    made = {}

    def get(case):
        if case not in made:
            mode, bath, norb, nbath, sec, rows = CASES[case]
            om, pm = make_models(mode, bath, norb, nbath, seed=31)
            ho = O.HFlat(om, sec)
            assert ho.dim == rows
            made[case] = (ho, {"stored": SectorHamiltonian.flat_from_model(pm, sec),
                               "direct": SectorHamiltonian.direct_from_model(pm, sec)}, om, pm)
        return made[case]

    yield get
    for _, hs, _, _ in made.values():
        for h in hs.values():
            h.destroy()


def _random(n, dim, seed, cplx=True):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, dim))
    return v + 1j * rng.standard_normal((n, dim)) if cplx else v


def _singles(h, seeds_dev, nlanc, thr=1e-12):
    out = [h.lanczos_tridiag_dev(seeds_dev[j].data_ptr(), nlanc, thr) for j in range(seeds_dev.shape[0])]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out]))


def _check_recurrence(got, ref, rows=None):
    """the checks of test_lanczos_tridiag_matches_oracle, per seed"""
    a, b, nd, n2 = got[:4]
    a_ref, b_ref, nd_ref, n2_ref = ref
    for j in (range(a.shape[0]) if rows is None else rows):
        print(f"seed {j}: niter {nd[j]} / {nd_ref[j]}  norm2 rel {abs(n2[j] - n2_ref[j]) / n2_ref[j]:.2e}  "
              f"a[:15] {rel_err(a[j, :15], a_ref[j, :15]):.2e}  b[:15] {rel_err(b[j, :15], b_ref[j, :15]):.2e}  cf "
              + " ".join(f"{abs(_cf(a[j], b[j], z) - _cf(a_ref[j], b_ref[j], z)) / abs(_cf(a_ref[j], b_ref[j], z)):.2e}" for z in ZS))
        assert nd[j] == nd_ref[j]
        assert abs(n2[j] - n2_ref[j]) <= 1e-12 * n2_ref[j]
        assert rel_err(a[j, :15], a_ref[j, :15]) < 1e-10 and rel_err(b[j, :15], b_ref[j, :15]) < 1e-10
        for z in ZS:
            g_ref, g = _cf(a_ref[j], b_ref[j], z), _cf(a[j], b[j], z)
            assert abs(g - g_ref) / abs(g_ref) < 1e-10
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(np.isfinite(n2))


# --------------------------------------------------------------------------------------------
# 1. product
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["stored", "direct"])
@pytest.mark.parametrize("case", ["S", "N", "L"])
def test_apply_multi_matches_single_products(sectors, case, form):
    import torch
    ho, hs, _, _ = sectors(case)
    h = hs[form]
    st = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(_random(9, ho.dim, 5)).cuda()
    ref = torch.zeros_like(x)
    for j in range(9):
        h.apply_dev(x[j].data_ptr(), ref[j].data_ptr(), st)
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    for nvec in (1, 2, 3, 4, 5, 8, 9):
        y = torch.full_like(x, 7.0)
        h.apply_multi_dev(x.data_ptr(), y.data_ptr(), nvec, st)
        torch.cuda.synchronize()
        y = y.cpu().numpy()
        errs = [rel_err(y[j], ref[j]) for j in range(nvec)]
        print(case, form, nvec, "max rel err", max(errs))
        assert max(errs) < 1e-13
        assert np.all(y[nvec:] == 7.0)  # nothing past the last vector is written
    if case == "S":
        xh = x.cpu().numpy()
        assert max(rel_err(y[j], ho.matvec(xh[j])) for j in range(9)) < 1e-12


# --------------------------------------------------------------------------------------------
# 2. recurrence
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["stored", "direct"])
@pytest.mark.parametrize("case", ["S", "N", "L"])
def test_batch_recurrence_matches_single_calls(sectors, case, form):
    import torch
    ho, hs, _, _ = sectors(case)
    h = hs[form]
    seeds = _random(11, ho.dim, 12345)
    sd = torch.from_numpy(seeds).cuda()
    ref = _singles(h, sd, NLANC)
    for nseed, want in ((2, 2), (3, 4), (5, 8), (8, 8), (11, 8)):
        got = h.lanczos_tridiag_batch_dev(sd.data_ptr(), nseed, NLANC)
        print(case, form, "nseed", nseed, "route", got[4])
        assert got[4] == want
        assert got[0].shape == got[1].shape == (nseed, NLANC)
        _check_recurrence(got, tuple(r[:nseed] for r in ref))
    if case == "S":
        ora = [ho.lanc_tridiag(seeds[j], NLANC) for j in range(3)]
        got = h.lanczos_tridiag_batch_dev(sd.data_ptr(), 3, NLANC)
        n2 = np.array([np.vdot(seeds[j], seeds[j]).real for j in range(3)])
        _check_recurrence(got, (np.array([o[0] for o in ora]), np.array([o[1] for o in ora]),
                                np.array([o[2] for o in ora]), n2))


# --------------------------------------------------------------------------------------------
# 3. stops: an eigenvector and a zero seed between two random ones
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["stored", "direct"])
def test_batch_stops_per_seed(sectors, form):
    import torch
    ho, hs, _, _ = sectors("S")
    h = hs[form]
    ev, vec, nconv, _ = h.lanczos_eigh_multi(1, tol=1e-12)
    assert nconv == 1
    rnd = _random(2, ho.dim, 77)
    seeds = np.stack([rnd[0], vec[0], np.zeros(ho.dim, complex), rnd[1]])
    sd = torch.from_numpy(seeds).cuda()
    thr = 1e-8
    ref = _singles(h, sd, NLANC, thr)
    a, b, nd, n2, route = h.lanczos_tridiag_batch_dev(sd.data_ptr(), 4, NLANC, thr)
    assert route == 4
    for arr in (a, b, n2):
        assert np.all(np.isfinite(arr))
    # the eigenvector: one step, alpha = the eigenvalue, nothing after; the zero seed: no step at all
    print("eigenvector seed: niter", nd[1], "alpha - E0", a[1, 0] - ev[0], "norm2", n2[1], "| zero seed: niter", nd[2])
    assert nd[1] == ref[2][1] == 1 and nd[2] == ref[2][2] == 0
    assert abs(a[1, 0] - ev[0]) < 1e-10 * max(1.0, abs(ev[0])) and abs(a[1, 0] - ref[0][1, 0]) < 1e-10 * max(1.0, abs(ev[0]))
    assert not a[1, 1:].any() and not b[1].any() and not ref[0][1, 1:].any() and not ref[1][1].any()
    assert abs(n2[1] - ref[3][1]) <= 1e-12 * ref[3][1]
    assert not a[2].any() and not b[2].any() and n2[2] == 0.0 == ref[3][2]
    assert np.array_equal(a[2], ref[0][2]) and np.array_equal(b[2], ref[1][2])
    # the random seeds beside them are not disturbed
    _check_recurrence((a, b, nd, n2), ref, rows=(0, 3))


# --------------------------------------------------------------------------------------------
# 4. route 0: normal mode and a phonon flat sector return the single calls' results unchanged
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["normal", "phonon"])
def test_route_zero_is_the_single_path(gpu, which):
    import torch
    from edipack_amd.hamiltonian import SectorHamiltonian
    from tests.ph_cases import set_phonons
    if which == "normal":
        _, pm = make_models("normal", "normal", 2, 3, seed=31)
        h = SectorHamiltonian.normal_from_model(pm, 4, 4)
        seeds = _random(3, h.nloc, 8, cplx=False)
    else:
        _, pm = make_models("superc", "normal", 2, 2, seed=31)
        h = SectorHamiltonian.flat_from_model(set_phonons(pm, 2), 0)
        seeds = _random(3, h.nloc, 8)
    sd = torch.from_numpy(seeds).cuda()
    ref = _singles(h, sd, 30)
    a, b, nd, n2, route = h.lanczos_tridiag_batch_dev(sd.data_ptr(), 3, 30)
    assert route == 0
    assert np.array_equal(a, ref[0]) and np.array_equal(b, ref[1]) and np.array_equal(nd, ref[2]) and np.array_equal(n2, ref[3])
    # and the product runs nvec plain products
    st = torch.cuda.current_stream().cuda_stream
    y, y1 = torch.zeros_like(sd), torch.zeros_like(sd)
    h.apply_multi_dev(sd.data_ptr(), y.data_ptr(), 3, st)
    for j in range(3):
        h.apply_dev(sd[j].data_ptr(), y1[j].data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(y, y1)
    h.destroy()


# --------------------------------------------------------------------------------------------
# 5. refusals
# --------------------------------------------------------------------------------------------
def test_row_shard_gets_the_single_calls_message(gpu):
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian
    mode, bath, norb, nbath, sec, rows = CASES["L"]
    _, pm = make_models(mode, bath, norb, nbath, seed=31)
    h = SectorHamiltonian.flat_from_model(pm, sec, row_first=0, row_count=rows // 2)
    sd = torch.from_numpy(_random(2, rows, 3)).cuda()
    with pytest.raises(capi.EdigpuError):
        h.lanczos_tridiag_dev(sd.data_ptr(), 10)
    single = capi.last_error()
    with pytest.raises(capi.EdigpuError):
        h.lanczos_tridiag_batch_dev(sd.data_ptr(), 2, 10)
    assert "handle is a shard" in single and capi.last_error() == single
    h.destroy()


# --------------------------------------------------------------------------------------------
# 6. real SELL images of hand-over matrices (edigpu_csr_create_d), plain and with the value dictionary
# --------------------------------------------------------------------------------------------
def _banded(n, offsets, values):
    """real symmetric band matrix as CSR, every row of (nearly) the same length: the SELL image takes it"""
    dense = np.zeros((n, n))
    rng = np.random.default_rng(4)
    for o in offsets:
        for i in range(n - o):
            v = rng.standard_normal() if values is None else values[(i + o) % len(values)]
            dense[i, i + o] = dense[i + o, i] = v
    rowptr, col, val = [0], [], []
    for i in range(n):
        nz = np.nonzero(dense[i])[0]
        col += list(nz)
        val += list(dense[i, nz])
        rowptr.append(len(col))
    return np.array(rowptr, np.int64), np.array(col, np.int32), np.array(val), dense


@pytest.mark.parametrize("image", ["sell", "sell_dictionary", "csr"])
def test_real_handover_matrix(gpu, image):
    import torch
    from edipack_amd.hamiltonian import SectorHamiltonian
    n = 301
    if image == "csr":
        # one full row and column among rows of three entries: too ragged for the SELL image (padding > 1.6)
        rowptr, col, val, dense = _banded(n, (0, 1), None)
        dense[0, :] = dense[:, 0] = 0.1
        rowptr, col, val = [0], [], []
        for i in range(n):
            nz = np.nonzero(dense[i])[0]
            col += list(nz)
            val += list(dense[i, nz])
            rowptr.append(len(col))
        rowptr, col, val = np.array(rowptr, np.int64), np.array(col, np.int32), np.array(val)
    else:
        rowptr, col, val, dense = _banded(n, (0, 1, 7, 40), None if image == "sell" else (0.5, -1.25, 2.0))
    h = SectorHamiltonian.csr_from_arrays(rowptr, col, val)
    seeds = _random(11, n, 21, cplx=False)
    sd = torch.from_numpy(seeds).cuda()
    ref = _singles(h, sd, NLANC)
    # test 2 with real seeds: every width of the real instantiations (two columns per 16-byte chunk at every width)
    for nseed, want in ((2, 2), (3, 4), (5, 8), (8, 8), (11, 8)):
        got = h.lanczos_tridiag_batch_dev(sd.data_ptr(), nseed, NLANC)
        print(image, "nseed", nseed, "route", got[4])
        assert got[4] == (0 if image == "csr" else want)
        _check_recurrence(got, tuple(r[:nseed] for r in ref))
    # the product: every width against single products, and against the dense matrix
    st = torch.cuda.current_stream().cuda_stream
    one = torch.zeros_like(sd)
    for j in range(11):
        h.apply_dev(sd[j].data_ptr(), one[j].data_ptr(), st)
    torch.cuda.synchronize()
    one = one.cpu().numpy()
    assert rel_err(one, seeds @ dense.T) < 1e-12
    for nvec in (1, 2, 3, 4, 5, 8, 9):
        y = torch.full_like(sd, 7.0)
        h.apply_multi_dev(sd.data_ptr(), y.data_ptr(), nvec, st)
        torch.cuda.synchronize()
        y = y.cpu().numpy()
        err = max(rel_err(y[j], one[j]) for j in range(nvec))
        print(image, "nvec", nvec, "max rel err against single products", err)
        assert err < 1e-13 and np.all(y[nvec:] == 7.0)
    if image != "csr":
        # pairs of seeds, the only width a matrix of more than 200 000 rows takes by default: 11 seeds = 5 pairs + 1 single
        h.batch_set_width(2)
        got = h.lanczos_tridiag_batch_dev(sd.data_ptr(), 11, NLANC)
        assert got[4] == 2
        _check_recurrence(got, ref)
        y = torch.full_like(sd, 7.0)
        h.apply_multi_dev(sd.data_ptr(), y.data_ptr(), 5, st)
        torch.cuda.synchronize()
        y = y.cpu().numpy()
        assert max(rel_err(y[j], one[j]) for j in range(5)) < 1e-13 and np.all(y[5:] == 7.0)
        h.batch_set_width(0)
        assert h.lanczos_tridiag_batch_dev(sd.data_ptr(), 11, NLANC)[4] == 8
    h.destroy()


# --------------------------------------------------------------------------------------------
# 7. end to end: the Sz+1 half of a superc G(i omega), all seeds of the target sector in one call
# --------------------------------------------------------------------------------------------
def test_superc_gf_all_seeds_of_a_sector_in_one_batch(gpu):
    import torch
    from oracle import oracle as O
    from edipack_amd.hamiltonian import SectorHamiltonian
    from tests import gf_flat
    # (2 + 4 levels: the target sector Sz = 0 of 924 rows is regular enough for the SELL image, so it takes the batch)
    om, pm = make_models("superc", "hybrid", 2, 4, seed=31)
    _, states = gf_flat._ground_states(om, 1e-9)
    sec, h_gs, e_gs, vec = states[0]
    h2o = O.HFlat(om, sec + 1)
    up, dw = 0, 1
    # channels of lanc_build_gf_superc_Gdiag / _Fmix that land in Sz+1: c^+_up, c_dw, c^+_up + c_dw, c^+_up + i c_dw
    chans = []
    for a in range(om.norb):
        chans += [[(1.0, True, a, up)], [(1.0, False, a, dw)], [(1.0, True, a, up), (1.0, False, a, dw)],
                  [(1.0, True, a, up), (1j, False, a, dw)]]
    seeds = np.stack([gf_flat.apply_cops(h_gs, h2o, vec, ops, om.ns) for ops in chans])
    h2 = SectorHamiltonian.flat_from_model(pm, sec + 1)
    sd = torch.from_numpy(seeds).cuda()
    nl = min(h2o.dim, NLANC)
    z = 1j * np.pi / 50.0 * (2.0 * np.arange(1, 65) - 1.0)

    def green(a, b, n2):
        g = np.zeros((len(chans), z.shape[0]), complex)
        for j in range(len(chans)):
            t = np.diag(a[j]) + np.diag(b[j, 1:], 1) + np.diag(b[j, 1:], -1)
            w, zz = np.linalg.eigh(t)
            g[j] = np.sum((n2[j] * zz[0, :] ** 2)[None, :] / (z[:, None] - (w - e_gs)[None, :]), axis=1)
        return g

    ref = _singles(h2, sd, nl)
    a, b, nd, n2, route = h2.lanczos_tridiag_batch_dev(sd.data_ptr(), len(chans), nl)
    assert route == 8 and np.array_equal(nd, ref[2])
    g_one, g_all = green(ref[0], ref[1], ref[3]), green(a, b, n2)
    live = ref[3] > 0.0  # (a channel that annihilates the ground state has no seed: both give zeros)
    assert live.sum() >= 2 * om.norb and np.array_equal(n2 > 0.0, live) and not g_all[~live].any()
    diff = np.max(np.abs(g_all[live] - g_one[live]) / np.abs(g_one[live]))
    print("G(i omega): max rel difference batch / one by one", diff)
    assert diff < 1e-10
    h2.destroy()
