"""The ED_TWIN=T reorder on the device (csrc/edigpu_twin.hip, kernels_twin.hip: edigpu_apply_twin): a twin sector's
vectors from the stored sector's, v_B[i] = v_A[order_A(i)] phonon block by phonon block (es_return_dvector,
ED_EIGENSPACE.f90:652-720).

A pure permutation: every result is compared BIT FOR BIT (np.array_equal on the float64 words) with numpy -- normal mode
with v.reshape(nblk, DimDw, DimUp).transpose(0, 2, 1), superc / nonsu2 with v[order] from the restatement of
twin_sector_order in tests/test_twin_host.py.  Shapes DimDw x DimUp of the normal-mode cases: 1 x 6 and 6 x 1 (a species
empty), 4 x 6, 6 x 6 (self-twin, one handle), 70 x 8 and 8 x 70, 126 x 84, 462 x 330 and 924 x 792 (several 64-tiles both
ways, none a multiple of the tile; odd and even row lengths, so both the 16-byte and the 8-byte accesses run).  Every case
raises AttributeError / EdigpuError without the feature."""
import numpy as np
import pytest

from tests.common import make_models
from tests.test_twin_host import NONSU2, SUPERC, twin_order_ref

pytestmark = pytest.mark.gpu

PAD = 7.0      # what a destination holds before a call: every element must be written


def _H():
    from edipack_amd.hamiltonian import SectorHamiltonian
    return SectorHamiltonian


def _words(a):
    return np.ascontiguousarray(a).view(np.float64)


def _twin_call(src, dst, v, nvec=1, off_src=0, off_dst=0):
    """nvec vectors of src (v[nvec, dim]) -> dst on fresh device buffers, the vectors off_src / off_dst DOUBLES past a
    16-byte boundary; checks that the source and the padding around the destination are untouched"""
    import torch
    w = 2 if src.is_complex else 1
    flat = _words(v).reshape(-1)
    assert flat.size == nvec * src.dim * w
    sbuf = torch.zeros(flat.size + 2, dtype=torch.float64, device="cuda")
    dbuf = torch.full((nvec * dst.dim * w + 4,), PAD, dtype=torch.float64, device="cuda")
    sbuf[off_src:off_src + flat.size] = torch.from_numpy(flat).cuda()
    st = torch.cuda.current_stream().cuda_stream
    src.twin_to(dst, sbuf.data_ptr() + 8 * off_src, dbuf.data_ptr() + 8 * (1 + off_dst), nvec, st)
    torch.cuda.synchronize()
    out = dbuf.cpu().numpy()
    n = nvec * dst.dim * w
    assert np.all(out[:1 + off_dst] == PAD) and np.all(out[1 + off_dst + n:] == PAD)
    assert np.array_equal(sbuf.cpu().numpy()[off_src:off_src + flat.size], flat)
    got = out[1 + off_dst:1 + off_dst + n]
    return (got.view(np.complex128) if src.is_complex else got).reshape(nvec, dst.dim)


def _vectors(h, nvec, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((nvec, h.dim))
    return v + 1j * rng.standard_normal((nvec, h.dim)) if h.is_complex else v


def _transpose_ref(v, nvec, nblk, dim_dw, dim_up):
    return np.ascontiguousarray(v.reshape(nvec, nblk, dim_dw, dim_up).transpose(0, 1, 3, 2)).reshape(nvec, -1)


def _check_transpose_pair(a, b, nblk, seed, variants=True):
    """a -> b (b may be a): nvec 1 and 3; source and destination one double off the 16-byte boundary"""
    assert (b.dim_up, b.dim_dw) == (a.dim_dw, a.dim_up) and a.dim == nblk * a.dim_up * a.dim_dw
    runs = [(1, 0, 0), (3, 0, 0), (1, 1, 1), (1, 1, 0), (3, 0, 1)] if variants else [(1, 0, 0)]
    for nvec, o1, o2 in runs:
        v = _vectors(a, nvec, seed + nvec)
        got = _twin_call(a, b, v, nvec, o1, o2)
        assert np.array_equal(_words(got), _words(_transpose_ref(v, nvec, nblk, a.dim_dw, a.dim_up))), (nvec, o1, o2)


def _phonons(pm, norb):
    pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = 2, 0.8, 0.15, np.diag([0.4, -0.3, 0.2][:norb])


# (bath, norb, nbath) -> Ns; (Nup, Ndw) of the source; the shape DimDw x DimUp it is named for
NORMAL_SHAPES = {
    "1x6": (("normal", 2, 1), (2, 0), (1, 6)),
    "6x1": (("normal", 2, 1), (0, 2), (6, 1)),
    "4x6": (("normal", 2, 1), (2, 1), (4, 6)),
    "6x6_self": (("normal", 2, 1), (2, 2), (6, 6)),
    "70x8": (("normal", 2, 3), (1, 4), (70, 8)),
    "8x70": (("normal", 2, 3), (4, 1), (8, 70)),
    "126x84": (("normal", 3, 2), (3, 4), (126, 84)),
    "462x330": (("hybrid", 2, 9), (4, 5), (462, 330)),
    "924x792": (("normal", 2, 5), (5, 6), (924, 792)),
}


@pytest.mark.parametrize("shape", sorted(NORMAL_SHAPES))
def test_normal_mode_is_the_transpose(gpu, shape):
    (bath, norb, nbath), (nup, ndw), (ddw, dup) = NORMAL_SHAPES[shape]
    _, pm = make_models("normal", bath, norb, nbath, seed=5)
    H = _H()
    a = H.normal_from_model(pm, nup, ndw)
    b = a if nup == ndw else H.normal_from_model(pm, ndw, nup)
    assert (a.dim_dw, a.dim_up) == (ddw, dup)
    _check_transpose_pair(a, b, 1, seed=40)
    if b is not a:
        b.destroy()
    a.destroy()


@pytest.mark.parametrize("shape", ["4x6", "6x6_self", "126x84"])
def test_normal_mode_phonon_blocks(gpu, shape):
    """nph = 2: three blocks per vector, each transposed on its own"""
    (bath, norb, nbath), (nup, ndw), (ddw, dup) = NORMAL_SHAPES[shape]
    _, pm = make_models("normal", bath, norb, nbath, seed=5)
    _phonons(pm, norb)
    H = _H()
    a = H.normal_from_model(pm, nup, ndw)
    b = a if nup == ndw else H.normal_from_model(pm, ndw, nup)
    assert a.dim == 3 * ddw * dup
    _check_transpose_pair(a, b, 3, seed=50)
    if b is not a:
        b.destroy()
    a.destroy()


@pytest.mark.parametrize("shape", ["4x6", "6x6_self", "70x8", "8x70", "126x84"])
def test_normal_mode_complex(gpu, shape):
    """_CMPLX_NORMAL: double2 elements, tiles of 32; one double off the boundary = the two-doubles path"""
    from tests.test_gpu_axisop import _complexify
    (bath, norb, nbath), (nup, ndw), (ddw, dup) = NORMAL_SHAPES[shape]
    om, pm = make_models("normal", bath, norb, nbath, seed=5)
    _complexify(om, pm, 32)
    H = _H()
    a = H.normal_cmplx_from_model(pm, nup, ndw)
    b = a if nup == ndw else H.normal_cmplx_from_model(pm, ndw, nup)
    assert a.is_complex and (a.dim_dw, a.dim_up) == (ddw, dup)
    _check_transpose_pair(a, b, 1, seed=60)
    if b is not a:
        b.destroy()
    a.destroy()


def test_normal_mode_hand_over_handles(gpu):
    """edigpu_normal_create: no model, no map -- the dimensions are the check"""
    from edipack_amd import capi
    from oracle import oracle as O
    om, _ = make_models("normal", "normal", 2, 1, seed=5)
    H = _H()
    hs = {}
    for sec in ((2, 1), (1, 2), (2, 2)):
        ho = O.HNormal(om, *sec)
        hs[sec] = H.normal_from_arrays(ho.dimup, ho.dimdw, ho.hd, ho.up, ho.dw, ho.nd)
    _check_transpose_pair(hs[(2, 1)], hs[(1, 2)], 1, seed=70)
    _check_transpose_pair(hs[(2, 2)], hs[(2, 2)], 1, seed=71, variants=False)
    import torch
    buf = torch.zeros(256, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.EdigpuError, match="edigpu_apply_twin: dst is not the twin sector"):
        hs[(2, 1)].twin_to(hs[(2, 2)], buf.data_ptr(), buf.data_ptr() + 8 * 128)
    for h in hs.values():
        h.destroy()


def test_normal_mode_per_orbital_sectors(gpu):
    """ed_total_ud = F, nups = (2, 1), ndws = (1, 2) of 4-level chains: the tensor [iup_1, iup_2, idw_1, idw_2] becomes
    [idw_1, idw_2, iup_1, iup_2] -- the 2-D transpose with DimUp = 6 * 4, DimDw = 4 * 6"""
    from edipack_amd import capi
    from tests.test_gpu_axisop import _orbs_models
    _, pm = _orbs_models(2, 3)
    H = _H()
    a, b = H.orbs_from_model(pm, (2, 1), (1, 2)), H.orbs_from_model(pm, (1, 2), (2, 1))
    assert a.dim == b.dim == 576
    for nvec, o1, o2 in ((1, 0, 0), (3, 1, 1)):
        v = _vectors(a, nvec, 80 + nvec)
        got = _twin_call(a, b, v, nvec, o1, o2)
        t = v.reshape(nvec, 6, 4, 4, 6)                      # [idw_2, idw_1, iup_2, iup_1], the first index fastest
        ref = np.ascontiguousarray(t.transpose(0, 3, 4, 1, 2)).reshape(nvec, -1)
        assert np.array_equal(got, ref)
        assert np.array_equal(ref, _transpose_ref(v, nvec, 1, 24, 24))
    c = H.orbs_from_model(pm, (2, 1), (2, 1))                # the same dimensions axis by axis as b, another sector
    import torch
    buf = torch.zeros(2 * 576, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.EdigpuError, match="edigpu_apply_twin: dst is not the twin sector"):
        a.twin_to(c, buf.data_ptr(), buf.data_ptr() + 8 * 576)
    for h in (a, b, c):
        h.destroy()


def _flat_sectors(mode, ns):
    return list(range(-ns, ns + 1)) if mode == SUPERC else list(range(0, 2 * ns + 1))


@pytest.mark.parametrize("nph", [0, 2])
@pytest.mark.parametrize("form", ["stored", "direct"])
@pytest.mark.parametrize("ed_mode,mode", [("superc", SUPERC), ("nonsu2", NONSU2)])
def test_superc_nonsu2_every_sector(gpu, ed_mode, mode, form, nph):
    """Norb = 2, Nbath = 2 (Ns = 6; the largest sector has 924 rows: four workgroups): every sector against v[order]"""
    from edipack_amd.hamiltonian import sector_map
    _, pm = make_models(ed_mode, "normal", 2, 2, seed=9)
    if nph:
        _phonons(pm, 2)
    H = _H()
    build = H.flat_from_model if form == "stored" else H.direct_from_model
    ns, nblk = pm.ns, nph + 1
    assert ns == 6
    done = 0
    for q in _flat_sectors(mode, ns):
        tq = -q if mode == SUPERC else 2 * ns - q
        states = sector_map(pm, q)
        a = build(pm, q)
        b = a if tq == q else build(pm, tq)
        assert a.dim == nblk * states.size and b.dim == a.dim
        order = twin_order_ref(mode, ns, states)
        for nvec, o1, o2 in ((1, 0, 0), (3, 1, 1)):
            v = _vectors(a, nvec, 90 + q)
            got = _twin_call(a, b, v, nvec, o1, o2)
            ref = v.reshape(nvec, nblk, states.size)[:, :, order].reshape(nvec, -1)
            assert np.array_equal(_words(got), _words(ref)), (q, nvec)
        if b is not a:
            b.destroy()
        a.destroy()
        done += 1
    assert done == 2 * ns + 1


def test_stored_and_direct_handles_go_together(gpu):
    """a stored source with an on-the-fly destination: one kind of sector, the same map"""
    from edipack_amd.hamiltonian import sector_map
    _, pm = make_models("superc", "normal", 2, 2, seed=9)
    H = _H()
    a, b = H.flat_from_model(pm, 1), H.direct_from_model(pm, -1)
    v = _vectors(a, 1, 3)
    assert np.array_equal(_words(_twin_call(a, b, v)), _words(v[:, twin_order_ref(SUPERC, pm.ns, sector_map(pm, 1))]))
    a.destroy(), b.destroy()


@pytest.mark.parametrize("kind", ["normal", "normal_phonon", "normal_cmplx", "superc", "nonsu2"])
def test_twin_of_the_twin_is_the_vector(gpu, kind):
    """the involution, bit for bit"""
    H = _H()
    if kind.startswith("normal"):
        om, pm = make_models("normal", "normal", 2, 3, seed=5)
        if kind == "normal_phonon":
            _phonons(pm, 2)
        if kind == "normal_cmplx":
            from tests.test_gpu_axisop import _complexify
            _complexify(om, pm, 32)
        build = H.normal_cmplx_from_model if kind == "normal_cmplx" else H.normal_from_model
        a, b = build(pm, 3, 5), build(pm, 5, 3)
    else:
        _, pm = make_models(kind, "normal", 2, 2, seed=9)
        a, b = (H.flat_from_model(pm, 1), H.flat_from_model(pm, -1)) if kind == "superc" else \
               (H.flat_from_model(pm, 5), H.flat_from_model(pm, 7))
    v = _vectors(a, 2, 21)
    mid = _twin_call(a, b, v, 2)
    assert not np.array_equal(mid, v)
    back = _twin_call(b, a, mid, 2)
    assert np.array_equal(_words(back), _words(v))
    a.destroy(), b.destroy()


# ---------------------------------------------------------------------------------------------------------
# what the reorder is for: with a spin-symmetric Hamiltonian it maps eigenvectors of A to eigenvectors of B
# ---------------------------------------------------------------------------------------------------------
def _golden_normal_model():
    from tests.test_oracle_golden import _from_dir, golden_models
    inp, par = _from_dir("NORMAL_NORMAL")
    pm_par = {k: v for k, v in par.items() if k not in ("ed_hw_bath", "deltasc")}
    return golden_models(inp["ED_MODE"], inp["BATH_TYPE"], int(inp["NORB"]), int(inp["NBATH"]), pm_par)


def _dense(h):
    eye = np.eye(h.dim)
    return np.stack([h.apply(eye[:, k].copy()) for k in range(h.dim)], axis=1)


@pytest.fixture(scope="module")
def symmetric_pair(gpu):
    """sectors (3, 2) and (2, 3) of the NORMAL_NORMAL fixture's model (Nspin = 1, Jx, Jp != 0), their dense matrices column
    by column from the handles' own products, computed once"""
    _, pm = _golden_normal_model()
    assert pm.nspin == 1 and pm.jx != 0.0 and pm.jp != 0.0
    H = _H()
    a, b = H.normal_from_model(pm, 3, 2), H.normal_from_model(pm, 2, 3)
    yield a, b, _dense(a), _dense(b)
    a.destroy(), b.destroy()


def test_spin_symmetric_hamiltonian_commutes_with_the_reorder(symmetric_pair):
    """H_B = P H_A P^T entry by entry, (P v)[i] = v[order[i]].  An entry is a sum of fewer than 16 terms of magnitude at
    most max|H| that the two sectors may add in another order: 16 eps max|H|."""
    a, b, ha, hb = symmetric_pair
    order = np.arange(a.dim).reshape(a.dim_dw, a.dim_up).T.reshape(-1)
    # P itself, from the device
    assert np.array_equal(_twin_call(a, b, np.arange(a.dim, dtype=np.float64)[None, :])[0], order.astype(np.float64))
    bound = 16 * np.finfo(float).eps * np.max(np.abs(ha))
    err = np.max(np.abs(hb - ha[np.ix_(order, order)]))
    print(f"max |H_B - P H_A P^T| = {err:.3e}, bound {bound:.3e}, max|H| = {np.max(np.abs(ha)):.3f}")
    assert np.count_nonzero(ha) > a.dim and err <= bound


def test_twin_of_an_eigenvector_has_up_and_down_swapped(symmetric_pair):
    """edigpu_occ_moments of the twin of an eigenvector of A = that of the eigenvector with the up and down blocks
    swapped, to 1e-13 relative (the bound tests/test_gpu_occupations.py applies to sums taken in another order); and the
    twin is an eigenvector of B with the same eigenvalue"""
    import torch
    a, b, ha, hb = symmetric_pair
    e, x = np.linalg.eigh(ha)
    v = np.ascontiguousarray(x[:, 0])
    src = torch.from_numpy(v).cuda()
    dst = torch.zeros(b.dim, dtype=torch.float64, device="cuda")
    a.twin_to(b, src.data_ptr(), dst.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ma, na = a.occ_moments(src.data_ptr())
    mb, nb = b.occ_moments(dst.data_ptr())
    norb = 2
    swap = np.r_[norb:2 * norb, 0:norb]
    err = np.max(np.abs(mb[0] - ma[0][np.ix_(swap, swap)])) / np.max(np.abs(ma[0]))
    print(f"moments: rel err {err:.3e}; norm2 {na[0]!r} {nb[0]!r}")
    assert err <= 1e-13 and abs(nb[0] - na[0]) <= 1e-13 * na[0]
    assert not np.allclose(ma[0][:norb, :norb], ma[0][norb:, norb:], atol=1e-6)      # (3, 2): the blocks do differ
    w = dst.cpu().numpy()
    resid = np.linalg.norm(hb @ w - e[0] * w)
    print(f"|H_B w - e0 w| = {resid:.3e}")
    assert resid <= 1e-12 * np.max(np.abs(e))


# ---------------------------------------------------------------------------------------------------------
def test_refusals_by_message(gpu):
    import ctypes as C

    import torch
    from edipack_amd import capi
    from tests.common import make_jz_models
    H = _H()
    L = capi.lib()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    p1, p2 = buf.data_ptr(), buf.data_ptr() + 8 * (1 << 15)
    made = []

    def keep(h):
        made.append(h)
        return h

    def refused(match, src, dst, a=p1, b=p2, nvec=1):
        with pytest.raises(capi.EdigpuError, match=match):
            src.twin_to(dst, a, b, nvec)
        if nvec == 1:      # the timer makes the same checks (on one vector)
            ms = C.c_double(0.0)
            assert L.edigpu_time_twin(src._h, dst._h, a, b, 0, 1, C.byref(ms)) != 0
            assert "edigpu_time_twin: " in capi.last_error()

    _, pn = make_models("normal", "normal", 2, 2, seed=11)
    _, pn2 = make_models("normal", "normal", 2, 2, seed=12)
    a, b = keep(H.normal_from_model(pn, 3, 2)), keep(H.normal_from_model(pn, 2, 3))
    # NULL arguments, nvec, overlap
    assert L.edigpu_apply_twin(None, b._h, p1, p2, 1, None) != 0 and "edigpu_apply_twin: NULL argument" in capi.last_error()
    assert L.edigpu_apply_twin(a._h, None, p1, p2, 1, None) != 0 and "edigpu_apply_twin: NULL argument" in capi.last_error()
    assert L.edigpu_apply_twin(a._h, b._h, None, p2, 1, None) != 0 and "edigpu_apply_twin: NULL argument" in capi.last_error()
    assert L.edigpu_apply_twin(a._h, b._h, p1, None, 1, None) != 0 and "edigpu_apply_twin: NULL argument" in capi.last_error()
    refused("edigpu_apply_twin: nvec must be at least 1", a, b, nvec=0)
    with pytest.raises(capi.EdigpuError, match="edigpu_apply_twin: nvec must be at least 1"):
        a.twin_to(b, p1, p2, -2)
    refused("edigpu_apply_twin: v_dst overlaps v_src", a, b, p1, p1)
    refused("edigpu_apply_twin: v_dst overlaps v_src", a, b, p1, p1 + 8 * (a.dim - 1))
    refused("edigpu_apply_twin: v_dst overlaps v_src", a, b, p1 + 8 * (2 * a.dim - 1), p1, nvec=2)
    a.twin_to(b, p1, p1 + 8 * a.dim)                              # adjacent is not overlapping
    # not the twin; a self-twin needs no second handle but any other sector does
    c = keep(H.normal_from_model(pn, 3, 3))
    refused(r"edigpu_apply_twin: dst is not the twin sector of src \(Nup, Ndw\) = \(2, 3\)", a, a)
    refused("edigpu_apply_twin: dst is not the twin sector", a, c)
    refused("edigpu_apply_twin: dst is not the twin sector", c, a)
    # shards
    rows = keep(H.normal_from_model(pn, 3, 2, dw_first=2, dw_count=5))
    refused("edigpu_apply_twin: the handles must hold the whole sector", rows, b)
    refused("edigpu_apply_twin: the handles must hold the whole sector", a, keep(H.normal_from_model(pn, 2, 3, dw_first=0, dw_count=3)))
    _, ps = make_models("superc", "normal", 2, 2, seed=9)
    s1, s2 = keep(H.flat_from_model(ps, 1)), keep(H.flat_from_model(ps, -1))
    refused("edigpu_apply_twin: the handles must hold the whole sector", keep(H.flat_from_model(ps, 1, row_first=1, row_count=10)), s2)
    # another model, another nph, another kind
    refused("edigpu_apply_twin: sectors of different models", a, keep(H.normal_from_model(pn2, 2, 3)))
    pp = make_models("normal", "normal", 2, 2, seed=11)[1]
    _phonons(pp, 2)
    refused("edigpu_apply_twin: the handles have different nph", a, keep(H.normal_from_model(pp, 2, 3)))
    refused("edigpu_apply_twin: the handles are of different kind", a, s2)
    refused("edigpu_apply_twin: the handles are of different kind", s1, b)
    from tests.test_gpu_axisop import _complexify
    oz, pz = make_models("normal", "normal", 2, 2, seed=11)
    _complexify(oz, pz, 32)
    refused("edigpu_apply_twin: the handles are of different kind", a, keep(H.normal_cmplx_from_model(pz, 2, 3)))
    from oracle import oracle as O
    om = make_models("normal", "normal", 2, 2, seed=11)[0]
    ho = O.HNormal(om, 2, 3)
    refused("edigpu_apply_twin: sectors of different models", a,
            keep(H.normal_from_arrays(ho.dimup, ho.dimdw, ho.hd, ho.up, ho.dw, ho.nd)))
    # superc / nonsu2: the wrong sector; JZ_BASIS; hand-over CSR
    refused("edigpu_apply_twin: dst is not the twin sector of src -1", s1, s1)
    refused("edigpu_apply_twin: dst is not the twin sector of src -1", s1, keep(H.flat_from_model(ps, 0)))
    _, pj = make_jz_models(1)
    hj = keep(H.flat_jz_from_model(pj, 3, 1))
    refused("edigpu_apply_twin: JZ_BASIS sectors are not supported", hj, hj)
    hd = keep(H.direct_jz_from_model(pj, 3, 1))
    refused("edigpu_apply_twin: JZ_BASIS sectors are not supported", hd, hd)
    csr = keep(H.csr_from_arrays(np.arange(5, dtype=np.int64), np.arange(4, dtype=np.int32), np.ones(4)))
    refused("edigpu_apply_twin: a hand-over flat handle .* has no sector map", csr, csr)
    refused("edigpu_apply_twin: a hand-over flat handle .* has no sector map", s1, csr)
    # the timer's own arguments
    ms = C.c_double(0.0)
    assert L.edigpu_time_twin(a._h, b._h, p1, p2, 0, 0, C.byref(ms)) != 0 and "edigpu_time_twin: bad argument" in capi.last_error()
    assert L.edigpu_time_twin(a._h, b._h, p1, p2, 1, 3, None) != 0 and "edigpu_time_twin: bad argument" in capi.last_error()
    assert a.time_twin(b, p1, p2, 1, 3) > 0.0
    torch.cuda.synchronize()
    assert np.isfinite(buf.sum().item())
    for h in made:
        h.destroy()


def test_order_table_is_built_once(gpu):
    """superc: the table belongs to the source handle -- the first call allocates it, a second call allocates nothing and
    returns the same bits"""
    import torch
    _, ps = make_models("superc", "normal", 2, 2, seed=9)
    H = _H()
    a, b = H.flat_from_model(ps, 1), H.flat_from_model(ps, -1)
    x = torch.from_numpy(_vectors(a, 1, 5)[0]).cuda()
    y = torch.zeros_like(x)
    a.twin_to(b, x.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()
    first = y.cpu().numpy().copy()
    free1 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        y.zero_()
        a.twin_to(b, x.data_ptr(), y.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_words(y.cpu().numpy()), _words(first))
    assert torch.cuda.mem_get_info()[0] == free1
    a.destroy(), b.destroy()
