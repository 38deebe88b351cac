"""Green's-function and pair seeds on sharded vectors (csrc/edigpu_shard_seeds.hip: edigpu_apply_cops_sharded on phonon and
complex normal-mode sectors and on superc / nonsu2 phonon row shards, edigpu_apply_pairs_sharded, their _info twins).

Ranks share the one GPU of the test box over the shared-memory transport (the process pattern of
tests/test_gpu_library_shards.py).  Reference: the single-GPU entry on the whole vector in the parent process
(apply_cops_to / apply_cops_flat_to / apply_pairs_to, which test_gpu_axisop.py / test_gpu_pairs.py pin on numpy).
Criterion: np.array_equal of the stitched shards with it -- every element is a gather with a fixed term order and no
cross-rank sum, and the arithmetic is the single-GPU kernel's, so equality and not a tolerance.  Every case raises
EdigpuError without the feature.  The ranks of one world serve all cases in turn on one communicator, so that a world costs
one start of its processes."""
import os

import numpy as np
import pytest

from tests.common import make_models, rel_err
from tests.test_gpu_library_shards import _run_world

pytestmark = pytest.mark.gpu

NPH = 3
UP, DW = 0, 1


def _pair_terms():
    from edipack_amd.observables import exct_chi_seeds, pair_chi_seeds
    return {"pair_00": pair_chi_seeds(0, 0)[0][0], "pair_01": pair_chi_seeds(0, 1)[0][0],
            "exct_singlet_01": exct_chi_seeds(1, 0, 1)[0][0], "up_up": [(1.0, (0, 1, UP), (1, 0, UP))]}


# name -> kind ("cops": ops = [(coef, create, iorb, ispin)]; "pairs": ops = a key of _pair_terms), model (mode, bath, norb,
# nbath), source and destination sector, ops, flags (phonon, cmplx, direct), worlds, the route _info must report (None: any)
CASES = {
    # rows kernel, I = 70 inside one 128-chunk; source rows 24, 24, 22 and destination rows 19, 19, 18 on three ranks
    "c01_down_rows_phonon": ("cops", ("normal", "normal", 2, 3), (4, 4), (4, 3), [(1.0, False, 1, DW)], "p", (1, 2, 3), 1),
    # up operators: the local route
    "c02_up_local_phonon": ("cops", ("normal", "normal", 2, 3), (4, 4), (5, 4), [(1.0, True, 0, UP), (0.7, True, 1, UP)], "p",
                            (1, 2, 3), 0),
    # I = 252: a full and a partial chunk, 211 680 elements
    "c03_down_two_chunks_phonon": ("cops", ("normal", "hybrid", 3, 7), (5, 4), (5, 5), [(1.0, True, 0, DW), (-0.4, True, 2, DW)],
                                   "p", (1, 2, 3), 1),
    # complex twin of c01: I = 140 doubles, complex coefficients
    "c04_down_cmplx": ("cops", ("normal", "normal", 2, 3), (4, 4), (4, 3), [(1.0, False, 0, DW), (-0.5j, False, 1, DW)], "z",
                       (1, 2, 3), 1),
    # gather kernel with I = 2, local route
    "c05_up_cmplx": ("cops", ("normal", "normal", 2, 3), (4, 4), (3, 4), [(1.0, False, 0, UP), (-0.5j, False, 1, UP)], "z",
                     (1, 2, 3), 0),
    # destination DimDw = 1: ranks >= 1 pass NULL destinations; world 10: ranks 6 .. 9 own no source row either; gather
    # kernel with the window (I = 20)
    "c06_one_row_phonon": ("cops", ("normal", "normal", 2, 2), (3, 1), (3, 0), [(1.0, False, 0, DW)], "p", (3, 10), 1),
    # flat kernel, window and blocks: stored rows, then on the fly
    "c07_superc_phonon": ("cops", ("superc", "hybrid", 2, 2), 0, -1, [(1.0, False, 0, UP), (1.0, True, 1, DW)], "p", (1, 2, 3), 1),
    "c08_nonsu2_phonon_direct": ("cops", ("nonsu2", "normal", 2, 2), 4, 3, [(1.0, False, 0, UP), (-1.0j, False, 1, DW)], "pd",
                                 (1, 2, 3), 1),
    # pairs: row partners and column partners through the all-gather
    "c09a_pairs_one_term": ("pairs", ("normal", "normal", 2, 3), (4, 4), (3, 3), "pair_00", "", (1, 2, 3), 1),
    "c09b_pairs_two_terms": ("pairs", ("normal", "normal", 2, 3), (4, 4), (3, 3), "pair_01", "", (1, 2, 3), 1),
    # src == dst: an up-up term and a down-down term
    "c10_pairs_same_sector": ("pairs", ("normal", "normal", 2, 3), (4, 4), (4, 4), "exct_singlet_01", "", (1, 2, 3), 1),
    "c11_pairs_up_only": ("pairs", ("normal", "normal", 2, 3), (4, 4), (4, 4), "up_up", "", (1, 2, 3), 0),
    # the block index in the source offset
    "c12_pairs_phonon": ("pairs", ("normal", "normal", 2, 3), (4, 4), (3, 3), "pair_01", "p", (1, 2, 3), 1),
    # the local pairs route with phonon blocks: the rank's rows of every block as one vector (the twin of c02)
    "c13_pairs_up_only_phonon": ("pairs", ("normal", "normal", 2, 3), (4, 4), (4, 4), "up_up", "p", (1, 2, 3), 0),
}
# the cases whose ranks repeat the call on device pointers (host and device vectors, two calls: the same bits)
TWICE = ("c01_down_rows_phonon", "c02_up_local_phonon", "c04_down_cmplx", "c07_superc_phonon", "c09b_pairs_two_terms",
         "c11_pairs_up_only", "c13_pairs_up_only_phonon")


def _model(case):
    kind, (mode, bath, norb, nbath), s1, s2, ops, flags, worlds, route = CASES[case]
    om, pm = make_models(mode, bath, norb, nbath, seed=31)
    if "p" in flags:      # the couplings of test_gpu_library_shards._reference(..., phonon=True)
        pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = NPH, 0.8, 0.15, np.diag([0.4, -0.3, 0.2][:norb])
    if "z" in flags:
        from tests.test_gpu_axisop import _complexify
        _complexify(om, pm, 32)
    return pm


def _whole_handles(case, pm):
    from edipack_amd.hamiltonian import SectorHamiltonian as H
    kind, (mode, _, _, _), s1, s2, ops, flags, _, _ = CASES[case]
    if mode != "normal":
        build = H.direct_from_model if "d" in flags else H.flat_from_model
        return build(pm, s1), build(pm, s2)
    build = H.normal_cmplx_from_model if "z" in flags else H.normal_from_model
    h1 = build(pm, *s1)
    return h1, (h1 if s2 == s1 else build(pm, *s2))


def _vector(case, dim):
    _, (mode, _, _, _), _, _, _, flags, _, _ = CASES[case]
    rng = np.random.default_rng(17)
    v = rng.standard_normal(dim)
    return v + 1j * rng.standard_normal(dim) if mode != "normal" or "z" in flags else v


def _shard_index(h, first, count):
    """global indices of a rank's shard, block after block of its rows"""
    ul = h.dim_up if h.kind in (0, 3, 4) and h.dim_up > 0 else 1
    nblk = h.nph + 1
    dim_el = h.dim // nblk
    base = np.arange(first * ul, (first + count) * ul)
    return np.concatenate([b * dim_el + base for b in range(nblk)])


def _call(comm, case, h1, h2, v_shard, nloc_dst, out=None):
    kind, ops = CASES[case][0], CASES[case][4]
    if kind == "pairs":
        terms = _pair_terms()[ops]
        return comm.apply_pairs(h1, h2, v_shard, nloc_dst, terms, out=out), comm.apply_pairs_info(h1, h2, terms)
    return comm.apply_cops(h1, h2, v_shard, nloc_dst, ops, out=out), comm.apply_cops_info(h1, h2, ops)


def _rank_handles(comm, case, pm):
    """(source handle, destination handle, (first, count) of either) of this rank"""
    from edipack_amd.sharding import library_sharded_sector
    _, (mode, _, _, _), s1, s2, _, flags, _, _ = CASES[case]
    if mode == "normal":
        h1, h2 = _whole_handles(case, pm)
        return h1, h2, comm.plan(h1.dim_dw)[:2], comm.plan(h2.dim_dw)[:2]
    h1, f1, c1 = library_sharded_sector(pm, s1, comm, direct="d" in flags)
    h2, f2, c2 = library_sharded_sector(pm, s2, comm, direct="d" in flags)
    return h1, h2, (f1, c1), (f2, c2)


def _rank_main(rank, world, name, cases, q):
    try:
        import torch
        from edipack_amd import capi
        from edipack_amd.sharding import LibraryComm
        capi.init(0)
        comm = LibraryComm(rank, world, shm_name=name, slot_bytes=1 << 22)
        res = {}
        for case in cases:
            pm = _model(case)
            h1, h2, (f1, c1), (f2, c2) = _rank_handles(comm, case, pm)
            ix1, ix2 = _shard_index(h1, f1, c1), _shard_index(h2, f2, c2)
            v = _vector(case, h1.dim)[ix1]
            out, info = _call(comm, case, h1, h2, v, len(ix2))
            same = None
            if case in TWICE:
                src = torch.from_numpy(np.ascontiguousarray(v)).cuda()
                same = True
                for _ in range(2):
                    dst = torch.full((max(len(ix2), 1),), 7.0, dtype=src.dtype, device="cuda")
                    _call(comm, case, h1, h2, src.data_ptr() if len(ix1) else 0, len(ix2), out=dst.data_ptr() if len(ix2) else 0)
                    torch.cuda.synchronize()
                    same = same and np.array_equal(dst.cpu().numpy()[:len(ix2)].view(np.float64), out.view(np.float64))
                    same = same and np.array_equal(src.cpu().numpy().view(np.float64), np.ascontiguousarray(v).view(np.float64))
            res[case] = (ix2, out, info, (c1, c2), same)
            if h2 is not h1:
                h2.destroy()
            h1.destroy()
        comm.destroy()
        q.put((rank, res, None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, traceback.format_exc() + str(e)))


_REF = {}


def _reference(case):
    """the single-GPU entry on the whole vector, computed once per case and shared by the worlds"""
    if case in _REF:
        return _REF[case]
    import torch
    kind, (mode, _, _, _), s1, s2, ops, flags, _, _ = CASES[case]
    pm = _model(case)
    g1, g2 = _whole_handles(case, pm)
    v = _vector(case, g1.dim)
    src = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    dst = torch.full((g2.dim,), 7.0, dtype=src.dtype, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if kind == "pairs":
        g1.apply_pairs_to(g2, src.data_ptr(), dst.data_ptr(), _pair_terms()[ops], st)
    else:
        fn = g1.apply_cops_to if mode == "normal" else g1.apply_cops_flat_to
        fn(g2, src.data_ptr(), dst.data_ptr(), [o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops], [o[3] for o in ops], st)
    torch.cuda.synchronize()
    ref = dst.cpu().numpy()
    if g2 is not g1:
        g2.destroy()
    g1.destroy()
    assert np.linalg.norm(ref) > 0.0 and not np.any(ref == 7.0)
    _REF[case] = ref
    return ref


@pytest.mark.parametrize("world", [1, 2, 3, 10])
def test_seeds_on_shards_equal_the_single_gpu_seeds(gpu, world):
    cases = [c for c in CASES if world in CASES[c][6]]
    refs = {c: _reference(c) for c in cases}
    res = _run_world(_rank_main, world, (f"edigpu_seeds_{os.getpid()}_{world}", cases))
    for case in cases:
        ref, route = refs[case], CASES[case][7]
        got = np.full_like(ref, np.nan)
        empty_dst = empty_src = 0
        for rank, out, _ in res:
            ix2, shard, info, (c1, c2), same = out[case]
            got[ix2] = shard
            assert info[0] == route, (case, rank, info)
            assert (info[1] == 0) == (route == 0) and info == res[0][1][case][2], (case, rank, info)
            assert same in (None, True), (case, rank, "host and device vectors, or two calls, differ")
            empty_src += c1 == 0
            empty_dst += c2 == 0
        assert np.array_equal(got.view(np.float64), ref.view(np.float64)), (case, world, rel_err(got, ref))
        if case == "c06_one_row_phonon":
            assert empty_dst == world - 1 and empty_src == (4 if world == 10 else 0), (world, empty_src, empty_dst)


def test_case_geometry_is_what_the_cases_name(gpu):
    """the shapes the table above quotes: row lengths on either side of the rows / gather threshold, rows per rank"""
    from edipack_amd.sharding import ShardPlan
    dims = {}
    for case in ("c01_down_rows_phonon", "c03_down_two_chunks_phonon", "c04_down_cmplx", "c06_one_row_phonon"):
        g1, g2 = _whole_handles(case, _model(case))
        dims[case] = (g1.dim_up, g1.dim_dw, g2.dim_dw, g1.dim)
        g1.destroy(), g2.destroy()
    assert dims["c01_down_rows_phonon"] == (70, 70, 56, 70 * 70 * 4)
    assert [ShardPlan(70, 70, 3, r).count for r in range(3)] == [24, 24, 22]
    assert [ShardPlan(56, 70, 3, r).count for r in range(3)] == [19, 19, 18]
    assert dims["c03_down_two_chunks_phonon"] == (252, 210, 252, 211680)
    assert dims["c04_down_cmplx"][:3] == (70, 70, 56)
    assert dims["c06_one_row_phonon"][:3] == (20, 6, 1)


def test_forced_collectives_world_of_one(gpu, monkeypatch):
    """a world of one with the collectives forced through RCCL equals the world of one that copies, and the reference"""
    import torch  # noqa: F401
    from edipack_amd.sharding import LibraryComm
    cases = ("c01_down_rows_phonon", "c02_up_local_phonon", "c04_down_cmplx", "c07_superc_phonon", "c09b_pairs_two_terms",
             "c12_pairs_phonon")
    outs = []
    for force in (True, False):
        if force:
            monkeypatch.setenv("EDIGPU_FORCE_COLLECTIVES", "1")
        else:
            monkeypatch.delenv("EDIGPU_FORCE_COLLECTIVES", raising=False)
        comm = LibraryComm(0, 1, unique_id=LibraryComm.unique_id())
        got = {}
        for case in cases:
            h1, h2, _, _ = _rank_handles(comm, case, _model(case))
            got[case] = _call(comm, case, h1, h2, _vector(case, h1.dim), h2.dim)[0]
            if h2 is not h1:
                h2.destroy()
            h1.destroy()
        comm.destroy()
        outs.append(got)
    for case in cases:
        ref = _reference(case)
        assert np.array_equal(outs[0][case].view(np.float64), ref.view(np.float64)), case
        assert np.array_equal(outs[1][case].view(np.float64), ref.view(np.float64)), case


def test_refusals_by_message(gpu):
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian as H
    from edipack_amd.sharding import LibraryComm
    comm = LibraryComm(0, 1)
    terms = _pair_terms()

    def refused(match, fn):
        with pytest.raises(capi.EdigpuError, match=match):
            fn()

    pm = _model("c01_down_rows_phonon")
    a, b, up = H.normal_from_model(pm, 4, 4), H.normal_from_model(pm, 4, 3), H.normal_from_model(pm, 5, 4)
    v = np.zeros(a.dim)
    # real handles: an imaginary part stays refused; wrong destination; operators of two spins
    refused("edigpu_apply_cops_sharded: .*complex coefficients", lambda: comm.apply_cops(a, b, v, b.dim, [(1.0j, False, 1, DW)]))
    refused("edigpu_apply_cops_sharded_info: .*complex coefficients", lambda: comm.apply_cops_info(a, b, [(1.0j, False, 1, DW)]))
    refused("edigpu_apply_cops_sharded: the destination handle is the sector",
            lambda: comm.apply_cops(a, up, v, up.dim, [(1.0, False, 1, DW)]))
    refused("edigpu_apply_cops_sharded: ", lambda: comm.apply_cops(a, b, v, b.dim, [(1.0, False, 1, DW), (1.0, False, 1, UP)]))
    # a phonon-free destination of a phonon source
    pm0 = _model("c09a_pairs_one_term")
    a0, b0, c0 = H.normal_from_model(pm0, 4, 4), H.normal_from_model(pm0, 4, 3), H.normal_from_model(pm0, 3, 3)
    refused("edigpu_apply_cops_sharded: the two handles have different nph",
            lambda: comm.apply_cops(a, b0, v, b0.dim, [(1.0, False, 1, DW)]))
    # a down-row shard handle on the one-axis route (phonon sectors are never built as row shards)
    rows = H.normal_from_model(pm0, 4, 4, dw_first=2, dw_count=5)
    refused("edigpu_apply_cops_sharded: the source handle is a shard",
            lambda: comm.apply_cops(rows, b, np.zeros(rows.nloc), b.dim, [(1.0, False, 1, DW)]))
    # overlapping device vectors, by name
    t = torch.zeros(a.dim + b.dim, dtype=torch.float64, device="cuda")
    refused("edigpu_apply_cops_sharded: v_dst_shard overlaps v_src_shard",
            lambda: comm.apply_cops(a, b, t.data_ptr(), b.dim, [(1.0, False, 1, DW)], out=t.data_ptr() + 8 * 16))
    refused("edigpu_apply_pairs_sharded: v_dst_shard overlaps v_src_shard",
            lambda: comm.apply_pairs(a0, c0, t.data_ptr(), c0.dim, terms["pair_00"], out=t.data_ptr() + 8 * 16))
    # NULL vectors where the rank owns rows
    refused("edigpu_apply_cops_sharded: NULL vector", lambda: comm.apply_cops(a, b, np.zeros(0), b.dim, [(1.0, False, 1, DW)]))
    # pairs: the refusals of the single-GPU entry under this entry's name
    shard = H.normal_from_model(pm0, 4, 4, dw_first=2, dw_count=5)
    refused("edigpu_apply_pairs_sharded: the source handle must hold the whole sector",
            lambda: comm.apply_pairs(shard, c0, np.zeros(shard.nloc), c0.dim, terms["pair_00"]))
    refused("edigpu_apply_pairs_sharded_info: the source handle must hold the whole sector",
            lambda: comm.apply_pairs_info(shard, c0, terms["pair_00"]))
    pz = _model("c04_down_cmplx")
    z = H.normal_cmplx_from_model(pz, 4, 4)
    refused("edigpu_apply_pairs_sharded: the source handle is a complex normal-mode sector",
            lambda: comm.apply_pairs(z, z, np.zeros(z.dim, complex), z.dim, terms["up_up"]))
    refused("edigpu_apply_pairs_sharded: the destination handle is the sector",
            lambda: comm.apply_pairs(a0, a0, np.zeros(a0.dim), a0.dim, terms["pair_00"]))
    refused("edigpu_apply_pairs_sharded: .*different models", lambda: comm.apply_pairs(a, c0, v, c0.dim, terms["pair_00"]))
    refused("edigpu_apply_pairs_sharded: nterms must be 1 .. 8",
            lambda: comm.apply_pairs(a0, c0, np.zeros(a0.dim), c0.dim, terms["pair_00"] * 9))
    # complex handle with a real one
    refused("edigpu_apply_cops_sharded: the handles are of different kinds",
            lambda: comm.apply_cops(z, b, np.zeros(z.dim, complex), b.dim, [(1.0, False, 1, DW)]))
    for h in (a, b, up, a0, b0, c0, rows, shard, z):
        h.destroy()
    comm.destroy()


# ---------------------------------------------------------------------------------------------------------
# end to end: solve -> seed -> tridiagonalise on two ranks (the chain the feature closes)
# ---------------------------------------------------------------------------------------------------------
E2E = {
    # Holstein model: Norb 1, Nbath 3, nph = 3, sector (2, 2); the four c / c^+ seeds of the Green's function
    "holstein": (("normal", "normal", 1, 3), (2, 2), "p"),
    # complex impHloc needs two orbitals: Norb 2, Nbath 2, sector (3, 3)
    "complex": (("normal", "normal", 2, 2), (3, 3), "z"),
}
E2E_OPS = [(True, UP), (False, UP), (True, DW), (False, DW)]      # (create, ispin) of orbital 0
NLANC = 20


def _e2e_model(which):
    (mode, bath, norb, nbath), sec, flags = E2E[which]
    om, pm = make_models(mode, bath, norb, nbath, seed=31)
    if "p" in flags:
        pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = NPH, 0.8, 0.15, np.diag([0.4, -0.3][:norb])
    if "z" in flags:
        from tests.test_gpu_axisop import _complexify
        _complexify(om, pm, 32)
    return pm, sec, flags


def _e2e_build(pm, flags, nup, ndw):
    from edipack_amd.hamiltonian import SectorHamiltonian as H
    return (H.normal_cmplx_from_model if "z" in flags else H.normal_from_model)(pm, nup, ndw)


def _e2e_dest(sec, create, spin):
    d = 1 if create else -1
    return (sec[0] + d, sec[1]) if spin == UP else (sec[0], sec[1] + d)


def _e2e_rank_main(rank, world, name, which, gs, q):
    try:
        import torch  # noqa: F401
        from edipack_amd import capi
        from edipack_amd.sharding import LibraryComm
        capi.init(0)
        comm = LibraryComm(rank, world, shm_name=name, slot_bytes=1 << 22)
        pm, sec, flags = _e2e_model(which)
        h = _e2e_build(pm, flags, *sec)
        ix = _shard_index(h, *comm.plan(h.dim_dw)[:2])
        out = []
        for create, spin in E2E_OPS:
            hd = _e2e_build(pm, flags, *_e2e_dest(sec, create, spin))
            ixd = _shard_index(hd, *comm.plan(hd.dim_dw)[:2])
            seed = comm.apply_cops(h, hd, gs[ix], len(ixd), [(1.0, create, 0, spin)])
            out.append(comm.tridiag(hd, seed, NLANC))
            hd.destroy()
        h.destroy()
        comm.destroy()
        q.put((rank, out, None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, traceback.format_exc() + str(e)))


@pytest.mark.parametrize("which", sorted(E2E))
def test_solve_seed_tridiagonalise_on_two_ranks(gpu, which):
    """the single-GPU ground state cut into two shards (no sign or degeneracy ambiguity), c / c^+ of either spin on the
    shards, then the sharded recurrence on the seed shards: alpha and beta against the single-GPU seeds and
    lanczos_tridiag_dev at the bound test_library_shards_share_one_gpu applies to sharded coefficients (1e-10)"""
    import torch
    pm, sec, flags = _e2e_model(which)
    g = _e2e_build(pm, flags, *sec)
    _, vec, nconv, _ = g.lanczos_eigh_multi(1, tol=1e-12)
    assert nconv == 1
    gs = np.ascontiguousarray(vec[0])
    src = torch.from_numpy(gs).cuda()
    refs = []
    for create, spin in E2E_OPS:
        gd = _e2e_build(pm, flags, *_e2e_dest(sec, create, spin))
        dst = torch.zeros(gd.dim, dtype=src.dtype, device="cuda")
        g.apply_cops_to(gd, src.data_ptr(), dst.data_ptr(), [1.0], [create], [0], [spin], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        refs.append(gd.lanczos_tridiag_dev(dst.data_ptr(), NLANC))
        gd.destroy()
    g.destroy()
    res = _run_world(_e2e_rank_main, 2, (f"edigpu_seeds_e2e_{os.getpid()}_{which}", which, gs))
    for rank, out, _ in res:
        for k, ((a, b, nd, n2), (ra, rb, rnd, rn2)) in enumerate(zip(out, refs)):
            print(which, "rank", rank, "op", E2E_OPS[k], "niter", nd, rnd, "alpha", rel_err(a[:rnd], ra[:rnd]), "beta",
                  rel_err(b[:rnd], rb[:rnd]), "norm2", n2, rn2)
            assert rn2 > 0.0 and abs(n2 - rn2) < 1e-10 * rn2
            assert nd == rnd and rel_err(a, ra) < 1e-10 and rel_err(b, rb) < 1e-10, (which, rank, E2E_OPS[k])
