"""The ED_TWIN=T reorder on sharded vectors (csrc/edigpu_twin.hip: edigpu_apply_twin_sharded): the twin sector's shards
from the shards the sharded solve leaves, by one all-gather and the window form of the single-GPU kernels.

Ranks share the one GPU of the test box over the shared-memory transport (the process pattern of
tests/test_gpu_library_shards.py).  Reference: edigpu_apply_twin on the whole vectors in the parent process (which
tests/test_gpu_twin.py pins on numpy).  Criterion: np.array_equal of the stitched shards with it -- a permutation has no
tolerance.  The ranks of one world serve all cases in turn on one communicator, so that a world costs one start of its
processes.  Every case raises AttributeError / EdigpuError without the feature."""
import os

import numpy as np
import pytest

from tests.common import make_models
from tests.test_gpu_library_shards import _run_world
from tests.test_gpu_shard_seeds import _shard_index

pytestmark = pytest.mark.gpu

# name -> model (mode, bath, norb, nbath), source sector, twin sector, flags (p: nph = 2, z: _CMPLX_NORMAL, d: on the fly),
# nvec, worlds
CASES = {
    # DimDw x DimUp = 70 x 8 -> 8 x 70: ten ranks cut the 8 destination rows one each, ranks 8 and 9 own none
    "t01_normal_70x8": (("normal", "normal", 2, 3), (1, 4), (4, 1), "", 2, (1, 2, 3, 10)),
    # 126 x 84 with three phonon blocks: the block index in the source offset, tiles cut by the window
    "t02_normal_126x84_phonon": (("normal", "normal", 3, 2), (3, 4), (4, 3), "p", 1, (1, 2, 3)),
    # 20 x 15 complex: an odd row length in double2
    "t03_cmplx_20x15": (("normal", "normal", 2, 2), (2, 3), (3, 2), "z", 2, (1, 2, 3)),
    # the other way round (8 x 70 -> 70 x 8): even rows on the write side only
    "t04_normal_8x70": (("normal", "normal", 2, 3), (4, 1), (1, 4), "", 1, (2, 3)),
    "t05_superc_stored": (("superc", "normal", 2, 2), 1, -1, "", 2, (1, 2, 3, 10)),
    "t06_superc_direct_phonon": (("superc", "normal", 2, 2), -2, 2, "pd", 1, (1, 2, 3)),
    "t07_nonsu2_stored_phonon": (("nonsu2", "normal", 2, 2), 5, 7, "p", 2, (1, 2, 3)),
    "t08_nonsu2_direct": (("nonsu2", "normal", 2, 2), 4, 8, "d", 1, (1, 2, 3)),
    # a self-twin sector: one handle on both sides
    "t09_superc_self": (("superc", "normal", 2, 2), 0, 0, "", 1, (2, 3)),
}
# the cases whose ranks repeat the call on device pointers (host and device vectors, two calls: the same bits)
TWICE = ("t01_normal_70x8", "t02_normal_126x84_phonon", "t03_cmplx_20x15", "t05_superc_stored", "t07_nonsu2_stored_phonon")


def _model(case):
    (mode, bath, norb, nbath), _, _, flags, _, _ = CASES[case]
    om, pm = make_models(mode, bath, norb, nbath, seed=31)
    if "p" in flags:
        pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = 2, 0.8, 0.15, np.diag([0.4, -0.3, 0.2][:norb])
    if "z" in flags:
        from tests.test_gpu_axisop import _complexify
        _complexify(om, pm, 32)
    return pm


def _whole_handles(case, pm):
    from edipack_amd.hamiltonian import SectorHamiltonian as H
    (mode, _, _, _), s1, s2, flags, _, _ = CASES[case]
    if mode != "normal":
        build = H.direct_from_model if "d" in flags else H.flat_from_model
        h1 = build(pm, s1)
        return h1, (h1 if s2 == s1 else build(pm, s2))
    build = H.normal_cmplx_from_model if "z" in flags else H.normal_from_model
    return build(pm, *s1), build(pm, *s2)


def _vectors(case, h):
    rng = np.random.default_rng(23)
    nvec = CASES[case][4]
    v = rng.standard_normal((nvec, h.dim))
    return v + 1j * rng.standard_normal((nvec, h.dim)) if h.is_complex else v


def _rank_handles(comm, case, pm):
    """(source handle, destination handle, (first, count) of either) of this rank"""
    from edipack_amd.sharding import library_sharded_sector
    (mode, _, _, _), s1, s2, flags, _, _ = CASES[case]
    if mode == "normal":
        h1, h2 = _whole_handles(case, pm)
        return h1, h2, comm.plan(h1.dim_dw)[:2], comm.plan(h2.dim_dw)[:2]
    h1, f1, c1 = library_sharded_sector(pm, s1, comm, direct="d" in flags)
    if s2 == s1:
        return h1, h1, (f1, c1), (f1, c1)
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
            nvec = CASES[case][4]
            h1, h2, (f1, c1), (f2, c2) = _rank_handles(comm, case, pm)
            ix1, ix2 = _shard_index(h1, f1, c1), _shard_index(h2, f2, c2)
            v = np.ascontiguousarray(_vectors(case, h1)[:, ix1])
            out = comm.apply_twin(h1, h2, v, len(ix2), nvec)
            same = None
            if case in TWICE:
                src = torch.from_numpy(v).cuda()
                same = True
                for _ in range(2):
                    dst = torch.full((nvec, max(len(ix2), 1)), 7.0, dtype=src.dtype, device="cuda")
                    comm.apply_twin(h1, h2, src.data_ptr() if len(ix1) else 0, len(ix2), nvec, out=dst.data_ptr() if len(ix2) else 0)
                    torch.cuda.synchronize()
                    if len(ix2):
                        same = same and np.array_equal(dst.cpu().numpy().view(np.float64), out.view(np.float64))
                    same = same and np.array_equal(src.cpu().numpy().view(np.float64), v.view(np.float64))
            res[case] = (ix2, out, (c1, c2), same)
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
    """edigpu_apply_twin on the whole vectors, computed once per case and shared by the worlds"""
    if case in _REF:
        return _REF[case]
    import torch
    pm = _model(case)
    g1, g2 = _whole_handles(case, pm)
    v = _vectors(case, g1)
    src = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    dst = torch.full(v.shape, 7.0, dtype=src.dtype, device="cuda")
    g1.twin_to(g2, src.data_ptr(), dst.data_ptr(), v.shape[0], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = dst.cpu().numpy()
    if g2 is not g1:
        g2.destroy()
    g1.destroy()
    # a permutation of the source: the same multiset of words, nothing left of the filling
    assert np.array_equal(np.sort(ref.view(np.float64), axis=None), np.sort(v.view(np.float64), axis=None))
    _REF[case] = ref
    return ref


@pytest.mark.parametrize("world", [1, 2, 3, 10])
def test_twin_on_shards_equals_the_single_gpu_twin(gpu, world):
    cases = [c for c in CASES if world in CASES[c][5]]
    refs = {c: _reference(c) for c in cases}
    res = _run_world(_rank_main, world, (f"edigpu_twin_{os.getpid()}_{world}", cases))
    for case in cases:
        ref = refs[case]
        got = np.full_like(ref, np.nan)
        empty_dst = empty_src = 0
        for rank, out, _ in res:
            ix2, shard, (c1, c2), same = out[case]
            got[:, ix2] = shard
            assert same in (None, True), (case, rank, "host and device vectors, or two calls, differ")
            empty_src += c1 == 0
            empty_dst += c2 == 0
        assert np.array_equal(got.view(np.float64), ref.view(np.float64)), (case, world)
        if case == "t01_normal_70x8" and world == 10:
            assert (empty_src, empty_dst) == (0, 2)


def test_case_geometry_is_what_the_cases_name(gpu):
    dims = {}
    for case in ("t01_normal_70x8", "t02_normal_126x84_phonon", "t03_cmplx_20x15", "t05_superc_stored"):
        g1, g2 = _whole_handles(case, _model(case))
        dims[case] = (g1.dim_dw, g1.dim_up, g1.dim, g1.is_complex)
        g1.destroy(), g2.destroy()
    assert dims["t01_normal_70x8"] == (70, 8, 560, False)
    assert dims["t02_normal_126x84_phonon"] == (126, 84, 3 * 126 * 84, False)
    assert dims["t03_cmplx_20x15"] == (20, 15, 300, True)
    assert dims["t05_superc_stored"][2] == 792


def test_forced_collectives_world_of_one(gpu, monkeypatch):
    """a world of one with the collectives forced through RCCL equals the world of one that copies, and the reference"""
    import torch  # noqa: F401
    from edipack_amd.sharding import LibraryComm
    cases = ("t01_normal_70x8", "t02_normal_126x84_phonon", "t03_cmplx_20x15", "t05_superc_stored", "t07_nonsu2_stored_phonon")
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
            got[case] = comm.apply_twin(h1, h2, _vectors(case, h1), h2.dim, CASES[case][4])
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
    from tests.common import make_jz_models
    from tests.test_gpu_axisop import _orbs_models
    comm = LibraryComm(0, 1)
    made = []

    def keep(h):
        made.append(h)
        return h

    def refused(match, src, dst, v=None, nvec=1, out=None, nloc=None):
        v = np.zeros(nvec * src.nloc, dtype=src.dtype) if v is None else v
        with pytest.raises(capi.EdigpuError, match="edigpu_apply_twin_sharded: " + match):
            comm.apply_twin(src, dst, v, dst.nloc if nloc is None else nloc, nvec, out=out)

    pm = _model("t01_normal_70x8")
    a, b, c = keep(H.normal_from_model(pm, 1, 4)), keep(H.normal_from_model(pm, 4, 1)), keep(H.normal_from_model(pm, 4, 4))
    refused("dst is not the twin sector", a, c)
    refused("dst is not the twin sector", a, a)
    refused("nvec must be at least 1", a, b, v=np.zeros(a.dim), nvec=0)
    refused("NULL vector", a, b, v=np.zeros(0))
    assert capi.lib().edigpu_apply_twin_sharded(a._h, b._h, None, None, None, 1) != 0
    assert "edigpu_apply_twin_sharded: NULL argument" in capi.last_error()
    t = torch.zeros(2 * a.dim, dtype=torch.float64, device="cuda")
    refused("v_dst overlaps v_src", a, b, v=t.data_ptr(), out=t.data_ptr() + 8 * 16)
    # normal mode shards through the whole-sector handle
    rows = keep(H.normal_from_model(pm, 1, 4, dw_first=2, dw_count=5))
    refused("normal mode shards through the whole-sector handle", rows, b)
    # other models, nph, kinds
    refused("sectors of different models", a, keep(H.normal_from_model(make_models("normal", "normal", 2, 3, seed=32)[1], 4, 1)))
    refused("the handles have different nph", a, keep(H.normal_from_model(_model("t02_normal_126x84_phonon"), 4, 3)))
    ps = _model("t05_superc_stored")
    s1, s2 = keep(H.flat_from_model(ps, 1)), keep(H.flat_from_model(ps, -1))
    refused("the handles are of different kind", a, s2)
    refused("dst is not the twin sector of src -1", s1, keep(H.flat_from_model(ps, 0)))
    # a superc handle that is not this rank's shard (this rank owns every row of a world of one)
    part = keep(H.flat_from_model(ps, 1, row_first=1, row_count=10))
    refused("the handle does not hold this rank's shard", part, s2)
    refused("the handle does not hold this rank's shard", s1, keep(H.flat_from_model(ps, -1, row_first=0, row_count=7)))
    # not served on shards: ed_total_ud=F, hand-over handles; JZ_BASIS and hand-over CSR as on one GPU
    _, po = _orbs_models(2, 3)
    o1, o2 = keep(H.orbs_from_model(po, (2, 1), (1, 2))), keep(H.orbs_from_model(po, (1, 2), (2, 1)))
    refused("ed_total_ud=F sectors are not served on shards", o1, o2)
    from oracle import oracle as O
    om, _ = make_models("normal", "normal", 2, 1, seed=5)
    hands = [O.HNormal(om, *sec) for sec in ((2, 1), (1, 2))]
    n1, n2 = [keep(H.normal_from_arrays(ho.dimup, ho.dimdw, ho.hd, ho.up, ho.dw, ho.nd)) for ho in hands]
    refused("hand-over handles are not served on shards", n1, n2)
    _, pj = make_jz_models(1)
    hj = keep(H.flat_jz_from_model(pj, 3, 1))
    refused("JZ_BASIS sectors are not supported", hj, hj)
    csr = keep(H.csr_from_arrays(np.arange(5, dtype=np.int64), np.arange(4, dtype=np.int32), np.ones(4)))
    refused("a hand-over flat handle .* has no sector map", csr, csr)
    for h in made:
        h.destroy()
    comm.destroy()
