"""GPU tests of the impurity reduced density matrix on sharded normal-mode vectors (edigpu_imp_rdm_sharded through
LibraryComm.imp_rdm): spawned ranks share the one GPU over the shared-memory transport, as in
tests/test_gpu_library_shards.py, whose cases, references and world runner are reused.

The reference is ref_rdm of tests/test_gpu_rdm.py (numpy in extended precision) with that file's derived bound
4 dim u norm2, dim the dimension of the WHOLE sector, phonon blocks included: an entry is still one sum of at most dim
rounded products, taken in another order (workgroups, then the interior and the boundary slab, then the ranks).  Every
(case, world) that is meant to cut a run of down rows asserts from the sector map that it does.  Every check of a case
runs in one rank function, so a case costs one spawn per world."""
import os

import numpy as np
import pytest

from tests.test_gpu_library_shards import CASES, NPH, _block_env, _reference, _run_world, _shard_index
from tests.test_gpu_rdm import U, ref_rdm
from tests.test_rdm_host import random_vector, sector_maps

pytestmark = pytest.mark.gpu

HYB33 = CASES[1]
PHONON = ("normal", "normal", 2, 2, (3, 3), False, "phonon")   # DimDw = 20: the cut at row 14 of 3 ranks splits [13, 15)
assert HYB33[:5] == ("normal", "hybrid", 3, 3, (3, 2)) and HYB33[6] == "auto"
assert CASES[2][6] == "allgather" and CASES[10][:5] == ("normal", "hybrid", 3, 5, (4, 3)) and CASES[10][6] == "block"
assert CASES[5][:5] == ("normal", "hybrid", 3, 2, (3, 2)) and CASES[5][6] == "cmplx"
# (case, world, a run of down rows is cut)
WORLDS = [
    (HYB33, 1, False),
    (HYB33, 2, True),                 # the cut at row 8 splits [6, 9)
    (HYB33, 3, True),                 # the cut at 5 splits [3, 6); the cut at 10 falls on a run start
    (("normal", "hybrid", 3, 3, (3, 1), False, "auto"), 10, True),   # q = 1: [0, 3) spans three ranks, ranks 6-9 own nothing
    (CASES[2], 2, False),             # row-shard handles
    (CASES[2], 3, False),
    (CASES[10], 2, True),             # whole sector on padded panels (kind 2); the caller's vectors are row layout
    (CASES[10], 3, False),
    (CASES[5], 2, True),              # cw = 2
    (CASES[5], 3, True),
    (PHONON, 3, True),                # the halo carries every phonon block
]


def _case_id(c):
    return f"{c[1]}{c[2]}x{c[3]}-{c[4][0]}.{c[4][1]}-{c[6]}"


def _flags(case):
    return dict(cmplx=case[6] == "cmplx", phonon=case[6] == "phonon")


def _second(v):
    """the second vector of the nvec = 2 calls: seeded, so every rank and the test make the same one"""
    return random_vector(v.size, np.iscomplexobj(v), 91)


def _cut_runs(md, norb, world):
    """the runs [start, end) of equal bath word that a boundary r q cuts"""
    bath = md >> norb
    starts = [0] + [i for i in range(1, md.size) if bath[i] != bath[i - 1]] + [md.size]
    q = -(-md.size // world)
    return [(s, e) for s, e in zip(starts, starts[1:]) for c in range(q, md.size, q) if s < c < e]


def _open(rank, world, name, case):
    import torch  # noqa: F401  (one HIP runtime per process)
    from edipack_amd import capi
    from edipack_amd.sharding import LibraryComm, library_sharded_sector
    capi.init(0)
    mode, bath, norb, nbath, sector, direct, exchange = case
    ho, pm, v = _reference(mode, bath, norb, nbath, sector, **_flags(case))
    comm = LibraryComm(rank, world, shm_name=name, slot_bytes=1 << 22)
    _block_env(exchange == "block")
    h, first, count = library_sharded_sector(pm, sector, comm, direct=direct, exchange="auto" if exchange == "block" else exchange,
                                             cmplx=exchange == "cmplx")
    info = comm.shard_info(h)
    assert exchange != "block" or info[0] == 2, info
    assert not (exchange == "auto" and world <= 3) or info[0] == 1, info
    ix = _shard_index(ho, mode, first, count, exchange == "phonon")
    return comm, h, pm, v, ix


def _case_rank_main(rank, world, name, case, q):
    try:
        import torch
        comm, h, pm, v, ix = _open(rank, world, name, case)
        vs2 = np.ascontiguousarray(np.stack([v[ix], _second(v)[ix]]))
        keep = vs2.copy()
        r = dict(n=ix.size)
        r["rho2"], r["n2"] = comm.imp_rdm(h, vs2, 2)
        r["rho2_again"], r["n2_again"] = comm.imp_rdm(h, vs2, 2)
        r["single"] = [comm.imp_rdm(h, vs2[k]) for k in range(2)]
        r["src_untouched"] = np.array_equal(vs2, keep)
        t = torch.from_numpy(vs2).cuda()
        torch.cuda.synchronize()
        r["rho2_dev"], r["n2_dev"] = comm.imp_rdm(h, t.data_ptr() if ix.size else 0, 2)
        r["dev_untouched"] = np.array_equal(t.cpu().numpy(), keep)
        if world == 1:                                   # the whole sector on one rank: the bits of edigpu_imp_rdm
            r["whole"] = h.imp_rdm(t.data_ptr(), 2)
        h.destroy()
        comm.destroy()
        q.put((rank, r, None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, traceback.format_exc() + str(e)))


@pytest.mark.parametrize("case,world,cut", WORLDS, ids=[f"w{w}-{_case_id(c)}" for c, w, _ in WORLDS])
def test_imp_rdm_on_shards(gpu, case, world, cut):
    mode, bath, norb, nbath, sector, direct, exchange = case
    ho, pm, v = _reference(mode, bath, norb, nbath, sector, **_flags(case))
    mu, md = sector_maps(pm, sector)
    nblk = NPH + 1 if exchange == "phonon" else 1
    assert mu.size * md.size * nblk == v.size
    cuts = _cut_runs(md, norb, world)
    assert bool(cuts) == cut, cuts
    if case[4] == (3, 1):
        assert md.size == 6 and (0, 3) in cuts and cuts.count((0, 3)) == 2         # one run over three ranks
    res = sorted(_run_world(_case_rank_main, world, (f"edigpu_rdm_{os.getpid()}_{world}_{abs(hash(case)) % 100000}", case)),
                 key=lambda x: x[0])
    assert sum(r["n"] for _, r, _ in res) == v.size
    if case[4] == (3, 1):
        assert [r["n"] for _, r, _ in res][6:] == [0, 0, 0, 0]                     # ranks that pass NULL
    D, cplx = 4 ** norb, np.iscomplexobj(v)
    rho0, n20 = res[0][1]["rho2"], res[0][1]["n2"]
    for k, vk in enumerate((v, _second(v))):
        ref, n2r = ref_rdm(mu, md, norb, vk, nblk)
        tol = 4 * v.size * U * n2r
        print(f"imp_rdm on {world} shards, vector {k}: dim={v.size} max|drho|={np.max(np.abs(rho0[k] - ref)):.3e} "
              f"|trace-norm2|={abs(np.trace(rho0[k]).real - n2r):.3e} |dnorm2|={abs(n20[k] - n2r):.3e} tol={tol:.3e}")
        assert np.max(np.abs(ref)) > 1e3 * tol
        assert np.max(np.abs(rho0[k] - ref)) <= tol
        assert abs(np.trace(rho0[k]).real - n2r) <= tol and abs(n20[k] - n2r) <= tol
        assert np.array_equal(rho0[k], rho0[k].conj().T)                            # exactly Hermitian
    for _, r, _ in res:
        assert r["rho2"].shape == (2, D, D) and r["rho2"].dtype == (np.complex128 if cplx else np.float64)
        assert np.array_equal(r["rho2"], rho0) and np.array_equal(r["n2"], n20)    # the same bits on every rank
        assert np.array_equal(r["rho2"], r["rho2_again"]) and np.array_equal(r["n2"], r["n2_again"])   # and call
        for k in range(2):                                                          # nvec = 2 is two single calls
            rk, nk = r["single"][k]
            assert rk.shape == (1, D, D) and np.array_equal(rk[0], r["rho2"][k]) and nk[0] == r["n2"][k]
        assert np.array_equal(r["rho2_dev"], r["rho2"]) and np.array_equal(r["n2_dev"], r["n2"])    # host = device pointer
        assert r["src_untouched"] and r["dev_untouched"]
        if world == 1:
            assert np.array_equal(r["whole"][0], r["rho2"]) and np.array_equal(r["whole"][1], r["n2"])


# ---------------------------------------------------------------------------------------------------------
# refusals: one world of 2; every rank is refused alike before any collective, and a served call still runs after
# ---------------------------------------------------------------------------------------------------------
def _refusal_rank_main(rank, world, name, q):
    try:
        import re
        import torch  # noqa: F401
        from edipack_amd import capi
        from edipack_amd.hamiltonian import SectorHamiltonian as H
        from edipack_amd.sharding import LibraryComm, library_sharded_sector
        from tests.common import make_models
        capi.init(0)
        comm = LibraryComm(rank, world, shm_name=name, slot_bytes=1 << 22)
        buf = np.random.default_rng(3).standard_normal(8192)
        seen = []

        def refused(what, match, call):
            try:
                call()
            except capi.EdigpuError as e:
                assert re.search(match, str(e)), (what, str(e))
                seen.append(what)
                return
            raise AssertionError(what + ": not refused")

        # a superc row shard
        _, ps = make_models("superc", "hybrid", 2, 3, seed=12)
        h, first, count = library_sharded_sector(ps, 0, comm)
        refused("superc shard", "edigpu_imp_rdm_sharded: only ed_mode=normal sectors are supported",
                lambda: comm.imp_rdm(h, buf[:2 * count].view(np.complex128)))
        h.destroy()
        # ed_total_ud=F
        om, pm = make_models("normal", "normal", 2, 2, seed=11, jxp=0.0)
        hl = np.zeros_like(om.hloc)
        for a in range(2):
            hl[0, 0, a, a] = om.hloc[0, 0, a, a].real
        pm.hloc = hl
        h = H.orbs_from_model(pm, (2, 1), (1, 2))
        refused("ed_total_ud=F", "edigpu_imp_rdm_sharded: ed_total_ud=F sectors are not supported", lambda: comm.imp_rdm(h, buf))
        h.destroy()
        # a hand-over shard
        ho, pn, v = _reference("normal", "normal", 2, 3, (4, 4))
        f, c, _ = comm.plan(ho.dimdw)
        h = H.normal_from_arrays(ho.dimup, ho.dimdw, ho.hd[f * ho.dimup:(f + c) * ho.dimup], ho.up, ho.dw, None, dw_first=f,
                                 dw_count=c)
        refused("hand-over", "edigpu_imp_rdm_sharded: .*must be built from a model", lambda: comm.imp_rdm(h, buf[:c * ho.dimup]))
        h.destroy()
        # nvec = 0, then the same handle is served: no rank was left waiting in a collective
        h, f, c = library_sharded_sector(pn, (4, 4), comm)
        vs = v[f * ho.dimup:(f + c) * ho.dimup]
        refused("nvec = 0", "edigpu_imp_rdm_sharded: nvec must be positive", lambda: comm.imp_rdm(h, vs, 0))
        rho, n2 = comm.imp_rdm(h, vs)
        h.destroy()
        comm.destroy()
        q.put((rank, seen, rho, n2, None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, None, None, traceback.format_exc() + str(e)))


def test_refusals_on_shards(gpu):
    res = _run_world(_refusal_rank_main, 2, (f"edigpu_rdm_refuse_{os.getpid()}",))
    ho, pm, v = _reference("normal", "normal", 2, 3, (4, 4))
    mu, md = sector_maps(pm, (4, 4))
    ref, n2r = ref_rdm(mu, md, 2, v)
    for _, seen, rho, n2, _ in res:
        assert seen == ["superc shard", "ed_total_ud=F", "hand-over", "nvec = 0"]
        assert np.max(np.abs(rho[0] - ref)) <= 4 * v.size * U * n2r and abs(n2[0] - n2r) <= 4 * v.size * U * n2r
        assert np.array_equal(rho, res[0][2])
