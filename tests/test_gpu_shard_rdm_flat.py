"""GPU tests of the impurity reduced density matrix on sharded superc / nonsu2 vectors (edigpu_imp_rdm_flat_sharded through
LibraryComm.imp_rdm_flat): spawned ranks share the one GPU over the shared-memory transport, through the world runner of
tests/test_gpu_library_shards.py.

The reference is ref_rdm_flat of tests/rdm_flat_cases.py (numpy in extended precision) with that file's derived bound
4 dim u norm2, dim the dimension of the WHOLE sector, phonon blocks included: an entry is still one sum of at most dim
rounded products, taken in another order (workgroups, then the interior slabs and the tail slab, then the ranks).  What
every (case, world) cuts is computed from the sector map and compared with edigpu_imp_rdm_flat_sharded_info on every rank.
Every check of a case runs in one rank function, so a case costs one spawn per world."""
import os

import numpy as np
import pytest

from tests.rdm_flat_cases import U, blocks_mask, flat_map, flat_model, random_vector, ref_rdm_flat
from tests.test_gpu_library_shards import CASES, NPH, _run_world

pytestmark = pytest.mark.gpu

assert CASES[7][:5] == ("superc", "hybrid", 2, 2, 0) and CASES[7][6] == "phonon" and not CASES[7][5]
assert CASES[8][:5] == ("nonsu2", "normal", 2, 2, 4) and CASES[8][6] == "phonon" and CASES[8][5]
SC23 = ("superc", "hybrid", 2, 3, 0, 12, False, False)
# (mode, bath, norb, nbath, sector, seed of make_models, on the fly, phonon), world, dim_el, heads or None, both handles
WORLDS = [
    (SC23, 1, 252, [0], False),
    (SC23, 2, 252, [0, 0], False),                       # no slab is cut: H = 0, no all-gather
    (SC23, 3, 252, [0, 7, 28], True),                    # cuts [56, 91) at 84 and [161, 196) at 168
    (SC23, 5, 252, [0, 5, 24, 8, 27], False),
    (("superc", "hybrid", 2, 3, 3, 12, False, False), 10, 45, None, False),     # [0, 21) spans ranks 0-4, rank 9 passes NULL
    (("nonsu2", "hybrid", 2, 3, 5, 13, True, False), 3, None, None, False),
    (("nonsu2", "hybrid", 3, 3, 6, 13, False, False), 3, 924, [0, 28, 98], False),
    (("nonsu2", "hybrid", 3, 3, 6, 13, False, False), 10, 924, [0, 93, 24, 57, 90, 93, 30, 63, 93, 3], False),
    (("nonsu2", "hybrid", 4, 2, 6, 13, False, False), 3, 924, [0, 154, 98], False),
    (("superc", "hybrid", 2, 2, 0, 12, False, True), 3, 70, [0, 11, 7], False),            # NPH = 3: the halo carries 4 blocks
    (("nonsu2", "normal", 2, 2, 4, 13, True, True), 2, 495, [0, 18], False),
    (("nonsu2", "normal", 3, 2, 9, 13, True, False), 3, 48620, [0, 876, 47], False),       # many workgroups per panel
]


def _model(case):
    mode, bath, norb, nbath, sec, seed, direct, phonon = case
    pm = flat_model(mode, bath, norb, nbath, seed)
    if phonon:
        pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = NPH, 0.8, 0.15, np.diag([0.4, -0.3][:norb])
    return pm


def _electronic_map(case):
    mode, bath, norb, nbath, sec, seed, _, _ = case
    pm = flat_model(mode, bath, norb, nbath, seed)
    return np.asarray(flat_map(pm, sec)), pm.ns


def _geometry(mp, ns, norb, world, nblk, cw):
    """per rank what edigpu_imp_rdm_flat_sharded_info must return, from the sector map alone, and the heads"""
    n = mp.size
    bdw = (mp.astype(np.int64) >> ns) >> norb
    starts = [0] + [i for i in range(1, n) if bdw[i] != bdw[i - 1]] + [n]
    slabs = list(zip(starts, starts[1:]))
    q = -(-n // world)
    rng = [(min(r * q, n), max(0, min(q, n - min(r * q, n)))) for r in range(world)]
    heads = []
    for f, c in rng:
        inside = [s for s, _ in slabs if f <= s < f + c]
        heads.append(inside[0] - f if inside else c)
    H = max(heads)
    infos = []
    for f, c in rng:
        walked = sum(1 for s, e in slabs if f <= s and e <= f + c and c > 0)
        tail = [(s, e) for s, e in slabs if f <= s < f + c < e]
        assert len(tail) <= 1
        t = (tail[0][0] - f, tail[0][1] - tail[0][0], f + c - tail[0][0]) if tail else (-1, 0, 0)
        infos.append([H, H * nblk * cw, walked, *t])
    return infos, heads, rng


def _vectors(dim, cplx):
    """the two vectors of a case: seeded, so every rank and the test make the same ones"""
    return np.stack([random_vector(dim, cplx, 17), random_vector(dim, cplx, 91)])


def _shard_index(first, count, dim_el, nblk):
    base = np.arange(first, first + count)
    return np.concatenate([b * dim_el + base for b in range(nblk)])


def _case_rank_main(rank, world, name, case, both, q):
    try:
        import torch
        from edipack_amd import capi
        from edipack_amd.sharding import LibraryComm, library_sharded_sector
        capi.init(0)
        mode, bath, norb, nbath, sec, seed, direct, phonon = case
        pm = _model(case)
        comm = LibraryComm(rank, world, shm_name=name, slot_bytes=1 << 22)
        h, first, count = library_sharded_sector(pm, sec, comm, direct=direct)
        nblk = NPH + 1 if phonon else 1
        dim_el = h.dim // nblk
        ix = _shard_index(first, count, dim_el, nblk)
        vs2 = np.ascontiguousarray(_vectors(h.dim, h.is_complex)[:, ix])
        keep = vs2.copy()
        r = dict(n=ix.size, cplx=h.is_complex, dim=h.dim, first=first, count=count)
        r["info"] = comm.imp_rdm_flat_info(h)
        r["rho2"], r["n2"] = comm.imp_rdm_flat(h, vs2, 2)
        r["rho2_again"], r["n2_again"] = comm.imp_rdm_flat(h, vs2, 2)
        r["single"] = [comm.imp_rdm_flat(h, vs2[k]) for k in range(2)]
        r["src_untouched"] = np.array_equal(vs2, keep)
        t = torch.from_numpy(vs2).cuda()
        torch.cuda.synchronize()
        r["rho2_dev"], r["n2_dev"] = comm.imp_rdm_flat(h, t.data_ptr() if ix.size else 0, 2)
        r["dev_untouched"] = np.array_equal(t.cpu().numpy(), keep)
        if world == 1:                                   # the whole sector on one rank: the bits of edigpu_imp_rdm_flat
            r["whole"] = h.imp_rdm_flat(t.data_ptr(), 2)
        if both:                                         # the other kind of shard handle: the same bits
            h2, f2, c2 = library_sharded_sector(pm, sec, comm, direct=not direct)
            assert (f2, c2) == (first, count) and h2.is_complex == h.is_complex
            r["other"] = comm.imp_rdm_flat(h2, vs2, 2)
            h2.destroy()
        h.destroy()
        comm.destroy()
        q.put((rank, r, None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, traceback.format_exc() + str(e)))


def _id(w):
    c = w[0]
    return f"w{w[1]}-{c[0]}-{c[1]}{c[2]}x{c[3]}-{c[4]}{'-direct' if c[6] else ''}{'-phonon' if c[7] else ''}"


@pytest.mark.parametrize("case,world,dim_el,heads,both", WORLDS, ids=[_id(w) for w in WORLDS])
def test_imp_rdm_flat_on_shards(gpu, case, world, dim_el, heads, both):
    mode, bath, norb, nbath, sec, seed, direct, phonon = case
    mp, ns = _electronic_map(case)
    nblk = NPH + 1 if phonon else 1
    assert dim_el is None or mp.size == dim_el
    res = _run_world(_case_rank_main, world, (f"edigpu_rdmf_{os.getpid()}_{world}_{abs(hash(case)) % 100000}", case, both))
    cplx, dim = res[0][1]["cplx"], res[0][1]["dim"]
    assert dim == mp.size * nblk and sum(r["n"] for _, r, _ in res) == dim
    infos, hd, rng = _geometry(mp, ns, norb, world, nblk, 2 if cplx else 1)
    assert heads is None or hd == heads, hd
    for (rank, r, _), want, (f, c) in zip(res, infos, rng):
        assert (r["first"], r["count"]) == (f, c)
        assert list(r["info"].values()) == want, (rank, r["info"], want)
    if case[4] == 3 and mode == "superc":
        assert res[9][1]["n"] == 0 and hd[:5] == [0, 5, 5, 5, 1]                       # a rank that passes NULL
    if dim_el == 48620:
        assert [(f + i[3], f + i[3] + i[4]) for i, (f, _) in zip(infos, rng) if i[4]] == [(16159, 17083), (31537, 32461)]
    if mode == "nonsu2" and norb == 3 and sec == 6:
        assert cplx
    D = 4 ** norb
    v2 = _vectors(dim, cplx)
    rho0, n20 = res[0][1]["rho2"], res[0][1]["n2"]
    outside = ~blocks_mask(mode, norb)
    for k in range(2):
        ref, n2r = ref_rdm_flat(mp, ns, norb, v2[k], nblk)
        tol = 4 * dim * U * n2r
        print(f"imp_rdm_flat on {world} shards, vector {k}: dim={dim} max|drho|={np.max(np.abs(rho0[k] - ref)):.3e} "
              f"|trace-norm2|={abs(np.trace(rho0[k]).real - n2r):.3e} |dnorm2|={abs(n20[k] - n2r):.3e} tol={tol:.3e}")
        assert np.max(np.abs(ref)) > 1e3 * tol
        assert np.max(np.abs(rho0[k] - ref)) <= tol
        assert abs(np.trace(rho0[k]).real - n2r) <= tol and abs(n20[k] - n2r) <= tol
        assert np.array_equal(rho0[k], rho0[k].conj().T)                            # exactly Hermitian
        assert np.count_nonzero(rho0[k][outside]) == 0
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
        if both:
            assert np.array_equal(r["other"][0], r["rho2"]) and np.array_equal(r["other"][1], r["n2"])


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
        from tests.common import make_jz_models, make_models
        capi.init(0)
        comm = LibraryComm(rank, world, shm_name=name, slot_bytes=1 << 22)
        buf = np.random.default_rng(3).standard_normal(8192)
        seen = []

        def refused(what, match, h, v, nvec=1):
            calls = [lambda: comm.imp_rdm_flat(h, v, nvec)] + ([lambda: comm.imp_rdm_flat_info(h)] if nvec == 1 else [])
            for call in calls:                             # _info runs the same checks
                try:
                    call()
                except capi.EdigpuError as e:
                    assert re.search(match, str(e)), (what, str(e))
                    continue
                raise AssertionError(what + ": not refused")
            seen.append(what)

        who = "edigpu_imp_rdm_flat_sharded(_info)?: "
        # a normal-mode down-row shard
        _, pn = make_models("normal", "normal", 2, 3, seed=31)
        h, f, c = library_sharded_sector(pn, (4, 4), comm, exchange="allgather")
        refused("normal mode", who + "normal-mode sectors are not served here, use edigpu_imp_rdm_sharded", h, buf)
        h.destroy()
        # Jz_basis
        _, pj = make_jz_models(1)
        h = H.flat_jz_from_model(pj, 3, 1)
        refused("Jz_basis", who + "Jz_basis sectors are not supported", h, buf)
        h.destroy()
        # five orbitals
        p5 = flat_model("nonsu2", "hybrid", 5, 1, 13)
        h, f, c = library_sharded_sector(p5, 2, comm)
        refused("Norb = 5", who + "Norb = 5 is not supported", h, buf)
        h.destroy()
        # a handle that is not this rank's range of the communicator
        ps = flat_model("superc", "hybrid", 2, 3, 12)
        h = H.flat_from_model(ps, 0, row_first=2, row_count=5)
        refused("another range", "the handle does not hold this rank's shard", h, buf)
        h.destroy()
        h = H.flat_from_model(ps, 0)                       # the whole sector in a world of two
        refused("whole sector", "the handle does not hold this rank's shard", h, buf)
        h.destroy()
        # a hand-over handle: this rank's four rows of a diagonal matrix
        h = H.csr_from_arrays(np.arange(5), np.arange(4) + 4 * rank, np.ones(4), ncol_global=8, row_first=4 * rank)
        refused("hand-over", who + ".*must be built from a model", h, buf[:4])
        h.destroy()
        # nvec = 0, then the same handle is served: no rank was left waiting in a collective
        h, f, c = library_sharded_sector(ps, 0, comm)
        v = random_vector(252, h.is_complex, 17)
        refused("nvec = 0", "edigpu_imp_rdm_flat_sharded: nvec must be positive", h, v[f:f + c], nvec=0)
        rho, n2 = comm.imp_rdm_flat(h, v[f:f + c])
        h.destroy()
        comm.destroy()
        q.put((rank, seen, rho, n2, None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, None, None, traceback.format_exc() + str(e)))


def test_refusals_on_shards(gpu):
    res = _run_world(_refusal_rank_main, 2, (f"edigpu_rdmf_refuse_{os.getpid()}",))
    mp, ns = _electronic_map(SC23)
    cplx = np.iscomplexobj(res[0][2])
    v = random_vector(252, cplx, 17)
    ref, n2r = ref_rdm_flat(mp, ns, 2, v)
    for _, seen, rho, n2, _ in res:
        assert seen == ["normal mode", "Jz_basis", "Norb = 5", "another range", "whole sector", "hand-over", "nvec = 0"]
        assert np.max(np.abs(rho[0] - ref)) <= 4 * v.size * U * n2r and abs(n2[0] - n2r) <= 4 * v.size * U * n2r
        assert np.array_equal(rho, res[0][2])


# ---------------------------------------------------------------------------------------------------------
# end to end: the golden phisc of a superc directory from an eigenvector that is born and measured on two shards
# ---------------------------------------------------------------------------------------------------------
def _golden_rank_main(rank, world, name, q):
    try:
        import torch  # noqa: F401
        from edipack_amd import capi
        from edipack_amd.sharding import LibraryComm, library_sharded_sector
        from oracle import oracle as O
        from tests.common import replica_golden_models
        from tests.test_oracle_golden import GOLD, REPLICA_DIRS
        capi.init(0)
        assert "GENERAL_SUPERC" in REPLICA_DIRS
        om, pm = replica_golden_models(GOLD["GENERAL_SUPERC"]["input"])
        O.to_struct(om)
        comm = LibraryComm(rank, world, shm_name=name, slot_bytes=1 << 22)
        h, first, count = library_sharded_sector(pm, 0, comm)
        v0 = random_vector(h.dim, h.is_complex, 5)[first:first + count]
        e, x, nmv = comm.eigh(h, count, v0_shard=v0, nitermax=300, tol=1e-13)
        rhos, n2 = comm.imp_rdm_flat(h, x)                 # the eigenvector never leaves its shards
        info = comm.imp_rdm_flat_info(h)
        h.destroy()
        comm.destroy()
        q.put((rank, e, rhos, n2, info, om.norb, None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, None, None, None, 0, traceback.format_exc() + str(e)))


def test_golden_phisc_from_an_eigenvector_on_two_shards(gpu):
    """the fixture and the tolerances of tests/test_gpu_rdm_flat.py::test_golden_phisc_from_a_device_eigenvector"""
    from edipack_amd.observables import rdm_anomalous, rdm_average, rdm_occupations
    from tests.test_oracle_golden import GOLD
    g = GOLD["GENERAL_SUPERC"]
    res = _run_world(_golden_rank_main, 2, (f"edigpu_rdmf_gold_{os.getpid()}",))
    for _, e, rhos, n2, info, norb, _ in res:
        assert abs(e - g["evals"][0]) < 1e-9     # the ground state of the fixture lies in this sector, alone
        assert np.array_equal(rhos, res[0][2]) and np.array_equal(n2, res[0][3])
        rho = rdm_average(rhos, n2)
        up, dw, docc = rdm_occupations(rho, norb)
        phi = rdm_anomalous(rho, norb).flatten(order="F")      # Fortran element order, as the fixture
        print(f"max |dens - check| = {np.max(np.abs(up + dw - np.array(g['dens']))):.3e} "
              f"|docc| {np.max(np.abs(docc - np.array(g['docc']))):.3e} |phisc| {np.max(np.abs(phi.real - np.array(g['phisc']))):.3e} "
              f"halo {info['H']}")
        assert np.max(np.abs(up + dw - np.array(g["dens"]))) < 1e-8 and np.max(np.abs(docc - np.array(g["docc"]))) < 1e-8
        assert np.max(np.abs(np.array(g["phisc"]))) > 1e-2
        assert np.max(np.abs(phi.real - np.array(g["phisc"]))) < 1e-8 and np.max(np.abs(phi.imag)) < 1e-8
