"""GPU tests of the occupation and phonon observables on sharded vectors (csrc/edigpu_shard_obs.hip through
LibraryComm.occ_moments / apply_occ / apply_n / apply_sz / apply_xph / ph_rdm): spawned ranks share the one GPU over the
shared-memory transport, as in tests/test_gpu_library_shards.py, whose cases, references and world runner are reused.

References and tolerances are those of the single-GPU tests: the extended-precision numpy moments of
tests/test_gpu_occupations.py with its bound 2 dim u norm2 -- dim the dimension of the WHOLE sector: a moment is still one
sum of dim rounded non-negative terms, taken in another order (per rank, then over the ranks) -- and ref_ph_rdm / ref_xph
of tests/ph_cases.py with (4 if complex else 2) dim_el u norm2.  The N_a, Sz_a and b + b+ products are bit-equal to numpy.
Every check of a case runs in one rank function, so a case costs one spawn per world."""
import os

import numpy as np
import pytest

from tests.ph_cases import flat_classes, normal_classes, ref_ph_rdm, ref_xph, set_phonons
from tests.test_gpu_library_shards import CASES, NPH, _block_env, _reference, _run_world, _shard_index
from tests.test_gpu_occupations import U, flat_bits, normal_bits, ref_moments

pytestmark = pytest.mark.gpu

# normal-normal auto (kind 1), normal-hybrid 3x3 (15 rows over 8 + 7), all-gather form, stored superc, on-the-fly nonsu2,
# cmplx, normal-hybrid 3x5 (4,3) on padded panels (kind 2), the three phonon cases
OBS_CASES = [CASES[k] for k in (0, 1, 2, 3, 4, 5, 10, 6, 7, 8)]
assert OBS_CASES[6][:5] == ("normal", "hybrid", 3, 5, (4, 3)) and OBS_CASES[6][6] == "block"
assert [c[6] for c in OBS_CASES[7:]] == ["phonon"] * 3
WORLDS = [(w, c) for c in OBS_CASES for w in (1, 2, 3) if w > 1 or c is OBS_CASES[0] or c is OBS_CASES[7]]


def _case_id(c):
    return f"{c[0]}-{c[1]}{c[2]}x{c[3]}-{c[6]}{'-direct' if c[5] else ''}"


def _flags(case):
    return dict(cmplx=case[6] == "cmplx", phonon=case[6] == "phonon")


def _open(rank, world, name, case):
    """capi initialised, the case's reference, communicator, this rank's handle and the indices of its shard"""
    import torch  # noqa: F401  (one HIP runtime per process)
    from edipack_amd import capi
    from edipack_amd.sharding import LibraryComm, library_sharded_sector
    capi.init(0)
    mode, bath, norb, nbath, sector, direct, exchange = case
    ho, pm, v = _reference(mode, bath, norb, nbath, sector, **_flags(case))
    comm = LibraryComm(rank, world, shm_name=name, slot_bytes=1 << 22)
    block = exchange.startswith("block")
    _block_env(block)
    h, first, count = library_sharded_sector(pm, sector, comm, direct=direct, exchange="auto" if block else exchange,
                                             cmplx=exchange == "cmplx")
    info = comm.shard_info(h)
    assert not block or info[0] == 2, info
    assert not (exchange == "auto" and mode == "normal") or info[0] == 1, info
    ix = _shard_index(ho, mode, first, count, exchange == "phonon")
    return comm, h, pm, np.ascontiguousarray(v[ix]), ix


def _weights(norb):
    rng = np.random.default_rng(77)
    return rng.standard_normal(norb), rng.standard_normal(norb)


def _case_rank_main(rank, world, name, case, q):
    try:
        comm, h, pm, vs, ix = _open(rank, world, name, case)
        norb, keep = case[2], vs.copy()
        r = dict(ix=ix)
        r["M"], r["n2"] = comm.occ_moments(h, vs)
        r["M_again"], r["n2_again"] = comm.occ_moments(h, vs)
        r["n"] = [comm.apply_n(h, vs, a) for a in range(norb)]
        r["sz"] = [comm.apply_sz(h, vs, a) for a in range(norb)]
        r["w"] = comm.apply_occ(h, vs, *_weights(norb))
        if case[6] == "phonon":
            r["xph"] = comm.apply_xph(h, vs)
            r["rho"], r["rho_n2"] = comm.ph_rdm(h, vs)
            r["rho_again"], _ = comm.ph_rdm(h, vs)
        r["src_untouched"] = np.array_equal(vs, keep)
        h.destroy()
        comm.destroy()
        q.put((rank, r, None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, traceback.format_exc() + str(e)))


def _bits(case, pm):
    from edipack_amd.hamiltonian import sector_map
    mode, sector = case[0], case[4]
    nblk = NPH + 1 if case[6] == "phonon" else 1
    if mode == "normal":
        return normal_bits(pm, *sector, nblk=nblk)
    return flat_bits(pm, sector_map(pm, sector), nblk=nblk)


def _assemble(res, key, v, k=None):
    got = np.full_like(v, np.nan)
    for _, r, _ in res:
        got[r["ix"]] = r[key] if k is None else r[key][k]
    return got


def _check_moments(res, nu, nd, v, key="M", key2="n2"):
    Mr, n2r = ref_moments(nu, nd, v)
    tol = 2 * v.size * U * n2r
    M0, n20 = res[0][1][key], res[0][1][key2]
    print(f"occ_moments on {len(res)} shards dim={v.size} max|dM|={np.max(np.abs(M0[0] - Mr)):.3e} "
          f"|dnorm2|={abs(n20[0] - n2r):.3e} tol={tol:.3e}")
    for _, r, _ in res:
        M, n2 = r[key], r[key2]
        assert M.shape == (1, 2 * nu.shape[0], 2 * nu.shape[0])
        assert np.max(np.abs(M[0] - Mr)) <= tol and abs(n2[0] - n2r) <= tol
        assert np.array_equal(M[0], M[0].T)
        assert np.array_equal(M, M0) and np.array_equal(n2, n20)            # the same bits on every rank
    return tol, n2r


@pytest.mark.parametrize("world,case", WORLDS, ids=[f"w{w}-{_case_id(c)}" for w, c in WORLDS])
def test_observables_on_shards(gpu, world, case):
    mode, bath, norb, nbath, sector, direct, exchange = case
    ho, pm, v = _reference(mode, bath, norb, nbath, sector, **_flags(case))
    name = f"edigpu_obs_{os.getpid()}_{world}_{abs(hash(case)) % 100000}"
    res = _run_world(_case_rank_main, world, (name, case))
    nu, nd = _bits(case, pm)
    assert nu.shape[1] == v.size and sum(r["ix"].size for _, r, _ in res) == v.size
    # ---- moments: tolerance, symmetry, the same bits on every rank and on a second call
    _check_moments(res, nu, nd, v)
    for _, r, _ in res:
        assert np.array_equal(r["M"], r["M_again"]) and np.array_equal(r["n2"], r["n2_again"])
        assert r["src_untouched"]
    # ---- N_a, Sz_a bit-equal; random weights inside the bound of two rounded table sums, their sum and the product
    for a in range(norb):
        assert np.array_equal(_assemble(res, "n", v, a), (nu[a] + nd[a]).astype(np.float64) * v)
        assert np.array_equal(_assemble(res, "sz", v, a), ((nu[a] - nd[a]) * 0.5) * v)
    wu, wd = _weights(norb)
    exact = (wu.astype(np.longdouble) @ nu + wd.astype(np.longdouble) @ nd) * v
    bound = 4 * U * (np.abs(wu).sum() + np.abs(wd).sum()) * np.abs(v)
    assert np.all(np.abs(_assemble(res, "w", v) - exact) <= bound)
    if exchange != "phonon":
        return
    # ---- phonon seed bit-equal on the assembled vector; density matrix: tolerance, Hermitian per class, trace, bits
    from edipack_amd.hamiltonian import sector_map
    dimph, ncls = NPH + 1, 3 ** norb
    assert np.array_equal(_assemble(res, "xph", v), ref_xph(v, dimph))
    cls = normal_classes(pm, *sector) if mode == "normal" else flat_classes(pm, sector_map(pm, sector))
    assert cls.size * dimph == v.size
    cplx = np.iscomplexobj(v)
    ref = ref_ph_rdm(cls, v, dimph, ncls)
    n2r = float(np.sum(np.abs(v.astype(np.clongdouble if cplx else np.longdouble)) ** 2))
    tol = (4 if cplx else 2) * cls.size * U * n2r
    rho0, rn0 = res[0][1]["rho"], res[0][1]["rho_n2"]
    print(f"ph_rdm on {world} shards dim_el={cls.size} max|drho|={np.max(np.abs(rho0[0] - ref)):.3e} "
          f"|dnorm2|={abs(rn0[0] - n2r):.3e} tol={tol:.3e}")
    for _, r, _ in res:
        rho, rn = r["rho"], r["rho_n2"]
        assert rho.shape == (1, ncls, dimph, dimph) and rho.dtype == (np.complex128 if cplx else np.float64)
        assert np.max(np.abs(rho[0] - ref)) <= tol
        assert all(np.array_equal(rho[0, c], rho[0, c].conj().T) for c in range(ncls))
        assert abs(rn[0] - n2r) <= tol
        assert abs(rn[0] - np.real(np.trace(rho[0], axis1=1, axis2=2)).sum()) <= tol
        assert np.array_equal(rho, rho0) and np.array_equal(rn, rn0) and np.array_equal(rho, r["rho_again"])


# ---------------------------------------------------------------------------------------------------------
# ranks without rows: DimDw = 8 over 10 ranks (the geometry of test_library_shards_wide_worlds)
# ---------------------------------------------------------------------------------------------------------
EMPTY_CASE = ("normal", "normal", 2, 3, (4, 1), False, "block")


def _empty_rank_main(rank, world, name, case, q):
    try:
        comm, h, pm, vs, ix = _open(rank, world, name, case)
        r = dict(ix=ix)
        r["M"], r["n2"] = comm.occ_moments(h, vs)
        r["n"] = [comm.apply_n(h, vs, a) for a in range(case[2])]
        h.destroy()
        comm.destroy()
        q.put((rank, r, None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, traceback.format_exc() + str(e)))


def test_ranks_without_rows_return_the_full_sums(gpu):
    mode, bath, norb, nbath, sector, direct, exchange = EMPTY_CASE
    ho, pm, v = _reference(mode, bath, norb, nbath, sector)
    res = _run_world(_empty_rank_main, 10, (f"edigpu_obs_empty_{os.getpid()}", EMPTY_CASE))
    assert [r["ix"].size for _, r, _ in res][8:] == [0, 0] and all(r["ix"].size > 0 for _, r, _ in res[:8])
    nu, nd = _bits(EMPTY_CASE, pm)
    _check_moments(res, nu, nd, v)
    assert all(x.size == 0 for _, r, _ in res[8:] for x in r["n"])
    for a in range(norb):
        assert np.array_equal(_assemble(res, "n", v, a), (nu[a] + nd[a]).astype(np.float64) * v)


# ---------------------------------------------------------------------------------------------------------
# device pointers, several vectors and the chain eigenvector shards -> moments: one world of 2 on the first case
# ---------------------------------------------------------------------------------------------------------
def _extras_rank_main(rank, world, name, case, q):
    try:
        import torch
        comm, h, pm, vs, ix = _open(rank, world, name, case)
        r = dict(ix=ix)
        # device pointers: the moments of the uploaded shard, N_0 in place on it
        r["M_host"], r["n2_host"] = comm.occ_moments(h, vs)
        t = torch.from_numpy(vs).cuda()
        torch.cuda.synchronize()
        r["M_dev"], r["n2_dev"] = comm.occ_moments(h, t.data_ptr())
        r["dev_untouched"] = np.array_equal(t.cpu().numpy(), vs)
        r["n0_host"] = comm.apply_n(h, vs, 0)
        assert comm.apply_n(h, t.data_ptr(), 0) is None
        r["n0_dev"] = t.cpu().numpy()
        # several vectors: consecutive shards with stride nloc
        vs3 = np.stack([vs, np.random.default_rng(5).standard_normal(vs.size), vs[::-1]])
        r["vs3"] = vs3
        r["M3"], r["n23"] = comm.occ_moments(h, vs3, 3)
        r["M1"] = [comm.occ_moments(h, vs3[k]) for k in range(3)]
        t3 = torch.from_numpy(vs3).cuda()
        torch.cuda.synchronize()
        r["M3_dev"], _ = comm.occ_moments(h, t3.data_ptr(), 3)
        # chain: the lowest eigenvector as shards -> moments
        e, x, _ = comm.eigh(h, vs.size, v0_shard=vs, tol=1e-11)
        r["e"], r["x"] = e, x
        r["M_eig"], r["n2_eig"] = comm.occ_moments(h, x)
        h.destroy()
        comm.destroy()
        q.put((rank, r, None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, traceback.format_exc() + str(e)))


@pytest.fixture(scope="module")
def extras(gpu):
    return _run_world(_extras_rank_main, 2, (f"edigpu_obs_extras_{os.getpid()}", CASES[0]))


def test_device_pointers_give_the_bits_of_host_arrays(gpu, extras):
    for _, r, _ in extras:
        assert np.array_equal(r["M_dev"], r["M_host"]) and np.array_equal(r["n2_dev"], r["n2_host"])
        assert r["dev_untouched"]
        assert np.array_equal(r["n0_dev"], r["n0_host"]) and np.any(r["n0_host"] != 0.0)
    mode, bath, norb, nbath, sector, _, _ = CASES[0]
    _, pm, v = _reference(mode, bath, norb, nbath, sector)
    nu, nd = normal_bits(pm, *sector)
    assert np.array_equal(_assemble(extras, "n0_dev", v), (nu[0] + nd[0]).astype(np.float64) * v)


def test_several_vectors_equal_single_calls_bit_for_bit(gpu, extras):
    mode, bath, norb, nbath, sector, _, _ = CASES[0]
    _, pm, v = _reference(mode, bath, norb, nbath, sector)
    nu, nd = normal_bits(pm, *sector)
    for _, r, _ in extras:
        assert r["M3"].shape == (3, 4, 4) and np.array_equal(r["M3"], r["M3_dev"])
        for k in range(3):
            Mk, nk = r["M1"][k]
            assert np.array_equal(r["M3"][k], Mk[0]) and r["n23"][k] == nk[0]
        assert np.array_equal(r["M3"], extras[0][1]["M3"])
    for k in range(3):
        vk = np.zeros_like(v)
        for _, r, _ in extras:
            vk[r["ix"]] = r["vs3"][k]
        Mr, n2r = ref_moments(nu, nd, vk)
        assert np.max(np.abs(extras[0][1]["M3"][k] - Mr)) <= 2 * v.size * U * n2r


def test_chain_eigenvector_shards_to_moments(gpu, extras):
    """comm.eigh -> comm.occ_moments on the returned shards against the single-GPU path of the same sector.  The two
    eigenvectors agree to the solvers' tol = 1e-11 only, so the bound, 1e-9 norm2, is the eigenvector's, not the
    reduction's."""
    import ctypes as C
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian
    mode, bath, norb, nbath, sector, _, _ = CASES[0]
    _, pm, _ = _reference(mode, bath, norb, nbath, sector)
    h = SectorHamiltonian.normal_from_model(pm, *sector)
    evec = torch.empty(h.dim, dtype=torch.float64, device="cuda")
    ev, nc, nmv = np.zeros(1), C.c_int(0), C.c_int(0)
    capi.check(capi.lib().edigpu_lanczos_eigh_multi(h._h, 1, 0, 1e-11, 300, None, capi.pd(ev), C.c_void_p(evec.data_ptr()),
                                                    C.byref(nc), C.byref(nmv)), "edigpu_lanczos_eigh_multi")
    M, n2 = h.occ_moments(evec.data_ptr())
    h.destroy()
    for _, r, _ in extras:
        assert abs(r["e"] - ev[0]) < 1e-9 * max(1.0, abs(ev[0]))
        print(f"chain: max|dM|={np.max(np.abs(r['M_eig'][0] - M[0])):.3e} norm2={r['n2_eig'][0]!r} / {n2[0]!r}")
        assert np.max(np.abs(r["M_eig"][0] - M[0])) <= 1e-9 * n2[0] and abs(r["n2_eig"][0] - n2[0]) <= 1e-9 * n2[0]
        assert np.array_equal(r["M_eig"], extras[0][1]["M_eig"])


# ---------------------------------------------------------------------------------------------------------
# the reference's fixtures from shards of the oracle's ground states
# ---------------------------------------------------------------------------------------------------------
def _golden_models(name):
    from oracle import oracle as O
    from tests.common import replica_golden_models
    from tests.test_oracle_golden import GOLD, REPLICA_DIRS, _from_dir, golden_models
    g = GOLD[name]
    if name in REPLICA_DIRS:
        om, pm = replica_golden_models(g["input"])
    else:
        inp, par = _from_dir(name)
        pm_par = {k: v for k, v in par.items() if k not in ("ed_hw_bath", "deltasc")}
        om, pm = golden_models(inp["ED_MODE"], inp["BATH_TYPE"], int(inp["NORB"]), int(inp["NBATH"]), pm_par)
    O.to_struct(om)
    return om, pm, g


def _golden_rank_main(rank, world, name, fixture, states, q):
    try:
        import torch  # noqa: F401
        from edipack_amd import capi
        from edipack_amd.sharding import LibraryComm, library_sharded_sector
        capi.init(0)
        om, pm, _ = _golden_models(fixture)
        comm = LibraryComm(rank, world, shm_name=name, slot_bytes=1 << 22)
        Ms, norms = [], []
        for sec, v in states:
            h, first, count = library_sharded_sector(pm, sec, comm)
            ul = h.dim_up if om.ed_mode == "normal" else 1
            M, n2 = comm.occ_moments(h, v[first * ul:(first + count) * ul])
            Ms.append(M[0])
            norms.append(n2[0])
            h.destroy()
        comm.destroy()
        q.put((rank, np.stack(Ms), np.array(norms), None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, None, traceback.format_exc() + str(e)))


@pytest.mark.parametrize("fixture", ["NORMAL_NORMAL", "GENERAL_SUPERC"])
def test_golden_observables_from_shards(gpu, fixture):
    """dens, docc, imp[0], doubles[0:2] of the reference's fixtures from occ_moments on the two shards of every state of
    the oracle's ground manifold, at the tolerance tests/test_occupations_host.py uses for the same numbers."""
    from edipack_amd.observables import from_moments
    from tests import observables as ob
    om, _, g = _golden_models(fixture)
    _, states = ob.ground_manifold(om)
    cplx = om.ed_mode != "normal"
    args = [(sec, np.ascontiguousarray(v, dtype=np.complex128 if cplx else np.float64)) for sec, _, v in states]
    res = _run_world(_golden_rank_main, 2, (f"edigpu_obs_gold_{os.getpid()}_{fixture}", fixture, args))
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    o = from_moments(res[0][1], om.norb, norm2=res[0][2])
    tol = 1e-9
    assert np.max(np.abs(o.dens - np.array(g["dens"]))) < tol and np.max(np.abs(o.docc - np.array(g["docc"]))) < tol
    assert abs(o.s2tot - g["imp"][0]) < tol
    assert abs(o.dust - g["doubles"][0]) < tol and abs(o.dund - g["doubles"][1]) < tol


# ---------------------------------------------------------------------------------------------------------
# refusals: one world of 2
# ---------------------------------------------------------------------------------------------------------
def _refusal_rank_main(rank, world, name, q):
    try:
        import ctypes as C
        import re
        import torch  # noqa: F401
        from edipack_amd import capi
        from edipack_amd.hamiltonian import SectorHamiltonian as H
        from edipack_amd.sharding import LibraryComm
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
                assert np.all(np.isfinite(buf)), what
                seen.append(what)
                return
            raise AssertionError(what + ": not refused")

        w = np.ones(2)
        # a whole flat handle in a world of 2
        _, ps = make_models("superc", "hybrid", 2, 3, seed=12)
        h = H.flat_from_model(ps, 0)
        vz = buf[:2 * h.dim].view(np.complex128)
        refused("whole flat / moments", "does not hold this rank's shard", lambda: comm.occ_moments(h, vz))
        refused("whole flat / apply", "does not hold this rank's shard", lambda: comm.apply_occ(h, vz, w, w))
        h.destroy()
        # a hand-over normal shard
        ho, pm, _ = _reference("normal", "normal", 2, 3, (4, 4))
        first, count, _ = comm.plan(ho.dimdw)
        h = H.normal_from_arrays(ho.dimup, ho.dimdw, ho.hd[first * ho.dimup:(first + count) * ho.dimup], ho.up, ho.dw, None,
                                 dw_first=first, dw_count=count)
        vr = buf[:count * ho.dimup]
        refused("hand-over / moments", "edigpu_occ_moments_sharded: .*must be built from a model", lambda: comm.occ_moments(h, vr))
        refused("hand-over / apply", "edigpu_apply_occ_sharded: .*must be built from a model", lambda: comm.apply_occ(h, vr, w, w))
        refused("hand-over / xph", "edigpu_apply_xph_sharded: .*must be built from a model", lambda: comm.apply_xph(h, vr))
        refused("hand-over / ph_rdm", "edigpu_ph_rdm_sharded: .*must be built from a model", lambda: comm.ph_rdm(h, vr))
        h.destroy()
        # no phonons
        h = H.normal_from_model(pm, 4, 4)
        vr = buf[:count * ho.dimup]
        refused("nph = 0 / xph", "edigpu_apply_xph_sharded: the handle has no phonons", lambda: comm.apply_xph(h, vr))
        refused("nph = 0 / ph_rdm", "edigpu_ph_rdm_sharded: the handle has no phonons", lambda: comm.ph_rdm(h, vr))
        refused("nvec = 0", "edigpu_occ_moments_sharded: nvec must be positive", lambda: comm.occ_moments(h, vr, 0))
        h.destroy()
        # DimPh = 33: the density matrix is refused
        _, pn = make_models("normal", "normal", 2, 2, seed=11)
        set_phonons(pn, 32)
        h = H.normal_from_model(pn, 1, 4)
        refused("DimPh = 33", "edigpu_ph_rdm_sharded: DimPh = 33 exceeds the limit of 32", lambda: comm.ph_rdm(h, buf))
        h.destroy()
        # overlapping vectors of the seed
        set_phonons(pn, 3)
        h = H.normal_from_model(pn, 3, 2)
        f2, c2, _ = comm.plan(h.dim_dw)
        n = c2 * h.dim_up * 4
        assert 0 < n and n + 1 <= buf.size
        L = capi.lib()
        for off in (0, 1, n - 1):
            refused(f"overlap +{off}", "edigpu_apply_xph_sharded: .*must not overlap",
                    lambda: capi.check(L.edigpu_apply_xph_sharded(h._h, comm._c, C.c_void_p(buf.ctypes.data),
                                                                  C.c_void_p(buf.ctypes.data + 8 * off)), "edigpu_apply_xph_sharded"))
        # and the same vectors side by side are served
        keep = buf.copy()
        capi.check(L.edigpu_apply_xph_sharded(h._h, comm._c, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 8 * n)),
                   "edigpu_apply_xph_sharded")
        ok = np.array_equal(buf[n:2 * n], ref_xph(keep[:n], 4)) and np.array_equal(buf[:n], keep[:n])
        h.destroy()
        comm.destroy()
        q.put((rank, seen, ok, None))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, None, False, traceback.format_exc() + str(e)))


def test_refusals_on_shards(gpu):
    res = _run_world(_refusal_rank_main, 2, (f"edigpu_obs_refuse_{os.getpid()}",))
    for _, seen, ok, _ in res:
        assert len(seen) == 13 and ok, seen
