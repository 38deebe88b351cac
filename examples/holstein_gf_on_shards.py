#!/usr/bin/env python3
"""Electron Green's function of a one-orbital Anderson-Holstein impurity from eigenvector SHARDS: solve -> seed ->
tridiagonalise without any rank ever holding a whole vector.

The sibling of examples/holstein_gf_on_device.py for a -D_MPI host (ED_NORMAL/ED_GF_NORMAL.f90:131-177 between
`ed_solve` and `ed_get_gimp`), which otherwise gathers the eigenvector on the master rank, applies c / c^+ there and
scatters the seed again:

  1. every rank solves for the ground state of the sector with its vectors as device-resident shards
     (edigpu_lanczos_eigh_sharded) and keeps ITS down rows of the eigenvector, every phonon block of them
  2. c^+ / c on the shards (edigpu_apply_cops_sharded): the up operators leave the sharded index alone and exchange
     nothing; the down operators take one all-gather of the shards and the window form of the one-axis kernel
  3. the neighbouring sector is tridiagonalised from the seed shards (edigpu_lanczos_tridiag_sharded)
  4. poles and weights of the small tridiagonal matrix give G(i w) of either spin

and prints G(i w_0) beside the value of the same chain on one GPU with whole vectors.  The ranks here share one GPU over
the library's shared-memory communicator; on a node with several GPUs they would be one process per GPU on the RCCL
communicator (LibraryComm(rank, world, unique_id=...)), the calls are the same.

Run on a machine with an MI355X:   python examples/holstein_gf_on_shards.py [ranks]
"""
import multiprocessing as mp
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NBATH, NPH, SECTOR, NLANC = 5, 8, (3, 3), 200
BETA = 50.0


def model():
    from edipack_amd.hamiltonian import ImpurityModel
    rng = np.random.default_rng(1)
    return ImpurityModel(ed_mode="normal", bath_type="normal", norb=1, nbath=NBATH, nspin=1, hfmode=True, xmu=0.0,
                         uloc=np.array([2.0]), hloc=np.zeros((1, 1, 1, 1), complex),
                         be=rng.uniform(-2, 2, (1, 1, NBATH)), bv=rng.uniform(0.2, 0.6, (1, 1, NBATH)),
                         nph=NPH, w0_ph=0.5, a_ph=0.0, g_ph=np.array([[0.4]]))


def dest(create, spin):
    d = 1 if create else -1
    return (SECTOR[0] + d, SECTOR[1]) if spin == 0 else (SECTOR[0], SECTOR[1] + d)


def add_channel(g, z, e0, al, bl, nit, norm2, sign):
    if norm2 == 0.0:
        return
    t = np.diag(al[:nit]) + np.diag(bl[1:nit], 1) + np.diag(bl[1:nit], -1)
    et, y = np.linalg.eigh(t)
    g += np.sum((norm2 * y[0] ** 2)[None, :] / (z[:, None] - sign * (et - e0)[None, :]), axis=1)


def rank_main(rank, world, name, out):
    import torch  # noqa: F401  (one HIP runtime per process)
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian
    from edipack_amd.sharding import LibraryComm
    capi.init(0)
    comm = LibraryComm(rank, world, shm_name=name)
    pm = model()
    src = SectorHamiltonian.normal_from_model(pm, *SECTOR)           # the whole sector: the library cuts its down rows
    first, count, _ = comm.plan(src.dim_dw)
    nblk = NPH + 1
    e0, x, nmv = comm.eigh(src, count * src.dim_up * nblk, tol=1e-12)
    z = 1j * np.pi / BETA * (2 * np.arange(4) + 1)
    g, routes = [np.zeros(z.size, complex), np.zeros(z.size, complex)], {}
    for spin in (0, 1):
        for create, sign in ((True, 1), (False, -1)):
            dst = SectorHamiltonian.normal_from_model(pm, *dest(create, spin))
            ops = [(1.0, create, 0, spin)]
            nloc = comm.plan(dst.dim_dw)[1] * dst.dim_up * nblk
            seed = comm.apply_cops(src, dst, x, nloc, ops)
            routes[(spin, create)] = comm.apply_cops_info(src, dst, ops)
            al, bl, nit, norm2 = comm.tridiag(dst, seed, min(dst.dim, NLANC))
            add_channel(g[spin], z, e0, al, bl, nit, norm2, sign)
            dst.destroy()
    src.destroy()
    comm.destroy()
    out.put((rank, first, count, e0, nmv, g, routes))


def single_main(out):
    """the same chain with whole vectors on one GPU (examples/holstein_gf_on_device.py)"""
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian
    capi.init(0)
    pm = model()
    src = SectorHamiltonian.normal_from_model(pm, *SECTOR)
    ev, vec, _, _ = src.lanczos_eigh_multi(1, tol=1e-12)
    gs = torch.from_numpy(np.ascontiguousarray(vec[0])).cuda()
    z = 1j * np.pi / BETA * (2 * np.arange(4) + 1)
    g = [np.zeros(z.size, complex), np.zeros(z.size, complex)]
    for spin in (0, 1):
        for create, sign in ((True, 1), (False, -1)):
            dst = SectorHamiltonian.normal_from_model(pm, *dest(create, spin))
            seed = torch.empty(dst.dim, dtype=torch.float64, device="cuda")
            src.apply_op_to(dst, gs.data_ptr(), seed.data_ptr(), 0, spin, create)
            al, bl, nit, norm2 = dst.lanczos_tridiag_dev(seed.data_ptr(), min(dst.dim, NLANC))
            add_channel(g[spin], z, float(ev[0]), al, bl, nit, norm2, sign)
            dst.destroy()
    src.destroy()
    out.put((float(ev[0]), g))


def main():
    world = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=rank_main, args=(r, world, f"edigpu_example_{os.getpid()}", out)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(out.get(timeout=300) for _ in procs)
    for p in procs:
        p.join()
    for rank, first, count, e0, nmv, g, routes in res:
        print(f"rank {rank}: down rows [{first}, {first + count}) of {NPH + 1} phonon blocks  E0 = {e0:.12f} ({nmv} products)")
        print(f"         G_up(i w_0) = {g[0][0]:.10f}   G_dw(i w_0) = {g[1][0]:.10f}")
    assert all(np.array_equal(r[5][0], res[0][5][0]) and np.array_equal(r[5][1], res[0][5][1]) for r in res)   # the same bits
    names = {0: "local, nothing exchanged", 1: "one all-gather"}
    for (spin, create), (route, doubles) in sorted(res[0][6].items()):
        print(f"  {'c^+' if create else 'c  '}_{'dw' if spin else 'up'}: {names[route]}" + (f" of {doubles} doubles per rank" if route else ""))
    p = ctx.Process(target=single_main, args=(out,))
    p.start()
    e1, g1 = out.get(timeout=300)
    p.join()
    g = res[0][5]
    print(f"one GPU: E0 = {e1:.12f}  G_up(i w_0) = {g1[0][0]:.10f}   G_dw(i w_0) = {g1[1][0]:.10f}")
    print(f"         shards - one GPU: {abs(g[0][0] - g1[0][0]):.2e} (up), {abs(g[1][0] - g1[1][0]):.2e} (down)")
    assert max(np.max(np.abs(g[s] - g1[s])) for s in (0, 1)) < 1e-8 * np.max(np.abs(g1[0]))


if __name__ == "__main__":
    main()
