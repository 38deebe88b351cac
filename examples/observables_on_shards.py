#!/usr/bin/env python3
"""Ground-state observables of an Anderson impurity from eigenvector SHARDS: no rank ever holds the whole state.

What a -D_MPI host does between `ed_solve` and `ed_get_dens` (ED_NORMAL/ED_DIAG_NORMAL.f90:221-242,
ED_NORMAL/ED_OBSERVABLES_NORMAL.f90:120-185), without the gather of es_return_dvector_mpi:

  1. every rank solves for the lowest eigenpair of the sector with its vectors as device-resident shards
     (edigpu_lanczos_eigh_sharded) and keeps ITS rows of the eigenvector
  2. the occupation moments sum_i |v_i|^2 n_x(i) n_y(i) of the shards are added over the ranks by one small all-reduce
     (edigpu_occ_moments_sharded); every rank receives the same bits
  3. from_moments turns them into dens, docc, magz, sz2, n2, s2tot, Dust, Dund
  4. the chi_spin seed Sz_a |gs> is made on the shard (edigpu_apply_occ_sharded, no exchange) and tridiagonalised there

The ranks here share one GPU over the library's shared-memory communicator; on a node with several GPUs they would be
one process per GPU on the RCCL communicator (LibraryComm(rank, world, unique_id=...)), the calls are the same.

Run on a machine with an MI355X:   python examples/observables_on_shards.py [ranks]
"""
import multiprocessing as mp
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NORB, NBATH, SECTOR = 2, 3, (4, 4)


def model():
    from edipack_amd.hamiltonian import ImpurityModel
    rng = np.random.default_rng(1)
    hloc = np.zeros((1, 1, NORB, NORB), complex)
    hloc[0, 0, 0, 0], hloc[0, 0, 1, 1] = 0.3, -0.3
    return ImpurityModel(ed_mode="normal", bath_type="normal", norb=NORB, nbath=NBATH, nspin=1, hfmode=True, xmu=0.0,
                         uloc=np.array([2.0, 2.0]), ust=1.2, jh=0.4, hloc=hloc,
                         be=rng.uniform(-2, 2, (1, NORB, NBATH)), bv=rng.uniform(0.2, 0.6, (1, NORB, NBATH)))


def rank_main(rank, world, name, out):
    import torch  # noqa: F401  (one HIP runtime per process)
    from edipack_amd import capi
    from edipack_amd.observables import from_moments
    from edipack_amd.sharding import LibraryComm, library_sharded_sector
    capi.init(0)
    comm = LibraryComm(rank, world, shm_name=name)
    h, first, count = library_sharded_sector(model(), SECTOR, comm)
    nloc = count * h.dim_up
    e0, x, nmv = comm.eigh(h, nloc, tol=1e-12)                 # x: this rank's rows of the ground state
    M, norm2 = comm.occ_moments(h, x)                          # the sums over all ranks
    o = from_moments(M[0], NORB, norm2=norm2[0])
    seed = comm.apply_sz(h, x, 0)                              # Sz_1 |gs> on the shard
    a, b, niter, seed_norm2 = comm.tridiag(h, seed, 30)
    h.destroy()
    comm.destroy()
    out.put((rank, first, count, e0, nmv, o.dens, o.docc, o.s2tot, seed_norm2, o.sz2[0, 0], a[:3]))


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
    for rank, first, count, e0, nmv, dens, docc, s2tot, sn2, sz2, a in res:
        print(f"rank {rank}: down rows [{first}, {first + count})  E0 = {e0:.12f} ({nmv} products)  dens = {dens}  "
              f"docc = {docc}  s2tot = {s2tot:.10f}")
        print(f"         <Sz_1 gs|Sz_1 gs> = {sn2:.12f} (sz2[0,0] = {sz2:.12f})  alpha[0:3] = {a}")
    assert all(np.array_equal(r[5], res[0][5]) and r[7] == res[0][7] for r in res)     # the same bits on every rank


if __name__ == "__main__":
    main()
