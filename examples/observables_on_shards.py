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
  5. the impurity reduced density matrix rho_imp = Tr_bath |gs><gs| (rdm_flag=T, ED_RDM_NORMAL.f90:146-209) is taken
     from the shards too (edigpu_imp_rdm_sharded: a run of down rows that a rank boundary cuts is completed by an
     all-gather of a few rows), and its entanglement entropy is printed beside the one edigpu_imp_rdm gives for the
     same state held whole on one GPU

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
    from edipack_amd.observables import entanglement_entropy, from_moments, rdm_average
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
    rho, rho_norm2 = comm.imp_rdm(h, x)                        # Tr_bath |gs><gs|, the sums over all ranks
    entropy = entanglement_entropy(rdm_average(rho, rho_norm2))
    h.destroy()
    comm.destroy()
    out.put((rank, first, count, e0, nmv, o.dens, o.docc, o.s2tot, seed_norm2, o.sz2[0, 0], a[:3], entropy, rho[0], x))


def single_main(x, out):
    """the same density matrix from the assembled state on one GPU (edigpu_imp_rdm)"""
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian
    from edipack_amd.observables import entanglement_entropy, rdm_average
    capi.init(0)
    h = SectorHamiltonian.normal_from_model(model(), *SECTOR)
    xd = torch.from_numpy(x).cuda()
    rho, norm2 = h.imp_rdm(xd.data_ptr())
    h.destroy()
    out.put((entanglement_entropy(rdm_average(rho, norm2)), rho[0], norm2[0]))


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
    for rank, first, count, e0, nmv, dens, docc, s2tot, sn2, sz2, a, entropy, rho, x in res:
        print(f"rank {rank}: down rows [{first}, {first + count})  E0 = {e0:.12f} ({nmv} products)  dens = {dens}  "
              f"docc = {docc}  s2tot = {s2tot:.10f}")
        print(f"         <Sz_1 gs|Sz_1 gs> = {sn2:.12f} (sz2[0,0] = {sz2:.12f})  alpha[0:3] = {a}")
        print(f"         entanglement entropy of the impurity = {entropy:.12f}")
    assert all(np.array_equal(r[5], res[0][5]) and r[7] == res[0][7] for r in res)     # the same bits on every rank
    assert all(r[11] == res[0][11] and np.array_equal(r[12], res[0][12]) for r in res)
    # the state assembled here only to compare: one GPU, the whole vector
    whole = np.concatenate([r[13] for r in res])
    p = ctx.Process(target=single_main, args=(whole, out))
    p.start()
    s1, rho1, norm2 = out.get(timeout=300)
    p.join()
    tol = 4 * whole.size * 2.0 ** -53 * norm2          # any order of the same rounded products (tests/test_gpu_rdm.py)
    print(f"one GPU: entanglement entropy = {s1:.12f}  (shards - one GPU = {res[0][11] - s1:.3e}, "
          f"max |rho - rho_1| = {np.max(np.abs(res[0][12] - rho1)):.3e}, bound {tol:.3e})")
    assert np.max(np.abs(res[0][12] - rho1)) <= tol


if __name__ == "__main__":
    main()
