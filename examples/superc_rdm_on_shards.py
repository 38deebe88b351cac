#!/usr/bin/env python3
"""The pair amplitude and the entanglement entropy of a superconducting impurity from eigenvector SHARDS: no rank ever
holds the whole state.

What a -D_MPI host does with rdm_flag=T in ed_mode=superc (imp_rdm_superc, ED_SUPERC/ED_RDM_SUPERC.f90:54-183), without
the gather of es_return_dvector_mpi:

  1. every rank solves for the lowest eigenpair of the sector Sz = 0 with its vectors as device-resident row shards
     (edigpu_lanczos_eigh_sharded) and keeps ITS elements of the eigenvector
  2. the impurity reduced density matrix rho_imp = Tr_bath |gs><gs| is taken from the shards
     (edigpu_imp_rdm_flat_sharded): a tile needs the 2^Norb consecutive rows of one bath word down, a row shard cuts
     anywhere in them, and the rank such a slab starts on completes it from one all-gather of less than a slab per rank;
     one small all-reduce adds the packed triangles, and every rank receives the same bits
  3. phisc_ab = <c_{b,up} c_{a,dw}> (rdm_anomalous) and the entanglement entropy follow from rho_imp on the host

The same density matrix is then taken from the assembled state on one GPU (edigpu_imp_rdm_flat) for comparison.

The ranks here share one GPU over the library's shared-memory communicator; on a node with several GPUs they would be
one process per GPU on the RCCL communicator (LibraryComm(rank, world, unique_id=...)), the calls are the same.

Run on a machine with an MI355X:   python examples/superc_rdm_on_shards.py [ranks]
"""
import multiprocessing as mp
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NORB, NBATH, SZ = 2, 4, 0


def model():
    from edipack_amd.hamiltonian import ImpurityModel
    rng = np.random.default_rng(1)
    hloc = np.zeros((1, 1, NORB, NORB), complex)
    hloc[0, 0] = np.diag([0.25, -0.25])
    return ImpurityModel(ed_mode="superc", bath_type="hybrid", norb=NORB, nbath=NBATH, nspin=1, hfmode=True, xmu=0.0,
                         uloc=np.array([2.0, 2.0]), ust=1.5, jh=0.25, jx=0.25, jp=0.25, hloc=hloc,
                         be=rng.uniform(-2, 2, (1, 1, NBATH)), bv=rng.uniform(0.2, 0.6, (1, NORB, NBATH)),
                         bd=rng.uniform(-0.3, 0.3, (1, 1, NBATH)))


def rank_main(rank, world, name, out):
    import torch  # noqa: F401  (one HIP runtime per process)
    from edipack_amd import capi
    from edipack_amd.observables import entanglement_entropy, rdm_anomalous, rdm_average
    from edipack_amd.sharding import LibraryComm, library_sharded_sector
    capi.init(0)
    comm = LibraryComm(rank, world, shm_name=name)
    h, first, count = library_sharded_sector(model(), SZ, comm)
    e0, x, nmv = comm.eigh(h, count, tol=1e-12)                # x: this rank's elements of the ground state
    geo = comm.imp_rdm_flat_info(h)                            # what the rank boundaries cut (host only)
    rho, norm2 = comm.imp_rdm_flat(h, x)                       # Tr_bath |gs><gs|, the sums over all ranks
    avg = rdm_average(rho, norm2)
    out.put((rank, first, count, e0, nmv, geo, rdm_anomalous(avg, NORB), entanglement_entropy(avg), rho[0], x))
    h.destroy()
    comm.destroy()


def single_main(x, out):
    """the same density matrix from the assembled state on one GPU (edigpu_imp_rdm_flat)"""
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import SectorHamiltonian
    from edipack_amd.observables import entanglement_entropy, rdm_average
    capi.init(0)
    h = SectorHamiltonian.flat_from_model(model(), SZ)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=h.dtype)).cuda()
    rho, norm2 = h.imp_rdm_flat(xd.data_ptr())
    h.destroy()
    out.put((entanglement_entropy(rdm_average(rho, norm2)), rho[0], norm2[0]))


def main():
    world = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=rank_main, args=(r, world, f"edigpu_example_{os.getpid()}", out)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(out.get(timeout=300) for _ in procs)
    for p in procs:
        p.join()
    for rank, first, count, e0, nmv, geo, phi, entropy, rho, x in res:
        print(f"rank {rank}: elements [{first}, {first + count})  E0 = {e0:.12f} ({nmv} products)  halo {geo['H']} elements, "
              f"{geo['slabs_in_place']} slabs in place, tail slab of {geo['tail_len']} ({geo['tail_own']} held here)")
        print(f"         phisc = {np.array2string(phi.real, precision=10)}  entanglement entropy = {entropy:.12f}")
    assert all(r[7] == res[0][7] and np.array_equal(r[8], res[0][8]) for r in res)      # the same bits on every rank
    # the state assembled here only to compare: one GPU, the whole vector
    whole = np.concatenate([r[9] for r in res])
    p = ctx.Process(target=single_main, args=(whole, out))
    p.start()
    s1, rho1, norm2 = out.get(timeout=300)
    p.join()
    tol = 4 * whole.size * 2.0 ** -53 * norm2          # any order of the same rounded products (tests/rdm_flat_cases.py)
    print(f"one GPU: entanglement entropy = {s1:.12f}  (shards - one GPU = {res[0][7] - s1:.3e}, "
          f"max |rho - rho_1| = {np.max(np.abs(res[0][8] - rho1)):.3e}, bound {tol:.3e})")
    assert np.max(np.abs(res[0][8] - rho1)) <= tol


if __name__ == "__main__":
    main()
