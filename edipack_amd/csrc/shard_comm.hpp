// shard_comm.hpp -- what the communicator (edigpu_comm.hip) and the sharded product and recurrence (edigpu_shard.hip)
// share with the observables and the seeds on shards (edigpu_shard_obs.hip, edigpu_shard_seeds.hip): the communicator's
// state, its three collectives and two predicates, the geometry of a shard.  Not part of the ABI.
#pragma once
#include <rccl/rccl.h>

#include <string>
#include <vector>

#include "dev_mem.hpp"

struct ShmHeader;  // edigpu_comm.hip

namespace edigpu {

// Device buffers of the sharded product and recurrence, kept by the communicator and grown on demand (comm_workspace in
// edigpu_shard.hip).  Capacities in doubles: vin / vout / tmp, vfull (all-gather form only), the four exchange buffers.
// Grow-only and tracked one by one: a communicator serves sectors of different geometry (transposed and all-gather) in turn
struct ShardWorkspace {
  int64_t ws_chunk = 0, ws_full = 0, ws_x = 0, ws_bp = 0;
  double *vin = nullptr, *vout = nullptr, *tmp = nullptr, *vfull = nullptr;
  double *send = nullptr, *recv = nullptr, *hvc = nullptr, *back = nullptr;
  // transposed exchange on padded panels (ShardGeom::block); bp[4]: the work vector of the recurrence kept in that layout
  double* bp[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  double *hist = nullptr, *work = nullptr, *scr = nullptr;
  int64_t hist_cap = 0;
  // observables on shards (edigpu_shard_obs.hip): host vectors staged for the kernels, the packed sums of a reduction
  double *obs = nullptr, *red = nullptr;
  int64_t obs_cap = 0, red_cap = 0;
  // impurity reduced density matrix on shards: the halo rows this rank sends, the halos of all ranks, the boundary slab
  double *halo = nullptr, *halos = nullptr, *slab = nullptr;
  int64_t halo_cap = 0, halos_cap = 0, slab_cap = 0;
  // c / c^+ and pair seeds on shards (edigpu_shard_seeds.hip): the padded chunk this rank sends, the gathered source, and
  // the staging of host vectors (source and destination shard)
  double *seed_send = nullptr, *seed_full = nullptr, *seed_io = nullptr;
  int64_t seed_send_cap = 0, seed_full_cap = 0, seed_io_cap = 0;
  void release() {  // (with the communicator's device current)
    dev_free_all(vin, vout, tmp, vfull, send, recv, hvc, back, hist, work, scr, bp[0], bp[1], bp[2], bp[3], bp[4], obs, red, halo,
                 halos, slab, seed_send, seed_full, seed_io);
  }
  ~ShardWorkspace() { release(); }
};

}  // namespace edigpu

struct edigpu_comm_s {
  const edigpu::CommSwitches sw = edigpu::CommSwitches::sample();  // the environment edigpu_comm_create* saw (switches.hpp)
  int rank = 0, world = 1;
  enum Transport : int { kRccl = 0, kHostStaged = 1 };  // (the values: edigpu_comm_info)
  Transport kind = kRccl;
  int device = -1;  // the calling thread's when the stream and events were made
  ncclComm_t nccl = nullptr;
  hipStream_t side = nullptr;  // exchange stream: the all-to-all / all-gather of a product runs beside its local part
  hipEvent_t ev_ready = nullptr, ev_done = nullptr;   // overlapped exchange: compute stream -> side, side -> compute stream
  hipEvent_t ev_in = nullptr, ev_out = nullptr;       // bracket of every other collective (side_begin / side_end)
  // shm transport
  std::string shm_name;
  bool shm_created = false;  // this rank (0) made the segment and removes its name again
  void* shm = nullptr;
  size_t shm_bytes = 0;
  ShmHeader* hdr = nullptr;
  char* slots = nullptr;
  std::vector<double> stage;  // host side of a host-staged exchange
  edigpu::ShardWorkspace ws;
};

namespace edigpu {

#pragma GCC visibility push(hidden)
// a world of one still issues its collectives through RCCL (one-GPU rehearsal of the calls)
inline bool force_collectives(const edigpu_comm_s* c) {
  return c->sw.force_collectives && c->kind == edigpu_comm_s::kRccl && c->nccl != nullptr;
}
// nobody to exchange with: a collective is at most a local copy, and a product needs no side stream
inline bool alone(const edigpu_comm_s* c) { return c->world == 1 && !force_collectives(c); }
// whether p is device (or managed) memory; a plain host pointer is not
inline bool on_device(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // (a plain host pointer, on runtimes that do not know "unregistered")
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}
// _CMPLX_NORMAL held as one real sector on the doubled up index: its down rows shard like any real sector's (each row
// 2 DimUp doubles = DimUp complex elements), so every sharded call on a complex sector runs on that image
inline edigpu_sector* real_image(edigpu_sector* s) { return s->kind == kCmplxNormal && s->sub_d ? s->sub_d : s; }

// How a sector's vector is cut over the ranks of a communicator (edigpu_shard.hip shard_geometry)
struct ShardGeom {
  bool transposed = false;  // normal mode, whole-sector handle: two all-to-alls per product
  int w = 1;                // doubles per element
  int64_t units = 0, unit_len = 1, q = 0, first = 0, count = 0;
  int64_t nloc = 0, chunk = 0;  // elements of this rank's shard / of the padded chunk
  int nblk = 1;                 // phonon blocks per vector (Nph + 1): the local vector is nblk blocks of blk elements
  int64_t blk = 0;
  // transposed exchange
  int halo = 0;
  int64_t pcol = 0, col_first = 0, col_count = 0, pw = 0, xlen = 0;
  // the same exchange on the padded panel layout of the local-block kernels (kernels_sb.hip, "row shards"): no packing,
  // no halo -- the partner columns of an Hnd term sit in the same panel
  bool block = false;
  int npmax = 0;      // panels per rank
  int64_t bplen = 0;  // doubles of a vector in the shard form: world * npmax * q * 16
  LoopSwitches loop = {};  // the environment shard_geometry saw: held for the product, recurrence or solve that g serves
};

// g <- the geometry of handle s on communicator c, 0; or 1 with the message set: the handle is not this rank's shard, a
// phonon sector with a general g_ph(a,b), a four-product complex sector.  Complex normal-mode handles: pass real_image(s).
int shard_geometry(const edigpu_sector* s, const edigpu_comm_s* c, ShardGeom& g);
// its first part, which cannot fail: how the rows are cut (w, nblk, units, unit_len, q, first, count, blk, nloc, chunk) and
// nothing of the product's exchange -- all that the seeds on shards need (edigpu_shard_seeds.hip)
void shard_rows(const edigpu_sector* s, const edigpu_comm_s* c, ShardGeom& g);

// The collectives (edigpu_comm.hip), each enqueued: on the communicator's own stream, bracketed by events so that it
// runs after what `caller` holds so far and `caller` goes on after it; a caller that passes c->side places its own events.
// recv[s * n .. (s+1) * n) <- block `rank` of rank s's send buffer; n doubles per block (equal split)
int comm_all_to_all(edigpu_comm_s* c, const double* send, double* recv, size_t n, hipStream_t caller);
// recv[s * n .. (s+1) * n) <- send of rank s
int comm_all_gather(edigpu_comm_s* c, const double* send, double* recv, size_t n, hipStream_t caller);
// buf[0..n) <- sum over the ranks (the same order on every rank: bit-identical results everywhere)
int comm_all_reduce(edigpu_comm_s* c, double* buf, size_t n, hipStream_t caller);
// ncclCommCount of the communicator; 0: shared-memory transport, 1: a world of one without RCCL, -1: RCCL has no such symbol
int comm_rccl_ranks(const edigpu_comm_s* c);
#pragma GCC visibility pop

}  // namespace edigpu
