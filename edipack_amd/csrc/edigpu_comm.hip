// edigpu_comm.hip -- the communicator of the N > 1 path: transports, collectives, life cycle.  It knows ranks, streams
// and buffers of doubles, nothing of sectors (the sharded product and recurrence on top of it: edigpu_shard.hip).
//
// One process per GPU.  The communicator is RCCL over xGMI (loaded at run time: the library a host already mapped --
// PyTorch ships its own copy -- or /opt/rocm's); a second, host-staged transport through POSIX shared memory lets
// several ranks of one node share a GPU (tests of the N > 1 data flow on a one-GPU box; no RCCL needed).
// Every collective is enqueued on a HIP stream.
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <thread>

#include "shard_comm.hpp"

namespace edigpu {

// ---------------------------------------------------------------------------------------------------------
// RCCL, resolved at run time
// ---------------------------------------------------------------------------------------------------------
// types and enum values from the vendor header; the entry points themselves are looked up with dlsym
typedef ncclUniqueId rccl_unique_id;
typedef ncclComm_t rccl_comm_t;
#define RCCL_SUM ncclSum
#define RCCL_FLOAT64 ncclFloat64

struct RcclApi {
  void* lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;  // optional
};

static RcclApi* rccl() {
  static RcclApi api;
  static bool tried = false;
  if (tried) return api.lib ? &api : nullptr;
  tried = true;
  // a copy the host process already mapped wins (one RCCL per process), then the system one
  const char* names[] = {"librccl.so", "librccl.so.1"};
  for (const char* n : names)
    if (!api.lib) api.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
  for (const char* n : names)
    if (!api.lib) api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
  if (!api.lib) api.lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!api.lib) return nullptr;
#define EDIGPU_SYM(field, name)                                  \
  *(void**)(&api.field) = dlsym(api.lib, name);                 \
  if (!api.field) {                                              \
    api.lib = nullptr;                                           \
    return nullptr;                                              \
  }
  EDIGPU_SYM(GetUniqueId, "ncclGetUniqueId")
  EDIGPU_SYM(CommInitRank, "ncclCommInitRank")
  EDIGPU_SYM(CommDestroy, "ncclCommDestroy")
  EDIGPU_SYM(AllReduce, "ncclAllReduce")
  EDIGPU_SYM(AllGather, "ncclAllGather")
  EDIGPU_SYM(Send, "ncclSend")
  EDIGPU_SYM(Recv, "ncclRecv")
  EDIGPU_SYM(GroupStart, "ncclGroupStart")
  EDIGPU_SYM(GroupEnd, "ncclGroupEnd")
  EDIGPU_SYM(GetErrorString, "ncclGetErrorString")
#undef EDIGPU_SYM
  *(void**)(&api.CommCount) = dlsym(api.lib, "ncclCommCount");
  return &api;
}

#define EDIGPU_RCCL(call)                                                                              \
  do {                                                                                                 \
    ncclResult_t _r = (call);                                                                          \
    if (_r != ncclSuccess) {                                                                                     \
      set_error(std::string(#call) + " failed: " + (rccl() ? rccl()->GetErrorString(_r) : "no RCCL")); \
      return 1;                                                                                        \
    }                                                                                                  \
  } while (0)

}  // namespace edigpu

// ---------------------------------------------------------------------------------------------------------
// communicator
// ---------------------------------------------------------------------------------------------------------
struct ShmHeader {
  std::atomic<int> ready;       // set by rank 0 once the region is initialised
  std::atomic<int> arrived;     // barrier: arrivals of the current generation
  std::atomic<int> generation;  // barrier: bumped by the last arriver
  int world;
  int64_t slot_bytes;
  int64_t created_s;            // CLOCK_REALTIME seconds when rank 0 made the segment (stale leftovers are refused)
};

namespace edigpu {

static int shm_barrier(edigpu_comm_s* c) {
  ShmHeader* h = c->hdr;
  const int gen = h->generation.load(std::memory_order_acquire);
  if (h->arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == c->world) {
    h->arrived.store(0, std::memory_order_relaxed);
    h->generation.store(gen + 1, std::memory_order_release);
    return 0;
  }
  const auto t0 = std::chrono::steady_clock::now();
  while (h->generation.load(std::memory_order_acquire) == gen) {
    std::this_thread::yield();
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) {
      set_error("edigpu_comm (shm): barrier timed out after 120 s (a rank is missing)");
      return 1;
    }
  }
  return 0;
}

static char* shm_slot(edigpu_comm_s* c, int r) { return c->slots + (size_t)r * (size_t)c->hdr->slot_bytes; }

static int shm_fits(edigpu_comm_s* c, size_t bytes) {
  if ((int64_t)bytes > c->hdr->slot_bytes) {
    set_error("edigpu_comm (shm): message of " + std::to_string(bytes) + " bytes exceeds the slot size given at creation");
    return 1;
  }
  return 0;
}

// Every collective of a communicator is enqueued on the communicator's OWN stream (c->side), whatever stream the caller
// computes on: one communicator driven from two streams is legal only as long as every rank issues the same order, and
// that is exactly what a single in-order stream guarantees (the first multi-GPU run should not be the one to find out).
// side_begin: the collective waits for what `st` has enqueued so far; side_end: `st` waits for the collective.  A caller
// that overlaps the exchange with its own kernels passes c->side itself and places the two events where it needs them.
// CommSwitches::comm_two_streams (measurement only): collectives on the caller's stream, as before round 3
static int side_begin(edigpu_comm_s* c, hipStream_t st) {
  if (st == c->side) return 0;
  EDIGPU_HIP(hipEventRecord(c->ev_in, st));
  EDIGPU_HIP(hipStreamWaitEvent(c->side, c->ev_in, 0));
  return 0;
}
static int side_end(edigpu_comm_s* c, hipStream_t st) {
  if (st == c->side) return 0;
  EDIGPU_HIP(hipEventRecord(c->ev_out, c->side));
  EDIGPU_HIP(hipStreamWaitEvent(st, c->ev_out, 0));
  return 0;
}

namespace {
// The bracket of one collective: st = the stream it is enqueued on; opened with begin(), closed when the scope ends
class SideScope {
 public:
  SideScope(edigpu_comm_s* c, hipStream_t caller)
      : st(c->sw.comm_two_streams ? caller : c->side), c_(c), waiter_(st == c->side ? caller : st) {}
  int begin() {
    if (side_begin(c_, waiter_)) return 1;
    open_ = true;
    return 0;
  }
  ~SideScope() {
    if (open_) (void)side_end(c_, waiter_);
  }
  const hipStream_t st;

 private:
  edigpu_comm_s* c_;
  hipStream_t waiter_;
  bool open_ = false;
};
}  // namespace

// Host-staged exchange: every rank puts nsend doubles into its slot of the segment; once all have, read(stage) fills
// this rank's nrecv doubles of c->stage from the slots; once all have read (the slots may be overwritten), they go up.
template <class Read>
static int shm_exchange(edigpu_comm_s* c, const double* send, size_t nsend, double* recv, size_t nrecv, hipStream_t st, Read read) {
  if (shm_fits(c, nsend * sizeof(double))) return 1;
  EDIGPU_HIP(hipMemcpyAsync(shm_slot(c, c->rank), send, nsend * sizeof(double), hipMemcpyDeviceToHost, st));
  EDIGPU_HIP(hipStreamSynchronize(st));
  if (shm_barrier(c)) return 1;
  if (c->stage.size() < nrecv) c->stage.resize(nrecv);  // (grow-only: a 3-double all-reduce leaves a product's size alone)
  read(c->stage.data());
  if (shm_barrier(c)) return 1;
  EDIGPU_HIP(hipMemcpyAsync(recv, c->stage.data(), nrecv * sizeof(double), hipMemcpyHostToDevice, st));
  EDIGPU_HIP(hipStreamSynchronize(st));
  return 0;
}

static const double* shm_slot_d(edigpu_comm_s* c, int r) { return reinterpret_cast<const double*>(shm_slot(c, r)); }

int comm_all_to_all(edigpu_comm_s* c, const double* send, double* recv, size_t n, hipStream_t caller) {
  if (alone(c)) {
    EDIGPU_HIP(hipMemcpyAsync(recv, send, n * sizeof(double), hipMemcpyDeviceToDevice, caller));
    return 0;
  }
  SideScope side(c, caller);
  if (side.begin()) return 1;
  if (c->kind == edigpu_comm_s::kRccl) {
    RcclApi* r = rccl();
    EDIGPU_RCCL(r->GroupStart());
    for (int p = 0; p < c->world; p++) {
      EDIGPU_RCCL(r->Send(send + (size_t)p * n, n, RCCL_FLOAT64, p, c->nccl, side.st));
      EDIGPU_RCCL(r->Recv(recv + (size_t)p * n, n, RCCL_FLOAT64, p, c->nccl, side.st));
    }
    EDIGPU_RCCL(r->GroupEnd());
    return 0;
  }
  return shm_exchange(c, send, n * c->world, recv, n * c->world, side.st, [&](double* stage) {
    for (int s = 0; s < c->world; s++) memcpy(stage + (size_t)s * n, shm_slot_d(c, s) + (size_t)c->rank * n, n * sizeof(double));
  });
}

int comm_all_gather(edigpu_comm_s* c, const double* send, double* recv, size_t n, hipStream_t caller) {
  if (alone(c)) {
    EDIGPU_HIP(hipMemcpyAsync(recv, send, n * sizeof(double), hipMemcpyDeviceToDevice, caller));
    return 0;
  }
  SideScope side(c, caller);
  if (side.begin()) return 1;
  if (c->kind == edigpu_comm_s::kRccl) {
    EDIGPU_RCCL(rccl()->AllGather(send, recv, n, RCCL_FLOAT64, c->nccl, side.st));
    return 0;
  }
  return shm_exchange(c, send, n, recv, n * c->world, side.st, [&](double* stage) {
    for (int s = 0; s < c->world; s++) memcpy(stage + (size_t)s * n, shm_slot_d(c, s), n * sizeof(double));
  });
}

int comm_all_reduce(edigpu_comm_s* c, double* buf, size_t n, hipStream_t caller) {
  if (alone(c)) return 0;
  SideScope side(c, caller);
  if (side.begin()) return 1;
  if (c->kind == edigpu_comm_s::kRccl) {
    EDIGPU_RCCL(rccl()->AllReduce(buf, buf, n, RCCL_FLOAT64, RCCL_SUM, c->nccl, side.st));
    return 0;
  }
  return shm_exchange(c, buf, n, buf, n, side.st, [&](double* acc) {  // in rank order on every rank
    std::fill(acc, acc + n, 0.0);
    for (int s = 0; s < c->world; s++) {
      const double* p = shm_slot_d(c, s);
      for (size_t i = 0; i < n; i++) acc[i] += p[i];
    }
  });
}

int comm_rccl_ranks(const edigpu_comm_s* c) {
  if (c->kind != edigpu_comm_s::kRccl) return 0;
  if (!c->nccl) return 1;  // (a world of one makes no RCCL communicator)
  int n = -1;
  if (rccl() && rccl()->CommCount && rccl()->CommCount(c->nccl, &n) != ncclSuccess) n = -1;
  return n;
}

// A communicator under construction, and the end of a finished one: everything it owns is released on every early
// return of its creation and by edigpu_comm_destroy
namespace {
struct CommDeleter {
  void operator()(edigpu_comm_s* self) const {
    if (!self) return;
    if (self->device >= 0) (void)hipSetDevice(self->device);  // (else nothing was made on a device yet)
    self->ws.release();
    if (self->nccl && rccl()) (void)rccl()->CommDestroy(self->nccl);
    if (self->side) (void)hipStreamDestroy(self->side);
    for (hipEvent_t ev : {self->ev_ready, self->ev_done, self->ev_in, self->ev_out})
      if (ev) (void)hipEventDestroy(ev);
    if (self->shm) munmap(self->shm, self->shm_bytes);
    // (a rank > 0 never removes the name, whatever became of its creation)
    if (self->shm_created) shm_unlink(self->shm_name.c_str());
    delete self;
  }
};
}  // namespace
using CommPtr = std::unique_ptr<edigpu_comm_s, CommDeleter>;

static CommPtr comm_new(int rank, int world, edigpu_comm_s::Transport kind) {
  CommPtr c(new edigpu_comm_s());
  c->rank = rank;
  c->world = world;
  c->kind = kind;
  return c;
}

static int comm_common(edigpu_comm_s* c) {
  EDIGPU_HIP(hipGetDevice(&c->device));
  EDIGPU_HIP(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
  EDIGPU_HIP(hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming));
  EDIGPU_HIP(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
  EDIGPU_HIP(hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
  EDIGPU_HIP(hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming));
  return 0;
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_comm_unique_id(void* id128) {
  if (!id128) {
    set_error("edigpu_comm_unique_id: NULL argument");
    return 1;
  }
  RcclApi* r = rccl();
  if (!r) {
    set_error("edigpu_comm_unique_id: RCCL (librccl.so) could not be loaded");
    return 1;
  }
  rccl_unique_id id;
  EDIGPU_RCCL(r->GetUniqueId(&id));
  memcpy(id128, &id, sizeof(id));
  return 0;
}

int edigpu_comm_create(edigpu_comm* out, int32_t rank, int32_t world, const void* id128) {
  if (!out || world < 1 || rank < 0 || rank >= world || (world > 1 && !id128)) {
    set_error("edigpu_comm_create: bad argument");
    return 1;
  }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    set_error("edigpu_comm_create: no usable HIP device; this library has no CPU fallback");
    return 1;
  }
  CommPtr c = comm_new(rank, world, edigpu_comm_s::kRccl);
  if (comm_common(c.get())) return 1;
  if (world > 1 || id128) {
    RcclApi* r = rccl();
    if (!r) {
      set_error("edigpu_comm_create: RCCL (librccl.so) could not be loaded");
      return 1;
    }
    rccl_unique_id id;
    memcpy(&id, id128, sizeof(id));
    ncclResult_t rc = r->CommInitRank(&c->nccl, world, id, rank);
    if (rc != ncclSuccess) {
      set_error(std::string("edigpu_comm_create: ncclCommInitRank failed: ") + r->GetErrorString(rc));
      return 1;
    }
  }
  *out = c.release();
  return 0;
}

int edigpu_comm_create_shm(edigpu_comm* out, int32_t rank, int32_t world, const char* name, int64_t slot_bytes) {
  if (!out || !name || world < 1 || rank < 0 || rank >= world || slot_bytes < 64) {
    set_error("edigpu_comm_create_shm: bad argument");
    return 1;
  }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    set_error("edigpu_comm_create_shm: no usable HIP device; this library has no CPU fallback");
    return 1;
  }
  CommPtr c = comm_new(rank, world, edigpu_comm_s::kHostStaged);
  c->shm_name = name[0] == '/' ? name : std::string("/") + name;
  slot_bytes = (slot_bytes + 63) / 64 * 64;
  c->shm_bytes = 4096 + (size_t)world * (size_t)slot_bytes;
  int fd = -1;
  if (rank == 0) {
    shm_unlink(c->shm_name.c_str());
    fd = shm_open(c->shm_name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
    c->shm_created = fd >= 0;
    if (fd >= 0 && ftruncate(fd, (off_t)c->shm_bytes) != 0) {
      close(fd);
      fd = -1;
    }
  }
  const int64_t started_s = (int64_t)time(nullptr);
  const auto t_open = std::chrono::steady_clock::now();
  // Ranks > 0 may find a segment a crashed run left under the same name (right size, ready = 1) before rank 0 has
  // replaced it.  A segment is taken only if rank 0 made it no more than two minutes before this call and the name
  // still refers to it once it reads ready; otherwise it is dropped and the name is opened again.
  for (;;) {
    if (rank != 0) {
      fd = -1;
      while (fd < 0 && std::chrono::steady_clock::now() - t_open < std::chrono::seconds(60)) {
        fd = shm_open(c->shm_name.c_str(), O_RDWR, 0600);
        struct stat sb;
        if (fd >= 0 && (fstat(fd, &sb) != 0 || (size_t)sb.st_size < c->shm_bytes)) {
          close(fd);
          fd = -1;
        }
        if (fd < 0) std::this_thread::sleep_for(std::chrono::milliseconds(5));
      }
    }
    if (fd < 0) {
      set_error("edigpu_comm_create_shm: cannot open the shared-memory segment " + c->shm_name);
      return 1;
    }
    struct stat mine;
    const bool have_ino = fstat(fd, &mine) == 0;
    c->shm = mmap(nullptr, c->shm_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (c->shm == MAP_FAILED) {
      set_error("edigpu_comm_create_shm: mmap failed");
      c->shm = nullptr;
      return 1;
    }
    c->hdr = reinterpret_cast<ShmHeader*>(c->shm);
    c->slots = reinterpret_cast<char*>(c->shm) + 4096;
    if (rank == 0) {
      c->hdr->arrived.store(0);
      c->hdr->generation.store(0);
      c->hdr->world = world;
      c->hdr->slot_bytes = slot_bytes;
      c->hdr->created_s = started_s;
      c->hdr->ready.store(1, std::memory_order_release);
      break;
    }
    bool ok = false, timeout = false;
    while (!ok && !timeout) {
      if (c->hdr->ready.load(std::memory_order_acquire) == 1) {
        struct stat now;
        const std::string path = "/dev/shm" + c->shm_name;
        const bool same = !have_ino || (stat(path.c_str(), &now) == 0 && now.st_ino == mine.st_ino);
        ok = same && c->hdr->created_s >= started_s - 120 && c->hdr->world == world && c->hdr->slot_bytes == slot_bytes;
        if (!ok) break;  // a leftover: map the name again
      } else {
        std::this_thread::yield();
      }
      timeout = std::chrono::steady_clock::now() - t_open > std::chrono::seconds(60);
    }
    if (ok) break;
    munmap(c->shm, c->shm_bytes);
    c->shm = nullptr;
    if (timeout || std::chrono::steady_clock::now() - t_open > std::chrono::seconds(60)) {
      set_error("edigpu_comm_create_shm: rank 0 never initialised the segment");
      return 1;
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(5));
  }
  if (comm_common(c.get()) || shm_barrier(c.get())) return 1;
  *out = c.release();
  return 0;
}

int edigpu_comm_info(edigpu_comm c, int32_t* rank, int32_t* world, int32_t* kind) {
  if (!c) {
    set_error("edigpu_comm_info: NULL communicator");
    return 1;
  }
  if (rank) *rank = c->rank;
  if (world) *world = c->world;
  if (kind) *kind = c->kind;
  return 0;
}

int edigpu_comm_destroy(edigpu_comm c) {
  CommDeleter()(c);
  return 0;
}

}  // extern "C"
