// rccl_stub.cpp — a stand-in for librccl that moves the collectives of the C ABI between PROCESSES THAT SHARE ONE GPU.
//
// TEST INFRASTRUCTURE. RCCL refuses two ranks on one device, and the build and round-end boxes of this project have one GPU, so
// the world > 1 branches of libykpred (ykpred_gather_bitmap / _compressed with its per-peer header exchange, the in-place
// all-reduces of ykpred_exchange_decisions and of the topology histograms inside ykpred_eval / ykpred_eval_nodes) had only ever
// run with world = 1. This library implements exactly the entry points libykpred resolves — ncclGetUniqueId, ncclCommInitRank,
// ncclCommDestroy, ncclAllGather, ncclAllReduce, ncclGetErrorString — with their RCCL semantics (device pointers, in-place
// forms, ordering after the work already queued on the stream) over a POSIX shared-memory segment: every rank copies its
// contribution into its slot, a barrier, every rank reads the slots. ykpred_comm_use_library() points the engine at it.
// It is slow on purpose (synchronous, through host memory): what it proves is argument marshalling, layouts and ordering.
// It is also STRICTER than RCCL about agreement: every rank records (count, type, op) of its call in the segment's header, and
// when the ranks disagree — or one of them could not stage its contribution — EVERY rank returns ncclInvalidArgument, after
// both barriers, instead of reducing or copying stale slot bytes (RCCL would hang or read garbage).
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace {
constexpr size_t kSlotBytes = (size_t)96 << 20;  // per rank (sparse: only what a test touches is ever backed by memory)
constexpr int kMaxRanks = 8;
struct Call {  // what a rank passed to the collective it is in (ok = 0: it could not stage its contribution)
  uint64_t count;
  int32_t type, op, ok, pad;
};
struct Header {
  std::atomic<int> arrived;
  std::atomic<int> generation;
  std::atomic<int> attached;
  Call call[kMaxRanks];
};
static_assert(sizeof(Header) <= 4096, "the header fits the segment's first page");
struct Comm {
  int rank = 0, world = 1;
  std::string name;
  char* base = nullptr;
  size_t bytes = 0;
  Header* hdr() const { return (Header*)base; }
  char* slot(int r) const { return base + 4096 + (size_t)r * kSlotBytes; }
};
void barrier(Comm* c) {
  Header* h = c->hdr();
  const int gen = h->generation.load(std::memory_order_acquire);
  if (h->arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == c->world) {
    h->arrived.store(0, std::memory_order_relaxed);
    h->generation.fetch_add(1, std::memory_order_release);
  } else {
    while (h->generation.load(std::memory_order_acquire) == gen) usleep(50);
  }
}
size_t type_size(ncclDataType_t t) {
  switch (t) {
    case ncclInt8: case ncclUint8: return 1;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return 0;
  }
}
// Records this rank's call, waits for everybody, and tells whether every rank made the same call and staged its part.
// Either way every rank has passed the first barrier; the caller passes the second one before it returns.
bool agree(Comm* c, size_t count, ncclDataType_t type, int op, bool ok) {
  Call& mine = c->hdr()->call[c->rank];
  mine.count = count;
  mine.type = (int32_t)type;
  mine.op = op;
  mine.ok = ok ? 1 : 0;
  barrier(c);
  const Call& first = c->hdr()->call[0];
  for (int r = 0; r < c->world; ++r) {
    const Call& o = c->hdr()->call[r];
    if (!o.ok || o.count != first.count || o.type != first.type || o.op != first.op) return false;
  }
  return true;
}
template <class T>
void reduce_into(T* acc, const T* in, size_t n, ncclRedOp_t op) {
  for (size_t i = 0; i < n; ++i) {
    if (op == ncclSum) acc[i] = (T)(acc[i] + in[i]);
    else if (op == ncclMax) acc[i] = in[i] > acc[i] ? in[i] : acc[i];
    else if (op == ncclMin) acc[i] = in[i] < acc[i] ? in[i] : acc[i];
  }
}
}  // namespace

extern "C" {

ncclResult_t ncclGetUniqueId(ncclUniqueId* id) {
  memset(id, 0, sizeof *id);
  snprintf(id->internal, sizeof id->internal, "/ykstub-%d-%ld", (int)getpid(), (long)random());
  return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t* out, int nranks, ncclUniqueId id, int rank) {
  if (nranks < 1 || nranks > kMaxRanks || rank < 0 || rank >= nranks) return ncclInvalidArgument;
  Comm* c = new Comm();
  c->rank = rank;
  c->world = nranks;
  c->name = std::string(id.internal, strnlen(id.internal, sizeof id.internal));
  c->bytes = 4096 + (size_t)nranks * kSlotBytes;
  const int fd = shm_open(c->name.c_str(), O_CREAT | O_RDWR, 0600);
  if (fd < 0 || ftruncate(fd, (off_t)c->bytes) != 0) {
    delete c;
    return ncclSystemError;
  }
  c->base = (char*)mmap(nullptr, c->bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (c->base == MAP_FAILED) {
    delete c;
    return ncclSystemError;
  }
  // every rank attaches before anybody uses the segment (a fresh segment is zero-filled: the counters start at 0)
  c->hdr()->attached.fetch_add(1, std::memory_order_acq_rel);
  while (c->hdr()->attached.load(std::memory_order_acquire) < nranks) usleep(50);
  *out = (ncclComm_t)c;
  return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
  Comm* c = (Comm*)comm;
  if (!c) return ncclSuccess;
  barrier(c);
  if (c->rank == 0) shm_unlink(c->name.c_str());
  munmap(c->base, c->bytes);
  delete c;
  return ncclSuccess;
}

ncclResult_t ncclAllGather(const void* send, void* recv, size_t count, ncclDataType_t type, ncclComm_t comm, hipStream_t stream) {
  Comm* c = (Comm*)comm;
  if (!c) return ncclInvalidArgument;
  const size_t bytes = count * type_size(type);
  bool ok = type_size(type) != 0 && bytes <= kSlotBytes;
  ok = ok && hipStreamSynchronize(stream) == hipSuccess;  // ordered after the work queued on the stream
  ok = ok && (!bytes || hipMemcpy(c->slot(c->rank), send, bytes, hipMemcpyDeviceToHost) == hipSuccess);
  if (!agree(c, count, type, -1, ok)) {
    barrier(c);
    return ncclInvalidArgument;
  }
  ncclResult_t res = ncclSuccess;
  for (int r = 0; r < c->world && bytes && res == ncclSuccess; ++r)
    if (hipMemcpy((char*)recv + (size_t)r * bytes, c->slot(r), bytes, hipMemcpyHostToDevice) != hipSuccess) res = ncclUnhandledCudaError;
  barrier(c);  // nobody overwrites a slot before everybody has read it
  return res;
}

ncclResult_t ncclAllReduce(const void* send, void* recv, size_t count, ncclDataType_t type, ncclRedOp_t op, ncclComm_t comm, hipStream_t stream) {
  Comm* c = (Comm*)comm;
  if (!c) return ncclInvalidArgument;
  const size_t bytes = count * type_size(type);
  bool ok = bytes <= kSlotBytes && (op == ncclSum || op == ncclMax || op == ncclMin) && (type == ncclInt32 || type == ncclInt64 || type == ncclUint64);
  ok = ok && hipStreamSynchronize(stream) == hipSuccess;
  ok = ok && (!bytes || hipMemcpy(c->slot(c->rank), send, bytes, hipMemcpyDeviceToHost) == hipSuccess);
  if (!agree(c, count, type, (int)op, ok)) {
    barrier(c);
    return ncclInvalidArgument;
  }
  ncclResult_t res = ncclSuccess;
  if (bytes) {
    char* acc = new char[bytes];
    memcpy(acc, c->slot(0), bytes);
    for (int r = 1; r < c->world; ++r) {
      if (type == ncclInt32) reduce_into((int32_t*)acc, (const int32_t*)c->slot(r), count, op);
      else if (type == ncclInt64) reduce_into((int64_t*)acc, (const int64_t*)c->slot(r), count, op);
      else reduce_into((uint64_t*)acc, (const uint64_t*)c->slot(r), count, op);
    }
    const hipError_t s = hipMemcpy(recv, acc, bytes, hipMemcpyHostToDevice);
    delete[] acc;
    if (s != hipSuccess) res = ncclUnhandledCudaError;
  }
  barrier(c);
  return res;
}

const char* ncclGetErrorString(ncclResult_t r) {
  switch (r) {
    case ncclSuccess: return "no error";
    case ncclInvalidArgument: return "invalid argument (rccl stub)";
    case ncclSystemError: return "system error (rccl stub: shared memory)";
    case ncclUnhandledCudaError: return "HIP call failed (rccl stub)";
    default: return "error (rccl stub)";
  }
}

}  // extern "C"
