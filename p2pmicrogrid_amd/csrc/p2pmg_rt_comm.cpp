// p2pmg_rt_comm.cpp — the world beyond one device: the RCCL loader, the communicator calls, the timed
// data-path collectives, and the DQN host exchange's registration.
#include <dlfcn.h>

#include <cstring>

#include "p2pmg_ctx.h"

using namespace p2pmg::rt;

namespace p2pmg::rt {

Rccl* rccl() {
  static Rccl r;
  static bool tried = false;
  if (!tried) {
    tried = true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
      r.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (r.h) break;
    }
    if (r.h) {
      r.getUniqueId = (int (*)(void*))dlsym(r.h, "ncclGetUniqueId");
      r.commInitRank = (int (*)(void**, int, Id128, int))dlsym(r.h, "ncclCommInitRank");
      r.allReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(r.h, "ncclAllReduce");
      r.commDestroy = (int (*)(void*))dlsym(r.h, "ncclCommDestroy");
      r.getErrorString = (const char* (*)(int))dlsym(r.h, "ncclGetErrorString");
      r.allGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(r.h, "ncclAllGather");
      r.commCount = (int (*)(const void*, int*))dlsym(r.h, "ncclCommCount");
    }
  }
  return (r.h && r.getUniqueId && r.commInitRank && r.allReduce && r.commDestroy) ? &r : nullptr;
}

// on the context's stream, so the bench line can report what the exchange step costs at world > 1
hipError_t coll_mark(p2pmg_ctx* c, int end) {
  hipError_t e = c->cring.ensure(p2pmg_ctx::kCRing);
  if (e != hipSuccess) return e;
  if (!end && c->n_coll >= p2pmg_ctx::kCRing && c->n_coll_folded == c->n_coll - p2pmg_ctx::kCRing) {
    // the slot's previous pair (kCRing collectives ago) is about to be overwritten: fold its
    // duration into the running total first, so p2pmg_collective_ms counts every collective.
    // Once per collective: a start whose collective then failed (no end mark, n_coll unchanged)
    // is followed by another start on the same slot, which must not fold the slot again
    float ms = 0.0f;
    e = c->cring.elapsed(c->n_coll, &ms);
    if (e != hipSuccess) return e;
    c->coll_folded_ms += ms;
    c->n_coll_folded++;
  }
  e = hipEventRecord(c->cring.pair(c->n_coll)[end], c->stream);
  if (end) c->n_coll++;
  return e;
}

}  // namespace p2pmg::rt

extern "C" {

int p2pmg_comm_unique_id(uint8_t id[128]) {
  if (!id) return P2PMG_E_INVALID;
  Rccl* r = rccl();
  if (!r) return P2PMG_E_UNSUPPORTED;
  return r->getUniqueId(id) == 0 ? P2PMG_OK : P2PMG_E_HIP;
}

int p2pmg_comm_init(p2pmg_ctx* c, const uint8_t id[128], int rank, int nranks) {
  if (!c || !id || rank < 0 || nranks <= 0 || rank >= nranks) return P2PMG_E_INVALID;
  if (c->dqn_roles) {
    std::string why;
    return fail(c, p2pmg::validate_dqn_roles_world("comm_init", nranks, true, &why), why);
  }
  Rccl* r = rccl();
  if (!r) return fail(c, P2PMG_E_UNSUPPORTED, "RCCL (librccl.so) not found");
  HIP_TRY(c, hipSetDevice(c->device));
  Id128 uid;
  std::memcpy(uid.b, id, 128);
  void* comm = nullptr;
  const int rc = r->commInitRank(&comm, nranks, uid, rank);
  if (rc != 0) return fail(c, P2PMG_E_HIP, std::string("ncclCommInitRank: ") + (r->getErrorString ? r->getErrorString(rc) : "?"));
  c->comm = comm;
  c->rank = rank;
  c->nranks = nranks;
  return P2PMG_OK;
}

int p2pmg_collective_ms(p2pmg_ctx* c, double* total_ms, int* count) {
  if (!c || !total_ms || !count) return P2PMG_E_INVALID;
  const long long n = c->n_coll < p2pmg_ctx::kCRing ? c->n_coll : p2pmg_ctx::kCRing;
  double sum = 0.0;
  for (long long k = c->n_coll - n; k < c->n_coll; ++k) {
    float ms = 0.0f;
    HIP_TRY(c, c->cring.elapsed(k, &ms));
    sum += ms;
  }
  *total_ms = c->coll_folded_ms + sum;
  *count = (int)c->n_coll;
  return P2PMG_OK;
}

int p2pmg_allreduce_q_delta(p2pmg_ctx* c) {
  if (!c) return P2PMG_E_INVALID;
  if (!c->qdelta) return fail(c, P2PMG_E_STATE, "allreduce_q_delta: context has no shared table");
  if (!c->comm) return fail(c, P2PMG_E_STATE, "allreduce_q_delta: p2pmg_comm_init first");
  Rccl* r = rccl();
  // ncclInt64 = 4, ncclSum = 0 (rccl.h)
  HIP_TRY(c, p2pmg::launch_fold_delta(c->qdelta, c->delta_n(), c->stream));
  HIP_TRY(c, coll_mark(c, 0));
  const int rc = r->allReduce(c->qdelta, c->qdelta, c->delta_n(), 4, 0, c->comm, c->stream);
  if (rc != 0) return fail(c, P2PMG_E_HIP, std::string("ncclAllReduce: ") + (r->getErrorString ? r->getErrorString(rc) : "?"));
  HIP_TRY(c, coll_mark(c, 1));
  return P2PMG_OK;
}

int p2pmg_comm_nranks(p2pmg_ctx* c, int* n) {
  if (!c || !n) return P2PMG_E_INVALID;
  if (!c->comm) {
    *n = 1;  // no communicator: a world of one
    return P2PMG_OK;
  }
  Rccl* r = rccl();
  if (!r->commCount) return fail(c, P2PMG_E_UNSUPPORTED, "ncclCommCount not found");
  const int rc = r->commCount(c->comm, n);
  if (rc != 0) return fail(c, P2PMG_E_HIP, std::string("ncclCommCount: ") + (r->getErrorString ? r->getErrorString(rc) : "?"));
  return P2PMG_OK;
}

int p2pmg_allreduce_metrics(p2pmg_ctx* c, double* out) {
  if (!c || !out) return P2PMG_E_INVALID;
  if (!c->ep_reward) return fail(c, P2PMG_E_STATE, "allreduce_metrics: no episode launched");
  if (!c->d_metrics) HIP_TRY(c, c->d_metrics.alloc(2));
  HIP_TRY(c, p2pmg::launch_metrics(c->S, c->ep_reward, c->d_metrics, c->stream));
  if (c->comm) {  // ncclFloat64 = 8, ncclSum = 0: sum and count over every rank (xGMI)
    Rccl* r = rccl();
    const int rc = r->allReduce(c->d_metrics, c->d_metrics, 2, 8, 0, c->comm, c->stream);
    if (rc != 0) return fail(c, P2PMG_E_HIP, std::string("ncclAllReduce(metrics): ") + (r->getErrorString ? r->getErrorString(rc) : "?"));
  }
  return read_small(c, out, c->d_metrics, 16);
}

int p2pmg_table_hash_allgather(p2pmg_ctx* c, uint64_t* out) {
  if (!c || !out) return P2PMG_E_INVALID;
  if (!c->q || c->n_tables == 0) return fail(c, P2PMG_E_STATE, "table_hash: context has no Q-table");
  const int n = c->comm ? c->nranks : 1;
  if (n > 1024) return fail(c, P2PMG_E_UNSUPPORTED, "table_hash: more than 1024 ranks");
  if (!c->d_hash) HIP_TRY(c, c->d_hash.alloc(1025));
  HIP_TRY(c, p2pmg::launch_table_hash(c->q, table_bytes(c, c->n_tables), c->d_hash + 1024, c->stream));
  if (c->comm) {  // ncclUint64 = 5: every rank's fingerprint, in rank order
    Rccl* r = rccl();
    if (!r->allGather) return fail(c, P2PMG_E_UNSUPPORTED, "ncclAllGather not found");
    const int rc = r->allGather(c->d_hash + 1024, c->d_hash, 1, 5, c->comm, c->stream);
    if (rc != 0) return fail(c, P2PMG_E_HIP, std::string("ncclAllGather: ") + (r->getErrorString ? r->getErrorString(rc) : "?"));
  } else {
    HIP_TRY(c, hipMemcpyAsync(c->d_hash, c->d_hash + 1024, 8, hipMemcpyDeviceToDevice, c->stream));
  }
  return download(c, {{out, c->d_hash, (size_t)n * 8}});
}

int p2pmg_comm_destroy(p2pmg_ctx* c) {
  if (!c) return P2PMG_E_INVALID;
  if (c->comm && rccl()) rccl()->commDestroy(c->comm);
  c->comm = nullptr;
  if (!c->xfn) c->rank = 0, c->nranks = 1;
  return P2PMG_OK;
}

int p2pmg_dqn_set_exchange(p2pmg_ctx* c, p2pmg_exchange_fn fn, void* user, int rank, int nranks) {
  if (!c) return P2PMG_E_INVALID;
  if (c->comm) return fail(c, P2PMG_E_STATE, "dqn_set_exchange: the context has an RCCL communicator");
  if (!fn) {
    c->xfn = nullptr;
    c->xuser = nullptr;
    c->rank = 0;
    c->nranks = 1;
    return P2PMG_OK;
  }
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(c, P2PMG_E_INVALID, "dqn_set_exchange: rank / nranks");
  if (c->dqn_roles && nranks > 1) {
    std::string why;
    return fail(c, p2pmg::validate_dqn_roles_world("dqn_set_exchange", nranks, false, &why), why);
  }
  c->xfn = fn;
  c->xuser = user;
  c->rank = rank;
  c->nranks = nranks;
  return P2PMG_OK;
}

}  // extern "C"
