// capi_comm.cpp — the RCCL part of the C ABI (include/wfpt_amd.h): the
// communicator and the likelihoods whose sums are exchanged between ranks.
#include "capi_internal.hpp"

using namespace wfpt::capi;

extern "C" {

int wfpt_comm_unique_id(unsigned char id[128]) {
  if (!id) return fail(WFPT_ERR_ARG, "null pointer");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  ncclUniqueId u;
  NCCL_TRY(ncclGetUniqueId(&u));
  std::memcpy(id, &u, 128);
  return WFPT_OK;
}

int wfpt_comm_init(wfpt_ctx* c, int nranks, int rank, const unsigned char id[128]) {
  if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks)
    return fail(WFPT_ERR_ARG, "bad communicator arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HIP_TRY(hipSetDevice(c->device));
  ncclUniqueId u;
  std::memcpy(&u, id, 128);
  if (c->comm) {
    (void)ncclCommDestroy(c->comm);
    c->comm = nullptr;
  }
  NCCL_TRY(ncclCommInitRank(&c->comm, nranks, u, rank));
  c->nranks = nranks;
  c->rank = rank;
  return WFPT_OK;
}

int wfpt_comm_init_tcp(wfpt_ctx* c, int nranks, int rank, const char* host, int port,
                       int timeout_ms) {
  if (!c || !host || nranks < 1 || rank < 0 || rank >= nranks)
    return fail(WFPT_ERR_ARG, "bad communicator arguments");
  WFPT_RANGE("wfpt_comm_init_tcp");
  unsigned char id[128];
  std::memset(id, 0, sizeof(id));
  if (rank == 0)
    if (int rc = wfpt_comm_unique_id(id)) return rc;
  if (int rc = wfpt_comm_exchange_id(nranks, rank, host, port, timeout_ms, id)) return rc;
  return wfpt_comm_init(c, nranks, rank, id);
}

int wfpt_comm_init_all(wfpt_ctx* const* ctxs, int n) {
  if (!ctxs || n < 1) return fail(WFPT_ERR_ARG, "bad communicator arguments");
  std::vector<int> devs(n);
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i]) return fail(WFPT_ERR_ARG, "null context");
    devs[i] = ctxs[i]->device;
    for (int j = 0; j < i; ++j)
      if (ctxs[j] == ctxs[i] || devs[j] == devs[i])
        return fail(WFPT_ERR_ARG, "wfpt_comm_init_all: one context per distinct device");
  }
  WFPT_RANGE("wfpt_comm_init_all");
  std::vector<ncclComm_t> comms(n, nullptr);
  for (int i = 0; i < n; ++i) {
    std::lock_guard<std::mutex> lk(ctxs[i]->mu);
    if (ctxs[i]->comm) {
      DeviceGuard g(ctxs[i]->device);
      (void)ncclCommDestroy(ctxs[i]->comm);
      ctxs[i]->comm = nullptr;
    }
  }
  NCCL_TRY(ncclCommInitAll(comms.data(), n, devs.data()));
  for (int i = 0; i < n; ++i) {
    std::lock_guard<std::mutex> lk(ctxs[i]->mu);
    ctxs[i]->comm = comms[i];
    ctxs[i]->nranks = n;
    ctxs[i]->rank = i;
  }
  return WFPT_OK;
}

}  // extern "C"

namespace {
// One rank's local part of an all-reduce likelihood, in two steps so that a
// single process can overlap its devices (wfpt_wiener_like_allreduce_group):
// ar_launch enqueues the level-0 pass (+ the deferred pass unless the lean
// prediction applies) whose finalize leaves {sum, #zeros, errors} in the
// context's dedicated device triple c->ar.p; ar_settle waits for a lean call's
// level-0 result and, on a misprediction, enqueues the redo + fold passes and
// a second finalize over the intact chunk partials (an unconditional redo
// launch would dispatch one wave per chunk: ~48k blocks at 12.5M trials).
// After ar_settle, c->ar.p holds the rank's triple in stream order.
struct ArState {
  bool eng = false, lean = false, launched = false;
};
int ar_launch(wfpt_ctx* c, const wfpt_ds* d, const wfpt::Params& P, const wfpt::Knobs& K,
              ArState* st) {
  st->eng = engine_family(P, K);
  st->lean = st->eng && lean_predicted(c, d) && !c->count;
  st->launched = true;
  if (st->lean)
    return run_sum(c, d->x.p, d->n, P, K, c->mres.d, wfpt::kPassFast | wfpt::kPassLean, d, c->ar.p);
  return run_sum(c, d->x.p, d->n, P, K, c->ar.p, wfpt::kPassAll, d);
}
int ar_settle(wfpt_ctx* c, const wfpt_ds* d, const wfpt::Params& P, const wfpt::Knobs& K,
              const ArState& st) {
  if (!st.lean) return WFPT_OK;
  if (int rc = wait_result(c, c->mres.h)) return rc;
  if (res_deferred(c->mres.h))
    return run_sum(c, d->x.p, d->n, P, K, c->mres.d, wfpt::kPassDeferred | wfpt::kPassRedo, d,
                   c->ar.p);
  return WFPT_OK;
}
// After the exchange: the summed triple to the mapped slot with a fresh
// completion word (the local finalize used the previous one), then decode.
int ar_finish(wfpt_ctx* c, const wfpt_ds* d, const ArState& st, double* out) {
  wfpt::launch_publish(c->ar.p, c->mres.d, ++c->seq, c->stream);
  HIP_TRY(hipGetLastError());
  if (int rc = wait_result(c, c->mres.h)) return rc;
  split_advance(d, st.eng && !st.lean, c->mres.h);
  const int rc = decode_sum(c, c->mres.h, out);
  if (rc == WFPT_OK && st.eng) note_tree(d, c->mres.h);
  return rc;
}
// A call that failed after its passes may have been enqueued: the dataset's
// heavy-chunk record (written by an engine pass into the next parity's list)
// and its predictions are reset, so the next call starts from a consistent
// state (no split, the full call sequence).
void ar_reset(wfpt_ctx* c, const wfpt_ds* d) {
  if (!d) return;
  (void)hipStreamSynchronize(c->stream);
  d->nsplit = 0;
  d->nsplit2 = 0;
  d->no_defer = false;
  d->no_tree = false;
  d->tree_frac = 1.0;
  if (d->hcount.p) (void)hipMemset(d->hcount.p, 0, 4 * sizeof(int));
}
}  // namespace

extern "C" {

int wfpt_wiener_like_allreduce(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* p,
                               const wfpt_knobs* k, double* out) {
  if (!c) return fail(WFPT_ERR_ARG, "null context");
  // no communicator: no collective exists that a peer could be waiting in
  if (!c->comm) return fail(WFPT_ERR_ARG, "wfpt_comm_init was not called");
  // every exit below, once the communicator exists, goes through the exchange
  if (p && !p_outlier_in_range(p->p_outlier) && d && k && out &&
      d->ctx == c) {
    *out = -INFINITY;  // the same parameters on every rank: no exchange needed
    return WFPT_OK;
  }
  WFPT_RANGE("wfpt_wiener_like_allreduce");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  ArState st;
  int lrc = WFPT_OK;
  if (!d || !p || !k || !out) lrc = fail(WFPT_ERR_ARG, "null pointer");
  else if (d->ctx != c) lrc = fail(WFPT_ERR_ARG, "dataset belongs to another context");
  if (lrc == WFPT_OK) {
    const wfpt::Params P = to_params(p);
    const wfpt::Knobs K = to_knobs(k);
    lrc = ar_launch(c, d, P, K, &st);
    if (lrc == WFPT_OK) lrc = ar_settle(c, d, P, K, st);
  }
  // fault injection for the failure path's tests (WFPT_FAULT=allreduce_local:
  // this rank's local pass reports a failure after it ran)
  if (lrc == WFPT_OK) {
    const char* fi = std::getenv("WFPT_FAULT");
    if (fi && std::strcmp(fi, "allreduce_local") == 0)
      lrc = fail(WFPT_ERR_HIP, "injected local failure (WFPT_FAULT=allreduce_local)");
  }
  std::string lmsg;
  if (lrc != WFPT_OK) {
    // A rank that failed locally still enters the collective, with a
    // poisoned triple (kPeerFailUnit) written by a one-thread kernel into its
    // preallocated device triple (nothing on the host stack is read after
    // this call returns), so no peer waits on it forever; every peer then
    // decodes "a rank failed" and this rank returns its own error. Only a
    // broken stream (a sticky device fault) cannot enqueue the exchange: the
    // communicator is then aborted.
    lmsg = g_last_error;
    wfpt::launch_poison(c->ar.p, c->stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      (void)ncclCommAbort(c->comm);
      c->comm = nullptr;
      if (st.launched) ar_reset(c, d);
      return fail(lrc, lmsg + " (device stream unusable: RCCL communicator aborted; "
                              "re-create it with wfpt_comm_init)");
    }
  }
  // {sum, zeros, encoded errors} of every rank summed: any zero trial or
  // failure anywhere reaches every rank (wfpt_internal.h: the error counts
  // stay apart under the sum)
  const ncclResult_t nr = ncclAllReduce(c->ar.p, c->ar.p, 3, ncclDouble, ncclSum, c->comm, c->stream);
  if (lrc != WFPT_OK) {
    (void)hipStreamSynchronize(c->stream);
    if (st.launched) ar_reset(c, d);
    return fail(lrc, lmsg);
  }
  if (nr != ncclSuccess) {
    if (st.launched) ar_reset(c, d);
    return fail(WFPT_ERR_COMM, std::string("ncclAllReduce: ") + ncclGetErrorString(nr));
  }
  return ar_finish(c, d, st, out);
}

int wfpt_wiener_like_local(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* p,
                           const wfpt_knobs* k, double triple[3]) {
  if (!c || !d || !p || !k || !triple) return fail(WFPT_ERR_ARG, "null pointer");
  if (d->ctx != c) return fail(WFPT_ERR_ARG, "dataset belongs to another context");
  const wfpt::Params P = to_params(p);
  const wfpt::Knobs K = to_knobs(k);
  if (!p_outlier_in_range(P.p_outlier)) {  // -inf on every rank: one zero trial
    triple[0] = 0.0;
    triple[1] = 1.0;
    triple[2] = 0.0;
    return WFPT_OK;
  }
  WFPT_RANGE("wfpt_wiener_like_local");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  ArState st;
  int rc = ar_launch(c, d, P, K, &st);
  if (rc == WFPT_OK) rc = ar_settle(c, d, P, K, st);
  if (rc != WFPT_OK) {
    ar_reset(c, d);
    return rc;
  }
  double h[8];
  HIP_TRY(hipMemcpyAsync(h, c->ar.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  split_advance(d, st.eng && !st.lean, h);
  if (st.eng) note_tree(d, h);
  d->no_defer = false;
  (void)finish_profile(c);
  triple[0] = h[0];
  triple[1] = h[1];
  triple[2] = h[2];
  return WFPT_OK;
}

int wfpt_wiener_like_allreduce_group(wfpt_ctx* const* ctxs, const wfpt_ds* const* dss, int n,
                                     const wfpt_params* p, const wfpt_knobs* k, double* out) {
  if (!ctxs || !dss || n < 1 || !p || !k || !out) return fail(WFPT_ERR_ARG, "null pointer");
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i] || !dss[i]) return fail(WFPT_ERR_ARG, "null context or dataset");
    if (dss[i]->ctx != ctxs[i]) return fail(WFPT_ERR_ARG, "dataset belongs to another context");
    if (!ctxs[i]->comm || ctxs[i]->nranks != n || ctxs[i]->rank != i)
      return fail(WFPT_ERR_ARG, "contexts need wfpt_comm_init_all over the same list");
  }
  const wfpt::Params P = to_params(p);
  const wfpt::Knobs K = to_knobs(k);
  if (!p_outlier_in_range(P.p_outlier)) {
    *out = -INFINITY;
    return WFPT_OK;
  }
  WFPT_RANGE("wfpt_wiener_like_allreduce_group");
  std::vector<std::unique_lock<std::mutex>> locks;
  for (int i = 0; i < n; ++i) locks.emplace_back(ctxs[i]->mu);
  int prev = 0;
  (void)hipGetDevice(&prev);
  std::vector<ArState> st(n);
  // every device's local pass in flight before any wait; a failure on any
  // device ends the call before the collective (no device has entered it)
  int rc = WFPT_OK;
  for (int i = 0; i < n && rc == WFPT_OK; ++i) {
    (void)hipSetDevice(ctxs[i]->device);
    rc = ar_launch(ctxs[i], dss[i], P, K, &st[i]);
  }
  for (int i = 0; i < n && rc == WFPT_OK; ++i) {
    (void)hipSetDevice(ctxs[i]->device);
    rc = ar_settle(ctxs[i], dss[i], P, K, st[i]);
  }
  if (rc == WFPT_OK) {
    ncclResult_t r = ncclGroupStart();
    for (int i = 0; i < n && r == ncclSuccess; ++i)
      r = ncclAllReduce(ctxs[i]->ar.p, ctxs[i]->ar.p, 3, ncclDouble, ncclSum, ctxs[i]->comm,
                        ctxs[i]->stream);
    const ncclResult_t r2 = ncclGroupEnd();
    if (r == ncclSuccess) r = r2;
    if (r != ncclSuccess)
      rc = fail(WFPT_ERR_COMM, std::string("ncclAllReduce (group): ") + ncclGetErrorString(r));
  }
  double v = 0.0;
  for (int i = 0; i < n && rc == WFPT_OK; ++i) {
    (void)hipSetDevice(ctxs[i]->device);
    double vi = 0.0;
    rc = ar_finish(ctxs[i], dss[i], st[i], &vi);
    if (i == 0) v = vi;
  }
  if (rc != WFPT_OK) {
    // as the single-context path: a device whose passes were enqueued may
    // hold a half-written heavy-chunk record; every such dataset restarts
    // from the full call sequence
    const std::string msg = g_last_error;
    for (int i = 0; i < n; ++i) {
      if (!st[i].launched) continue;
      (void)hipSetDevice(ctxs[i]->device);
      ar_reset(ctxs[i], dss[i]);
    }
    g_last_error = msg;
  }
  (void)hipSetDevice(prev);
  if (rc == WFPT_OK) *out = v;
  return rc;
}

int wfpt_wiener_like_nodes_allreduce(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* per_node,
                                     int32_t n_nodes, const wfpt_knobs* k, double* out) {
  if (!c) return fail(WFPT_ERR_ARG, "null context");
  if (!c->comm) return fail(WFPT_ERR_ARG, "wfpt_comm_init was not called");
  // the exchange's count comes from the argument every rank passes, never
  // from this rank's dataset: a rank with a bad dataset still all-reduces
  // the same n_nodes + 1 doubles as its peers
  if (n_nodes < 0) return fail(WFPT_ERR_ARG, "n_nodes < 0 (no exchange entered)");
  WFPT_RANGE("wfpt_wiener_like_nodes_allreduce");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  // every exit once the communicator exists goes through the exchange: a
  // rank whose pass fails enters it with a poisoned vector
  int lrc = nodes_check(c, d, per_node, k, out);
  const int32_t m = n_nodes;
  if (lrc == WFPT_OK && d->n_nodes != n_nodes)
    lrc = fail(WFPT_ERR_ARG, "dataset has " + std::to_string(d->n_nodes) +
                                 " nodes, the call passes n_nodes = " + std::to_string(n_nodes));
  const wfpt::Knobs K = k ? to_knobs(k) : wfpt::Knobs{};  // (null k: nodes_check failed)
  wfpt::NodeSum ns{};
  if (lrc == WFPT_OK) lrc = nodes_launch(c, d, per_node, K, &ns);
  // fault injection for the failure path's tests (WFPT_FAULT=nodes_allreduce_local:
  // this rank's per-node pass reports a failure after it was enqueued)
  if (lrc == WFPT_OK) {
    const char* fi = std::getenv("WFPT_FAULT");
    if (fi && std::strcmp(fi, "nodes_allreduce_local") == 0)
      lrc = fail(WFPT_ERR_HIP, "injected local failure (WFPT_FAULT=nodes_allreduce_local)");
  }
  std::string lmsg = lrc != WFPT_OK ? g_last_error : std::string();
  if (c->res.cap < (size_t)m + 1) {  // the node vector of an early failure
    if (c->res.reserve((size_t)m + 1) != hipSuccess) {
      (void)ncclCommAbort(c->comm);
      c->comm = nullptr;
      return fail(WFPT_ERR_HIP, "node all-reduce: no device buffer for the exchange "
                                "(RCCL communicator aborted)");
    }
  }
  wfpt::launch_segment_res(lrc == WFPT_OK ? c->lp.p : nullptr, lrc == WFPT_OK ? d->off.p : nullptr,
                           m, c->res.p, c->status.p, lrc != WFPT_OK, c->stream, c->ncnt.p, &ns);
  if (hipGetLastError() != hipSuccess) {
    (void)ncclCommAbort(c->comm);
    c->comm = nullptr;
    return nodes_recover(c, fail(lrc != WFPT_OK ? lrc : WFPT_ERR_HIP,
                                 lmsg + " (device stream unusable: RCCL communicator aborted)"));
  }
  // per-node sums (and the error count) of every rank summed: a node's
  // -inf on any rank reaches every rank (wfpt.pyx:71-72 per node)
  const ncclResult_t nr = ncclAllReduce(c->res.p, c->res.p, (size_t)m + 1, ncclDouble, ncclSum,
                                        c->comm, c->stream);
  if (lrc != WFPT_OK) return nodes_recover(c, fail(lrc, lmsg));
  if (nr != ncclSuccess)
    return nodes_recover(c, fail(WFPT_ERR_COMM, std::string("ncclAllReduce: ") +
                                                    ncclGetErrorString(nr)));
  wfpt::launch_publish_vec(c->res.p, m, c->mnode.d, ++c->seq, c->stream);
  if (hipGetLastError() != hipSuccess)
    return nodes_recover(c, fail(WFPT_ERR_HIP, "publish_vec_kernel launch failed"));
  if (int rc = wait_word(c, c->mnode.h + m + 1)) return nodes_recover(c, rc);
  if (int rc = check_status_value(c->mnode.h[m])) return rc;
  if (int rc = finish_profile(c)) return rc;
  std::memcpy(out, c->mnode.h, m * sizeof(double));
  return WFPT_OK;
}

}  // extern "C"
