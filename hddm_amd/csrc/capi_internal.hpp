// capi_internal.hpp — what the C ABI's translation units (capi_*.cpp,
// wfpt_rendezvous.cpp) share: the last-error slot, the error macros, owning
// device / pinned buffers, the context, the dataset base and the call-sequence
// helpers that capi_core.cpp defines. Not part of the public ABI: everything
// declared here has hidden visibility.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/wfpt_amd.h"
#include "pointwise_internal.h"
#include "wfpt_internal.h"
#include "wfpt_lean_tables.hpp"
#include "wfpt_types.hpp"

#pragma GCC visibility push(hidden)

namespace wfpt {
struct RlRow;     // rl_internal.h
struct DriftRow;  // sim_internal.h
struct RlSimRow;  // sim_internal.h

namespace capi {

extern thread_local std::string g_last_error;
int fail(int code, const std::string& msg);

// roctx range around each C-ABI entry point (rocprofv3 --marker-trace shows
// the host side of a call next to its kernels); WFPT_ROCTX=0 turns them off.
bool roctx_on();
struct RoctxRange {
  bool on;
  explicit RoctxRange(const char* name) : on(roctx_on()) {
    if (on) roctxRangePushA(name);
  }
  ~RoctxRange() {
    if (on) roctxRangePop();
  }
};
#define WFPT_RANGE(name) ::wfpt::capi::RoctxRange wfpt_range_(name)

#define HIP_TRY(expr)                                                                 \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return ::wfpt::capi::fail(WFPT_ERR_HIP,                                         \
                                std::string(#expr) + ": " + hipGetErrorString(e_));   \
  } while (0)

#define NCCL_TRY(expr)                                                                 \
  do {                                                                                 \
    ncclResult_t r_ = (expr);                                                          \
    if (r_ != ncclSuccess)                                                             \
      return ::wfpt::capi::fail(WFPT_ERR_COMM,                                         \
                                std::string(#expr) + ": " + ncclGetErrorString(r_));   \
  } while (0)

// Grow-only device array; frees itself (with whatever device is current: the
// owner is destroyed or released inside a DeviceGuard).
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    size_t want = std::max<size_t>(n, 256);
    hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Pinned host memory mapped into the device address space (fine-grained,
// coherent): the host writes per-call inputs / reads results there directly.
template <class T>
struct MappedBuf {
  T* h = nullptr;  // host pointer
  T* d = nullptr;  // device alias
  size_t cap = 0;
  MappedBuf() = default;
  MappedBuf(const MappedBuf&) = delete;
  MappedBuf& operator=(const MappedBuf&) = delete;
  ~MappedBuf() { release(); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    const size_t want = std::max<size_t>(n, 64);
    hipError_t e = hipHostMalloc((void**)&h, want * sizeof(T),
                                 hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&d, h, 0);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (h) (void)hipHostFree(h);
    h = nullptr;
    d = nullptr;
    cap = 0;
  }
};

// A host vector into a device array of its own (datasets: uploaded once).
template <class T>
hipError_t upload_vec(DevBuf<T>& dst, const std::vector<T>& v) {
  hipError_t e = dst.reserve(std::max<size_t>(v.size(), 1));
  if (e == hipSuccess && !v.empty())
    e = hipMemcpy(dst.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}
template <class... B>
void release_all(B&... b) {
  (b.release(), ...);
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    (void)hipGetDevice(&prev);
    if (prev != dev) (void)hipSetDevice(dev);
    // a stale error of an earlier, already reported runtime call must not be
    // read as this call's launch failure (hipGetLastError after launches)
    (void)hipGetLastError();
  }
  ~DeviceGuard() {
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
  }
};

// A resident dataset of any family: registered with its context, which frees
// its device memory and detaches it at wfpt_close (a dataset destroyed after
// its context only frees its host part).
struct DsBase {
  wfpt_ctx* ctx = nullptr;
  virtual void free_device() = 0;
  virtual ~DsBase() = default;
};
void ds_register(wfpt_ctx* c, DsBase* d);
void ds_destroy(DsBase* d);  // the body of every wfpt_*_dataset_destroy

// Per-call workspaces of the RL family (rl_kernels.hip)
struct RlWork {
  DevBuf<double> drift;     // the scan's drifts, compact (scored trials)
  DevBuf<double> drift_in;  // ... of every trial in the caller's order (_ex calls)
  DevBuf<double> arr;       // node batch: per-trial parameter arrays (rl_fill_kernel)
  DevBuf<double> npart;     // node batch: block partials of the per-node sums
  DevBuf<RlRow> rows;       // node batch: the nodes' Q-learning rows
  DevBuf<Params> par;       // node batch: the nodes' DDM rows
};
// ... of the regression front end (reg_kernels.hip)
struct RegWork {
  DevBuf<double> arr;    // per-trial parameter arrays (reg_fill_kernel), stored order
  DevBuf<double> pred;   // the predicted parameters in the caller's order (_ex calls)
  DevBuf<double> coef;   // the call's coefficient rows
  DevBuf<Params> par;    // groups call: the groups' DDM rows
  DevBuf<double> npart;  // groups call: block partials of the per-group sums
};
// ... of the RT sampler (sim_kernels.hip): the call's grid, rows, draw offsets,
// row totals, tile workspace, uniforms, draws and (debugging calls) grid indices
struct SimWork {
  DevBuf<double> grid, tot, ws, u, out;
  DevBuf<Params> rows;
  DevBuf<int64_t> off, idx;
  DevBuf<DriftRow> drift_rows;  // the diffusion-path simulator's row table
  DevBuf<RlSimRow> rl_rows;     // the closed-loop RLDDM simulator's row table,
  DevBuf<double> rl_in;         // its supplied rewards / observed feedback,
  DevBuf<int64_t> rl_idx;       // observed responses and the statistics' group offsets
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  double ms[4] = {0, 0, 0, 0};  // profiled time by stage: density, scan, normalise, draws
  ~SimWork() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// ... of the per-row RT statistics (stats_kernels.hip)
struct StatsWork {
  DevBuf<double> out;    // [R x K] the rows' statistics
  DevBuf<int32_t> list;  // the rows of each tier and block-tier LDS size, one group after the other
  DevBuf<double> ws;     // global tier: the padded row being sorted
  DevBuf<unsigned long long> count;  // NaN draws of a drift call whose draws stay on the device
};

// ... of the model-comparison pass (pointwise_kernels.hip): the per-trial
// accumulator state, one array per field, and the finished statistics
struct PointwiseWork {
  DevBuf<double> st;    // [4 x len] m | r | mean | M2
  DevBuf<int32_t> cnt;  // [2 x len] k | n_inf
  DevBuf<double> out;   // [4 x len] lppd | p_waic | mean | n_inf
  int64_t len = 0;      // trials of the pass in progress
  hipEvent_t ev[2] = {nullptr, nullptr};
  double ms = 0.0;      // profiled time of the accumulate kernel
  ~PointwiseWork() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace capi
}  // namespace wfpt

using wfpt::capi::DevBuf;
using wfpt::capi::MappedBuf;

struct wfpt_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  DevBuf<double> x;       // uploads of host arrays
  DevBuf<double> part;    // block partial sums
  DevBuf<int> zero;       // block zero counts
  DevBuf<double> res;     // per-node results
  DevBuf<double> ar;      // this rank's {sum, zeros, errors, ...} of an all-reduce call (8
                          // doubles, allocated at open: a failed workspace reserve cannot
                          // keep a rank out of the exchange)
  DevBuf<double> lp;      // per-trial outputs
  DevBuf<double> marr;    // wiener_like_multi parameter arrays
  DevBuf<double*> mptr;
  DevBuf<double> mscal;
  // deferred-trial state of adaptive calls (wfpt_internal.h: Work), sized for
  // the largest call so far: slot-indexed, nslots = 64 * chunks
  DevBuf<unsigned char> wl;  // lane of the deferred trial in each slot
  DevBuf<int> wl_n;          // per chunk: deferred trials
  DevBuf<int> rflag;         // per slot: kFlagExact | kFlagFallback
  DevBuf<unsigned char> redo;  // per chunk: the lean pass left it to the engine (0 at rest)
  // one-off device words, allocated and zeroed at open
  DevBuf<int> tree_any;      // some chunk refined in-wave (finalize reports + clears)
  DevBuf<double> fin;        // multi-block finalize scratch (3 x 64 doubles)
  DevBuf<int> fin_ticket;    // its last-block ticket (0 at rest)
  DevBuf<int> prof;          // 16 refinement work counters (PROF_EVALS)
  DevBuf<unsigned long long> phase;  // engine phase cycles (diagnostic builds)
  // The lean pass's series-decision table (wfpt_lean_tables.hpp: decision_tab). It
  // depends on err alone and costs ~0.2 ms of bisection, so it is kept here,
  // keyed by err's bit pattern, and rebuilt only when err changes. It travels
  // to the kernel by value, so there is nothing to upload.
  wfpt::DecisionTab dtab;
  uint64_t dtab_err = 0;
  bool dtab_valid = false;
  DevBuf<int> defer;         // dmat_cdf_array: deferred trial indices + count
  DevBuf<double> cdf_tab;    // dmat_cdf_array: the call's parameter-only tables
  DevBuf<double> rows_in;    // dmat_cdf_rows: the call's rows | x | freq_obs | n_samples, packed
  DevBuf<double> rows_out;   // ... and its cdf | chisq | gsq
  std::vector<double> rows_host;  // host side of both (one copy each way)
  DevBuf<int64_t> nd_idx;    // wiener_like_nodes: deferred trial indices
  DevBuf<int64_t> rare_v;    // wiener_like_nodes: the rare trials (wfpt_engine.hpp: NodeRare)
  DevBuf<int32_t> rare_j;
  DevBuf<wfpt::Params> nd_par;  // ... and their parameter rows
  DevBuf<int> nd_chunks;     // wiener_like_nodes: chunks the level-0 pass left to the chunk engine
  DevBuf<int> ncnt;          // [4]: the node path's listed chunks / records counters and [3]
                             // the publish ticket (0 at rest: the call's last kernel resets
                             // them; a failed call restores them)
  DevBuf<int> n_defer;       // [4]: the per-node path's listed chunks, chunk-path records,
                             // fast-pass records (0 at rest)
  DevBuf<unsigned long long> evals;
  DevBuf<int> status;          // Simpson-stack overflow flag
  MappedBuf<int> host_status;  // pinned mirror
  MappedBuf<double> mres;  // mapped pinned {sum, zeros, errors, deferred, word, heavy, #tree}
  unsigned long long seq = 0;  // completion word finalize writes to mres[4]
  MappedBuf<wfpt::Params> mnodep;  // per-node parameter table of wiener_like_nodes
  DevBuf<wfpt::Params> dnodep;     // its device copy (node_table_dev: WFPT_NODE_TABLE_DEV=1)
  // WFPT_HOST_TIMING=1: host time of the multi-table node calls by phase
  // (table rows, launches, wait, copy-out; ns summed), printed at wfpt_close
  bool host_timing = false;
  std::chrono::steady_clock::time_point ht_mark;
  double ht[5] = {0, 0, 0, 0, 0};
  int64_t ht_calls = 0;
  bool node_table_dev = false;
  MappedBuf<double> mnode;         // per-node sums + status + completion word
  bool spin = true;            // poll mres[3] instead of hipStreamSynchronize
  bool nodes_generic = false;  // WFPT_NODES=generic: per-trial generic node kernel only
  // WFPT_NODE_SPLIT=1: the per-node level 0 of the adaptive t families split
  // over five lanes per trial (node_split_kernel; measured slower on config 4:
  // the per-lane grid and hints are redone by every lane); WFPT_NODE_SPEC=0:
  // sparse deferred trials through the breadth-first rounds instead of
  // node_record_spec
  bool node_split = false;
  bool node_spec = true;
  bool fast_only = true;       // WFPT_FAST_ONLY=0: resident calls always enqueue the slow pass
  bool lean = true;            // WFPT_LEAN=0: resident calls never use the lean level-0 pass
  bool small = true;           // WFPT_SMALL=0: one-block calls keep the separate finalize
  // WFPT_LEAN_FIRST=0: the lean pass takes every chunk in stored order. Else a
  // call whose chunks exceed lean_first_min (the device's wave slots at the
  // lean kernel's 4 waves per SIMD: more than one dispatch round;
  // WFPT_LEAN_FIRST_MIN overrides it, for tests on small data) dispatches the
  // chunks predicted to take the generic site first (lean_first_search).
  // Above lean_first_max chunks (kLeanFirstRounds dispatch rounds) the list is
  // off again: the gain is one generic wave's excess at the launch's end (4.4
  // us of C3's 60.9), while the build that reads the list runs its uniform
  // waves up to 2% slower (0.9 us per 1M trials by the 100M-trial set), which
  // overtakes the gain near 5M trials = 19 rounds; 8 keeps a factor of two.
  bool lean_first = true;
  int64_t lean_first_min = 0, lean_first_max = 0;
  wfpt::LeanFirst first_last{};  // the last likelihood call's list (wfpt_debug_lean_first)
  // WFPT_LEAN_TREE: the largest fraction of refining chunks (last call) for
  // which the lean pass + engine redo of those chunks beats the engine over
  // every chunk
  double lean_tree_max = 0.0;
  bool profile = false;      // HIP events around the main kernel
  bool count = false;        // pdf_sv evaluation counting
  double k_ms = 0.0;
  int64_t launches = 0;
  int64_t n_evals = 0;
  // per-trial check (wfpt_wiener_like_trials): device buffer of the call's
  // per-trial log terms (the summing kernels' OUT_BOTH build), else null
  double* trial = nullptr;
  int path = 0;  // WFPT_PATH_* bits of the kernels the last likelihood call launched
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  std::vector<wfpt::capi::DsBase*> dsets;  // the live datasets of every family
  wfpt::capi::RlWork rl;
  wfpt::capi::RegWork reg;
  wfpt::capi::SimWork sim;
  wfpt::capi::StatsWork stats;
  wfpt::capi::PointwiseWork pw;
};

struct wfpt_ds : wfpt::capi::DsBase {
  int64_t n = 0;
  DevBuf<double> x;
  DevBuf<int32_t> node;
  DevBuf<int64_t> off;
  int32_t n_nodes = 0;
  // the last call on this dataset deferred no trial: the next one runs the
  // level-0 pass + finalize only (run_sum_fast), no slow pass
  mutable bool no_defer = false;
  // the last call on this dataset refined no chunk in-wave: the next one's
  // level-0 pass is the lean kernel (kPassLean)
  mutable bool no_tree = false;
  // fraction of chunks that refined in-wave in the last call: up to
  // lean_tree_max the lean pass still runs, the engine redoing those chunks
  mutable double tree_frac = 1.0;
  bool input_order = false;  // WFPT_DS_INPUT_ORDER: trials kept in the caller's order
  // heavy-chunk record (wfpt_internal.h: Split), double-buffered by call
  // parity: the engine writes [1 - parity] while it reads [parity]
  int64_t nw = 0;
  int split_cap = 0;
  DevBuf<unsigned char> hpred[2];
  DevBuf<int> hlist[2];
  DevBuf<int> hcount;  // [4]: class 1 by parity, then class 2 by parity
  DevBuf<double> hlp;
  DevBuf<int> hmeta;
  DevBuf<int> hdone;
  DevBuf<int> hzn;
  mutable int nsplit = 0;  // class-1 chunks the next call splits
  mutable int nsplit2 = 0; // class-2 chunks the next call splits
  mutable int parity = 0;
  // device: the caller's index of each stored trial (per-trial outputs of the
  // diagnostic calls are returned in the caller's order; kept in HBM, not in
  // host memory: 8 B per trial); null = identity (WFPT_DS_INPUT_ORDER)
  DevBuf<int64_t> perm;
  // host: the lean pass's dispatch index of a dataset in stored order (first
  // |rt| of every chunk, 8 B per chunk; wfpt_lean_tables.hpp: LeanIndex).
  // Empty for input-order and per-node datasets.
  std::vector<double> chunk_first;
  wfpt::LeanIndex lean_index{};
  bool identity = true;  // stored order == the caller's order (perm never allocated)
  void free_device() override {
    wfpt::capi::release_all(x, node, off, perm, hpred[0], hpred[1], hlist[0], hlist[1], hcount,
                            hlp, hmeta, hdone, hzn);
  }
};

namespace wfpt {
namespace capi {

inline Params to_params(const wfpt_params* p) {
  return Params{p->v, p->sv, p->a, p->z, p->sz, p->t, p->st, p->p_outlier};
}
inline Knobs to_knobs(const wfpt_knobs* k) {  // use_adaptive: `bint` in the reference signatures
  return Knobs{k->err, k->n_st, k->n_sz, k->use_adaptive != 0, k->simps_err, k->w_outlier};
}
inline bool p_outlier_in_range(double p) { return (p >= 0) & (p <= 1); }  // wfpt.pyx:50-51

// ---- defined in capi_core.cpp --------------------------------------------
// Paths without finalize_kernel (pdf_array, the sampler): clear the overflow
// flag before the launch, copy it back (and clear it again) before the sync.
int begin_status(wfpt_ctx* c);
int fetch_status(wfpt_ctx* c);
int check_status(wfpt_ctx* c);
int check_status_value(double enc);
bool engine_family(const Params& P, const Knobs& K);
int run_sum(wfpt_ctx* c, const double* dx, int64_t n, const Params& P, const Knobs& K,
            double* out, int part = kPassAll, const wfpt_ds* d = nullptr,
            double* mirror = nullptr);
int finish_profile(wfpt_ctx* c);
int wait_word(wfpt_ctx* c, const void* word);
int wait_result(wfpt_ctx* c, const double* r);
bool res_deferred(const double* r);
int decode_sum(wfpt_ctx* c, const double* r, double* out, bool* deferred = nullptr);
void split_advance(const wfpt_ds* d, bool engine, const double* r);
void note_tree(const wfpt_ds* d, const double* r);
bool lean_predicted(const wfpt_ctx* c, const wfpt_ds* d);
int nodes_check(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* per_node, const wfpt_knobs* k,
                const void* out);
int nodes_launch(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* per_node, const Knobs& K,
                 NodeSum* ns, int32_t n_tables = 1);
int nodes_recover(wfpt_ctx* c, int rc);

// wiener_like_multi's scoring over device arrays: dptr[j] (j = v, sv, a, z, sz,
// t, st) holds m values, or is null for the scalar scal[j]. A uniform adaptive /
// direct family (sz and st scalar) takes the level-0 pass + deferred records
// (launch_multi_fast), anything else the generic per-trial kernel.
// multi_score_reserve sizes the workspaces for `total` trials (lp: per-trial
// terms; records: the fast path's deferred records) and uploads the 7-wide
// pointer / scalar tables of slots [0, nslots), which stay alive for the call.
int multi_score_reserve(wfpt_ctx* c, int64_t total, int nslots, double* const* dptr,
                        const double* scal, bool lp = true, bool records = true);
// The scoring launch over m trials with the tables of `slot`: block sums into
// c->part / c->zero, terms into lp (nullable on the generic path).
int multi_score_launch(wfpt_ctx* c, const double* dx, int64_t m, int slot, double* const dptr[7],
                       const double scal[7], const Knobs& K, double p_outlier, double* lp);
int multi_score(wfpt_ctx* c, const double* dx, int64_t m, double* const dptr[7],
                const double scal[7], const Knobs& K, double p_outlier);
// Closes the profile bracket, adds the m trials' block sums in finalize's fixed
// order and waits: *out = the sum (a zero density's log, -inf, is a term of it).
int multi_finish(wfpt_ctx* c, int64_t m, double* out);
// The given ones of `count` host arrays of n doubles into c->marr, packed: dev[j]
// = array j's copy or null. substitute (nullable) goes up in place of the last.
int upload_multi_arrays(wfpt_ctx* c, const double* const* arrays, int count, int64_t n,
                        const double* substitute, double** dev);
// The per-group sums of a batch call (RL nodes, regression groups) whose G
// groups lie one after the other (off_host / off_dev: G + 1 offsets). field[f]:
// the device array backing parameter f for every trial, or null for a scalar of
// the pass (sz and st then come from the group's row). One launch per run of
// groups that share those scalars (compared exactly), then the per-group sums
// (npart: scratch), a finalize over no partials and the copy to out_logp.
int score_runs(wfpt_ctx* c, const double* dx, double* const field[7], const wfpt_params* rows,
               int32_t G, const int64_t* off_host, const int64_t* off_dev,
               DevBuf<double>& npart, const Knobs& K, double p_outlier, double* out_logp);
// off[r] = counts[0] + ... + counts[r - 1] (R + 1 entries); a negative count
// is "<name>: negative count in row r".
int counts_to_offsets(const char* name, const int64_t* counts, int64_t R,
                      std::vector<int64_t>* off);
// The checks of a regression term list that need no data set (defined in
// capi_reg.cpp): max_param 6 for the regression entries, 7 (alpha) for the RL
// regression entries.
int reg_check_terms(const wfpt_reg_term* terms, int32_t n_terms, int max_param = 6);
// The learning rate of the unbounded alpha as every RL entry forms it
// (wfpt.pyx:123-125), defined in capi_rl.cpp.
double rl_rate(double alpha);

// The model-comparison pass, shared by the three
// wfpt_pointwise_* entries; the context is locked by the caller.
// Sweeps per tile: max(1, max_workspace / (8 len)), 1 GiB when max_workspace
// <= 0, at most S and at most (INT32_MAX / 2) / nodes tables per node call.
int64_t pointwise_tile(int64_t max_workspace, int64_t len, int64_t S, int64_t nodes);
// Sizes and clears the state of `len` trials.
int pointwise_begin(wfpt_ctx* c, int64_t len);
// T sweeps of terms (sweep t's trial i at lp[t len + i], device memory) into the
// state; enqueued on the context's stream, behind the kernels that wrote lp.
int pointwise_add(wfpt_ctx* c, const double* lp, int64_t T);
// The statistics after S sweeps: out_stats[f len + to[i]] = field f (lppd,
// p_waic, mean, n_inf) of stored trial i; to (host, nullable: identity) is the
// caller's position of a stored trial. *out_ninf_total = the n_inf summed.
// Returns after the stream has drained.
int pointwise_finish(wfpt_ctx* c, int64_t S, const int64_t* to, double* out_stats,
                     int64_t* out_ninf_total);
// A pass that runs no device work (p_outlier outside [0, 1]: every term is
// -inf): the statistics of `len` trials that saw S zero densities each.
void pointwise_all_inf(int64_t len, int64_t S, double* out_stats, int64_t* out_ninf_total);

// ---- defined in capi_sim.cpp ----------------------------------------------
// The percentile arguments of a statistics request: "<name>: ..." WFPT_ERR_ARG.
int stats_check_q(const char* name, const double* q, int32_t nq, const double* out);
// The statistics of R rows of draws that are already in device memory (row r
// is d_rts[off[r] .. off[r + 1]), off on the host) into host_out [R x (8 + 2
// nq)]: plans the tiers by row length, launches them on the context's stream
// and returns after it has drained. The context is locked; c->sim.off is used.
int stats_device_rows(wfpt_ctx* c, const char* name, const double* d_rts, const int64_t* off,
                      int64_t R, const double* q, int32_t nq, double* host_out);

}  // namespace capi
}  // namespace wfpt

#pragma GCC visibility pop
