// capi_core.cpp — C ABI of the MI355X WFPT engine (include/wfpt_amd.h): the
// context, the plain datasets and the likelihoods over them, the profiling and
// debug entries, and the helpers every family's unit shares (capi_internal.hpp).
//
// Host runtime: one context per GPU (HIP stream, grow-only device workspaces,
// pinned result slot, optional RCCL communicator), resident datasets, and the
// call sequences  fast pass -> slow pass -> finalize  per likelihood. The last
// kernel writes {sum, #zeros, status} straight into mapped pinned host memory
// (no copy, no memset, no stream sync).
// Calls into one context are serialised by its mutex; the ctypes binding
// releases the GIL around every call.
#include <cstdio>

#include "capi_internal.hpp"
#include "rl_internal.h"  // launch_rl_node_sum: the per-group sums of score_runs

using namespace wfpt::capi;

constexpr int64_t kSplitCap = 16384;  // heavy chunks a dataset records per call (both classes)
// class-2 heavy chunks (Split::n2) are split while the dataset's heavy chunks
// are at most 1 / kHeavyFewDiv of its chunks: then they are the launch's
// tail; when many chunks are heavy, splitting them only adds waves
constexpr int64_t kHeavyFewDiv = 16;
// dispatch rounds up to which the lean pass's list of first chunks is used
// (capi_internal.hpp: lean_first_max)
constexpr int64_t kLeanFirstRounds = 8;

namespace wfpt {
namespace capi {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

bool roctx_on() {
  static const bool on = [] {
    const char* e = std::getenv("WFPT_ROCTX");
    return !(e && std::strcmp(e, "0") == 0);
  }();
  return on;
}

void ds_register(wfpt_ctx* c, DsBase* d) {
  d->ctx = c;
  c->dsets.push_back(d);
}

void ds_destroy(DsBase* d) {
  if (!d) return;
  if (wfpt_ctx* c = d->ctx) {
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->dsets.erase(std::remove(c->dsets.begin(), c->dsets.end(), d), c->dsets.end());
    d->free_device();
  }
  delete d;
}

int begin_status(wfpt_ctx* c) {
  HIP_TRY(hipMemsetAsync(c->status.p, 0, sizeof(int), c->stream));
  return WFPT_OK;
}
int fetch_status(wfpt_ctx* c) {
  HIP_TRY(hipMemcpyAsync(c->host_status.h, c->status.p, sizeof(int), hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipMemsetAsync(c->status.p, 0, sizeof(int), c->stream));  // 0 at rest
  return WFPT_OK;
}
// the raw device flag word (kFlagDepth | kFlagBudget) in the encoded form
static double encode_status(int st) {
  return (double)(st & wfpt::kFlagDepth) + ((st & wfpt::kFlagBudget) ? wfpt::kBudgetUnit : 0.0);
}
int check_status(wfpt_ctx* c) { return check_status_value(encode_status(*c->host_status.h)); }

// Deferred-trial state for adaptive calls over up to n trials (grow-only).
static int reserve_work(wfpt_ctx* c, int64_t n, wfpt::Work* W) {
  const int64_t nw = std::max<int64_t>((n + 63) / 64, 1);
  const int64_t ns = nw * 64;
  HIP_TRY(c->wl.reserve(ns));
  HIP_TRY(c->wl_n.reserve(nw));
  HIP_TRY(c->rflag.reserve(ns));
  if (c->redo.cap < (size_t)nw) {
    HIP_TRY(c->redo.reserve(nw));
    HIP_TRY(hipMemsetAsync(c->redo.p, 0, c->redo.cap, c->stream));
  }
  W->redo = c->redo.p;
  W->tree_any = c->tree_any.p;
  W->wl = c->wl.p;
  W->wl_n = c->wl_n.p;
  W->rflag = c->rflag.p;
  W->prof = c->prof.p;
  W->phase = c->phase.p;
  W->nslots = ns;
  return WFPT_OK;
}

// Status words are 0 at rest: finalize_kernel resets the device flag after
// reporting it, and the other paths clear it before their launch. enc:
// #depth errors + kBudgetUnit * #budget errors (summed over ranks).
int check_status_value(double enc) {
  if (enc == 0) return WFPT_OK;
  const double peers = std::floor(enc / wfpt::kPeerFailUnit);
  enc -= peers * wfpt::kPeerFailUnit;
  const double budget = std::floor(enc / wfpt::kBudgetUnit);
  const double depth = enc - budget * wfpt::kBudgetUnit;
  std::string msg;
  if (peers > 0)
    msg = std::to_string((long long)peers) +
          " rank(s) failed before the likelihood exchange (their own call returned the error)";
  if (depth > 0) {
    if (!msg.empty()) msg += "; ";
    msg += "adaptive Simpson refinement deeper than WFPT_MAX_DEPTH=" +
           std::to_string(WFPT_MAX_DEPTH) + " levels (lower n_st/n_sz or raise simps_err)";
  }
  if (budget > 0) {
    if (!msg.empty()) msg += "; ";
    msg += "a trial exceeded WFPT_EVAL_BUDGET pdf_sv evaluations (raise simps_err)";
  }
  return fail((depth > 0 || budget > 0) ? WFPT_ERR_UNSUPPORTED : WFPT_ERR_COMM, msg);
}

// The dataset's heavy-chunk state for one engine call (null: no split, no
// record).
static wfpt::Split split_of(const wfpt_ds* d) {
  wfpt::Split S{};
  if (!d || !d->hcount.p) return S;
  const int cur = d->parity, nx = 1 - cur;
  S.n = d->nsplit;
  S.n2 = d->nsplit2;
  S.cap = d->split_cap;
  S.list = d->hlist[cur].p;
  S.pred = d->hpred[cur].p;
  S.next_pred = d->hpred[nx].p;
  S.next_list = d->hlist[nx].p;
  S.next_n = d->hcount.p + nx;
  S.lp = d->hlp.p;
  S.meta = d->hmeta.p;
  S.done = d->hdone.p;
  S.zn = d->hzn.p;
  return S;
}

// After a call's result r is in host memory: the next call splits the heavy
// chunks this one recorded (engine calls), or none.
void split_advance(const wfpt_ds* d, bool engine, const double* r) {
  if (!d) return;
  if (!engine || !d->hcount.p) {
    d->nsplit = 0;
    d->nsplit2 = 0;
    return;
  }
  const int half = d->split_cap / 2;
  d->nsplit = (int)std::min<double>(r[5], (double)half);
  const int n2 = (int)std::min<double>(r[7], (double)half);
  d->nsplit2 = (int64_t)(d->nsplit + n2) * kHeavyFewDiv <= d->nw ? n2 : 0;
  d->parity = 1 - d->parity;
}

bool engine_family(const wfpt::Params& P, const wfpt::Knobs& K) {
  const int m = wfpt::select_mode(P.sz, P.st, K.use_adaptive);
  return m >= wfpt::kAdaptT && m <= wfpt::kAdaptTZ;
}

// The context's decision table for err (the caller holds the context's lock).
// Outside decide32's range of err the uniform site keeps what it had before
// the table: no wave settled there (a table that never answers).
static const wfpt::DecisionTab* decision_tab_of(wfpt_ctx* c, double err) {
  uint64_t key;
  std::memcpy(&key, &err, sizeof key);
  if (!c->dtab_valid || c->dtab_err != key) {
    if (err > 1e-30 && err < 1e30) wfpt::decision_tab(err, c->dtab);
    else wfpt::decision_tab_clear(c->dtab);
    c->dtab_err = key;
    c->dtab_valid = true;
  }
  return &c->dtab;
}

// Likelihood sum over device x[n]: adaptive / direct families run the level-0
// pass and (part & kPassDeferred) the deferred-trial pass, fixed Simpson one
// trial kernel; then finalize writes {sum, zeros, errors, deferred} + the
// completion word to `out` (mapped host memory or device).
int run_sum(wfpt_ctx* c, const double* dx, int64_t n, const wfpt::Params& P,
            const wfpt::Knobs& K, double* out, int part, const wfpt_ds* d,
            double* mirror) {
  const int64_t nb = wfpt::partials_for(n, P, K);
  HIP_TRY(c->part.reserve(std::max<int64_t>(nb, 1)));
  HIP_TRY(c->zero.reserve(std::max<int64_t>(nb, 1)));
  wfpt::Work W;
  if (int rc = reserve_work(c, n, &W)) return rc;
  const bool adaptive = wfpt::has_deferred_pass(P, K);
  if (part & wfpt::kPassFast) {  // a call sequence starts
    c->path = 0;
    c->first_last.n = 0;
  }
  if (c->count && (part & wfpt::kPassFast))
    HIP_TRY(hipMemsetAsync(c->evals.p, 0, sizeof(unsigned long long), c->stream));
  // profiling: ev0..ev1 bracket the level-0 fast kernel (the dominant kernel,
  // lean_kernel, engine_kernel or direct_kernel in a rocprofv3 trace)
  const bool prof = c->profile && (part & wfpt::kPassFast);
  if (prof) HIP_TRY(hipEventRecord(c->ev0, c->stream));
  // heavy-chunk splitting belongs to full engine calls (not the lean / redo
  // passes)
  const bool eng = d && d->hcount.p && engine_family(P, K) &&
                   !(part & (wfpt::kPassLean | wfpt::kPassRedo));
  // one block of trials, level-0 pass only (direct family, or the lean pass):
  // level 0 and finalize in one launch (WFPT_SMALL=0: two launches)
  const bool level0_only = adaptive && (engine_family(P, K)
                                            ? part == (wfpt::kPassFast | wfpt::kPassLean)
                                            : part == wfpt::kPassFast);
  const bool direct = adaptive && !engine_family(P, K);
  if (c->small && level0_only && !prof && !c->count && !mirror) {
    const int sk = wfpt::launch_small(dx, n, P, K, c->part.p, c->zero.p, c->status.p, W, out,
                                      c->seq + 1, c->tree_any.p, c->stream, c->trial);
    if (sk != wfpt::kSmallNone) {
      ++c->seq;
      HIP_TRY(hipGetLastError());
      c->path |= WFPT_PATH_SMALL | (direct ? WFPT_PATH_DIRECT : WFPT_PATH_LEAN) |
                 (sk == wfpt::kSmallSplit ? WFPT_PATH_SMALL_SPLIT : 0);
      return WFPT_OK;
    }
  }
  const wfpt::Split S = eng ? split_of(d) : wfpt::Split{};
  // the 2-D family's lean pass over more than one dispatch round of a dataset
  // in stored order: the chunks that hold a breakpoint of the decision table
  // go first (one binary search per boundary, t node and finite upper edge of
  // a piece over the host index: 60 at err = 1e-4)
  const bool lean2d = (part & wfpt::kPassLean) &&
                      wfpt::select_mode(P.sz, P.st, K.use_adaptive) == wfpt::kAdaptTZ;
  if (lean2d && c->lean_first && d && d->lean_index.first && d->nw > c->lean_first_min &&
      d->nw <= c->lean_first_max)
    wfpt::lean_first_search(*decision_tab_of(c, K.err), d->lean_index, P.a, P.t, P.st,
                            c->first_last);
  wfpt::launch_trials(c->trial ? 3 : 0, adaptive ? part : wfpt::kPassAll, dx, n, P, K, c->part.p,
                      c->zero.p, c->count ? c->evals.p : nullptr, c->status.p, 0, W, c->stream,
                      prof ? c->ev1 : nullptr, &S, c->trial,
                      // (only the 2-D family's lean kernel reads the table and the list)
                      lean2d ? decision_tab_of(c, K.err) : nullptr,
                      lean2d ? &c->first_last : nullptr);
  if (!adaptive) {
    c->path |= WFPT_PATH_FIXED;
  } else {
    if (part & wfpt::kPassFast)
      c->path |= direct ? WFPT_PATH_DIRECT
                        : (part & wfpt::kPassLean)
                              ? WFPT_PATH_LEAN
                              : (WFPT_PATH_ENGINE | (S.n + S.n2 > 0 ? WFPT_PATH_SPLIT : 0));
    if (!direct && (part & wfpt::kPassRedo)) c->path |= WFPT_PATH_REDO;
    if (part & wfpt::kPassDeferred) c->path |= WFPT_PATH_FOLD;
  }
  HIP_TRY(hipGetLastError());
  wfpt::launch_finalize(c->part.p, c->zero.p, nb, adaptive ? 1 : 0,
                        c->status.p, out, ++c->seq, c->stream, eng ? S.next_n : nullptr,
                        eng ? d->hcount.p + d->parity : nullptr, c->tree_any.p, mirror, c->fin.p,
                        c->fin_ticket.p);
  HIP_TRY(hipGetLastError());
  return WFPT_OK;
}

int finish_profile(wfpt_ctx* c) {
  if (c->profile) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->k_ms += ms;
    c->launches += 1;
  }
  if (c->count) {
    unsigned long long ev = 0;
    HIP_TRY(hipMemcpy(&ev, c->evals.p, sizeof(ev), hipMemcpyDeviceToHost));
    c->n_evals += (int64_t)ev;
  }
  return WFPT_OK;
}

// Waits for the completion word `word` (mapped host memory) to reach c->seq:
// the last kernel of a call writes it after its results (a stream sync's
// wake-up costs several microseconds per call). Every 4096 polls the stream is
// asked whether it failed; after 5 s, or if the stream is idle without the
// word, it falls back to a stream sync so a device error is reported, never a
// stale number.
int wait_word(wfpt_ctx* c, const void* word) {
  if (c->spin) {
    // the word is the device's system-scope release store (fin_write,
    // segment_publish_kernel, publish_*): read it with acquire semantics, so
    // every result store the device ordered before it is visible below
    const unsigned long long* w = reinterpret_cast<const unsigned long long*>(word);
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 1;; ++it) {
      if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == c->seq) {
        if (c->profile) HIP_TRY(hipEventSynchronize(c->ev1));
        return WFPT_OK;
      }
      if ((it & 4095u) == 0) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q != hipSuccess && q != hipErrorNotReady)
          return fail(WFPT_ERR_HIP, std::string("likelihood kernels: ") + hipGetErrorString(q));
        if (q == hipSuccess && __atomic_load_n(w, __ATOMIC_ACQUIRE) != c->seq)
          break;  // idle: let the stream sync decide
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) break;
      }
    }
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (*reinterpret_cast<const volatile unsigned long long*>(word) != c->seq)
    return fail(WFPT_ERR_HIP, "the call's completion word was not written");
  return WFPT_OK;
}

int wait_result(wfpt_ctx* c, const double* r) {
  if (r == c->mres.h) return wait_word(c, r + 4);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return WFPT_OK;
}

// Decodes {sum, zeros, errors, deferred} from host memory `r` of a finished
// call; *deferred (if given) = the level-0 pass deferred trials.
bool res_deferred(const double* r) { return ((int)r[3] & wfpt::kResDeferred) != 0; }
static bool res_tree(const double* r) { return ((int)r[3] & wfpt::kResTree) != 0; }
int decode_sum(wfpt_ctx* c, const double* r, double* out, bool* deferred) {
  if (deferred) *deferred = res_deferred(r);
  if (int rc = wfpt_decode_result(r, out)) return rc;
  return finish_profile(c);
}

// The dataset's in-wave refinement record from a finished call's result.
void note_tree(const wfpt_ds* d, const double* r) {
  d->no_tree = !res_tree(r);
  d->tree_frac = d->nw > 0 ? r[6] / (double)d->nw : 0.0;
}
// The lean level-0 pass is predicted to pay: nothing refined last time, or
// few enough chunks that their engine redo beats an engine pass over all.
bool lean_predicted(const wfpt_ctx* c, const wfpt_ds* d) {
  return c->lean && (d->no_tree || d->tree_frac <= c->lean_tree_max);
}

// Waits for a resident call, updates the dataset's predictions from its
// result and decodes it.
static int finish_sum(wfpt_ctx* c, const wfpt_ds* d, const wfpt::Params& P, const wfpt::Knobs& K,
               double* out, bool lean) {
  if (int rc = wait_result(c, c->mres.h)) return rc;
  const bool eng = engine_family(P, K);
  split_advance(d, eng && !lean, c->mres.h);
  bool deferred = true;
  const int rc = decode_sum(c, c->mres.h, out, &deferred);
  if (rc == WFPT_OK) {
    d->no_defer = c->fast_only && !deferred;
    if (eng) note_tree(d, c->mres.h);
  }
  return rc;
}

// Resident-data sums with a predicted call sequence (from the dataset's last
// call), each giving the full sequence's result bit for bit:
//   * no deferred trial predicted: level-0 pass + finalize only (no fold
//     launch). If the pass did defer this time (finalize reports it), the
//     deferred pass and a second finalize run over the intact chunk partials;
//     only that call pays a host round trip.
//   * no in-wave refinement predicted (engine families): the level-0 pass is
//     the lean kernel; chunks that do refine are flagged and the engine's redo
//     pass processes them before the fold (as part of the deferred pass).
// Returns -1 when neither prediction applies (nothing launched).
static int run_sum_fast(wfpt_ctx* c, const wfpt_ds* d, const wfpt::Params& P, const wfpt::Knobs& K,
                 double* out) {
  const int64_t n = d->n;
  if (n <= 0 || !wfpt::has_deferred_pass(P, K)) return -1;
  const bool eng = engine_family(P, K);
  const bool lean = eng && lean_predicted(c, d);
  // a counting call (WFPT_PROF_EVALS) keeps the predicted lean pass, whose
  // counting build tallies its generic-site waves (wfpt_profile_lists); it
  // never takes the level-0-only prediction of the other families
  if (c->count && !lean) return -1;
  const bool fast = c->fast_only && d->no_defer;
  if (!lean && !fast) return -1;
  const int lp = lean ? wfpt::kPassLean : 0;
  double ntree0 = 0.0;  // chunks the first of two launches reported as refined in-wave
  if (!fast) {  // deferred trials expected: the whole sequence at once
    if (int rc = run_sum(c, d->x.p, n, P, K, c->mres.d, wfpt::kPassAll | lp | wfpt::kPassRedo, d))
      return rc;
  } else {
    if (int rc = run_sum(c, d->x.p, n, P, K, c->mres.d, wfpt::kPassFast | lp, d)) return rc;
    if (int rc = wait_result(c, c->mres.h)) return rc;
    if (res_deferred(c->mres.h)) {
      if (int rc = check_status_value(c->mres.h[2])) return rc;
      ntree0 = c->mres.h[6];
      if (int rc = run_sum(c, d->x.p, n, P, K, c->mres.d,
                           wfpt::kPassDeferred | (lean ? wfpt::kPassRedo : 0), d))
        return rc;
    }
  }
  const int rc = finish_sum(c, d, P, K, out, lean);
  // an engine level-0 pass whose deferred trials took a second launch: its own
  // finalize reported (and reset) the refinement count, so the second result
  // holds the deferred pass's alone (0 without a redo pass) and would predict
  // the lean pass for data that refines
  if (rc == WFPT_OK && eng && ntree0 > 0.0) {
    d->no_tree = false;
    d->tree_frac += d->nw > 0 ? ntree0 / (double)d->nw : 0.0;
  }
  return rc;
}

// |a| < |b| with NaN RTs last: a strict weak order for any input (the
// dataset sorts must not hit std::stable_sort's undefined behaviour)
// Stored order of a dataset: |rt| ascending with NaN RTs last (a strict weak
// order for any input), as an unsigned key: |rt|'s bits (monotone for
// non-negative doubles), every NaN one key above +inf. `upper_last` adds the boundary bit
// (x > 0 sorts after x <= 0). Keys are equal exactly when neither comparator
// orders the pair, so a stable sort by key is the stable comparator sort.
static uint64_t order_key(double r, bool upper_last) {
  uint64_t b;
  std::memcpy(&b, &r, sizeof(b));
  b &= 0x7fffffffffffffffull;
  if (std::isnan(r)) b = 0x7ff8000000000000ull;
  return (upper_last && r > 0) ? (b | 0x8000000000000000ull) : b;
}

// Stable sort of idx by key[idx] (ties keep idx order): LSD radix, 16-bit
// digits, for large datasets (C5's 100M trials: seconds instead of a minute
// of comparator sorting); the comparator sort below 64k trials.
static void stable_order(std::vector<int64_t>& idx, const double* rt, bool upper_last) {
  const size_t n = idx.size();
  if (n < (1u << 16)) {
    std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) {
      return order_key(rt[a], upper_last) < order_key(rt[b], upper_last);
    });
    return;
  }
  std::vector<uint64_t> k(n), k2(n);
  std::vector<int64_t> i2(n);
  for (size_t j = 0; j < n; ++j) k[j] = order_key(rt[idx[j]], upper_last);
  std::vector<size_t> cnt(1u << 16);
  for (int sh = 0; sh < 64; sh += 16) {
    std::fill(cnt.begin(), cnt.end(), 0);
    for (size_t j = 0; j < n; ++j) cnt[(k[j] >> sh) & 0xffffu]++;
    if (cnt[(k[0] >> sh) & 0xffffu] == n) continue;  // one digit value: nothing moves
    size_t acc = 0;
    for (auto& c : cnt) {
      const size_t t = c;
      c = acc;
      acc += t;
    }
    for (size_t j = 0; j < n; ++j) {
      const size_t p = cnt[(k[j] >> sh) & 0xffffu]++;
      k2[p] = k[j];
      i2[p] = idx[j];
    }
    k.swap(k2);
    idx.swap(i2);
  }
}

// Per-trial values of a dataset's stored order (device) -> the caller's order
// (host) through the dataset's stored permutation (diagnostic calls only).
static int trials_to_caller(const wfpt_ds* d, const double* dev, double* out) {
  if (d->n <= 0) return WFPT_OK;
  std::vector<double> h(d->n);
  HIP_TRY(hipMemcpy(h.data(), dev, d->n * sizeof(double), hipMemcpyDeviceToHost));
  if (!d->perm.p) {
    std::memcpy(out, h.data(), d->n * sizeof(double));
    return WFPT_OK;
  }
  std::vector<int64_t> perm(d->n);
  HIP_TRY(hipMemcpy(perm.data(), d->perm.p, d->n * sizeof(int64_t), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < d->n; ++i) out[perm[i]] = h[i];
  return WFPT_OK;
}

static int upload(wfpt_ctx* c, const double* x, int64_t n) {
  HIP_TRY(c->x.reserve(std::max<int64_t>(n, 1)));
  if (n > 0)
    HIP_TRY(hipMemcpyAsync(c->x.p, x, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return WFPT_OK;
}

}  // namespace capi
}  // namespace wfpt

extern "C" {

const char* wfpt_last_error(void) { return g_last_error.c_str(); }

int wfpt_result_poison(double r[3]) {
  if (!r) return fail(WFPT_ERR_ARG, "null pointer");
  r[0] = 0.0;
  r[1] = 0.0;
  r[2] = wfpt::kPeerFailUnit;
  return WFPT_OK;
}

int wfpt_decode_result(const double r[3], double* out) {
  if (!r || !out) return fail(WFPT_ERR_ARG, "null pointer");
  if (int rc = check_status_value(r[2])) return rc;
  *out = (r[1] > 0) ? -INFINITY : r[0];  // any zero-density trial: -inf (wfpt.pyx:71-72)
  return WFPT_OK;
}

int wfpt_device_count(int* n) {
  if (!n) return fail(WFPT_ERR_ARG, "null pointer");
  HIP_TRY(hipGetDeviceCount(n));
  return WFPT_OK;
}

int wfpt_open(int device, wfpt_ctx** out) {
  if (!out) return fail(WFPT_ERR_ARG, "null pointer");
  int nd = 0;
  HIP_TRY(hipGetDeviceCount(&nd));
  if (device < 0 || device >= nd)
    return fail(WFPT_ERR_ARG, "device " + std::to_string(device) + " not present (" +
                                  std::to_string(nd) + " visible)");
  DeviceGuard g(device);
  HIP_TRY(hipSetDevice(device));
  auto* c = new wfpt_ctx();
  c->device = device;
  if (const char* sm = std::getenv("WFPT_SYNC")) c->spin = std::strcmp(sm, "stream") != 0;
  if (const char* nm = std::getenv("WFPT_NODES")) c->nodes_generic = std::strcmp(nm, "generic") == 0;
  if (const char* ns = std::getenv("WFPT_NODE_SPLIT")) c->node_split = std::strcmp(ns, "0") != 0;
  if (const char* nq = std::getenv("WFPT_NODE_SPEC")) c->node_spec = std::strcmp(nq, "0") != 0;
  if (const char* ht = std::getenv("WFPT_HOST_TIMING")) c->host_timing = std::strcmp(ht, "0") != 0;
  if (const char* nt = std::getenv("WFPT_NODE_TABLE_DEV"))
    c->node_table_dev = std::strcmp(nt, "0") != 0;
  if (const char* fm = std::getenv("WFPT_FAST_ONLY")) c->fast_only = std::strcmp(fm, "0") != 0;
  if (const char* lm = std::getenv("WFPT_LEAN")) c->lean = std::strcmp(lm, "0") != 0;
  if (const char* sm = std::getenv("WFPT_SMALL")) c->small = std::strcmp(sm, "0") != 0;
  if (const char* lt = std::getenv("WFPT_LEAN_TREE")) c->lean_tree_max = std::atof(lt);
  if (const char* lf = std::getenv("WFPT_LEAN_FIRST")) c->lean_first = std::strcmp(lf, "0") != 0;
  {  // the list pays from more than one dispatch round up to kLeanFirstRounds of them
    const int64_t slots = wfpt::lean_wave_slots();
    c->lean_first_min = slots > 0 ? slots : INT64_MAX;
    c->lean_first_max = slots > 0 ? slots * kLeanFirstRounds : 0;
    if (const char* fm = std::getenv("WFPT_LEAN_FIRST_MIN")) c->lean_first_min = std::atoll(fm);
  }
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&c->ev0);
  if (e == hipSuccess) e = hipEventCreate(&c->ev1);
  // the one-off device words, zeroed
  auto words = [&](auto& b, size_t n) {
    if (e == hipSuccess) e = b.reserve(n);
    if (e == hipSuccess) e = hipMemset(b.p, 0, n * sizeof(*b.p));
  };
  words(c->evals, 1), words(c->status, 1), words(c->n_defer, 4), words(c->ncnt, 4);
  words(c->tree_any, 1), words(c->fin, 3 * 64), words(c->fin_ticket, 1), words(c->ar, 8);
  words(c->prof, 16), words(c->phase, 8 * wfpt::kPhaseWaves);
  if (e == hipSuccess) e = c->host_status.reserve(1);
  if (e == hipSuccess) e = c->mres.reserve(8);
  if (e == hipSuccess) std::memset(c->mres.h, 0, 8 * sizeof(double));
  if (e != hipSuccess) {
    wfpt_close(c);
    return fail(WFPT_ERR_HIP, std::string("wfpt_open: ") + hipGetErrorString(e));
  }
  *out = c;
  return WFPT_OK;
}

void wfpt_close(wfpt_ctx* c) {
  if (!c) return;
  if (c->host_timing && c->ht_calls > 0)
    std::fprintf(stderr,
                 "wfpt host timing over %lld multi-table node calls (us per call): rows %.1f, "
                 "launches %.1f, wait %.1f, copy-out %.1f, total %.1f\n",
                 (long long)c->ht_calls, c->ht[0] / c->ht_calls / 1e3, c->ht[1] / c->ht_calls / 1e3,
                 c->ht[2] / c->ht_calls / 1e3, c->ht[3] / c->ht_calls / 1e3,
                 c->ht[4] / c->ht_calls / 1e3);
  DeviceGuard g(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  // detached: destroying a dataset later frees only its host part
  for (DsBase* d : c->dsets) {
    d->free_device();
    d->ctx = nullptr;
  }
  c->dsets.clear();
  if (c->comm) (void)ncclCommDestroy(c->comm);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;  // the owning members free the device memory: still inside the guard, after the sync
}

void wfpt_shard_range(int64_t n, int nranks, int rank, int64_t* lo, int64_t* hi) {
  if (nranks < 1) nranks = 1;
  const int64_t base = n / nranks, rem = n % nranks;
  const int64_t l = rank * base + std::min<int64_t>(rank, rem);
  *lo = l;
  *hi = l + base + (rank < rem ? 1 : 0);
}

int wfpt_dataset_create(wfpt_ctx* c, const double* rt, int64_t n, const int32_t* node_id,
                        int32_t n_nodes, wfpt_ds** out) {
  return wfpt_dataset_create_ex(c, rt, n, node_id, n_nodes, 0, out);
}

int wfpt_dataset_create_ex(wfpt_ctx* c, const double* rt, int64_t n, const int32_t* node_id,
                           int32_t n_nodes, int flags, wfpt_ds** out) {
  if (!c || !out || (n > 0 && !rt) || n < 0) return fail(WFPT_ERR_ARG, "bad dataset arguments");
  if (flags & ~WFPT_DS_INPUT_ORDER) return fail(WFPT_ERR_ARG, "unknown dataset flags");
  if (node_id && n_nodes <= 0) return fail(WFPT_ERR_ARG, "node ids need n_nodes > 0");
  WFPT_RANGE("wfpt_dataset_create_ex");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  // host-side layout: group by node, order by |rt| inside a node so that each
  // wavefront sees one series branch / similar quadrature depth.
  const bool keep_order = (flags & WFPT_DS_INPUT_ORDER) ||
                          (std::getenv("WFPT_DATASET_ORDER") &&
                           std::strcmp(std::getenv("WFPT_DATASET_ORDER"), "input") == 0);
  std::vector<int64_t> idx(n);
  for (int64_t i = 0; i < n; ++i) idx[i] = i;
  std::vector<int64_t> off;
  if (node_id) {
    for (int64_t i = 0; i < n; ++i)
      if (node_id[i] < 0 || node_id[i] >= n_nodes)
        return fail(WFPT_ERR_ARG, "node id out of range at trial " + std::to_string(i));
    std::vector<int64_t> cnt(n_nodes + 1, 0);
    for (int64_t i = 0; i < n; ++i) cnt[node_id[i] + 1]++;
    for (int32_t j = 0; j < n_nodes; ++j) cnt[j + 1] += cnt[j];
    off = cnt;
    // |rt| order first (stable), then a stable counting placement by node:
    // grouped by node, |rt|-ordered inside a node, ties in input order
    std::vector<int64_t> ord(n);
    for (int64_t i = 0; i < n; ++i) ord[i] = i;
    if (!keep_order) stable_order(ord, rt, false);
    std::vector<int64_t> pos(cnt.begin(), cnt.end() - 1);
    for (int64_t q : ord) idx[pos[node_id[q]]++] = q;
  } else if (!keep_order) {
    // boundary first (x > 0 is the upper boundary, pdf.pxi:116), then |rt|:
    // the lean pass keeps a wave's root z grid in scalar registers when the
    // wave holds one boundary (wfpt_level0.hip: lean_kernel)
    // (NaN RTs last in their group: a strict weak order for any input)
    stable_order(idx, rt, true);
  }
  std::vector<double> hx(n);
  std::vector<int32_t> hn(node_id ? n : 0);
  for (int64_t i = 0; i < n; ++i) {
    hx[i] = rt[idx[i]];
    if (node_id) hn[i] = node_id[idx[i]];
  }
  auto* d = new wfpt_ds();
  d->n = n;
  d->input_order = (flags & WFPT_DS_INPUT_ORDER) != 0;
  d->n_nodes = node_id ? n_nodes : 0;
  hipError_t e = upload_vec(d->x, hx);
  d->identity = !((!keep_order || node_id) && n > 0);
  if (e == hipSuccess && !d->identity) e = upload_vec(d->perm, idx);
  if (e == hipSuccess && node_id) e = upload_vec(d->node, hn);
  if (e == hipSuccess && node_id) e = upload_vec(d->off, off);
  // heavy-chunk record (Split): lists sized for up to kSplitCap chunks
  d->nw = (n + 63) / 64;
  if (!node_id && !keep_order && n > 0) {  // stored order: the lean pass's dispatch index
    d->chunk_first.resize(d->nw);
    wfpt::lean_index(hx.data(), n, d->chunk_first.data(), d->lean_index);
  }
  d->split_cap = (int)std::min<int64_t>(std::max<int64_t>(d->nw, 1), kSplitCap);
  const size_t cap = d->split_cap;
  auto zeroed = [&](auto& b, size_t count) {
    if (e == hipSuccess) e = b.reserve(count);
    if (e == hipSuccess) e = hipMemset(b.p, 0, count * sizeof(*b.p));
  };
  for (int k = 0; k < 2; ++k) {
    zeroed(d->hpred[k], std::max<int64_t>(d->nw, 1));
    if (e == hipSuccess) e = d->hlist[k].reserve(cap);
  }
  zeroed(d->hcount, 4);
  if (e == hipSuccess) e = d->hlp.reserve(cap * 64);
  if (e == hipSuccess) e = d->hmeta.reserve(cap * 64);
  zeroed(d->hdone, cap);
  zeroed(d->hzn, cap);
  if (e != hipSuccess) {
    delete d;  // frees what was allocated (this context's device is current)
    return fail(WFPT_ERR_HIP, std::string("wfpt_dataset_create: ") + hipGetErrorString(e));
  }
  ds_register(c, d);
  *out = d;
  return WFPT_OK;
}

void wfpt_dataset_destroy(wfpt_ds* d) { ds_destroy(d); }

int64_t wfpt_dataset_size(const wfpt_ds* d) { return d ? d->n : -1; }

int wfpt_wiener_like(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* p, const wfpt_knobs* k,
                     double* out) {
  if (!c || !d || !p || !k || !out) return fail(WFPT_ERR_ARG, "null pointer");
  if (d->ctx != c) return fail(WFPT_ERR_ARG, "dataset belongs to another context");
  const wfpt::Params P = to_params(p);
  const wfpt::Knobs K = to_knobs(k);
  if (!p_outlier_in_range(P.p_outlier)) {  // wfpt.pyx:63-64
    *out = -INFINITY;
    return WFPT_OK;
  }
  WFPT_RANGE("wfpt_wiener_like");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const int rc = run_sum_fast(c, d, P, K, out);
  if (rc >= 0) return rc;
  if (int rc2 = run_sum(c, d->x.p, d->n, P, K, c->mres.d, wfpt::kPassAll, d)) return rc2;
  return finish_sum(c, d, P, K, out, false);
}

int wfpt_wiener_like_trials(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* p,
                            const wfpt_knobs* k, double* out, double* out_trial) {
  if (!c || !d || !p || !k || !out || (!out_trial && d && d->n > 0))
    return fail(WFPT_ERR_ARG, "null pointer");
  if (d->ctx != c) return fail(WFPT_ERR_ARG, "dataset belongs to another context");
  const wfpt::Params P = to_params(p);
  const wfpt::Knobs K = to_knobs(k);
  if (!p_outlier_in_range(P.p_outlier)) {  // wfpt.pyx:63-64: no trial is scored
    *out = -INFINITY;
    for (int64_t i = 0; i < d->n; ++i) out_trial[i] = -INFINITY;
    return WFPT_OK;
  }
  WFPT_RANGE("wfpt_wiener_like_trials");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HIP_TRY(c->lp.reserve(std::max<int64_t>(d->n, 1)));
  c->trial = c->lp.p;
  int rc = run_sum_fast(c, d, P, K, out);
  if (rc < 0) {
    rc = run_sum(c, d->x.p, d->n, P, K, c->mres.d, wfpt::kPassAll, d);
    if (rc == WFPT_OK) rc = finish_sum(c, d, P, K, out, false);
  }
  c->trial = nullptr;
  if (rc != WFPT_OK) return rc;
  return trials_to_caller(d, c->lp.p, out_trial);
}

int wfpt_dataset_order(const wfpt_ds* d, int64_t* perm) {
  if (!d || (!perm && d->n > 0)) return fail(WFPT_ERR_ARG, "null pointer");
  if (d->identity) {  // identity order (input-order or empty dataset): host only
    for (int64_t i = 0; i < d->n; ++i) perm[i] = i;
    return WFPT_OK;
  }
  if (!d->ctx || !d->perm.p) return fail(WFPT_ERR_ARG, "the dataset's context was closed");
  wfpt_ctx* c = d->ctx;
  std::lock_guard<std::mutex> lk(c->mu);  // serialised with calls on the context
  DeviceGuard g(c->device);
  HIP_TRY(hipMemcpyAsync(perm, d->perm.p, d->n * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return WFPT_OK;
}

int wfpt_debug_partials(wfpt_ctx* c, double* part, int32_t* zero, int64_t n) {
  if (!c || n < 0 || (n > 0 && (!part || !zero))) return fail(WFPT_ERR_ARG, "bad arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if ((size_t)n > c->part.cap || (size_t)n > c->zero.cap)
    return fail(WFPT_ERR_ARG, "more partials requested than the last calls wrote");
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n > 0) {
    HIP_TRY(hipMemcpy(part, c->part.p, n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(zero, c->zero.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return WFPT_OK;
}

int wfpt_last_path(wfpt_ctx* c, int* path) {
  if (!c || !path) return fail(WFPT_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(c->mu);
  *path = c->path;
  return WFPT_OK;
}

int wfpt_wiener_like_host(wfpt_ctx* c, const double* x, int64_t n, const wfpt_params* p,
                          const wfpt_knobs* k, double* out) {
  if (!c || (!x && n > 0) || !p || !k || !out || n < 0) return fail(WFPT_ERR_ARG, "bad arguments");
  const wfpt::Params P = to_params(p);
  const wfpt::Knobs K = to_knobs(k);
  if (!p_outlier_in_range(P.p_outlier)) {
    *out = -INFINITY;
    return WFPT_OK;
  }
  WFPT_RANGE("wfpt_wiener_like_host");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (int rc = upload(c, x, n)) return rc;
  if (int rc = run_sum(c, c->x.p, n, P, K, c->mres.d)) return rc;
  if (int rc = wait_result(c, c->mres.h)) return rc;
  return decode_sum(c, c->mres.h, out);
}

int wfpt_pdf_array(wfpt_ctx* c, const double* x, int64_t n, const wfpt_params* p,
                   const wfpt_knobs* k, int logp, double* out) {
  if (!c || (!x && n > 0) || !p || !k || (!out && n > 0) || n < 0)
    return fail(WFPT_ERR_ARG, "bad arguments");
  const wfpt::Params P = to_params(p);
  const wfpt::Knobs K = to_knobs(k);
  if (n == 0) return WFPT_OK;
  WFPT_RANGE("wfpt_pdf_array");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (int rc = upload(c, x, n)) return rc;
  HIP_TRY(c->lp.reserve(n));
  if (int rc = begin_status(c)) return rc;
  wfpt::Work W;
  if (int rc = reserve_work(c, n, &W)) return rc;
  wfpt::launch_trials(1, wfpt::kPassAll, c->x.p, n, P, K, c->lp.p, nullptr, nullptr, c->status.p,
                      logp == 1, W, c->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, c->lp.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (int rc = fetch_status(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return check_status(c);
}

int wfpt_full_pdf(wfpt_ctx* c, double x, const wfpt_params* p, const wfpt_knobs* k,
                  double* out) {
  if (!p || !k) return fail(WFPT_ERR_ARG, "null pointer");
  wfpt_params q = *p;
  q.p_outlier = 0.0;
  wfpt_knobs kk = *k;
  kk.w_outlier = 0.0;
  return wfpt_pdf_array(c, &x, 1, &q, &kk, 0, out);
}

int wfpt_wiener_like_nodes(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* per_node,
                           const wfpt_knobs* k, double* out) {
  return wfpt_wiener_like_nodes_ex(c, d, per_node, k, out, nullptr);
}

}  // extern "C"

namespace wfpt {
namespace capi {
// The per-node pass of a node dataset (everything before the per-node sums):
// the parameter table into mapped pinned memory (node_fast_kernel stages the
// rows each block needs in LDS: no H2D copy per call), the family every node
// selects, and the level-0 / chunk-engine / record kernels writing each
// trial's term to c->lp.
int nodes_launch(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* per_node,
                 const wfpt::Knobs& K, wfpt::NodeSum* ns, int32_t n_tables) {
  const int32_t m = d->n_nodes;
  const int64_t T = std::max<int32_t>(n_tables, 1);
  const int64_t rows = T * m;  // table t's node j at t m + j
  HIP_TRY(c->mnodep.reserve(std::max<int64_t>(rows, 1)));
  int mode = -2;  // the integration family every node of every table selects, or -1 if mixed
  for (int64_t j = 0; j < rows; ++j) {
    c->mnodep.h[j] = to_params(&per_node[j]);
    const int mj = wfpt::select_mode(per_node[j].sz, per_node[j].st, K.use_adaptive);
    mode = (mode == -2 || mode == mj) ? mj : -1;
  }
  if (c->host_timing) c->ht_mark = std::chrono::steady_clock::now();
  if (mode > wfpt::kAdaptTZ) mode = -1;  // fixed Simpson: generic kernel
  if (c->nodes_generic) mode = -1;
  HIP_TRY(c->res.reserve((size_t)rows + 1));
  if (mode >= 0) {  // deferred records / listed chunks of the per-node fast path
    HIP_TRY(c->nd_idx.reserve(std::max<int64_t>(T * d->n, 1)));
    HIP_TRY(c->nd_par.reserve(std::max<int64_t>(T * d->n, 1)));
    HIP_TRY(c->nd_chunks.reserve(std::max<int64_t>(T * ((d->n + 63) / 64), 1)));
    HIP_TRY(c->rare_v.reserve(std::max<int64_t>(T * d->n, 1)));
    HIP_TRY(c->rare_j.reserve(std::max<int64_t>(T * d->n, 1)));
  }
  // the split level 0 (adaptive t families, non-counting one-table calls):
  // the call's node rows + root z grids in device memory
  const bool split = (mode == wfpt::kAdaptT || mode == wfpt::kAdaptTZ) && !c->count &&
                     c->node_split && T == 1;
  wfpt::NodeTables nt{m, split, !c->count && c->node_spec};
  nt.n_tables = (int32_t)T;
  nt.rare_v = c->rare_v.p;
  nt.rare_j = c->rare_j.p;
  *ns = wfpt::NodeSum{d->x.p, d->node.p, c->mnodep.d, &K, mode, c->rare_v.p, c->rare_j.p,
                      c->count ? c->evals.p : nullptr, c->status.p};
  c->path = split ? WFPT_PATH_NODE_SPLIT : 0;
  HIP_TRY(c->mnode.reserve((size_t)rows + 2));
  HIP_TRY(c->lp.reserve(std::max<int64_t>(T * d->n, 1)));
  if (c->count) HIP_TRY(hipMemsetAsync(c->evals.p, 0, sizeof(unsigned long long), c->stream));
  const wfpt::Params* table = c->mnodep.d;
  if (c->node_table_dev && rows > 0) {  // one H2D copy instead of per-block mapped reads
    HIP_TRY(c->dnodep.reserve(rows));
    HIP_TRY(hipMemcpyAsync(c->dnodep.p, c->mnodep.h, rows * sizeof(wfpt::Params),
                           hipMemcpyHostToDevice, c->stream));
    table = c->dnodep.p;
    ns->P = table;
  }
  if (c->profile) HIP_TRY(hipEventRecord(c->ev0, c->stream));
  wfpt::launch_nodes(d->x.p, d->node.p, d->n, table, K, mode, c->lp.p, c->nd_idx.p,
                     c->nd_par.p, c->ncnt.p, c->nd_chunks.p, c->count ? c->evals.p : nullptr,
                     c->status.p, c->prof.p, c->stream, &nt);
  HIP_TRY(hipGetLastError());
  if (c->profile) HIP_TRY(hipEventRecord(c->ev1, c->stream));
  return WFPT_OK;
}

// A node call that failed after its kernels were enqueued: the node counters
// (0 at rest, reset by the call's last kernel) may be left set; restore them.
int nodes_recover(wfpt_ctx* c, int rc) {
  (void)hipStreamSynchronize(c->stream);
  (void)hipMemset(c->ncnt.p, 0, 4 * sizeof(int));
  return rc;
}

// The per-node sums of the call's n_tables x n_nodes virtual nodes into the
// mapped slot (segment_publish_kernel). A call whose kernels left rare trials
// (the exact path, trees deeper than kTreeDepth: nearly never) is reported
// pending by that launch; its rare trials are then settled (node_rare_kernel)
// and the sums published again: one more host round trip, that call only.
static int nodes_publish(wfpt_ctx* c, const wfpt_ds* d, const wfpt::NodeSum& ns, int32_t n_tables) {
  const int32_t m = d->n_nodes;
  const int32_t rows = n_tables * m;
  for (int pass = 0; pass < 2; ++pass) {
    ++c->seq;
    wfpt::launch_segment_sum(c->lp.p, d->off.p, m, c->res.p, c->mnode.d, c->status.p, c->seq,
                             c->stream, c->ncnt.p + 3, c->ncnt.p, n_tables, d->n, pass == 0);
    if (hipGetLastError() != hipSuccess)
      return nodes_recover(c, fail(WFPT_ERR_HIP, "segment_publish_kernel launch failed"));
    if (int rc = wait_word(c, c->mnode.h + rows + 1)) return nodes_recover(c, rc);
    if (c->mnode.h[rows] != wfpt::kRarePendingHost) break;
    c->path |= WFPT_PATH_NODE_RARE;
    wfpt::launch_node_rare(c->lp.p, ns, c->ncnt.p, m, d->n, c->stream);
    if (hipGetLastError() != hipSuccess)
      return nodes_recover(c, fail(WFPT_ERR_HIP, "node_rare_kernel launch failed"));
  }
  return check_status_value(c->mnode.h[rows]);
}

int nodes_check(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* per_node, const wfpt_knobs* k,
                const void* out) {
  if (!c || !d || !per_node || !k || !out) return fail(WFPT_ERR_ARG, "null pointer");
  if (d->ctx != c) return fail(WFPT_ERR_ARG, "dataset belongs to another context");
  if (!d->node.p) return fail(WFPT_ERR_ARG, "dataset was created without node ids");
  return WFPT_OK;
}

// ---- the model-comparison pass (pointwise_kernels.hip) ------

int64_t pointwise_tile(int64_t max_workspace, int64_t len, int64_t S, int64_t nodes) {
  const int64_t ws = max_workspace > 0 ? max_workspace : (int64_t)1 << 30;
  int64_t T = std::max<int64_t>(1, ws / (8 * std::max<int64_t>(len, 1)));
  if (nodes > 0) T = std::min<int64_t>(T, std::max<int64_t>(1, ((int64_t)INT32_MAX / 2) / nodes));
  return std::min<int64_t>(T, std::max<int64_t>(S, 1));
}

static wfpt::PointwiseState pointwise_state(wfpt_ctx* c) {
  const int64_t len = c->pw.len;
  double* s = c->pw.st.p;
  return wfpt::PointwiseState{s, s + len, s + 2 * len, s + 3 * len, c->pw.cnt.p,
                              c->pw.cnt.p + len};
}

int pointwise_begin(wfpt_ctx* c, int64_t len) {
  c->pw.len = len;
  const size_t n = (size_t)std::max<int64_t>(len, 1);
  HIP_TRY(c->pw.st.reserve(4 * n));
  HIP_TRY(c->pw.cnt.reserve(2 * n));
  HIP_TRY(c->pw.out.reserve(4 * n));
  // all zero bytes is the empty state (k = 0: the first finite term sets m and r)
  HIP_TRY(hipMemsetAsync(c->pw.st.p, 0, 4 * n * sizeof(double), c->stream));
  HIP_TRY(hipMemsetAsync(c->pw.cnt.p, 0, 2 * n * sizeof(int32_t), c->stream));
  if (c->profile && !c->pw.ev[0]) {
    HIP_TRY(hipEventCreate(&c->pw.ev[0]));
    HIP_TRY(hipEventCreate(&c->pw.ev[1]));
  }
  return WFPT_OK;
}

int pointwise_add(wfpt_ctx* c, const double* lp, int64_t T) {
  if (c->pw.len <= 0 || T <= 0) return WFPT_OK;
  if (c->profile) HIP_TRY(hipEventRecord(c->pw.ev[0], c->stream));
  wfpt::launch_pointwise_accumulate(lp, T, c->pw.len, pointwise_state(c), c->stream);
  HIP_TRY(hipGetLastError());
  if (c->profile) {  // a profiled pass waits for every tile's kernel: its time alone
    float ms = 0.f;
    HIP_TRY(hipEventRecord(c->pw.ev[1], c->stream));
    HIP_TRY(hipEventSynchronize(c->pw.ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms, c->pw.ev[0], c->pw.ev[1]));
    c->pw.ms += ms;
  }
  return WFPT_OK;
}

int pointwise_finish(wfpt_ctx* c, int64_t S, const int64_t* to, double* out_stats,
                     int64_t* out_ninf_total) {
  const int64_t len = c->pw.len;
  *out_ninf_total = 0;
  if (len <= 0) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    return WFPT_OK;
  }
  wfpt::launch_pointwise_finish(pointwise_state(c), len, S, c->pw.out.p, c->stream);
  HIP_TRY(hipGetLastError());
  if (!to) {
    HIP_TRY(hipMemcpyAsync(out_stats, c->pw.out.p, 4 * len * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  } else {
    std::vector<double> h(4 * (size_t)len);
    HIP_TRY(hipMemcpyAsync(h.data(), c->pw.out.p, 4 * len * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int f = 0; f < 4; ++f)
      for (int64_t i = 0; i < len; ++i) out_stats[f * len + to[i]] = h[f * len + i];
  }
  int64_t total = 0;
  for (int64_t i = 0; i < len; ++i) total += (int64_t)out_stats[3 * len + i];
  *out_ninf_total = total;
  return WFPT_OK;
}

void pointwise_all_inf(int64_t len, int64_t S, double* out_stats, int64_t* out_ninf_total) {
  for (int64_t i = 0; i < len; ++i) {
    out_stats[i] = -INFINITY;
    out_stats[len + i] = std::nan("");
    out_stats[2 * len + i] = -INFINITY;
    out_stats[3 * len + i] = (double)S;
  }
  *out_ninf_total = len * S;
}
}  // namespace capi
}  // namespace wfpt

extern "C" {

int wfpt_wiener_like_nodes_ex(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* per_node,
                              const wfpt_knobs* k, double* out, double* out_trial) {
  if (int rc = nodes_check(c, d, per_node, k, out)) return rc;
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_wiener_like_nodes");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const int32_t m = d->n_nodes;
  wfpt::NodeSum ns{};
  if (int rc = nodes_launch(c, d, per_node, K, &ns)) return nodes_recover(c, rc);
  if (m > 0) {
    // per-node sums, status and the completion word land in mapped memory
    // (one launch; its last block resets the node counters)
    if (int rc = nodes_publish(c, d, ns, 1)) return rc;
  } else {
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  if (int rc = finish_profile(c)) return rc;
  std::memcpy(out, c->mnode.h, m * sizeof(double));
  // each trial's term (node_logp: the node's mixture, log, -inf for a zero
  // density or p_outlier outside [0, 1]) in the caller's trial order
  if (out_trial) return trials_to_caller(d, c->lp.p, out_trial);
  return WFPT_OK;
}

int wfpt_wiener_like_nodes_multi_ex(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* tables,
                                    int32_t n_tables, const wfpt_knobs* k, double* out,
                                    double* out_trial) {
  if (int rc = nodes_check(c, d, tables, k, out)) return rc;
  if (n_tables < 1) return fail(WFPT_ERR_ARG, "n_tables < 1");
  const int32_t m = d->n_nodes;
  if ((int64_t)n_tables * m > (int64_t)INT32_MAX / 2)
    return fail(WFPT_ERR_ARG, "n_tables x n_nodes too large");
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_wiener_like_nodes_multi");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const int32_t rows = n_tables * m;
  using clk = std::chrono::steady_clock;
  const auto h0 = clk::now();
  wfpt::NodeSum ns{};
  if (int rc = nodes_launch(c, d, tables, K, &ns, n_tables)) return nodes_recover(c, rc);
  const auto h1 = clk::now();
  if (rows > 0) {
    if (int rc = nodes_publish(c, d, ns, n_tables)) return rc;
  } else {
    if (hipStreamSynchronize(c->stream) != hipSuccess)
      return nodes_recover(c, fail(WFPT_ERR_HIP, "node pass failed on the device"));
    (void)hipMemset(c->ncnt.p, 0, 4 * sizeof(int));
  }
  if (int rc = finish_profile(c)) return rc;
  const auto h2 = clk::now();
  std::memcpy(out, c->mnode.h, (size_t)rows * sizeof(double));
  if (c->host_timing) {
    const auto h3 = clk::now();
    auto ns_ = [](clk::duration d_) {
      return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(d_).count();
    };
    c->ht[0] += ns_(c->ht_mark - h0);
    c->ht[1] += ns_(h1 - c->ht_mark);
    c->ht[2] += ns_(h2 - h1);
    c->ht[3] += ns_(h3 - h2);
    c->ht[4] += ns_(h3 - h0);
    ++c->ht_calls;
  }
  if (out_trial)
    for (int32_t t = 0; t < n_tables; ++t)
      if (int rc = trials_to_caller(d, c->lp.p + (int64_t)t * d->n, out_trial + (int64_t)t * d->n))
        return rc;
  return WFPT_OK;
}

int wfpt_wiener_like_nodes_multi(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* tables,
                                 int32_t n_tables, const wfpt_knobs* k, double* out) {
  return wfpt_wiener_like_nodes_multi_ex(c, d, tables, n_tables, k, out, nullptr);
}

int wfpt_pointwise_nodes(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* tables, int64_t S,
                         const wfpt_knobs* k, int64_t max_workspace, double* out_sums,
                         double* out_stats, int64_t* out_ninf_total) {
  if (!out_stats || !out_ninf_total) return fail(WFPT_ERR_ARG, "null pointer");
  if (int rc = nodes_check(c, d, tables, k, out_sums)) return rc;
  if (S < 1) return fail(WFPT_ERR_ARG, "S < 1");
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_pointwise_nodes");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const int32_t m = d->n_nodes;
  const int64_t n = d->n;
  const int64_t tile = pointwise_tile(max_workspace, n, S, m);
  if (int rc = pointwise_begin(c, n)) return rc;
  for (int64_t s0 = 0; s0 < S; s0 += tile) {
    // the multi-table node call's sequence on sweeps [s0, s0 + T): the publish
    // returns once the tile's sums are final, its rare trials settled in c->lp
    const int32_t T = (int32_t)std::min<int64_t>(tile, S - s0);
    const int64_t rows = (int64_t)T * m;
    wfpt::NodeSum ns{};
    if (int rc = nodes_launch(c, d, tables + s0 * m, K, &ns, T)) return nodes_recover(c, rc);
    if (rows > 0) {
      if (int rc = nodes_publish(c, d, ns, T)) return rc;
    } else {
      if (hipStreamSynchronize(c->stream) != hipSuccess)
        return nodes_recover(c, fail(WFPT_ERR_HIP, "node pass failed on the device"));
      (void)hipMemset(c->ncnt.p, 0, 4 * sizeof(int));
    }
    if (int rc = finish_profile(c)) return rc;
    std::memcpy(out_sums + s0 * m, c->mnode.h, (size_t)rows * sizeof(double));
    if (int rc = pointwise_add(c, c->lp.p, T)) return rc;
  }
  std::vector<int64_t> perm;
  if (d->perm.p && n > 0) {
    perm.resize(n);
    HIP_TRY(hipMemcpyAsync(perm.data(), d->perm.p, n * sizeof(int64_t), hipMemcpyDeviceToHost,
                           c->stream));
  }
  return pointwise_finish(c, S, perm.empty() ? nullptr : perm.data(), out_stats, out_ninf_total);
}

int wfpt_pointwise_profile(wfpt_ctx* c, double* accumulate_ms, int reset) {
  if (!c || !accumulate_ms) return fail(WFPT_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(c->mu);
  *accumulate_ms = c->pw.ms;
  if (reset) c->pw.ms = 0.0;
  return WFPT_OK;
}

int wfpt_wiener_like_nodes_local(wfpt_ctx* c, const wfpt_ds* d, const wfpt_params* per_node,
                                 const wfpt_knobs* k, double* out) {
  if (int rc = nodes_check(c, d, per_node, k, out)) return rc;
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_wiener_like_nodes_local");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const int32_t m = d->n_nodes;
  wfpt::NodeSum ns{};
  if (int rc = nodes_launch(c, d, per_node, K, &ns)) return nodes_recover(c, rc);
  // every exit after nodes_launch restores the node counters (0 at rest)
  wfpt::launch_segment_res(c->lp.p, d->off.p, m, c->res.p, c->status.p, false, c->stream, c->ncnt.p,
                           &ns);
  if (hipGetLastError() != hipSuccess)
    return nodes_recover(c, fail(WFPT_ERR_HIP, "segment_res launch failed"));
  if (hipMemcpyAsync(out, c->res.p, ((size_t)m + 1) * sizeof(double), hipMemcpyDeviceToHost,
                     c->stream) != hipSuccess)
    return nodes_recover(c, fail(WFPT_ERR_HIP, "node vector copy failed"));
  if (hipStreamSynchronize(c->stream) != hipSuccess)
    return nodes_recover(c, fail(WFPT_ERR_HIP, "node pass failed on the device"));
  return finish_profile(c);
}

}  // extern "C"

namespace wfpt {
namespace capi {

static bool multi_fast(double* const dptr[7], const double scal[7], const Knobs& K, int64_t m) {
  if (dptr[4] || dptr[6] || m <= 0) return false;
  const int mode = select_mode(scal[4], scal[6], K.use_adaptive);
  return mode >= 0 && mode <= kAdaptTZ;
}

int multi_score_reserve(wfpt_ctx* c, int64_t total, int nslots, double* const* dptr,
                        const double* scal, bool lp, bool records) {
  HIP_TRY(c->mptr.reserve(7 * (size_t)nslots));
  HIP_TRY(c->mscal.reserve(7 * (size_t)nslots));
  HIP_TRY(hipMemcpyAsync(c->mptr.p, dptr, 7 * nslots * sizeof(double*), hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipMemcpyAsync(c->mscal.p, scal, 7 * nslots * sizeof(double), hipMemcpyHostToDevice,
                         c->stream));
  const int64_t nb = blocks_for(total);
  HIP_TRY(c->part.reserve(std::max<int64_t>(nb, 1)));
  HIP_TRY(c->zero.reserve(std::max<int64_t>(nb, 1)));
  if (lp) HIP_TRY(c->lp.reserve(std::max<int64_t>(total, 1)));
  if (records) {
    HIP_TRY(c->nd_idx.reserve(std::max<int64_t>(total, 1)));
    HIP_TRY(c->nd_par.reserve(std::max<int64_t>(total, 1)));
  }
  return WFPT_OK;
}

int multi_score_launch(wfpt_ctx* c, const double* dx, int64_t m, int slot, double* const dptr[7],
                       const double scal[7], const Knobs& K, double p_outlier, double* lp) {
  if (multi_fast(dptr, scal, K, m)) {
    HIP_TRY(hipMemsetAsync(c->n_defer.p, 0, sizeof(int), c->stream));
    launch_multi_fast(select_mode(scal[4], scal[6], K.use_adaptive), dx, m, c->mptr.p + 7 * slot,
                      c->mscal.p + 7 * slot, K, p_outlier, lp, c->nd_idx.p, c->nd_par.p,
                      c->n_defer.p, c->part.p, c->zero.p, c->count ? c->evals.p : nullptr,
                      c->status.p, c->stream);
  } else {
    launch_multi(dx, m, c->mptr.p + 7 * slot, c->mscal.p + 7 * slot, K, p_outlier, c->part.p,
                 c->zero.p, c->status.p, c->stream, lp);
  }
  HIP_TRY(hipGetLastError());
  return WFPT_OK;
}

int multi_score(wfpt_ctx* c, const double* dx, int64_t m, double* const dptr[7],
                const double scal[7], const Knobs& K, double p_outlier) {
  if (int rc = multi_score_reserve(c, m, 1, dptr, scal)) return rc;
  return multi_score_launch(c, dx, m, 0, dptr, scal, K, p_outlier, c->lp.p);
}

int multi_finish(wfpt_ctx* c, int64_t m, double* out) {
  if (c->profile) HIP_TRY(hipEventRecord(c->ev1, c->stream));
  launch_finalize(c->part.p, c->zero.p, blocks_for(m), 0, c->status.p, c->mres.d, ++c->seq,
                  c->stream, nullptr, nullptr, nullptr, nullptr, c->fin.p, c->fin_ticket.p);
  HIP_TRY(hipGetLastError());
  if (int rc = wait_result(c, c->mres.h)) return rc;
  if (int rc = check_status_value(c->mres.h[2])) return rc;
  if (int rc = finish_profile(c)) return rc;
  *out = c->mres.h[0];
  return WFPT_OK;
}

int upload_multi_arrays(wfpt_ctx* c, const double* const* arrays, int count, int64_t n,
                        const double* substitute, double** dev) {
  int na = 0;
  for (int j = 0; j < count; ++j) na += arrays[j] != nullptr;
  HIP_TRY(c->marr.reserve(std::max<int64_t>((int64_t)na * n, 1)));
  int slot = 0;
  for (int j = 0; j < count; ++j) {
    dev[j] = nullptr;
    if (!arrays[j]) continue;
    dev[j] = c->marr.p + (int64_t)slot++ * n;
    const double* src = (substitute && j == count - 1) ? substitute : arrays[j];
    if (n > 0)
      HIP_TRY(hipMemcpyAsync(dev[j], src, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  return WFPT_OK;
}

int score_runs(wfpt_ctx* c, const double* dx, double* const field[7], const wfpt_params* rows,
               int32_t G, const int64_t* off_host, const int64_t* off_dev,
               DevBuf<double>& npart, const Knobs& K, double p_outlier, double* out_logp) {
  const bool sz_fix = !field[4], st_fix = !field[6];
  std::vector<int32_t> run_lo;  // first group of each run
  for (int32_t j = 0; j < G; ++j)
    if (j == 0 || (sz_fix && rows[j].sz != rows[j - 1].sz) ||
        (st_fix && rows[j].st != rows[j - 1].st))
      run_lo.push_back(j);
  const int nruns = (int)run_lo.size();
  run_lo.push_back(G);
  std::vector<double*> tabs(7 * (size_t)nruns, nullptr);
  std::vector<double> scals(7 * (size_t)nruns, 0.0);
  for (int r = 0; r < nruns; ++r) {
    const int64_t lo = off_host[run_lo[r]];
    for (int f = 0; f < 7; ++f)
      if (field[f]) tabs[7 * r + f] = field[f] + lo;
    if (sz_fix) scals[7 * r + 4] = rows[run_lo[r]].sz;
    if (st_fix) scals[7 * r + 6] = rows[run_lo[r]].st;
  }
  const int64_t n = off_host[G];
  if (int rc = multi_score_reserve(c, n, nruns, tabs.data(), scals.data())) return rc;
  for (int r = 0; r < nruns; ++r) {
    const int64_t lo = off_host[run_lo[r]], hi = off_host[run_lo[r + 1]];
    if (hi == lo) continue;  // no trial, no launch
    if (int rc = multi_score_launch(c, dx + lo, hi - lo, r, &tabs[7 * r], &scals[7 * r], K,
                                    p_outlier, c->lp.p + lo))
      return rc;
  }
  HIP_TRY(npart.reserve(rl_node_partials(n, G)));
  HIP_TRY(c->res.reserve(G));
  launch_rl_node_sum(c->lp.p, off_dev, G, npart.p, c->res.p, c->stream);
  HIP_TRY(hipGetLastError());
  double total;  // a finalize over no partials: the status word and the call's completion
  if (int rc = multi_finish(c, 0, &total)) return rc;
  HIP_TRY(hipMemcpy(out_logp, c->res.p, G * sizeof(double), hipMemcpyDeviceToHost));
  return WFPT_OK;
}

int counts_to_offsets(const char* name, const int64_t* counts, int64_t R,
                      std::vector<int64_t>* off) {
  *off = std::vector<int64_t>((size_t)R + 1, 0);
  for (int64_t r = 0; r < R; ++r) {
    if (counts[r] < 0)
      return fail(WFPT_ERR_ARG, std::string(name) + ": negative count in row " + std::to_string(r));
    (*off)[r + 1] = (*off)[r] + counts[r];
  }
  return WFPT_OK;
}

}  // namespace capi
}  // namespace wfpt

// wiener_like_multi over device x[n]: the per-trial parameter arrays go up for
// this call, then the shared scoring sequence. The generic kernel writes the
// per-trial terms only when out_trial asks for them; the deferred records
// belong to the level-0 path.
static int run_multi(wfpt_ctx* c, const double* dx, int64_t n, const double* const arrays[7],
                     const double scalars[7], const wfpt::Knobs& K, double p_outlier,
                     double* out, double* out_trial) {
  double* dev[7];
  if (int rc = upload_multi_arrays(c, arrays, 7, n, nullptr, dev)) return rc;
  const bool fast = multi_fast(dev, scalars, K, n);
  const bool want_lp = fast || (out_trial && n > 0);
  if (int rc = multi_score_reserve(c, n, 1, dev, scalars, want_lp, fast)) return rc;
  if (c->count) HIP_TRY(hipMemsetAsync(c->evals.p, 0, sizeof(unsigned long long), c->stream));
  if (c->profile) HIP_TRY(hipEventRecord(c->ev0, c->stream));
  if (int rc = multi_score_launch(c, dx, n, 0, dev, scalars, K, p_outlier,
                                  want_lp ? c->lp.p : nullptr))
    return rc;
  if (int rc = multi_finish(c, n, out)) return rc;
  // each trial's term log(p (1 - p_outlier) + w_outlier p_outlier), or the
  // log prob_ub of a missing response (wfpt.pyx:261-272), in trial order
  if (out_trial && n > 0)
    HIP_TRY(hipMemcpy(out_trial, c->lp.p, n * sizeof(double), hipMemcpyDeviceToHost));
  return WFPT_OK;
}

extern "C" {

int wfpt_wiener_like_multi(wfpt_ctx* c, const double* x, int64_t n,
                           const double* const arrays[7], const double scalars[7],
                           const wfpt_knobs* k, double p_outlier, double* out) {
  return wfpt_wiener_like_multi_ex(c, x, n, arrays, scalars, k, p_outlier, out, nullptr);
}

int wfpt_wiener_like_multi_ex(wfpt_ctx* c, const double* x, int64_t n,
                              const double* const arrays[7], const double scalars[7],
                              const wfpt_knobs* k, double p_outlier, double* out,
                              double* out_trial) {
  if (!c || (!x && n > 0) || !arrays || !scalars || !k || !out || n < 0)
    return fail(WFPT_ERR_ARG, "bad arguments");
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_wiener_like_multi");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (int rc = upload(c, x, n)) return rc;
  return run_multi(c, c->x.p, n, arrays, scalars, K, p_outlier, out, out_trial);
}

int wfpt_wiener_like_multi_resident(wfpt_ctx* c, const wfpt_ds* d, const double* const arrays[7],
                                    const double scalars[7], const wfpt_knobs* k,
                                    double p_outlier, double* out) {
  return wfpt_wiener_like_multi_resident_ex(c, d, arrays, scalars, k, p_outlier, out, nullptr);
}

int wfpt_wiener_like_multi_resident_ex(wfpt_ctx* c, const wfpt_ds* d,
                                       const double* const arrays[7], const double scalars[7],
                                       const wfpt_knobs* k, double p_outlier, double* out,
                                       double* out_trial) {
  if (!c || !d || !arrays || !scalars || !k || !out) return fail(WFPT_ERR_ARG, "null pointer");
  if (d->ctx != c) return fail(WFPT_ERR_ARG, "dataset belongs to another context");
  if (!d->input_order || d->node.p)
    return fail(WFPT_ERR_ARG,
                "wiener_like_multi on a dataset needs one created with WFPT_DS_INPUT_ORDER "
                "and no node ids (per-trial arrays follow the caller's trial order)");
  const wfpt::Knobs K = to_knobs(k);
  WFPT_RANGE("wfpt_wiener_like_multi_resident");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  return run_multi(c, d->x.p, d->n, arrays, scalars, K, p_outlier, out, out_trial);
}

int wfpt_dmat_cdf_array(wfpt_ctx* c, const double* x, int64_t n, const wfpt_params* p,
                        double w_outlier, double* out) {
  if (!c || (!x && n > 0) || !p || (!out && n > 0) || n < 0)
    return fail(WFPT_ERR_ARG, "bad arguments");
  const double v = p->v, sv = p->sv, a = p->a, z = p->z, sz = p->sz, t = p->t, st = p->st;
  const double po = p->p_outlier;
  // cdfdif_wrapper.pyx:23-25
  if ((sv < 0) || (a <= 0) || (z < 0) || (z > 1) || (sz < 0) || (sz > 1) || (z + sz / 2. > 1) ||
      (z - sz / 2. < 0) || (t - st / 2. < 0) || (t < 0) || (st < 0) || !p_outlier_in_range(po))
    return fail(WFPT_ERR_ARG, "at least one of the parameters is out of the support");
  if (n == 0) return WFPT_OK;
  if (n >= (int64_t)1 << 31) return fail(WFPT_ERR_ARG, "dmat_cdf_array: n must be < 2^31");
  // cdfdif_wrapper.pyx:35-42 (the model's units: a and z scaled by 1/10, s = 0.1)
  const double epsi = 1e-10;
  const double par[7] = {a / 10., t, sv / 10. + epsi, z * (a / 10.), sz * (a / 10.) + epsi,
                         st + epsi, v / 10.};
  WFPT_RANGE("wfpt_dmat_cdf_array");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (int rc = upload(c, x, n)) return rc;
  HIP_TRY(c->lp.reserve(n));
  if (c->profile) HIP_TRY(hipEventRecord(c->ev0, c->stream));
  HIP_TRY(c->defer.reserve(n + 1));
  HIP_TRY(c->cdf_tab.reserve(wfpt::kCdfTableDoubles));
  HIP_TRY(hipMemsetAsync(c->defer.p + n, 0, sizeof(int), c->stream));
  wfpt::launch_dmat_cdf(c->x.p, n, par, po, w_outlier, c->lp.p, c->cdf_tab.p, c->defer.p,
                        c->defer.p + n, c->stream);
  HIP_TRY(hipGetLastError());
  if (c->profile) HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipMemcpyAsync(out, c->lp.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->profile) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->k_ms += ms;
    c->launches += 1;
  }
  return WFPT_OK;
}

int wfpt_dmat_cdf_rows(wfpt_ctx* c, const wfpt_params* rows, const double* x,
                       const double* freq_obs, const double* n_samples, int64_t R, int32_t E,
                       double w_outlier, double* out_cdf, double* out_chisq, double* out_gsq) {
  if (!c || !rows || !x) return fail(WFPT_ERR_ARG, "dmat_cdf_rows: null pointer");
  if (R < 1) return fail(WFPT_ERR_ARG, "dmat_cdf_rows: R must be >= 1");
  if (E < 1 || E > wfpt::kCdfRowsMaxEdges)
    return fail(WFPT_ERR_ARG, "dmat_cdf_rows: E must be in 1.." +
                                  std::to_string(wfpt::kCdfRowsMaxEdges));
  if (R > ((int64_t)1 << 31) / (E + 1))
    return fail(WFPT_ERR_ARG, "dmat_cdf_rows: R * (E + 1) must be <= 2^31");
  const bool stats = freq_obs != nullptr;
  if (stats != (n_samples != nullptr) || stats != (out_chisq != nullptr) ||
      stats != (out_gsq != nullptr))
    return fail(WFPT_ERR_ARG,
                "dmat_cdf_rows: freq_obs, n_samples, out_chisq and out_gsq go together");
  if (!stats && !out_cdf) return fail(WFPT_ERR_ARG, "dmat_cdf_rows: no output requested");
  static_assert(sizeof(wfpt_params) == 8 * sizeof(double), "rows pack as doubles");
  WFPT_RANGE("wfpt_dmat_cdf_rows");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  // in: rows | x | freq_obs | n_samples; out: cdf | chisq | gsq
  const size_t o_x = (size_t)R * 8, o_f = o_x + (size_t)R * E;
  const size_t o_n = o_f + (stats ? (size_t)R * (E + 1) : 0), n_in = o_n + (stats ? R : 0);
  const size_t o_c = out_cdf ? (size_t)R * E : 0, n_out = o_c + (stats ? 2 * (size_t)R : 0);
  std::vector<double>& h = c->rows_host;
  h.resize(std::max(n_in, n_out));
  std::memcpy(h.data(), rows, (size_t)R * sizeof(wfpt_params));
  std::memcpy(h.data() + o_x, x, (size_t)R * E * sizeof(double));
  if (stats) {
    std::memcpy(h.data() + o_f, freq_obs, (size_t)R * (E + 1) * sizeof(double));
    std::memcpy(h.data() + o_n, n_samples, (size_t)R * sizeof(double));
  }
  HIP_TRY(c->rows_in.reserve(n_in));
  HIP_TRY(c->rows_out.reserve(n_out));
  HIP_TRY(hipMemcpyAsync(c->rows_in.p, h.data(), n_in * sizeof(double), hipMemcpyHostToDevice,
                         c->stream));
  if (c->profile) HIP_TRY(hipEventRecord(c->ev0, c->stream));
  double* d = c->rows_in.p;
  double* o = c->rows_out.p;
  wfpt::launch_dmat_cdf_rows(reinterpret_cast<const wfpt_params*>(d), d + o_x,
                             stats ? d + o_f : nullptr, stats ? d + o_n : nullptr, R, E, w_outlier,
                             out_cdf ? o : nullptr, stats ? o + o_c : nullptr,
                             stats ? o + o_c + R : nullptr, c->stream);
  HIP_TRY(hipGetLastError());
  if (c->profile) HIP_TRY(hipEventRecord(c->ev1, c->stream));
  // the upload is complete before the kernel runs (same stream), so h is free
  HIP_TRY(hipMemcpyAsync(h.data(), o, n_out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (out_cdf) std::memcpy(out_cdf, h.data(), o_c * sizeof(double));
  if (stats) {
    std::memcpy(out_chisq, h.data() + o_c, (size_t)R * sizeof(double));
    std::memcpy(out_gsq, h.data() + o_c + R, (size_t)R * sizeof(double));
  }
  if (c->profile) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->k_ms += ms;
    c->launches += 1;
  }
  return WFPT_OK;
}

int wfpt_profile_enable(wfpt_ctx* c, int flags) {
  if (!c) return fail(WFPT_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(c->mu);
  c->profile = (flags & WFPT_PROF_EVENTS) != 0;
  c->count = (flags & WFPT_PROF_EVALS) != 0;
  return WFPT_OK;
}

int wfpt_profile_read(wfpt_ctx* c, double* kernel_ms, int64_t* launches, int64_t* n_evals,
                      int reset) {
  if (!c) return fail(WFPT_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(c->mu);
  if (kernel_ms) *kernel_ms = c->k_ms;
  if (launches) *launches = c->launches;
  if (n_evals) *n_evals = c->n_evals;
  if (reset) {
    c->k_ms = 0.0;
    c->launches = 0;
    c->n_evals = 0;
  }
  return WFPT_OK;
}

int wfpt_profile_lists(wfpt_ctx* c, int64_t counts[16], int reset) {
  if (!c || !counts) return fail(WFPT_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  int h[16];
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(h, c->prof.p, sizeof(h), hipMemcpyDeviceToHost));
  for (int k = 0; k < 16; ++k) counts[k] = h[k];
  std::vector<unsigned long long> ph(8 * wfpt::kPhaseWaves);
  HIP_TRY(hipMemcpy(ph.data(), c->phase.p, ph.size() * sizeof(ph[0]), hipMemcpyDeviceToHost));
  for (int k = 0; k < 5; ++k) {
    unsigned long long t = 0;
    for (int w = 0; w < wfpt::kPhaseWaves; ++w) t += ph[w * 8 + 2 + k];
    counts[11 + k] = (int64_t)(t / 1000);
  }
  if (reset) {
    HIP_TRY(hipMemset(c->prof.p, 0, sizeof(h)));
    HIP_TRY(hipMemset(c->phase.p, 0, ph.size() * sizeof(ph[0])));
  }
  return WFPT_OK;
}

int wfpt_debug_waves(wfpt_ctx* c, uint64_t* out, int64_t max_records) {
  if (!c || !out) return fail(WFPT_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int64_t n = std::min<int64_t>(max_records, wfpt::kPhaseWaves);
  HIP_TRY(hipMemcpy(out, c->phase.p, n * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return WFPT_OK;
}

int wfpt_debug_lean_first(wfpt_ctx* c, int32_t* chunks, int32_t max_chunks, int32_t* n) {
  if (!c || !n || (max_chunks > 0 && !chunks) || max_chunks < 0)
    return fail(WFPT_ERR_ARG, "bad arguments");
  std::lock_guard<std::mutex> lk(c->mu);
  *n = c->first_last.n;
  for (int k = 0; k < c->first_last.n && k < max_chunks; ++k) chunks[k] = c->first_last.c[k];
  return WFPT_OK;
}

int wfpt_synchronize(wfpt_ctx* c) {
  if (!c) return fail(WFPT_ERR_ARG, "null pointer");
  DeviceGuard g(c->device);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return WFPT_OK;
}

}  // extern "C"
