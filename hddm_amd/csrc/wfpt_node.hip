// wfpt_node.hip — per-node parameters (wfpt_wiener_like_nodes) on gfx950:
// node_fast_kernel (level 0, LDS-staged node rows) + node_chunk_kernel (the
// deferred trials one wave each when they are sparse in their chunks, else
// the listed chunks 64 trials per wave per node segment); the generic
// node_kernel for mixed families; node_rare_kernel for the rare trials; the
// per-node sums and their publication (segment_publish_kernel).
#include "wfpt_engine.hpp"

#pragma clang fp contract(off)

namespace wfpt {

// The node path's rare trials -- the exact path (near-ties, ambiguous series
// decisions, densities below kExactBelow) and trees deeper than kTreeDepth --
// are not settled by the level-0 / record / chunk kernels: they append the
// trial to a list and leave lp[v] = +0.0, and the summing kernel settles each
// node's rare trials (exact_pdf / fallback_pdf, one lane each) before it
// publishes the node. Their code (wfpt_exact.hpp's double-double libm, the
// per-lane walk's memory stack) is thus out of the hot kernels' registers and
// scratch: node_fast_kernel<kDirect> 168 -> ~54 VGPRs (3 -> 8 waves/SIMD),
// node_chunk_kernel without its 7.5 KB/lane of scratch.
// Entry k: v[k] = virtual trial index (t n + i) | kind << kRareShift, j[k] =
// its virtual node (t m + node[i]); *n the count (0 at rest: the summing
// kernel's last block resets it).

// Node vj's sum, one wave (vj = t m + jr: the trials [t n + off[jr],
// t n + off[jr + 1]) of lp): each lane adds its strided terms in order, then
// a wave_sum; -inf if any term is -inf (wfpt.pyx:71-72 per node). The rare
// trials' terms are in lp by then (node_rare_kernel).
__device__ inline double node_sum(const double* lp, const int64_t* off, int32_t vj, int32_t m,
                                  int64_t n, int lane) {
  const int tab = vj / m, jr = vj - tab * m;
  const int64_t lo = tab * n + off[jr], hi = tab * n + off[jr + 1];
  double s = 0.0;
  int zero = 0;
  // four strided terms per lane loaded together, then added in order (one
  // memory latency per 256 trials instead of per 64)
  for (int64_t i0 = lo + lane; i0 < hi; i0 += 256) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = i0 + 64 * u < hi ? lp[i0 + 64 * u] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (v[u] == -INFINITY) zero = 1;
      else s += v[u];
    }
  }
  s = wave_sum(s);
  return __ballot(zero != 0) != 0ull ? -INFINITY : s;
}

// node_sum of NB nodes of one wave at once (vj[b], on[b]): the same per-node
// operations -- each lane's strided terms in the same order, the same 0.0
// additions past a segment's end inside an active batch, one wave_sum per
// node -- with every node's loads issued before any node's additions, so the
// wave waits one memory latency per batch instead of one per node.
template <int NB>
__device__ inline void node_sums(const double* lp, const int64_t* off, const int32_t (&vj)[NB],
                                 const bool (&on)[NB], int32_t m, int64_t n, int lane,
                                 double (&out)[NB]) {
  int64_t lo[NB], hi[NB];
  double s[NB];
  int zero[NB];
  int64_t len = 0;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int tab = on[b] ? vj[b] / m : 0, jr = on[b] ? vj[b] - tab * m : 0;
    lo[b] = on[b] ? tab * n + off[jr] : 0;
    hi[b] = on[b] ? tab * n + off[jr + 1] : 0;
    len = hi[b] - lo[b] > len ? hi[b] - lo[b] : len;
    s[b] = 0.0;
    zero[b] = 0;
  }
  for (int64_t q = lane; q < len; q += 256) {
    double v[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = lo[b] + q + 64 * u;
        v[b][u] = i < hi[b] ? lp[i] : 0.0;
      }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (lo[b] + q < hi[b]) {  // node_sum's iteration i0 = lo + q is active
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (v[b][u] == -INFINITY) zero[b] = 1;
          else s[b] += v[b][u];
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const double t = wave_sum(s[b]);
    out[b] = __ballot(zero[b] != 0) != 0ull ? -INFINITY : t;
  }
}

// The rare trials of a node call (rare_push), one lane each: the exact path
// or the per-lane walk of the trial's family, its node term into lp. Launched
// only when the publication found the list non-empty (the host re-publishes;
// a call with no rare trial -- nearly all of them -- never runs this code, and
// its kernels carry neither its registers nor its scratch). n_tab: trials per
// table, m: nodes per table (table t's node j at t m + j).
__global__ __launch_bounds__(64, WFPT_SLOW_WAVES) void node_rare_kernel(NodeRare R, double* lp, const double* x,
                                                          const Params* P, int32_t m,
                                                          int64_t n_tab, Knobs K, int mode,
                                                          int* status, unsigned long long* evals) {
  const int nr = *R.n;
  int errf = 0;
  long long ne = 0;
  for (int k = blockIdx.x * 64 + threadIdx.x; k < nr; k += gridDim.x * 64) {
    const int64_t r = R.v[k];
    const int64_t v = r & kRareMask;
    const int kind = (int)(r >> kRareShift);
    const int32_t vj = R.j[k];
    const int64_t i = v - (int64_t)(vj / m) * n_tab;
    const Params Q = P[vj];
    long long n1 = 0;
    double p;
    if (kind == kRareExact) p = exact_pdf(x[i], Q, K, &n1, &errf);
    else if (mode == kAdaptT) p = fallback_pdf<kAdaptT>(x[i], Q, K, &n1, &errf);
    else if (mode == kAdaptZ) p = fallback_pdf<kAdaptZ>(x[i], Q, K, &n1, &errf);
    else p = fallback_pdf<kAdaptTZ>(x[i], Q, K, &n1, &errf);
    ne += n1;
    lp[v] = node_logp(p, Q, K);
  }
  if (errf & kFlagErrors) atomicOr(status, errf & kFlagErrors);
  if (evals && ne) atomicAdd(evals, (unsigned long long)ne);
}

// One wave per node (grid-stride): the per-node sums into res (the node
// all-reduce's vector and wfpt_wiener_like_nodes_local).
__global__ __launch_bounds__(256) void segment_sum_kernel(const double* lp, const int64_t* off,
                                                          int32_t n_nodes, double* res) {
  const int lane = threadIdx.x & 63;
  for (int j = blockIdx.x * 4 + (threadIdx.x >> 6); j < n_nodes; j += gridDim.x * 4) {
    const double s = node_sum(lp, off, j, n_nodes, 0, lane);
    if (lane == 0) res[j] = s;
  }
}

// segment_sum_kernel's per-node sums and publish_nodes_kernel's publication in
// one launch. The ordering is the memory model's, not the hardware's (LLVM
// AMDGPUUsage memory model for GFX942/GFX950, the HSA / OpenCL 2.0 scoped
// model: happens-before is the transitive closure of program order and scoped
// synchronizes-with edges, each edge between threads inside its scope):
//   1. lane 0 of node j's wave stores res[j] (device memory; an agent-scope
//      atomic store, performed at agent scope before the wave goes on);
//   2. __syncthreads (workgroup-scope release + acquire): every store of the
//      block happens-before thread 0's next operation;
//   3. thread 0: acq_rel fetch_add on the agent-scope ticket. The ticket's
//      RMWs form one release sequence, so the block that draws G - 1
//      synchronizes-with every earlier block's release;
//   4. __syncthreads: the last block's threads happen-after all G releases,
//      read res[] and store it to the mapped slot;
//   5. __syncthreads, then thread 0 stores the completion word with a
//      system-scope release; the host polls it with an acquire load
//      (capi_core.cpp: wait_word), so every sum is visible when it reads.
// r05 let each wave store its sum straight into the mapped slot, ordered
// before the completion word by nothing: one GPU-suite run read a node sum
// of the previous call (profiles/r06/stale_diag/ shows the test catching that
// order deterministically in the WFPT_PUB_DIAG build,
// segment_publish_diag_kernel below). The last block also resets the call's
// counters (the node path's n_defer words and the ticket: 0 at rest, stream
// order).
constexpr int32_t kPubBlocks = 128;
// nodes a publishing wave sums at once (node_sums; 1: one node at a time)
#ifndef WFPT_PUB_NODES
#define WFPT_PUB_NODES 4
#endif
constexpr int kPubNodes = WFPT_PUB_NODES;
// Multi-table calls: n_nodes = T m virtual nodes, node j of table t at
// t m + j, summing trials [t n + off[j], t n + off[j + 1]) of lp.
// check_rare: a call whose level-0 / record / chunk kernels left rare trials
// (*n_rare > 0) is not summed: the last block writes kRarePending in the
// error slot and the completion word, the host runs node_rare_kernel and
// launches this kernel again with check_rare = 0.
constexpr double kRarePending = -1.0;  // (error counts are >= 0)
__global__ __launch_bounds__(256) void segment_publish_kernel(const double* lp, const int64_t* off,
                                                              int32_t n_nodes, int* status,
                                                              double* res, double* out,
                                                              unsigned long long seq, int* ticket,
                                                              int* counters, int32_t m_tab,
                                                              int64_t n_tab, int check_rare) {
  __shared__ int last;
  const int lane = threadIdx.x & 63;
  const int nwv = (int)gridDim.x * 4;  // waves; wave w sums nodes w, w + nwv, ...
  const int j0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  // (written by the call's earlier kernels: stream order)
  const bool pending = check_rare && counters[1] > 0;
  // wave w sums nodes w, w + nwv, ..., kPubNodes of them at a time
  for (int j = pending ? n_nodes : j0; j < n_nodes; j += kPubNodes * nwv) {
    int32_t vj[kPubNodes];
    bool on[kPubNodes];
    double sums[kPubNodes];
#pragma unroll
    for (int b = 0; b < kPubNodes; ++b) {
      vj[b] = j + b * nwv;
      on[b] = vj[b] < n_nodes;
    }
    node_sums<kPubNodes>(lp, off, vj, on, m_tab, n_tab, lane, sums);
    if (lane == 0) {  // (1)
#pragma unroll
      for (int b = 0; b < kPubNodes; ++b)
        if (on[b]) __hip_atomic_store(&res[vj[b]], sums[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // the storing wave waits for its agent-scope stores (and status atomics) to
  // be performed: LLVM's workgroup barrier does not wait for other waves'
  // vector memory operations (non-tgsplit gfx950 emits only lgkmcnt(0) before
  // s_barrier), and thread 0's release below waits only for its own wave's
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // (2)
  if (threadIdx.x == 0)  // (3)
    last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
           (int)gridDim.x - 1;
  __syncthreads();  // (4)
  if (pending) {  // the host settles the rare trials and publishes again
    if (!last) return;
    if (threadIdx.x == 0) {
      *ticket = 0;
      out[n_nodes] = kRarePending;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      publish_word(reinterpret_cast<unsigned long long*>(out + n_nodes + 1), seq);
    return;
  }
  if (!last) return;
  // plain loads: every block's stores happen-before them (the acquire above
  // invalidates this XCD's caches at agent scope); sixteen in flight per
  // thread, then the stores (the compiler does not move a load of res above a
  // store to out: they may alias)
  for (int k0 = threadIdx.x; k0 < n_nodes; k0 += 16 * 256) {
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = k0 + 256 * u < n_nodes ? res[k0 + 256 * u] : 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (k0 + 256 * u < n_nodes) out[k0 + 256 * u] = v[u];
  }
  if (threadIdx.x == 0) {
    *ticket = 0;
    counters[0] = 0;
    counters[1] = 0;  // the rare list's count
    counters[2] = 0;
    const int st = atomicExch(status, 0);
    out[n_nodes] = (double)(st & kFlagDepth) + ((st & kFlagBudget) ? kBudgetUnit : 0.0);
  }
  __syncthreads();  // (5)
  if (threadIdx.x == 0)
    publish_word(reinterpret_cast<unsigned long long*>(out + n_nodes + 1), seq);
}

// Diagnostic builds only (WFPT_PUB_DIAG=1, never the shipped library):
// segment_publish_kernel with the publication order broken on purpose. One
// node per wave; every block takes its ticket *first*, and every block but the
// last writes its nodes' sums into the mapped slot ~70 us later, i.e. the
// completion word deterministically overtakes the sums -- the failure the
// regression test must be able to see.
#ifndef WFPT_PUB_DIAG
#define WFPT_PUB_DIAG 0
#endif
#if WFPT_PUB_DIAG
__global__ __launch_bounds__(256) void segment_publish_diag_kernel(
    const double* lp, const int64_t* off, int32_t n_nodes, int* status, double* res, double* out,
    unsigned long long seq, int* ticket, int* counters, int32_t m_tab, int64_t n_tab,
    int check_rare) {
  __shared__ int last;
  const int lane = threadIdx.x & 63;
  const int nwv = (int)gridDim.x * 4;
  const int j0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool pending = check_rare && counters[1] > 0;
  double sum = 0.0;
  for (int j = pending ? n_nodes : j0; j < n_nodes; j += nwv)
    sum = node_sum(lp, off, j, m_tab, n_tab, lane);
  __syncthreads();
  if (threadIdx.x == 0)
    last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
           (int)gridDim.x - 1;
  __syncthreads();
  if (pending) {  // as segment_publish_kernel
    if (!last) return;
    if (threadIdx.x == 0) {
      *ticket = 0;
      out[n_nodes] = kRarePending;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      publish_word(reinterpret_cast<unsigned long long*>(out + n_nodes + 1), seq);
    return;
  }
  if (!last) {
    for (int r = 0; r < 20; ++r) __builtin_amdgcn_s_sleep(127);
    if (j0 < n_nodes && lane == 0) out[j0] = sum;  // after the word: stale reads follow
    return;
  }
  if (j0 < n_nodes && lane == 0) out[j0] = sum;
  if (threadIdx.x == 0) {
    *ticket = 0;
    counters[0] = 0;
    counters[1] = 0;
    counters[2] = 0;
    const int st = atomicExch(status, 0);
    out[n_nodes] = (double)(st & kFlagDepth) + ((st & kFlagBudget) ? kBudgetUnit : 0.0);
  }
  __syncthreads();
  if (threadIdx.x == 0)
    publish_word(reinterpret_cast<unsigned long long*>(out + n_nodes + 1), seq);
}
#endif

// Node all-reduce (wfpt_wiener_like_nodes_allreduce): the encoded error
// count of this rank's node pass appended to its per-node sums (res[n]),
// status reset; or a failed rank's poisoned vector {0 ..., kPeerFailUnit}.
__global__ __launch_bounds__(64) void node_status_kernel(double* res, int32_t n, int* status,
                                                         int poison, int* counters) {
  if (threadIdx.x == 0) {
    counters[0] = 0;  // the node path's n_defer words: 0 at rest
    counters[1] = 0;
    counters[2] = 0;
    const int st = atomicExch(status, 0);
    res[n] = poison ? kPeerFailUnit
                    : (double)(st & kFlagDepth) + ((st & kFlagBudget) ? kBudgetUnit : 0.0);
  }
}
__global__ __launch_bounds__(256) void node_poison_kernel(double* res, int32_t n) {
  for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) res[j] = 0.0;
}
// The all-reduced vector (n sums + the error count) to mapped memory, then
// the completion word out[n + 1].
__global__ __launch_bounds__(256) void publish_vec_kernel(const double* res, int32_t n,
                                                          double* out, unsigned long long seq) {
  for (int j = threadIdx.x; j <= n; j += 256) out[j] = res[j];
  __syncthreads();  // every thread's stores happen-before thread 0's release
  if (threadIdx.x == 0) publish_word(reinterpret_cast<unsigned long long*>(out + n + 1), seq);
}

// ---------------------------------------------------------------------------
// Per-node parameters (wfpt_wiener_like_nodes): trials of node j use P[j].
// The dataset is grouped by node, so a 256-trial block spans a short run of
// node ids; their parameter rows (P is the mapped pinned table the host
// filled for this call) are staged once per block in LDS and every trial
// reads its row there. Blocks spanning more than kStageRows ids (empty nodes
// between) read the table directly.
constexpr int kStageRows = 256;

template <int STK, bool COUNT>
__global__ __launch_bounds__(kBlock, WFPT_SLOW_WAVES) void node_kernel(
    const double* x, const int32_t* node, int64_t n, const Params* P, Knobs K, double* lp,
    unsigned long long* evals, int* status) {
  using Stack = typename StackOf<STK>::type;
  __shared__ Params rows[kStageRows];
  const int64_t i0 = (int64_t)blockIdx.x * kBlock;
  const int64_t i = i0 + threadIdx.x;
  const int first = node[i0];
  const int last = node[(i0 + kBlock - 1 < n) ? i0 + kBlock - 1 : n - 1];
  const int span = last - first + 1;
  const bool staged = span <= kStageRows;
  if (staged) {
    const double* src = reinterpret_cast<const double*>(P + first);
    double* dst = reinterpret_cast<double*>(rows);
    for (int k = threadIdx.x; k < span * 8; k += kBlock) dst[k] = src[k];
  }
  __syncthreads();
  long long ne = 0;
  int zero = 0, flags = 0;
  if (i < n) {
    const int nj = node[i];
    const Params Q = staged ? rows[nj - first] : P[nj];
    double p = full_pdf<kRuntime, Stack>(x[i], Q, K, ne, flags);
    p = settle(p, x[i], Q, K, !trial_setup(x[i], Q).valid, ne, flags);
    if (flags & kFlagErrors) atomicOr(status, flags & kFlagErrors);
    lp[i] = node_logp(p, Q, K);
  }
  if (COUNT) {
    double d = 0.0;
    block_reduce<COUNT>(d, zero, ne);
    if (threadIdx.x == 0) atomicAdd(evals, (unsigned long long)ne);
  }
}

// Two-pass per-node path (used when every node's parameters select the same
// integration family, the usual HDDM case: sv/sz/st are group-level):
// node_fast_kernel is the level-0 pass with the node's parameter row (staged
// in LDS as in node_kernel) and per-trial log p out. Adaptive families: a wave
// (64 consecutive stored trials: a chunk) with a trial that needs refinement
// or the exact path appends its chunk id to a dense list (one atomic per
// wave), which node_chunk_kernel completes 64 trials per wave. Direct family:
// the rare exact-path trials go to the rare list (rare_push), which the
// summing kernel settles.
template <int MODE, bool COUNT>
__global__ __launch_bounds__(kBlock, FastWaves<MODE>::value > 0 ? FastWaves<MODE>::value : 1)
void node_fast_kernel(const double* x, const int32_t* node, int64_t n, const Params* P, Knobs K,
                      double* lp, int64_t* d_idx, Params* d_par, int* n_defer, int* clist,
                      int* n_chunks, unsigned long long* evals, int* status, int* prof,
                      int32_t n_nodes, int64_t nw_tab, NodeRare R) {
  // parameter table blockIdx.y (multi-table calls: T tables x the same
  // trials): its rows, its terms lp[t n + i], its records' virtual indices
  // t n + i and its chunks' ids t nw_tab + c
  const int64_t tab = blockIdx.y;
  double* const lp0 = lp;
  P += tab * n_nodes;
  lp += tab * n;
  const int64_t vbase = tab * n, cbase = tab * nw_tab;
  __shared__ Params rows[kStageRows];
  const int64_t i0 = (int64_t)blockIdx.x * kBlock;
  const int64_t i = i0 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int first = node[i0];
  const int last = node[(i0 + kBlock - 1 < n) ? i0 + kBlock - 1 : n - 1];
  const int span = last - first + 1;
  const bool staged = span <= kStageRows;
  if (staged) {
    const double* src = reinterpret_cast<const double*>(P + first);
    double* dst = reinterpret_cast<double*>(rows);
    for (int k = threadIdx.x; k < span * 8; k += kBlock) dst[k] = src[k];
  }
  __syncthreads();
  long long ne = 0;
  bool defer = false;
  Params Q;
  int nj = 0;
  if (i < n) {
    nj = node[i];
    Q = staged ? rows[nj - first] : P[nj];
    double p, f[5];
    int flags = 0;
    unsigned pend;
    const int oc = fast_level0<MODE>(x[i], Q, K, p, f, ne, flags, pend);
    if (oc == kFinal) lp[i] = node_logp(p, Q, K);
    else defer = true;
  }
  const unsigned long long b = __ballot(defer);
  if (b) {
    if (MODE == kDirect) {
      // the rare exact-path trials (near-ties, densities below kExactBelow:
      // fast_level0's kExact) go to the rare list; the summing kernel settles
      // them with exact_pdf -- what full_pdf + settle gives such a trial
      if (defer) {
        rare_push(R, vbase + i, (int32_t)(tab * n_nodes + nj), kRareExact, lp0);
        if (COUNT) ne = 0;  // (the summing kernel counts the exact path's evaluations)
      }
    } else {
      // the chunk for node_chunk_kernel and the trials as records for
      // node_records (fast-pass records counted in n_chunks[2])
      int base = 0;
      if (lane == 0) {
        clist[atomicAdd(n_chunks, 1)] = (int)(cbase + (i >> 6));
        base = atomicAdd(n_chunks + 2, __popcll(b));
      }
      base = __shfl(base, 0, 64);
      if (defer) {
        const int k = base + __popcll(b & lanemask_lt(lane));
        d_idx[k] = vbase + i;
        d_par[k] = Q;
      }
    }
  }
  if (COUNT) {
    ne = wave_sum_ll((defer && MODE != kDirect) ? 0 : ne);
    if (lane == 0) {
      atomicAdd(evals, (unsigned long long)ne);
      if (b && MODE != kDirect) atomicAdd(&prof[3], __popcll(b));
    }
  }
}

// Split per-node level 0 (the adaptive t families: kAdaptT, kAdaptTZ -- the
// full DDM of config 4). A batched node call of ~100k trials is ~1.5k waves:
// fewer than the chip's SIMDs, so node_fast_kernel's one-lane-per-trial level
// 0 lasts one wave's latency (25 dependent evaluations per lane). Here block c
// takes chunk c (64 stored trials) with kNodeSplit = 5 waves: wave j evaluates
// t node j of all 64 trials (l0_node: the function of the per-lane loop and of
// the split units, bit-identical to it; j is wave-uniform), on the trial's
// node row (the mapped table) and its root z grid (zgrid_setup per lane, as
// fast_level0). Then wave 0 takes one trial per lane again: the root
// stop test and value from the five node values (l0_finish, as
// small_split_kernel), the term, and -- exactly as node_fast_kernel -- a chunk
// with a trial that refines or needs the exact path is listed for
// node_chunk_kernel with its deferred trials as records.
constexpr int kNodeSplit = 5;
template <int MODE>
__global__ __launch_bounds__(kNodeSplit * 64) void node_split_kernel(
    const double* x, const int32_t* node, int64_t n, const Params* P, Knobs K, double* lp,
    int64_t* d_idx, Params* d_par, int* clist, int* n_chunks) {
  static_assert(MODE == kAdaptT || MODE == kAdaptTZ, "t-node split");
  __shared__ double sf[kNodeSplit][64];
  __shared__ int sfl[kNodeSplit][64];
  __shared__ int spd[kNodeSplit][64];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t c = blockIdx.x;
  const int64_t i = c * 64 + lane;
  const bool own = i < n;
  const double x0 = own ? x[i] : 0.0;
  const int nj = own ? node[i] : 0;
  const Params Q = P[nj];  // the mapped table the host filled for this call
  const Trial tr = trial_setup(x0, Q);
  double y = 0.0;
  int flags = 0;
  bool pj = false;
  if (own && tr.valid) {
    double lb, ub;
    tree_root<MODE>(tr, Q, lb, ub);
    const L0Hints H = l0_hints(tr.x, lb, ub, Q.a, K.err);
    long long ne = 0;
    // the trial's root z grid per lane, as fast_level0 builds it (the
    // large-time sines by the per-lane recurrence: no table loads in the
    // series loop)
    ZGrid G{};
    if (MODE == kAdaptTZ) G = zgrid_setup(tr.z - tr.sz / 2., tr.z + tr.sz / 2., tr.v, Q.sv, Q.a);
    y = l0_node<MODE>(tr, Q, K, lb, ub, H, wv, G, flags, pj, ne, nullptr);
  }
  sf[wv][lane] = y;
  sfl[wv][lane] = flags;
  spd[wv][lane] = pj ? 1 : 0;
  __syncthreads();
  if (wv != 0) return;
  int fl = 0;
  unsigned pd = 0u;
#pragma unroll
  for (int q = 0; q < kNodeSplit; ++q) {
    fl |= sfl[q][lane];
    if (spd[q][lane]) pd |= 1u << (q * (kTreeW / 4));
  }
  const double f[5] = {sf[0][lane], sf[1][lane], sf[2][lane], sf[3][lane], sf[4][lane]};
  double p = 0.0;
  int oc = kFinal;
  if (own) oc = l0_finish<MODE>(tr, Q, K, fl, pd, f, p);
  const bool defer = own && oc != kFinal;
  if (own && !defer) lp[i] = node_logp(p, Q, K);
  const unsigned long long b = __ballot(defer);
  if (b) {  // node_fast_kernel's listing: the chunk, and its deferred trials as records
    int base = 0;
    if (lane == 0) {
      clist[atomicAdd(n_chunks, 1)] = (int)c;
      base = atomicAdd(n_chunks + 2, __popcll(b));
    }
    base = __shfl(base, 0, 64);
    if (defer) {
      const int k = base + __popcll(b & lanemask_lt(lane));
      d_idx[k] = i;
      d_par[k] = Q;
    }
  }
}

// Per-node path: deferred trials run as records (one wave per trial,
// node_records) when they average at most kNodeRecPerChunk per listed
// chunk, else 64 trials per wave through their chunks (node_chunk_kernel),
// which re-runs every trial of a chunk. Both produce each trial's term with
// the same operations; the choice depends only on the call's inputs.
constexpr int kNodeRecPerChunk = 8;
__device__ inline bool node_records_sparse(int n_records, int n_chunks) {
  return (long long)n_records <= (long long)kNodeRecPerChunk * n_chunks;
}

// Speculative record (non-counting node calls of the adaptive t families,
// with the call's node tables): a deferred trial of a sparse call is one
// wave's work, and the breadth-first rounds (node_records) walk its tree
// level by level -- six or more dependent rounds of one grid evaluation each.
// Here the wave evaluates EVERY value the reference's recursion can reach at
// n_st = n_sz = kTreeDepth in two rounds: the 17 dyadic t points x the 4 z
// grids (kAdaptTZ; kAdaptT: the 17 t points), plus the level-0 t points' root
// grids once more with the level-0 hints, exactly as the engine evaluates
// them (its stage-0 tasks of level 0 take l0_hints, its z walks do not).
// Then 17 lanes settle each t point's value as the engine's task completion
// does (the root test, simp_value, or the z walk's tree17 over its 17
// values), and lane 0 runs tree17 over the t points. Only the points that
// recursion reads (tree17's `used`) contribute their flags (ambiguous
// decisions, ties, deeper trees), so the trial's density and its deferral
// are the engine's; the extra values are never read. LDS: buf (>= 314
// doubles: the walk values and the hinted root grids), tv (17 t values),
// pf (>= 39 ints of point flags); lp[i] gets the node term.
constexpr int kOvfBit = 1 << 8;  // a grid's drift factor overflowed (literal values)
// The record's tables (eng_tables_wave's values) built by a team of NW waves:
// with NW = 4 each wave computes one group (the 8 z grids, the t points, the
// z points, the interval reciprocals), so the divergent groups run side by
// side instead of one after another.
template <int NW>
__device__ inline void eng_tables_team(const Params& P, EngTables& T, int wave, int lane) {
  if (NW == 1) {
    eng_tables_wave(P, T, lane);
    return;
  }
  constexpr int kP = kTreePoints;
  if (wave == 0) {
    if (lane < 8) {
      const int flip = lane >> 2, sel = lane & 3;
      const double zf = flip ? 1. - P.z : P.z, vf = flip ? -P.v : P.v;
      T.G[flip][sel] = zgrid_of(zf - P.sz / 2., zf + P.sz / 2., sel, vf, P.sv, P.a);
    }
  } else if (wave == 1) {
    if (lane < kP) T.tP[lane] = dyadic_point(P.t - P.st / 2., P.t + P.st / 2., lane);
  } else if (wave == 2) {
    if (lane < 2 * kP) {
      const int flip = lane / kP, k = lane % kP;
      const double zf = flip ? 1. - P.z : P.z;
      T.zP[flip][k] = dyadic_point(zf - P.sz / 2., zf + P.sz / 2., k);
    }
  } else if (lane < 2) {
    const int flip = lane;
    const double zf = flip ? 1. - P.z : P.z;
    T.iz[flip] = 1.0 / ((zf + P.sz / 2.) - (zf - P.sz / 2.));
  }
}
// WFPT_REC_FENCE: a scheduling barrier between the record's phases. Without
// them the compiler's schedule over the record's divergent phases makes the
// call's records 1.5x slower (node_chunk_kernel 24.0 -> 15.6 us at config 4's
// generating parameters, same code otherwise).
#define WFPT_REC_FENCE() __builtin_amdgcn_sched_barrier(0)
template <int NW>
__device__ inline void record_sync() {
  if (NW == 1) wave_sync();
  else __syncthreads();
}
// NW waves per record (NW = 1: the wave alone; NW = kEngWaves: the block,
// every wave calling with the same record, wave = its index): the NE
// evaluations are dealt to the waves in contiguous runs of t points, so each
// wave's lanes take similar x - t (similar code paths: a round costs the
// union of its lanes' paths), and the waves evaluate side by side. The
// values, and so every output bit, are the same for any NW.
template <int MODE, int NW>
__device__ inline void node_record_spec(double* buf, double* tv, int* pf, EngTables& T, int wave,
                                        int lane, const double* x, const Knobs& K, double* lp,
                                        int64_t i, const Params& Q, const NodeRare& R,
                                        double* lp_base, int64_t v, int32_t vj) {
  constexpr int NP = kTreePoints;
  constexpr int NG = MODE == kAdaptTZ ? 4 : 1;  // grids per t point
  constexpr int NE = NP * NG + (MODE == kAdaptTZ ? 5 : 0);
  constexpr int kPer = (NE + NW - 1) / NW;  // evaluations per wave (NW > 1: one trip)
  static_assert(NW == 1 || kPer <= 64, "record team");
  double* zv = buf;             // [NP][NP] the unhinted grids' values (the z walks)
  double* hv = buf + NP * NP;   // [5][5] the hinted root grids of the level-0 t points
  int* fu = pf;                 // [NP] unhinted root grid: kFlagExact (ambiguous) | kOvfBit
  int* fh = pf + NP;            // [5] hinted root grid: the same
  int* fp = pf + NP + 5;        // [NP] the t point's settled flags
  const double x0 = x[i];
  const Trial tr = trial_setup(x0, Q);
  if (!tr.valid) {  // (never deferred: p = 0 settles at level 0)
    if (wave == 0 && lane == 0) lp[i] = node_logp(0.0, Q, K);
    return;
  }
  WFPT_REC_FENCE();
  eng_tables_team<NW>(Q, T, wave, lane);  // the record's tables in LDS
  record_sync<NW>();
  WFPT_REC_FENCE();
  const int flip = x0 > 0 ? 1 : 0;
  const double a = Q.a, sv = Q.sv;
  const double iwt = 1.0 / (T.tP[kTreeW] - T.tP[0]);
  const double ia2 = 1.0 / (a * a);  // as l0_hints / refine_rounds
  const L0Hints H = l0_hints(tr.x, T.tP[0], T.tP[kTreeW], a, K.err);
  const double izf = T.iz[flip];
  const int e_lo = NW == 1 ? 0 : wave * kPer;
  const int e_hi = NW == 1 ? NE : ((wave + 1) * kPer < NE ? (wave + 1) * kPer : NE);
  for (int e0 = e_lo; e0 < e_hi; e0 += 64) {
    const int e = e0 + lane;
    if (e >= e_hi) continue;
    int k, gs, jh = -1;
    if (e < NP * NG) {
      k = e / NG;
      gs = e - k * NG;
      if (MODE == kAdaptT && (k & 3) == 0) jh = k >> 2;  // kAdaptT level 0: hinted
    } else {
      jh = e - NP * NG;
      k = jh * (kTreeW / 4);
      gs = kGridRoot;
    }
    double qh = -1.0;
    bool known = false;
    Decision kd{0, 0, 0};
    if (jh >= 0) {
      qh = H.qh(jh);
      known = jh == 0 ? H.ok0 : (jh == 4 ? H.ok4 : H.shared);
      kd = jh == 4 ? H.D4 : H.D0;
    }
    const TNode N = tnode_setup_r(tr.x - T.tP[k], tr.v, sv, a, ia2, K.err, qh, known, kd);
    const int amb = N.amb ? (int)kFlagExact : 0;
    if (MODE == kAdaptT) {
      tv[k] = tnode_pdf_sv(N, tr.z, tr.v, sv, a) * iwt;
      fp[k] = amb;
    } else {
      double y[5];
      const bool ok = tnode_pdf_sv_grid5(N, T.G[flip][gs], tr.v, sv, a, y);  // literal values
      if (jh < 0) {
#pragma unroll
        for (int j = 0; j < 5; ++j)
          if (grid_owns(gs, j)) zv[k * NP + grid_point(gs, j)] = y[j] * izf;
        if (gs == kGridRoot) fu[k] = amb | (ok ? 0 : kOvfBit);
      } else {
#pragma unroll
        for (int j = 0; j < 5; ++j) hv[jh * 5 + j] = y[j] * izf;
        fh[jh] = amb | (ok ? 0 : kOvfBit);
      }
    }
  }
  record_sync<NW>();
  WFPT_REC_FENCE();
  if (MODE == kAdaptTZ && wave == 0 && lane < NP) {
    // t point k's task completion (refine_rounds stage 0): the root test on
    // its root grid (hinted at level 0), then -- if it refines or the grid
    // overflowed -- the z walk over the unhinted grids
    const int k = lane;
    const bool l0 = (k & 3) == 0;
    const double* r = l0 ? hv + (k >> 2) * 5 : nullptr;
    const double r0 = l0 ? r[0] : zv[k * NP], r1 = l0 ? r[1] : zv[k * NP + 4],
                 r2 = l0 ? r[2] : zv[k * NP + 8], r3 = l0 ? r[3] : zv[k * NP + 12],
                 r4 = l0 ? r[4] : zv[k * NP + 16];
    const int rf = l0 ? fh[k >> 2] : fu[k];
    const ZGrid& gr = T.G[flip][kGridRoot];
    const Simp sm = simp5p(gr.h6, gr.h12, r0, r1, r2, r3, r4);
    int f = 0;
    const bool ovf = (rf & kOvfBit) != 0;
    const bool pend = simpson_refine(sm.S, sm.S2, K.simps_err, K.n_sz, f) || ovf;
    if (ovf) f = 0;
    int flags = (rf & kFlagExact) | f;
    double val;
    if (!pend) {
      val = simp_value(sm) * iwt;
    } else {
      flags |= fu[k] & kFlagExact;  // the walk's own (unhinted) t node
      const double(&zk)[kTreePoints] =
          *reinterpret_cast<const double(*)[kTreePoints]>(zv + k * NP);
      int f2 = 0, nref = 0;
      unsigned need = 0u;
      const double zi = tree17(zk, T.zP[flip], K.simps_err, K.n_sz, kTreeDepth, f2, need, nref);
      if (need) f2 |= kFlagFallback;  // z tree deeper than the walk's levels
      flags |= f2 & (kFlagExact | kFlagFallback);
      val = zi * iwt;
    }
    tv[k] = val;
    fp[k] = flags;
  }
  if (wave == 0) wave_sync();
  WFPT_REC_FENCE();
  if (wave == 0 && lane == 0) {
    const double(&tk)[kTreePoints] = *reinterpret_cast<const double(*)[kTreePoints]>(tv);
    unsigned need = 0u, used = 0u;
    int fl = 0, nref = 0;
    double p = tree17(tk, T.tP, K.simps_err, K.n_st, kTreeDepth, fl, need, nref, &used);
#pragma unroll 1
    for (int k = 0; k < NP; ++k)
      if ((used >> k) & 1u) fl |= fp[k];
    if (need) fl |= kFlagFallback;  // t tree deeper than kTreeDepth
    fl &= kFlagExact | kFlagFallback;
    // tree_density's settlement
    const bool structural = tr.x - T.tP[0] <= 0;
    bool defer = fl != 0 || !(p > kExactBelow || structural);
    if (defer && fl == 0 && tiny_absorbed(p, Q.p_outlier, K.w_outlier)) {
      defer = false;
      p = 0.0;
    }
    // the rare list (node_sum settles it): the exact path, or the per-lane
    // walk for a tree deeper than kTreeDepth
    if (defer)
      rare_push(R, v, vj, (fl & kFlagExact) || fl == 0 ? kRareExact : kRareWalk, lp_base);
    else
      lp[i] = node_logp(p, Q, K);
  }
  record_sync<NW>();  // the next record reuses the LDS
}

// The node path's completion of the chunks node_fast_kernel listed: one wave
// per chunk, as the dataset engine (engine_kernel) runs a chunk, per node
// segment of the chunk (nodes are contiguous and |rt|-ordered: a chunk holds
// one node, or the end of one and the start of the next). Per segment: the
// node's parameter row (wave-uniform), its tables built by the lanes in
// parallel into the wave's LDS (eng_tables_wave), level 0 per lane on the
// segment's trials, the in-wave refinement rounds over all of them together,
// then each trial's density (tree17 over its values; the exact path or the
// per-lane walk for the rare trials the rounds hand on) and its term. Every
// trial of a listed chunk is rewritten (the same level-0 operations as the
// fast pass), so a chunk's terms do not depend on which lanes deferred.
// A call where most trials refine (an MCMC proposal far in the tails) runs
// 64 trials per wave this way; when the deferred trials are sparse in their
// chunks (node_records_sparse: the usual MCMC call) the same launch runs the
// fast pass's records one wave each instead (node_records), which skips the
// level 0 of the chunks' settled trials. Trials the rounds hand on (the exact
// path, trees deeper than kTreeDepth) are settled on their own lane (rare).
// A speculative record is one block's work (its waves evaluate side by side)
// or one wave's: team records (one block each, ~12 us) while the call's records fit in one
// round of resident blocks (2 per CU: the kernel's 68 KB of LDS); beyond, one
// wave per record (~21 us, but 4x as many side by side): multi-table calls of
// several chains defer thousands of trials
constexpr int kRecTeamMax = 512;
// waves per SIMD the node chunk engine is compiled for (register budget)
#ifndef WFPT_NODE_CHUNK_WAVES
#define WFPT_NODE_CHUNK_WAVES 2
#endif
template <int MODE, bool COUNT>
__global__ __launch_bounds__(kEngBlock, WFPT_NODE_CHUNK_WAVES) void node_chunk_kernel(
    const double* x, const int32_t* node, int64_t n, const Params* P, Knobs K, double* lp,
    const int* clist, const int* n_chunks, const int64_t* r_idx, const Params* r_par,
    unsigned long long* evals, int* status, int* prof, int spec, int32_t n_nodes,
    int64_t nw_tab, NodeRare R) {
  __shared__ ChunkLds<1> lds[kEngWaves];
  const int lane = threadIdx.x & 63;
  ChunkLds<1>& cl = lds[threadIdx.x >> 6];
  const int nc = n_chunks[0], nrec = n_chunks[2];
  const int nwaves = (int)gridDim.x * kEngWaves;
  const int w0 =
      __builtin_amdgcn_readfirstlane((int)blockIdx.x * kEngWaves + (int)(threadIdx.x >> 6));
  if (node_records_sparse(nrec, nc)) {  // a few deferred trials: one wave each
    if constexpr (!COUNT && (MODE == kAdaptT || MODE == kAdaptTZ)) {
      if (spec) {  // every tree point in two rounds (node_record_spec)
        if (nrec <= kRecTeamMax) {
          // one block per record, its waves side by side (wave 0's LDS)
          ChunkLds<1>& c0 = lds[0];
          const int wv = threadIdx.x >> 6;
          for (int k = (int)blockIdx.x; k < nrec; k += (int)gridDim.x) {
            const int64_t v = r_idx[k];  // virtual: table t's trial i at t n + i
            const int64_t t = v / n, ix = v - t * n;
            node_record_spec<MODE, kEngWaves>(c0.F, c0.X, c0.fl, c0.tab, wv, lane, x + ix, K,
                                              lp + v, 0, r_par[k], R, lp, v,
                                              (int32_t)(t * n_nodes + node[ix]));
          }
        } else {
          for (int k = w0; k < nrec; k += nwaves) {
            const int64_t v = r_idx[k];
            const int64_t t = v / n, ix = v - t * n;
            // F: 1088 doubles, fl: 64 ints
            node_record_spec<MODE, 1>(cl.F, cl.X, cl.fl, cl.tab, 0, lane, x + ix, K, lp + v, 0,
                                      r_par[k], R, lp, v, (int32_t)(t * n_nodes + node[ix]));
          }
        }
        return;
      }
    }
    node_records<MODE, COUNT, false>(cl, lane, w0, nwaves, x, K, lp, r_idx, r_par, nrec, evals,
                                     status, n, &R, node, n_nodes);
    return;
  }
  long long ne = 0;
  int nseg = 0, nex = 0, nwk = 0;
  Tally ty;
  for (int k = w0; k < nc; k += nwaves) {
    const int64_t vc = clist[k];  // virtual: table t's chunk c at t nw_tab + c
    const int64_t tab = vc / nw_tab;
    const int64_t c = vc - tab * nw_tab;
    const Params* Pt = P + tab * n_nodes;
    double* lpt = lp + tab * n;
    const int64_t i = c * 64 + lane;
    const bool own = i < n;
    const double x0 = own ? x[i] : 0.0;
    const int nj = own ? node[i] : -1;
    bool todo = own;
    for (unsigned long long left = __ballot(todo); left; left = __ballot(todo)) {
      // the next node segment: the node of the first lane still to do
      const int jn = __shfl(nj, __ffsll((long long)left) - 1, 64);
      const bool mine = todo && nj == jn;
      todo = todo && !mine;
      ++nseg;
      const Params Q = Pt[__builtin_amdgcn_readfirstlane(jn)];
      TrialArgs A{};
      A.x = x;
      A.n = n;
      A.P = Q;
      A.K = K;
      A.wp_outlier = K.w_outlier * Q.p_outlier;
      eng_tables_wave(Q, cl.tab, lane);
      double p = 0.0, f0[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      long long ne0 = 0;
      unsigned pend0 = 0u;
      int oc = kFinal;
      if (mine) oc = eng_level0<MODE>(x0, Q, K, cl.tab.G[x0 > 0][kGridRoot], p, f0, ne0, pend0);
      if (__ballot(mine && oc == kTree) != 0ull) {
        cl.X[lane] = x0;
        cl.fl[lane] = (mine && oc == kTree) ? 0 : (mine && oc == kExact ? (int)kFlagExact
                                                                         : (int)kFlagIdle);
        if (COUNT) cl.cnt[lane] = (int)ne0;
        if (mine && oc == kTree) {
#pragma unroll
          for (int j = 0; j < 5; ++j) cl.F[j * (kTreeW / 4) * 64 + lane] = f0[j];
        }
        if (lane == 0) {
          cl.qn[0] = 0;
          cl.qn[1] = 0;
        }
        wave_sync();
        if (MODE == kAdaptTZ) {
#pragma unroll
          for (int j = 0; j < 5; ++j)
            team_push(mine && oc == kTree && ((pend0 >> (j * (kTreeW / 4))) & 1u),
                      lane | ((j * (kTreeW / 4)) << 6), cl.ZQ, &cl.qn[1]);
        }
        wave_sync();
        PhaseClock pc;
        Tally t1;
        refine_rounds<MODE, COUNT, 1>(A, cl, lane, 1, t1, pc);
        if (COUNT) {
          ty.t1 += t1.t1;
          ty.t2 += t1.t2;
          ty.rec += t1.rec;
          for (int q = 0; q < 3; ++q) ty.z[q] += t1.z[q];
        }
      }
      bool defer = mine && oc == kExact;
      int rf = kFlagExact;
      long long n1 = ne0;
      if (mine && oc == kTree) {
        tree_density<MODE, 1>(A, cl, lane, x0, p, defer, rf);
        if (COUNT) n1 = cl.cnt[lane];
      }
      if (defer) {  // rare: the exact path or the per-lane walk, by node_sum
        rare_push(R, tab * n + i, (int32_t)(tab * n_nodes + jn),
                  (rf & kFlagExact) ? kRareExact : kRareWalk, lp);
        n1 = 0;
        if (COUNT) ++((rf & kFlagExact) ? nex : nwk);
      }
      if (mine && !defer) {
        if (oc != kFinal) ne += n1;  // node_fast_kernel counted the trials it settled
        lpt[i] = node_logp(p, Q, K);
      }
      wave_sync();  // the next segment rebuilds this wave's LDS
    }
  }
  if (COUNT) {
    ne = wave_sum_ll(ne);
    nex = (int)wave_sum_ll(nex);
    nwk = (int)wave_sum_ll(nwk);
    if (lane == 0) {
      atomicAdd(evals, (unsigned long long)ne);
      atomicAdd(&prof[0], nseg);
      atomicAdd(&prof[5], nex);
      atomicAdd(&prof[6], nwk);
      atomicAdd(&prof[1], ty.t1);
      atomicAdd(&prof[2], ty.t2);
      atomicAdd(&prof[4], ty.rec);
      atomicAdd(&prof[7], ty.z[0] + ty.z[1] + ty.z[2]);
      atomicAdd(&prof[8], ty.z[0]);
      atomicAdd(&prof[9], ty.z[1]);
      atomicAdd(&prof[10], ty.z[2]);
    }
  }
}

// ---------------------------------------------------------------------------
// launchers

template <int MODE, bool COUNT>
static void launch_nodes_two_pass(const double* x, const int32_t* node, int64_t n,
                                  const Params* P, const Knobs& K, double* lp, int64_t* d_idx,
                                  Params* d_par, int* n_defer, int* clist,
                                  unsigned long long* evals, int* status, int* prof,
                                  hipStream_t s, const NodeTables* nt) {
  bool split = false, spec = false;
  const int T = nt ? std::max(nt->n_tables, 1) : 1;
  const int32_t m = nt ? nt->n_nodes : 0;
  const int64_t nw = (n + 63) / 64;
  if constexpr ((MODE == kAdaptT || MODE == kAdaptTZ) && !COUNT) {
    spec = nt && nt->spec;
    if (nt && nt->split && nt->n_nodes > 0 && T == 1) {
      // the call's node tables, then the t-node split level 0; the chunk
      // engine / records below read the device copy of the rows
      hipLaunchKernelGGL((node_split_kernel<MODE>), dim3((n + 63) / 64), dim3(kNodeSplit * 64), 0,
                         s, x, node, n, P, K, lp, d_idx, d_par, clist, n_defer);
      split = true;
    }
  }
  const NodeRare R{nt ? nt->rare_v : nullptr, nt ? nt->rare_j : nullptr, n_defer + 1};
  if (!split)
    hipLaunchKernelGGL((node_fast_kernel<MODE, COUNT>), dim3(blocks_for(n), T), dim3(kBlock), 0, s,
                       x, node, n, P, K, lp, d_idx, d_par, n_defer, clist, n_defer, evals, status,
                       prof, m, nw, R);
  if constexpr (MODE != kDirect) {
    // adaptive families, one launch: the fast pass's records one wave each
    // when they are sparse in their chunks, else one wave per listed chunk
    // (node_chunk_kernel reads the counts and picks)
    const int64_t nb = std::min<int64_t>((T * nw + kEngWaves - 1) / kEngWaves, 2048);
    hipLaunchKernelGGL((node_chunk_kernel<MODE, COUNT>), dim3(nb), dim3(kEngBlock), 0, s, x, node,
                       n, P, K, lp, clist, n_defer, d_idx, d_par, evals, status, prof,
                       spec ? 1 : 0, m, nw, R);
  }
  // direct family: node_fast_kernel settles its exact-path trials itself
}

void launch_nodes(const double* x, const int32_t* node, int64_t n, const Params* P,
                  const Knobs& K, int mode, double* lp, int64_t* d_idx, Params* d_par,
                  int* n_defer, int* clist, unsigned long long* evals, int* status, int* prof,
                  hipStream_t s, const NodeTables* nt) {
  const int64_t nb = blocks_for(n);
  if (nb == 0) return;
  if (mode >= kDirect && mode <= kAdaptTZ) {
    with_mode(mode, [&](auto m) {
      with_flag(evals != nullptr, [&](auto c) {
        launch_nodes_two_pass<decltype(m)::value, decltype(c)::value>(
            x, node, n, P, K, lp, d_idx, d_par, n_defer, clist, evals, status, prof, s, nt);
      });
    });
    return;
  }
  // mixed families: the generic per-trial kernel once per parameter table
  const int T = nt ? std::max(nt->n_tables, 1) : 1;
  for (int t = 0; t < T; ++t) {
    const Params* Pt = P + (int64_t)t * (nt ? nt->n_nodes : 0);
    double* lpt = lp + (int64_t)t * n;
    with_value<0, 2>(stack_kind(K), [&](auto stk) {
      with_flag(evals != nullptr, [&](auto c) {
        hipLaunchKernelGGL((node_kernel<decltype(stk)::value, decltype(c)::value>), dim3(nb),
                           dim3(kBlock), 0, s, x, node, n, Pt, K, lpt, evals, status);
      });
    });
  }
}

void launch_segment_res(double* lp, const int64_t* off, int32_t n_nodes, double* res,
                        int* status, bool poison, hipStream_t s, int* counters,
                        const NodeSum* ns) {
  if (poison) {
    hipLaunchKernelGGL(node_poison_kernel, dim3(std::max<int32_t>((n_nodes + 255) / 256, 1)),
                       dim3(256), 0, s, res, n_nodes);
  } else if (n_nodes > 0) {
    // the all-reduce / local paths have no host round trip before their sums:
    // the rare kernel always runs first (it exits at once on an empty list)
    launch_node_rare(lp, *ns, counters, n_nodes, 0, s);
    hipLaunchKernelGGL(segment_sum_kernel,
                       dim3(std::min<int32_t>((n_nodes + 3) / 4, kPubBlocks)), dim3(256), 0, s,
                       lp, off, n_nodes, res);
  }
  hipLaunchKernelGGL(node_status_kernel, dim3(1), dim3(64), 0, s, res, n_nodes, status,
                     poison ? 1 : 0, counters);
}

void launch_publish_vec(const double* res, int32_t n, double* out, unsigned long long seq,
                        hipStream_t s) {
  hipLaunchKernelGGL(publish_vec_kernel, dim3(1), dim3(256), 0, s, res, n, out, seq);
}

void launch_node_rare(double* lp, const NodeSum& ns, int* counters, int32_t m, int64_t n,
                      hipStream_t s) {
  const NodeRare R{ns.rare_v, ns.rare_j, counters + 1};
  hipLaunchKernelGGL(node_rare_kernel, dim3(64), dim3(64), 0, s, R, lp, ns.x, ns.P, m, n, *ns.K,
                     ns.mode, ns.status, ns.evals);
}

void launch_segment_sum(const double* lp, const int64_t* off, int32_t n_nodes, double* res,
                        double* out, int* status, unsigned long long seq, hipStream_t s,
                        int* ticket, int* counters, int32_t n_tables, int64_t n,
                        int check_rare) {
  if (n_nodes <= 0) return;
  const int32_t nv = n_nodes * std::max(n_tables, 1);  // virtual nodes t m + j
#if WFPT_PUB_DIAG
  hipLaunchKernelGGL(segment_publish_diag_kernel, dim3((nv + 3) / 4), dim3(256), 0, s, lp, off, nv,
                     status, res, out, seq, ticket, counters, n_nodes, n, check_rare);
#else
  // one node per wave up to kPubBlocks blocks, then several per wave: the
  // blocks' ticket releases serialise on one word
  const int32_t nb = std::min<int32_t>((nv + 3) / 4, kPubBlocks);
  hipLaunchKernelGGL(segment_publish_kernel, dim3(nb), dim3(256), 0, s, lp, off, nv, status, res,
                     out, seq, ticket, counters, n_nodes, n, check_rare);
#endif
}

}  // namespace wfpt
