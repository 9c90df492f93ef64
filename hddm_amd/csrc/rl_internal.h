// rl_internal.h — launcher interface between the C ABI (capi_*.cpp) and the
// reinforcement-learning kernels (rl_kernels.hip). Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wfpt {
struct Params;


// One Q-learning row (wfpt.pyx:83): the start value of both Q values, the two
// learning rates already squashed on the host (pow(2.718281828459, alpha) /
// (1 + pow(2.718281828459, alpha)), wfpt.pyx:123-125) and the drift scaling v.
struct RlRow {
  double q, alfa, pos_alfa, v;
};

// Device layout of an RL dataset's fixed inputs. A segment is
// one Q recurrence: the trials of one (node, condition) pair, or, for
// wiener_like_multi_rlddm, one run of equal adjacent split_by values. Trials
// are held segment-major ("stored order": segment after segment, the caller's
// order inside a segment). One lane scans one segment; lanes are the segments
// ordered by falling length, so a wave's lanes run similar trip counts.
// Response and feedback are stored step-major over the lanes: step k of lane
// r is element step_off[k] + r (only the lanes with more than k trials have
// one, and they are the first ones), so the lanes of a wave read consecutive
// addresses in every step.
struct RlLayout {
  int32_t n_seg;
  const int64_t* lane_start;  // [n_seg] stored index of the segment's first trial
  const int64_t* lane_out;    // [n_seg] compact index of its first scored trial
  const int64_t* lane_len;    // [n_seg] trials of the segment (>= 1)
  const int32_t* lane_node;   // [n_seg] node of the segment (null: one node)
  const int64_t* step_off;    // [longest segment + 1]
  const unsigned char* resp_t;  // [n] responses (0 / 1), step-major
  const double* fb_t;           // [n] feedback, step-major
  const int64_t* caller;      // [n] the caller's index of a stored trial (null: identity)
  int score_first;  // 1: every trial is scored (wfpt.pyx:300-318); 0: all but a segment's first
};

// The recurrence of wfpt.pyx:118-153 (rows / one, score_first = 0) or
// wfpt.pyx:298-318 (vmul / rate per trial, score_first = 1), one lane per
// segment. drift_c[compact index] = the drift (qs[1] - qs[0]) * v the
// recurrence holds at a scored trial; drift_in (nullable, n): the same for
// every trial, in the caller's order. rows (nullable, device): one row per
// node, else `one`. vmul / rate (nullable, device, n, stored order): the
// trial's drift scaling / learning rate instead of the row's.
void launch_rl_scan(const RlLayout& L, const RlRow& one, const RlRow* rows,
                    const double* vmul, const double* rate, double* drift_c,
                    double* drift_in, hipStream_t s);

// The shape of a multi-table node batch: n_tables row tables of n_nodes rows
// over a dataset of n trials, m of them scored.
struct RlTables {
  int32_t n_tables, n_nodes;
  int64_t m, n;
};

// launch_rl_scan with the rows of T.n_tables tables (rows[t n_nodes + node]),
// one lane per (table, segment): table t's drifts at drift_c[t m ..] and
// drift_in[t n ..] (nullable), each bit for bit the one-table scan's with that
// table's rows. n_tables x n_seg must fit an int32_t.
void launch_rl_scan_multi(const RlLayout& L, const RlTables& T, const RlRow* rows,
                          double* drift_c, double* drift_in, hipStream_t s);

// wiener_like_rl's choice probability (wfpt.pyx:210-227) of m compact trials:
// lp[i] = log(p (1 - p_outlier) + wp_outlier), then the per-block sums into
// part / zeros (blocks_for(m) of them, lp_sum_kernel's order) for
// launch_finalize.
void launch_rl_choice(const double* drift_c, const unsigned char* resp_c, int64_t m,
                      double z, double p_outlier, double wp_outlier, double* lp,
                      double* part, int* zeros, hipStream_t s);

// Node rows -> per-trial arrays: dst[slot * m + i] = field f of P[node_c[i]]
// for every field f (1 = sv .. 6 = st; wfpt_params order) whose bit is set in
// mask, slots counted over the set bits in rising order.
void launch_rl_fill(const int32_t* node_c, int64_t m, const Params* P, int mask,
                    double* dst, hipStream_t s);

// launch_rl_fill over T.n_tables tables: dst[slot * (n_tables m) + t m + i] =
// field f of P[t n_nodes + node_c[i]].
void launch_rl_fill_multi(const int32_t* node_c, const RlTables& T, const Params* P, int mask,
                          double* dst, hipStream_t s);

// res[j] = the sum of lp[off[j] .. off[j + 1]) in the order lp_sum_kernel +
// finalize_kernel (one block) add a call's terms: bit for bit the sum of the
// single-node call over that node's trials. scratch: rl_node_partials(m,
// n_nodes) doubles. A node may hold at most kRlNodeMax scored trials (beyond
// it the single-node call's finalize splits over blocks, another order).
constexpr int64_t kRlNodeMax = 2 * 8192 * 256;
inline int64_t rl_node_partials(int64_t m, int32_t n_nodes) { return m / 256 + n_nodes + 1; }
void launch_rl_node_sum(const double* lp, const int64_t* off, int32_t n_nodes,
                        double* scratch, double* res, hipStream_t s);
}  // namespace wfpt
