// capi_layout.hpp — the index arithmetic of the RL (capi_rl.cpp) and regression
// (capi_reg.cpp) datasets as pure host functions over plain vectors: they run
// (and are tested) without a GPU; the dataset constructors upload the result.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)
namespace wfpt {
namespace capi {

// rl_internal.h: RlLayout describes the arrays. rc != 0: msg says why.
struct RlHostLayout {
  int rc = 0;
  std::string msg;
  int64_t m = 0;       // scored trials (all but each segment's first; all when by_runs)
  int32_t n_seg = 0;
  int64_t node_max = 0;  // most scored trials in one node
  std::vector<int64_t> caller;  // [n] the caller's index of a stored trial
  std::vector<int64_t> lane_start, lane_out, lane_len;  // [n_seg]
  std::vector<int32_t> lane_node;                       // [n_seg] with node ids
  std::vector<int64_t> step_off;                        // [longest segment + 1]
  std::vector<unsigned char> resp_t;                    // [n] step-major
  std::vector<double> fb_t;                             // [n] step-major
  std::vector<double> x_c;            // [m] RTs of the scored trials (empty without RTs)
  std::vector<unsigned char> resp_c;  // [m] their responses
  std::vector<int32_t> node_c;        // [m] their nodes (with node ids)
  std::vector<int64_t> c2caller;      // [m] the caller's index of a compact trial
  std::vector<int64_t> node_off;      // [n_nodes + 1] compact range of each node
};
// by_runs: segments are the runs of equal adjacent split_by values, every
// trial scored (wfpt.pyx:300-318), with node ids the runs inside each node,
// trials node-major (a node boundary always starts a segment: the RL
// regression data set, capi_rl_reg.cpp); else the (node, condition) groups, conditions
// rising as np.unique gives them, the caller's order kept inside a group
// (wfpt.pyx:114-116), each group's first trial unscored. rt, node_id: nullable.
RlHostLayout rl_layout_host(const double* rt, const int64_t* response, const double* feedback,
                            const int64_t* split_by, int64_t n, const int32_t* node_id,
                            int32_t n_nodes, bool by_runs);

// Trials group-major (the caller's order kept inside a group), the design
// matrix column-major so that a column is contiguous over trials.
struct RegHostLayout {
  int rc = 0;
  std::string msg;
  bool identity = true;         // stored order == the caller's order
  int64_t group_max = 0;        // most trials in one group
  std::vector<int64_t> caller;  // [n] the caller's index of a stored trial
  std::vector<int64_t> off;     // [G + 1] stored range of each group
  std::vector<double> x;        // [n] signed RTs, stored order
  std::vector<double> X;        // [C * n] column c at X + c * n, stored order
  std::vector<int32_t> group;   // [n] group of a stored trial (empty without group ids)
};
// group_id nullable: one group (n_groups is then not read).
RegHostLayout reg_layout_host(const double* rt, int64_t n, const double* X, int32_t C,
                              const int32_t* group_id, int32_t n_groups);

}  // namespace capi
}  // namespace wfpt
#pragma GCC visibility pop
