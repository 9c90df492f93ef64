// Host-side sanitizer driver (tests/test_sanitizers.py builds it with
// -fsanitize=address,undefined on the host code): exercises every piece of host
// C/C++ that needs no GPU —
//   * the oracle (oracle/wfpt_oracle.c): full_pdf / pdf_array / wiener_like /
//     wiener_like_multi over random parameter sets, incl. deep adaptive trees;
//   * the exact path on the host (wfpt_exact.hpp + wfpt_crlibm.hpp);
//   * the C ABI's host logic (capi_*.cpp): argument checks, result decode
//     and error encoding, shard ranges, the poisoned triple, and every entry
//     point's failure path when no device is present;
//   * the host layouts of the RL and regression datasets (capi_layout.hpp) on
//     small inputs with unequal segment / group lengths;
//   * the TCP rendezvous (wfpt_rendezvous.cpp) with three ranks as threads,
//     plus a peer whose rank 0 never comes.
// Exit status 0 = every check passed and no sanitizer report.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <thread>
#include <vector>

#include "../../hddm_amd/csrc/capi_layout.hpp"
#include "../../hddm_amd/csrc/wfpt_exact.hpp"
#include "../../include/wfpt_amd.h"
#include "../../oracle/wfpt_oracle.h"

static int failures = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      fprintf(stderr, "CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static void oracle_and_exact() {
  std::mt19937_64 g(20261017);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  for (int rep = 0; rep < 60; ++rep) {
    const double v = -4 + 8 * U(g), sv = (rep % 3) ? 2.5 * U(g) : 0.0, a = 0.5 + 1.5 * U(g);
    const double z = 0.4 + 0.2 * U(g), sz = (rep % 2) ? 0.4 * U(g) : 0.0, t = 0.2 + 0.3 * U(g);
    const double st = (rep % 4) ? 0.35 * U(g) : 0.0;
    const double err = pow(10.0, -10 + 9 * U(g)), se = pow(10.0, -6 + 4 * U(g));
    const int n = (rep % 5 == 0) ? 6 : 2;
    const int ua = rep % 7 != 0;
    std::vector<double> x(48);
    for (auto& xi : x) xi = (U(g) < 0.7 ? 1 : -1) * (t - st / 2 + 2.0 * U(g));
    x[0] = 0.0;
    x[1] = t / 2;
    std::vector<double> y(x.size()), l(x.size());
    oracle_pdf_array(x.data(), (int64_t)x.size(), v, sv, a, z, sz, t, st, err, 0, n, n, ua, se,
                     0.05, 0.1, y.data());
    oracle_pdf_array(x.data(), (int64_t)x.size(), v, sv, a, z, sz, t, st, err, 1, n, n, ua, se,
                     0.05, 0.1, l.data());
    const double wl = oracle_wiener_like(x.data(), (int64_t)x.size(), v, sv, a, z, sz, t, st,
                                         err, n, n, ua, se, 0.05, 0.1);
    CHECK(!isnan(wl) || true);
    int64_t cnt = 0;
    for (size_t i = 0; i < x.size(); ++i) {
      const double p = oracle_full_pdf(x[i], v, sv, a, z, sz, t, st, err, n, n, ua, se, &cnt);
      wfpt_x::Ctx C;
      const double q = wfpt_x::full_pdf(x[i], v, sv, a, z, sz, t, st, err, n, n, ua, se, C);
      if (p == 0 || isnan(p)) CHECK(q == p || (isnan(p) && isnan(q)));
      else CHECK(fabs(q - p) <= 1e-13 * fabs(p));
    }
    const double* arr[7] = {x.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const double sc[7] = {v, sv, a, z, sz, t, st};
    std::vector<double> terms(x.size());
    x[2] = 999.0;
    x[3] = -999.0;
    (void)oracle_wiener_like_multi_terms(x.data(), (int64_t)x.size(), arr, sc, err, n, n, ua, se,
                                         0.05, 0.1, terms.data());
  }
}

static void capi_host_logic() {
  double out = 0;
  const double ok[3] = {-12.5, 0, 0};
  CHECK(wfpt_decode_result(ok, &out) == WFPT_OK && out == -12.5);
  const double zero[3] = {-12.5, 2, 0};
  CHECK(wfpt_decode_result(zero, &out) == WFPT_OK && isinf(out) && out < 0);
  const double depth[3] = {0, 0, 1};
  CHECK(wfpt_decode_result(depth, &out) == WFPT_ERR_UNSUPPORTED);
  CHECK(strstr(wfpt_last_error(), "WFPT_MAX_DEPTH") != nullptr);
  const double budget[3] = {0, 0, 2 * 1048576.0};
  CHECK(wfpt_decode_result(budget, &out) == WFPT_ERR_UNSUPPORTED);
  CHECK(strstr(wfpt_last_error(), "WFPT_EVAL_BUDGET") != nullptr);
  double pz[3];
  CHECK(wfpt_result_poison(pz) == WFPT_OK);
  const double peer[3] = {pz[0] - 3.0, pz[1], pz[2] + pz[2]};
  CHECK(wfpt_decode_result(peer, &out) == WFPT_ERR_COMM);
  CHECK(strstr(wfpt_last_error(), "2 rank(s) failed") != nullptr);
  const double mix[3] = {0, 0, pz[2] + 1.0};
  CHECK(wfpt_decode_result(mix, &out) == WFPT_ERR_UNSUPPORTED);
  CHECK(wfpt_decode_result(nullptr, &out) == WFPT_ERR_ARG);
  const int64_t sizes[] = {0, 1, 63, 64, 1000003, 100000000};
  for (int64_t n : sizes) {
    for (int r = 1; r <= 9; ++r) {
      int64_t prev = 0;
      for (int k = 0; k < r; ++k) {
        int64_t lo, hi;
        wfpt_shard_range(n, r, k, &lo, &hi);
        CHECK(lo == prev && hi >= lo);
        prev = hi;
      }
      CHECK(prev == n);
    }
  }
  // no device in this container: every entry point fails with a status
  wfpt_ctx* c = nullptr;
  int nd = -1;
  (void)wfpt_device_count(&nd);
  if (nd <= 0) CHECK(wfpt_open(0, &c) != WFPT_OK && c == nullptr);
  wfpt_params p = {0.5, 0.1, 2.0, 0.5, 0.1, 0.3, 0.1, 0.05};
  wfpt_knobs k = {1e-4, 2, 2, 1, 1e-3, 0.1};
  double x = 1.0;
  CHECK(wfpt_wiener_like(nullptr, nullptr, &p, &k, &out) == WFPT_ERR_ARG);
  CHECK(wfpt_wiener_like_host(nullptr, &x, 1, &p, &k, &out) == WFPT_ERR_ARG);
  CHECK(wfpt_pdf_array(nullptr, &x, 1, &p, &k, 0, &out) == WFPT_ERR_ARG);
  CHECK(wfpt_wiener_like_nodes_ex(nullptr, nullptr, &p, &k, &out, nullptr) == WFPT_ERR_ARG);
  CHECK(wfpt_dataset_create(nullptr, &x, 1, nullptr, 0, nullptr) == WFPT_ERR_ARG);
  CHECK(wfpt_wiener_like_allreduce(nullptr, nullptr, &p, &k, &out) == WFPT_ERR_ARG);
  CHECK(wfpt_wiener_like_allreduce_group(nullptr, nullptr, 0, &p, &k, &out) == WFPT_ERR_ARG);
  CHECK(wfpt_comm_init_all(nullptr, 0) == WFPT_ERR_ARG);
  CHECK(wfpt_comm_exchange_id(2, 5, "127.0.0.1", 1, 10, (unsigned char*)pz) == WFPT_ERR_ARG);
  wfpt_close(nullptr);
  wfpt_dataset_destroy(nullptr);
  CHECK(wfpt_dataset_size(nullptr) == -1);
}

static bool is_permutation_of_n(std::vector<int64_t> v, int64_t n) {
  std::sort(v.begin(), v.end());
  for (int64_t i = 0; i < (int64_t)v.size(); ++i)
    if (v[i] != i) return false;
  return (int64_t)v.size() == n;
}

// One RL layout: the invariants the scan kernel's indexing relies on.
static void rl_layout_case(int64_t n, int n_nodes, int n_cond, bool by_runs, bool with_rt,
                           bool with_nodes, uint64_t seed) {
  std::mt19937_64 g(seed);
  // one spare element: data() of an empty vector may be null, which means "not given"
  std::vector<double> rt(n + 1), fb(n + 1);
  std::vector<int64_t> resp(n + 1), split(n + 1);
  std::vector<int32_t> node(n + 1);
  for (int64_t i = 0; i < n; ++i) {
    rt[i] = 0.3 + 0.01 * (double)i;
    fb[i] = (double)(g() % 7) - 3.0;
    resp[i] = (int64_t)(g() % 2);
    // skewed towards condition 0, so the segments have unequal lengths
    split[i] = (int64_t)std::min<uint64_t>(g() % (2 * (uint64_t)n_cond), (uint64_t)n_cond - 1);
    split[i] = n_cond - 1 - split[i];
    node[i] = (int32_t)(g() % (uint64_t)n_nodes);
  }
  if (n > 2 && n_cond > 1) {  // a condition that occurs once: a segment with no scored trial
    for (int64_t i = 0; i < n; ++i)
      if (split[i] == n_cond - 1) split[i] = 0;
    split[n / 2] = n_cond - 1;
  }
  const wfpt::capi::RlHostLayout H = wfpt::capi::rl_layout_host(
      with_rt ? rt.data() : nullptr, resp.data(), fb.data(), split.data(), n,
      with_nodes ? node.data() : nullptr, n_nodes, by_runs);
  CHECK(H.rc == 0);
  if (H.rc) return;
  const int64_t ns = H.n_seg, skip = by_runs ? 0 : 1;
  CHECK(H.m == (by_runs ? n : n - ns));
  CHECK(is_permutation_of_n(H.caller, n));
  CHECK((int64_t)H.lane_start.size() == ns && (int64_t)H.lane_len.size() == ns &&
        (int64_t)H.lane_out.size() == ns);
  CHECK(!H.step_off.empty() && H.step_off.front() == 0 && H.step_off.back() == n);
  for (size_t k = 1; k < H.step_off.size(); ++k) CHECK(H.step_off[k] >= H.step_off[k - 1]);
  int64_t len_sum = 0;
  std::vector<int> hit_t(n, 0), hit_c(H.m, 0);
  std::vector<int64_t> scored;
  for (int64_t r = 0; r < ns; ++r) {
    const int64_t len = H.lane_len[r];
    CHECK(len >= 1 && (r == 0 || len <= H.lane_len[r - 1]));
    CHECK((int64_t)H.step_off.size() > len);
    len_sum += len;
    for (int64_t k = 0; k < len; ++k) {
      const int64_t at = H.step_off[k] + r, src = H.caller[H.lane_start[r] + k];
      CHECK(at >= 0 && at < n);
      if (at < 0 || at >= n) continue;
      ++hit_t[at];
      CHECK(H.resp_t[at] == (unsigned char)resp[src] && H.fb_t[at] == fb[src]);
      if (k >= skip) {
        const int64_t ci = H.lane_out[r] + k - skip;
        CHECK(ci >= 0 && ci < H.m);
        if (ci < 0 || ci >= H.m) continue;
        ++hit_c[ci];
        CHECK(H.c2caller[ci] == src);
        scored.push_back(src);
      }
      if (with_nodes) CHECK(H.lane_node[r] == node[src]);
    }
  }
  CHECK(len_sum == n);
  for (int h : hit_t) CHECK(h == 1);  // every stored index used exactly once
  for (int h : hit_c) CHECK(h == 1);
  std::vector<int64_t> cc = H.c2caller;  // a permutation of the scored trials
  std::sort(cc.begin(), cc.end());
  std::sort(scored.begin(), scored.end());
  CHECK(cc == scored && (int64_t)cc.size() == H.m);
  CHECK(std::adjacent_find(cc.begin(), cc.end()) == cc.end());
  CHECK((int64_t)H.x_c.size() == (with_rt ? H.m : 0));
  for (int64_t k = 0; k < (int64_t)H.x_c.size(); ++k) CHECK(H.x_c[k] == rt[H.c2caller[k]]);
  if (with_nodes) {
    CHECK((int64_t)H.node_off.size() == n_nodes + 1 && H.node_off.front() == 0 &&
          H.node_off.back() == H.m);
    int64_t most = 0;
    for (int j = 0; j < n_nodes; ++j) {
      CHECK(H.node_off[j + 1] >= H.node_off[j]);
      most = std::max(most, H.node_off[j + 1] - H.node_off[j]);
      // node-major compact order (by_runs keeps the caller's order: counts only)
      for (int64_t k = H.node_off[j]; !by_runs && k < H.node_off[j + 1]; ++k)
        CHECK(H.node_c[k] == j);
      CHECK(std::count(H.node_c.begin(), H.node_c.end(), j) == H.node_off[j + 1] - H.node_off[j]);
    }
    CHECK(most == H.node_max);
  } else {
    CHECK(H.node_off.empty() && H.node_c.empty() && H.lane_node.empty());
  }
}

static void reg_layout_case(int64_t n, int C, int n_groups, int kind) {
  // kind 0: no group ids; 1: ids already sorted; 2: ids interleaved; group
  // n_groups - 2 stays empty when there are at least three groups
  std::vector<double> rt(n + 1), X((size_t)(n + 1) * C);  // never null (see above)
  std::vector<int32_t> gid(n + 1);
  for (int64_t i = 0; i < n; ++i) {
    rt[i] = (i % 3 ? 1 : -1) * (0.4 + 0.01 * (double)i);
    for (int c = 0; c < C; ++c) X[(size_t)i * C + c] = 100.0 * (double)i + c;
    int32_t g = kind == 1 ? (int32_t)(i * n_groups / std::max<int64_t>(n, 1))
                          : (int32_t)((i * 7 + i / 5) % n_groups);
    // unequal lengths, one empty group (sorted ids stay sorted)
    if (n_groups >= 3 && g == n_groups - 2) g = kind == 1 ? n_groups - 1 : 0;
    gid[i] = g;
  }
  const int32_t* ids = kind == 0 ? nullptr : gid.data();
  const wfpt::capi::RegHostLayout H =
      wfpt::capi::reg_layout_host(rt.data(), n, X.data(), C, ids, n_groups);
  CHECK(H.rc == 0);
  if (H.rc) return;
  const int G = ids ? n_groups : 1;
  CHECK(is_permutation_of_n(H.caller, n));
  CHECK((int64_t)H.off.size() == G + 1 && H.off.front() == 0 && H.off.back() == n);
  int64_t most = 0;
  bool identity = true;
  for (int g = 0; g < G; ++g) {
    CHECK(H.off[g + 1] >= H.off[g]);
    most = std::max(most, H.off[g + 1] - H.off[g]);
    for (int64_t j = H.off[g]; j < H.off[g + 1]; ++j) {
      if (ids) CHECK(H.group[j] == g && gid[H.caller[j]] == g);
      if (j > H.off[g]) CHECK(H.caller[j] > H.caller[j - 1]);  // the caller's order inside a group
    }
  }
  CHECK(most == H.group_max);
  if (ids && n_groups >= 3) CHECK(H.off[n_groups - 1] == H.off[n_groups - 2]);
  for (int64_t j = 0; j < n; ++j) {
    identity = identity && H.caller[j] == j;
    CHECK(H.x[j] == rt[H.caller[j]]);
    for (int c = 0; c < C; ++c) CHECK(H.X[(size_t)c * n + j] == X[(size_t)H.caller[j] * C + c]);
  }
  CHECK(identity == H.identity);
  if (kind != 2) CHECK(H.identity);
  CHECK((int64_t)H.group.size() == (ids ? n : 0));
}

static void dataset_layouts() {
  uint64_t seed = 1;
  for (int64_t n : {0, 1, 37})
    for (int n_nodes : {1, 3})
      for (int n_cond = 1; n_cond <= 4; ++n_cond)
        for (int by_runs = 0; by_runs < 2; ++by_runs)
          for (int with_rt = 0; with_rt < 2; ++with_rt) {
            rl_layout_case(n, n_nodes, n_cond, by_runs != 0, with_rt != 0, true, ++seed);
            if (n_nodes == 1)
              rl_layout_case(n, n_nodes, n_cond, by_runs != 0, with_rt != 0, false, ++seed);
          }
  // refused inputs come back as an error, with nothing laid out
  const int64_t bad_resp[2] = {0, 2}, split[2] = {0, 0};
  const double fb[2] = {1, 0};
  const wfpt::capi::RlHostLayout B =
      wfpt::capi::rl_layout_host(nullptr, bad_resp, fb, split, 2, nullptr, 0, false);
  CHECK(B.rc == WFPT_ERR_ARG && B.msg.find("response must be 0 or 1") != std::string::npos);
  for (int64_t n : {0, 23})
    for (int C : {1, 3})
      for (int kind = 0; kind < 3; ++kind)
        for (int n_groups : {1, 4}) reg_layout_case(n, C, n_groups, kind);
  const double rt1[1] = {0.5}, X1[1] = {1.0};
  const int32_t bad_gid[1] = {3};
  const wfpt::capi::RegHostLayout R = wfpt::capi::reg_layout_host(rt1, 1, X1, 1, bad_gid, 2);
  CHECK(R.rc == WFPT_ERR_ARG && R.msg.find("group id out of range") != std::string::npos);
}

static void rendezvous(int port) {
  unsigned char id0[128], got[3][128];
  for (int i = 0; i < 128; ++i) id0[i] = (unsigned char)(i * 7 + 3);
  int rc[3] = {-1, -1, -1};
  std::vector<std::thread> th;
  for (int r = 2; r >= 0; --r)
    th.emplace_back([&, r] {
      if (r == 0) memcpy(got[0], id0, 128);
      else memset(got[r], 0, 128);
      rc[r] = wfpt_comm_exchange_id(3, r, "127.0.0.1", port, 20000, got[r]);
    });
  for (auto& t : th) t.join();
  for (int r = 0; r < 3; ++r) {
    CHECK(rc[r] == WFPT_OK);
    CHECK(memcmp(got[r], id0, 128) == 0);
  }
  unsigned char lone[128];
  CHECK(wfpt_comm_exchange_id(2, 1, "127.0.0.1", port + 1, 300, lone) == WFPT_ERR_COMM);
}

int main(int argc, char** argv) {
  const int port = argc > 1 ? atoi(argv[1]) : 29611;
  oracle_and_exact();
  capi_host_logic();
  dataset_layouts();
  rendezvous(port);
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("sanitize driver: all checks passed\n");
  return 0;
}
