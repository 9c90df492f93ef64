// Host build of the model-comparison pass's update rule
// (hddm_amd/csrc/pointwise_update.hpp) for tests/test_pointwise.py: the same
// walk the device kernels make, one trial after the other.
#include <stdint.h>
#include "../../hddm_amd/csrc/pointwise_update.hpp"
// lp[s * len + i]: sweep s's term of trial i. out[f * len + i], f = lppd,
// p_waic, mean; n_inf[i].
extern "C" void pointwise_host(const double* lp, int64_t S, int64_t len, double* out,
                               int64_t* n_inf) {
  for (int64_t i = 0; i < len; ++i) {
    wfpt_pw::State st{0.0, 0.0, 0.0, 0.0, 0, 0};
    for (int64_t s = 0; s < S; ++s) wfpt_pw::update(st, lp[s * len + i]);
    const wfpt_pw::Result R = wfpt_pw::finish(st, S);
    out[i] = R.lppd;
    out[len + i] = R.p_waic;
    out[2 * len + i] = R.mean;
    n_inf[i] = st.n_inf;
  }
}
