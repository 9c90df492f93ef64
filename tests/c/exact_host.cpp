// Host build of the exact path (hddm_amd/csrc/wfpt_exact.hpp) for
// tests/test_exact_path.py: per-trial full_pdf, compared with the oracle.
#include <stdint.h>
#include "../../hddm_amd/csrc/wfpt_exact.hpp"
extern "C" void exact_pdf_array(const double* x, int64_t n, double v, double sv, double a,
                                double z, double sz, double t, double st, double err, int n_st,
                                int n_sz, int use_adaptive, double simps_err, double* out) {
  for (int64_t i = 0; i < n; ++i) {
    wfpt_x::Ctx C;
    out[i] = wfpt_x::full_pdf(x[i], v, sv, a, z, sz, t, st, err, n_st, n_sz, use_adaptive,
                              simps_err, C);
  }
}
// The host build of the correctly rounded libm, fn as in tests/c/crlibm_check.cpp
// (0-3: cr_exp, cr_log, cr_sin, cr_cube): what the device probe's values are
// compared with.
extern "C" void cr_fn_array(int fn, const double* x, int64_t n, double* out) {
  for (int64_t i = 0; i < n; ++i) {
    switch (fn) {
      case 0: out[i] = wfpt_cr::cr_exp(x[i]); break;
      case 1: out[i] = wfpt_cr::cr_log(x[i]); break;
      case 2: out[i] = wfpt_cr::cr_sin(x[i]); break;
      default: out[i] = wfpt_cr::cr_cube(x[i]); break;
    }
  }
}
// exact_pdf_array with each trial's Ctx::ne (pdf_sv evaluations: equal counts mean
// the same tree) and Ctx::ovf, for tests/test_exact_device.py.
extern "C" void exact_pdf_array_ex(const double* x, int64_t n, double v, double sv, double a,
                                   double z, double sz, double t, double st, double err, int n_st,
                                   int n_sz, int use_adaptive, double simps_err, double* out,
                                   int64_t* ne, int32_t* ovf) {
  for (int64_t i = 0; i < n; ++i) {
    wfpt_x::Ctx C;
    out[i] = wfpt_x::full_pdf(x[i], v, sv, a, z, sz, t, st, err, n_st, n_sz, use_adaptive,
                              simps_err, C);
    ne[i] = C.ne;
    ovf[i] = C.ovf;
  }
}
