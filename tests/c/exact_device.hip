// Device probe of the exact path (tests/test_exact_device.py): the two product
// headers hddm_amd/csrc/wfpt_crlibm.hpp and wfpt_exact.hpp compiled for gfx950
// with the library's flags, one element per lane. Test infrastructure only;
// built as hddm_amd/lib/libwfpt_exact_probe.so (hddm_amd/build.py:
// build_probe), never linked into the library.
//
// Each entry allocates, copies, launches on the current device, synchronises
// and frees; it returns the first HIP error code (0 = ok).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../hddm_amd/csrc/wfpt_exact.hpp"

namespace {

constexpr int kBlock = 256;

// fn 0-3: the numbering of tests/c/crlibm_check.cpp; 4: sqrt(x); 5: x / y
__global__ void fn_kernel(int fn, const double* __restrict__ x, const double* __restrict__ y,
                          int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double xi = x[i];
  double r;
  switch (fn) {
    case 0: r = wfpt_cr::cr_exp(xi); break;
    case 1: r = wfpt_cr::cr_log(xi); break;
    case 2: r = wfpt_cr::cr_sin(xi); break;
    case 3: r = wfpt_cr::cr_cube(xi); break;
    case 4: r = sqrt(xi); break;
    default: r = xi / y[i]; break;
  }
  out[i] = r;
}

__global__ void pdf_kernel(const double* __restrict__ x, int64_t n, double v, double sv, double a,
                           double z, double sz, double t, double st, double err, int n_st,
                           int n_sz, int use_adaptive, double simps_err, double* __restrict__ out,
                           int64_t* __restrict__ ne, int32_t* __restrict__ ovf) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  wfpt_x::Ctx C;
  out[i] = wfpt_x::full_pdf(x[i], v, sv, a, z, sz, t, st, err, n_st, n_sz, use_adaptive,
                            simps_err, C);
  ne[i] = C.ne;
  ovf[i] = C.ovf;
}

// Device buffers of one call, freed on every return path.
struct Buffers {
  void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int used = 0;
  hipError_t alloc(void** d, size_t bytes) {
    const hipError_t e = hipMalloc(d, bytes);
    if (e == hipSuccess) p[used++] = *d;
    return e;
  }
  ~Buffers() {
    for (int i = 0; i < used; ++i) (void)hipFree(p[i]);
  }
};

#define PROBE_CHECK(call)                  \
  do {                                     \
    const hipError_t e_ = (call);          \
    if (e_ != hipSuccess) return (int)e_;  \
  } while (0)

}  // namespace

extern "C" int probe_fn(int fn, const double* x, const double* y, int64_t n, double* out) {
  if (fn < 0 || fn > 5 || !x || !out || (fn == 5 && !y) || n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = (size_t)n * sizeof(double);
  Buffers B;
  void *dx, *dy = nullptr, *dout;
  PROBE_CHECK(B.alloc(&dx, bytes));
  PROBE_CHECK(B.alloc(&dout, bytes));
  PROBE_CHECK(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice));
  if (fn == 5) {
    PROBE_CHECK(B.alloc(&dy, bytes));
    PROBE_CHECK(hipMemcpy(dy, y, bytes, hipMemcpyHostToDevice));
  }
  const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
  fn_kernel<<<grid, kBlock>>>(fn, (const double*)dx, (const double*)dy, n, (double*)dout);
  PROBE_CHECK(hipGetLastError());
  PROBE_CHECK(hipDeviceSynchronize());
  PROBE_CHECK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int probe_exact_pdf(const double* x, int64_t n, double v, double sv, double a, double z,
                               double sz, double t, double st, double err, int n_st, int n_sz,
                               int use_adaptive, double simps_err, double* out, int64_t* ne,
                               int32_t* ovf) {
  if (!x || !out || !ne || !ovf || n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  Buffers B;
  void *dx, *dout, *dne, *dovf;
  PROBE_CHECK(B.alloc(&dx, (size_t)n * sizeof(double)));
  PROBE_CHECK(B.alloc(&dout, (size_t)n * sizeof(double)));
  PROBE_CHECK(B.alloc(&dne, (size_t)n * sizeof(int64_t)));
  PROBE_CHECK(B.alloc(&dovf, (size_t)n * sizeof(int32_t)));
  PROBE_CHECK(hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
  pdf_kernel<<<grid, kBlock>>>((const double*)dx, n, v, sv, a, z, sz, t, st, err, n_st, n_sz,
                               use_adaptive, simps_err, (double*)dout, (int64_t*)dne,
                               (int32_t*)dovf);
  PROBE_CHECK(hipGetLastError());
  PROBE_CHECK(hipDeviceSynchronize());
  PROBE_CHECK(hipMemcpy(out, dout, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  PROBE_CHECK(hipMemcpy(ne, dne, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
  PROBE_CHECK(hipMemcpy(ovf, dovf, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return 0;
}
