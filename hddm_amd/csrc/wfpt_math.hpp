// wfpt_math.hpp — the device density's elementary functions for gfx950, fp64:
// sin / cos of pi w, the fitted exponentials and logarithm, the fused series
// steps, the fp32 estimates' hardware functions and the register-array
// selects. Values only: no decision of the reference is taken here. Device
// code, except the pieces the host tables are built from with the same bits
// (horner_hd, sincospi01, madd / msub).
// Compiled with -ffp-contract=off: no FMA contraction, like the x86-64 build
// of the reference.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace wfpt {

// One Horner step of sincospi01: on the device a three-operand v_fma_f64 with
// the coefficient in SGPRs (see horner below: fma() costs a v_mov_b64 per
// step there), on the host fma() (the host builds the sine tables from the same
// correctly rounded operations, so both produce the same bits).
__host__ __device__ inline double horner_hd(double p, double r, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(p), "v"(r), "s"(c));
  return d;
#else
  return fma(p, r, c);
#endif
}

// sin(pi w) and cos(pi w) for w in [0, 1] (the only range full_pdf produces:
// validity + flip keep every z node in [0, 1]). Exact reduction t = 2w,
// n = rint(t), f = t - n in [-1/2, 1/2], x = f pi/2 in [-pi/4, pi/4]; Taylor
// polynomials to x^17 / x^18 (truncation < 1e-19) by FMA Horner: <= 1.1 ulp
// relative (checked against 120-bit arithmetic). 30 fp64 ops instead of OCML's
// general-range sincospi (127). w == 1 is seeded with the reference's own
// sin(fl(pi)) = 1.2246e-16 so the z = 1 edge keeps its nonzero value.
__host__ __device__ inline void sincospi01(double w, double& s, double& c) {
  const double t = 2.0 * w;
  const double n = rint(t);
  const double f = t - n;
  const double x = f * 1.5707963267948966;  // pi/2
  const double x2 = x * x;
  double ps = 0x1.952c77030ad4ap-49;
  ps = horner_hd(ps, x2, -0x1.ae7f3e733b81fp-41);
  ps = horner_hd(ps, x2, 0x1.6124613a86d09p-33);
  ps = horner_hd(ps, x2, -0x1.ae64567f544e4p-26);
  ps = horner_hd(ps, x2, 0x1.71de3a556c734p-19);
  ps = horner_hd(ps, x2, -0x1.a01a01a01a01ap-13);
  ps = horner_hd(ps, x2, 0x1.1111111111111p-7);
  ps = horner_hd(ps, x2, -0x1.5555555555555p-3);
  const double sx = fma(x * x2, ps, x);
  double pc = -0x1.6827863b97d97p-53;
  pc = horner_hd(pc, x2, 0x1.ae7f3e733b81fp-45);
  pc = horner_hd(pc, x2, -0x1.93974a8c07c9dp-37);
  pc = horner_hd(pc, x2, 0x1.1eed8eff8d898p-29);
  pc = horner_hd(pc, x2, -0x1.27e4fb7789f5cp-22);
  pc = horner_hd(pc, x2, 0x1.a01a01a01a01ap-16);
  pc = horner_hd(pc, x2, -0x1.6c16c16c16c17p-10);
  pc = horner_hd(pc, x2, 0x1.5555555555555p-5);
  const double cx = fma(x2 * x2, pc, fma(-0.5, x2, 1.0));
  const bool q1 = n == 1.0, q2 = n == 2.0;
  s = q1 ? cx : (q2 ? -sx : sx);
  c = q1 ? -sx : (q2 ? -cx : cx);
  if (w == 1.0) {
    s = 1.2246467991473532e-16;  // sin(M_PI) in double, as the reference computes
    c = -1.0;
  }
}

// Hardware fp32 log / sqrt / reciprocal for the estimate (v_log_f32,
// v_sqrt_f32, v_rcp_f32: ~1 ulp on the normal range these arguments stay in,
// i.e. relative errors ~1e-7 in kl / ks, 100x inside the 1e-5 guard band).
__device__ inline float log32(float x) { return __builtin_amdgcn_logf(x) * 0.69314718055994531f; }
__device__ inline float sqrt32(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ inline float rcp32(float x) { return __builtin_amdgcn_rcpf(x); }

// Series accumulation c + a b. Values only (never a decision input: the series
// choice, K and the Simpson stop tests use the reference's operations, and a
// stop test within kTieBand = 1e-11 of its threshold is re-decided on the exact
// path), so one fused rounding instead of two is within the few-ulp value
// error the recurrences already carry.
__host__ __device__ inline double madd(double a, double b, double c) {
  return fma(a, b, c);
}
// a b - c (the Chebyshev step 2cos(pi w) sin(k pi w) - sin((k-1) pi w))
__host__ __device__ inline double msub(double a, double b, double c) {
  return fma(a, b, -c);
}

// One Horner step p r + c as a single three-operand v_fma_f64. Written with
// fma(), the compiler selects the two-address v_fmac_f64 and, because the
// coefficient c stays live for the next call site, copies it into the
// accumulator first (a v_mov_b64 per step: 9 extra VALU instructions per
// exponential).
__device__ inline double horner(double p, double r, double c) {
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(p), "v"(r), "s"(c));
  return d;
}

// exp(x) for the grid evaluation's finite arguments (series terms and drift
// factors, values only): x = k ln2 + r, |r| <= ln2/2, a degree-11 polynomial
// (Chebyshev-node fit: max relative error 1.2e-16 in double Horner steps),
// then ldexp, which also saturates to inf / 0 / subnormals for |x| > 709. No
// special-case selects (OCML's exp carries them for inf / NaN arguments,
// which the hot call sites never pass: their arguments are bounded by the
// -600 / 600 guards around them; the rare sites use exp_sat).
//
// Tried and not kept, values only like this one: the degree-11 polynomial by
// Estrin's scheme (dependency depth 4 instead of Horner's 11, three more
// operations), and 2^(k/64) from a 64-entry table (global memory or LDS) times
// a degree-5 polynomial (10 fp64 operations and a table load instead of 15, a
// 7-deep chain instead of 13). Estrin was 2.6% slower on the lean pass; the
// table was 2.6% faster there but 7.8% slower on the engine's stress set
// (its loads), and within noise from LDS.
__device__ inline double exp_val(double x) {
  const double k = rint(x * 1.4426950408889634);
  double r = fma(-k, 6.9314718055994529e-01, x);
  r = fma(-k, 2.3190468138462996e-17, r);
  double p = 2.5110037605963777e-08;
  p = horner(p, r, 2.763263963904103e-07);
  p = horner(p, r, 2.755724091857897e-06);
  p = horner(p, r, 2.4801485482328494e-05);
  p = horner(p, r, 1.9841269890047113e-04);
  p = horner(p, r, 1.3888888952314775e-03);
  p = horner(p, r, 8.333333333319601e-03);
  p = horner(p, r, 4.16666666664881e-02);
  p = horner(p, r, 1.666666666666668e-01);
  p = horner(p, r, 5.000000000000019e-01);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)k);
}

// N exponentials at once for the uniform site (lean_uniform_level0): per
// argument exactly exp_val's operations on the same operands in the same
// order, so every result has exp_val's bits, but written level by level
// across the N independent chains. The next instruction of a lone wave then
// never reads the result of the one before it: no hazard no-ops between the
// dependent v_fma_f64 of the last chains, and each coefficient is
// materialised once per level, not once per chain.
template <int N>
__device__ inline void exp_val_n(const double (&x)[N], double (&y)[N]) {
  constexpr double kC[9] = {2.763263963904103e-07,  2.755724091857897e-06, 2.4801485482328494e-05,
                            1.9841269890047113e-04, 1.3888888952314775e-03, 8.333333333319601e-03,
                            4.16666666664881e-02,   1.666666666666668e-01,  5.000000000000019e-01};
  double k[N], r[N], p[N];
#pragma unroll
  for (int i = 0; i < N; ++i) k[i] = rint(x[i] * 1.4426950408889634);
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = fma(-k[i], 6.9314718055994529e-01, x[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = fma(-k[i], 2.3190468138462996e-17, r[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = 2.5110037605963777e-08;
#pragma unroll
  for (int l = 0; l < 9; ++l) {
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = horner(p[i], r[i], kC[l]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = fma(p[i], r[i], 1.0);
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = fma(p[i], r[i], 1.0);
#pragma unroll
  for (int i = 0; i < N; ++i) y[i] = ldexp(p[i], (int)k[i]);
}

// Exponentials of the single-node path (tnode_ftt / tnode_pdf_sv): values
// only, the fitted exp with its argument clamped to [-1100, 1100] (exp_val
// would make NaN of +-inf; the clamp keeps 0 / inf and NaN).
__device__ inline double exp_node(double x) {
  x = x < -1100.0 ? -1100.0 : (x > 1100.0 ? 1100.0 : x);
  return exp_val(x);
}

// The rare paths' exponentials, whose arguments can be infinite (|v| ~ 1e154
// makes v^2 x overflow; a subnormal tt makes the exponent multiplier
// overflow): libm's exp, which gives 0 for -inf like the reference
// (exp_val's range reduction would make NaN of it).
__device__ inline double exp_sat(double x) { return exp(x); }

// log of a trial's density term (wfpt.pyx:44, :70 — every per-trial log the
// kernels emit). Values only: the published fdlibm reduction x = 2^k (1 + f),
// sqrt(2)/2 <= 1 + f < sqrt(2), s = f / (2 + f) (hardware reciprocal + two
// Newton steps + one residual correction), log(1 + f) = f - (hfsq - s (hfsq +
// R(s^2))) with fdlibm's degree-7 R, plus k ln2 in two parts. <= 0.81 ulp
// (2e7 random arguments incl. subnormals against long double, unbiased), 38
// VALU operations against OCML's double-double log (~98). Zero, negative,
// infinite and NaN arguments take OCML's log.
__device__ inline double log_val(double x) {
  if (!(x > 0.0 && x < __builtin_inf())) return log(x);
  int e;
  double m = frexp(x, &e);
  if (m < 0.70710678118654752440) {
    m = m + m;
    e -= 1;
  }
  const double f = m - 1.0;
  const double d = 2.0 + f;
  double r = __builtin_amdgcn_rcp(d);
  r = fma(r, fma(-d, r, 1.0), r);
  r = fma(r, fma(-d, r, 1.0), r);
  double sq = f * r;
  sq = fma(r, fma(-d, sq, f), sq);
  const double z = sq * sq, w = z * z;
  const double t1 = w * horner(fma(w, 1.531383769920937332e-01, 2.222219843214978396e-01), w,
                               3.999999999940941908e-01);
  const double t2 = z * horner(horner(fma(w, 1.479819860511658591e-01, 1.818357216161805012e-01),
                                      w, 2.857142874366239149e-01),
                               w, 6.666666666666735130e-01);
  const double R = t2 + t1;
  const double hfsq = (0.5 * f) * f;
  const double k = (double)e;
  return k * 6.93147180369123816490e-01 -
         ((hfsq - fma(sq, hfsq + R, k * 1.90821492927058770002e-10)) - f);
}

// Element i (a run-time index) of a 5-element register array, and its store:
// selects, so the array stays in registers inside a non-unrolled loop.
// Written out with constant subscripts (no loop): every access is a constant
// index from the start, so the array is split into registers, never
// promoted to memory.
__device__ inline double pick5(const double (&v)[5], int i) {
  const double a0 = v[0], a1 = v[1], a2 = v[2], a3 = v[3], a4 = v[4];
  return i == 0 ? a0 : i == 1 ? a1 : i == 2 ? a2 : i == 3 ? a3 : a4;
}
__device__ inline void put5(double (&v)[5], int i, double x) {
  v[0] = i == 0 ? x : v[0];
  v[1] = i == 1 ? x : v[1];
  v[2] = i == 2 ? x : v[2];
  v[3] = i == 3 ? x : v[3];
  v[4] = i == 4 ? x : v[4];
}

// The clean test's running minimum (lean_uniform_level0) as one v_min_f64.
// fmin() first quiets every operand the compiler cannot prove canonical (a
// v_max_f64 x, x per series value); the test does not care whether a NaN
// operand is passed over or returned.
__device__ inline double min_raw(double a, double b) {
  double d;
  asm("v_min_f64 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}

}  // namespace wfpt
