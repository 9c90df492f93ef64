/*
 * ORACLE — TEST INFRASTRUCTURE ONLY.
 *
 * Plain-C CPU restatement of the reference's DMAT / Tuerlinckx (2004) CDF:
 * cdfdif (/root/reference/src/cdfdif.c:59-221) and its array wrapper
 * dmat_cdf_array (/root/reference/src/cdfdif_wrapper.pyx:16-53), written as
 * separate steps (quadrature set-up, boundary probability, the two series)
 * with each expression in the reference's operation order, so that it gives
 * the reference's doubles. Used only by tests/ (pinned to the reference's
 * outputs in tests/golden/cdfdif*.npz) and as the timed CPU baseline of the
 * CDF row (tools/bench_rows.py); the product path (hddm_amd) never loads it.
 *
 * One source, two builds. `real` is double by default; cdfdif_oracle_ld.c
 * defines CD_LONG and includes this file, which makes `real` the x86-64
 * 80-bit long double with the `l` math functions and exports only the `_ld`
 * entry points. Every constant keeps its double-rounded value in both builds
 * (K()), so the two evaluate the same formulae on the same numbers in the
 * same order and differ through rounding alone.
 *
 * Every entry point goes through cd_eval. It either runs the reference's own
 * stop rule with the series cap as a parameter (vcap = 5000 is the
 * reference) and records where each series stopped, or — given the record of
 * such a run — sums exactly those terms with no test of its own (the long
 * double twin: its branch, its zero-drift nodes and its series lengths are
 * the double run's). Alongside F it returns S, the sum of the absolute values
 * of every addend of F at F's final scaling: p0 (1 - x) and p1 x, every term
 * of every series and each closed-form part (ser; sl and su), each after its
 * own multipliers. 2^-52 S is the unit in which the tier tests measure error.
 */
#include <math.h>
#include <stdint.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#ifdef CD_LONG
typedef long double real;
#define RM(f) f##l
#else
typedef double real;
#define RM(f) f
#endif
#define K(c) ((real)(c)) /* a constant at its double value */

#define CD_PI 3.1415926535897932384626433832795028841971693993751
#define CD_VMAX 5000

/* stop[] slots of a cd_record: window series (m, i) at m * 6 + i, the
 * zero-drift series of node m at 36 + m, the series beyond the window at 42.
 * A slot holds the index v of the last term added (CD_VMAX: the stop rule
 * never fired), or -1 for a series that did not run. */
#define CD_NSTOP 43
#define CD_SLOT_ZERO 36
#define CD_SLOT_BEYOND 42
typedef struct {
    int branch; /* 0 below the Ter window, 1 beyond it, 2 inside it */
    int stop[CD_NSTOP];
} cd_record;
typedef struct {
    double S, prob;
    cd_record rec;
} cd_probe;

/* 6-point Gauss-Hermite (drift) and Gauss-Legendre (start point) rules,
 * cdfdif.c:78-81 */
static const double GH_X[6] = {-2.3506049736744922818, -1.3358490740136970132,
                               -.43607741192761650950, .43607741192761650950,
                               1.3358490740136970132, 2.3506049736744922818};
static const double GH_W[6] = {.45300099055088421593e-2, .15706732032114842368,
                               .72462959522439207571, .72462959522439207571,
                               .15706732032114842368, .45300099055088421593e-2};
static const double GL_X[6] = {-.93246951420315193904, -.66120938646626381541,
                               -.23861918608319693247, .23861918608319712676,
                               .66120938646626459256, .93246951420315160597};
static const double GL_W[6] = {.17132449237917049545, .36076157304813916138,
                               .46791393457269092604, .46791393457269092604,
                               .36076157304813843973, .17132449237917132812};

typedef struct {
    real a, ter, eta, z, sz, st, nu, a2;
    real gk[6], wgh[6], gz[6];
} cd_model;

/* How one evaluation runs its series: to the stop rule under the cap `vcap`,
 * writing `rec`; or, with `forced`, through the terms `rec` lists. */
typedef struct {
    int vcap, forced;
    cd_record *rec;
} cd_run;

static void cd_setup(cd_model *M, const double *par)
{
    M->a = par[0];
    M->ter = par[1];
    M->eta = par[2];
    M->z = par[3];
    M->sz = par[4];
    M->st = par[5];
    M->nu = par[6];
    M->a2 = M->a * M->a;
    for (int m = 0; m < 6; m++) {
        M->gk[m] = K(1.41421356237309505) * K(GH_X[m]) * M->eta + M->nu; /* drift nodes */
        M->wgh[m] = K(GH_W[m]) / K(1.772453850905515882);
    }
    for (int i = 0; i < 6; i++)
        M->gz[i] = (K(.5) * M->sz * K(GL_X[i])) + M->z; /* start nodes */
}

/* the reference's |gk| ~ 0 test (cdfdif.c:68); a forced run takes the double
 * run's answer */
static int cd_node_is_zero(const cd_model *M, const cd_run *R, int m)
{
    if (R->forced) return R->rec->stop[CD_SLOT_ZERO + m] >= 0;
    return !(RM(fabs)(M->gk[m]) > K(1e-7));
}

/* P(absorbed at the lower boundary), averaged over drift and start point
 * (cdfdif.c:91-109) */
static real cd_prob(const cd_model *M, const cd_run *R)
{
    real tot = 0;
    for (int i = 0; i < 6; i++) {
        real acc = 0;
        for (int m = 0; m < 6; m++) {
            if (!cd_node_is_zero(M, R, m))
                acc += (RM(exp)(-200 * M->gz[i] * M->gk[m]) - 1) /
                       (RM(exp)(-200 * M->a * M->gk[m]) - 1) * M->wgh[m];
            else
                acc += M->gz[i] / M->a * M->wgh[m];
        }
        tot += acc * K(GL_W[i]) / 2;
    }
    return tot;
}

/* The partial-sum stop rule shared by every series (cdfdif.c:139-141 etc.) */
static int cd_converged(const real h[3])
{
    return (RM(fabs)(h[0] - h[1]) < K(1e-29)) && (RM(fabs)(h[1] - h[2]) < K(1e-29)) && (h[2] > 0);
}

/* After term v of the series in `slot`: 1 when the series ends here. */
static int cd_series_ends(const cd_run *R, int slot, int v, const real h[3])
{
    if (R->forced) return v >= R->rec->stop[slot];
    if (cd_converged(h)) {
        R->rec->stop[slot] = v;
        return 1;
    }
    return 0;
}

/* t beyond the Ter window (cdfdif.c:120-145): the series over v with the
 * drift integral inside each term. *sabs: the sum of |term|. */
static real cd_series_beyond(const cd_model *M, const cd_run *R, real t, int x, real zu, real zl,
                             real up, real lo, real *sabs)
{
    real h[3] = {0, 0, 0};
    real sa = 0;
    const real sgn = 2 * x - 1;
    if (!R->forced) R->rec->stop[CD_SLOT_BEYOND] = CD_VMAX;
    for (int v = 0; v < R->vcap; v++) {
        h[0] = h[1];
        h[1] = h[2];
        real acc = 0;
        const real sifa = K(CD_PI) * v / M->a;
        for (int m = 0; m < 6; m++) {
            const real g = M->gk[m];
            const real den = (100 * g * g + (K(CD_PI) * K(CD_PI)) * (v * v) / (100 * M->a2));
            const real eu = RM(exp)(sgn * zu * g * 100 - 3 * RM(log)(den) + RM(log)(M->wgh[m]) -
                                    2 * RM(log)(K(100)));
            const real el = RM(exp)(sgn * zl * g * 100 - 3 * RM(log)(den) + RM(log)(M->wgh[m]) -
                                    2 * RM(log)(K(100)));
            const real f =
                eu * (sgn * g * RM(sin)(sifa * zu) * 100 - sifa * RM(cos)(sifa * zu)) -
                el * (sgn * g * RM(sin)(sifa * zl) * 100 - sifa * RM(cos)(sifa * zl));
            const real ed = RM(exp)((K(-.5) * den * (t - up)) +
                                    RM(log)(1 - RM(exp)(K(-.5) * den * (up - lo))));
            acc += f * ed;
        }
        h[2] = h[1] + v * acc;
        sa += RM(fabs)(v * acc);
        if (cd_series_ends(R, CD_SLOT_BEYOND, v, h)) break;
    }
    *sabs = sa;
    return h[2];
}

/* t inside the Ter window, drift node m away from zero (cdfdif.c:152-177).
 * *sabs: the sum over i of (|ser| + 4 sum |term|) under the same multipliers. */
static real cd_window_node(const cd_model *M, const cd_run *R, real t, int x, real lo, int m,
                           real *sabs)
{
    const real g = M->gk[m];
    const real a = M->a, a2 = M->a2;
    real tot = 0, sa_tot = 0;
    for (int i = 0; i < 6; i++) {
        const int slot = m * 6 + i;
        const real zz = (a - M->gz[i]) * x + M->gz[i] * (1 - x);
        const real sh = RM(sinh)((1 - 2 * x) * g * a / K(.01));
        const real ser = -((a * a2) / ((1 - 2 * x) * g * K(CD_PI) * K(.01))) *
                             RM(sinh)(zz * (1 - 2 * x) * g / K(.01)) / (sh * sh) +
                         (zz * a2) / ((1 - 2 * x) * g * K(CD_PI) * K(.01)) *
                             RM(cosh)((a - zz) * (1 - 2 * x) * g / K(.01)) / sh;
        real h[3] = {0, 0, 0};
        real sa = 0;
        if (!R->forced) R->rec->stop[slot] = CD_VMAX;
        for (int v = 0; v < R->vcap; v++) {
            h[0] = h[1];
            h[1] = h[2];
            const real sifa = K(CD_PI) * v / a;
            const real den = (g * g * 100 + (K(CD_PI) * v) * (K(CD_PI) * v) / (a2 * 100));
            const real term = v * RM(sin)(sifa * zz) *
                              RM(exp)(K(-.5) * den * (t - lo) - 2 * RM(log)(den));
            h[2] = h[1] + term;
            sa += RM(fabs)(term);
            if (cd_series_ends(R, slot, v, h)) break;
        }
        const real scale = RM(exp)((2 * x - 1) * zz * g * 100);
        tot += K(.5) * K(GL_W[i]) * (ser - 4 * h[2]) * (K(CD_PI) / 100) / (a2 * M->st) * scale;
        sa_tot += K(.5) * K(GL_W[i]) * (RM(fabs)(ser) + 4 * sa) * (K(CD_PI) / 100) / (a2 * M->st) *
                  scale;
    }
    *sabs = sa_tot;
    return tot;
}

/* t inside the Ter window, drift node at zero (cdfdif.c:179-197).
 * *sabs: (|sl| + |su| + sum |term|) under the same multiplier. */
static real cd_window_zero(const cd_model *M, const cd_run *R, real t, real zu, real zl, real lo,
                           int m, real *sabs)
{
    const int slot = CD_SLOT_ZERO + m;
    const real a = M->a, a2 = M->a2;
    real h[3] = {0, 0, 0};
    real sa = 0;
    const real su = -(zu * zu) / (12 * a2) + (zu * zu * zu) / (12 * a * a2) -
                    (zu * zu * zu * zu) / (48 * a2 * a2);
    const real sl = -(zl * zl) / (12 * a2) + (zl * zl * zl) / (12 * a * a2) -
                    (zl * zl * zl * zl) / (48 * a2 * a2);
    if (!R->forced) R->rec->stop[slot] = CD_VMAX;
    for (int v = 1; v < R->vcap; v++) {
        h[0] = h[1];
        h[1] = h[2];
        const real sifa = K(CD_PI) * v / a;
        const real den = (K(CD_PI) * v) * (K(CD_PI) * v) / (a2 * 100);
        const real term = 1 / (K(CD_PI) * K(CD_PI) * K(CD_PI) * K(CD_PI) * v * v * v * v) *
                          (RM(cos)(sifa * zl) - RM(cos)(sifa * zu)) *
                          RM(exp)(K(-.5) * den * (t - lo));
        h[2] = h[1] + term;
        sa += RM(fabs)(term);
        if (cd_series_ends(R, slot, v, h)) break;
    }
    *sabs = 400 * a2 * a * (RM(fabs)(sl) + RM(fabs)(su) + sa) / (M->st * M->sz);
    return 400 * a2 * a * (sl - su - h[2]) / (M->st * M->sz);
}

/* cdfdif(t, x, par, &prob) (cdfdif.c:59-221) under the run R; *S: the scale */
static real cd_eval(real t, int x, const double *par, const cd_run *R, real *prob, real *S)
{
    cd_model M;
    cd_setup(&M, par);
    const real zu = (1 - x) * M.z + x * (M.a - M.z) + M.sz / 2;
    const real zl = (1 - x) * M.z + x * (M.a - M.z) - M.sz / 2;
    const real lo = M.ter - M.st / 2;
    real F = 0;
    int branch;
    *prob = cd_prob(&M, R);
    *S = 0;
    if (R->forced) {
        branch = R->rec->branch;
    } else {
        branch = 0;
        if (t - M.ter + M.st / 2 > K(0.001)) branch = (t > M.ter + M.st / 2) ? 1 : 2;
        R->rec->branch = branch;
        for (int k = 0; k < CD_NSTOP; k++) R->rec->stop[k] = -1;
    }
    if (branch != 0) {
        /* min(t, Ter + st/2): beyond the window that is its edge, inside it t */
        const real up = branch == 1 ? M.ter + M.st / 2 : t;
        const real p1 = *prob * (up - lo) / M.st;
        const real p0 = (1 - *prob) * (up - lo) / M.st;
        real sa;
        *S = RM(fabs)(p0 * (1 - x)) + RM(fabs)(p1 * x);
        if (branch == 1) {
            const real s = cd_series_beyond(&M, R, t, x, zu, zl, up, lo, &sa);
            F = (p0 * (1 - x) + p1 * x) - s * 4 * K(CD_PI) / (M.a2 * M.sz * M.st);
            *S += sa * 4 * K(CD_PI) / (M.a2 * M.sz * M.st);
        } else {
            real acc = 0;
            for (int m = 0; m < 6; m++) {
                const real part = !cd_node_is_zero(&M, R, m)
                                      ? cd_window_node(&M, R, t, x, lo, m, &sa)
                                      : cd_window_zero(&M, R, t, zu, zl, lo, m, &sa);
                acc += part * M.wgh[m];
                *S += sa * M.wgh[m];
            }
            F = (p0 * (1 - x) + p1 * x) - acc;
        }
    }
    return F > K(1e-29) ? F : 0;
}

/* One trial of dmat_cdf_array's loop (cdfdif_wrapper.pyx:46-51): the fold
 * (1 - P) + sign(x) F and the outlier mix. *S_out: the scale carried through
 * both, every addend of the output in absolute value. */
static real cd_fold(double xi, real F, real pb, real S, double p_outlier, double w_outlier,
                    real *S_out)
{
    const real sg = xi > 0 ? 1.0 : (xi < 0 ? -1.0 : (xi == 0 ? 0.0 : xi));
    const real y = (1 - pb) + sg * F; /* np.sign: NaN stays NaN */
    const real mix = (K(xi) + (K(1.) / (2 * K(w_outlier)))) * K(w_outlier) * K(p_outlier);
    *S_out = (RM(fabs)(1 - pb) + S) * (1 - K(p_outlier)) + RM(fabs)(mix);
    return y * (1 - K(p_outlier)) + mix;
}

static int cd_support(double sv, double a, double z, double sz, double t, double st,
                      double p_outlier)
{
    return !((sv < 0) || (a <= 0) || (z < 0) || (z > 1) || (sz < 0) || (sz > 1) ||
             (z + sz / 2. > 1) || (z - sz / 2. < 0) || (t - st / 2. < 0) || (t < 0) || (st < 0) ||
             !((p_outlier >= 0) && (p_outlier <= 1)));
}

#ifndef CD_LONG

/* cdfdif(t, x, par, &prob) (cdfdif.c:59-221) */
double oracle_cdfdif(double t, int x, const double *par, double *prob)
{
    cd_record rec;
    const cd_run R = {CD_VMAX, 0, &rec};
    double S;
    return cd_eval(t, x, par, &R, prob, &S);
}

/* The same arithmetic with the series cap as a parameter (vcap = 5000: the
 * reference). Returns F; out: F's scale S, P(lower boundary) and the record
 * of the run (branch, stop[]). */
double oracle_cdfdif_probe(double t, int x, const double *par, int vcap, cd_probe *out)
{
    const cd_run R = {vcap, 0, &out->rec};
    return cd_eval(t, x, par, &R, &out->prob, &out->S);
}

/* The replay mode of the long double twin, here in double: sums the terms
 * io->rec lists with no test of its own, so a test can show that a replay
 * reproduces the run bit for bit. */
double oracle_cdfdif_replay(double t, int x, const double *par, int vcap, cd_probe *io)
{
    const cd_run R = {vcap, 1, &io->rec};
    return cd_eval(t, x, par, &R, &io->prob, &io->S);
}

/* dmat_cdf_array's loop (cdfdif_wrapper.pyx:35-53) after its argument checks;
 * returns 0, or -1 for parameters outside the support (the wrapper raises). */
int oracle_dmat_cdf_array(const double *x, int64_t n, double v, double sv, double a, double z,
                          double sz, double t, double st, double p_outlier, double w_outlier,
                          double *out)
{
    if (!cd_support(sv, a, z, sz, t, st, p_outlier)) return -1;
    const double epsi = 1e-10;
    const double par[7] = {a / 10., t, sv / 10. + epsi, z * (a / 10.), sz * (a / 10.) + epsi,
                           st + epsi, v / 10.};
    for (int64_t i = 0; i < n; i++) {
        double pb;
        const int bnd = x[i] > 0;
        double y = oracle_cdfdif(fabs(x[i]), bnd, par, &pb);
        const double sg = x[i] > 0 ? 1.0 : (x[i] < 0 ? -1.0 : (x[i] == 0 ? 0.0 : x[i]));
        y = (1 - pb) + sg * y; /* np.sign: NaN stays NaN */
        out[i] = y * (1 - p_outlier) + (x[i] + (1. / (2 * w_outlier))) * w_outlier * p_outlier;
    }
    return 0;
}

/* The same loop through the probe: out[n] the wrapper's outputs, F[n] cdfdif's
 * values, S[n] the scale of each output, rec[n] the records. */
int oracle_dmat_cdf_probe_array(const double *x, int64_t n, double v, double sv, double a,
                                double z, double sz, double t, double st, double p_outlier,
                                double w_outlier, int vcap, double *out, double *F, double *S,
                                cd_record *rec)
{
    if (!cd_support(sv, a, z, sz, t, st, p_outlier)) return -1;
    const double epsi = 1e-10;
    const double par[7] = {a / 10., t, sv / 10. + epsi, z * (a / 10.), sz * (a / 10.) + epsi,
                           st + epsi, v / 10.};
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t i = 0; i < n; i++) {
        cd_probe pr;
        F[i] = oracle_cdfdif_probe(fabs(x[i]), x[i] > 0, par, vcap, &pr);
        rec[i] = pr.rec;
        out[i] = cd_fold(x[i], F[i], pr.prob, pr.S, p_outlier, w_outlier, &S[i]);
    }
    return 0;
}

/* the same loop over n_threads OpenMP threads (the multi-core CPU baseline;
 * not the reference's build) */
int oracle_dmat_cdf_array_omp(const double *x, int64_t n, double v, double sv, double a,
                              double z, double sz, double t, double st, double p_outlier,
                              double w_outlier, double *out, int n_threads)
{
    int rc = 0, used = 1;
#pragma omp parallel num_threads(n_threads > 0 ? n_threads : 1)
    {
#pragma omp single
        {
#ifdef _OPENMP
            used = omp_get_num_threads();
#endif
        }
        const int64_t nt = used;
        int tid = 0;
#ifdef _OPENMP
        tid = omp_get_thread_num();
#endif
        const int64_t lo = n * tid / nt, hi = n * (tid + 1) / nt;
        if (oracle_dmat_cdf_array(x + lo, hi - lo, v, sv, a, z, sz, t, st, p_outlier, w_outlier,
                                  out + lo) != 0)
            rc = -1;
    }
    return rc < 0 ? -1 : used;
}

#else /* CD_LONG */

/* dmat_cdf_array's loop in long double over the terms the double run summed
 * (rec[n] from oracle_dmat_cdf_probe_array at the same vcap). The wrapper's
 * parameter transform stays in double: its results are cdfdif's inputs. */
int oracle_dmat_cdf_array_ld(const double *x, int64_t n, double v, double sv, double a, double z,
                             double sz, double t, double st, double p_outlier, double w_outlier,
                             int vcap, const cd_record *rec, long double *out)
{
    if (!cd_support(sv, a, z, sz, t, st, p_outlier)) return -1;
    const double epsi = 1e-10;
    const double par[7] = {a / 10., t, sv / 10. + epsi, z * (a / 10.), sz * (a / 10.) + epsi,
                           st + epsi, v / 10.};
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t i = 0; i < n; i++) {
        real pb, s, s_out;
        const cd_run R = {vcap, 1, (cd_record *)&rec[i]};
        const real F = cd_eval(RM(fabs)(K(x[i])), x[i] > 0, par, &R, &pb, &s);
        out[i] = cd_fold(x[i], F, pb, s, p_outlier, w_outlier, &s_out);
    }
    return 0;
}

#endif
