/*
 * wfpt_amd — MI355X (gfx950) Wiener first-passage-time likelihood engine.
 *
 * C ABI that replaces the reference's `wfpt` Cython extension module on its
 * hot path. Plain pointers and sizes only; device memory, streams and RCCL
 * communicators live behind opaque handles. Every entry point returns a
 * status (WFPT_OK == 0); a non-zero status is a device / argument error and is
 * never folded into a numeric result. Numeric failure keeps the reference's
 * conventions exactly: -inf for an impossible likelihood, 0 for an invalid
 * parameter set per trial, NaN where the reference yields NaN (a == 0).
 *
 * Reference interfaces replaced (file:line under the reference tree):
 *   wfpt_wiener_like*      <- wfpt.wiener_like         src/wfpt.pyx:54-76
 *   wfpt_pdf_array         <- wfpt.pdf_array           src/wfpt.pyx:32-48
 *   wfpt_full_pdf          <- wfpt.full_pdf (cpdef)    src/pdf.pxi:104-146
 *   wfpt_wiener_like_nodes <- one wfpt_like per PyMC node, batched
 *   wfpt_wiener_like_nodes_multi <- the same for several parameter tables (chains)
 *                             hddm/likelihoods.py:52-73 via base.py:754-757
 *   wfpt_wiener_like_multi <- wfpt.wiener_like_multi   src/wfpt.pyx:244-274
 *   wfpt_wiener_like_rl_reg_groups <- HDDMrlRegressor's wienerRL_multi_like per subject,
 *                             batched  hddm/models/hddm_rl_regression.py:25-38
 *   wfpt_dmat_cdf_array    <- cdfdif_wrapper.dmat_cdf_array
 *                             src/cdfdif_wrapper.pyx:16-53, src/cdfdif.c:59-221
 *   wfpt_gen_rts_nodes     <- wfpt.gen_rts_from_cdf, one call for many rows
 *                             src/wfpt.pyx:323-354
 *   wfpt_gen_rts_drift_nodes <- generate._gen_rts_from_simulated_drift, many rows
 *                             hddm/generate.py:208-319
 *   wfpt_gen_rlddm_rows    <- generate.gen_rand_rlddm_data, many sequences in closed loop
 *   wfpt_rt_stats_rows     <- utils.gen_ppc_stats applied to many rows of RTs
 *                             hddm/utils.py:241-265
 * The Python binding that keeps the reference signatures is
 * hddm_amd/wfpt.py (ctypes); INTEGRATION.md shows the drop-in.
 */
#ifndef WFPT_AMD_H
#define WFPT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFPT_OK 0
#define WFPT_ERR_HIP 1         /* HIP runtime / kernel failure */
#define WFPT_ERR_ARG 2         /* bad argument (null pointer, size, depth) */
#define WFPT_ERR_COMM 3        /* RCCL failure */
#define WFPT_ERR_UNSUPPORTED 4 /* e.g. n_st/n_sz beyond WFPT_MAX_DEPTH */

/* Maximum adaptive-Simpson recursion depth (n_st, n_sz) supported on device.
 * The reference recurses without bound; 2^24 leaves per trial is far past any
 * practical use (HDDM passes 2, wiener_like's default is 10). */
#define WFPT_MAX_DEPTH 24
/* Per-trial cap on pdf_sv evaluations (2^24). The heaviest call in the
 * reference's own tests needs 1.2e5 (wiener_like defaults n=10,
 * simps_err=1e-8). Exceeding either limit fails the call with
 * WFPT_ERR_UNSUPPORTED; no value is returned. */
#define WFPT_EVAL_BUDGET (1ll << 24)

typedef struct wfpt_ctx wfpt_ctx;
typedef struct wfpt_ds wfpt_ds;

/* DDM parameters of one likelihood call (src/wfpt.pyx:54: v sv a z sz t st
 * p_outlier). */
typedef struct wfpt_params {
    double v, sv, a, z, sz, t, st, p_outlier;
} wfpt_params;

/* Numerical knobs (src/wfpt.pyx:55-56). All explicit: the reference's own
 * defaults differ between wiener_like and pdf_array. */
typedef struct wfpt_knobs {
    double err;           /* series truncation error (pdf.pxi:36-47) */
    int32_t n_st;         /* max recursion depth over st */
    int32_t n_sz;         /* max recursion depth over sz */
    int32_t use_adaptive; /* 0 => fixed Simpson with n_st/n_sz panels */
    double simps_err;     /* adaptive Simpson tolerance */
    double w_outlier;     /* outlier density */
} wfpt_knobs;

/* ---- context ---------------------------------------------------------- */
int wfpt_device_count(int *n);
int wfpt_open(int device, wfpt_ctx **out);
void wfpt_close(wfpt_ctx *ctx);
/* message of the last failing call on this thread ("" if none) */
const char *wfpt_last_error(void);

/* ---- resident datasets ------------------------------------------------- */
/* Uploads rt[n] (signed RTs, sign = boundary, hddm/utils.py:15-37) once.
 * node_id (nullable) assigns each trial to one of n_nodes likelihood nodes
 * (hierarchical models); trials are regrouped by node and, inside a node,
 * ordered by |rt| so one wavefront sees one series branch.
 * The caller's arrays are not retained. */
int wfpt_dataset_create(wfpt_ctx *ctx, const double *rt, int64_t n, const int32_t *node_id,
                        int32_t n_nodes, wfpt_ds **out);
/* As wfpt_dataset_create; flags: WFPT_DS_INPUT_ORDER keeps the trials in the
 * caller's order (no |rt| ordering), as wfpt_wiener_like_multi_resident's
 * per-trial parameter arrays require. */
#define WFPT_DS_INPUT_ORDER 1
int wfpt_dataset_create_ex(wfpt_ctx *ctx, const double *rt, int64_t n, const int32_t *node_id,
                           int32_t n_nodes, int flags, wfpt_ds **out);
void wfpt_dataset_destroy(wfpt_ds *ds);
int64_t wfpt_dataset_size(const wfpt_ds *ds);
/* The i-th rank's contiguous shard [lo, hi) of n trials (multi-GPU). */
void wfpt_shard_range(int64_t n, int nranks, int rank, int64_t *lo, int64_t *hi);

/* ---- likelihoods -------------------------------------------------------- */
/* Sum of log mixture densities over a resident dataset (wfpt.pyx:54-76). */
int wfpt_wiener_like(wfpt_ctx *ctx, const wfpt_ds *ds, const wfpt_params *p,
                     const wfpt_knobs *k, double *out_logp);
/* wfpt_wiener_like with each trial's addend of the sum too (the
 * `log(p * (1 - p_outlier) + wp_outlier)` terms of wfpt.pyx:66-74; -inf for a
 * zero mixture density) in out_trial[n], in the caller's trial order. It takes
 * the same predicted call sequence (lean level-0 pass, one-launch small path,
 * engine, redo, fold) as wfpt_wiener_like would, with the same kernels built
 * with one extra store per trial, and leaves the same chunk partials: the
 * per-trial check of the summing path (tests), not a hot-path call. */
int wfpt_wiener_like_trials(wfpt_ctx *ctx, const wfpt_ds *ds, const wfpt_params *p,
                            const wfpt_knobs *k, double *out_logp, double *out_trial);
/* perm[i] = the caller's index of the dataset's stored trial i (datasets are
 * stored grouped by node / boundary and ordered by |rt|; identity for
 * WFPT_DS_INPUT_ORDER). An identity order is answered from the host, also after
 * the dataset's context was closed; a stored permutation lives in device memory
 * and needs the context (WFPT_ERR_ARG once it is closed). The copy is serialised
 * with the context's calls. */
int wfpt_dataset_order(const wfpt_ds *ds, int64_t *perm);
/* Same on a host array (uploaded for this call). */
int wfpt_wiener_like_host(wfpt_ctx *ctx, const double *x, int64_t n, const wfpt_params *p,
                          const wfpt_knobs *k, double *out_logp);
/* Per-node sums for a dataset created with node ids: params[n_nodes] in,
 * out_logp[n_nodes] out (each = wiener_like of that node's trials). */
int wfpt_wiener_like_nodes(wfpt_ctx *ctx, const wfpt_ds *ds, const wfpt_params *per_node,
                           const wfpt_knobs *k, double *out_logp);
/* As wfpt_wiener_like_nodes; out_trial (nullable, ds size) also receives
 * each trial's log term, in the order the caller passed the trials to
 * wfpt_dataset_create: log of the node's mixture p (1 - p_outlier) +
 * w_outlier p_outlier, -inf for a zero mixture density or a p_outlier outside
 * [0, 1] (wfpt.pyx:63-72 per node). */
int wfpt_wiener_like_nodes_ex(wfpt_ctx *ctx, const wfpt_ds *ds, const wfpt_params *per_node,
                              const wfpt_knobs *k, double *out_logp, double *out_trial);
/* n_tables parameter tables over the same resident node dataset in ONE
 * launch: tables[t * n_nodes + j] is node j's row in table t, out_logp[t *
 * n_nodes + j] its sum. Replaces n_tables separate wfpt_like evaluations of
 * every node (hddm/likelihoods.py:52-73, reached once per node per slice
 * evaluation by the reference's samplers): several MCMC chains in lockstep
 * (HDDM's multi-chain usage, docs/source/howto.rst:267-291) or both probes of
 * a slice step's stepping-out. Table t's sums are bit for bit those of
 * wfpt_wiener_like_nodes on table t alone. out_trial (nullable, n_tables x
 * ds size): table t's per-trial terms at out_trial[t * n + i], caller order. */
int wfpt_wiener_like_nodes_multi(wfpt_ctx *ctx, const wfpt_ds *ds, const wfpt_params *tables,
                                 int32_t n_tables, const wfpt_knobs *k, double *out_logp);
int wfpt_wiener_like_nodes_multi_ex(wfpt_ctx *ctx, const wfpt_ds *ds, const wfpt_params *tables,
                                    int32_t n_tables, const wfpt_knobs *k, double *out_logp,
                                    double *out_trial);
/* Per-trial mixture density, or its log if logp != 0 (wfpt.pyx:32-48). */
int wfpt_pdf_array(wfpt_ctx *ctx, const double *x, int64_t n, const wfpt_params *p,
                   const wfpt_knobs *k, int logp, double *out);
/* Single full_pdf (no mixture) (pdf.pxi:104-146). */
int wfpt_full_pdf(wfpt_ctx *ctx, double x, const wfpt_params *p, const wfpt_knobs *k,
                  double *out);
/* Per-trial parameters (wfpt.pyx:244-274). arrays[j] (j = v,sv,a,z,sz,t,st)
 * is a host array of n values or NULL to use scalars[j]. |x| == 999 marks a
 * missing response scored by prob_ub (pdf.pxi:67-72). */
int wfpt_wiener_like_multi(wfpt_ctx *ctx, const double *x, int64_t n,
                           const double *const arrays[7], const double scalars[7],
                           const wfpt_knobs *k, double p_outlier, double *out_logp);
/* As wfpt_wiener_like_multi; out_trial (nullable, n values) also receives
 * each trial's term of the sum (wfpt.pyx:261-272), in trial order. */
int wfpt_wiener_like_multi_ex(wfpt_ctx *ctx, const double *x, int64_t n,
                              const double *const arrays[7], const double scalars[7],
                              const wfpt_knobs *k, double p_outlier, double *out_logp,
                              double *out_trial);
/* Same over a resident dataset created with WFPT_DS_INPUT_ORDER (the RTs of a
 * regression model stay fixed across MCMC; only the per-trial parameter
 * arrays, hddm_regression.py:26-36, go up per call). */
int wfpt_wiener_like_multi_resident(wfpt_ctx *ctx, const wfpt_ds *ds,
                                    const double *const arrays[7], const double scalars[7],
                                    const wfpt_knobs *k, double p_outlier, double *out_logp);
int wfpt_wiener_like_multi_resident_ex(wfpt_ctx *ctx, const wfpt_ds *ds,
                                       const double *const arrays[7], const double scalars[7],
                                       const wfpt_knobs *k, double p_outlier, double *out_logp,
                                       double *out_trial);

/* ---- reinforcement-learning likelihoods (Q-learning drift) --------------- */
/* The reference's RL family: a Q-value pair per condition, updated trial by
 * trial from the feedback, sets each trial's drift (qs[1] - qs[0]) * v.
 *   wfpt_wiener_like_rlddm*       <- wfpt.wiener_like_rlddm       src/wfpt.pyx:79-154
 *   wfpt_wiener_like_rl*          <- wfpt.wiener_like_rl          src/wfpt.pyx:157-241
 *   wfpt_wiener_like_multi_rlddm* <- wfpt.wiener_like_multi_rlddm src/wfpt.pyx:277-320
 *   wfpt_wiener_like_rlddm_nodes* <- one wiener_like_rlddm per node, batched
 *   wfpt_wiener_like_rlddm_nodes_multi* <- ... for several row tables at once
 * The recurrence runs on the device bit for bit as the reference computes it
 * (learning rates pow(2.718281828459, alpha) / (1 + pow(2.718281828459,
 * alpha)) from the host's libm; q + alfa * (f - q) in three roundings; strict
 * feedback > q), so every drift equals the reference's exactly. The densities
 * come from the per-trial-parameter pass of wfpt_wiener_like_multi with the
 * drifts in its v slot.
 * Divergence from the reference: |rt| == 999 is rejected (WFPT_ERR_ARG). The
 * per-trial-parameter pass scores +-999 as a missing response by prob_ub
 * (wfpt.pyx:267-270); the reference's RL functions pass it to full_pdf like
 * any other RT. */
typedef struct wfpt_rl_ds wfpt_rl_ds;
/* Uploads the fixed inputs of the RL likelihoods once (wfpt.pyx:79-82: x,
 * response, feedback, split_by). rt is nullable (choice-only model,
 * wfpt_wiener_like_rl); response[n] must be 0 or 1 (the reference indexes qs
 * with it unchecked); node_id (nullable) / n_nodes as in wfpt_dataset_create.
 * Trials are grouped into one segment per (node, condition), conditions in
 * rising split_by order (np.unique, wfpt.pyx:100), the caller's order kept
 * inside a condition (the masks of wfpt.pyx:114-116). WFPT_ERR_ARG: a response
 * outside {0, 1}, n < 0, a null array with n > 0, |rt| == 999, a node id out
 * of range. The caller's arrays are not retained. */
int wfpt_rl_dataset_create(wfpt_ctx *ctx, const double *rt, const int64_t *response,
                           const double *feedback, const int64_t *split_by, int64_t n,
                           const int32_t *node_id, int32_t n_nodes, wfpt_rl_ds **out);
void wfpt_rl_dataset_destroy(wfpt_rl_ds *ds);
/* wiener_like_rlddm (wfpt.pyx:79-154) over a resident RL dataset; p->v is the
 * drift scaling. pos_alpha == 100.0 means "use alpha" (wfpt.pyx:105-108).
 * -inf for a p_outlier outside [0, 1] (wfpt.pyx:102-103; the _ex outputs are
 * then left untouched) or a scored trial of zero mixture density (:138-139).
 * The first trial of every condition only updates q (:121-130). */
int wfpt_wiener_like_rlddm(wfpt_ctx *ctx, const wfpt_rl_ds *ds, double q, double alpha,
                           double pos_alpha, const wfpt_params *p, const wfpt_knobs *k,
                           double *out_logp);
/* The _ex siblings of the RL entries: out_trial (nullable, n values, the
 * caller's order) receives each trial's log term, 0.0 for an unscored first
 * trial; out_drift (nullable, n values) the drift the recurrence holds when it
 * reaches the trial, for every trial. */
int wfpt_wiener_like_rlddm_ex(wfpt_ctx *ctx, const wfpt_rl_ds *ds, double q, double alpha,
                              double pos_alpha, const wfpt_params *p, const wfpt_knobs *k,
                              double *out_logp, double *out_trial, double *out_drift);
/* wiener_like_rl (wfpt.pyx:157-241): the choice probability alone. As the
 * reference does, it applies p_outlier and w_outlier, no a, and ignores err,
 * n_st, n_sz, use_adaptive and simps_err (not taken here). */
int wfpt_wiener_like_rl(wfpt_ctx *ctx, const wfpt_rl_ds *ds, double q, double alpha,
                        double pos_alpha, double v, double z, double p_outlier,
                        double w_outlier, double *out_logp);
int wfpt_wiener_like_rl_ex(wfpt_ctx *ctx, const wfpt_rl_ds *ds, double q, double alpha,
                           double pos_alpha, double v, double z, double p_outlier,
                           double w_outlier, double *out_logp, double *out_trial,
                           double *out_drift);
/* wiener_like_multi_rlddm (wfpt.pyx:277-320) on host arrays (uploaded for this
 * call). arrays[j] (j = v, sv, a, z, sz, t, st, alpha) is a host array of n
 * values or NULL to use scalars[j]. Its semantics differ from
 * wiener_like_rlddm's, as in the reference: the Q pair resets where split_by[i]
 * != split_by[i - 1] (an adjacent change, not a grouping), every trial is
 * scored (the first at drift 0), there is one learning rate, no p_outlier
 * range check and no early -inf (log(0) enters the sum). */
int wfpt_wiener_like_multi_rlddm(wfpt_ctx *ctx, const double *x, const int64_t *response,
                                 const double *feedback, const int64_t *split_by, int64_t n,
                                 double q, const double *const arrays[8],
                                 const double scalars[8], const wfpt_knobs *k, double p_outlier,
                                 double *out_logp);
int wfpt_wiener_like_multi_rlddm_ex(wfpt_ctx *ctx, const double *x, const int64_t *response,
                                    const double *feedback, const int64_t *split_by, int64_t n,
                                    double q, const double *const arrays[8],
                                    const double scalars[8], const wfpt_knobs *k,
                                    double p_outlier, double *out_logp, double *out_trial,
                                    double *out_drift);
/* One wiener_like_rlddm per node of a dataset created with node ids, in one
 * scan launch and one scoring pass: rl_rows[3 j ..] = node j's (q, alpha,
 * pos_alpha), per_node[j] its DDM row, out_logp[n_nodes]. Node j's sum is bit
 * for bit wfpt_wiener_like_rlddm on that node's trials with that node's row.
 * sz and st stay scalars of the scoring pass: one launch when all nodes share
 * them (HDDM's default: group-only parameters), else one per run of
 * consecutive nodes that do. The nodes must share p_outlier, and a node may
 * hold at most 2^22 scored trials (WFPT_ERR_UNSUPPORTED otherwise). */
int wfpt_wiener_like_rlddm_nodes(wfpt_ctx *ctx, const wfpt_rl_ds *ds, const double *rl_rows,
                                 const wfpt_params *per_node, const wfpt_knobs *k,
                                 double *out_logp);
int wfpt_wiener_like_rlddm_nodes_ex(wfpt_ctx *ctx, const wfpt_rl_ds *ds, const double *rl_rows,
                                    const wfpt_params *per_node, const wfpt_knobs *k,
                                    double *out_logp, double *out_trial, double *out_drift);
/* n_tables evaluations of wienerRL_like per node (hddm/models/hddm_rl.py:61-73)
 * in one call: the node batch above over n_tables row tables, e.g. both
 * stepping-out probes of a slice step. rl_tables[3 (t n_nodes + j) ..] = (q,
 * alpha, pos_alpha) of node j in table t, tables[t n_nodes + j] its DDM row,
 * out_logp[t n_nodes + j] its sum. out_trial / out_drift (nullable): n_tables
 * x n values, table t's at [t n + i] in the caller's order. Row t of every
 * output is bit for bit what wfpt_wiener_like_rlddm_nodes_ex returns for
 * table t alone. When every row of every table shares sz and st the call makes
 * the one-table call's launches, each over n_tables times the work (one scan
 * over n_tables x segments lanes, one fill, one scoring pass, one per-node
 * sum, one finalize, one wait); otherwise the scoring pass splits into runs of
 * consecutive (table, node) rows that share them. WFPT_ERR_ARG: a null
 * pointer, n_tables < 1, a dataset without node ids. WFPT_ERR_UNSUPPORTED: a
 * p_outlier that differs anywhere across rows or tables, a node of more than
 * 2^22 scored trials, n_tables x segments (or scored trials) beyond 2^31 - 1.
 * A p_outlier outside [0, 1] sets every sum to -inf. */
int wfpt_wiener_like_rlddm_nodes_multi(wfpt_ctx *ctx, const wfpt_rl_ds *ds,
                                       const double *rl_tables, const wfpt_params *tables,
                                       int32_t n_tables, const wfpt_knobs *k, double *out_logp);
int wfpt_wiener_like_rlddm_nodes_multi_ex(wfpt_ctx *ctx, const wfpt_rl_ds *ds,
                                          const double *rl_tables, const wfpt_params *tables,
                                          int32_t n_tables, const wfpt_knobs *k, double *out_logp,
                                          double *out_trial, double *out_drift);

/* ---- regression likelihoods (HDDMRegressor) ------------------------------ */
/* The reference's regression node (hddm/models/hddm_regression.py:26-36,
 * wiener_multi_like) computes each regressed parameter per trial on the host
 * as link(design matrix . coefficients) and passes the arrays to
 * wfpt.wiener_like_multi (src/wfpt.pyx:244-274). Here the design matrix is
 * resident and the predictor runs on the device (reg_fill_kernel); only the
 * coefficients go up per call.
 *   wfpt_wiener_like_reg*        <- wiener_multi_like  hddm_regression.py:26-36
 *                                   + wiener_like_multi src/wfpt.pyx:244-274
 *   wfpt_wiener_like_reg_groups* <- one such node per subject, batched
 * Order contract: a term's linear predictor is
 *   eta = X[i, col0] * b[col0]; eta = eta + X[i, col0 + 1] * b[col0 + 1]; ...
 * left to right, every product and every sum rounded separately (no fused
 * multiply-add). Link contract: IDENTITY eta; EXP the correctly rounded
 * exponential of eta; INVLOGIT 1 / (1 + exp(-eta)) with that exponential, the
 * sum and the quotient each rounded once.
 * Semantics are wiener_like_multi's: no p_outlier range check, |rt| == 999 is
 * a missing response scored by prob_ub (wfpt.pyx:261-270), a zero mixture
 * density contributes -inf. */
#define WFPT_LINK_IDENTITY 0
#define WFPT_LINK_EXP 1
#define WFPT_LINK_INVLOGIT 2
typedef struct {
  int32_t param, link, col0, ncol; /* param 0..6 = v, sv, a, z, sz, t, st; 7 = alpha in
                                      the wfpt_wiener_like_rl_reg_groups* entries only */
} wfpt_reg_term;
typedef struct wfpt_reg_ds wfpt_reg_ds;
/* Uploads n signed RTs and the row-major (n, C) design matrix X once (the
 * `data` and design matrices hddm_regression.py:84-101 keeps per node).
 * group_id (nullable, n_groups): trials are stored group-major, the caller's
 * order kept inside a group; without it there is one group in the caller's
 * order. WFPT_ERR_ARG: n < 0, C < 1, a null array with n > 0, a group id out
 * of range. The caller's arrays are not retained. */
int wfpt_reg_dataset_create(wfpt_ctx *ctx, const double *rt, int64_t n, const double *X,
                            int32_t C, const int32_t *group_id, int32_t n_groups,
                            wfpt_reg_ds **out);
void wfpt_reg_dataset_destroy(wfpt_reg_ds *ds);
/* The reference's wfpt_reg node (hddm_regression.py:26-36, 103-113): one
 * coefficient vector coef[C], one parameter row; out_logp = the sum over all
 * trials. A regressed parameter's field of p is ignored; the others are the
 * scalars of the per-trial-parameter pass, so the result is bit for bit
 * wfpt_wiener_like_multi_resident given the predicted arrays.
 * WFPT_ERR_ARG, before any device work: null pointers, more than 7 terms, a
 * term parameter outside 0..6, a parameter named twice, an unknown link,
 * ncol < 1, a column range outside [0, C), a data set of another context. */
int wfpt_wiener_like_reg(wfpt_ctx *ctx, const wfpt_reg_ds *ds, const wfpt_reg_term *terms,
                         int32_t n_terms, const double *coef, const wfpt_params *p,
                         const wfpt_knobs *k, double *out_logp);
/* out_trial (nullable, n): each trial's log term; out_pred (nullable,
 * n_terms * n): term k's predicted parameter of trial i at [k * n + i]. Both
 * in the caller's order. */
int wfpt_wiener_like_reg_ex(wfpt_ctx *ctx, const wfpt_reg_ds *ds, const wfpt_reg_term *terms,
                            int32_t n_terms, const double *coef, const wfpt_params *p,
                            const wfpt_knobs *k, double *out_logp, double *out_trial,
                            double *out_pred);
/* One regression node per group (subject) in one fill launch and one scoring
 * pass (the per-subject nodes hddm_regression.py:214-236 builds when
 * group_only_regressors is False, and what a block update over subjects
 * needs): coef[n_groups * C] one coefficient row per group, per_group[n_groups]
 * its parameter row, out_logp[n_groups]. Group g's sum is bit for bit
 * wfpt_wiener_like_reg on that group's trials alone with row g; a group
 * without trials sums to 0.0. sz and st stay scalars of the pass unless
 * regressed: one scoring launch per run of consecutive groups that share them.
 * The groups must share p_outlier and a group may hold at most 2^22 trials
 * (WFPT_ERR_UNSUPPORTED otherwise). */
int wfpt_wiener_like_reg_groups(wfpt_ctx *ctx, const wfpt_reg_ds *ds, const wfpt_reg_term *terms,
                                int32_t n_terms, const double *coef,
                                const wfpt_params *per_group, const wfpt_knobs *k,
                                double *out_logp);
int wfpt_wiener_like_reg_groups_ex(wfpt_ctx *ctx, const wfpt_reg_ds *ds,
                                   const wfpt_reg_term *terms, int32_t n_terms,
                                   const double *coef, const wfpt_params *per_group,
                                   const wfpt_knobs *k, double *out_logp, double *out_trial,
                                   double *out_pred);

/* ---- RL regression likelihood (hddm/models/hddm_rl_regression.py) ---------
 * HDDMrlRegressor's node (hddm_rl_regression.py:25-38) forms trial-wise
 * parameters, the learning rate's alpha among them, as link(design matrix .
 * coefficients) and passes them to wfpt.wiener_like_multi_rlddm
 * (src/wfpt.pyx:277-320), once per subject node with a fresh Q pair. Here the
 * design matrix, responses, feedback and segment layout are resident and only
 * a coefficient table and a few rows per group go up per call.
 *   wfpt_wiener_like_rl_reg_groups* <- one such node per subject, batched
 * Uploads n signed RTs, responses (0 / 1), feedback, conditions and the
 * row-major (n, C) design matrix once. Trials are stored group-major, the
 * caller's order kept inside a group (wfpt_reg_dataset_create). A segment (one
 * Q recurrence) is a maximal run of equal adjacent split_by inside a group; a
 * group boundary always starts a segment; every trial is scored, a segment's
 * first at drift 0 (wiener_like_multi_rlddm's segments). WFPT_ERR_ARG: n < 0,
 * C < 1, a null array with n > 0, a response outside {0, 1}, |rt| == 999, a
 * group id out of range. The caller's arrays are not retained. */
typedef struct wfpt_rl_reg_ds wfpt_rl_reg_ds;
int wfpt_rl_reg_dataset_create(wfpt_ctx *ctx, const double *rt, const int64_t *response,
                               const double *feedback, const int64_t *split_by, int64_t n,
                               const double *X, int32_t C, const int32_t *group_id,
                               int32_t n_groups, wfpt_rl_reg_ds **out);
void wfpt_rl_reg_dataset_destroy(wfpt_rl_reg_ds *ds);
/* One RL regression node per group: coef[n_groups * C], q[n_groups] the start
 * of both Q values, alpha[n_groups] the unbounded learning-rate parameter,
 * per_group[n_groups], out_logp[n_groups]. In these entries only,
 * wfpt_reg_term.param may also be 7 = alpha (at most 8 terms). alpha[g] is
 * ignored when alpha is regressed; per_group[g].v is the drift scaling unless v
 * is regressed. Three launches, in this order: a trial-parallel fill (the
 * terms by the order and link contract above, the non-regressed fields from
 * the group rows); the Q recurrence, one lane per segment, which writes each
 * trial's drift (q_up - q_low) * v into the scoring pass's v slot; the scoring
 * pass and per-group sums of wfpt_wiener_like_reg_groups, whose p_outlier, sz /
 * st and 2^22-trials-per-group rules apply. A group's sum does not depend on
 * the other groups of the call; a group without trials sums to 0.0.
 * Learning-rate contract: rate = e / (1 + e), e = 2.718281828459**alpha (the
 * double nearest that literal), the sum and the quotient each rounded once. A
 * non-regressed alpha[g] is squashed on the host with libm's pow, bit for bit
 * what wfpt_wiener_like_multi_rlddm does with a scalar alpha. A regressed
 * alpha is squashed on the device, per trial, with the power correctly
 * rounded: it differs from the reference's libm value by one ulp of the power
 * where libm misrounds (DESIGN.md §25 has the measured share).
 * _ex outputs (each nullable, the caller's order): out_trial[n] each trial's
 * log term; out_pred[n_terms * n] term k's prediction of trial i at [k * n +
 * i], the alpha term's after the link and before squashing; out_drift[n];
 * out_rate[n] each trial's learning rate.
 * WFPT_ERR_ARG, before any device work: null pointers and the term-list
 * errors of wfpt_wiener_like_reg with parameters 0..7. */
int wfpt_wiener_like_rl_reg_groups(wfpt_ctx *ctx, const wfpt_rl_reg_ds *ds,
                                   const wfpt_reg_term *terms, int32_t n_terms,
                                   const double *coef, const double *q, const double *alpha,
                                   const wfpt_params *per_group, const wfpt_knobs *k,
                                   double *out_logp);
int wfpt_wiener_like_rl_reg_groups_ex(wfpt_ctx *ctx, const wfpt_rl_reg_ds *ds,
                                      const wfpt_reg_term *terms, int32_t n_terms,
                                      const double *coef, const double *q, const double *alpha,
                                      const wfpt_params *per_group, const wfpt_knobs *k,
                                      double *out_logp, double *out_trial, double *out_pred,
                                      double *out_drift, double *out_rate);

/* The regressor's posterior predictive: one simulated RT per (sweep, trial),
 * each at the trial's own regressed parameters (wfpt_reg_like's random(),
 * hddm_regression.py:39-56, which calls gen_rts(size=1, method='drift') per
 * trial; the walk is _gen_rts_from_simulated_drift, generate.py:208-319, as in
 * wfpt_gen_rts_drift_nodes, without the in-trial switch).
 *   coef    S * n_groups * C: sweep s's coefficient row of group g at
 *           (s * n_groups + g) * C
 *   params  S * n_groups rows: the non-regressed fields of a trial come from
 *           row s * n_groups + its group (a regressed field and p_outlier are
 *           ignored)
 *   out     S * n signed RTs in the caller's order: out[s * n + i] is trial i
 * A trial's parameters are formed on the device when a lane picks the (sweep,
 * trial) up, by the order and link contract above: bit for bit what
 * wfpt_wiener_like_reg_groups_ex returns in out_pred for sweep s's rows.
 * Random numbers: wfpt_gen_rts_drift_nodes' streams at counter {s lo, s hi, i,
 * stream}: out[s * n + i] is bit for bit draw s of row i of a
 * wfpt_gen_rts_drift_nodes table that holds the trials' parameters in the
 * caller's order. It depends on (seed, s, i) and the parameters only, not on
 * the grouping, the stored order, wave_draws or workspace_bytes.
 * A trial whose formed parameters cannot be walked (one is not finite, a <= 0,
 * z - sz / 2 < 0 or z + sz / 2 > 1: only the device sees them) is NaN and
 * counted in *n_invalid; a walk that has not crossed after max_steps steps is
 * NaN and counted in *n_unfinished.
 * WFPT_ERR_ARG before any device work: null pointers, S < 1, dt <= 0,
 * intra_sv <= 0, max_steps outside [1, 2^31], the term-list errors of
 * wfpt_wiener_like_reg, a data set of another context or of 2^31 trials or
 * more. */
int wfpt_gen_rts_reg_drift(wfpt_ctx *ctx, const wfpt_reg_ds *ds, const wfpt_reg_term *terms,
                           int32_t n_terms, const double *coef, const wfpt_params *params,
                           int64_t S, double dt, double intra_sv, int64_t max_steps,
                           uint64_t seed, double *out, int64_t *n_unfinished,
                           int64_t *n_invalid);
/* As wfpt_gen_rts_reg_drift (hddm_regression.py:39-56, generate.py:208-319),
 * for tests and measurements. wave_draws: (sweep, trial) elements handed to one
 * wave, a multiple of 64 (0: the library's choice). workspace_bytes: device
 * bytes for the draws (0: 1 GiB); more sweeps than fit run in tiles. Neither
 * changes a value. Per (sweep, trial) in the caller's order, each nullable:
 * out_params [S * n * 7] the formed v, sv, a, z, sz, t, st; out_y0, out_delay,
 * out_drift (NaN for an invalid trial); out_n_steps (0 for an invalid trial).
 * out_wave_steps [ceil(S * n / wave_draws)]: needs wave_draws > 0 and a
 * workspace that holds every sweep. */
int wfpt_gen_rts_reg_drift_ex(wfpt_ctx *ctx, const wfpt_reg_ds *ds, const wfpt_reg_term *terms,
                              int32_t n_terms, const double *coef, const wfpt_params *params,
                              int64_t S, double dt, double intra_sv, int64_t max_steps,
                              uint64_t seed, int32_t wave_draws, int64_t workspace_bytes,
                              double *out, int64_t *n_unfinished, int64_t *n_invalid,
                              double *out_params, double *out_y0, double *out_delay,
                              double *out_drift, int64_t *out_n_steps, int64_t *out_wave_steps);
/* wfpt_gen_rts_reg_drift (hddm_regression.py:39-56, generate.py:208-319)
 * followed by the statistics of its draws (utils.py:241-265) while they are
 * still in device memory: row (s, g) holds sweep s's draws of group g's trials,
 * stats_out [S * n_groups * (8 + 2 nq)] is what wfpt_rt_stats_rows gives for
 * them. out may be NULL: no draw is copied to the host; both NaN counts are
 * returned either way. A NaN counts in its row's n and in neither boundary. */
int wfpt_gen_rts_reg_drift_stats(wfpt_ctx *ctx, const wfpt_reg_ds *ds,
                                 const wfpt_reg_term *terms, int32_t n_terms, const double *coef,
                                 const wfpt_params *params, int64_t S, double dt, double intra_sv,
                                 int64_t max_steps, uint64_t seed, int64_t workspace_bytes,
                                 double *out, int64_t *n_unfinished, int64_t *n_invalid,
                                 const double *q, int32_t nq, double *stats_out);

/* ---- model comparison: pointwise log-likelihood statistics ---------------- */
/* DIC and WAIC need, for S kept posterior sweeps, the per-sweep node sums and,
 * per trial, a reduction over the sweeps of that trial's log term l_s. The
 * S x n matrix of terms never leaves the device: the sweeps are scored in
 * tiles of T = max(1, max_workspace / (8 len)) sweeps (max_workspace <= 0: 1
 * GiB; T x nodes <= INT32_MAX / 2) by the family's existing batch call, and
 * after each tile one kernel folds its terms into a per-trial state, one lane
 * per trial, the sweeps in rising order (pointwise_update.hpp states the rule):
 *   l == -inf:  n_inf += 1                        nothing else changes
 *   else k += 1
 *     k == 1:   m = l; r = 1
 *     l <= m:   r = r + exp(l - m)
 *     else:     r = r * exp(m - l) + 1; m = l
 *     d = l - mean; mean = mean + d / k; M2 = M2 + d * (l - mean)
 *   finish:     lppd = m + log(r) - log(S)        S counts the -inf sweeps too
 *               p_waic = k >= 2 ? M2 / (k - 1) : 0
 *               k == 0: lppd = -inf, mean = -inf, p_waic = NaN
 * with correctly rounded exp and log and no fused multiply-add, so the result
 * does not depend on the tiling and equals a host build of the rule bit for
 * bit. A NaN term makes the trial's lppd, p_waic and mean NaN.
 * out_sums[S * nodes]: row s is bit for bit what the family's one-call entry
 * returns for table s. out_stats[4 * len]: lppd at [i], p_waic at [len + i],
 * the mean term at [2 len + i], n_inf (a whole number) at [3 len + i].
 * *out_ninf_total: the (sweep, trial) pairs with a zero density.
 * WFPT_ERR_ARG before any device work: a null pointer, S < 1, a data set
 * without node ids or of another context; the family's own WFPT_ERR_UNSUPPORTED
 * cases apply (one p_outlier per sweep's batch, node sizes). */
/* tables[S * n_nodes]: sweep s's row of node j at [s n_nodes + j]. len = the
 * data set's size; out_stats is in the caller's trial order. */
int wfpt_pointwise_nodes(wfpt_ctx *ctx, const wfpt_ds *ds, const wfpt_params *tables, int64_t S,
                         const wfpt_knobs *k, int64_t max_workspace, double *out_sums,
                         double *out_stats, int64_t *out_ninf_total);
/* Over the multi-table RL node batch: rl_tables[3 * S * n_nodes], tables[S *
 * n_nodes] as in wfpt_wiener_like_rlddm_nodes_multi. len = m_scored, the trials
 * that are scored (all but each segment's first), in the data set's compact
 * order; out_index[m_scored] is the caller's index of each entry. A p_outlier
 * outside [0, 1] makes every sum -inf and every term a zero density. */
int wfpt_pointwise_rlddm_nodes(wfpt_ctx *ctx, const wfpt_rl_ds *ds, const double *rl_tables,
                               const wfpt_params *tables, int64_t S, const wfpt_knobs *k,
                               int64_t max_workspace, double *out_sums, double *out_stats,
                               int64_t *out_index, int64_t *out_ninf_total);
/* Over the regression groups call: coef[S * n_groups * C], per_group[S *
 * n_groups]. That call scores one table, so a tile is one sweep (max_workspace
 * is not used); the state stays on the device between sweeps. len = n;
 * out_stats is in the caller's trial order. */
int wfpt_pointwise_reg_groups(wfpt_ctx *ctx, const wfpt_reg_ds *ds, const wfpt_reg_term *terms,
                              int32_t n_terms, const double *coef, const wfpt_params *per_group,
                              int64_t S, const wfpt_knobs *k, int64_t max_workspace,
                              double *out_sums, double *out_stats, int64_t *out_ninf_total);
/* Device ms of the accumulate kernel since the last reset, summed over the
 * tiles of profiled passes (wfpt_profile_enable with WFPT_PROF_EVENTS; such a
 * pass waits for each tile's kernel). */
int wfpt_pointwise_profile(wfpt_ctx *ctx, double *accumulate_ms, int reset);

/* ---- DMAT / Tuerlinckx CDF ---------------------------------------------- */
/* Per-trial CDF of signed RTs with the outlier mixture, exactly
 * cdfdif_wrapper.dmat_cdf_array(x, v, sv, a, z, sz, t, st, p_outlier, w_outlier)
 * (src/cdfdif_wrapper.pyx:16-53 over cdfdif, src/cdfdif.c:59-221); p->p_outlier
 * is the mixture weight. Parameters outside the support return WFPT_ERR_ARG
 * (the reference raises ValueError, cdfdif_wrapper.pyx:23-25). */
int wfpt_dmat_cdf_array(wfpt_ctx *ctx, const double *x, int64_t n, const wfpt_params *p,
                        double w_outlier, double *out);
/* The quantile objectives (hddm/likelihoods.py:200-239) for R rows in one
 * launch. Row r has its own parameters rows[r], E signed RT edges x[r * E ..]
 * (ascending: lower-boundary edges negative), E + 1 observed bin counts
 * freq_obs[r * (E + 1) ..] and n_samples[r]; one w_outlier for the call.
 *   out_cdf[R * E] (nullable)  bit for bit wfpt_dmat_cdf_array of x[r][e] with
 *                              rows[r]
 *   out_chisq[R]  sum_k (f_k - p_k n)^2 / (p_k n), k = 0..E in order, with
 *                 p = diff([0, cdf, 1]) and p_k <= 1e-6 replaced by 1e-6
 *   out_gsq[R]    2 sum_k f_k log(p_k)
 * freq_obs, n_samples, out_chisq and out_gsq are null together (CDF values
 * only). A row outside the support (cdfdif_wrapper.pyx:23-25, or with a NaN
 * parameter) does not fail the call: its chisq is +inf, its gsq -inf and its
 * cdf NaN, as the reference's `except ValueError` branches give; no other row
 * changes. Results depend on neither a row's position nor R.
 * WFPT_ERR_ARG: null pointers, R < 1, E outside 1..64. The RT range check of
 * the reference wrapper is the caller's (hddm_amd.cdfdif_wrapper). */
int wfpt_dmat_cdf_rows(wfpt_ctx *ctx, const wfpt_params *rows, const double *x,
                       const double *freq_obs, const double *n_samples, int64_t R, int32_t E,
                       double w_outlier, double *out_cdf, double *out_chisq, double *out_gsq);

/* ---- multi-GPU: trials sharded over GPUs, RCCL all-reduce over xGMI ----- */
/* (The reference has no multi-device path; SURVEY.md §8(e). Every entry point
 * below is new, combining per-shard wiener_like sums, src/wfpt.pyx:66-76.) */
/* One process per GPU. The 128-byte RCCL unique id is created on rank 0 and
 * handed to every rank, either by the caller (wfpt_comm_init) or by the
 * library's own TCP rendezvous: rank 0 listens on host:port and sends the id
 * to each rank that connects (wfpt_comm_exchange_id; no GPU, no PyTorch). */
int wfpt_comm_unique_id(unsigned char id[128]);
int wfpt_comm_init(wfpt_ctx *ctx, int nranks, int rank, const unsigned char id[128]);
int wfpt_comm_exchange_id(int nranks, int rank, const char *host, int port, int timeout_ms,
                          unsigned char id[128]);
/* unique id on rank 0 + wfpt_comm_exchange_id + wfpt_comm_init */
int wfpt_comm_init_tcp(wfpt_ctx *ctx, int nranks, int rank, const char *host, int port,
                       int timeout_ms);
/* wiener_like over this rank's resident shard, combined across ranks with one
 * ncclAllReduce of 3 doubles {sum log p, #zero-density trials, encoded error
 * counts}; every rank receives the global total (-inf if any rank holds a
 * zero-density trial) or every rank fails: WFPT_ERR_UNSUPPORTED if some rank
 * exceeded the depth / evaluation limits; a rank whose call fails after its
 * communicator exists (bad dataset or pointer arguments, workspace allocation,
 * a kernel or timeout error in its local pass) returns its own error after
 * entering the exchange with a poisoned triple (wfpt_result_poison, written on
 * the device into a triple allocated at wfpt_open), and its peers return
 * WFPT_ERR_COMM — no rank is left waiting in the collective. Not covered: a
 * context without a communicator (no collective exists), and a broken device
 * stream (sticky fault), which cannot enqueue the exchange: that rank aborts
 * its communicator, and its peers' collective fails or times out in RCCL. A
 * failed call resets the dataset's call-sequence predictions. */
int wfpt_wiener_like_allreduce(wfpt_ctx *ctx, const wfpt_ds *ds, const wfpt_params *p,
                               const wfpt_knobs *k, double *out_logp);
/* One process driving n GPUs (e.g. a single PyMC sampler): ctxs[i] (distinct
 * devices) get one communicator each from ncclCommInitAll; dss[i] is the i-th
 * shard, resident on ctxs[i]. The group call overlaps the devices' level-0
 * passes and issues the n all-reduces inside one ncclGroupStart/End; a local
 * failure on any device ends the call before the collective. */
int wfpt_comm_init_all(wfpt_ctx *const *ctxs, int n);
int wfpt_wiener_like_allreduce_group(wfpt_ctx *const *ctxs, const wfpt_ds *const *dss, int n,
                                     const wfpt_params *p, const wfpt_knobs *k,
                                     double *out_logp);
/* This rank's local triple {sum log p, #zero-density trials, encoded error
 * counts} of its resident shard — exactly what wfpt_wiener_like_allreduce
 * contributes to its all-reduce — for a caller that combines shards with its
 * own collective (sum the triples, then wfpt_decode_result). A p_outlier
 * outside [0, 1] gives {0, 1, 0} (decodes to -inf). */
int wfpt_wiener_like_local(wfpt_ctx *ctx, const wfpt_ds *ds, const wfpt_params *p,
                           const wfpt_knobs *k, double triple[3]);
/* Hierarchical (batched) mode across ranks ("count =
 * n_nodes"): each rank holds a node dataset of its own trial shard with the
 * global node ids (a node may be split over ranks or absent); its per-node
 * partial sums plus the encoded error count (n_nodes + 1 doubles) are summed
 * with one ncclAllReduce, and every rank receives the per-node totals of all
 * trials in out_logp[n_nodes] (a node with a zero-density trial on any rank is
 * -inf). n_nodes is the length of per_node, the same on every rank; the
 * exchange's count is taken from it, never from the dataset, so a rank whose
 * dataset is bad (null, another context's, without node ids, or with another
 * node count: WFPT_ERR_ARG) still enters the same n_nodes + 1 exchange,
 * poisoned. Failure semantics otherwise as wfpt_wiener_like_allreduce;
 * n_nodes < 0 returns WFPT_ERR_ARG before any collective. */
int wfpt_wiener_like_nodes_allreduce(wfpt_ctx *ctx, const wfpt_ds *ds,
                                     const wfpt_params *per_node, int32_t n_nodes,
                                     const wfpt_knobs *k, double *out_logp);
/* This rank's part of that exchange, for a caller with its own collective:
 * out[n_nodes + 1] = the per-node partial sums of its shard and the encoded
 * error count (sum over ranks, then a nonzero last entry decodes as in
 * wfpt_decode_result's third word). */
int wfpt_wiener_like_nodes_local(wfpt_ctx *ctx, const wfpt_ds *ds, const wfpt_params *per_node,
                                 const wfpt_knobs *k, double *out);
/* The triple a rank that failed before the exchange contributes: {0, 0,
 * 2^40} (one "failed rank" unit; see wfpt_decode_result). */
int wfpt_result_poison(double r[3]);

/* Decodes a likelihood result triple {sum of log p over trials with nonzero
 * density, #zero-density trials, encoded error counts} — the 3 doubles that
 * wfpt_wiener_like_allreduce sums over ranks — into the reference's value:
 * -inf if any trial had zero density (wfpt.pyx:71-72), else the sum; a nonzero
 * error count returns an error naming each kind: WFPT_ERR_UNSUPPORTED for the
 * depth / budget limits, WFPT_ERR_COMM when only failed ranks are counted.
 * Error encoding: (#ranks past WFPT_MAX_DEPTH) + 2^20 * (#ranks past
 * WFPT_EVAL_BUDGET) + 2^40 * (#ranks failed before the exchange), so kinds
 * stay apart under the sum. */
int wfpt_decode_result(const double r[3], double *out_logp);

/* ---- RT sampler --------------------------------------------------------- */
/* gen_rts_from_cdf (src/wfpt.pyx:323-354) for R parameter rows in one call:
 * per row the density full_pdf(x, v, sv, a, z, sz, 0, 0, 1e-4) at grid[1 .. G),
 * its running sum in the reference's order, the division by the last sum,
 * np.searchsorted(side='left') of each choice uniform, and the
 * non-decision-time shift rt + sign(rt) t (st == 0) or rt + sign(rt) (u st +
 * (t - st / 2)). Grid, CDF and search stay on the device; only the draws come
 * back.
 *   grid      G >= 2 rising doubles (the caller's: np.arange's own values)
 *   rows      R >= 1 parameter rows (p_outlier ignored)
 *   counts    R draws per row, >= 0
 *   u_choice, u_delay   sum(counts) uniforms in [0, 1) each, row after row, or
 *             both NULL: then each uniform is a Philox4x32-10 draw with the
 *             key {seed lo, seed hi} at counter {draw lo, draw hi, row, stream}
 *             (stream 0 choice, 1 delay; draw = the index inside the row), u =
 *             ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53. u_delay may be NULL when
 *             every row has st == 0.
 *   workspace_bytes   device bytes for the rows' grids (0: 1 GiB); the rows
 *             are processed in tiles of max(1, workspace_bytes / (8 (G - 1)))
 *             rows, and the result does not depend on the tiling (the
 *             allocation is rounded up to whole blocks of 64 rows)
 *   out       sum(counts) signed RTs, row after row
 * A row whose densities do not sum to a finite positive value (invalid
 * parameters: all zero; a == 0: NaN) fails the call with WFPT_ERR_UNSUPPORTED
 * and a message naming the first such row; nothing is written to out. */
int wfpt_gen_rts_nodes(wfpt_ctx *ctx, const double *grid, int64_t G, const wfpt_params *rows,
                       int64_t R, const int64_t *counts, const double *u_choice,
                       const double *u_delay, uint64_t seed, int64_t workspace_bytes,
                       double *out);
/* As wfpt_gen_rts_nodes (wfpt.pyx:323-354), with the intermediate arrays of a
 * debugging call (each nullable): out_pdf / out_cdf [R x (G - 1)] the grid
 * densities and the normalised CDF, out_idx [sum(counts)] each draw's grid
 * index, out_u_choice / out_u_delay [sum(counts)] the uniforms used (the delay
 * uniform of a row with st == 0 is 0). */
int wfpt_gen_rts_nodes_ex(wfpt_ctx *ctx, const double *grid, int64_t G, const wfpt_params *rows,
                          int64_t R, const int64_t *counts, const double *u_choice,
                          const double *u_delay, uint64_t seed, int64_t workspace_bytes,
                          double *out, double *out_pdf, double *out_cdf, int64_t *out_idx,
                          double *out_u_choice, double *out_u_delay);

/* _gen_rts_from_simulated_drift (hddm/generate.py:208-319), the 'drift'
 * sampling method, for R parameter rows in one call: every draw is one
 * +-sqrt(dt) intra_sv random walk from y0 = ((z + sz u_z) - sz / 2) a between 0
 * and a, going up with probability 0.5 (1 + sqrt(dt) / intra_sv drift), until
 * the first step k whose position y2 is < 0 or > a; the crossing time is
 * interpolated on the last segment (m = (y2 - y1) / dt, b = y2 - (m k) dt, rt
 * = ((y2 < 0 ? 0 : a) - b) / m) and the draw is (rt + delay) sign, delay = (t +
 * st u_t) - st / 2. drift = v, or v + sv n when sv != 0. The arithmetic is the
 * reference's, operation for operation.
 *   rows      R >= 1 parameter rows (p_outlier ignored)
 *   sw        NULL, or R triples {v_switch, V_switch, t_switch}: steps k >=
 *             nn = round(t_switch / dt) (half to even; >= 1) use the drift
 *             v_switch, or v_switch + V_switch n' when V_switch != 0
 *   counts    R draws per row, >= 0
 *   max_steps 1 .. 2^31: a draw that has not crossed after max_steps steps is
 *             NaN; *n_unfinished is the number of such draws
 *   out       sum(counts) signed RTs, row after row
 * Random numbers: Philox4x32-10 with the key {seed lo, seed hi} at counter
 * {draw lo, draw hi, row, stream}, draw = the index inside the row. Stream 1:
 * u_t, stream 2: u_z (53-bit uniforms as in wfpt_gen_rts_nodes; stream 0 stays
 * that sampler's choice); stream 3: n = sqrt(-2 log(1 - u1)) cos(2 pi u2) with
 * u1 from words 0, 1 and u2 from words 2, 3; stream 4: n' likewise; stream 16 +
 * k / 4: word k % 4 decides step k, up iff w 2^-32 < the probability. A draw's
 * value therefore depends on (seed, row, draw) and the row's parameters only.
 * WFPT_ERR_ARG before any device work: null pointers, dt <= 0, intra_sv <= 0,
 * a negative count, max_steps out of range, round(t_switch / dt) < 1.
 * WFPT_ERR_UNSUPPORTED, naming the first such row, also before any device
 * work: a non-finite parameter, a <= 0, z - sz / 2 < 0 or z + sz / 2 > 1. */
int wfpt_gen_rts_drift_nodes(wfpt_ctx *ctx, const wfpt_params *rows, int64_t R, const double *sw,
                             const int64_t *counts, double dt, double intra_sv,
                             int64_t max_steps, uint64_t seed, double *out,
                             int64_t *n_unfinished);
/* As wfpt_gen_rts_drift_nodes (generate.py:208-319), for tests and
 * measurements. row0: added to the row index in the Philox counter (a slice
 * of a larger table draws what it draws there). wave_draws: draws handed to
 * one wave, a multiple of 64 (0: the library's choice; 64: one draw per lane;
 * more: lanes take the next draw as they finish) -- it changes no value. Per
 * draw, each nullable: out_y0 the start point, out_delay, out_drift,
 * out_drift_switch (0 without a switch), out_n_steps the steps taken (the
 * crossing step's index + 1, or max_steps). out_wave_steps
 * [ceil(sum(counts) / wave_draws), wave_draws > 0]: the steps each wave's loop
 * ran. */
int wfpt_gen_rts_drift_nodes_ex(wfpt_ctx *ctx, const wfpt_params *rows, int64_t R,
                                const double *sw, const int64_t *counts, double dt,
                                double intra_sv, int64_t max_steps, uint64_t seed, int64_t row0,
                                int32_t wave_draws, double *out, int64_t *n_unfinished,
                                double *out_y0, double *out_delay, double *out_drift,
                                double *out_drift_switch, int64_t *out_n_steps,
                                int64_t *out_wave_steps);

/* ---- closed-loop RLDDM simulator ------------------------------------------ */
/* Where the reward of a simulated trial comes from; exactly one of the three
 * must be given (the other pointers NULL):
 *   p             R pairs {p_upper, p_lower} in [0, 1]: the option's reward is
 *                 1.0 if u < p else 0.0, u a device uniform (below)
 *   rew_up/_low   the two options' rewards per trial (any finite or infinite
 *                 value; generate.py:463-464 draws them up front)
 *   obs_response/ observed mode, the reference's one-step-ahead simulator
 *   obs_feedback  (generate.py:608-661): Q moves by the observed pair (response
 *                 0 lower, else upper) and the simulated RT is only recorded
 * Trial k of row r reads element start[r] + k of the supplied / observed
 * arrays of n elements (start NULL: the row's own offset, sum of the counts
 * before it), so replicate rows can share one copy. */
typedef struct {
  const double *p;
  const double *rew_up, *rew_low;
  const int64_t *obs_response;
  const double *obs_feedback;
  const int64_t *start;
  int64_t n;
} wfpt_rl_source;
/* gen_rand_rlddm_data (hddm/generate.py:430-516) for R sequence rows in one
 * launch, one lane per sequence. Row r: the DDM row rows[r] (v is the drift
 * scaling; p_outlier ignored), the RL row rl_rows[3 r ..] = {q, alpha,
 * pos_alpha} with wfpt_wiener_like_rlddm's conventions (alpha unbounded, the
 * rate 2.718281828459**alpha / (1 + 2.718281828459**alpha) by libm pow;
 * pos_alpha == 100.0: use alpha) and counts[r] >= 0 trials; trial k of row r is
 * element off[r] + k of out. Per trial, in this order: drift = (q_up - q_low)
 * v (+ sv n when sv != 0); start point, delay and walk as in
 * wfpt_gen_rts_drift_nodes, operation for operation; response = rt > 0; the
 * feedback is the chosen option's reward; rate = pos rate if feedback >
 * q_chosen (strict) else rate; q_chosen += rate (feedback - q_chosen), three
 * separately rounded operations as in the likelihood.
 * Random numbers: wfpt_gen_rts_drift_nodes' Philox counters with draw = the
 * trial index k: {k lo, k hi, row, stream}, streams 1, 2, 3 and 16 + step / 4
 * as there; stream 5 / 6: the upper / lower option's reward uniform. A row
 * whose drift never moves draws what row r of wfpt_gen_rts_drift_nodes draws.
 * A walk cut at max_steps makes its trial NaN and ends the sequence: every
 * later trial of the row is NaN; *n_unfinished counts the NaN trials.
 * WFPT_ERR_ARG before any device work: null pointers, R < 1, dt / intra_sv /
 * max_steps as in wfpt_gen_rts_drift_nodes, a negative count, none or more than
 * one reward source, a p outside [0, 1], a NaN in rl_rows, a start[r] with
 * start[r] + counts[r] outside the n elements. WFPT_ERR_UNSUPPORTED, naming
 * the row: a row wfpt_gen_rts_drift_nodes cannot simulate. */
int wfpt_gen_rlddm_rows(wfpt_ctx *ctx, const wfpt_params *rows, const double *rl_rows, int64_t R,
                        const int64_t *counts, const wfpt_rl_source *source, double dt,
                        double intra_sv, int64_t max_steps, uint64_t seed, double *out,
                        int64_t *n_unfinished);
/* As wfpt_gen_rlddm_rows. row0 (row0 + R <= 2^31): added to the row index in
 * the Philox counter. wave_rows: rows handed to one wave, a multiple of 64 (0:
 * the library's choice) -- it changes no value. Per trial, each nullable:
 * out_feedback; out_q_up / out_q_low the Q values before the trial's update;
 * out_sim_drift = (q_up - q_low) v; out_drift the walk's drift; out_y0;
 * out_delay; out_n_steps (0 for a trial after a cut one, whose other outputs
 * are NaN). out_wave_steps [ceil(R / wave_rows), wave_rows > 0]. */
int wfpt_gen_rlddm_rows_ex(wfpt_ctx *ctx, const wfpt_params *rows, const double *rl_rows,
                           int64_t R, const int64_t *counts, const wfpt_rl_source *source,
                           double dt, double intra_sv, int64_t max_steps, uint64_t seed,
                           int64_t row0, int32_t wave_rows, double *out, int64_t *n_unfinished,
                           double *out_feedback, double *out_q_up, double *out_q_low,
                           double *out_sim_drift, double *out_drift, double *out_y0,
                           double *out_delay, int64_t *out_n_steps, int64_t *out_wave_steps);

/* ---- per-row RT statistics ----------------------------------------------- */
/* gen_ppc_stats (hddm/utils.py:241-265), the posterior predictive check's
 * summary statistics, for R rows of signed RTs in one call. Row r's draws are
 * rts[off[r] .. off[r + 1]) (off: R + 1 rising offsets from 0); ub is the set
 * of draws x > 0, lb the set x < 0; a draw that is 0 or NaN is in neither but
 * counts in n. Per row, K = 8 + 2 nq doubles go to out[r K ..):
 *   n, n_ub, n_lb, accuracy = n_ub / n,
 *   mean_ub, std_ub, q_ub[0 .. nq),  mean_lb (signed: negative), std_lb, q_lb[0 .. nq)
 * std is the population standard deviation (np.std, ddof = 0), two-pass. q_ub[k]
 * / q_lb[k] is scipy.stats.scoreatpercentile(x[x > 0] / abs(x[x < 0]), q[k]) bit
 * for bit: on the m sorted values s, idx = q / 100. * (m - 1), i = (int)idx, s[i]
 * when i == idx, else (s[i] w0 + s[i + 1] w1) / (w0 + w1) with w0 = (i + 1) - idx,
 * w1 = idx - i. An empty set gives NaN for its mean, std and percentiles, n == 0 a
 * NaN accuracy. The counts, the accuracy and the percentiles do not depend on
 * the kernel that scored the row; the means and standard deviations are summed
 * in an order that depends on the row's values alone.
 *   q         nq percentiles in [0, 100], 0 <= nq <= 16 (NULL when nq == 0)
 * WFPT_ERR_ARG before any device work: null pointers, R < 1, nq outside
 * 0..16, a q outside [0, 100] or NaN, off[0] != 0 or a falling off. */
int wfpt_rt_stats_rows(wfpt_ctx *ctx, const double *rts, const int64_t *off, int64_t R,
                       const double *q, int32_t nq, double *out);
/* As wfpt_rt_stats_rows (utils.py:241-265), for tests: tier 0 is the library's
 * choice by row length, 1 / 2 / 3 force the wave (rows of at most 256 draws) /
 * block (at most 4096) / global tier for every row. WFPT_ERR_ARG: a row the
 * forced tier cannot hold, tier outside 0..3. */
int wfpt_rt_stats_rows_ex(wfpt_ctx *ctx, const double *rts, const int64_t *off, int64_t R,
                          const double *q, int32_t nq, int32_t tier, double *out);
/* wfpt_gen_rts_nodes followed by the statistics of its draws (utils.py:241-265)
 * while they are still in device memory: the draws are those of
 * wfpt_gen_rts_nodes for the same arguments bit for bit, stats_out [R x (8 + 2
 * nq)] is what wfpt_rt_stats_rows gives for them. out may be NULL: no draw is
 * copied to the host. A call that fails (an argument error, a row without a
 * CDF) writes neither out nor stats_out. */
int wfpt_gen_rts_nodes_stats(wfpt_ctx *ctx, const double *grid, int64_t G,
                             const wfpt_params *rows, int64_t R, const int64_t *counts,
                             const double *u_choice, const double *u_delay, uint64_t seed,
                             int64_t workspace_bytes, double *out, const double *q, int32_t nq,
                             double *stats_out);
/* wfpt_gen_rts_drift_nodes followed by the statistics of its draws
 * (utils.py:241-265), as wfpt_gen_rts_nodes_stats: the same draws bit for bit,
 * out may be NULL, *n_unfinished is counted either way. An unfinished walk's
 * NaN counts in its row's n and in neither boundary. */
int wfpt_gen_rts_drift_nodes_stats(wfpt_ctx *ctx, const wfpt_params *rows, int64_t R,
                                   const double *sw, const int64_t *counts, double dt,
                                   double intra_sv, int64_t max_steps, uint64_t seed,
                                   double *out, int64_t *n_unfinished, const double *q,
                                   int32_t nq, double *stats_out);

/* wfpt_gen_rlddm_rows followed by the statistics of its draws while they are
 * still in device memory. Statistics row g covers the trials of the rows
 * [group_off[g], group_off[g + 1]) (n_groups + 1 rising offsets from 0 to R):
 * a node made of its condition sequences. stats_out [n_groups x (8 + 2 nq)] is
 * what wfpt_rt_stats_rows gives for those draws; out may be NULL; *n_unfinished
 * is counted either way. */
int wfpt_gen_rlddm_rows_stats(wfpt_ctx *ctx, const wfpt_params *rows, const double *rl_rows,
                              int64_t R, const int64_t *counts, const wfpt_rl_source *source,
                              double dt, double intra_sv, int64_t max_steps, uint64_t seed,
                              double *out, int64_t *n_unfinished, const int64_t *group_off,
                              int64_t n_groups, const double *q, int32_t nq, double *stats_out);

/* ---- measurement -------------------------------------------------------- */
/* Under WFPT_PROF_EVENTS: device milliseconds of the RT sampler's stages
 * {density, running sum, normalisation, draws} since the last reset (they are
 * also part of wfpt_profile_read's total, four launches per tile). */
int wfpt_profile_stages(wfpt_ctx *ctx, double stage_ms[4], int reset);
/* flags & WFPT_PROF_EVENTS: bracket the main likelihood kernel of each call
 * with HIP events on the context's stream (per-launch device time);
 * flags & WFPT_PROF_EVALS: count pdf_sv evaluations (a separate kernel build
 * with one integer atomic per block; use it in an untimed pass). 0 = off. */
#define WFPT_PROF_EVENTS 1
#define WFPT_PROF_EVALS 2
int wfpt_profile_enable(wfpt_ctx *ctx, int flags);
/* Accumulated main-kernel milliseconds, launches and pdf_sv evaluations since
 * the last reset. */
int wfpt_profile_read(wfpt_ctx *ctx, double *kernel_ms, int64_t *launches, int64_t *n_evals,
                      int reset);
/* Refinement work of the adaptive calls made under WFPT_PROF_EVALS since the
 * last reset (synchronises the stream): counts[L] (L = 1, 2) t-node (or z
 * grid) evaluations of tree level L, counts[4] trials whose root interval was
 * refined, counts[5] trials settled on the exact path, counts[6] trials
 * continued on the per-lane walk, counts[7] z walks (counts[8 + L]: at tree
 * level L). counts[11..15]: per-phase engine time of diagnostic builds
 * (WFPT_PHASE_TIMING), kilo-cycles summed over waves. The per-node path
 * (wfpt_wiener_like_nodes, adaptive families) adds to the same counters, plus
 * counts[3] trials its level-0 pass left to the chunk engine and counts[0]
 * node segments the chunk engine ran (one per node present in a listed
 * chunk). A resident full-DDM call whose level 0 is the lean pass adds to
 * counts[3] the number of its waves (64-trial chunks) that took the generic
 * per-lane site instead of the uniform-wave one, and to counts[0] the number
 * of its waves whose five series decisions came from the decision table and
 * that completed on the uniform-wave site (every slot 0..10 has a writer:
 * counts[8] is the z walks after level 0; slots 0 and 3 are the ones a
 * resident call leaves alone). */
int wfpt_profile_lists(wfpt_ctx *ctx, int64_t counts[16], int reset);
/* Diagnostic builds (WFPT_PHASE_TIMING): the last engine launch's per-wave
 * records, 8 words per 64-trial chunk {start, end (100 MHz real-time clock),
 * 5 phase cycle counts, z rounds | t rounds << 32}; zeros otherwise. */
int wfpt_debug_waves(wfpt_ctx *ctx, uint64_t *out, int64_t max_records);
/* The chunks the last likelihood call's lean level-0 pass dispatched first
 * (ascending chunk ids, at most 64; *n = 0: stored order): the chunks the
 * host predicted to hold a breakpoint of the series decision. Up to
 * max_chunks of them are written to chunks. */
int wfpt_debug_lean_first(wfpt_ctx *ctx, int32_t *chunks, int32_t max_chunks, int32_t *n);
/* The first n per-chunk partials {sum of the chunk's log terms, zero word}
 * the last summing call left on the device (64 stored trials per chunk for
 * the adaptive / direct families; synchronises the stream). Tests compare
 * them with the reference's per-chunk sums. */
int wfpt_debug_partials(wfpt_ctx *ctx, double *part, int32_t *zero, int64_t n);
/* Kernels the last likelihood call launched (OR of WFPT_PATH_*). */
#define WFPT_PATH_LEAN 1     /* lean level-0 pass (lean_kernel) */
#define WFPT_PATH_ENGINE 2   /* in-wave adaptive engine over every chunk */
#define WFPT_PATH_SMALL 4    /* one-block level 0 + finalize (small_kernel) */
#define WFPT_PATH_REDO 8     /* engine over the chunks the lean pass flagged */
#define WFPT_PATH_FOLD 16    /* deferred trials (exact path / deep trees) */
#define WFPT_PATH_DIRECT 32  /* simple-DDM level 0 (fast_kernel) */
#define WFPT_PATH_FIXED 64   /* fixed Simpson (trial_kernel) */
#define WFPT_PATH_SPLIT 128  /* heavy chunks split into one-wave units */
#define WFPT_PATH_SMALL_SPLIT 256 /* the full DDM's one-block call, three lanes per
                                     trial (small_split_kernel; with WFPT_PATH_SMALL) */
#define WFPT_PATH_NODE_SPLIT 512  /* per-node call: t-node split level 0
                                     (node_grid_kernel + node_split_kernel) */
#define WFPT_PATH_NODE_RARE 1024  /* per-node call: rare trials (exact path / deep trees)
                                     settled by node_rare_kernel, sums published again */
int wfpt_last_path(wfpt_ctx *ctx, int *path);
int wfpt_synchronize(wfpt_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* WFPT_AMD_H */
