/* lorads_host.h -- plain-C host side of the MI355X low-rank SDP solver.
 *
 * The host keeps what BASELINE.json's north_star says it keeps: the SDPA reader, the pre-solver,
 * the rank rule, the LoRADS-compatible parameter block and the scalar outer-loop control of both
 * phases.  Every per-iteration numerical step is reached through ONE table, `lrd_backend`, which
 * mirrors the reference's operator table `lorads_func`
 * (reference: src_semi/data/def_lorads_solver.h:109-127, filled by LORADSInitFuncSet,
 * src_semi/data/lorads_solver.c:717-756).  The product wires that table to the HIP C-ABI library
 * (include/lorads_hip.h) and to nothing else; tests wire it to the CPU oracle to check the HIP path.
 */
#ifndef LORADS_HOST_H
#define LORADS_HOST_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* return codes of the four *Optimize* loops (reference: src_semi/lorads.h:62-65) */
#define LRD_RET_OK 0
#define LRD_RET_TIME_OUT 1
#define LRD_RET_NUM_ERR 4
#define LRD_RET_BAD_ITER 8

/* solver status (reference: src_semi/lorads.h:45-51) */
enum { LRD_UNKNOWN = 0, LRD_PRIMAL_DUAL_OPTIMAL, LRD_PRIMAL_OPTIMAL, LRD_MAXITER, LRD_TIME_LIMIT };

/* parameter block, field-for-field the reference's lorads_params (src_semi/lorads.h:82-105);
 * defaults in lrd_params_default() are the reference CLI defaults (src_semi/main.c:19-43). */
typedef struct {
    const char *fname;
    double initRho, rhoMax, rhoCellingALM, rhoCellingADMM;
    int maxALMIter, maxADMMIter;
    double timesLogRank;
    int rhoFreq;
    double rhoFactor, ALMRhoFactor, phase1Tol, phase2Tol, timeSecLimit, heuristicFactor;
    int lbfgsListLength;
    double endTauTol, endALMSubTol;
    int l2Rescaling, reoptLevel, dyrankLevel, highAccMode;
    int verbose; /* ours: 0 silences the log lines */
} lrd_params;

/* One SDP cone ("block") as a flat image.  All symmetric matrices are lower-triangular triplets
 * (row >= col) ordered by packed column-major index, which is the order the reference's reader
 * produces (src_semi/io/lorads_file_io.c:273-283, linalg/lorads_sparse_opts.c:37-52). */
typedef struct {
    int n;        /* cone dimension */
    int nrow;     /* constraints whose A_i is non-zero on this cone (reference nRowElem / nnzStat) */
    int *row_idx; /* [nrow] global constraint index, ascending */
    int *a_ptr;   /* [nrow+1] */
    int *a_row, *a_col;
    double *a_val;
    int c_nnz;
    int *c_row, *c_col;
    double *c_val; /* C = -F0 already applied (src_semi/io/lorads_file_io.c:279-281) */
    /* decisions the reference takes in its pre-solver, restated */
    int cone_sparse; /* 1: LORADS_CONETYPE_SPARSE_SDP (io/lorads_user_data.c:58-71, threshold 0.3 m) */
    int dense_mode;  /* 1: union scratch is dense packed (data/lorads_sdp_conic.c:884,970,989,1072) */
    /* union pattern of C and all A_i, unique lower-tri positions sorted by (col,row)
     * (data/lorads_sdp_conic.c:965-1068); the full lower triangle when dense_mode */
    int np;
    int *p_row, *p_col;
    int *a_pidx; /* [a_ptr[nrow]] position of each A entry in the pattern (nnzIdx2ResIdx) */
    int *c_pidx; /* [c_nnz] */
    int rank, rank_max; /* data/lorads_solver.c:290-319 */
    /* 1: this "cone" is the LP block of the file (one diagonal block, last; io/lorads_file_io.c:120-124,260-269):
     * n = number of LP columns, every entry diagonal, rank fixed at 1 -- x_i = r_i^2 (u_i v_i).  In phase 1 and in
     * every evaluation it behaves as a diagonal cone (data/lorads_lp_conic.c:172-217); only the ADMM update differs:
     * column by column in closed form (lorads_alg/lorads_admm.c:595-629, lorads_alg_common.c:225-248). */
    int is_lp;
    int global_id;      /* index of this cone in the file (multi-GPU sharding keeps a subset) */
} lrd_block;

typedef struct {
    int m;     /* number of constraints (global) */
    double *b; /* [m] */
    int nblk;  /* blocks held by THIS process */
    lrd_block *blk;
    int nblk_global;
    int nsdp_global;     /* SDP cones of the file (ASolver->nCones): the LP block is not one of them */
    int sum_dims_global; /* sum of all SDP block dims, for rho0 = 1/sqrt(.) (data/lorads_solver.c:1155-1162) */
    /* norms (data/lorads_solver.c:1054-1073), over ALL blocks of the file */
    double cObjNrm1, cObjNrm2, cObjNrmInf, bNrm1, bNrm2, bNrmInf;
    /* set by lrd_problem_localize: this image is one rank's sub-problem of a block-separable deal -- m, b and the row indices are
     * the rank's own; con_global[i] = index of local constraint i in the file (m_global constraints) */
    int separable, m_global;
    int *con_global;
} lrd_problem;

/* which factor pair an evaluation uses */
enum { LRD_PAIR_RR = 0, LRD_PAIR_UV = 1 };
/* state arrays that can be moved across the boundary (column-major n x r, as the reference) */
enum { LRD_MAT_R = 0, LRD_MAT_U = 1, LRD_MAT_V = 2, LRD_MAT_GRAD = 3 };
enum { LRD_VEC_LAMBDA = 0, LRD_VEC_CONSTR_SUM = 1, LRD_VEC_Q1 = 2, LRD_VEC_Q2 = 3 };

/* Cross-process reduction hook (multi-GPU, one process per GPU): sums `count` doubles in place over
 * all ranks.  `on_device` tells whether buf is a device pointer.  NULL hook = single process. */
typedef int (*lrd_allreduce_fn)(void *user, double *buf, int count, int on_device);

/* The operator table.  One slot per lorads_func slot, plus the non-table calls on the path
 * (LORADSUpdateDualVar / LORADSCalDualObj, lorads_alg/lorads_alg_common.h:22-23; the m-vector part
 * of ALMLineSearch, lorads_alg/lorads_alm.c:161-172) and the state movers listed in SURVEY.md 8(b).
 * All return 0 on success.  Objective values are returned UNSCALED by scaleObjHis. */
typedef struct lrd_backend {
    void *ctx;
    const char *name;
    /* lorads_func.InitConstrValAll + InitConstrValSum  (lorads_alg_common.c:78-84,134-142) */
    int (*init_constr)(void *ctx, int pair);
    /* lorads_func.ALMCalGrad (lorads_alm.c:9-54): Grad_k = 2 (C + sum_i M1_i A_i) R_k, returns sum ||Grad_k||^2 */
    int (*alm_cal_grad)(void *ctx, double rho, double *lag_norm_sq);
    /* lorads_func.LBFGSDirection + LBFGSDirUseGrad (lorads_alm.c:230-391,469-489); D is stored in U */
    int (*lbfgs_direction)(void *ctx, int inner_iter);
    /* lorads_func.ALMCalq12p12 (lorads_alm.c:540-560): q1,q2 stay in the backend; p12 returned */
    int (*alm_q12p12)(void *ctx, double p12[2]);
    /* m-vector part of ALMLineSearch (lorads_alm.c:164-172): quartic coefficients a,b,c,d */
    int (*alm_linesearch_coeffs)(void *ctx, double rho, double p1, double p2, double coef[4]);
    /* lorads_func.setAsNegGrad (lorads_alm.c:583-598) */
    int (*set_y_as_neg_grad)(void *ctx);
    /* lorads_func.ALMupdateVar + the two axpys on constrValSum (lorads_alm.c:619-648,1122-1124) */
    int (*alm_update_var)(void *ctx, double tau);
    /* lorads_func.setlbfgsHisTwo (lorads_alm.c:657-678) */
    int (*set_lbfgs_his_two)(void *ctx, double tau);
    /* lorads_func.updateDimacsALM / updateDimacsADMM (lorads_alg_common.c:250-290): returns
     * ||b - sum_k A_k(.)||_2 / (1 + ||b||_1); ADMM variant first sets R = (U+V)/2 */
    int (*update_dimacs)(void *ctx, int pair, double *err1);
    /* lorads_func.calObj_alm / calObj_admm (lorads_alm.c:1259-1268, lorads_admm.c:325-337) */
    int (*cal_obj)(void *ctx, int pair, double *pobj);
    /* lorads_func.admmUpdateVar (lorads_alg_common.c:187-215): U- and V-solve per cone by CG */
    int (*admm_update_var)(void *ctx, double rho, double cg_tol, int cg_max_iter, int *cg_iters);
    /* LORADSUpdateDualVar / LORADSCalDualObj (lorads_alg_common.c:319-340) */
    int (*update_dual_var)(void *ctx, double rho);
    int (*cal_dual_obj)(void *ctx, double *dobj);
    /* state movers */
    int (*alm_to_admm)(void *ctx);                   /* R -> V -> U   (data/lorads_solver.c:968-983) */
    int (*average_uv_to_v)(void *ctx);               /* R=(U+V)/2; V=R (main.c:441-448) */
    int (*scale_obj)(void *ctx, double s);           /* C *= s, lambda *= s (data/lorads_solver.c:1040-1052) */
    int (*resize_rank)(void *ctx, const int *new_rank); /* AUG_RANK (data/lorads_solver.c:806-906) */
    int (*set_mat)(void *ctx, int which, int blk, const double *colmajor);
    int (*get_mat)(void *ctx, int which, int blk, double *colmajor);
    int (*set_vec)(void *ctx, int which, const double *v);
    int (*get_vec)(void *ctx, int which, double *v);
    int (*set_allreduce)(void *ctx, lrd_allreduce_fn fn, void *user);
    void (*destroy)(void *ctx);
    /* OPTIONAL (may be NULL): admm_update_var + cal_obj(UV) + cal_dual_obj + update_dimacs(UV) in one
     * call, same order and results (lorads_admm.c:76-81); out = {cg iterations, pobj, dobj, err1} */
    int (*admm_step)(void *ctx, double rho, double cg_tol, int cg_max_iter, double out[4]);
    /* OPTIONAL (may be NULL): calculate_dual_infeasibility_solver without its two divisions
     * (data/lorads_solver.c:1007-1033): sum over this table's cones of |min(lambda_min(C_k - A_k^*(lambda)), 0)| */
    int (*dual_infeasibility)(void *ctx, double *sum_neg_eig);
    /* OPTIONAL pair (both or neither): the phase-1 inner iteration in two calls with one host round trip each
     * (lorads_alm.c:1066-1131).  alm_front = lbfgs_direction(inner) + alm_q12p12 + alm_linesearch_coeffs,
     * out = {p1, p2, a, b, c, d};  alm_step = set_y_as_neg_grad + alm_update_var(tau) + alm_cal_grad(rho) +
     * set_lbfgs_his_two(tau) + update_dimacs(RR), then alm_front(next_inner) when next_inner >= 0,
     * out = {lagNormSq, err1, p1, p2, a, b, c, d}.  Same results as the separate slots. */
    int (*alm_front)(void *ctx, double rho, int inner, double out[6]);
    int (*alm_step)(void *ctx, double rho, double tau, int next_inner, double out[8]);
    /* OPTIONAL pair (both or neither): solution export, read-only on the state (include/lorads_hip.h: lorads_hip_certificate,
     * lorads_hip_get_slack).  certificate: src = LRD_PAIR_UV (R = (U+V)/2) or LRD_PAIR_RR, Lanczos tol (<= 0: no eigen-solves),
     * out[LRD_CERT_N] in the backend's terms (scaled by scaleObjHis); lam_min [nblk], residual [m] and y [m] (the multipliers the
     * certificate used: a dual update still waiting inside the backend applied, not stored) may be NULL.
     * get_slack: S of block blk as lower-triangle triplets; NULL arrays return the count alone. */
    int (*certificate)(void *ctx, int src, double tol, double *out, double *lam_min, double *residual, double *y);
    /* OPTIONAL (between the export pair: the table's mirror is checked to hold get_slack, round_stable, round_pm1, round_kcut and the
     * primal pair side by side): balanced partitions of a bisection-structured context read off the factors + repair + swap search,
     * read-only on the state (include/lorads_hip.h: lorads_hip_round_bisect, the same arguments and return codes; values in the
     * backend's terms) */
    int (*round_bisect)(void *ctx, int src, int trials, uint64_t seed, int max_rounds, double *obj, double *obj0, int *best, int *best0,
                        int8_t *sign, int *imbalance, int *rounds, double *hyperplanes, double *t, int *diff);
    int (*get_slack)(void *ctx, int blk, int64_t *nnz, int *row, int *col, double *val);
    /* OPTIONAL (in front of round_pm1: the table's mirror is checked to hold round_pm1, round_kcut and the primal pair side by side):
     * stable sets of a theta-structured context read off the factors + the (1, 2)-swap search, read-only on the state
     * (include/lorads_hip.h: lorads_hip_round_stable, the same arguments and return codes; values in the backend's terms) */
    int (*round_stable)(void *ctx, int src, int trials, uint64_t seed, int max_rounds, double *obj, double *obj0, int *best, int *best0,
                        uint8_t *member, int *sizes, int *rounds, double *scores, double *T);
    /* OPTIONAL: hyperplane rounding + 1-flip local search of a +-1-structured context, read-only on the state (include/lorads_hip.h:
     * lorads_hip_round_pm1, the same arguments and return codes; values in the backend's terms) */
    int (*round_pm1)(void *ctx, int src, int trials, uint64_t seed, int max_rounds, double *obj, double *obj0, int *best, int *best0,
                     int8_t *sign, int *rounds, double *hyperplanes);
    /* OPTIONAL (beside round_pm1: the table's mirror is checked to end with entry_bounds and the spectral pair): Frieze-Jerrum
     * rounding into `parts` parts + 1-move local search of a k-cut-structured context, read-only on the state (include/lorads_hip.h:
     * lorads_hip_round_kcut, the same arguments and return codes; values in the backend's terms) */
    int (*round_kcut)(void *ctx, int src, int parts, int trials, uint64_t seed, int max_rounds, double *obj, double *obj0, int *best,
                      int *best0, uint8_t *label, int *rounds, double *vectors, double *t, double *lp_upper);
    /* OPTIONAL pair (both or neither; the table's mirror is checked to END with the spectral pair, so this one stands before it):
     * entries of the primal X = F F^T and its products with a block of vectors (include/lorads_hip.h:
     * lorads_hip_primal_entries, lorads_hip_primal_apply, the same arguments and return codes; X in the file's units) */
    int (*primal_entries)(void *ctx, int src, int blk, int64_t count, const int *row, const int *col, double *val, const double *ref,
                          double *stats);
    int (*primal_apply)(void *ctx, int src, int blk, int ncols, const double *B, double *Y, double *T);
    /* OPTIONAL (beside the primal pair: the table's mirror is checked to end with entry_bounds and the spectral pair): the k best
     * entries per row of X = F F^T of one SDP cone, read-only on the state (include/lorads_hip.h: lorads_hip_primal_topk, the same
     * arguments and return codes) */
    int (*primal_topk)(void *ctx, int src, int blk, int nq, const int *row, int col_lo, int col_hi, int k, int smallest, int include_diag,
                       const int64_t *skip_ptr, const int *skip_col, int *idx, double *val, int *found);
    /* OPTIONAL (before the spectral pair for the same reason): separation of the triangle inequalities of one SDP cone of a
     * +-1-structured context, read-only on the state (include/lorads_hip.h: lorads_hip_triangle_cuts, the same arguments and
     * return codes) */
    int (*triangle_cuts)(void *ctx, int src, int blk, double min_violation, int max_cuts, int64_t *count, int *p, int *q, int *s,
                         int8_t *cls, double *viol, int *kept, int *passes);
    /* OPTIONAL (before the spectral pair for the same reason): separation of the entry bounds lower <= X_pq <= upper of one SDP cone
     * of any context, read-only on the state (include/lorads_hip.h: lorads_hip_entry_bounds, the same arguments and return codes) */
    int (*entry_bounds)(void *ctx, int src, int blk, double lower, double upper, double min_violation, int max_cuts, int64_t *count,
                        int *p, int *q, int8_t *cls, double *viol, int *kept, int *passes);
    /* OPTIONAL pair (both or neither): spectrum of the factors and their reduction to a lower rank (include/lorads_hip.h:
     * lorads_hip_spectrum, lorads_hip_compress_rank, the same arguments and return codes) */
    int (*spectrum)(void *ctx, int src, double *eig, double *q, int *sweeps);
    int (*compress_rank)(void *ctx, int src, const int *new_rank, double *eig);
} lrd_backend;
#define LRD_CERT_N 10

/* iteration states, as the reference's lorads_alm_state / lorads_admm_state
 * (data/def_lorads_solver.h:130-161) */
typedef struct {
    int outerIter, innerIter;
    double rho, l_inf_primal_infeasibility, l_1_primal_infeasibility, l_2_primal_infeasibility;
    double primal_dual_gap, primal_objective_value, dual_objective_value;
    double l_inf_dual_infeasibility, l_1_dual_infeasibility, l_2_dual_infeasibility, tau;
} lrd_alm_state;

typedef struct {
    int iter, nBlks, cg_iter;
    double rho, l_1_dual_infeasibility, l_inf_dual_infeasibility, l_1_primal_infeasibility;
    double l_inf_primal_infeasibility, l_2_primal_infeasibility, l_2_dual_infeasibility;
    double primal_objective_value, dual_objective_value, primal_dual_gap;
} lrd_admm_state;

typedef struct {
    lrd_problem *prob;
    lrd_backend *be;
    lrd_alm_state alm;
    lrd_admm_state admm;
    double pObjVal, dObjVal, err_constr_l1, err_pdgap; /* dimacError[0], [1] */
    double err_dual_l1;   /* dimacError[LORADS_DIMAC_ERROR_DUALFEASIBLE_L1]; -1 = not evaluated */
    double t_dual_infeas; /* seconds spent evaluating it (main.c all_dual_infea) */
    double scaleObjHis;
    int cgIter;     /* cumulative CG iterations of the current ADMM call (ASolver->cgIter) */
    int max_alm_sub_iter; /* the reference's global MAX_ALM_SUB_ITER (lorads_alm.c:7) */
    int status;
    int *rank;      /* [nblk] current ranks */
    lrd_allreduce_fn allreduce;
    void *allreduce_user;
    double t_alm, t_admm;
    int admm_iters_first, cg_iters_first;
    int use_fused_step; /* 1: use lrd_backend.admm_step when the table has it */
    int be_fail;        /* a table slot returned non-zero (device error, refused resize, failed all-reduce): the loops
                         * stop with LRD_RET_NUM_ERR instead of steering on numbers nobody produced */
    int in_admm;        /* phase 2 has begun (lrd_alm_to_admm) and no phase-1 round has followed: the point is R = (U+V)/2 */
} lrd_solver;

/* ---- params / problem ---- */
void lrd_params_default(lrd_params *p);
int lrd_params_set(lrd_params *p, const char *key, const char *val); /* reference CLI names, main.c:57-80 */
/* SDPA sparse reader (own implementation; conventions of src_semi/io/lorads_file_io.c:21-293). */
int lrd_read_sdpa(const char *fname, lrd_problem **out);
/* one entry line of an SDPA file, "mat blk i j value": returns the number of fields found (5 = a full entry), exactly as
 * sscanf("%d %d %d %d %lg") would; the value is converted as strtod converts it (problem.c; exported for the tests) */
int lrd_parse_entry_line(const char *line, int ij[4], double *val);
/* digest of the whole image (dimensions, every array, norms): equal digests = the same problem */
uint64_t lrd_problem_digest(const lrd_problem *p);
/* 1 when the start point is drawn by the inline copy of glibc's rand() recurrence (verified against rand() at run time), 0 when by rand() */
int lrd_start_generator_is_inline(void);

/* ---- shmx.c: sums of a few doubles (n <= 16) over the ranks of one node through POSIX shared memory; the scalar exchange of
 * separable shards (include/lorads_hip.h: lorads_hip_set_scalar_exchange).  name: "/..." -- the same on every rank, unique per run;
 * rank 0 creates and removes the segment.  All return 0 on success. */
typedef struct lrd_shmx lrd_shmx;
int lrd_shmx_open(const char *name, int world, int rank, lrd_shmx **out);
int lrd_shmx_allreduce(lrd_shmx *x, double *v, int n);
int lrd_shmx_hook(void *user, double *vals, int32_t n);
void lrd_shmx_close(lrd_shmx *x);
/* Build a problem from arrays (bench / tests; 0-based mat: 0 = F0, blk, row, col); same
 * post-processing as the reader (F0 negated, lower triangle, tiny entries dropped, pre-solve). */
int lrd_problem_from_triplets(int m, const double *b, int nblk, const int *dims, int64_t nent, const int *e_mat,
                              const int *e_blk, const int *e_row, const int *e_col, const double *e_val,
                              lrd_problem **out);
/* multi-GPU sharding: keep only the blocks with keep[k] != 0 (global consts stay global) */
void lrd_problem_select(lrd_problem *p, const int *keep);
int lrd_problem_localize(lrd_problem *p, int world, int rank_id);
void lrd_problem_free(lrd_problem *p);
/* rank rule, data/lorads_solver.c:290-319 */
void lrd_determine_rank(lrd_problem *p, double times_log_rank);
/* start point: srand(925) and the reference's draw order (data/lorads_solver.c:361-371,415,652-653):
 * R for every block, then U,V per block; call BEFORE lrd_problem_select so that every rank draws
 * the whole sequence; returns malloc'd col-major arrays indexed by block. */
int lrd_init_point(const lrd_problem *p, double ***R, double ***U, double ***V);
void lrd_free_point(int nblk, double **R, double **U, double **V);

/* ---- solver ---- */
int lrd_solver_init(lrd_solver *s, lrd_problem *prob, lrd_backend *be, const lrd_params *par);
void lrd_solver_clear(lrd_solver *s);
int lrd_alm_optimize(lrd_params *par, lrd_solver *s, int reopt_variant, int early_stop, double rho_update_factor,
                     double t_start);
int lrd_admm_optimize(lrd_params *par, lrd_solver *s, int reopt_variant, int iter_ceiling, double t_start);
void lrd_alm_to_admm(lrd_params *par, lrd_solver *s);
double lrd_reopt(lrd_params *par, lrd_solver *s, double reopt_param, int reopt_alm_iter, int reopt_admm_iter,
                 double t_start, int *admm_bad_iter_flag, int reopt_level);
/* whole solve = reference main.c:321-398 (dual infeasibility / level-2 reopt need the ARPACK step
 * and are "next") */
int lrd_solve(lrd_params *par, lrd_solver *s);
int lrd_dual_infeasibility(lrd_solver *s); /* data/lorads_solver.c:1007-1037 through the table's optional slot */

/* ---- solution export (session.c, solution.c; DESIGN.md "Exporting a solution").  Everything in the file's units (divided by
 * scaleObjHis) and numbering.  Problem: min <C, X> s.t. <A_i, X> = b_i, X psd, C = -F0, A_i = F_i (SDPA: Y_sdpa = X, x_sdpa = -y,
 * X_sdpa = S). */
typedef struct {
    int n, rank;     /* rank: the cone's current rank (LP block: 1) */
    int is_lp;
    double *R, *U, *V; /* column-major n x rank; R = (U+V)/2 in phase 2, the phase-1 R otherwise; X = R R^T */
    double *x;         /* LP block: x_j = r_j^2 (NULL on SDP cones) */
    int64_t s_nnz;     /* S = C - sum_i y_i A_i, lower-triangle triplets (LP block: one (j, j) entry per column) */
    int *s_row, *s_col;
    double *s_val;
    double lam_min;    /* lambda_min(S) (LP block: min_j s_j) */
} lrd_solution_cone;
typedef struct {
    int m, nblk, status;
    int src;           /* LRD_PAIR_UV or LRD_PAIR_RR: where R came from */
    double scale;      /* scaleObjHis the backend's values were divided by */
    double pobj, dobj; /* <C, X> + c_lp . x,  b . y */
    /* DIMACS errors of (X, y, S): err1 = ||A(X) - b||_2 / (1 + ||b||_1), err1_inf = ||.||_inf / (1 + ||b||_inf), err2 = err3 = 0 by
     * construction, err4 = max(0, -min_k lambda_min(S_k)) / (1 + ||C||_1), err5 = (p - d) / (1 + |p| + |d|), err6 = <X, S> / (same) */
    double err1, err1_inf, err2, err3, err4, err5, err6;
    double xs;         /* <X, S> */
    int matvecs;       /* Lanczos S x products */
    double *y;         /* [m] */
    lrd_solution_cone *cone; /* [nblk], file order */
} lrd_solution;
/* fill *out from the session's current state (tol: Lanczos tolerance of lambda_min); refuses (non-zero) when the table lacks the
 * export slots or the session holds a sharded deal.  lrd_solution_free releases what it allocated. */
typedef struct lrd_session lrd_session;
/* what a session holds (session.c): the solver and the table are NULL until a backend has been attached */
lrd_problem *lrd_session_problem(lrd_session *s);
lrd_solver *lrd_session_solver(lrd_session *s);
lrd_backend *lrd_session_backend(lrd_session *s);
/* The way in of every post-solve entry point below.  0: the session can be asked -- *v, *be and *src (the pair the solver's phase
 * works on: LRD_PAIR_UV in ADMM, LRD_PAIR_RR before) are filled (each may be NULL); 1: no solver; 2: the table lacks the slots
 * (have_slots == 0: "lorads: the <name> backend cannot <cannot>" on stderr); 3: the session holds a sharded deal ("lorads: <sharded>
 * not supported"). */
int lrd_session_postsolve(lrd_session *s, int have_slots, const char *cannot, const char *sharded, lrd_solver **v, lrd_backend **be,
                          int *src);
int lrd_session_solution(lrd_session *s, double tol, lrd_solution **out);
void lrd_solution_free(lrd_solution *sol);
/* plain-text file of a solution (a pure function of the struct): "lorads-solution 1", status, pobj, dobj, the certificate, "y m" and
 * m values, then per cone "sdp k n r" and n rows of R, or "lp k n" and n values of x (k: 1-based block of the file); every double %.17g */
int lrd_solution_write(const char *path, const lrd_solution *sol);

/* ---- rounding of +-1-structured contexts (rounding.c).  Everything in the file's units: x = sigma o t
 * is feasible for every sigma (t_p = sqrt(b_i / a_i) of the one constraint a_i X[p,p] = b_i on the diagonal), f = sum_k x_k^T C_k x_k;
 * the dual bound d = b.y + sum_k T_k min(0, lambda_min(S_k)) <= every f (T_k = sum_p t_p^2, the trace of every feasible X_k). */
typedef struct {
    int n, rank;       /* rank: the cone's own current rank (the hyperplanes' dimension) */
    int8_t *sigma;     /* [n] the best trial's signs after the local search */
    double *t, *x;     /* [n] t and x = sigma o t */
    double T;          /* sum_p t_p^2 */
    double lam_min;    /* lambda_min(S_k) (NaN without a bound) */
    double *G;         /* rank x trials (row-major), only when asked for (else NULL) */
} lrd_rounding_cone;
/* what the results of the four roundings (lrd_rounding, lrd_kcut, lrd_stable, lrd_bisection) begin with */
typedef struct {
    int trials, max_rounds, rounds;
    int src;            /* LRD_PAIR_UV or LRD_PAIR_RR: where the factor came from */
    uint64_t seed;
    double scale;       /* scaleObjHis the backend's values were divided by */
    int best, best0;    /* argmin of obj / obj0, lowest index on ties */
    double f_best, f_best0;
    double *obj, *obj0; /* [trials] f after / before the search */
    double by, bound, gap; /* b.y, d, (f_best - d) / max(1, |d|); NaN when tol <= 0 */
    double tol;         /* Lanczos tolerance of lambda_min */
} lrd_round_head;
typedef struct {
    lrd_round_head head;
    int nblk;
    lrd_rounding_cone *cone; /* [nblk], file order; the LP block of a cut-tightened problem (section 20) is an empty cone, n = 0 */
    /* a cut-tightened problem: the bound has the k-cut's LP term, d = ... + sum_j u_j min(0, s_j) over the slack columns */
    int nlp, lp_neg;         /* LP columns; how many of their dual slacks were negative (as lrd_kcut) */
    double *lp_upper;        /* [nlp] u_j (NULL without an LP block) */
} lrd_rounding;
/* trials = 0: applicability alone (*out stays NULL).  Returns 2 when the context does not qualify or the table lacks the slot, 3 when
 * it is sharded.  with_hyperplanes: also fill every cone's G. */
int lrd_session_round(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, lrd_rounding **out);
int lrd_session_round_ex(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, int with_hyperplanes,
                         lrd_rounding **out);
void lrd_rounding_free(lrd_rounding *r);
/* plain-text file, a pure function of the struct (rounding.c) */
int lrd_rounding_write(const char *path, const lrd_rounding *r);

/* ---- spectrum and rank reduction of the solution factors (spectral.c).  Per SDP cone the eigenvalues of F^T F
 * (F = (U+V)/2 in phase 2, the phase-1 R otherwise): the non-zero eigenvalues of X = F F^T.
 * The rank rule: max(1, min(cap, #{j : eig[j] > tol eig[0]})) for eig descending of length rl; cap <= 0: no cap. */
int lrd_spectral_choose(const double *eig, int rl, double tol, int cap);
int lrd_session_block_is_lp(lrd_session *s, int k); /* 1: block k of the session is the LP block (it has no factor and no spectrum) */
typedef struct {
    int n, is_lp;
    int rank_before, rank_after; /* LP block: 1, 1 */
    int sweeps;                  /* Jacobi sweeps of the eigen-solve */
    double *eig;                 /* [rank_before] descending (NULL on the LP block) */
    double trace_lost;           /* sum_{j > k} eig_j / sum_j eig_j */
    double frob_lost;            /* predicted ||X - X_k||_F / ||X||_F = (sum_{j > k} eig_j^2 / sum_j eig_j^2)^(1/2) */
} lrd_spectral_cone;
typedef struct {
    int nblk, src;
    double tol;
    int cap;
    double pobj_before, pobj_after; /* <C, X>, file units */
    double err1_before, err1_after; /* ||A(X) - b||_2 / (1 + ||b||_1) */
    lrd_spectral_cone *cone;        /* [nblk], file order */
} lrd_spectral_report;
/* eig: [sum of the SDP cones' ranks] (cone after cone), sweeps: [nblk] (may be NULL).  Returns 2 when the table lacks the slots, 3 on a
 * sharded deal. */
int lrd_session_spectrum(lrd_session *s, double *eig, int *sweeps);
/* spectrum -> ranks by the rule -> compress_rank -> the solver's ranks, constraint values, objective and err1 refreshed.  rank_max is
 * untouched: a later AUG_RANK may grow the cone again.  *report (may be NULL) is the caller's to free with lrd_spectral_report_free. */
int lrd_session_compress(lrd_session *s, double tol, int cap, lrd_spectral_report **report);
/* ranks != NULL: [nblk] ranks given by the caller instead of the rule (the backend refuses what is out of range: nothing changes) */
int lrd_session_compress_ex(lrd_session *s, double tol, int cap, const int *ranks, lrd_spectral_report **report);
void lrd_spectral_report_free(lrd_spectral_report *r);

/* ---- entries of the primal X = F F^T and its products (primal.c).  F = (U+V)/2 in phase 2, the phase-1 R otherwise
 * (as the export chooses).  Both return 2 when the table lacks the slots, 3 on a sharded deal, else the backend's code. */
int lrd_session_primal_entries(lrd_session *s, int blk, int64_t count, const int *row, const int *col, double *val, const double *ref,
                               double *stats);
int lrd_session_primal_apply(lrd_session *s, int blk, int ncols, const double *B, double *Y, double *T);
/* A query file: one `k i j` or `k i j v` per line (block, row, column 1-based as in .dat-s; v a reference value), every line with v or
 * none; blank lines and lines that start with `*`, `#` or `"` are skipped.  The output file: `lorads-entries 1`, `count N`,
 * `src uv|rr`, `refs 0|1`, with refs `rmse`, `mae`, `maxabs`, `refnorm`, then `k i j x [v]` per query in the query file's order, every
 * double with %.17g. */
typedef struct {
    int64_t count;
    int has_ref, src;           /* src: filled by lrd_session_entries */
    int *blk, *row, *col;       /* [count] 0-based */
    double *ref, *val;          /* [count] (ref: NULL without refs; val: filled by lrd_session_entries) */
    double stats[4];            /* over all queries: sum (x - v)^2, sum |x - v|, max |x - v|, sum v^2 */
} lrd_entries;
/* 0: read; 1: the file cannot be opened; 2: malformed (*bad_line, may be NULL, gets the 1-based line number) */
int lrd_entries_read(const char *path, lrd_entries **out, int *bad_line);
int lrd_entries_write(const char *path, const lrd_entries *q);
void lrd_entries_free(lrd_entries *q);
/* perm [count]: the queries' indices ordered by block, file order kept inside a block; start [nblk + 1]: block k's run of perm */
int lrd_entries_group(const lrd_entries *q, int nblk, int64_t *perm, int64_t *start);
/* the values of all queries: grouped per block for the backend's calls, the file order restored.  1: a block index out of range, else
 * as lrd_session_primal_entries */
int lrd_session_entries(lrd_session *s, lrd_entries *q);

/* ---- the k best entries per row of the primal X (topk.c).  The backend's slot with the session's F, plus
 * skip_constrained: for query row p every column q at which some constraint matrix of the cone stores an entry (p, q) or (q, p) is
 * skipped as well (on a completion problem: the observed entries), combined with the caller's own list.  Returns 2 when the table lacks
 * the slot or blk is the LP block, 3 on a sharded deal, else the backend's code (1: a bad argument, in its words). */
int lrd_session_primal_topk(lrd_session *s, int blk, int nq, const int *row, int col_lo, int col_hi, int k, int smallest, int include_diag,
                            const int64_t *skip_ptr, const int *skip_col, int skip_constrained, int *idx, double *val, int *found);
/* A query file: one `blk row lo hi [skip ...]` per line (1-based as in .dat-s, the window lo..hi inclusive, then the columns to skip);
 * blank lines and lines that start with `*`, `#` or `"` are skipped.  The output file: `lorads-topk 1`, `count N`, `k K`, `src uv|rr`,
 * `order largest|smallest`, then per query in the query file's order `blk row found` and found lines `col value` (1-based, %.17g). */
typedef struct {
    int count, k, src;          /* src: filled by lrd_session_topk */
    int smallest, include_diag, skip_constrained;
    int *blk, *row, *lo, *hi;   /* [count] 0-based, the window [lo, hi) */
    int64_t *skip_ptr;          /* [count + 1] */
    int *skip_col;              /* 0-based */
    int *found, *idx;           /* [count], [count * k] 0-based (filled by lrd_session_topk) */
    double *val;                /* [count * k] */
} lrd_topk;
/* 0: read; 1: the file cannot be opened; 2: malformed (*bad_line, may be NULL, gets the 1-based line number) */
int lrd_topk_read(const char *path, lrd_topk **out, int *bad_line);
int lrd_topk_write(const char *path, const lrd_topk *q);
void lrd_topk_free(lrd_topk *q);
/* all queries of the struct: one call per (block, window), the file order restored */
int lrd_session_topk(lrd_session *s, lrd_topk *q);

/* ---- triangle inequalities of +-1-structured problems (cuts.c).  With rho_xy = X_xy / (t_x t_y) (t as the
 * rounding's) every triple p < q < s of a cone has four inequalities sign . (rho_pq, rho_ps, rho_qs) >= -1, class 0..3 with the signs
 * (+,+,+), (+,-,-), (-,+,-), (-,-,+); v = -1 - lhs > 0 is a violation. */
typedef struct {
    int nblk, src;              /* src: LRD_PAIR_UV or LRD_PAIR_RR, where F came from */
    double min_violation;
    int max_cuts;
    int64_t *count;             /* [nblk] pairs (triple, class) with v > min_violation per cone, exact */
    int kept, passes;           /* cuts listed (<= max_cuts in total); enumeration passes of all cones */
    int *cone, *p, *q, *s;      /* [kept] 0-based, ordered by (v descending, cone, p, q, s, class ascending) */
    int8_t *cls;
    double *viol;
} lrd_cuts;
/* F = (U+V)/2 in phase 2, the phase-1 R otherwise; the slot once per SDP cone, the cones' lists merged.  Returns 2 when the table
 * lacks the slot or the context is not +-1-structured, 3 on a sharded deal, else the backend's code. */
int lrd_session_triangle_cuts(lrd_session *s, double min_violation, int max_cuts, lrd_cuts **out);
void lrd_cuts_free(lrd_cuts *c);
/* The problem of the session as it was read (m, blocks, b, every stored entry; doubles %.17g) in SDPA sparse format plus, per cut e,
 * constraint m + 1 + e: the three entries sign / (2 t_x t_y) in the cut's cone (an off-diagonal entry counts twice in <A, X>), -1 in
 * column e of a new last LP block of dimension -(cuts), b = -1.  Only kept, cone, p, q, s and cls of `cuts` are read; NULL or no cuts
 * writes the problem alone.  A pure function of the problem image and the list.  1: cannot write; 2: a cut outside the problem or a
 * problem with an LP block; 3: sharded. */
int lrd_session_write_tightened(lrd_session *s, const char *path, const lrd_cuts *cuts);
/* The cut-tightened +-1 structure (the rule: include/lorads_cut_rows.h, the device check's own).  The cuts a
 * problem with one LP block holds, in constraint order: triple, class, constraint and LP column (0-based), scale = -b / c (1 as
 * written: the slack x_j / scale = 1 + sum_w sign_w rho_w), and t of all blocks, stacked (zero on the LP block).  A problem without an
 * LP block: n = 0, lpk = -1, t NULL. */
typedef struct {
    int n, lpk;
    int *cone, *p, *q, *s, *cls, *row, *col;
    double *scale, *t;
} lrd_present;
/* 0; 2: the LP block's columns are not all triangle-cut slacks (the first reason: lrd_cuts_why()); 3: sharded */
int lrd_session_present_cuts(lrd_session *s, lrd_present **out);
void lrd_present_free(lrd_present *c);
/* the reason of the last refusal (rc 2) of lrd_session_present_cuts and lrd_session_write_tightened_keep */
const char *lrd_cuts_why(void);
/* lrd_session_write_tightened that also takes a cut-tightened problem: the new cuts follow as constraints m + 1 ... and as columns of
 * the LP block behind its own, the block stays where it is.  keep (NULL: all; else [nkeep], nkeep = the present cuts' number, in
 * lrd_session_present_cuts' order): a present cut with keep[e] = 0 leaves with its constraint and its column, the others are renumbered
 * in order.  A problem without an LP block takes no mask and gives lrd_session_write_tightened's bytes.  2 as well: a new cut that is
 * already in the problem or listed twice, an LP block that is not all cut slacks. */
int lrd_session_write_tightened_keep(lrd_session *s, const char *path, const lrd_cuts *cuts, const unsigned char *keep, int nkeep);
/* ... with the mask from the session's current point (lrd_session_solution at Lanczos tolerance tol): a present cut leaves when its
 * slack x_j / scale_j = 1 + sum_w sign_w rho_w exceeds drop_slack.  *dropped (may be NULL): how many left. */
int lrd_session_write_tightened_drop(lrd_session *s, const char *path, const lrd_cuts *cuts, double drop_slack, double tol, int *dropped);

/* ---- entry bounds on the primal X (bounds.c).  Every pair p < q of an SDP cone has two inequalities: class 0,
 * X_pq >= lower with v = lower - X_pq, and class 1, X_pq <= upper with v = X_pq - upper; v > min_violation is a violation. */
typedef struct {
    int nblk, src;              /* src: LRD_PAIR_UV or LRD_PAIR_RR, where F came from */
    double lower, upper, min_violation;
    int max_cuts;
    int64_t *count;             /* [nblk] (pair, class) with v > min_violation per cone, exact (LP block: 0) */
    int kept, passes;           /* cuts listed (<= max_cuts in total); enumeration passes of all cones */
    int *cone, *p, *q;          /* [kept] 0-based, ordered by (v descending, cone, p, q, class ascending) */
    int8_t *cls;
    double *viol;
    double *bound;              /* [kept] the cut's own bound (lower for class 0, upper for class 1): lists of calls with different
                                 * bounds can be concatenated */
} lrd_bounds;
/* F = (U+V)/2 in phase 2, the phase-1 R otherwise; the slot once per SDP cone (LP blocks are passed over), the cones' lists merged.
 * Returns 2 when the table lacks the slot, 3 on a sharded deal, else the backend's code. */
int lrd_session_entry_bounds(lrd_session *s, double lower, double upper, double min_violation, int max_cuts, lrd_bounds **out);
void lrd_bounds_free(lrd_bounds *c);
/* The problem of the session as it was read (m, blocks, b, every stored entry; doubles %.17g, F0 = -C) in SDPA sparse format plus, per
 * cut e, constraint m + 1 + e: 0.5 at (p, q) of the cut's cone (an off-diagonal entry counts twice in <A, X>) and one slack column,
 * class 0: -1 with b = bound, class 1: +1 with b = bound.  The slack columns form a new last LP block when the problem has none and
 * are appended to the LP block (which keeps its position and its columns their indices) when it has one.  Only kept, cone, p, q, cls and
 * bound of `bounds` are read; NULL or no cuts writes the problem alone.  A pure function of the problem image and the list.
 * 1: cannot write; 2: a cut outside the problem (p >= q, a cone out of range or an LP block, a class outside {0, 1}, a bound that is
 * not finite) or a problem with more than one LP block; 3: sharded. */
int lrd_session_write_bounded(lrd_session *s, const char *path, const lrd_bounds *bounds);

/* ---- rounding into k parts (kcut.c).  Everything in the file's units.  A k-cut-structured problem fixes every
 * diagonal (t_p as the +-1 rounding's) and may bound off-diagonal entries through rows 2 a X_pq + c x_j = b with one LP column each.
 * X(l)_pq = t_p t_q (l_p = l_q), -t_p t_q / (parts - 1) (otherwise); f = sum_k <C_k, X(l_k)>; the dual bound
 * d = b.y + sum_k T_k min(0, lambda_min(S_k)) + sum_j u_j min(0, s_j) <= the optimum <= f(l) for every l whose X(l) is feasible. */
typedef struct {
    int blk;           /* the cone's block in the file, 0-based */
    int n, rank;       /* rank: the cone's own current rank (the vectors' dimension) */
    uint8_t *label;    /* [n] the best trial's labels after the local search */
    double *t;         /* [n] */
    int *size;         /* [parts] vertices per part */
    double T;          /* sum_p t_p^2 */
    double lam_min;    /* lambda_min(S_k) (NaN without a bound) */
    double *G;         /* parts x rank x trials (part, then column, then trial), only when asked for (else NULL) */
} lrd_kcut_cone;
typedef struct {
    lrd_round_head head;
    int nblk;           /* SDP cones */
    int parts;
    int nlp, lp_neg;    /* LP columns; how many of them have a dual slack s_j < 0 (0 without a bound) */
    double *lp_upper;   /* [nlp] u_j */
    lrd_kcut_cone *cone; /* [nblk], file order */
} lrd_kcut;
/* trials = 0: applicability alone (*out stays NULL).  Returns 1 on a bad argument, 2 when the context does not qualify or the table
 * lacks the slot, 3 when it is sharded.  with_vectors: also fill every cone's G. */
int lrd_session_kcut(lrd_session *s, int parts, int trials, uint64_t seed, int max_rounds, double tol, int with_vectors, lrd_kcut **out);
void lrd_kcut_free(lrd_kcut *r);
/* plain-text file, a pure function of the struct (kcut.c) */
int lrd_kcut_write(const char *path, const lrd_kcut *r);

/* ---- stable sets of theta-structured problems (stable.c).  Everything in the file's units.  Every SDP cone has
 * one trace row a tr(X_k) = b (T_k = b / a) and edge rows X_pq = 0, the cone's graph; LP columns only in bound rows as above.  For a
 * stable set S of the graph X(S) = T_k 1_S 1_S^T / |S| is feasible; f = sum_k <C_k, X(S_k)> (the theta files: -|S|); the dual bound
 * d = b.y + sum_k T_k min(0, lambda_min(S_k)) + sum_j u_j min(0, s_j) <= the optimum <= f. */
typedef struct {
    int blk;           /* the cone's block in the file, 0-based */
    int n, rank;       /* rank: the cone's own current rank (the directions' dimension) */
    int size;          /* |S| of the best trial after the search */
    int *member;       /* [size] the set, 0-based, ascending */
    int *sizes;        /* [trials] |S| of every trial after the search */
    double T;
    double lam_min;    /* lambda_min(S_k) (NaN without a bound) */
    double *scores;    /* trials x n priorities (trial, then vertex) in the backend's terms, only when asked for (else NULL) */
} lrd_stable_cone;
typedef struct {
    lrd_round_head head; /* (obj0: f of the greedy sets) */
    int nblk;           /* SDP cones */
    int nlp, lp_neg;    /* LP columns; how many of them have a dual slack s_j < 0 (0 without a bound) */
    double *lp_upper;   /* [nlp] u_j */
    lrd_stable_cone *cone; /* [nblk], file order */
} lrd_stable;
/* trials = 0: applicability alone (*out stays NULL).  Returns 1 on a bad argument, 2 when the context does not qualify or the table
 * lacks the slot, 3 when it is sharded.  with_scores: also fill every cone's scores. */
int lrd_session_round_stable(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, int with_scores, lrd_stable **out);
void lrd_stable_free(lrd_stable *r);
/* plain-text file, a pure function of the struct (stable.c) */
int lrd_stable_write(const char *path, const lrd_stable *r);

/* ---- balanced partitions of bisection-structured problems (bisect.c).  Everything in the file's units.  Every
 * cone has the +-1 diagonal rows with one value t of sqrt(b_i / a_i) and one sum row a <11^T, X_k> = b with b / (a t^2) = d^2: for
 * signs with sum(sigma) = +-d the point x = t sigma is feasible, the parts have (n + d) / 2 and (n - d) / 2 vertices, and
 * f = sum_k x_k^T C_k x_k; the dual bound d = b.y + sum_k n_k t_k^2 min(0, lambda_min(S_k)) <= the optimum <= f. */
typedef struct {
    int n, rank;       /* rank: the cone's own current rank (the hyperplanes' dimension) */
    int diff;          /* d_k */
    int plus, minus;   /* vertices with sigma = +1 / -1 in the best trial: (n + d) / 2 and (n - d) / 2 in either order */
    int8_t *sigma;     /* [n] the best trial's signs after the search */
    int *imbalance;    /* [trials] sum of the hyperplane's signs, before the repair */
    double t;
    double lam_min;    /* lambda_min(S_k) (NaN without a bound) */
    double *G;         /* rank x trials hyperplanes, only when asked for (else NULL) */
} lrd_bisection_cone;
typedef struct {
    lrd_round_head head; /* (obj0: f after the repair) */
    int nblk;           /* cones */
    lrd_bisection_cone *cone; /* [nblk], file order */
} lrd_bisection;
/* trials = 0: applicability alone (*out stays NULL).  Returns 1 on a bad argument, 2 when the context does not qualify or the table
 * lacks the slot, 3 when it is sharded.  with_hyperplanes: also fill every cone's G. */
int lrd_session_round_bisect(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, int with_hyperplanes,
                             lrd_bisection **out);
void lrd_bisection_free(lrd_bisection *r);
/* plain-text file, a pure function of the struct (bisect.c) */
int lrd_bisection_write(const char *path, const lrd_bisection *r);

/* ---- internal: what the post-solve drivers and writers above share (not part of the interface)
 * A list of cuts is kept as ncol parallel columns; a column names the list's own pointer field (`field`: its address) and the size of
 * an element.  Two adjacent runs [0, at) and [at, at + got) of the list, each sorted by `before(list, a, b)` (is entry a before entry
 * b?): merged in place, the first min(at + got, max_cuts) entries kept; returns how many (separation.c). */
typedef struct { void *field; size_t size; } lrd_column;
int lrd_merge_runs(const void *list, int (*before)(const void *list, int a, int b), const lrd_column *col, int ncol, int at, int got,
                   int max_cuts);
/* One separation of the current point (separation.c): the post-solve gate in the feature's words (have_slot, cannot), nblk, src and a
 * zeroed count [nblk] into the list, 2 max_cuts elements per column (the merged list and one cone's list behind it), then `cone` once
 * per SDP cone k -- the feature's table slot with the columns from `at` on, *count, *got and *np as the slot gives them -- col[0] (the
 * cone, int) filled in and the runs merged by `before` into kept, passes summed.  lone_lp: an LP block that is the problem's only
 * block gets the call too.  Non-zero: the gate's or the slot's code; the caller frees its list. */
typedef struct {
    void *list;
    int (*before)(const void *list, int a, int b);
    int (*cone)(lrd_backend *be, void *list, int src, int k, int at, int64_t *count, int *got, int *np);
    int *nblk, *src, *kept, *passes;
    int64_t **count;
    int ncol;
    lrd_column col[6];
} lrd_separation;
int lrd_session_separate(lrd_session *s, int have_slot, const char *cannot, int lone_lp, int max_cuts, const lrd_separation *sp);
/* The problem image in SDPA sparse format (m, blocks, b, every stored entry; doubles %.17g; lower triangle inside, upper triangle
 * i <= j in the file; F0 = -C), extended by x (NULL: as it was read): the rows with drop_row[i] != 0 (may be NULL, else [m]) and the
 * columns with drop_col[j] != 0 of the LP block (likewise) leave and the others are renumbered in order; new row e follows as
 * constraint (rows that stay) + 1 + e with right-hand side rhs, its entries value at (i, j), i <= j, of SDP cone `cone` as given
 * (0-based), and `slack` in a column of its own: behind the LP block's columns that stay, or in a new last LP block where the problem
 * has none.  Opens path first: the caller has validated.  1: cannot write (separation.c). */
typedef struct {
    double rhs, slack;
    int nent;
    struct { int cone, i, j; double value; } ent[3];
} lrd_new_row;
typedef struct {
    int nrow;
    const lrd_new_row *row;
    const unsigned char *drop_row, *drop_col;
} lrd_extension;
int lrd_write_extended(const char *path, const lrd_problem *pr, const lrd_extension *x);
/* The dual bound of a rounding, d = b.y + sum_i T_i min(0, lambda_min(S_blk[i])) + sum_j u_j min(0, s_j), from the certificate's y and
 * eigenvalues at Lanczos tolerance tol and the dual slack of the LP block lpk (-1: none, no third sum); sc: scaleObjHis.  Fills *out
 * (gap = (f_best - d) / max(1, |d|); lp_neg: how many s_j < 0) and lam_min [ncone]; all NaN / 0 when tol <= 0 or the table lacks the
 * slots.  Non-zero: the backend failed (rounding.c). */
typedef struct { double by, bound, gap; int lp_neg; } lrd_dual_bound;
int lrd_rounded_dual_bound(lrd_backend *be, int src, double tol, double sc, int nblk, int ncone, const int *blk, const double *T, int lpk,
                           int nlp, const double *lp_upper, double f_best, lrd_dual_bound *out, double *lam_min);
/* What the four roundings' drivers and writers do with their lrd_round_head (rounding.c).  lrd_zalloc: calloc of at least one element.
 * lrd_round_begin: lrd_session_postsolve in a rounding's words (have_slot: the table has the feature's slot; cannot: what it cannot do
 * without).  _init: the call's arguments and zeroed obj, obj0; _scale: both divided by scale, f_best and f_best0 picked; _bound:
 * lrd_rounded_dual_bound at the head's src, tol, scale and f_best into by, bound, gap, *lp_neg (may be NULL) and lam_min; _free: obj and
 * obj0.  _write: opens path and writes "<magic>\n", the integer lines -- `first` (lines of the feature's own, may be NULL), trials
 * .. best0, `last` -- and the seven %.17g lines scale .. tol; the open file, or NULL where it cannot be opened. */
void *lrd_zalloc(size_t n, size_t size);
int lrd_round_begin(lrd_session *s, int have_slot, const char *cannot, lrd_solver **v, lrd_backend **be, int *src);
void lrd_round_head_init(lrd_round_head *h, int trials, uint64_t seed, int max_rounds, int src, double scale, double tol);
void lrd_round_head_scale(lrd_round_head *h);
int lrd_round_head_bound(lrd_round_head *h, lrd_backend *be, int nblk, int ncone, const int *blk, const double *T, int lpk, int nlp,
                         const double *lp_upper, int *lp_neg, double *lam_min);
void lrd_round_head_free(lrd_round_head *h);
FILE *lrd_round_head_write(const char *path, const char *magic, const lrd_round_head *h, const char *first, const char *last);

/* scalar helpers of the line search (lorads_alm.c:102-228) */
int lrd_cubic_roots(double a, double b, double c, double d, double res[3]);
int lrd_linesearch_tau(const double coef[4], double *tau);
double lrd_time(void);

#ifdef __cplusplus
}
#endif
#endif
