/* lorads_hip.h -- C ABI of the MI355X (gfx950) backend for the LoRADS per-iteration path.
 *
 * Drop-in boundary: the reference reaches every per-iteration step of both phases
 * through its operator table `lorads_func` (src_semi/data/def_lorads_solver.h:109-127, filled by
 * LORADSInitFuncSet, src_semi/data/lorads_solver.c:717-756) plus three non-table calls.  Each entry
 * point below replaces one of those slots; the citation on each names the reference function whose
 * result it reproduces.  The state the reference keeps in `lorads_solver`/`lorads_variable`
 * (R, U, V, Grad, dualVar, constrVal[], constrValSum, ARDSum, ADDSum, L-BFGS ring, CG workspaces,
 * src_semi/data/def_lorads_solver.h:12-106) lives on the device inside the opaque context; the
 * movers at the end upload/download it in the reference's own layout (column-major n x r, ld = n).
 *
 * Plain C: opaque pointer, int32/double pointers and sizes only; every function returns 0 on
 * success and a non-zero code on failure (lorads_hip_last_error gives the text).  One context per
 * process/GPU; calls on one context must be serialised by the caller (as the reference's single
 * thread does).  INTEGRATION.md shows the shim a reference maintainer would add.
 */
#ifndef LORADS_HIP_H
#define LORADS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lorads_hip_ctx lorads_hip_ctx;

/* One SDP cone after the reference's pre-solve, flat (what AConeProcData leaves in
 * lorads_cone_sdp_dense/sparse, src_semi/data/def_lorads_sdp_conic.h:101-127): lower-triangular
 * triplets, CSR by constraint.  Pointers are HOST pointers and are copied. */
typedef struct {
    int32_t n;              /* cone dimension */
    int32_t rank;           /* current factor rank r (LORADSDetermineRank) */
    int32_t nrow;           /* constraints with a non-zero A_i on this cone */
    const int32_t *row_idx; /* [nrow] global constraint index (sparse cone: rowIdx) */
    const int32_t *a_ptr;   /* [nrow+1] */
    const int32_t *a_row;   /* [a_ptr[nrow]] row >= col */
    const int32_t *a_col;
    const double *a_val;
    int32_t c_nnz; /* objective matrix C (sign as stored by the reference: C = -F0) */
    const int32_t *c_row;
    const int32_t *c_col;
    const double *c_val;
    /* 1: this is the LP block of the file (lorads_lp_cone, data/def_lorads_lp_conic.h; at most one, the last block):
     * n = number of LP columns, rank 1, every entry diagonal ((i,i,a) = coefficient a of column i).  Phase 1 and the
     * evaluations treat it as a diagonal cone; admm_update_var updates it column by column in closed form
     * (LORADSUpdateSDPLPVar, lorads_alg_common.c:225-248). */
    int32_t is_lp;
} lorads_hip_block;

typedef struct {
    int32_t m;          /* number of constraints (ASolver->nRows) */
    const double *b;    /* [m] rowRHS */
    double b_nrm1;      /* ||b||_1 (bRHSNrm1) */
    int32_t nblocks;    /* cones held by this context (multi-GPU: a subset) */
    const lorads_hip_block *blocks;
    int32_t lbfgs_len;  /* params->lbfgsListLength */
    int32_t device;     /* HIP device ordinal, -1 = current */
} lorads_hip_problem;

/* sum `count` doubles in place over all ranks; buf is a DEVICE pointer when on_device != 0.  The
 * library synchronises its stream before the call. */
typedef int (*lorads_hip_allreduce_fn)(void *user, double *buf, int32_t count, int32_t on_device);

enum { LORADS_HIP_PAIR_RR = 0, LORADS_HIP_PAIR_UV = 1 };
enum { LORADS_HIP_MAT_R = 0, LORADS_HIP_MAT_U = 1, LORADS_HIP_MAT_V = 2, LORADS_HIP_MAT_GRAD = 3 };
enum { LORADS_HIP_VEC_LAMBDA = 0, LORADS_HIP_VEC_CONSTR_SUM = 1, LORADS_HIP_VEC_Q1 = 2, LORADS_HIP_VEC_Q2 = 3 };

int lorads_hip_create(const lorads_hip_problem *prob, lorads_hip_ctx **out);
void lorads_hip_destroy(lorads_hip_ctx *ctx);
const char *lorads_hip_last_error(void);

/* lorads_func.InitConstrValAll + InitConstrValSum (lorads_alg/lorads_alg_common.c:78-84,134-142):
 * constrVal[k] = A_k(sym(X Y^T)), constrValSum = sum_k; pair RR uses (R,R), pair UV uses (U,V) */
int lorads_hip_init_constr(lorads_hip_ctx *ctx, int32_t pair);
/* lorads_func.ALMCalGrad (lorads_alg/lorads_alm.c:9-54): Grad_k = 2 (C + sum_i M1_i A_i) R_k with
 * M1 = -lambda - rho b + rho constrValSum; *lag_norm_sq = sum_k ||Grad_k||_F^2 */
int lorads_hip_alm_cal_grad(lorads_hip_ctx *ctx, double rho, double *lag_norm_sq);
/* lorads_func.LBFGSDirection + LBFGSDirUseGrad (lorads_alm.c:230-391,469-489); direction D in U */
int lorads_hip_lbfgs_direction(lorads_hip_ctx *ctx, int32_t inner_iter);
/* lorads_func.ALMCalq12p12 (lorads_alm.c:540-560): q1 = 2A(sym(R D^T)), q2 = A(D D^T) stay on the
 * device; p12 = { 2<C,sym(R D^T)>, <C, D D^T> } */
int lorads_hip_alm_q12p12(lorads_hip_ctx *ctx, double p12[2]);
/* vector half of ALMLineSearch (lorads_alm.c:161-172): coefficients a,b,c,d of the quartic in tau;
 * the host solves the cubic (lorads_alm.c:114-154,173-227) */
int lorads_hip_alm_linesearch_coeffs(lorads_hip_ctx *ctx, double rho, double p1, double p2, double coef[4]);
/* lorads_func.setAsNegGrad (lorads_alm.c:583-598) */
int lorads_hip_set_y_as_neg_grad(lorads_hip_ctx *ctx);
/* lorads_func.ALMupdateVar + constrValSum += tau q1 + tau^2 q2 (lorads_alm.c:619-648,1122-1124) */
int lorads_hip_alm_update_var(lorads_hip_ctx *ctx, double tau);
/* lorads_func.setlbfgsHisTwo (lorads_alm.c:657-678) */
int lorads_hip_set_lbfgs_his_two(lorads_hip_ctx *ctx, double tau);
/* lorads_func.updateDimacsALM / updateDimacsADMM (lorads_alg_common.c:250-290): refreshes
 * constrVal/constrValSum from R R^T (pair UV: after R = (U+V)/2) and returns
 * ||b - constrValSum||_2 / (1 + ||b||_1) */
int lorads_hip_update_dimacs(lorads_hip_ctx *ctx, int32_t pair, double *err1);
/* lorads_func.calObj_alm / calObj_admm (lorads_alm.c:1259-1268, lorads_admm.c:325-337): <C, R R^T>
 * summed over this context's cones (pair UV: after R = (U+V)/2); not divided by scaleObjHis */
int lorads_hip_cal_obj(lorads_hip_ctx *ctx, int32_t pair, double *pobj);
/* Fused phase-1 inner iteration (optional; the slot-by-slot calls above give identical results).  The body of
 * the reference's inner loop (lorads_alm.c:1066-1131) is  [direction, q12p12, line-search sums] -> scalar cubic
 * on the host -> [setAsNegGrad, ALMupdateVar(tau), ALMCalGrad, setlbfgsHisTwo, updateDimacsALM].
 *   alm_front: first bracket for inner-iteration counter `inner`; out = {p1, p2, a, b, c, d}
 *   alm_step : second bracket with the host's tau, then (next_inner >= 0) the first bracket of the NEXT iteration,
 *              enqueued back to back with ONE host synchronisation;
 *              out = {lagNormSq, err1, p1, p2, a, b, c, d} (p, a..d belong to the next iteration)
 * If the host leaves the loop instead, the pre-computed direction is discarded (it lives in D = U, q1, q2). */
int lorads_hip_alm_front(lorads_hip_ctx *ctx, double rho, int32_t inner, double out[6]);
int lorads_hip_alm_step(lorads_hip_ctx *ctx, double rho, double tau, int32_t next_inner, double out[8]);
/* lorads_func.admmUpdateVar = LORADSUpdateSDPVar (lorads_alg_common.c:187-215) with
 * LORADSUpdateSDPVarOne (lorads_admm.c:428-480) and CGSolve (linalg/lorads_cgs.c:81-240);
 * *cg_iters = sum of the CG iteration counts the reference would add to ASolver->cgIter */
int lorads_hip_admm_update_var(lorads_hip_ctx *ctx, double rho, double cg_tol, int32_t cg_max_iter,
                               int32_t *cg_iters);
/* One ADMM iteration up to (not including) the dual update, i.e. admmUpdateVar + calObj_admm +
 * LORADSCalDualObj + updateDimacsADMM in the order of lorads_admm.c:76-81, with ONE host
 * synchronisation: out = { cg iterations, <C,RR^T> (unscaled), b.lambda (unscaled), err1 } */
int lorads_hip_admm_step(lorads_hip_ctx *ctx, double rho, double cg_tol, int32_t cg_max_iter, double out[4]);
/* LORADSUpdateDualVar / LORADSCalDualObj (lorads_alg_common.c:319-340) */
int lorads_hip_update_dual_var(lorads_hip_ctx *ctx, double rho);
int lorads_hip_cal_dual_obj(lorads_hip_ctx *ctx, double *dobj);

/* calculate_dual_infeasibility_solver + dual_infeasible (data/lorads_solver.c:1007-1037,
 * data/lorads_sdp_conic.c:1286-1349): *sum_neg = sum over this context's cones of
 * |min(lambda_min(C_k - sum_i lambda_i A_ik), 0)| -- the caller divides by scaleObjHis (1 + ||C||_1) as
 * :1034-1035 do.  tol, ncv, max_restarts are the ARPACK parameters of the reference (1e-2, 40, 600); the
 * eigenvalue comes from an on-device thick-restart Lanczos with the same subspace size and stopping rule.
 * lam_min ([nblocks], may be NULL) receives the per-cone eigenvalue, *matvecs (may be NULL) the S x count. */
int lorads_hip_dual_infeasibility(lorads_hip_ctx *ctx, double tol, int32_t ncv, int32_t max_restarts, double *sum_neg,
                                  double *lam_min, int32_t *matvecs);

/* Solution export (DESIGN.md "Exporting a solution"; no reference counterpart).  The exported point is X_k = R_k R_k^T per SDP cone
 * (x_j = r_j^2 on the LP block), the multipliers lambda -- with a dual update that still waits for a carrier applied to a copy -- and
 * the slack S_k = C_k - sum_i lambda_i A_ik.  src = LORADS_HIP_PAIR_UV takes R = (U + V) / 2 (phase 2), LORADS_HIP_PAIR_RR takes R
 * itself (phase 1).  Neither call writes any state of the solve: the next iteration computes what it would have computed.
 * Values are in device terms like the neighbouring entries (objective, multipliers and slack scaled by scaleObjHis; the caller
 * divides).  Sharded contexts (an all-reduce hook, a separable shard) are refused.
 *   out[0] ||A(X) - b||_2 / (1 + ||b||_1)        out[1] ||A(X) - b||_inf / (1 + ||b||_inf)
 *   out[2] <C, X> (+ c_lp . x)                    out[3] b . lambda
 *   out[4] <X, S> (+ x . s_lp)                    out[5] min over cones of lambda_min(S_k) (LP block: min_j s_j)
 *   out[6] Lanczos matvecs                        out[7] ||A(X) - b||_2   out[8] ||A(X) - b||_inf   out[9] ||b||_inf
 * lam_min ([nblocks], may be NULL) gets the per-cone eigenvalue, residual ([m], may be NULL) A(X) - b.  tol, ncv, max_restarts are
 * the Lanczos parameters of lorads_hip_dual_infeasibility; tol <= 0 skips the eigen-solves (out[5] and lam_min are NaN).
 * lambda ([m], may be NULL) receives the multipliers of the certificate: lorads_hip_get_vec would first store a waiting dual update. */
#define LORADS_HIP_CERT_N 10
int lorads_hip_certificate(lorads_hip_ctx *ctx, int32_t src, double tol, int32_t ncv, int32_t max_restarts,
                           double out[LORADS_HIP_CERT_N], double *lam_min, double *residual, double *lambda);
/* S of cone blk as lower-triangle triplets (row >= col) in device terms: the union pattern's entries (ordered by column, then row);
 * the whole lower triangle on a cone with dense storage; one (j, j) entry per column on the LP block.  NULL arrays: *nnz = the count
 * and nothing else. */
int lorads_hip_get_slack(lorads_hip_ctx *ctx, int32_t blk, int64_t *nnz, int32_t *row, int32_t *col, double *val);

/* Hyperplane rounding of a +-1-structured context (no reference counterpart).  Qualifies: no LP block, every
 * constraint one stored entry a_i X_k[p,p] = b_i with b_i / a_i > 0, every diagonal of every cone fixed by exactly one; then
 * x = sigma o t with t_p = sqrt(b_i / a_i) is feasible for every sigma in {+-1}^n.  Per cone k and trial t a Gaussian g_{k,t} of the
 * cone's own rank (counter-based on (seed, k, t, column)), sigma_p = sign(R_p . g) with R as lorads_hip_certificate takes it (src),
 * f_t = x^T C x, then at most max_rounds rounds of the 1-flip local search by colour classes (0: none).  Values in device terms
 * (C scaled by scaleObjHis).  Read-only on the solver's state; the same state and arguments give the same bits.
 *   obj [trials]            f after the local search        obj0 [trials] (may be NULL)  f before it
 *   best / best0            argmin of obj / obj0 (lowest index on ties; may be NULL)
 *   sign [sum_k n_k]        the best trial's signs (+1 / -1), cone after cone (may be NULL)
 *   rounds                  local-search rounds run (may be NULL)
 *   hyperplanes             per cone rank_k x trials (row-major: column j of cone k, then trial), cone after cone (may be NULL)
 * Also qualifies (the rule: lorads_cut_rows.h): the cut-tightened form of such a context -- one LP block whose
 * columns are all slacks of triangle rows (what lrd_session_write_tightened writes and its positive multiples).  The LP block has no
 * signs (zeros in `sign`) and no hyperplanes; the local search colours the union pattern, cut positions included.
 * trials = 0 checks applicability only.  1 <= trials <= 65536.  Returns 2 when the context does not qualify (lorads_hip_last_error
 * names the first offending constraint, cone or LP column), 3 when it is sharded. */
int lorads_hip_round_pm1(lorads_hip_ctx *ctx, int32_t src, int32_t trials, uint64_t seed, int32_t max_rounds, double *obj,
                         double *obj0, int32_t *best, int32_t *best0, int8_t *sign, int32_t *rounds, double *hyperplanes);

/* Frieze-Jerrum rounding of a k-cut-structured context into `parts` parts, with a 1-move local search (no
 * reference counterpart).  Qualifies: at least one SDP cone, at most one LP block, no dense constraint matrices; every constraint
 * without an LP entry one stored entry a_i X_k[p,p] = b_i with b_i / a_i > 0, every diagonal of every cone fixed by exactly one
 * (t_p = sqrt(b_i / a_i)); every constraint with an LP entry a bound row 2 a X_pq + c x_j = b: one off-diagonal cone entry and one LP
 * column, which occurs in no other constraint and has no objective coefficient (what lrd_session_write_bounded writes).  Without an LP
 * block that is lorads_hip_round_pm1's rule.  For labels l_p in {0 .. parts-1} the point X(l)_pq = t_p t_q where l_p = l_q and
 * -t_p t_q / (parts - 1) elsewhere is PSD and meets every diagonal constraint; it meets a bound row X_pq >= lower when
 * lower <= -t_p t_q / (parts - 1).  Per cone k, trial t and part a a Gaussian g of the cone's own rank, lorads_hip_round_pm1's generator
 * at the counter (k << 32) | (a << 26) | (t << 10) | column (part 0 is that call's hyperplane); l_p = the lowest a that attains
 * max_a R_p . g_a, every score one chain of FP64 matrix-core steps over the columns in fours; f_t = sum_k <C_k, X(l_k)>; then at most
 * max_rounds rounds of the 1-move local search by colour classes (0: none).  Values in device terms (C scaled by scaleObjHis).
 * Read-only on the solver's state; the same state and arguments give the same bits.
 *   obj [trials]            f after the local search        obj0 [trials] (may be NULL)  f before it
 *   best / best0            argmin of obj / obj0 (lowest index on ties; may be NULL)
 *   label [sum_k n_k]       the best trial's labels, SDP cone after SDP cone (may be NULL)
 *   rounds                  local-search rounds run (may be NULL)
 *   vectors                 per SDP cone parts x rank_k x trials (part, then column, then trial), cone after cone (may be NULL)
 *   t [sum_k n_k]           t_p, SDP cone after SDP cone (may be NULL)
 *   lp_upper [LP columns]   u_j = (|b| + 2 |a| t_p t_q) / |c| of the column's row: x_j <= u_j at every feasible point (may be NULL)
 * trials = 0 checks applicability only (t and lp_upper are still filled).  Returns 1 on a bad argument (src, parts outside [2, 64],
 * trials outside [0, 65536], trials x parts above 2^20, max_rounds < 0, obj NULL with trials > 0) or a failed allocation (the context
 * stays usable), 2 when the context does not qualify (lorads_hip_last_error names the first offending constraint, cone or column),
 * 3 when it is sharded -- all before any device work. */
int lorads_hip_round_kcut(lorads_hip_ctx *ctx, int32_t src, int32_t parts, int32_t trials, uint64_t seed, int32_t max_rounds,
                          double *obj, double *obj0, int32_t *best, int32_t *best0, uint8_t *label, int32_t *rounds, double *vectors,
                          double *t, double *lp_upper);

/* Stable sets read off the factors of a theta-structured context, with a (1, 2)-swap search (no reference
 * counterpart).  Qualifies: at least one SDP cone, at most one LP block, no dense constraint matrices; per SDP cone exactly one trace
 * row -- a I over all n rows with a > 0 and b > 0, touching no other cone: T_k = b / a; every other constraint without an LP entry an
 * edge row: one off-diagonal entry (p, q) of one cone, b = 0 (the edge rows are the cone's graph G_k); every constraint with an LP
 * entry a bound row as lorads_hip_round_kcut takes it.  C is arbitrary.  For a stable set S of G_k the point X(S) = T_k 1_S 1_S^T / |S|
 * is feasible; f_k = <C_k, X(S)> (the theta files: -|S|).  Per cone k and trial t a priority per vertex: trial 0 takes |F_p|^2, trial
 * t >= 1 takes F_p . g_t with g_t lorads_hip_round_pm1's hyperplane t of that seed and F the factor lorads_hip_certificate takes (src),
 * the projections one product on the FP64 matrix cores.  The trial's set is the lexicographically first maximal stable set in the
 * order (priority descending, index ascending); then at most max_rounds rounds of the (1, 2)-swap search (0: none): the member of
 * least index that has two non-adjacent neighbours with no other member next to them leaves, the lexicographically first such pair
 * joins, and the vertices left without a member next to them are completed greedily in the trial's order; the round that finds no
 * such member is the last and is counted.  One workgroup owns one trial.  Values in device terms (C scaled by scaleObjHis).
 * Read-only on the solver's state; the same state and arguments give the same bits.
 *   obj [trials]            sum_k f_k after the search       obj0 [trials] (may be NULL)  of the greedy sets
 *   best / best0            argmin of obj / obj0 (lowest index on ties; may be NULL)
 *   member [sum_k n_k]      the best trial's sets after the search, 1: in the set, SDP cone after SDP cone (may be NULL)
 *   sizes [cones x trials]  |S| after the search, cone after cone, per trial (may be NULL)
 *   rounds                  the largest number of search rounds a trial ran (may be NULL)
 *   scores                  per SDP cone trials x n_k priorities (trial, then vertex), cone after cone (may be NULL)
 *   T [cones + LP columns]  T_k of the SDP cones, then u_j = (|2 a| T_k / 2 + |b|) / |c| of the LP columns' bound rows: x_j <= u_j at
 *                           every feasible point, since |X_pq| <= (X_pp + X_qq) / 2 <= T_k / 2 (may be NULL)
 * trials = 0 checks applicability only (T is still filled).  There is no limit on n or on a vertex's degree.  Returns 1 on a bad
 * argument (src, trials outside [0, 65536], max_rounds < 0, obj NULL with trials > 0) or a failed allocation (the context stays
 * usable), 2 when the context does not qualify (lorads_hip_last_error names the first offending constraint, cone or column), 3 when
 * it is sharded -- all before any device work. */
int lorads_hip_round_stable(lorads_hip_ctx *ctx, int32_t src, int32_t trials, uint64_t seed, int32_t max_rounds, double *obj,
                            double *obj0, int32_t *best, int32_t *best0, uint8_t *member, int32_t *sizes, int32_t *rounds,
                            double *scores, double *T);

/* Balanced partitions read off the factors of a bisection-structured context, with a repair step and a swap search (DESIGN.md section
 * 19; no reference counterpart).  Qualifies: no LP block; per cone k the diagonal rows of lorads_hip_round_pm1 -- one a_i X_k[p,p] = b_i
 * with b_i / a_i > 0 per diagonal position --, all t_p = sqrt(b_i / a_i) bit-equal (t_k), and exactly one sum row: every position of
 * the cone's lower triangle, all values bit-equal to one a != 0, no entry on another cone, and |q - d_k^2| <= 1e-9 max(1, q) for
 * q = b / (a t_k^2) and an integer 0 <= d_k <= n_k with d_k = n_k (mod 2).  The sum row may sit in the sparse structures or in the dense
 * store.  C is arbitrary.  x = t_k sigma with sum(sigma) = +-d_k is feasible; f = sum_k x_k^T C_k x_k.  Per cone k and trial t:
 *   signs    lorads_hip_round_pm1's hyperplane t of that seed and its sign bits; D = sum_p sigma_p
 *   repair   |D - target| / 2 flips, target = +d_k where D >= 0, else -d_k: each flips the vertex of least Delta_p = -4 x_p h_p on the
 *            side in excess (h_p = sum_{q != p} C_pq x_q over p's stored row list in its stored order), the lowest index on ties
 *   search   at most max_rounds rounds (0: none).  Order A: p = argmin over sigma = +1 of Delta_p, q = argmin over sigma = -1 of
 *            Delta_q + 8 C_pq x_p x_q, Delta_A their sum; order B the same from the -1 side; the round takes A unless Delta_B < Delta_A
 *            and swaps the pair where Delta < -2^-40 (tau_p + tau_q), tau_p = 4 t_k^2 sum_{q != p} |C_pq|.  A round that does not swap
 *            is the last and is counted.  sum(sigma) is untouched and every swap lowers f by exactly its Delta.
 * One workgroup owns one (cone, trial); the result of a trial does not depend on `trials`.  Values in device terms (C scaled by
 * scaleObjHis).  Read-only on the solver's state; the same state and arguments give the same bits.
 *   obj [trials]               f after the search          obj0 [trials] (may be NULL)  f after the repair
 *   best / best0               argmin of obj / obj0 (lowest index on ties; may be NULL)
 *   sign [sum_k n_k]           the best trial's signs after the search, cone after cone (may be NULL)
 *   imbalance [cones x trials] D of the hyperplane's signs, before the repair, cone after cone, per trial (may be NULL)
 *   rounds                     the largest number of search rounds a trial ran on a cone (may be NULL)
 *   hyperplanes                as lorads_hip_round_pm1's (may be NULL)
 *   t [cones], diff [cones]    t_k and d_k (may be NULL)
 * trials = 0 checks applicability only (t and diff are still filled).  Returns 1 on a bad argument (src, trials outside [0, 65536],
 * max_rounds < 0, obj NULL with trials > 0) or a failed allocation (the context stays usable), 2 when the context does not qualify
 * (lorads_hip_last_error names the first offending constraint or cone), 3 when it is sharded -- all before any device work.
 * LORADS_BISECT_LDS=0 at the context's creation keeps a trial's state in device memory at every size (the path of cones too large
 * for the LDS); the results are the same bits. */
int lorads_hip_round_bisect(lorads_hip_ctx *ctx, int32_t src, int32_t trials, uint64_t seed, int32_t max_rounds, double *obj,
                            double *obj0, int32_t *best, int32_t *best0, int8_t *sign, int32_t *imbalance, int32_t *rounds,
                            double *hyperplanes, double *t, int32_t *diff);

/* Spectrum and rank reduction of the solution factors (no reference counterpart).  Per SDP cone k (the LP block
 * has no factor and is passed over) F_k is the factor lorads_hip_certificate takes (src) at the cone's own rank rl_k, G_k = F_k^T F_k =
 * Q_k Lambda_k Q_k^T with lambda_1 >= lambda_2 >= ... (ties: lower original index first): the non-zero eigenvalues of X_k = F_k F_k^T.
 * G on the FP64 matrix cores, the eigen-solve by cyclic Jacobi in the round-robin ordering (one workgroup per cone).
 *   eig    [sum_k rl_k]    eigenvalues, descending per SDP cone, cone after cone
 *   q      (may be NULL)   eigenvectors, column-major rl_k x rl_k per SDP cone, cone after cone
 *   sweeps [nblocks] (may be NULL)  Jacobi sweeps run per cone, the one that rotated nothing included (LP block: 0)
 * lorads_hip_spectrum is read-only on the solver's state; the same state gives the same bits.  Returns 3 on a sharded context, 4 when a
 * cone's iteration still rotates after 30 sweeps or its factor holds a value that is not finite (lorads_hip_last_error names it).
 * lorads_hip_compress_rank replaces every factor by F_k Q_k[:, :new_rank[k]] -- the best approximation of X_k at that rank; mutually
 * orthogonal columns of squared norms lambda_1.. -- written to R, U and V alike (Grad and the L-BFGS history cleared):
 * 1 <= new_rank[k] <= rl_k (LP block: 1); anything else, a sharded context (3) or an eigen-solve that fails (4) is refused with host
 * and device at the old ranks and the old bits.  new_rank[k] = rl_k is a pure rotation.  eig (may be NULL) as above, of the factor
 * before the reduction.  Constraint values are the caller's to refresh (lorads_hip_init_constr), as after lorads_hip_resize_rank. */
int lorads_hip_spectrum(lorads_hip_ctx *ctx, int32_t src, double *eig, double *q, int32_t *sweeps);
int lorads_hip_compress_rank(lorads_hip_ctx *ctx, int32_t src, const int32_t *new_rank, double *eig);

/* Entries of the primal and its products with a block of vectors (no reference counterpart).  X_blk = F F^T with F
 * the factor lorads_hip_certificate takes (src) at the cone's own rank, in the file's units (X carries no scaleObjHis); on the LP block
 * X = diag(f_j^2).  X is never formed.
 *   primal_entries: val[e] = F_row[e] . F_col[e] (LP block: f_i^2 where row = col, else 0); positions 0-based, in any order, duplicates
 *     allowed; val(i, j) and val(j, i) are the same bits.  With ref the device also forms stats = { sum (val - ref)^2, sum |val - ref|,
 *     max |val - ref|, sum ref^2 }: a held-out score needs no read-back of val (val may then be NULL).  stats is given with ref and only
 *     with it.  count = 0: nothing is launched, the statistics are zero.  The positions go to the device in chunks of
 *     LORADS_HIP_PRIMAL_CHUNK entries; a workgroup takes LORADS_HIP_PRIMAL_EPW of them.
 *   primal_apply: T = F^T B (rl x ncols, may be NULL), Y = F T = X_blk B; B, Y column-major n x ncols on the host, 1 <= ncols <= 1024;
 *     on the FP64 matrix cores, in panels of 16 columns.  A column of Y does not depend on which other columns share the call.
 *     LP block: Y = diag(f^2) B and T must be NULL.
 * Both are read-only on the solver's state and deterministic (no float atomics; the same state and arguments give the same bits).
 * Everything is validated on the host before any device work -- src, blk, count < 0, ncols, a NULL that is not allowed, every row[e]
 * and col[e] against [0, n) -- and lorads_hip_last_error names the first offending position.  Returns 3 on a sharded context. */
#define LORADS_HIP_PRIMAL_CHUNK 262144
#define LORADS_HIP_PRIMAL_EPW 128
int lorads_hip_primal_entries(lorads_hip_ctx *ctx, int32_t src, int32_t blk, int64_t count, const int32_t *row, const int32_t *col,
                              double *val, const double *ref, double stats[4]);
int lorads_hip_primal_apply(lorads_hip_ctx *ctx, int32_t src, int32_t blk, int32_t ncols, const double *B, double *Y, double *T);

/* Separation of the triangle inequalities of a +-1-structured context (no reference counterpart).  With F the
 * factor lorads_hip_certificate takes (src) of SDP cone blk at its own rank, t as lorads_hip_round_pm1 derives it and
 * rho_xy = (F_x . F_y) / (t_x t_y), every triple p < q < s has four inequalities, class 0..3:
 *     rho_pq + rho_ps + rho_qs >= -1,   rho_pq - rho_ps - rho_qs >= -1,   -rho_pq + rho_ps - rho_qs >= -1,   -rho_pq - rho_ps + rho_qs >= -1
 * and v = -1 - lhs is the violation, evaluated on the device in one fixed order of operations.
 *   count: the exact number of (triple, class) pairs with v > min_violation among all 4 C(n, 3) (X is never formed);
 *   p, q, s, cls, viol [max_cuts]: the *kept = min(count, max_cuts) largest pairs in the total order "v descending, then p, q, s, class
 *     ascending" (0-based rows), written in that order -- exact with respect to the device's v whatever ties at the cut-off;
 *   max_cuts = 0 counts only (the five arrays and kept may then be NULL); passes (may be NULL): enumeration passes that ran.
 * On a cut-tightened context the pairs that are rows of the problem already are neither counted nor listed:
 * count is "violated and not present".
 * Read-only on the solver's state and deterministic (no float atomics; the same state and arguments give the same bits and list).
 * Scratch: the packed factor, max_cuts + 16384 keys rounded up to a power of two, one histogram.
 * Returns 1 on a bad argument (src, blk out of range or the LP block, max_cuts outside [0, 2^20], min_violation negative or not finite,
 * a required array NULL), 3 on a sharded context, 2 with lorads_hip_round_pm1's reason when the context is not +-1-structured -- all
 * before any device work.  n < 3: count 0, nothing is launched. */
int lorads_hip_triangle_cuts(lorads_hip_ctx *ctx, int32_t src, int32_t blk, double min_violation, int32_t max_cuts, int64_t *count,
                             int32_t *p, int32_t *q, int32_t *s, int8_t *cls, double *viol, int32_t *kept, int32_t *passes);

/* Separation of entry bounds on the primal X = F F^T (no reference counterpart).  With F the factor
 * lorads_hip_certificate takes (src) of SDP cone blk at its own rank, every pair p < q has two inequalities:
 *     class 0: X_pq >= lower, v = lower - X_pq        class 1: X_pq <= upper, v = X_pq - upper
 * and v > min_violation is a violation; lower = -inf or upper = +inf switches a class off.  X_pq is one chain of FP64 matrix-core steps
 * over the columns in fours, then one subtraction: |v - exact| <= (r + 2) 2^-53 (|F_p| |F_q| + |bound|).
 *   count: the exact number of (pair, class) with v > min_violation among all n (n - 1) (X is never formed);
 *   p, q, cls, viol [max_cuts]: the *kept = min(count, max_cuts) largest in the total order "v descending, then p, q, class ascending"
 *     (0-based rows), written in that order -- exact with respect to the device's v whatever ties at the cut-off;
 *   max_cuts = 0 counts only (the four arrays and kept may then be NULL); passes (may be NULL): enumeration passes that ran.
 * Any SDP cone of any context; read-only on the solver's state and deterministic (no float atomics).
 * Scratch: the packed factor, max_cuts + 16384 keys rounded up to a power of two, one histogram.
 * Returns 1 on a bad argument (src, blk out of range or the LP block, max_cuts outside [0, 2^20], min_violation negative or not finite,
 * a NaN bound, lower > upper, both classes off, a required array NULL, n above 2^24), 3 on a sharded context -- all before any device
 * work.  n < 2: count 0, nothing is launched. */
int lorads_hip_entry_bounds(lorads_hip_ctx *ctx, int32_t src, int32_t blk, double lower, double upper, double min_violation,
                            int32_t max_cuts, int64_t *count, int32_t *p, int32_t *q, int8_t *cls, double *viol, int32_t *kept,
                            int32_t *passes);

/* The k best entries per row of the primal X = F F^T (no reference counterpart).  With F the factor
 * lorads_hip_certificate takes (src) of SDP cone blk at its own rank, X_pq = F_p . F_q: one chain of FP64 matrix-core steps over the
 * columns in fours, ascending (|X_pq - exact| <= (r + 1) 2^-53 |F_p| |F_q|); its bits depend on the two rows alone.
 *   row [nq]: the query rows, 0-based, any order, duplicates allowed.
 *   Candidates of query i (p = row[i]): the columns q of the window [col_lo, col_hi), minus q = p unless include_diag, minus
 *     skip_col[skip_ptr[i] .. skip_ptr[i + 1]) (any order, duplicates and columns outside the window allowed; both NULL: none), minus
 *     every q whose X_pq is NaN.  +-inf order as numbers.
 *   Order: X_pq descending (smallest = 1: ascending), then q ascending; -0.0 and +0.0 are one value.
 *   found [nq] = min(k, candidates); idx, val [nq * k]: the first found[i] candidates of query i in the order at i * k ..., the
 *     device's own bits of X_pq; the slots past found[i] hold idx -1 and val 0.0.
 * 1 <= k <= 128.  nq = 0 or an empty window: found all zero, nothing is launched.  Read-only on the solver's state and deterministic (no
 * float atomics; the same state and arguments give the same bytes).  Scratch: the packed factor and, per batch of at most 16384
 * queries, the packed query rows, the results and the partial lists of a split window -- bounded whatever nq is.
 * Returns 1 on a bad argument (src, blk, nq < 0, a row outside [0, n), a window not within 0 <= lo <= hi <= n, k outside [1, 128],
 * smallest or include_diag not 0 or 1, exactly one skip pointer NULL, skip_ptr not starting at 0 or decreasing, a skip column outside
 * [0, n), idx, val or found NULL with nq > 0) or a failed allocation (the context stays usable), 2 on the LP block, 3 on a sharded
 * context -- all refusals before any device work. */
int lorads_hip_primal_topk(lorads_hip_ctx *ctx, int32_t src, int32_t blk, int32_t nq, const int32_t *row, int32_t col_lo, int32_t col_hi,
                           int32_t k, int32_t smallest, int32_t include_diag, const int64_t *skip_ptr, const int32_t *skip_col,
                           int32_t *idx, double *val, int32_t *found);

/* state movers ("mutators outside the table") */
int lorads_hip_alm_to_admm(lorads_hip_ctx *ctx);        /* LORADS_ALMtoADMM copies, data/lorads_solver.c:968-983 */
int lorads_hip_average_uv_to_v(lorads_hip_ctx *ctx);    /* averageUV + copyRtoV, main.c:441-448 */
int lorads_hip_scale_obj(lorads_hip_ctx *ctx, double s); /* objScale_dualvar, data/lorads_solver.c:1040-1052 */
int lorads_hip_resize_rank(lorads_hip_ctx *ctx, const int32_t *new_rank); /* AUG_RANK, data/lorads_solver.c:806-906 */
/* column-major n x r host arrays, as lorads_sdp_dense.matElem (data/def_lorads_elements.h:29-33) */
int lorads_hip_set_mat(lorads_hip_ctx *ctx, int32_t which, int32_t blk, const double *colmajor);
int lorads_hip_get_mat(lorads_hip_ctx *ctx, int32_t which, int32_t blk, double *colmajor);
int lorads_hip_set_vec(lorads_hip_ctx *ctx, int32_t which, const double *v);
int lorads_hip_get_vec(lorads_hip_ctx *ctx, int32_t which, double *v);
int lorads_hip_set_allreduce(lorads_hip_ctx *ctx, lorads_hip_allreduce_fn fn, void *user);
/* The library's HIP stream (hipStream_t).  A hook that ENQUEUES its collective on this stream (RCCL
 * ncclAllReduce(..., stream)) can declare itself stream-ordered: the library then does not synchronise
 * the host before calling it, so a multi-GPU ADMM iteration still has a single host sync. */
void *lorads_hip_stream(lorads_hip_ctx *ctx);
int lorads_hip_set_allreduce_stream_ordered(lorads_hip_ctx *ctx, int32_t on);
/* Sharded cones whose constraints are BLOCK-SEPARABLE over the ranks (no constraint touches cones of two ranks): the caller
 * creates each rank's context on the sub-problem over the rank's own constraints (m, b, row indices local; b_nrm1 of the
 * whole problem) and declares it here.  Every m-vector of the method then lives on one rank only, and the library sums
 * SCALARS over the ranks instead of constrValSum, q1, q2: per ADMM iteration one all-reduce of four doubles
 * {||b - A(RR^T)||^2 part, b.lambda part, <C,RR^T> part, "my sweep is unfinished"}, and the rank's iteration is the
 * single-GPU iteration (all its fused paths) around it.  lorads_hip_get_vec / set_vec move the rank's own pieces. */
int lorads_hip_set_separable(lorads_hip_ctx *ctx, int32_t on);
/* Separable shards on the GPUs of ONE node: the four scalars of an ADMM iteration's evaluation are read by nobody but the ranks'
 * hosts, which wait for their GPU's result hand-over at that very point.  With a scalar exchange installed the library takes the
 * collective off the stream: the evaluation leaves the rank's LOCAL sums in the control block, the hand-over kernel delivers them
 * with everything else, and each rank's host calls fn(user, vals, 4) -- which must leave in vals the sums over all ranks, the same
 * bits on every rank -- before it looks at them (lorads_amd/csrc/host/shmx.c: a page of POSIX shared memory, sums in rank order).
 * The sharded iteration's launch chain is then the single-GPU chain + one one-workgroup kernel.  Phase 1's collectives (which feed
 * device-side consumers) and the m-vector form keep the all-reduce hook.  fn = NULL removes it.  (The reference has no counterpart:
 * it sweeps all cones in one process, lorads_alg/lorads_alg_common.c:190-214.) */
typedef int (*lorads_hip_scalar_exchange_fn)(void *user, double *vals, int32_t n);
int lorads_hip_set_scalar_exchange(lorads_hip_ctx *ctx, lorads_hip_scalar_exchange_fn fn, void *user);
/* all-reduces constrValSum through the hook once (lets the caller validate its hook) */
int lorads_hip_selfcheck_allreduce(lorads_hip_ctx *ctx);

int lorads_hip_sync(lorads_hip_ctx *ctx);
/* the U front of the next ADMM step, enqueued behind a step's result hand-over (LORADS_SPEC_FRONT=0 switches it off): out = {fronts
 * enqueued ahead, taken by the next lorads_hip_admm_step, discarded (the caller did something other than lorads_hip_update_dual_var
 * and lorads_hip_admm_step with the same rho), blocked by their gate (the step's V-solve resumed: they wrote nothing)} */
int lorads_hip_spec_front_stats(lorads_hip_ctx *ctx, int64_t out[4]);
/* a step's result hand-over rides on the launch of that front as one more workgroup where the front follows the evaluation's own
 * hand-over (LORADS_HANDOVER_ON_FRONT=0, read at creation: always a launch of its own, the front behind it): out = {hand-overs
 * carried on a front, hand-overs launched alone}.  Results do not depend on it.  Leaves a front in flight alone. */
int lorads_hip_handover_stats(lorads_hip_ctx *ctx, int64_t out[2]);
/* the rows per workgroup of the two row-tile gather kernels (k_front_cw, k_spmm_ell) on cone `block`: out = {rows per workgroup,
 * grid, compute units dealt over}.  LORADS_ROW_DEAL, read at creation: unset or "auto" deals a cone of more than 32 rows per
 * compute unit evenly, 0 keeps 32 rows per workgroup, 1..32 forces that many for every cone (a test switch: a cone for which that
 * many rows would give more workgroups than a partial-sum slot holds keeps 32, as `out` then shows).  Leaves a front in flight alone. */
int lorads_hip_row_deal_stats(lorads_hip_ctx *ctx, int32_t block, int out[3]);
/* which row outputs of those two kernels are stored through the L2 (write-through) instead of left dirty in it for the end-of-kernel
 * release: the mask in effect.  LORADS_WT_STORES, read at creation: bit 0 the front's initial residual, 1 its right-hand side, 2 the
 * slot contributions, 3 x and r of CG iteration 0 inside k_spmm_ell, 4 the average R written there, 5 the output of the plain
 * k_spmm_ell; 0 = plain stores everywhere; unset = the default.  Results do not depend on it.  Leaves a front in flight alone. */
int lorads_hip_wt_stores(lorads_hip_ctx *ctx, int *mask);
/* the cuts in the solve front's chain of dependent loads (k_front_cw): LORADS_FRONT_CHAIN, read at creation: bit 0 the neighbour
 * rows loaded without the mask of the slice beyond r (masked once in the epilogue), bit 1 the row's own operands requested late;
 * 0 = the front without them; unset = the default (both).  *mask is the context's mask.  The cuts belong to the form of the front
 * with the LDS park (r <= 48, LORADS_FRONT_LDS on); other cones launch the uncut kernel whatever the mask says: *effective (may
 * be null) is the mask if some cone of the context launches the cut form, else 0.  Results do not depend on either, bit for
 * bit.  Leaves a front in flight alone. */
int lorads_hip_front_chain(lorads_hip_ctx *ctx, int *mask, int *effective);
/* what the dense-coefficient GEMM (k_dense_cx_b: a dense objective, dense constraint matrices) launches for cone `block` at its
 * current device rank: out = {n padded to 64, K split over workgroups (slabs that k_sum_slabs adds when > 1), number of launches L,
 * then (first column, column tiles of 16 on the matrix cores, single columns on plain FMAs) for each of the L <= 4 launches}, zeros
 * behind them and for a cone without dense storage.  LORADS_DENSE_REM=0, read at creation, gives the single columns a tile of
 * their own.  out[15]: the factor array whose products A_j Y with the dense constraint matrices are kept at this moment (0 none,
 * 1 U, 2 V, 3 another array): whoever overwrites that array has to drop them.  Leaves a front in flight alone. */
int lorads_hip_dense_plan(lorads_hip_ctx *ctx, int32_t block, int64_t out[16]);

#ifdef __cplusplus
}
#endif
#endif
