/* rounding.c -- hyperplane rounding of a +-1-structured session (lorads_host.h: lrd_session_round_ex), the dual
 * bound it shares with the rounding into k parts (lrd_rounded_dual_bound; kcut.c), and the plain-text rounding file
 * (lrd_rounding_write), a pure function of the struct so that the command line and the Python session write the same bytes and the
 * format can be checked without a GPU.
 *
 *   lorads-rounding 1
 *   trials <K>  seed <S>  max_rounds <L>  rounds <r>  src <0|1>  best <i>  best0 <i>     (one per line, integers)
 *   scale, f_best, f_best0, by, bound, gap, tol                                          (one per line, %.17g)
 *   cone <k> <n>        then n lines: +1 or -1, the best trial's signs
 *
 * k is the block's 1-based number in the file. */
#include "lorads_host.h"

#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void lrd_rounding_free(lrd_rounding *r) {
    if (!r) return;
    for (int k = 0; r->cone && k < r->nblk; ++k) {
        lrd_rounding_cone *q = &r->cone[k];
        free(q->sigma); free(q->t); free(q->x); free(q->G);
    }
    free(r->cone);
    free(r->obj);
    free(r->obj0);
    free(r);
}

int lrd_rounded_dual_bound(lrd_backend *be, int src, double tol, double sc, int nblk, int ncone, const int *blk, const double *T, int lpk,
                           int nlp, const double *lp_upper, double f_best, lrd_dual_bound *out, double *lam_min) {
    out->by = out->bound = out->gap = NAN;
    out->lp_neg = 0;
    for (int i = 0; i < ncone; ++i) lam_min[i] = NAN;
    if (!(tol > 0 && be->certificate && (lpk < 0 || be->get_slack))) return 0;
    double c[LRD_CERT_N];
    double *lm = (double *)calloc((size_t)(nblk > 0 ? nblk : 1), sizeof(double));
    int rc = be->certificate(be->ctx, src, tol, c, lm, NULL, NULL);
    if (!rc) {
        out->by = c[3] / sc;
        double d = out->by;
        for (int i = 0; i < ncone; ++i) {
            lam_min[i] = lm[blk ? blk[i] : i] / sc;
            if (lam_min[i] < 0) d += T[i] * lam_min[i];
        }
        if (lpk >= 0 && nlp > 0) {
            int64_t nnz = 0;
            int *row = (int *)calloc((size_t)nlp, sizeof(int)), *col = (int *)calloc((size_t)nlp, sizeof(int));
            double *val = (double *)calloc((size_t)nlp, sizeof(double));
            rc = be->get_slack(be->ctx, lpk, &nnz, NULL, NULL, NULL);
            if (!rc && nnz != nlp) rc = 1;
            if (!rc) rc = be->get_slack(be->ctx, lpk, &nnz, row, col, val);
            for (int64_t e = 0; e < nnz && !rc; ++e) {
                const double sj = val[e] / sc;
                if (sj < 0) { d += lp_upper[row[e]] * sj; out->lp_neg++; }
            }
            free(row); free(col); free(val);
        }
        out->bound = d;
        out->gap = (f_best - d) / (fabs(d) > 1.0 ? fabs(d) : 1.0);
    }
    free(lm);
    return rc;
}

/* hyperplane rounding of a +-1-structured context, in the file's units (lorads_host.h: lrd_rounding) */
int lrd_session_round_ex(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, int with_hyperplanes,
                         lrd_rounding **out) {
    *out = NULL;
    lrd_backend *be = lrd_session_backend(s);
    lrd_solver *v = NULL;
    int src;
    const int refused = lrd_session_postsolve(s, be && be->round_pm1 != NULL, "round a solution",
                                              "rounding the solution of a sharded deal (world > 1) is", &v, NULL, &src);
    if (refused) return refused;
    const lrd_problem *p = lrd_session_problem(s);
    if (trials <= 0) return trials < 0 ? 1 : be->round_pm1(be->ctx, src, 0, seed, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    const double sc = v->scaleObjHis;
    size_t ntot = 0, gtot = 0;
    for (int k = 0; k < p->nblk; ++k) {
        ntot += (size_t)p->blk[k].n;
        gtot += (size_t)v->rank[k] * (size_t)trials;
    }
    lrd_rounding *r = (lrd_rounding *)calloc(1, sizeof *r);
    r->nblk = p->nblk; r->trials = trials; r->max_rounds = max_rounds; r->src = src; r->seed = seed; r->scale = sc; r->tol = tol;
    r->obj = (double *)calloc((size_t)trials, sizeof(double));
    r->obj0 = (double *)calloc((size_t)trials, sizeof(double));
    r->cone = (lrd_rounding_cone *)calloc((size_t)(p->nblk > 0 ? p->nblk : 1), sizeof(lrd_rounding_cone));
    int8_t *sign = (int8_t *)calloc(ntot ? ntot : 1, 1);
    double *g = with_hyperplanes ? (double *)calloc(gtot ? gtot : 1, sizeof(double)) : NULL;
    int rc = be->round_pm1(be->ctx, src, trials, seed, max_rounds, r->obj, r->obj0, &r->best, &r->best0, sign, &r->rounds, g);
    if (rc) {
        free(sign); free(g);
        lrd_rounding_free(r);
        return rc;
    }
    for (int t = 0; t < trials; ++t) { r->obj[t] /= sc; r->obj0[t] /= sc; }
    r->f_best = r->obj[r->best];
    r->f_best0 = r->obj0[r->best0];
    size_t at = 0, gat = 0;
    for (int k = 0; k < p->nblk; ++k) { /* t from the problem: the one constraint on every diagonal (the backend has checked it) */
        const lrd_block *b = &p->blk[k];
        lrd_rounding_cone *q = &r->cone[k];
        const int n = b->n;
        q->n = n; q->rank = v->rank[k];
        q->sigma = (int8_t *)calloc((size_t)(n > 0 ? n : 1), 1);
        q->t = (double *)calloc((size_t)(n > 0 ? n : 1), sizeof(double));
        q->x = (double *)calloc((size_t)(n > 0 ? n : 1), sizeof(double));
        for (int i = 0; i < b->nrow; ++i) {
            const int e = b->a_ptr[i];
            q->t[b->a_row[e]] = sqrt(p->b[b->row_idx[i]] / b->a_val[e]);
        }
        q->T = 0.0;
        for (int j = 0; j < n; ++j) {
            q->sigma[j] = sign[at + (size_t)j];
            q->x[j] = q->sigma[j] * q->t[j];
            q->T += q->t[j] * q->t[j];
        }
        if (g) {
            const size_t len = (size_t)q->rank * (size_t)trials;
            q->G = (double *)malloc((len ? len : 1) * sizeof(double));
            memcpy(q->G, g + gat, len * sizeof(double));
            gat += len;
        }
        at += (size_t)n;
    }
    free(sign); free(g);
    double *T = (double *)calloc(2 * (size_t)(p->nblk > 0 ? p->nblk : 1), sizeof(double)), *lm = T + (p->nblk > 0 ? p->nblk : 1);
    for (int k = 0; k < p->nblk; ++k) T[k] = r->cone[k].T;
    lrd_dual_bound db;
    rc = lrd_rounded_dual_bound(be, src, tol, sc, p->nblk, p->nblk, NULL, T, -1, 0, NULL, r->f_best, &db, lm);
    r->by = db.by; r->bound = db.bound; r->gap = db.gap;
    for (int k = 0; k < p->nblk; ++k) r->cone[k].lam_min = lm[k];
    free(T);
    if (rc) { lrd_rounding_free(r); return 1; }
    *out = r;
    return 0;
}
int lrd_session_round(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, lrd_rounding **out) {
    return lrd_session_round_ex(s, trials, seed, max_rounds, tol, 0, out);
}


int lrd_rounding_write(const char *path, const lrd_rounding *r) {
    if (!path || !r) return 1;
    FILE *f = fopen(path, "w");
    if (!f) return 2;
    fprintf(f, "lorads-rounding 1\n");
    fprintf(f, "trials %d\nseed %" PRIu64 "\nmax_rounds %d\nrounds %d\nsrc %d\nbest %d\nbest0 %d\n", r->trials, r->seed,
            r->max_rounds, r->rounds, r->src, r->best, r->best0);
    fprintf(f, "scale %.17g\nf_best %.17g\nf_best0 %.17g\nby %.17g\nbound %.17g\ngap %.17g\ntol %.17g\n", r->scale, r->f_best,
            r->f_best0, r->by, r->bound, r->gap, r->tol);
    for (int k = 0; k < r->nblk; ++k) {
        const lrd_rounding_cone *q = &r->cone[k];
        fprintf(f, "cone %d %d\n", k + 1, q->n);
        for (int j = 0; j < q->n; ++j) fprintf(f, "%s\n", q->sigma[j] > 0 ? "+1" : "-1");
    }
    return fclose(f) == 0 ? 0 : 3;
}
