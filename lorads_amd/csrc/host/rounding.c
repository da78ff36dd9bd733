/* rounding.c -- what the four roundings (this file, kcut.c, stable.c, bisect.c) do with the head of their results (lrd_round_head:
 * lrd_round_begin, lrd_round_head_*) and their dual bound (lrd_rounded_dual_bound); hyperplane rounding of a +-1-structured session
 * (lorads_host.h: lrd_session_round_ex) and the plain-text rounding file
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
    free(r->lp_upper);
    lrd_round_head_free(&r->head);
    free(r);
}

void *lrd_zalloc(size_t n, size_t size) { return calloc(n ? n : 1, size); }

int lrd_round_begin(lrd_session *s, int have_slot, const char *cannot, lrd_solver **v, lrd_backend **be, int *src) {
    return lrd_session_postsolve(s, have_slot, cannot, "rounding the solution of a sharded deal (world > 1) is", v, be, src);
}

void lrd_round_head_init(lrd_round_head *h, int trials, uint64_t seed, int max_rounds, int src, double scale, double tol) {
    h->trials = trials; h->max_rounds = max_rounds; h->src = src; h->seed = seed; h->scale = scale; h->tol = tol;
    h->obj = (double *)lrd_zalloc((size_t)trials, sizeof(double));
    h->obj0 = (double *)lrd_zalloc((size_t)trials, sizeof(double));
}

void lrd_round_head_scale(lrd_round_head *h) {
    for (int t = 0; t < h->trials; ++t) { h->obj[t] /= h->scale; h->obj0[t] /= h->scale; }
    h->f_best = h->obj[h->best];
    h->f_best0 = h->obj0[h->best0];
}

void lrd_round_head_free(lrd_round_head *h) {
    free(h->obj);
    free(h->obj0);
}

FILE *lrd_round_head_write(const char *path, const char *magic, const lrd_round_head *h, const char *first, const char *last) {
    FILE *f = fopen(path, "w");
    if (!f) return NULL;
    fprintf(f, "%s\n%s", magic, first ? first : "");
    fprintf(f, "trials %d\nseed %" PRIu64 "\nmax_rounds %d\nrounds %d\nsrc %d\nbest %d\nbest0 %d\n%s", h->trials, h->seed,
            h->max_rounds, h->rounds, h->src, h->best, h->best0, last ? last : "");
    fprintf(f, "scale %.17g\nf_best %.17g\nf_best0 %.17g\nby %.17g\nbound %.17g\ngap %.17g\ntol %.17g\n", h->scale, h->f_best,
            h->f_best0, h->by, h->bound, h->gap, h->tol);
    return f;
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

int lrd_round_head_bound(lrd_round_head *h, lrd_backend *be, int nblk, int ncone, const int *blk, const double *T, int lpk, int nlp,
                         const double *lp_upper, int *lp_neg, double *lam_min) {
    lrd_dual_bound db;
    const int rc = lrd_rounded_dual_bound(be, h->src, h->tol, h->scale, nblk, ncone, blk, T, lpk, nlp, lp_upper, h->f_best, &db, lam_min);
    h->by = db.by; h->bound = db.bound; h->gap = db.gap;
    if (lp_neg) *lp_neg = db.lp_neg;
    return rc;
}

/* hyperplane rounding of a +-1-structured context, in the file's units (lorads_host.h: lrd_rounding) */
int lrd_session_round_ex(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, int with_hyperplanes,
                         lrd_rounding **out) {
    *out = NULL;
    lrd_backend *be = lrd_session_backend(s);
    lrd_solver *v = NULL;
    int src;
    const int refused = lrd_round_begin(s, be && be->round_pm1 != NULL, "round a solution", &v, NULL, &src);
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
    lrd_round_head *h = &r->head;
    lrd_round_head_init(h, trials, seed, max_rounds, src, sc, tol);
    r->nblk = p->nblk;
    r->cone = (lrd_rounding_cone *)calloc((size_t)(p->nblk > 0 ? p->nblk : 1), sizeof(lrd_rounding_cone));
    int8_t *sign = (int8_t *)calloc(ntot ? ntot : 1, 1);
    double *g = with_hyperplanes ? (double *)calloc(gtot ? gtot : 1, sizeof(double)) : NULL;
    int rc = be->round_pm1(be->ctx, src, trials, seed, max_rounds, h->obj, h->obj0, &h->best, &h->best0, sign, &h->rounds, g);
    if (rc) {
        free(sign); free(g);
        lrd_rounding_free(r);
        return rc;
    }
    lrd_round_head_scale(h);
    size_t at = 0, gat = 0;
    int lpk = -1;
    for (int k = 0; k < p->nblk; ++k) { /* t from the problem: the one constraint on every diagonal (the backend has checked it) */
        const lrd_block *b = &p->blk[k];
        lrd_rounding_cone *q = &r->cone[k];
        if (b->is_lp) { /* the slacks of a cut-tightened problem: no signs and no hyperplanes, an empty cone of the result */
            lpk = k;
            q->sigma = (int8_t *)lrd_zalloc(0, 1);
            q->t = (double *)lrd_zalloc(0, sizeof(double));
            q->x = (double *)lrd_zalloc(0, sizeof(double));
            at += (size_t)b->n;
            continue;
        }
        const int n = b->n;
        q->n = n; q->rank = v->rank[k];
        q->sigma = (int8_t *)calloc((size_t)(n > 0 ? n : 1), 1);
        q->t = (double *)calloc((size_t)(n > 0 ? n : 1), sizeof(double));
        q->x = (double *)calloc((size_t)(n > 0 ? n : 1), sizeof(double));
        for (int i = 0; i < b->nrow; ++i) {
            const int e = b->a_ptr[i];
            if (b->a_ptr[i + 1] - e != 1 || b->a_row[e] != b->a_col[e]) continue; /* (a triangle row of a cut-tightened problem) */
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
    if (lpk < 0) {
        rc = lrd_round_head_bound(h, be, p->nblk, p->nblk, NULL, T, -1, 0, NULL, NULL, lm);
        for (int k = 0; k < p->nblk; ++k) r->cone[k].lam_min = lm[k];
    } else { /* cut-tightened: the LP term of the k-cut's bound with u_j = 4 scale_j of column j's triangle row (cuts.c) */
        lrd_present *pc = NULL;
        rc = lrd_session_present_cuts(s, &pc);
        int *blk = (int *)lrd_zalloc((size_t)p->nblk, sizeof(int)), nsdp = 0;
        for (int k = 0; k < p->nblk; ++k)
            if (k != lpk) { blk[nsdp] = k; T[nsdp++] = r->cone[k].T; }
        if (!rc) {
            r->nlp = p->blk[lpk].n;
            r->lp_upper = (double *)lrd_zalloc((size_t)r->nlp, sizeof(double));
            for (int e = 0; e < pc->n; ++e) r->lp_upper[pc->col[e]] = 4.0 * pc->scale[e];
            rc = lrd_round_head_bound(h, be, p->nblk, nsdp, blk, T, lpk, r->nlp, r->lp_upper, &r->lp_neg, lm);
            r->cone[lpk].lam_min = NAN;
            for (int i = 0; i < nsdp; ++i) r->cone[blk[i]].lam_min = lm[i];
        }
        lrd_present_free(pc);
        free(blk);
    }
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
    FILE *f = lrd_round_head_write(path, "lorads-rounding 1", &r->head, NULL, NULL);
    if (!f) return 2;
    for (int k = 0; k < r->nblk; ++k) {
        const lrd_rounding_cone *q = &r->cone[k];
        fprintf(f, "cone %d %d\n", k + 1, q->n);
        for (int j = 0; j < q->n; ++j) fprintf(f, "%s\n", q->sigma[j] > 0 ? "+1" : "-1");
    }
    return fclose(f) == 0 ? 0 : 3;
}
