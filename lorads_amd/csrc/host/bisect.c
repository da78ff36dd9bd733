/* bisect.c -- balanced partitions of a bisection-structured session read off its factors (lorads_host.h: lrd_session_round_bisect;
 * DESIGN.md section 19) and their plain-text file (lrd_bisection_write), a pure function of the struct so that the command line and
 * the Python session write the same bytes and the format can be checked without a GPU.
 *
 *   lorads-bisection 1
 *   trials <K>  seed <S>  max_rounds <L>  rounds <r>  src <0|1>  best <i>  best0 <i>     (one per line, integers)
 *   scale, f_best, f_best0, by, bound, gap, tol                                          (one per line, %.17g)
 *   cone <k> <n> <d> <plus> <minus> <t %.17g>     then n lines: +1 or -1, the best trial's signs
 *   objectives <K>                                then K lines: f0 f (%.17g each), after the repair / after the search
 *
 * k is the block's 1-based number in the file; plus and minus are the part sizes, (n + d) / 2 and (n - d) / 2 in either order. */
#include "lorads_host.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void lrd_bisection_free(lrd_bisection *r) {
    if (!r) return;
    for (int k = 0; r->cone && k < r->nblk; ++k) {
        lrd_bisection_cone *q = &r->cone[k];
        free(q->sigma); free(q->imbalance); free(q->G);
    }
    free(r->cone);
    free(r->obj);
    free(r->obj0);
    free(r);
}

int lrd_bisection_write(const char *path, const lrd_bisection *r) {
    if (!path || !r) return 1;
    FILE *f = fopen(path, "w");
    if (!f) return 2;
    fprintf(f, "lorads-bisection 1\n");
    fprintf(f, "trials %d\nseed %" PRIu64 "\nmax_rounds %d\nrounds %d\nsrc %d\nbest %d\nbest0 %d\n", r->trials, r->seed,
            r->max_rounds, r->rounds, r->src, r->best, r->best0);
    fprintf(f, "scale %.17g\nf_best %.17g\nf_best0 %.17g\nby %.17g\nbound %.17g\ngap %.17g\ntol %.17g\n", r->scale, r->f_best,
            r->f_best0, r->by, r->bound, r->gap, r->tol);
    for (int k = 0; k < r->nblk; ++k) {
        const lrd_bisection_cone *q = &r->cone[k];
        fprintf(f, "cone %d %d %d %d %d %.17g\n", k + 1, q->n, q->diff, q->plus, q->minus, q->t);
        for (int j = 0; j < q->n; ++j) fprintf(f, "%s\n", q->sigma[j] > 0 ? "+1" : "-1");
    }
    fprintf(f, "objectives %d\n", r->trials);
    for (int i = 0; i < r->trials; ++i) fprintf(f, "%.17g %.17g\n", r->obj0[i], r->obj[i]);
    return fclose(f) == 0 ? 0 : 3;
}

static void *zalloc(size_t n, size_t size) { return calloc(n ? n : 1, size); }

int lrd_session_round_bisect(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, int with_hyperplanes,
                             lrd_bisection **out) {
    *out = NULL;
    lrd_backend *be = NULL;
    lrd_solver *v = NULL;
    int src;
    const int refused = lrd_session_postsolve(s, lrd_session_backend(s) && lrd_session_backend(s)->round_bisect != NULL,
                                              "read a balanced partition off a solution",
                                              "rounding the solution of a sharded deal (world > 1) is", &v, &be, &src);
    if (refused) return refused;
    const lrd_problem *p = lrd_session_problem(s);
    if (trials <= 0)
        return trials < 0 ? 1 : be->round_bisect(be->ctx, src, 0, seed, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    const double sc = v->scaleObjHis;
    const int nblk = p->nblk;
    size_t ntot = 0, gtot = 0;
    for (int k = 0; k < nblk; ++k) {
        ntot += (size_t)p->blk[k].n;
        gtot += (size_t)v->rank[k] * (size_t)trials;
    }
    lrd_bisection *r = (lrd_bisection *)calloc(1, sizeof *r);
    r->nblk = nblk; r->trials = trials; r->max_rounds = max_rounds; r->src = src; r->seed = seed; r->scale = sc; r->tol = tol;
    r->obj = (double *)zalloc((size_t)trials, sizeof(double));
    r->obj0 = (double *)zalloc((size_t)trials, sizeof(double));
    r->cone = (lrd_bisection_cone *)zalloc((size_t)nblk, sizeof(lrd_bisection_cone));
    int8_t *sign = (int8_t *)zalloc(ntot, 1);
    int *imb = (int *)zalloc((size_t)nblk * (size_t)trials, sizeof(int)), *diff = (int *)zalloc((size_t)nblk, sizeof(int));
    double *t = (double *)zalloc((size_t)nblk, sizeof(double));
    /* (the backend validates trials before it writes anything: the hyperplanes are never written when it refuses) */
    double *g = with_hyperplanes && trials <= 65536 ? (double *)zalloc(gtot, sizeof(double)) : NULL;
    int rc = be->round_bisect(be->ctx, src, trials, seed, max_rounds, r->obj, r->obj0, &r->best, &r->best0, sign, imb, &r->rounds, g, t,
                              diff);
    if (rc) {
        free(sign); free(imb); free(diff); free(t); free(g);
        lrd_bisection_free(r);
        return rc;
    }
    for (int i = 0; i < trials; ++i) { r->obj[i] /= sc; r->obj0[i] /= sc; }
    r->f_best = r->obj[r->best];
    r->f_best0 = r->obj0[r->best0];
    double *T = (double *)zalloc((size_t)nblk, sizeof(double)), *lm = (double *)zalloc((size_t)nblk, sizeof(double));
    size_t at = 0, gat = 0;
    for (int k = 0; k < nblk; ++k) {
        lrd_bisection_cone *q = &r->cone[k];
        const int n = p->blk[k].n;
        q->n = n; q->rank = v->rank[k]; q->diff = diff[k]; q->t = t[k];
        q->sigma = (int8_t *)zalloc((size_t)n, 1);
        q->imbalance = (int *)zalloc((size_t)trials, sizeof(int));
        memcpy(q->imbalance, imb + (size_t)k * (size_t)trials, (size_t)trials * sizeof(int));
        for (int j = 0; j < n; ++j) {
            q->sigma[j] = sign[at + (size_t)j];
            if (q->sigma[j] > 0) q->plus++; else q->minus++;
        }
        if (g) {
            const size_t len = (size_t)q->rank * (size_t)trials;
            q->G = (double *)malloc((len ? len : 1) * sizeof(double));
            memcpy(q->G, g + gat, len * sizeof(double));
            gat += len;
        }
        T[k] = (double)n * t[k] * t[k]; /* the trace of every feasible X_k */
        at += (size_t)n;
    }
    free(sign); free(imb); free(diff); free(t); free(g);
    lrd_dual_bound db;
    rc = lrd_rounded_dual_bound(be, src, tol, sc, nblk, nblk, NULL, T, -1, 0, NULL, r->f_best, &db, lm);
    r->by = db.by; r->bound = db.bound; r->gap = db.gap;
    for (int k = 0; k < nblk; ++k) r->cone[k].lam_min = lm[k];
    free(T); free(lm);
    if (rc) { lrd_bisection_free(r); return 1; }
    *out = r;
    return 0;
}
