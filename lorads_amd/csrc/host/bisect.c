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
    lrd_round_head_free(&r->head);
    free(r);
}

int lrd_bisection_write(const char *path, const lrd_bisection *r) {
    if (!path || !r) return 1;
    FILE *f = lrd_round_head_write(path, "lorads-bisection 1", &r->head, NULL, NULL);
    if (!f) return 2;
    for (int k = 0; k < r->nblk; ++k) {
        const lrd_bisection_cone *q = &r->cone[k];
        fprintf(f, "cone %d %d %d %d %d %.17g\n", k + 1, q->n, q->diff, q->plus, q->minus, q->t);
        for (int j = 0; j < q->n; ++j) fprintf(f, "%s\n", q->sigma[j] > 0 ? "+1" : "-1");
    }
    fprintf(f, "objectives %d\n", r->head.trials);
    for (int i = 0; i < r->head.trials; ++i) fprintf(f, "%.17g %.17g\n", r->head.obj0[i], r->head.obj[i]);
    return fclose(f) == 0 ? 0 : 3;
}

int lrd_session_round_bisect(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, int with_hyperplanes,
                             lrd_bisection **out) {
    *out = NULL;
    lrd_backend *be = NULL;
    lrd_solver *v = NULL;
    int src;
    const int refused = lrd_round_begin(s, lrd_session_backend(s) && lrd_session_backend(s)->round_bisect != NULL,
                                        "read a balanced partition off a solution", &v, &be, &src);
    if (refused) return refused;
    const lrd_problem *p = lrd_session_problem(s);
    if (trials <= 0)
        return trials < 0 ? 1 : be->round_bisect(be->ctx, src, 0, seed, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    const int nblk = p->nblk;
    size_t ntot = 0, gtot = 0;
    for (int k = 0; k < nblk; ++k) {
        ntot += (size_t)p->blk[k].n;
        gtot += (size_t)v->rank[k] * (size_t)trials;
    }
    lrd_bisection *r = (lrd_bisection *)calloc(1, sizeof *r);
    lrd_round_head *h = &r->head;
    lrd_round_head_init(h, trials, seed, max_rounds, src, v->scaleObjHis, tol);
    r->nblk = nblk;
    r->cone = (lrd_bisection_cone *)lrd_zalloc((size_t)nblk, sizeof(lrd_bisection_cone));
    int8_t *sign = (int8_t *)lrd_zalloc(ntot, 1);
    int *imb = (int *)lrd_zalloc((size_t)nblk * (size_t)trials, sizeof(int)), *diff = (int *)lrd_zalloc((size_t)nblk, sizeof(int));
    double *t = (double *)lrd_zalloc((size_t)nblk, sizeof(double));
    /* (the backend validates trials before it writes anything: the hyperplanes are never written when it refuses) */
    double *g = with_hyperplanes && trials <= 65536 ? (double *)lrd_zalloc(gtot, sizeof(double)) : NULL;
    int rc = be->round_bisect(be->ctx, src, trials, seed, max_rounds, h->obj, h->obj0, &h->best, &h->best0, sign, imb, &h->rounds, g, t,
                              diff);
    if (rc) {
        free(sign); free(imb); free(diff); free(t); free(g);
        lrd_bisection_free(r);
        return rc;
    }
    lrd_round_head_scale(h);
    double *T = (double *)lrd_zalloc((size_t)nblk, sizeof(double)), *lm = (double *)lrd_zalloc((size_t)nblk, sizeof(double));
    size_t at = 0, gat = 0;
    for (int k = 0; k < nblk; ++k) {
        lrd_bisection_cone *q = &r->cone[k];
        const int n = p->blk[k].n;
        q->n = n; q->rank = v->rank[k]; q->diff = diff[k]; q->t = t[k];
        q->sigma = (int8_t *)lrd_zalloc((size_t)n, 1);
        q->imbalance = (int *)lrd_zalloc((size_t)trials, sizeof(int));
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
    rc = lrd_round_head_bound(h, be, nblk, nblk, NULL, T, -1, 0, NULL, NULL, lm);
    for (int k = 0; k < nblk; ++k) r->cone[k].lam_min = lm[k];
    free(T); free(lm);
    if (rc) { lrd_bisection_free(r); return 1; }
    *out = r;
    return 0;
}
