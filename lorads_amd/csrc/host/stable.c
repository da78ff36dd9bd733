/* stable.c -- stable sets of a theta-structured session read off its factors (lorads_host.h: lrd_session_round_stable; DESIGN.md
 * section 18) and their plain-text file (lrd_stable_write), a pure function of the struct so that the command line and the Python
 * session write the same bytes and the format can be checked without a GPU.
 *
 *   lorads-stableset 1
 *   trials <K>  seed <S>  max_rounds <L>  rounds <r>  src <0|1>  best <i>  best0 <i>  lp_columns <n>  lp_negative <n>
 *                                                                                        (one per line, integers)
 *   scale, f_best, f_best0, by, bound, gap, tol                                          (one per line, %.17g)
 *   cone <b> <n> <size>     then size lines: the members of the best trial's set, 1-based, ascending
 *
 * b is the cone's 1-based block number in the file. */
#include "lorads_host.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void lrd_stable_free(lrd_stable *r) {
    if (!r) return;
    for (int k = 0; r->cone && k < r->nblk; ++k) {
        lrd_stable_cone *q = &r->cone[k];
        free(q->member); free(q->sizes); free(q->scores);
    }
    free(r->cone);
    free(r->obj);
    free(r->obj0);
    free(r->lp_upper);
    free(r);
}

int lrd_stable_write(const char *path, const lrd_stable *r) {
    if (!path || !r) return 1;
    FILE *f = fopen(path, "w");
    if (!f) return 2;
    fprintf(f, "lorads-stableset 1\n");
    fprintf(f, "trials %d\nseed %" PRIu64 "\nmax_rounds %d\nrounds %d\nsrc %d\nbest %d\nbest0 %d\nlp_columns %d\nlp_negative %d\n", r->trials,
            r->seed, r->max_rounds, r->rounds, r->src, r->best, r->best0, r->nlp, r->lp_neg);
    fprintf(f, "scale %.17g\nf_best %.17g\nf_best0 %.17g\nby %.17g\nbound %.17g\ngap %.17g\ntol %.17g\n", r->scale, r->f_best,
            r->f_best0, r->by, r->bound, r->gap, r->tol);
    for (int k = 0; k < r->nblk; ++k) {
        const lrd_stable_cone *q = &r->cone[k];
        fprintf(f, "cone %d %d %d\n", q->blk + 1, q->n, q->size);
        for (int j = 0; j < q->size; ++j) fprintf(f, "%d\n", q->member[j] + 1);
    }
    return fclose(f) == 0 ? 0 : 3;
}

static void *zalloc(size_t n, size_t size) { return calloc(n ? n : 1, size); }

int lrd_session_round_stable(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, int with_scores, lrd_stable **out) {
    *out = NULL;
    lrd_backend *be = NULL;
    lrd_solver *v = NULL;
    int src;
    const int refused = lrd_session_postsolve(s, lrd_session_backend(s) && lrd_session_backend(s)->round_stable != NULL,
                                              "read a stable set off a solution",
                                              "rounding the solution of a sharded deal (world > 1) is", &v, &be, &src);
    if (refused) return refused;
    const lrd_problem *p = lrd_session_problem(s);
    if (trials <= 0)
        return trials < 0 ? 1 : be->round_stable(be->ctx, src, 0, seed, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    const double sc = v->scaleObjHis;
    size_t ntot = 0;
    int nsdp = 0, nlp = 0, lpk = -1;
    for (int k = 0; k < p->nblk; ++k) {
        if (p->blk[k].is_lp) { nlp += p->blk[k].n; lpk = k; continue; }
        ++nsdp;
        ntot += (size_t)p->blk[k].n;
    }
    lrd_stable *r = (lrd_stable *)calloc(1, sizeof *r);
    r->nblk = nsdp; r->trials = trials; r->max_rounds = max_rounds; r->src = src; r->seed = seed; r->scale = sc;
    r->tol = tol; r->nlp = nlp;
    r->obj = (double *)zalloc((size_t)trials, sizeof(double));
    r->obj0 = (double *)zalloc((size_t)trials, sizeof(double));
    r->lp_upper = (double *)zalloc((size_t)nlp, sizeof(double));
    r->cone = (lrd_stable_cone *)zalloc((size_t)nsdp, sizeof(lrd_stable_cone));
    uint8_t *member = (uint8_t *)zalloc(ntot, 1);
    int *sizes = (int *)zalloc((size_t)nsdp * (size_t)trials, sizeof(int));
    double *Tu = (double *)zalloc((size_t)nsdp + (size_t)nlp, sizeof(double));
    /* (the backend validates trials before it writes anything: the scores are never written when it refuses) */
    double *scores = with_scores && trials <= 65536 ? (double *)zalloc(ntot * (size_t)trials, sizeof(double)) : NULL;
    int rc = be->round_stable(be->ctx, src, trials, seed, max_rounds, r->obj, r->obj0, &r->best, &r->best0, member, sizes, &r->rounds,
                              scores, Tu);
    if (rc) {
        free(member); free(sizes); free(Tu); free(scores);
        lrd_stable_free(r);
        return rc;
    }
    for (int i = 0; i < trials; ++i) { r->obj[i] /= sc; r->obj0[i] /= sc; }
    r->f_best = r->obj[r->best];
    r->f_best0 = r->obj0[r->best0];
    for (int j = 0; j < nlp; ++j) r->lp_upper[j] = Tu[nsdp + j];
    size_t at = 0;
    int kc = 0;
    for (int k = 0; k < p->nblk; ++k) {
        const lrd_block *b = &p->blk[k];
        if (b->is_lp) continue;
        lrd_stable_cone *q = &r->cone[kc];
        const int n = b->n;
        q->blk = k; q->n = n; q->rank = v->rank[k]; q->T = Tu[kc];
        q->member = (int *)zalloc((size_t)n, sizeof(int));
        q->sizes = (int *)zalloc((size_t)trials, sizeof(int));
        memcpy(q->sizes, sizes + (size_t)kc * (size_t)trials, (size_t)trials * sizeof(int));
        for (int j = 0; j < n; ++j)
            if (member[at + (size_t)j]) q->member[q->size++] = j;
        if (scores) {
            const size_t len = (size_t)n * (size_t)trials;
            q->scores = (double *)malloc((len ? len : 1) * sizeof(double));
            memcpy(q->scores, scores + at * (size_t)trials, len * sizeof(double));
        }
        at += (size_t)n;
        ++kc;
    }
    free(member); free(sizes); free(scores);
    int *blk = (int *)zalloc((size_t)nsdp, sizeof(int));
    double *lm = (double *)zalloc((size_t)nsdp, sizeof(double));
    for (int i = 0; i < nsdp; ++i) blk[i] = r->cone[i].blk;
    lrd_dual_bound db;
    rc = lrd_rounded_dual_bound(be, src, tol, sc, p->nblk, nsdp, blk, Tu, lpk, nlp, r->lp_upper, r->f_best, &db, lm);
    r->by = db.by; r->bound = db.bound; r->gap = db.gap; r->lp_neg = db.lp_neg;
    for (int i = 0; i < nsdp; ++i) r->cone[i].lam_min = lm[i];
    free(blk); free(lm); free(Tu);
    if (rc) { lrd_stable_free(r); return 1; }
    *out = r;
    return 0;
}
