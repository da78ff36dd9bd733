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
    lrd_round_head_free(&r->head);
    free(r->lp_upper);
    free(r);
}

int lrd_stable_write(const char *path, const lrd_stable *r) {
    if (!path || !r) return 1;
    char last[64];
    snprintf(last, sizeof last, "lp_columns %d\nlp_negative %d\n", r->nlp, r->lp_neg);
    FILE *f = lrd_round_head_write(path, "lorads-stableset 1", &r->head, NULL, last);
    if (!f) return 2;
    for (int k = 0; k < r->nblk; ++k) {
        const lrd_stable_cone *q = &r->cone[k];
        fprintf(f, "cone %d %d %d\n", q->blk + 1, q->n, q->size);
        for (int j = 0; j < q->size; ++j) fprintf(f, "%d\n", q->member[j] + 1);
    }
    return fclose(f) == 0 ? 0 : 3;
}

int lrd_session_round_stable(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, int with_scores, lrd_stable **out) {
    *out = NULL;
    lrd_backend *be = NULL;
    lrd_solver *v = NULL;
    int src;
    const int refused = lrd_round_begin(s, lrd_session_backend(s) && lrd_session_backend(s)->round_stable != NULL,
                                        "read a stable set off a solution", &v, &be, &src);
    if (refused) return refused;
    const lrd_problem *p = lrd_session_problem(s);
    if (trials <= 0)
        return trials < 0 ? 1 : be->round_stable(be->ctx, src, 0, seed, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    size_t ntot = 0;
    int nsdp = 0, nlp = 0, lpk = -1;
    for (int k = 0; k < p->nblk; ++k) {
        if (p->blk[k].is_lp) { nlp += p->blk[k].n; lpk = k; continue; }
        ++nsdp;
        ntot += (size_t)p->blk[k].n;
    }
    lrd_stable *r = (lrd_stable *)calloc(1, sizeof *r);
    lrd_round_head *h = &r->head;
    lrd_round_head_init(h, trials, seed, max_rounds, src, v->scaleObjHis, tol);
    r->nblk = nsdp; r->nlp = nlp;
    r->lp_upper = (double *)lrd_zalloc((size_t)nlp, sizeof(double));
    r->cone = (lrd_stable_cone *)lrd_zalloc((size_t)nsdp, sizeof(lrd_stable_cone));
    uint8_t *member = (uint8_t *)lrd_zalloc(ntot, 1);
    int *sizes = (int *)lrd_zalloc((size_t)nsdp * (size_t)trials, sizeof(int));
    double *Tu = (double *)lrd_zalloc((size_t)nsdp + (size_t)nlp, sizeof(double));
    /* (the backend validates trials before it writes anything: the scores are never written when it refuses) */
    double *scores = with_scores && trials <= 65536 ? (double *)lrd_zalloc(ntot * (size_t)trials, sizeof(double)) : NULL;
    int rc = be->round_stable(be->ctx, src, trials, seed, max_rounds, h->obj, h->obj0, &h->best, &h->best0, member, sizes, &h->rounds,
                              scores, Tu);
    if (rc) {
        free(member); free(sizes); free(Tu); free(scores);
        lrd_stable_free(r);
        return rc;
    }
    lrd_round_head_scale(h);
    for (int j = 0; j < nlp; ++j) r->lp_upper[j] = Tu[nsdp + j];
    size_t at = 0;
    int kc = 0;
    for (int k = 0; k < p->nblk; ++k) {
        const lrd_block *b = &p->blk[k];
        if (b->is_lp) continue;
        lrd_stable_cone *q = &r->cone[kc];
        const int n = b->n;
        q->blk = k; q->n = n; q->rank = v->rank[k]; q->T = Tu[kc];
        q->member = (int *)lrd_zalloc((size_t)n, sizeof(int));
        q->sizes = (int *)lrd_zalloc((size_t)trials, sizeof(int));
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
    int *blk = (int *)lrd_zalloc((size_t)nsdp, sizeof(int));
    double *lm = (double *)lrd_zalloc((size_t)nsdp, sizeof(double));
    for (int i = 0; i < nsdp; ++i) blk[i] = r->cone[i].blk;
    rc = lrd_round_head_bound(h, be, p->nblk, nsdp, blk, Tu, lpk, nlp, r->lp_upper, &r->lp_neg, lm);
    for (int i = 0; i < nsdp; ++i) r->cone[i].lam_min = lm[i];
    free(blk); free(lm); free(Tu);
    if (rc) { lrd_stable_free(r); return 1; }
    *out = r;
    return 0;
}
