/* kcut.c -- rounding of a k-cut-structured session into k parts (lorads_host.h: lrd_session_kcut) and its
 * plain-text file (lrd_kcut_write), a pure function of the struct so that the command line and the Python session write the same
 * bytes and the format can be checked without a GPU.
 *
 *   lorads-kcut 1
 *   parts <k>  trials <K>  seed <S>  max_rounds <L>  rounds <r>  src <0|1>  best <i>  best0 <i>  lp_columns <n>  lp_negative <n>
 *                                                                                        (one per line, integers)
 *   scale, f_best, f_best0, by, bound, gap, tol                                          (one per line, %.17g)
 *   cone <b> <n>        then "sizes" and k integers (vertices per part), then n lines: the best trial's labels 0 .. k-1
 *
 * b is the cone's 1-based block number in the file. */
#include "lorads_host.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void lrd_kcut_free(lrd_kcut *r) {
    if (!r) return;
    for (int k = 0; r->cone && k < r->nblk; ++k) {
        lrd_kcut_cone *q = &r->cone[k];
        free(q->label); free(q->t); free(q->size); free(q->G);
    }
    free(r->cone);
    lrd_round_head_free(&r->head);
    free(r->lp_upper);
    free(r);
}

int lrd_kcut_write(const char *path, const lrd_kcut *r) {
    if (!path || !r) return 1;
    char first[32], last[64];
    snprintf(first, sizeof first, "parts %d\n", r->parts);
    snprintf(last, sizeof last, "lp_columns %d\nlp_negative %d\n", r->nlp, r->lp_neg);
    FILE *f = lrd_round_head_write(path, "lorads-kcut 1", &r->head, first, last);
    if (!f) return 2;
    for (int k = 0; k < r->nblk; ++k) {
        const lrd_kcut_cone *q = &r->cone[k];
        fprintf(f, "cone %d %d\nsizes", q->blk + 1, q->n);
        for (int a = 0; a < r->parts; ++a) fprintf(f, " %d", q->size[a]);
        fprintf(f, "\n");
        for (int j = 0; j < q->n; ++j) fprintf(f, "%d\n", (int)q->label[j]);
    }
    return fclose(f) == 0 ? 0 : 3;
}

int lrd_session_kcut(lrd_session *s, int parts, int trials, uint64_t seed, int max_rounds, double tol, int with_vectors, lrd_kcut **out) {
    *out = NULL;
    lrd_backend *be = NULL;
    lrd_solver *v = NULL;
    int src;
    const int refused = lrd_round_begin(s, lrd_session_backend(s) && lrd_session_backend(s)->round_kcut != NULL,
                                        "round a solution into k parts", &v, &be, &src);
    if (refused) return refused;
    const lrd_problem *p = lrd_session_problem(s);
    if (trials <= 0)
        return trials < 0 ? 1 : be->round_kcut(be->ctx, src, parts, 0, seed, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    size_t ntot = 0, gtot = 0;
    int nsdp = 0, nlp = 0, lpk = -1;
    for (int k = 0; k < p->nblk; ++k) {
        if (p->blk[k].is_lp) { nlp += p->blk[k].n; lpk = k; continue; }
        ++nsdp;
        ntot += (size_t)p->blk[k].n;
        if (parts > 0) gtot += (size_t)v->rank[k] * (size_t)trials * (size_t)parts;
    }
    lrd_kcut *r = (lrd_kcut *)calloc(1, sizeof *r);
    lrd_round_head *h = &r->head;
    lrd_round_head_init(h, trials, seed, max_rounds, src, v->scaleObjHis, tol);
    r->nblk = nsdp; r->parts = parts; r->nlp = nlp;
    r->lp_upper = (double *)lrd_zalloc((size_t)nlp, sizeof(double));
    r->cone = (lrd_kcut_cone *)lrd_zalloc((size_t)nsdp, sizeof(lrd_kcut_cone));
    uint8_t *label = (uint8_t *)lrd_zalloc(ntot, 1);
    double *t = (double *)lrd_zalloc(ntot, sizeof(double));
    /* (the backend validates parts and trials x parts before it writes anything: g is never written when it refuses) */
    double *g = with_vectors && parts >= 2 && parts <= 64 && (int64_t)trials * parts <= (1 << 20) ? (double *)lrd_zalloc(gtot, sizeof(double)) : NULL;
    int rc = be->round_kcut(be->ctx, src, parts, trials, seed, max_rounds, h->obj, h->obj0, &h->best, &h->best0, label, &h->rounds, g, t,
                            r->lp_upper);
    if (rc) {
        free(label); free(t); free(g);
        lrd_kcut_free(r);
        return rc;
    }
    lrd_round_head_scale(h);
    size_t at = 0, gat = 0;
    int kc = 0;
    for (int k = 0; k < p->nblk; ++k) {
        const lrd_block *b = &p->blk[k];
        if (b->is_lp) continue;
        lrd_kcut_cone *q = &r->cone[kc++];
        const int n = b->n;
        q->blk = k; q->n = n; q->rank = v->rank[k];
        q->label = (uint8_t *)lrd_zalloc((size_t)n, 1);
        q->t = (double *)lrd_zalloc((size_t)n, sizeof(double));
        q->size = (int *)lrd_zalloc((size_t)parts, sizeof(int));
        q->T = 0.0;
        for (int j = 0; j < n; ++j) {
            q->label[j] = label[at + (size_t)j];
            q->t[j] = t[at + (size_t)j];
            q->T += q->t[j] * q->t[j];
            if (q->label[j] < parts) q->size[q->label[j]]++;
        }
        if (g) {
            const size_t len = (size_t)q->rank * (size_t)trials * (size_t)parts;
            q->G = (double *)malloc((len ? len : 1) * sizeof(double));
            memcpy(q->G, g + gat, len * sizeof(double));
            gat += len;
        }
        at += (size_t)n;
    }
    free(label); free(t); free(g);
    int *blk = (int *)lrd_zalloc((size_t)nsdp, sizeof(int));
    double *T = (double *)lrd_zalloc(2 * (size_t)(nsdp > 0 ? nsdp : 1), sizeof(double)), *lm = T + (nsdp > 0 ? nsdp : 1);
    for (int i = 0; i < nsdp; ++i) { blk[i] = r->cone[i].blk; T[i] = r->cone[i].T; }
    rc = lrd_round_head_bound(h, be, p->nblk, nsdp, blk, T, lpk, nlp, r->lp_upper, &r->lp_neg, lm);
    for (int i = 0; i < nsdp; ++i) r->cone[i].lam_min = lm[i];
    free(blk); free(T);
    if (rc) { lrd_kcut_free(r); return 1; }
    *out = r;
    return 0;
}
