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
    free(r->obj);
    free(r->obj0);
    free(r->lp_upper);
    free(r);
}

int lrd_kcut_write(const char *path, const lrd_kcut *r) {
    if (!path || !r) return 1;
    FILE *f = fopen(path, "w");
    if (!f) return 2;
    fprintf(f, "lorads-kcut 1\n");
    fprintf(f, "parts %d\ntrials %d\nseed %" PRIu64 "\nmax_rounds %d\nrounds %d\nsrc %d\nbest %d\nbest0 %d\nlp_columns %d\nlp_negative %d\n",
            r->parts, r->trials, r->seed, r->max_rounds, r->rounds, r->src, r->best, r->best0, r->nlp, r->lp_neg);
    fprintf(f, "scale %.17g\nf_best %.17g\nf_best0 %.17g\nby %.17g\nbound %.17g\ngap %.17g\ntol %.17g\n", r->scale, r->f_best,
            r->f_best0, r->by, r->bound, r->gap, r->tol);
    for (int k = 0; k < r->nblk; ++k) {
        const lrd_kcut_cone *q = &r->cone[k];
        fprintf(f, "cone %d %d\nsizes", q->blk + 1, q->n);
        for (int a = 0; a < r->parts; ++a) fprintf(f, " %d", q->size[a]);
        fprintf(f, "\n");
        for (int j = 0; j < q->n; ++j) fprintf(f, "%d\n", (int)q->label[j]);
    }
    return fclose(f) == 0 ? 0 : 3;
}

static void *zalloc(size_t n, size_t size) { return calloc(n ? n : 1, size); }

int lrd_session_kcut(lrd_session *s, int parts, int trials, uint64_t seed, int max_rounds, double tol, int with_vectors, lrd_kcut **out) {
    *out = NULL;
    lrd_backend *be = NULL;
    lrd_solver *v = NULL;
    int src;
    const int refused = lrd_session_postsolve(s, lrd_session_backend(s) && lrd_session_backend(s)->round_kcut != NULL,
                                              "round a solution into k parts",
                                              "rounding the solution of a sharded deal (world > 1) is", &v, &be, &src);
    if (refused) return refused;
    const lrd_problem *p = lrd_session_problem(s);
    if (trials <= 0)
        return trials < 0 ? 1 : be->round_kcut(be->ctx, src, parts, 0, seed, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    const double sc = v->scaleObjHis;
    size_t ntot = 0, gtot = 0;
    int nsdp = 0, nlp = 0, lpk = -1;
    for (int k = 0; k < p->nblk; ++k) {
        if (p->blk[k].is_lp) { nlp += p->blk[k].n; lpk = k; continue; }
        ++nsdp;
        ntot += (size_t)p->blk[k].n;
        if (parts > 0) gtot += (size_t)v->rank[k] * (size_t)trials * (size_t)parts;
    }
    lrd_kcut *r = (lrd_kcut *)calloc(1, sizeof *r);
    r->nblk = nsdp; r->parts = parts; r->trials = trials; r->max_rounds = max_rounds; r->src = src; r->seed = seed; r->scale = sc;
    r->tol = tol; r->nlp = nlp;
    r->obj = (double *)zalloc((size_t)trials, sizeof(double));
    r->obj0 = (double *)zalloc((size_t)trials, sizeof(double));
    r->lp_upper = (double *)zalloc((size_t)nlp, sizeof(double));
    r->cone = (lrd_kcut_cone *)zalloc((size_t)nsdp, sizeof(lrd_kcut_cone));
    uint8_t *label = (uint8_t *)zalloc(ntot, 1);
    double *t = (double *)zalloc(ntot, sizeof(double));
    /* (the backend validates parts and trials x parts before it writes anything: g is never written when it refuses) */
    double *g = with_vectors && parts >= 2 && parts <= 64 && (int64_t)trials * parts <= (1 << 20) ? (double *)zalloc(gtot, sizeof(double)) : NULL;
    int rc = be->round_kcut(be->ctx, src, parts, trials, seed, max_rounds, r->obj, r->obj0, &r->best, &r->best0, label, &r->rounds, g, t,
                            r->lp_upper);
    if (rc) {
        free(label); free(t); free(g);
        lrd_kcut_free(r);
        return rc;
    }
    for (int i = 0; i < trials; ++i) { r->obj[i] /= sc; r->obj0[i] /= sc; }
    r->f_best = r->obj[r->best];
    r->f_best0 = r->obj0[r->best0];
    size_t at = 0, gat = 0;
    int kc = 0;
    for (int k = 0; k < p->nblk; ++k) {
        const lrd_block *b = &p->blk[k];
        if (b->is_lp) continue;
        lrd_kcut_cone *q = &r->cone[kc++];
        const int n = b->n;
        q->blk = k; q->n = n; q->rank = v->rank[k];
        q->label = (uint8_t *)zalloc((size_t)n, 1);
        q->t = (double *)zalloc((size_t)n, sizeof(double));
        q->size = (int *)zalloc((size_t)parts, sizeof(int));
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
    int *blk = (int *)zalloc((size_t)nsdp, sizeof(int));
    double *T = (double *)zalloc(2 * (size_t)(nsdp > 0 ? nsdp : 1), sizeof(double)), *lm = T + (nsdp > 0 ? nsdp : 1);
    for (int i = 0; i < nsdp; ++i) { blk[i] = r->cone[i].blk; T[i] = r->cone[i].T; }
    lrd_dual_bound db;
    rc = lrd_rounded_dual_bound(be, src, tol, sc, p->nblk, nsdp, blk, T, lpk, nlp, r->lp_upper, r->f_best, &db, lm);
    r->by = db.by; r->bound = db.bound; r->gap = db.gap; r->lp_neg = db.lp_neg;
    for (int i = 0; i < nsdp; ++i) r->cone[i].lam_min = lm[i];
    free(blk); free(T);
    if (rc) { lrd_kcut_free(r); return 1; }
    *out = r;
    return 0;
}
