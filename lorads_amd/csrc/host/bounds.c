/* bounds.c -- separation of entry bounds lower <= X_pq <= upper on the primal and the problem file with the violated ones added
 * (DESIGN.md section 15).  The enumeration is the backend's (lrd_backend.entry_bounds); here: the session-level driver that merges the
 * cones' lists (cuts.c: lrd_merge_runs), and the writer of the problem with one constraint and one slack column per cut, a pure function of the problem
 * image and the list (so the format can be checked without a GPU). */
#include "lorads_host.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void lrd_bounds_free(lrd_bounds *c) {
    if (!c) return;
    free(c->count); free(c->cone); free(c->p); free(c->q); free(c->cls); free(c->viol); free(c->bound);
    free(c);
}

/* is a before b in (v descending, cone, p, q, class ascending)? */
static int bound_before(const void *list, int a, int b) {
    const lrd_bounds *c = (const lrd_bounds *)list;
    if (c->viol[a] != c->viol[b]) return c->viol[a] > c->viol[b];
    if (c->cone[a] != c->cone[b]) return c->cone[a] < c->cone[b];
    if (c->p[a] != c->p[b]) return c->p[a] < c->p[b];
    if (c->q[a] != c->q[b]) return c->q[a] < c->q[b];
    return c->cls[a] < c->cls[b];
}

int lrd_session_entry_bounds(lrd_session *s, double lower, double upper, double min_violation, int max_cuts, lrd_bounds **out) {
    *out = NULL;
    lrd_backend *be = lrd_session_backend(s);
    int src;
    const int refused = lrd_session_postsolve(s, be && be->entry_bounds, "separate entry bounds",
                                              "the separation of a sharded deal (world > 1) is", NULL, NULL, &src);
    if (refused) return refused;
    const lrd_problem *pr = lrd_session_problem(s);
    const int nb = pr->nblk, cap = max_cuts > 0 ? max_cuts : 1;
    lrd_bounds *c = (lrd_bounds *)calloc(1, sizeof *c);
    c->nblk = nb;
    c->src = src;
    c->lower = lower; c->upper = upper; c->min_violation = min_violation;
    c->max_cuts = max_cuts;
    c->count = (int64_t *)calloc((size_t)(nb > 0 ? nb : 1), sizeof(int64_t));
    /* room for the merged list and one cone's list behind it */
    c->cone = (int *)calloc(2 * (size_t)cap, sizeof(int));
    c->p = (int *)calloc(2 * (size_t)cap, sizeof(int));
    c->q = (int *)calloc(2 * (size_t)cap, sizeof(int));
    c->cls = (int8_t *)calloc(2 * (size_t)cap, sizeof(int8_t));
    c->viol = (double *)calloc(2 * (size_t)cap, sizeof(double));
    c->bound = (double *)calloc(2 * (size_t)cap, sizeof(double));
    const lrd_column col[5] = {{c->cone, sizeof(int)}, {c->p, sizeof(int)}, {c->q, sizeof(int)}, {c->cls, sizeof(int8_t)},
                               {c->viol, sizeof(double)}};
    int rc = 0;
    for (int k = 0; k < nb && !rc; ++k) {
        if (pr->blk[k].is_lp) continue;
        const int at = c->kept;
        int got = 0, np = 0;
        rc = be->entry_bounds(be->ctx, c->src, k, lower, upper, min_violation, max_cuts, &c->count[k], c->p + at, c->q + at, c->cls + at,
                              c->viol + at, &got, &np);
        if (rc) break;
        c->passes += np;
        for (int e = 0; e < got; ++e) c->cone[at + e] = k;
        c->kept = lrd_merge_runs(c, bound_before, col, 5, at, got, max_cuts);
    }
    if (rc) { lrd_bounds_free(c); return rc; }
    for (int e = 0; e < c->kept; ++e) c->bound[e] = c->cls[e] ? upper : lower;
    *out = c;
    return 0;
}

int lrd_session_write_bounded(lrd_session *s, const char *path, const lrd_bounds *bounds) {
    const lrd_problem *pr = lrd_session_problem(s);
    if (!pr || !path) return 1;
    if (pr->separable || pr->nblk != pr->nblk_global) return 3;
    const int ncut = bounds ? bounds->kept : 0, nb = pr->nblk;
    int lp = -1, nlp = 0; /* the LP block the slack columns join (-1: a new last one) */
    for (int k = 0; k < nb; ++k)
        if (pr->blk[k].is_lp) { lp = k; ++nlp; }
    if (nlp > 1 && ncut > 0) {
        fprintf(stderr, "lorads: a problem with more than one LP block cannot take bound cuts\n");
        return 2;
    }
    for (int e = 0; e < ncut; ++e) {
        const int k = bounds->cone[e], p = bounds->p[e], q = bounds->q[e];
        if (k < 0 || k >= nb || pr->blk[k].is_lp || !(0 <= p && p < q && q < pr->blk[k].n) || bounds->cls[e] < 0 || bounds->cls[e] > 1 ||
            !isfinite(bounds->bound[e])) {
            fprintf(stderr, "lorads: a bound cut is outside the problem\n");
            return 2;
        }
    }
    FILE *f = fopen(path, "w");
    if (!f) return 1;
    const int new_block = ncut > 0 && lp < 0;
    const int col0 = ncut > 0 && lp >= 0 ? pr->blk[lp].n : 0; /* the first slack column, 0-based */
    fprintf(f, "%d\n%d\n", pr->m + ncut, nb + new_block);
    for (int k = 0; k < nb; ++k) {
        const int n = pr->blk[k].n + (ncut > 0 && k == lp ? ncut : 0);
        fprintf(f, "%s%d", k ? " " : "", pr->blk[k].is_lp ? -n : n);
    }
    if (new_block) fprintf(f, "%s%d", nb ? " " : "", -ncut);
    fputc('\n', f);
    for (int i = 0; i < pr->m; ++i) fprintf(f, "%s%.17g", i ? " " : "", pr->b[i]);
    for (int e = 0; e < ncut; ++e) fprintf(f, "%s%.17g", pr->m + e ? " " : "", bounds->bound[e]);
    fputc('\n', f);
    lrd_write_problem_as_read(f, pr);
    /* the cuts: X_pq -+ slack = bound; an off-diagonal entry counts twice in <A, X> */
    const int sblk = lp >= 0 ? lp + 1 : nb + 1;
    for (int e = 0; e < ncut; ++e) {
        fprintf(f, "%d %d %d %d 0.5\n", pr->m + e + 1, bounds->cone[e] + 1, bounds->p[e] + 1, bounds->q[e] + 1);
        fprintf(f, "%d %d %d %d %d\n", pr->m + e + 1, sblk, col0 + e + 1, col0 + e + 1, bounds->cls[e] ? 1 : -1);
    }
    return fclose(f) ? 1 : 0;
}
