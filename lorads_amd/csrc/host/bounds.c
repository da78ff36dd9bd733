/* bounds.c -- separation of entry bounds lower <= X_pq <= upper on the primal and the problem file with the violated ones added
 * (DESIGN.md section 15).  The enumeration is the backend's (lrd_backend.entry_bounds) and the session-level driver separation.c's;
 * here: the list, its order and its slot call, and the bounded problem -- the validation of a list and the rows it becomes, one
 * constraint and one slack column per cut, handed to separation.c's writer. */
#include "lorads_host.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

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

static int bound_cone(lrd_backend *be, void *list, int src, int k, int at, int64_t *count, int *got, int *np) {
    lrd_bounds *c = (lrd_bounds *)list;
    return be->entry_bounds(be->ctx, src, k, c->lower, c->upper, c->min_violation, c->max_cuts, count, c->p + at, c->q + at, c->cls + at,
                            c->viol + at, got, np);
}

int lrd_session_entry_bounds(lrd_session *s, double lower, double upper, double min_violation, int max_cuts, lrd_bounds **out) {
    lrd_backend *be = lrd_session_backend(s);
    lrd_bounds *c = (lrd_bounds *)calloc(1, sizeof *c);
    c->lower = lower; c->upper = upper; c->min_violation = min_violation;
    c->max_cuts = max_cuts;
    const lrd_separation sp = {c, bound_before, bound_cone, &c->nblk, &c->src, &c->kept, &c->passes, &c->count, 5,
                               {{&c->cone, sizeof(int)}, {&c->p, sizeof(int)}, {&c->q, sizeof(int)}, {&c->cls, sizeof(int8_t)},
                                {&c->viol, sizeof(double)}}};
    *out = NULL;
    const int rc = lrd_session_separate(s, be && be->entry_bounds, "separate entry bounds", 0, max_cuts, &sp); /* (no LP block gets the call) */
    if (rc) { lrd_bounds_free(c); return rc; }
    c->bound = (double *)lrd_zalloc((size_t)c->kept, sizeof(double));
    for (int e = 0; e < c->kept; ++e) c->bound[e] = c->cls[e] ? upper : lower;
    *out = c;
    return 0;
}

int lrd_session_write_bounded(lrd_session *s, const char *path, const lrd_bounds *bounds) {
    const lrd_problem *pr = lrd_session_problem(s);
    if (!pr || !path) return 1;
    if (pr->separable || pr->nblk != pr->nblk_global) return 3;
    const int ncut = bounds ? bounds->kept : 0, nb = pr->nblk;
    int nlp = 0; /* (the slack columns join the one LP block, or form a new last one) */
    for (int k = 0; k < nb; ++k) nlp += pr->blk[k].is_lp;
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
    /* the cuts: X_pq -+ slack = bound */
    lrd_new_row *row = (lrd_new_row *)lrd_zalloc((size_t)ncut, sizeof *row);
    for (int e = 0; e < ncut; ++e) {
        const lrd_new_row r = {bounds->bound[e], bounds->cls[e] ? 1.0 : -1.0, 1, {{bounds->cone[e], bounds->p[e], bounds->q[e], 0.5}}};
        row[e] = r;
    }
    const lrd_extension ext = {ncut, row, NULL, NULL};
    const int rc = lrd_write_extended(path, pr, &ext);
    free(row);
    return rc;
}
