/* cuts.c -- separation of the triangle inequalities of a +-1-structured problem and the tightened problem file (DESIGN.md
 * section 14).  The enumeration is the backend's (lrd_backend.triangle_cuts); here: the session-level driver that merges the cones'
 * lists (lrd_merge_runs, shared with bounds.c like lrd_write_problem_as_read), and the writer of the problem with one constraint and one slack column per cut, a pure function of the problem image and
 * the cut list (so the format can be checked without a GPU). */
#include "lorads_host.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* coefficients of rho_pq, rho_ps, rho_qs in the four classes */
static const int cut_sign[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};

void lrd_cuts_free(lrd_cuts *c) {
    if (!c) return;
    free(c->count); free(c->cone); free(c->p); free(c->q); free(c->s); free(c->cls); free(c->viol);
    free(c);
}

int lrd_merge_runs(const void *list, int (*before)(const void *list, int a, int b), const lrd_column *col, int ncol, int at, int got,
                   int max_cuts) {
    const int tot = at + got, keep = tot < max_cuts ? tot : max_cuts;
    size_t wide = 1;
    for (int w = 0; w < ncol; ++w) wide = col[w].size > wide ? col[w].size : wide;
    int *order = (int *)malloc((size_t)(keep > 0 ? keep : 1) * sizeof(int));
    char *tmp = (char *)malloc((size_t)(keep > 0 ? keep : 1) * wide);
    for (int i = 0, j = at, n = 0; n < keep;) {
        if (j >= tot || (i < at && before(list, i, j))) order[n++] = i++;
        else order[n++] = j++;
    }
    for (int w = 0; w < ncol; ++w) {
        const size_t sz = col[w].size;
        for (int e = 0; e < keep; ++e) memcpy(tmp + (size_t)e * sz, (const char *)col[w].base + (size_t)order[e] * sz, sz);
        memcpy(col[w].base, tmp, (size_t)keep * sz);
    }
    free(order); free(tmp);
    return keep;
}

void lrd_write_problem_as_read(FILE *f, const lrd_problem *pr) {
    for (int k = 0; k < pr->nblk; ++k) {
        const lrd_block *b = &pr->blk[k];
        for (int e = 0; e < b->c_nnz; ++e) fprintf(f, "0 %d %d %d %.17g\n", k + 1, b->c_col[e] + 1, b->c_row[e] + 1, -b->c_val[e]);
    }
    for (int k = 0; k < pr->nblk; ++k) {
        const lrd_block *b = &pr->blk[k];
        for (int i = 0; i < b->nrow; ++i)
            for (int e = b->a_ptr[i]; e < b->a_ptr[i + 1]; ++e)
                fprintf(f, "%d %d %d %d %.17g\n", b->row_idx[i] + 1, k + 1, b->a_col[e] + 1, b->a_row[e] + 1, b->a_val[e]);
    }
}

/* is a before b in (v descending, cone, p, q, s, class ascending)? */
static int cut_before(const void *list, int a, int b) {
    const lrd_cuts *c = (const lrd_cuts *)list;
    if (c->viol[a] != c->viol[b]) return c->viol[a] > c->viol[b];
    if (c->cone[a] != c->cone[b]) return c->cone[a] < c->cone[b];
    if (c->p[a] != c->p[b]) return c->p[a] < c->p[b];
    if (c->q[a] != c->q[b]) return c->q[a] < c->q[b];
    if (c->s[a] != c->s[b]) return c->s[a] < c->s[b];
    return c->cls[a] < c->cls[b];
}

int lrd_session_triangle_cuts(lrd_session *s, double min_violation, int max_cuts, lrd_cuts **out) {
    *out = NULL;
    lrd_backend *be = lrd_session_backend(s);
    int src;
    const int refused = lrd_session_postsolve(s, be && be->triangle_cuts, "separate triangle inequalities",
                                              "the separation of a sharded deal (world > 1) is", NULL, NULL, &src);
    if (refused) return refused;
    const int nb = lrd_session_problem(s)->nblk, cap = max_cuts > 0 ? max_cuts : 1;
    lrd_cuts *c = (lrd_cuts *)calloc(1, sizeof *c);
    c->nblk = nb;
    c->src = src;
    c->min_violation = min_violation;
    c->max_cuts = max_cuts;
    c->count = (int64_t *)calloc((size_t)(nb > 0 ? nb : 1), sizeof(int64_t));
    /* room for the merged list and one cone's list behind it */
    c->cone = (int *)calloc(2 * (size_t)cap, sizeof(int));
    c->p = (int *)calloc(2 * (size_t)cap, sizeof(int));
    c->q = (int *)calloc(2 * (size_t)cap, sizeof(int));
    c->s = (int *)calloc(2 * (size_t)cap, sizeof(int));
    c->cls = (int8_t *)calloc(2 * (size_t)cap, sizeof(int8_t));
    c->viol = (double *)calloc(2 * (size_t)cap, sizeof(double));
    const lrd_column col[6] = {{c->cone, sizeof(int)}, {c->p, sizeof(int)}, {c->q, sizeof(int)}, {c->s, sizeof(int)},
                               {c->cls, sizeof(int8_t)}, {c->viol, sizeof(double)}};
    int rc = 0;
    for (int k = 0; k < nb && !rc; ++k) {
        const int at = c->kept;
        int got = 0, np = 0;
        rc = be->triangle_cuts(be->ctx, c->src, k, min_violation, max_cuts, &c->count[k], c->p + at, c->q + at, c->s + at, c->cls + at,
                               c->viol + at, &got, &np);
        if (rc) break;
        c->passes += np;
        for (int e = 0; e < got; ++e) c->cone[at + e] = k;
        c->kept = lrd_merge_runs(c, cut_before, col, 6, at, got, max_cuts);
    }
    if (rc) { lrd_cuts_free(c); return rc; }
    *out = c;
    return 0;
}

/* t_p = sqrt(b_i / a_i) of the one constraint a_i X[p,p] = b_i on diagonal p of cone k; 0 where no such constraint is found */
static double *cone_t(const lrd_problem *pr, int k) {
    const lrd_block *b = &pr->blk[k];
    double *t = (double *)calloc((size_t)(b->n > 0 ? b->n : 1), sizeof(double));
    for (int i = 0; i < b->nrow; ++i) {
        if (b->a_ptr[i + 1] - b->a_ptr[i] != 1) continue;
        const int e = b->a_ptr[i];
        if (b->a_row[e] != b->a_col[e]) continue;
        const double ratio = pr->b[b->row_idx[i]] / b->a_val[e];
        if (ratio > 0 && isfinite(ratio)) t[b->a_row[e]] = sqrt(ratio);
    }
    return t;
}

int lrd_session_write_tightened(lrd_session *s, const char *path, const lrd_cuts *cuts) {
    const lrd_problem *pr = lrd_session_problem(s);
    if (!pr || !path) return 1;
    if (pr->separable || pr->nblk != pr->nblk_global) return 3;
    const int ncut = cuts ? cuts->kept : 0, nb = pr->nblk;
    for (int k = 0; k < nb && ncut > 0; ++k)
        if (pr->blk[k].is_lp) {
            fprintf(stderr, "lorads: a problem with an LP block cannot take cuts\n");
            return 2;
        }
    double **t = (double **)calloc((size_t)(nb > 0 ? nb : 1), sizeof(double *));
    int bad = 0;
    for (int e = 0; e < ncut && !bad; ++e) {
        const int k = cuts->cone[e], p = cuts->p[e], q = cuts->q[e], r = cuts->s[e];
        if (k < 0 || k >= nb || !(0 <= p && p < q && q < r && r < pr->blk[k].n) || cuts->cls[e] < 0 || cuts->cls[e] > 3) { bad = 1; break; }
        if (!t[k]) t[k] = cone_t(pr, k);
        if (!(t[k][p] > 0) || !(t[k][q] > 0) || !(t[k][r] > 0)) bad = 2;
    }
    FILE *f = bad ? NULL : fopen(path, "w");
    if (!f) {
        if (bad) fprintf(stderr, bad == 1 ? "lorads: a cut is outside the problem\n" : "lorads: a cut names a row whose diagonal no constraint fixes\n");
        for (int k = 0; k < nb; ++k) free(t[k]);
        free(t);
        return bad ? 2 : 1;
    }
    fprintf(f, "%d\n%d\n", pr->m + ncut, nb + (ncut > 0 ? 1 : 0));
    for (int k = 0; k < nb; ++k) fprintf(f, "%s%d", k ? " " : "", pr->blk[k].is_lp ? -pr->blk[k].n : pr->blk[k].n);
    if (ncut > 0) fprintf(f, " %d", -ncut);
    fputc('\n', f);
    for (int i = 0; i < pr->m; ++i) fprintf(f, "%s%.17g", i ? " " : "", pr->b[i]);
    for (int e = 0; e < ncut; ++e) fprintf(f, "%s-1", pr->m + e ? " " : "");
    fputc('\n', f);
    lrd_write_problem_as_read(f, pr);
    /* the cuts: sum of sign_xy X_xy / (t_x t_y) - slack = -1; an off-diagonal entry counts twice in <A, X> */
    for (int e = 0; e < ncut; ++e) {
        const int k = cuts->cone[e], x[3] = {cuts->p[e], cuts->q[e], cuts->s[e]};
        const int *sg = cut_sign[cuts->cls[e]];
        const int pair[3][2] = {{0, 1}, {0, 2}, {1, 2}};
        for (int w = 0; w < 3; ++w) {
            const int a = x[pair[w][0]], c = x[pair[w][1]];
            fprintf(f, "%d %d %d %d %.17g\n", pr->m + e + 1, k + 1, a + 1, c + 1, (double)sg[w] / (2.0 * (t[k][a] * t[k][c])));
        }
        fprintf(f, "%d %d %d %d -1\n", pr->m + e + 1, nb + 1, e + 1, e + 1);
    }
    for (int k = 0; k < nb; ++k) free(t[k]);
    free(t);
    return fclose(f) ? 1 : 0;
}
