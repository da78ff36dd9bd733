/* cuts.c -- separation of the triangle inequalities of a +-1-structured problem and the tightened problem file (DESIGN.md
 * section 14).  The enumeration is the backend's (lrd_backend.triangle_cuts); here: the session-level driver that merges the cones'
 * lists (lrd_merge_runs, shared with bounds.c like lrd_write_problem_as_read), and the writer of the problem with one constraint and one slack column per cut, a pure function of the problem image and
 * the cut list (so the format can be checked without a GPU).  A tightened problem can be tightened again: the
 * recogniser of the cuts it holds (lrd_session_present_cuts) and the writer that appends to and drops from them. */
#include "lorads_host.h"
#include "lorads_cut_rows.h"

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
        if (lrd_session_problem(s)->blk[k].is_lp && nb > 1) continue; /* (the slacks of a cut-tightened problem: count 0) */
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

/* ---- the cut-tightened structure on the host: the recogniser of include/lorads_cut_rows.h over the problem image */
static char cuts_why[384];
const char *lrd_cuts_why(void) { return cuts_why; }

void lrd_present_free(lrd_present *c) {
    if (!c) return;
    free(c->cone); free(c->p); free(c->q); free(c->s); free(c->cls); free(c->row); free(c->col); free(c->scale); free(c->t);
    free(c);
}

/* 0 and *out (lpk = -1 and no cuts without an LP block), or 2 with the reason in cuts_why */
static int present_cuts(const lrd_problem *pr, lrd_present **out) {
    *out = NULL;
    cuts_why[0] = 0;
    const int nb = pr->nblk, m = pr->m;
    lrd_present *c = (lrd_present *)calloc(1, sizeof *c);
    c->lpk = -1;
    int nlp = 0;
    for (int k = 0; k < nb; ++k)
        if (pr->blk[k].is_lp) { c->lpk = k; ++nlp; }
    if (nlp == 0) { *out = c; return 0; }
    if (nlp > 1) {
        snprintf(cuts_why, sizeof cuts_why, "block %d is an LP block: more than one LP block", c->lpk + 1);
        lrd_present_free(c);
        return 2;
    }
    int *ptr = (int *)calloc((size_t)m + 2, sizeof(int)), *dim = (int *)calloc((size_t)nb, sizeof(int));
    int *t_off = (int *)calloc((size_t)nb + 1, sizeof(int));
    for (int k = 0; k < nb; ++k) {
        const lrd_block *b = &pr->blk[k];
        dim[k] = b->n;
        t_off[k + 1] = t_off[k] + b->n;
        for (int i = 0; i < b->nrow; ++i) ptr[b->row_idx[i] + 2] += b->a_ptr[i + 1] - b->a_ptr[i];
    }
    for (int i = 0; i < m; ++i) ptr[i + 2] += ptr[i + 1];
    lrd_cr_entry *ent = (lrd_cr_entry *)calloc((size_t)(ptr[m + 1] > 0 ? ptr[m + 1] : 1), sizeof *ent);
    for (int k = 0; k < nb; ++k) { /* block after block: a constraint's entries in block order (ptr + 1: the fill cursors) */
        const lrd_block *b = &pr->blk[k];
        for (int i = 0; i < b->nrow; ++i)
            for (int e = b->a_ptr[i]; e < b->a_ptr[i + 1]; ++e) {
                const lrd_cr_entry x = {k, b->a_row[e], b->a_col[e], b->a_val[e]};
                ent[ptr[b->row_idx[i] + 1]++] = x;
            }
    }
    const lrd_block *L = &pr->blk[c->lpk];
    double *obj = (double *)calloc((size_t)(L->n > 0 ? L->n : 1), sizeof(double));
    for (int e = 0; e < L->c_nnz; ++e) obj[L->c_row[e]] = L->c_val[e];
    c->cone = (int *)lrd_zalloc((size_t)m, sizeof(int)); c->p = (int *)lrd_zalloc((size_t)m, sizeof(int));
    c->q = (int *)lrd_zalloc((size_t)m, sizeof(int)); c->s = (int *)lrd_zalloc((size_t)m, sizeof(int));
    c->cls = (int *)lrd_zalloc((size_t)m, sizeof(int)); c->row = (int *)lrd_zalloc((size_t)m, sizeof(int));
    c->col = (int *)lrd_zalloc((size_t)m, sizeof(int)); c->scale = (double *)lrd_zalloc((size_t)m, sizeof(double));
    c->t = (double *)lrd_zalloc((size_t)t_off[nb], sizeof(double));
    lrd_cr_cut *cut = (lrd_cr_cut *)lrd_zalloc((size_t)m, sizeof *cut);
    double *u = (double *)lrd_zalloc((size_t)L->n, sizeof(double));
    const lrd_cr_problem P = {m, nb, c->lpk, dim, ptr, ent, pr->b, obj};
    char why[256];
    const int bad = lrd_cr_check(&P, t_off, c->t, cut, &c->n, u, why, sizeof why);
    for (int e = 0; e < c->n && !bad; ++e) {
        c->cone[e] = cut[e].cone; c->p[e] = cut[e].p; c->q[e] = cut[e].q; c->s[e] = cut[e].s; c->cls[e] = cut[e].cls;
        c->row[e] = cut[e].row; c->col[e] = cut[e].col; c->scale[e] = cut[e].scale;
    }
    free(ptr); free(dim); free(t_off); free(ent); free(obj); free(cut); free(u);
    if (bad) {
        snprintf(cuts_why, sizeof cuts_why, "block %d is an LP block whose columns are not all triangle-cut slacks: %s", c->lpk + 1, why);
        lrd_present_free(c);
        return 2;
    }
    *out = c;
    return 0;
}

int lrd_session_present_cuts(lrd_session *s, lrd_present **out) {
    const lrd_problem *pr = lrd_session_problem(s);
    *out = NULL;
    if (!pr) return 1;
    if (pr->separable || pr->nblk != pr->nblk_global) return 3;
    return present_cuts(pr, out);
}

/* is cut a before cut b in (cone, p, q, s, class)?  x = {cone, p, q, s, cls} */
static int key_cmp(const void *a, const void *b) {
    const int *x = (const int *)a, *y = (const int *)b;
    for (int w = 0; w < 5; ++w)
        if (x[w] != y[w]) return x[w] < y[w] ? -1 : 1;
    return 0;
}

/* The tightened problem of a cut-tightened one: the present cuts with keep[e] == 0 leave with their rows and columns, the others are
 * renumbered in order, the new cuts follow as rows and as columns of the LP block, which stays where it is. */
static int write_appended(const lrd_problem *pr, const char *path, const lrd_cuts *cuts, const unsigned char *keep, int nkeep) {
    lrd_present *P = NULL;
    if (present_cuts(pr, &P)) {
        fprintf(stderr, "lorads: a problem with an LP block cannot take cuts: %s\n", cuts_why);
        return 2;
    }
    const int ncut = cuts ? cuts->kept : 0, nb = pr->nblk, lpk = P->lpk, m = pr->m, nl = pr->blk[lpk].n;
    int rc = 0, ndrop = 0;
    if (keep && nkeep != P->n) {
        snprintf(cuts_why, sizeof cuts_why, "the keep mask has %d entries, the problem %d cuts", nkeep, P->n);
        rc = 2;
    }
    int t_off = 0, *toff = (int *)calloc((size_t)nb + 1, sizeof(int));
    for (int k = 0; k < nb; ++k) { toff[k] = t_off; t_off += pr->blk[k].n; }
    int *key = (int *)lrd_zalloc((size_t)(P->n + ncut), 6 * sizeof(int));
    int nkey = 0;
    for (int e = 0; e < P->n && !rc; ++e) {
        if (keep && !keep[e]) { ++ndrop; continue; }
        int *x = key + 6 * (size_t)nkey++;
        x[0] = P->cone[e]; x[1] = P->p[e]; x[2] = P->q[e]; x[3] = P->s[e]; x[4] = P->cls[e]; x[5] = 0;
    }
    for (int e = 0; e < ncut && !rc; ++e) {
        const int k = cuts->cone[e], p = cuts->p[e], q = cuts->q[e], r = cuts->s[e];
        if (k < 0 || k >= nb || k == lpk || !(0 <= p && p < q && q < r && r < pr->blk[k].n) || cuts->cls[e] < 0 || cuts->cls[e] > 3) {
            snprintf(cuts_why, sizeof cuts_why, "a cut is outside the problem");
            rc = 2;
            break;
        }
        int *x = key + 6 * (size_t)nkey++;
        x[0] = k; x[1] = p; x[2] = q; x[3] = r; x[4] = cuts->cls[e]; x[5] = 1;
    }
    if (!rc) {
        qsort(key, (size_t)nkey, 6 * sizeof(int), key_cmp);
        for (int e = 1; e < nkey && !rc; ++e)
            if (key_cmp(key + 6 * (size_t)e, key + 6 * (size_t)(e - 1)) == 0 && (key[6 * (size_t)e + 5] || key[6 * (size_t)(e - 1) + 5])) {
                const int *x = key + 6 * (size_t)e;
                snprintf(cuts_why, sizeof cuts_why, "a cut is already in the problem: cone %d, (%d, %d, %d), class %d", x[0] + 1, x[1] + 1,
                         x[2] + 1, x[3] + 1, x[4]);
                rc = 2;
            }
    }
    free(key);
    FILE *f = rc ? NULL : fopen(path, "w");
    if (!f) {
        if (rc) fprintf(stderr, "lorads: %s\n", cuts_why);
        free(toff);
        lrd_present_free(P);
        return rc ? rc : 1;
    }
    int *rowmap = (int *)lrd_zalloc((size_t)m, sizeof(int)), *colmap = (int *)lrd_zalloc((size_t)nl, sizeof(int));
    for (int e = 0; e < P->n; ++e)
        if (keep && !keep[e]) { rowmap[P->row[e]] = -1; colmap[P->col[e]] = -1; }
    for (int i = 0, at = 0; i < m; ++i) rowmap[i] = rowmap[i] < 0 ? -1 : at++;
    for (int j = 0, at = 0; j < nl; ++j) colmap[j] = colmap[j] < 0 ? -1 : at++;
    const int m2 = m - ndrop, nl2 = nl - ndrop;
    fprintf(f, "%d\n%d\n", m2 + ncut, nb);
    for (int k = 0; k < nb; ++k) fprintf(f, "%s%d", k ? " " : "", k == lpk ? -(nl2 + ncut) : pr->blk[k].n);
    fputc('\n', f);
    for (int i = 0, first = 1; i < m; ++i)
        if (rowmap[i] >= 0) { fprintf(f, "%s%.17g", first ? "" : " ", pr->b[i]); first = 0; }
    for (int e = 0; e < ncut; ++e) fprintf(f, "%s-1", m2 + e ? " " : "");
    fputc('\n', f);
    for (int k = 0; k < nb; ++k) { /* (the LP block of a recognised problem has no objective) */
        const lrd_block *b = &pr->blk[k];
        for (int e = 0; e < b->c_nnz; ++e) fprintf(f, "0 %d %d %d %.17g\n", k + 1, b->c_col[e] + 1, b->c_row[e] + 1, -b->c_val[e]);
    }
    for (int k = 0; k < nb; ++k) {
        const lrd_block *b = &pr->blk[k];
        for (int i = 0; i < b->nrow; ++i)
            for (int e = b->a_ptr[i]; e < b->a_ptr[i + 1] && rowmap[b->row_idx[i]] >= 0; ++e) {
                const int col = k == lpk ? colmap[b->a_col[e]] : b->a_col[e], row = k == lpk ? colmap[b->a_row[e]] : b->a_row[e];
                fprintf(f, "%d %d %d %d %.17g\n", rowmap[b->row_idx[i]] + 1, k + 1, col + 1, row + 1, b->a_val[e]);
            }
    }
    for (int e = 0; e < ncut; ++e) {
        const int k = cuts->cone[e], x[3] = {cuts->p[e], cuts->q[e], cuts->s[e]};
        const int *sg = cut_sign[cuts->cls[e]];
        const int pair[3][2] = {{0, 1}, {0, 2}, {1, 2}};
        const double *t = P->t + toff[k];
        for (int w = 0; w < 3; ++w) {
            const int a = x[pair[w][0]], c = x[pair[w][1]];
            fprintf(f, "%d %d %d %d %.17g\n", m2 + e + 1, k + 1, a + 1, c + 1, (double)sg[w] / (2.0 * (t[a] * t[c])));
        }
        fprintf(f, "%d %d %d %d -1\n", m2 + e + 1, lpk + 1, nl2 + e + 1, nl2 + e + 1);
    }
    free(rowmap); free(colmap); free(toff);
    lrd_present_free(P);
    return fclose(f) ? 1 : 0;
}

int lrd_session_write_tightened(lrd_session *s, const char *path, const lrd_cuts *cuts) {
    return lrd_session_write_tightened_keep(s, path, cuts, NULL, 0);
}

int lrd_session_write_tightened_keep(lrd_session *s, const char *path, const lrd_cuts *cuts, const unsigned char *keep, int nkeep) {
    const lrd_problem *pr = lrd_session_problem(s);
    if (!pr || !path) return 1;
    if (pr->separable || pr->nblk != pr->nblk_global) return 3;
    const int ncut = cuts ? cuts->kept : 0, nb = pr->nblk;
    for (int k = 0; k < nb && (ncut > 0 || keep); ++k)
        if (pr->blk[k].is_lp) return write_appended(pr, path, cuts, keep, nkeep);
    if (keep && nkeep != 0) {
        fprintf(stderr, "lorads: a keep mask for a problem without cuts\n");
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

int lrd_session_write_tightened_drop(lrd_session *s, const char *path, const lrd_cuts *cuts, double drop_slack, double tol, int *dropped) {
    lrd_present *pc = NULL;
    lrd_solution *sol = NULL;
    if (dropped) *dropped = 0;
    int rc = lrd_session_present_cuts(s, &pc);
    if (rc) {
        if (rc == 2) fprintf(stderr, "lorads: a problem with an LP block cannot take cuts: %s\n", cuts_why);
        return rc;
    }
    if (pc->n == 0) {
        lrd_present_free(pc);
        return lrd_session_write_tightened_keep(s, path, cuts, NULL, 0);
    }
    rc = lrd_session_solution(s, tol, &sol);
    if (rc) { lrd_present_free(pc); return rc; }
    unsigned char *keep = (unsigned char *)lrd_zalloc((size_t)pc->n, 1);
    for (int e = 0; e < pc->n; ++e) { /* the slack in the row's rho units: 1 + sum_w sign_w rho_w, zero where the cut is tight */
        keep[e] = !(sol->cone[pc->lpk].x[pc->col[e]] / pc->scale[e] > drop_slack);
        if (dropped && !keep[e]) ++*dropped;
    }
    rc = lrd_session_write_tightened_keep(s, path, cuts, keep, pc->n);
    free(keep);
    lrd_solution_free(sol);
    lrd_present_free(pc);
    return rc;
}
