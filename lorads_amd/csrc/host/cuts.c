/* cuts.c -- separation of the triangle inequalities of a +-1-structured problem and the tightened problem file (DESIGN.md
 * section 14).  The enumeration is the backend's (lrd_backend.triangle_cuts) and the session-level driver separation.c's; here: the
 * list, its order and its slot call, and the tightened problem -- the validation of a cut list and the rows it becomes, one constraint
 * and one slack column per cut, handed to separation.c's writer.  A tightened problem can be tightened again:
 * the recogniser of the cuts it holds (lrd_session_present_cuts), the duplicate check and the mask of the cuts that leave. */
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

static int cut_cone(lrd_backend *be, void *list, int src, int k, int at, int64_t *count, int *got, int *np) {
    lrd_cuts *c = (lrd_cuts *)list;
    return be->triangle_cuts(be->ctx, src, k, c->min_violation, c->max_cuts, count, c->p + at, c->q + at, c->s + at, c->cls + at,
                             c->viol + at, got, np);
}

int lrd_session_triangle_cuts(lrd_session *s, double min_violation, int max_cuts, lrd_cuts **out) {
    lrd_backend *be = lrd_session_backend(s);
    lrd_cuts *c = (lrd_cuts *)calloc(1, sizeof *c);
    c->min_violation = min_violation;
    c->max_cuts = max_cuts;
    const lrd_separation sp = {c, cut_before, cut_cone, &c->nblk, &c->src, &c->kept, &c->passes, &c->count, 6,
                               {{&c->cone, sizeof(int)}, {&c->p, sizeof(int)}, {&c->q, sizeof(int)}, {&c->s, sizeof(int)},
                                {&c->cls, sizeof(int8_t)}, {&c->viol, sizeof(double)}}};
    /* (an LP block beside the cones holds the slacks of a cut-tightened problem and is passed over: count 0) */
    const int rc = lrd_session_separate(s, be && be->triangle_cuts, "separate triangle inequalities", 1, max_cuts, &sp);
    *out = rc ? NULL : c;
    if (rc) lrd_cuts_free(c);
    return rc;
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

int lrd_session_write_tightened_keep(lrd_session *s, const char *path, const lrd_cuts *cuts, const unsigned char *keep, int nkeep) {
    const lrd_problem *pr = lrd_session_problem(s);
    if (!pr || !path) return 1;
    if (pr->separable || pr->nblk != pr->nblk_global) return 3;
    const int ncut = cuts ? cuts->kept : 0, nb = pr->nblk;
    int has_lp = 0;
    for (int k = 0; k < nb; ++k) has_lp |= pr->blk[k].is_lp;
    lrd_present *P = NULL; /* the cuts the problem holds, where there is something to append to them or to drop from them */
    if (has_lp && (ncut > 0 || keep) && present_cuts(pr, &P)) {
        fprintf(stderr, "lorads: a problem with an LP block cannot take cuts: %s\n", cuts_why);
        return 2;
    }
    const int npres = P ? P->n : 0;
    char why[sizeof cuts_why] = "";
    if (keep && nkeep != npres) {
        if (P) snprintf(why, sizeof why, "the keep mask has %d entries, the problem %d cuts", nkeep, npres);
        else snprintf(why, sizeof why, "a keep mask for a problem without cuts");
    }
    double **t = (double **)lrd_zalloc((size_t)nb, sizeof(double *));
    for (int e = 0; e < ncut && !why[0]; ++e) {
        const int k = cuts->cone[e], p = cuts->p[e], q = cuts->q[e], r = cuts->s[e];
        if (k < 0 || k >= nb || pr->blk[k].is_lp || !(0 <= p && p < q && q < r && r < pr->blk[k].n) || cuts->cls[e] < 0 || cuts->cls[e] > 3) {
            snprintf(why, sizeof why, "a cut is outside the problem");
            break;
        }
        if (!t[k]) t[k] = cone_t(pr, k);
        if (!(t[k][p] > 0) || !(t[k][q] > 0) || !(t[k][r] > 0)) snprintf(why, sizeof why, "a cut names a row whose diagonal no constraint fixes");
    }
    if (P && !why[0]) { /* a new cut that the problem keeps, or that is listed twice (x[5]: new) */
        int *key = (int *)lrd_zalloc((size_t)(npres + ncut), 6 * sizeof(int)), nkey = 0;
        for (int e = 0; e < npres; ++e) {
            if (keep && !keep[e]) continue;
            int *x = key + 6 * (size_t)nkey++;
            x[0] = P->cone[e]; x[1] = P->p[e]; x[2] = P->q[e]; x[3] = P->s[e]; x[4] = P->cls[e]; x[5] = 0;
        }
        for (int e = 0; e < ncut; ++e) {
            int *x = key + 6 * (size_t)nkey++;
            x[0] = cuts->cone[e]; x[1] = cuts->p[e]; x[2] = cuts->q[e]; x[3] = cuts->s[e]; x[4] = cuts->cls[e]; x[5] = 1;
        }
        qsort(key, (size_t)nkey, 6 * sizeof(int), key_cmp);
        for (int e = 1; e < nkey && !why[0]; ++e) {
            const int *x = key + 6 * (size_t)e;
            if (key_cmp(x, x - 6) == 0 && (x[5] || x[-1]))
                snprintf(why, sizeof why, "a cut is already in the problem: cone %d, (%d, %d, %d), class %d", x[0] + 1, x[1] + 1, x[2] + 1,
                         x[3] + 1, x[4]);
        }
        free(key);
    }
    int rc = 2;
    if (why[0]) {
        fprintf(stderr, "lorads: %s\n", why);
        if (P) memcpy(cuts_why, why, sizeof why); /* (lrd_cuts_why() speaks of cut-tightened problems alone) */
    } else {
        /* the cuts: sum of sign_xy X_xy / (t_x t_y) - slack = -1; the present cuts with keep[e] == 0 leave with their rows and columns */
        lrd_new_row *row = (lrd_new_row *)lrd_zalloc((size_t)ncut, sizeof *row);
        for (int e = 0; e < ncut; ++e) {
            const int k = cuts->cone[e], x[3] = {cuts->p[e], cuts->q[e], cuts->s[e]};
            const int *sg = cut_sign[cuts->cls[e]];
            const int pair[3][2] = {{0, 1}, {0, 2}, {1, 2}};
            row[e].rhs = row[e].slack = -1.0;
            row[e].nent = 3;
            for (int w = 0; w < 3; ++w) {
                const int a = x[pair[w][0]], c = x[pair[w][1]];
                row[e].ent[w].cone = k; row[e].ent[w].i = a; row[e].ent[w].j = c;
                row[e].ent[w].value = (double)sg[w] / (2.0 * (t[k][a] * t[k][c]));
            }
        }
        unsigned char *drop_row = P ? (unsigned char *)lrd_zalloc((size_t)pr->m, 1) : NULL;
        unsigned char *drop_col = P ? (unsigned char *)lrd_zalloc((size_t)pr->blk[P->lpk].n, 1) : NULL;
        for (int e = 0; e < npres && keep; ++e)
            if (!keep[e]) drop_row[P->row[e]] = drop_col[P->col[e]] = 1;
        const lrd_extension ext = {ncut, row, drop_row, drop_col};
        rc = lrd_write_extended(path, pr, &ext);
        free(row); free(drop_row); free(drop_col);
    }
    for (int k = 0; k < nb; ++k) free(t[k]);
    free(t);
    lrd_present_free(P);
    return rc;
}

int lrd_session_write_tightened(lrd_session *s, const char *path, const lrd_cuts *cuts) {
    return lrd_session_write_tightened_keep(s, path, cuts, NULL, 0);
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
