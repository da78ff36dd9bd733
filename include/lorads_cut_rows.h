/* lorads_cut_rows.h -- the recogniser of the cut-tightened +-1 structure, one text for the device check
 * (csrc/hip/rounding.inc: rnd_check on a context with an LP block) and for the host's (csrc/host/cuts.c: lrd_session_present_cuts,
 * lrd_session_write_tightened_keep), so that both apply one rule and give one first reason.  Plain C that a C++ compiler takes too.
 *
 * A problem with exactly one LP block qualifies when
 *   - every constraint without an LP entry is a_i X_k[p,p] = b_i with b_i / a_i > 0, one per diagonal position of every cone
 *     (t_p = sqrt(b_i / a_i), the +-1 structure's own conditions);
 *   - every constraint with an LP entry is a triangle row: one LP entry c != 0 and three entries a_w of one cone at (p,q), (p,s), (q,s),
 *     p < q < s.  Divided by -c: b~ = b / (-c) < 0, and g_w = 2 (a_w / -c) t_x t_y / (-b~) is +-1 with the signs of one of the four
 *     classes (+,+,+), (+,-,-), (-,+,-), (-,-,+) -- every positive multiple of sum_w g_w rho_w - slack = -1, rho_xy = X_xy / (t_x t_y);
 *   - every LP column lies in exactly one triangle row and has no objective coefficient.
 * The bound on g: the writer forms a_w = g / (2 (t_x t_y)) with two roundings, a multiple of the row adds one each to a_w, c and b, and
 * the check's own a_w / -c, b / -c, two products with t and the last division add six: at most eleven roundings of 2^-53 each, so
 * | |g_w| - 1 | <= 2^-48 (32 of them) holds for every such row and fails for a coefficient that is off by a part in 10^14 or more.
 * The slack of such a row is x_j = -b~ (1 + sum_w g_w rho_w) and |rho| <= 1 on the feasible set, so x_j <= u_j = 4 (-b~). */
#ifndef LORADS_CUT_ROWS_H
#define LORADS_CUT_ROWS_H

#include <math.h>
#include <stddef.h>
#include <stdio.h>

typedef struct { int blk, p, q; double a; } lrd_cr_entry; /* one stored entry (either triangle); an LP entry: p = q = its column */
typedef struct {
    int m, nblk, lpk;         /* lpk: the LP block */
    const int *dim;           /* [nblk] */
    const int *ptr;           /* [m + 1] constraint i's entries are ent[ptr[i] .. ptr[i + 1]) */
    const lrd_cr_entry *ent;
    const double *b;          /* [m] */
    const double *lp_obj;     /* [dim[lpk]] */
} lrd_cr_problem;
/* a present cut: its triple and class, its constraint and LP column (0-based), and scale = -b~ (1 for the written form) */
typedef struct { int cone, p, q, s, cls, row, col; double scale; } lrd_cr_cut;

static const int lrd_cr_sign[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
#define LRD_CR_TOL 0x1p-48

/* 0: the problem qualifies -- t (stacked, cone k at t_off[k]; zero on the LP block), the cuts in constraint order (room for m) and u
 * [dim[lpk]] are filled; 1: it does not, and why holds the first reason.  All numbers in the messages are 1-based. */
static inline int lrd_cr_check(const lrd_cr_problem *P, const int *t_off, double *t, lrd_cr_cut *cuts, int *ncut, double *u, char *why,
                               size_t len) {
    const int lpk = P->lpk, nl = P->dim[lpk];
    *ncut = 0;
    for (int i = 0; i < t_off[P->nblk]; ++i) t[i] = 0.0;
    for (int j = 0; j < nl; ++j) u[j] = 0.0;
    /* the diagonal rows; t doubles as the cover count until they are all seen (a second row on a diagonal is refused at once) */
    for (int i = 0; i < P->m; ++i) {
        const lrd_cr_entry *E = P->ent + P->ptr[i];
        const int ne = P->ptr[i + 1] - P->ptr[i];
        int lp = 0;
        for (int e = 0; e < ne; ++e) lp += E[e].blk == lpk;
        if (lp) continue;
        if (ne != 1) { snprintf(why, len, "constraint %d has %d stored entries", i + 1, ne); return 1; }
        if (E->p != E->q) { snprintf(why, len, "constraint %d is not on a diagonal", i + 1); return 1; }
        const double ratio = P->b[i] / E->a;
        if (!(ratio > 0) || !isfinite(ratio)) { snprintf(why, len, "constraint %d has b / a = %g (not positive)", i + 1, ratio); return 1; }
        if (t[t_off[E->blk] + E->p] != 0.0) {
            snprintf(why, len, "diagonal %d of cone %d is fixed by 2 constraints", E->p + 1, E->blk + 1);
            return 1;
        }
        t[t_off[E->blk] + E->p] = sqrt(ratio);
    }
    for (int k = 0; k < P->nblk; ++k)
        for (int p = 0; k != lpk && p < P->dim[k]; ++p)
            if (t[t_off[k] + p] == 0.0) { snprintf(why, len, "diagonal %d of cone %d is fixed by 0 constraints", p + 1, k + 1); return 1; }
    /* the triangle rows */
    for (int i = 0; i < P->m; ++i) {
        const lrd_cr_entry *E = P->ent + P->ptr[i];
        const int ne = P->ptr[i + 1] - P->ptr[i];
        int lp = 0, ns = 0, x[3][2] = {{0, 0}, {0, 0}, {0, 0}}, cone = -1, j = -1;
        double a[3] = {0, 0, 0}, c = 0.0;
        for (int e = 0; e < ne; ++e) {
            if (E[e].blk == lpk) { ++lp; j = E[e].p; c = E[e].a; continue; }
            if (cone >= 0 && E[e].blk != cone) {
                snprintf(why, len, "constraint %d has entries in cones %d and %d", i + 1, cone + 1, E[e].blk + 1);
                return 1;
            }
            cone = E[e].blk;
            if (ns < 3) { x[ns][0] = E[e].p < E[e].q ? E[e].p : E[e].q; x[ns][1] = E[e].p < E[e].q ? E[e].q : E[e].p; a[ns] = E[e].a; }
            ++ns;
        }
        if (lp == 0) continue;
        if (lp != 1) { snprintf(why, len, "constraint %d has %d LP entries", i + 1, lp); return 1; }
        if (ns != 3) { snprintf(why, len, "constraint %d has an LP entry and %d cone entries, not the 3 of a triangle row", i + 1, ns); return 1; }
        for (int w = 1; w < 3; ++w) /* (p,q) < (p,s) < (q,s) in (row, column) order */
            for (int v = w; v > 0 && (x[v][0] < x[v - 1][0] || (x[v][0] == x[v - 1][0] && x[v][1] < x[v - 1][1])); --v) {
                const int r0 = x[v][0], r1 = x[v][1]; const double av = a[v];
                x[v][0] = x[v - 1][0]; x[v][1] = x[v - 1][1]; a[v] = a[v - 1];
                x[v - 1][0] = r0; x[v - 1][1] = r1; a[v - 1] = av;
            }
        const int p = x[0][0], q = x[0][1], s = x[1][1];
        if (!(p < q && q < s && x[1][0] == p && x[2][0] == q && x[2][1] == s)) {
            snprintf(why, len, "constraint %d has entries at (%d, %d), (%d, %d), (%d, %d): not the three pairs of a triple", i + 1, x[0][0] + 1,
                     x[0][1] + 1, x[1][0] + 1, x[1][1] + 1, x[2][0] + 1, x[2][1] + 1);
            return 1;
        }
        if (c == 0.0) { snprintf(why, len, "constraint %d has a zero LP coefficient", i + 1); return 1; }
        const double bt = P->b[i] / -c;
        if (!(bt < 0) || !isfinite(bt)) { snprintf(why, len, "constraint %d has b / -c = %g (not negative)", i + 1, bt); return 1; }
        int sg[3];
        for (int w = 0; w < 3; ++w) {
            const double g = 2.0 * (a[w] / -c) * t[t_off[cone] + x[w][0]] * t[t_off[cone] + x[w][1]] / -bt;
            if (!(fabs(fabs(g) - 1.0) <= LRD_CR_TOL)) {
                snprintf(why, len, "constraint %d has a coefficient at (%d, %d) that is not +-1 of a triangle row's", i + 1, x[w][0] + 1,
                         x[w][1] + 1);
                return 1;
            }
            sg[w] = g > 0 ? 1 : -1;
        }
        int cls = -1;
        for (int cl = 0; cl < 4; ++cl)
            if (sg[0] == lrd_cr_sign[cl][0] && sg[1] == lrd_cr_sign[cl][1] && sg[2] == lrd_cr_sign[cl][2]) cls = cl;
        if (cls < 0) { snprintf(why, len, "constraint %d has the signs (%d, %d, %d) of no class", i + 1, sg[0], sg[1], sg[2]); return 1; }
        if (j < 0 || j >= nl) { snprintf(why, len, "constraint %d names LP column %d", i + 1, j + 1); return 1; }
        if (u[j] != 0.0) { snprintf(why, len, "LP column %d occurs in 2 constraints", j + 1); return 1; }
        u[j] = 4.0 * -bt;
        const lrd_cr_cut cut = {cone, p, q, s, cls, i, j, -bt};
        cuts[(*ncut)++] = cut;
    }
    for (int j = 0; j < nl; ++j) {
        if (u[j] == 0.0) { snprintf(why, len, "LP column %d occurs in 0 constraints", j + 1); return 1; }
        if (P->lp_obj[j] != 0.0) { snprintf(why, len, "LP column %d has an objective coefficient", j + 1); return 1; }
    }
    return 0;
}

#endif
