/* separation.c -- what the separations of cuts.c and bounds.c share (DESIGN.md sections 14, 15 and 20): the session-level driver that
 * calls a table slot once per cone and merges the cones' lists (lrd_session_separate, lrd_merge_runs), and the one writer of a problem
 * image in SDPA sparse format, as it was read or extended by new rows with one new slack column each (lrd_write_extended), a pure
 * function of the image and the extension (so the format can be checked without a GPU). */
#include "lorads_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the array a column's field points to */
static void *column_base(const lrd_column *c) {
    void *base;
    memcpy(&base, c->field, sizeof base);
    return base;
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
        char *base = (char *)column_base(&col[w]);
        for (int e = 0; e < keep; ++e) memcpy(tmp + (size_t)e * sz, base + (size_t)order[e] * sz, sz);
        memcpy(base, tmp, (size_t)keep * sz);
    }
    free(order); free(tmp);
    return keep;
}

int lrd_session_separate(lrd_session *s, int have_slot, const char *cannot, int lone_lp, int max_cuts, const lrd_separation *sp) {
    const int refused = lrd_session_postsolve(s, have_slot, cannot, "the separation of a sharded deal (world > 1) is", NULL, NULL, sp->src);
    if (refused) return refused;
    lrd_backend *be = lrd_session_backend(s);
    const lrd_problem *pr = lrd_session_problem(s);
    const int nb = *sp->nblk = pr->nblk;
    int64_t *count = *sp->count = (int64_t *)lrd_zalloc((size_t)nb, sizeof(int64_t));
    for (int w = 0; w < sp->ncol; ++w) { /* room for the merged list and one cone's list behind it */
        void *base = calloc(2 * (size_t)(max_cuts > 0 ? max_cuts : 1), sp->col[w].size);
        memcpy(sp->col[w].field, &base, sizeof base);
    }
    int *cone = (int *)column_base(&sp->col[0]);
    for (int k = 0; k < nb; ++k) {
        if (pr->blk[k].is_lp && (nb > 1 || !lone_lp)) continue; /* (count 0) */
        const int at = *sp->kept;
        int got = 0, np = 0;
        const int rc = sp->cone(be, sp->list, *sp->src, k, at, &count[k], &got, &np);
        if (rc) return rc;
        *sp->passes += np;
        for (int e = 0; e < got; ++e) cone[at + e] = k;
        *sp->kept = lrd_merge_runs(sp->list, sp->before, sp->col, sp->ncol, at, got, max_cuts);
    }
    return 0;
}

int lrd_write_extended(const char *path, const lrd_problem *pr, const lrd_extension *x) {
    static const lrd_extension none = {0, NULL, NULL, NULL};
    if (!x) x = &none;
    const int m = pr->m, nb = pr->nblk, nnew = x->nrow;
    int lp = -1; /* the LP block the slack columns join and the column mask speaks of (-1: a new last block) */
    for (int k = 0; k < nb; ++k)
        if (pr->blk[k].is_lp) lp = k;
    const int nl = lp >= 0 ? pr->blk[lp].n : 0;
    FILE *f = fopen(path, "w");
    if (!f) return 1;
    /* the rows and LP columns that stay, renumbered in order (-1: leaves) */
    int *rowmap = (int *)lrd_zalloc((size_t)m, sizeof(int)), *colmap = (int *)lrd_zalloc((size_t)nl, sizeof(int));
    int m2 = 0, nl2 = 0;
    for (int i = 0; i < m; ++i) rowmap[i] = x->drop_row && x->drop_row[i] ? -1 : m2++;
    for (int j = 0; j < nl; ++j) colmap[j] = x->drop_col && x->drop_col[j] ? -1 : nl2++;
    const int new_block = nnew > 0 && lp < 0;
    fprintf(f, "%d\n%d\n", m2 + nnew, nb + new_block);
    for (int k = 0; k < nb; ++k) fprintf(f, "%s%d", k ? " " : "", pr->blk[k].is_lp ? -(k == lp ? nl2 + nnew : pr->blk[k].n) : pr->blk[k].n);
    if (new_block) fprintf(f, "%s%d", nb ? " " : "", -nnew);
    fputc('\n', f);
    for (int i = 0, first = 1; i < m; ++i)
        if (rowmap[i] >= 0) { fprintf(f, "%s%.17g", first ? "" : " ", pr->b[i]); first = 0; }
    for (int e = 0; e < nnew; ++e) fprintf(f, "%s%.17g", m2 + e ? " " : "", x->row[e].rhs);
    fputc('\n', f);
    /* lower triangle inside, upper triangle (i <= j) in the file; F0 = -C */
    for (int k = 0; k < nb; ++k) {
        const lrd_block *b = &pr->blk[k];
        const int *map = k == lp ? colmap : NULL;
        for (int e = 0; e < b->c_nnz; ++e) {
            const int i = map ? map[b->c_col[e]] : b->c_col[e], j = map ? map[b->c_row[e]] : b->c_row[e];
            if (i >= 0 && j >= 0) fprintf(f, "0 %d %d %d %.17g\n", k + 1, i + 1, j + 1, -b->c_val[e]);
        }
    }
    for (int k = 0; k < nb; ++k) {
        const lrd_block *b = &pr->blk[k];
        const int *map = k == lp ? colmap : NULL;
        for (int r = 0; r < b->nrow; ++r)
            for (int e = b->a_ptr[r]; e < b->a_ptr[r + 1] && rowmap[b->row_idx[r]] >= 0; ++e) {
                const int i = map ? map[b->a_col[e]] : b->a_col[e], j = map ? map[b->a_row[e]] : b->a_row[e];
                if (i >= 0 && j >= 0) fprintf(f, "%d %d %d %d %.17g\n", rowmap[b->row_idx[r]] + 1, k + 1, i + 1, j + 1, b->a_val[e]);
            }
    }
    /* the new rows: an off-diagonal entry counts twice in <A, X>; the row's own slack column behind the ones that stay */
    for (int e = 0; e < nnew; ++e) {
        const lrd_new_row *r = &x->row[e];
        for (int w = 0; w < r->nent; ++w)
            fprintf(f, "%d %d %d %d %.17g\n", m2 + e + 1, r->ent[w].cone + 1, r->ent[w].i + 1, r->ent[w].j + 1, r->ent[w].value);
        fprintf(f, "%d %d %d %d %.17g\n", m2 + e + 1, (new_block ? nb : lp) + 1, nl2 + e + 1, nl2 + e + 1, r->slack);
    }
    free(rowmap); free(colmap);
    return fclose(f) ? 1 : 0;
}
