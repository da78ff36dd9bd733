/* topk.c -- the k best entries per row of the primal X = F F^T.  The search is the backend's
 * (lrd_backend.primal_topk); here: the session-level call with the one convenience the device does not know (skip_constrained: the
 * columns at which a constraint matrix of the cone stores an entry in the query's row), the query file reader, the grouping of a
 * file's queries into calls and the output file writer, a pure function of the result struct. */
#include "lorads_host.h"

#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* CSR of the columns q with a stored entry (p, q) or (q, p) in some A_i of the cone: ptr [n + 1], col (duplicates stay: the backend
 * removes them) */
static void constrained_pattern(const lrd_block *b, int64_t **ptr_out, int **col_out) {
    const int n = b->n;
    const int64_t na = b->nrow > 0 ? (int64_t)b->a_ptr[b->nrow] : 0;
    int64_t *ptr = (int64_t *)calloc((size_t)n + 2, sizeof(int64_t));
    for (int64_t e = 0; e < na; ++e) {
        ++ptr[b->a_row[e] + 2];
        if (b->a_row[e] != b->a_col[e]) ++ptr[b->a_col[e] + 2];
    }
    for (int p = 0; p < n; ++p) ptr[p + 2] += ptr[p + 1];
    int *col = (int *)malloc(sizeof(int) * (size_t)(ptr[n + 1] > 0 ? ptr[n + 1] : 1));
    for (int64_t e = 0; e < na; ++e) { /* (ptr[p + 1] is row p's cursor and ends as its end) */
        col[ptr[b->a_row[e] + 1]++] = b->a_col[e];
        if (b->a_row[e] != b->a_col[e]) col[ptr[b->a_col[e] + 1]++] = b->a_row[e];
    }
    *ptr_out = ptr;
    *col_out = col;
}

int lrd_session_primal_topk(lrd_session *s, int blk, int nq, const int *row, int col_lo, int col_hi, int k, int smallest, int include_diag,
                            const int64_t *skip_ptr, const int *skip_col, int skip_constrained, int *idx, double *val, int *found) {
    lrd_backend *be;
    int src;
    const lrd_backend *t = lrd_session_backend(s);
    const int refused = lrd_session_postsolve(s, t && t->primal_topk, "search the rows of the primal",
                                              "the top-k search of a sharded deal (world > 1) is", NULL, &be, &src);
    if (refused) return refused;
    const lrd_problem *pr = lrd_session_problem(s);
    /* what cannot be combined here is the backend's to refuse, in its words */
    int plain = !skip_constrained || blk < 0 || blk >= pr->nblk || pr->blk[blk].is_lp || nq <= 0 || !row || (!skip_ptr) != (!skip_col);
    if (!plain && skip_ptr) {
        plain = skip_ptr[0] != 0;
        for (int i = 0; i < nq && !plain; ++i) plain = skip_ptr[i + 1] < skip_ptr[i];
    }
    for (int i = 0; i < nq && !plain; ++i) plain = row[i] < 0 || row[i] >= pr->blk[blk].n;
    if (plain)
        return be->primal_topk(be->ctx, src, blk, nq, row, col_lo, col_hi, k, smallest, include_diag, skip_ptr, skip_col, idx, val, found);
    int64_t *cp, *ptr = (int64_t *)calloc((size_t)nq + 1, sizeof(int64_t));
    int *cc;
    constrained_pattern(&pr->blk[blk], &cp, &cc);
    for (int i = 0; i < nq; ++i)
        ptr[i + 1] = ptr[i] + (cp[row[i] + 1] - cp[row[i]]) + (skip_ptr ? skip_ptr[i + 1] - skip_ptr[i] : 0);
    int *col = (int *)malloc(sizeof(int) * (size_t)(ptr[nq] > 0 ? ptr[nq] : 1));
    for (int i = 0; i < nq; ++i) {
        int64_t at = ptr[i];
        for (int64_t e = cp[row[i]]; e < cp[row[i] + 1]; ++e) col[at++] = cc[e];
        for (int64_t e = skip_ptr ? skip_ptr[i] : 0; skip_ptr && e < skip_ptr[i + 1]; ++e) col[at++] = skip_col[e];
    }
    const int rc = be->primal_topk(be->ctx, src, blk, nq, row, col_lo, col_hi, k, smallest, include_diag, ptr, col, idx, val, found);
    free(cp); free(cc); free(ptr); free(col);
    return rc;
}

void lrd_topk_free(lrd_topk *q) {
    if (!q) return;
    free(q->blk); free(q->row); free(q->lo); free(q->hi); free(q->skip_ptr); free(q->skip_col); free(q->found); free(q->idx); free(q->val);
    free(q);
}

/* a 1-based index at *p (digits only, within int); advances *p; 0 on failure */
static int read_index(char **p, int *out) {
    while (**p == ' ' || **p == '\t') ++*p;
    if (!isdigit((unsigned char)**p)) return 0;
    char *end = NULL;
    const long v = strtol(*p, &end, 10);
    if (end == *p || v < 1 || v > 2147483647L || (*end && !isspace((unsigned char)*end))) return 0;
    *p = end;
    *out = (int)v;
    return 1;
}

int lrd_topk_read(const char *path, lrd_topk **out, int *bad_line) {
    *out = NULL;
    if (bad_line) *bad_line = 0;
    FILE *f = fopen(path, "r");
    if (!f) return 1;
    lrd_topk *q = (lrd_topk *)calloc(1, sizeof *q);
    size_t cap = 0, scap = 0;
    int64_t ns = 0;
    char *line = NULL;
    size_t lcap = 0;
    int ln = 0, bad = 0;
    q->skip_ptr = (int64_t *)calloc(1, sizeof(int64_t));
    while (!bad && getline(&line, &lcap, f) >= 0) {
        ++ln;
        char *p = line;
        while (*p == ' ' || *p == '\t') ++p;
        if (*p == 0 || *p == '\n' || *p == '\r' || *p == '*' || *p == '#' || *p == '"') continue;
        int k, i, lo, hi;
        if (!read_index(&p, &k) || !read_index(&p, &i) || !read_index(&p, &lo) || !read_index(&p, &hi) || lo > hi) { bad = ln; break; }
        if ((size_t)q->count == cap) {
            cap = cap ? 2 * cap : 1024;
            q->blk = (int *)realloc(q->blk, cap * sizeof(int));
            q->row = (int *)realloc(q->row, cap * sizeof(int));
            q->lo = (int *)realloc(q->lo, cap * sizeof(int));
            q->hi = (int *)realloc(q->hi, cap * sizeof(int));
            q->skip_ptr = (int64_t *)realloc(q->skip_ptr, (cap + 1) * sizeof(int64_t));
        }
        for (;;) { /* the skip columns up to the end of the line */
            while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') ++p;
            if (!*p) break;
            int c;
            if (!read_index(&p, &c)) { bad = ln; break; }
            if ((size_t)ns == scap) {
                scap = scap ? 2 * scap : 1024;
                q->skip_col = (int *)realloc(q->skip_col, scap * sizeof(int));
            }
            q->skip_col[ns++] = c - 1;
        }
        if (bad) break;
        q->blk[q->count] = k - 1; q->row[q->count] = i - 1; q->lo[q->count] = lo - 1; q->hi[q->count] = hi; /* [lo - 1, hi) */
        q->skip_ptr[++q->count] = ns;
    }
    free(line);
    fclose(f);
    if (bad) {
        if (bad_line) *bad_line = bad;
        lrd_topk_free(q);
        return 2;
    }
    *out = q;
    return 0;
}

int lrd_topk_write(const char *path, const lrd_topk *q) {
    FILE *f = fopen(path, "w");
    if (!f) return 1;
    fprintf(f, "lorads-topk 1\ncount %d\nk %d\nsrc %s\norder %s\n", q->count, q->k, q->src == LRD_PAIR_UV ? "uv" : "rr",
            q->smallest ? "smallest" : "largest");
    for (int e = 0; e < q->count; ++e) {
        fprintf(f, "%d %d %d\n", q->blk[e] + 1, q->row[e] + 1, q->found[e]);
        for (int j = 0; j < q->found[e]; ++j)
            fprintf(f, "%d %.17g\n", q->idx[(size_t)e * (size_t)q->k + (size_t)j] + 1, q->val[(size_t)e * (size_t)q->k + (size_t)j]);
    }
    return fclose(f) ? 1 : 0;
}

/* file order within (block, window): the queries of one call */
typedef struct { int blk, lo, hi, e; } topk_call;
static int by_call(const void *a, const void *b) {
    const topk_call *x = (const topk_call *)a, *y = (const topk_call *)b;
    if (x->blk != y->blk) return x->blk < y->blk ? -1 : 1;
    if (x->lo != y->lo) return x->lo < y->lo ? -1 : 1;
    if (x->hi != y->hi) return x->hi < y->hi ? -1 : 1;
    return x->e < y->e ? -1 : x->e > y->e;
}

int lrd_session_topk(lrd_session *s, lrd_topk *q) {
    int rc = lrd_session_postsolve(s, lrd_session_backend(s) && lrd_session_backend(s)->primal_topk, "search the rows of the primal",
                                   "the top-k search of a sharded deal (world > 1) is", NULL, NULL, &q->src);
    if (rc) return rc;
    const size_t cnt = q->count > 0 ? (size_t)q->count : 1, k = (size_t)(q->k > 0 ? q->k : 1);
    free(q->found); free(q->idx); free(q->val);
    q->found = (int *)calloc(cnt, sizeof(int));
    q->idx = (int *)calloc(cnt * k, sizeof(int));
    q->val = (double *)calloc(cnt * k, sizeof(double));
    int *perm = (int *)malloc(sizeof(int) * cnt), *row = (int *)malloc(sizeof(int) * cnt), *found = (int *)malloc(sizeof(int) * cnt);
    int *idx = (int *)malloc(sizeof(int) * cnt * k), *col = (int *)malloc(sizeof(int) * (size_t)(q->skip_ptr[q->count] > 0 ? q->skip_ptr[q->count] : 1));
    double *val = (double *)malloc(sizeof(double) * cnt * k);
    int64_t *ptr = (int64_t *)malloc(sizeof(int64_t) * (cnt + 1));
    topk_call *rec = (topk_call *)malloc(sizeof(topk_call) * cnt);
    for (int e = 0; e < q->count; ++e) rec[e] = (topk_call){q->blk[e], q->lo[e], q->hi[e], e};
    qsort(rec, (size_t)q->count, sizeof(topk_call), by_call);
    for (int e = 0; e < q->count; ++e) perm[e] = rec[e].e;
    free(rec);
    for (int a = 0; a < q->count && !rc;) {
        int b = a;
        ptr[0] = 0;
        while (b < q->count && q->blk[perm[b]] == q->blk[perm[a]] && q->lo[perm[b]] == q->lo[perm[a]] && q->hi[perm[b]] == q->hi[perm[a]]) {
            const int e = perm[b], t = b - a;
            row[t] = q->row[e];
            ptr[t + 1] = ptr[t];
            for (int64_t x = q->skip_ptr[e]; x < q->skip_ptr[e + 1]; ++x) col[ptr[t + 1]++] = q->skip_col[x];
            ++b;
        }
        const int e0 = perm[a];
        rc = lrd_session_primal_topk(s, q->blk[e0], b - a, row, q->lo[e0], q->hi[e0], q->k, q->smallest, q->include_diag, ptr, col,
                                     q->skip_constrained, idx, val, found);
        for (int t = 0; t < b - a && !rc; ++t) {
            const size_t e = (size_t)perm[a + t];
            q->found[e] = found[t];
            memcpy(q->idx + e * k, idx + (size_t)t * k, sizeof(int) * k);
            memcpy(q->val + e * k, val + (size_t)t * k, sizeof(double) * k);
        }
        a = b;
    }
    free(perm); free(row); free(found); free(idx); free(col); free(val); free(ptr);
    return rc;
}
