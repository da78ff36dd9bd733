/* primal.c -- entries of the primal X = F F^T and its products with a block of vectors.
 * The numerical work is the backend's (lrd_backend.primal_entries / primal_apply); here: the session-level drivers, the query file
 * reader, the per-block grouping and the output file writer. */
#include "lorads_host.h"

#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int primal_refuse(lrd_session *s, lrd_backend **be, int *src) {
    const lrd_backend *t = lrd_session_backend(s);
    return lrd_session_postsolve(s, t && t->primal_entries && t->primal_apply, "query the primal",
                                 "primal queries of a sharded deal (world > 1) are", NULL, be, src);
}

int lrd_session_primal_entries(lrd_session *s, int blk, int64_t count, const int *row, const int *col, double *val, const double *ref,
                               double *stats) {
    lrd_backend *be;
    int src;
    const int rc = primal_refuse(s, &be, &src);
    return rc ? rc : be->primal_entries(be->ctx, src, blk, count, row, col, val, ref, stats);
}

int lrd_session_primal_apply(lrd_session *s, int blk, int ncols, const double *B, double *Y, double *T) {
    lrd_backend *be;
    int src;
    const int rc = primal_refuse(s, &be, &src);
    return rc ? rc : be->primal_apply(be->ctx, src, blk, ncols, B, Y, T);
}

void lrd_entries_free(lrd_entries *q) {
    if (!q) return;
    free(q->blk); free(q->row); free(q->col); free(q->ref); free(q->val);
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

int lrd_entries_read(const char *path, lrd_entries **out, int *bad_line) {
    *out = NULL;
    if (bad_line) *bad_line = 0;
    FILE *f = fopen(path, "r");
    if (!f) return 1;
    lrd_entries *q = (lrd_entries *)calloc(1, sizeof *q);
    q->has_ref = -1; /* (the first data line decides) */
    size_t cap = 0;
    char *line = NULL;
    size_t lcap = 0;
    int ln = 0, bad = 0;
    while (!bad && getline(&line, &lcap, f) >= 0) {
        ++ln;
        char *p = line;
        while (*p == ' ' || *p == '\t') ++p;
        if (*p == 0 || *p == '\n' || *p == '\r' || *p == '*' || *p == '#' || *p == '"') continue;
        int k, i, j;
        if (!read_index(&p, &k) || !read_index(&p, &i) || !read_index(&p, &j)) { bad = ln; break; }
        while (*p == ' ' || *p == '\t') ++p;
        int has = 0;
        double v = 0.0;
        if (*p && *p != '\n' && *p != '\r') {
            char *end = NULL;
            v = strtod(p, &end);
            if (end == p || !isfinite(v)) { bad = ln; break; }
            p = end;
            while (isspace((unsigned char)*p)) ++p;
            if (*p) { bad = ln; break; } /* (a fifth field) */
            has = 1;
        }
        if (q->has_ref < 0) q->has_ref = has;
        if (q->has_ref != has) { bad = ln; break; } /* (every line carries v or none does) */
        if ((size_t)q->count == cap) {
            cap = cap ? 2 * cap : 1024;
            q->blk = (int *)realloc(q->blk, cap * sizeof(int));
            q->row = (int *)realloc(q->row, cap * sizeof(int));
            q->col = (int *)realloc(q->col, cap * sizeof(int));
            q->ref = (double *)realloc(q->ref, cap * sizeof(double));
        }
        q->blk[q->count] = k - 1; q->row[q->count] = i - 1; q->col[q->count] = j - 1; q->ref[q->count] = v;
        ++q->count;
    }
    free(line);
    fclose(f);
    if (bad) {
        if (bad_line) *bad_line = bad;
        lrd_entries_free(q);
        return 2;
    }
    if (q->has_ref < 0) q->has_ref = 0;
    if (!q->has_ref) { free(q->ref); q->ref = NULL; }
    q->val = (double *)calloc(q->count ? (size_t)q->count : 1, sizeof(double));
    *out = q;
    return 0;
}

int lrd_entries_write(const char *path, const lrd_entries *q) {
    FILE *f = fopen(path, "w");
    if (!f) return 1;
    fprintf(f, "lorads-entries 1\ncount %lld\nsrc %s\nrefs %d\n", (long long)q->count, q->src == LRD_PAIR_UV ? "uv" : "rr", q->has_ref ? 1 : 0);
    if (q->has_ref) {
        const double c = q->count > 0 ? (double)q->count : 1.0;
        fprintf(f, "rmse %.17g\nmae %.17g\nmaxabs %.17g\nrefnorm %.17g\n", sqrt(q->stats[0] / c), q->stats[1] / c, q->stats[2], sqrt(q->stats[3]));
    }
    for (int64_t e = 0; e < q->count; ++e) {
        fprintf(f, "%d %d %d %.17g", q->blk[e] + 1, q->row[e] + 1, q->col[e] + 1, q->val[e]);
        if (q->has_ref) fprintf(f, " %.17g", q->ref[e]);
        fputc('\n', f);
    }
    return fclose(f) ? 1 : 0;
}

int lrd_entries_group(const lrd_entries *q, int nblk, int64_t *perm, int64_t *start) {
    for (int k = 0; k <= nblk; ++k) start[k] = 0;
    for (int64_t e = 0; e < q->count; ++e) {
        if (q->blk[e] < 0 || q->blk[e] >= nblk) return 1;
        ++start[q->blk[e] + 1];
    }
    for (int k = 0; k < nblk; ++k) start[k + 1] += start[k];
    int64_t *at = (int64_t *)malloc(sizeof(int64_t) * (size_t)(nblk > 0 ? nblk : 1));
    for (int k = 0; k < nblk; ++k) at[k] = start[k];
    for (int64_t e = 0; e < q->count; ++e) perm[at[q->blk[e]]++] = e; /* (stable: the file order inside a block) */
    free(at);
    return 0;
}

int lrd_session_entries(lrd_session *s, lrd_entries *q) {
    int rc = primal_refuse(s, NULL, &q->src);
    if (rc) return rc;
    const lrd_problem *p = lrd_session_problem(s);
    const int nb = p->nblk;
    const size_t cnt = q->count ? (size_t)q->count : 1;
    int64_t *perm = (int64_t *)malloc(sizeof(int64_t) * cnt), *start = (int64_t *)malloc(sizeof(int64_t) * (size_t)(nb + 1));
    int *row = (int *)malloc(sizeof(int) * cnt), *col = (int *)malloc(sizeof(int) * cnt);
    double *val = (double *)malloc(sizeof(double) * cnt), *ref = (double *)malloc(sizeof(double) * cnt);
    q->stats[0] = q->stats[1] = q->stats[2] = q->stats[3] = 0.0;
    rc = lrd_entries_group(q, nb, perm, start);
    if (rc) fprintf(stderr, "lorads: a query names a block outside 1..%d\n", nb);
    for (int k = 0; k < nb && !rc; ++k) {
        const int64_t a = start[k], c = start[k + 1] - a;
        if (c == 0) continue;
        for (int64_t t = 0; t < c; ++t) {
            row[t] = q->row[perm[a + t]]; col[t] = q->col[perm[a + t]];
            if (q->has_ref) ref[t] = q->ref[perm[a + t]];
        }
        double st[4] = {0, 0, 0, 0};
        rc = lrd_session_primal_entries(s, k, c, row, col, val, q->has_ref ? ref : NULL, q->has_ref ? st : NULL);
        if (rc) break;
        for (int64_t t = 0; t < c; ++t) q->val[perm[a + t]] = val[t];
        /* (the blocks' statistics in block order) */
        q->stats[0] += st[0]; q->stats[1] += st[1]; q->stats[2] = st[2] > q->stats[2] ? st[2] : q->stats[2]; q->stats[3] += st[3];
    }
    free(perm); free(start); free(row); free(col); free(val); free(ref);
    return rc;
}
