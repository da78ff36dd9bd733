/* rounding.c -- the plain-text rounding file (lorads_host.h: lrd_rounding_write), a pure function of the struct so that the command
 * line and the Python session write the same bytes and the format can be checked without a GPU.
 *
 *   lorads-rounding 1
 *   trials <K>  seed <S>  max_rounds <L>  rounds <r>  src <0|1>  best <i>  best0 <i>     (one per line, integers)
 *   scale, f_best, f_best0, by, bound, gap, tol                                          (one per line, %.17g)
 *   cone <k> <n>        then n lines: +1 or -1, the best trial's signs
 *
 * k is the block's 1-based number in the file. */
#include "lorads_host.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

void lrd_rounding_free(lrd_rounding *r) {
    if (!r) return;
    for (int k = 0; r->cone && k < r->nblk; ++k) {
        lrd_rounding_cone *q = &r->cone[k];
        free(q->sigma); free(q->t); free(q->x); free(q->G);
    }
    free(r->cone);
    free(r->obj);
    free(r->obj0);
    free(r);
}

int lrd_rounding_write(const char *path, const lrd_rounding *r) {
    if (!path || !r) return 1;
    FILE *f = fopen(path, "w");
    if (!f) return 2;
    fprintf(f, "lorads-rounding 1\n");
    fprintf(f, "trials %d\nseed %" PRIu64 "\nmax_rounds %d\nrounds %d\nsrc %d\nbest %d\nbest0 %d\n", r->trials, r->seed,
            r->max_rounds, r->rounds, r->src, r->best, r->best0);
    fprintf(f, "scale %.17g\nf_best %.17g\nf_best0 %.17g\nby %.17g\nbound %.17g\ngap %.17g\ntol %.17g\n", r->scale, r->f_best,
            r->f_best0, r->by, r->bound, r->gap, r->tol);
    for (int k = 0; k < r->nblk; ++k) {
        const lrd_rounding_cone *q = &r->cone[k];
        fprintf(f, "cone %d %d\n", k + 1, q->n);
        for (int j = 0; j < q->n; ++j) fprintf(f, "%s\n", q->sigma[j] > 0 ? "+1" : "-1");
    }
    return fclose(f) == 0 ? 0 : 3;
}
