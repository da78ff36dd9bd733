/* solution.c -- the plain-text solution file (lorads_host.h: lrd_solution_write), a pure function of the struct so that the
 * command line and the Python session write the same bytes and the format can be checked without a GPU.
 *
 *   lorads-solution 1
 *   status <int>
 *   pobj <p>            dobj <d>            (one per line)
 *   err1 .. err1_inf .. err2 .. err3 .. err4 .. err5 .. err6 ..   (one per line)
 *   y <m>               then m lines, one multiplier each
 *   sdp <k> <n> <r>     then n lines of r values: row i of R (X_k = R R^T)
 *   lp <k> <n>          then n lines: x_j
 *
 * k is the block's 1-based number in the file; every double is printed with %.17g (round-trips exactly). */
#include "lorads_host.h"

#include <stdio.h>
#include <stdlib.h>

void lrd_solution_free(lrd_solution *x) {
    if (!x) return;
    for (int k = 0; x->cone && k < x->nblk; ++k) {
        lrd_solution_cone *q = &x->cone[k];
        free(q->R); free(q->U); free(q->V); free(q->x); free(q->s_row); free(q->s_col); free(q->s_val);
    }
    free(x->cone);
    free(x->y);
    free(x);
}

int lrd_solution_write(const char *path, const lrd_solution *x) {
    if (!path || !x) return 1;
    FILE *f = fopen(path, "w");
    if (!f) return 2;
    fprintf(f, "lorads-solution 1\n");
    fprintf(f, "status %d\n", x->status);
    fprintf(f, "pobj %.17g\ndobj %.17g\n", x->pobj, x->dobj);
    fprintf(f, "err1 %.17g\nerr1_inf %.17g\nerr2 %.17g\nerr3 %.17g\nerr4 %.17g\nerr5 %.17g\nerr6 %.17g\n", x->err1, x->err1_inf,
            x->err2, x->err3, x->err4, x->err5, x->err6);
    fprintf(f, "y %d\n", x->m);
    for (int i = 0; i < x->m; ++i) fprintf(f, "%.17g\n", x->y[i]);
    for (int k = 0; k < x->nblk; ++k) {
        const lrd_solution_cone *q = &x->cone[k];
        if (q->is_lp) {
            fprintf(f, "lp %d %d\n", k + 1, q->n);
            for (int j = 0; j < q->n; ++j) fprintf(f, "%.17g\n", q->x[j]);
            continue;
        }
        fprintf(f, "sdp %d %d %d\n", k + 1, q->n, q->rank);
        for (int i = 0; i < q->n; ++i)
            for (int j = 0; j < q->rank; ++j) fprintf(f, j + 1 < q->rank ? "%.17g " : "%.17g\n", q->R[(size_t)j * q->n + i]);
    }
    return fclose(f) == 0 ? 0 : 3;
}
