/* spectral.c -- spectrum of the solution factors and their reduction to the rank the solution uses.
 * The numerical work is the backend's (lrd_backend.spectrum / compress_rank); here: the rank rule, the session-level drivers and the
 * report. */
#include "lorads_host.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int lrd_session_block_is_lp(lrd_session *s, int k) {
    const lrd_problem *p = lrd_session_problem(s);
    return k >= 0 && k < p->nblk && p->blk[k].is_lp;
}

/* max(1, min(cap, #{j : eig[j] > tol eig[0]})); cap <= 0: no cap.  eig descending, so eig[0] is the largest (<= 0: nothing counts) */
int lrd_spectral_choose(const double *eig, int rl, double tol, int cap) {
    int k = 0;
    for (int j = 0; j < rl; ++j)
        if (eig[j] > tol * eig[0]) ++k;
    if (cap > 0 && k > cap) k = cap;
    return k < 1 ? 1 : k;
}

static int spectral_slots(lrd_session *s) {
    const lrd_backend *be = lrd_session_backend(s);
    return be && be->spectrum && be->compress_rank;
}

int lrd_session_spectrum(lrd_session *s, double *eig, int *sweeps) {
    lrd_backend *be;
    int src;
    const int rc = lrd_session_postsolve(s, spectral_slots(s), "compute the spectrum of the solution",
                                         "the spectrum of the solution of a sharded deal (world > 1) is", NULL, &be, &src);
    return rc ? rc : be->spectrum(be->ctx, src, eig, NULL, sweeps);
}

void lrd_spectral_report_free(lrd_spectral_report *r) {
    if (!r) return;
    for (int k = 0; k < r->nblk && r->cone; ++k) free(r->cone[k].eig);
    free(r->cone);
    free(r);
}

int lrd_session_compress(lrd_session *s, double tol, int cap, lrd_spectral_report **report) {
    return lrd_session_compress_ex(s, tol, cap, NULL, report);
}

int lrd_session_compress_ex(lrd_session *s, double tol, int cap, const int *ranks, lrd_spectral_report **report) {
    if (report) *report = NULL;
    lrd_solver *v;
    lrd_backend *be;
    int src;
    int rc = lrd_session_postsolve(s, spectral_slots(s), "compute the rank reduction of the solution",
                                   "the rank reduction of the solution of a sharded deal (world > 1) is", &v, &be, &src);
    if (rc) return rc;
    if (!(tol >= 0)) return 1;
    const lrd_problem *p = lrd_session_problem(s);
    const int nb = p->nblk;
    const double sc = v->scaleObjHis;
    for (int k = 0; k < nb && ranks; ++k) /* (refused before anything is asked of the backend) */
        if (p->blk[k].is_lp ? ranks[k] != 1 : (ranks[k] < 1 || ranks[k] > v->rank[k])) {
            fprintf(stderr, "lorads: rank %d of block %d is outside 1..%d\n", ranks[k], k, p->blk[k].is_lp ? 1 : v->rank[k]);
            return 1;
        }
    size_t ne = 0;
    for (int k = 0; k < nb; ++k) ne += p->blk[k].is_lp ? 0 : (size_t)v->rank[k];
    double *eig = (double *)calloc(ne ? ne : 1, sizeof(double));
    int *sweeps = (int *)calloc((size_t)(nb > 0 ? nb : 1), sizeof(int)), *nr = (int *)calloc((size_t)(nb > 0 ? nb : 1), sizeof(int));
    lrd_spectral_report *r = (lrd_spectral_report *)calloc(1, sizeof *r);
    r->nblk = nb; r->src = src; r->tol = tol; r->cap = cap;
    r->cone = (lrd_spectral_cone *)calloc((size_t)(nb > 0 ? nb : 1), sizeof(lrd_spectral_cone));
    double pobj = 0.0;
    rc = be->cal_obj(be->ctx, src, &pobj) || be->update_dimacs(be->ctx, src, &r->err1_before);
    r->pobj_before = pobj / sc;
    if (!rc) rc = be->spectrum(be->ctx, src, eig, NULL, sweeps);
    size_t at = 0;
    for (int k = 0; k < nb && !rc; ++k) {
        lrd_spectral_cone *q = &r->cone[k];
        q->n = p->blk[k].n; q->is_lp = p->blk[k].is_lp; q->sweeps = sweeps[k];
        q->rank_before = q->rank_after = nr[k] = v->rank[k];
        if (q->is_lp) { if (ranks) q->rank_after = nr[k] = ranks[k]; continue; }
        const int rl = v->rank[k];
        const double *e = eig + at;
        const int kk = ranks ? ranks[k] : lrd_spectral_choose(e, rl, tol, cap);
        q->rank_after = nr[k] = kk;
        q->eig = (double *)malloc(sizeof(double) * (size_t)(rl > 0 ? rl : 1));
        memcpy(q->eig, e, sizeof(double) * (size_t)rl);
        double t_all = 0, t_lost = 0, f_all = 0, f_lost = 0; /* (small terms first) */
        for (int j = rl - 1; j >= 0; --j) {
            t_all += e[j]; f_all += e[j] * e[j];
            if (j >= kk && kk >= 0) { t_lost += e[j]; f_lost += e[j] * e[j]; }
        }
        q->trace_lost = t_all > 0 ? t_lost / t_all : 0.0;
        q->frob_lost = f_all > 0 ? sqrt(f_lost / f_all) : 0.0;
        at += (size_t)rl;
    }
    if (!rc) rc = be->compress_rank(be->ctx, src, nr, NULL);
    if (!rc) {
        for (int k = 0; k < nb; ++k) v->rank[k] = nr[k];
        rc = be->init_constr(be->ctx, src) || be->cal_obj(be->ctx, src, &pobj) || be->update_dimacs(be->ctx, src, &r->err1_after);
        r->pobj_after = pobj / sc;
        if (!rc) {
            v->pObjVal = r->pobj_after;
            v->err_constr_l1 = r->err1_after;
            v->err_pdgap = fabs(v->pObjVal - v->dObjVal) / (1 + fabs(v->pObjVal) + fabs(v->dObjVal));
        }
    }
    free(eig); free(sweeps); free(nr);
    if (rc || !report) lrd_spectral_report_free(r);
    else *report = r;
    return rc;
}
