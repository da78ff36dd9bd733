/* main.c -- command line with the reference's option names (src_semi/main.c:57-80):
 *   lorads file.dat-s [--phase1Tol x] [--timesLogRank x] ... ; solves on the MI355X backend. */
#include <libgen.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "lorads_host.h"

typedef struct lrd_session lrd_session;
lrd_session *lrd_session_open(const char *fname);
int lrd_session_set_param(lrd_session *s, const char *key, const char *val);
int lrd_session_prepare(lrd_session *s, int world, int rank_id);
int lrd_session_attach(lrd_session *s, const lrd_backend *be);
int lrd_session_solve(lrd_session *s);
int lrd_session_results(lrd_session *s, double out[16]);
int lrd_session_results2(lrd_session *s, double out[4]);
lrd_params *lrd_session_params(lrd_session *s);
void lrd_session_close(lrd_session *s);
int lrd_hip_backend_create(const lrd_problem *p, int lbfgs_len, const char *libpath, lrd_backend *out);
int lrd_session_round(lrd_session *s, int trials, uint64_t seed, int max_rounds, double tol, lrd_rounding **out);

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s file.dat-s [--option value ...]   (options: the reference's long options)\n", argv[0]);
        fprintf(stderr, "  --cutsMax K [--cutsMinViolation V] [--cutsFile OUT.dat-s] [--cutsDropSlack S] and --roundTrials T also take a file\n"
                        "  that --cutsFile wrote: the cuts it holds are passed over, the new ones appended, and with --cutsDropSlack the\n"
                        "  ones whose slack exceeds S dropped\n");
        return 2;
    }
    lrd_session *s = lrd_session_open(argv[1]);
    if (!s) return 1;
    const char *solution_file = NULL; /* ours, not the reference's: taken before the parameter block sees the options */
    /* The four roundings (ours as well): hyperplane rounding of a +-1-structured problem, rounding of a k-cut-structured problem into
     * k parts, stable sets of a theta-structured problem, balanced partitions of a bisection-structured problem.  Each has the options
     * --<prefix>Trials, Seed, LocalSearch and File; `gate` is the option the family's others need (--round* has none), `other` the last
     * of those others given.  strict = 0 is --round* as it always parsed: trials from 0, an empty value reads as 0, and a refusal
     * leaves the session open. */
    enum { RND, KCUT, STB, BIS };
    struct { const char *prefix, *gate; int strict, trials, ls; unsigned long long seed; const char *file, *other; } ro[4] = {
        {"round", NULL, 0, 0, 100, 0, NULL, NULL}, {"kcut", "--kcutParts", 1, 1024, 100, 0, NULL, NULL},
        {"stable", "--stableTrials", 1, 0, 100, 0, NULL, NULL}, {"bisect", "--bisectTrials", 1, 0, 1000, 0, NULL, NULL}};
    int kcut_parts = 0;
    int compress = 0, compress_cap = 0; /* rank reduction of the solution (ours as well): after the solve, before the file and the rounding */
    double compress_tol = 1e-12;
    const char *entries_in = NULL, *entries_out = NULL; /* entries of the primal at the positions of a query file (ours as well) */
    lrd_entries *queries = NULL;
    int cuts_max = -1;                /* separation of the triangle inequalities of a +-1-structured problem (ours as well) */
    double cuts_minv = 1e-3;
    int cuts_minv_given = 0;
    const char *cuts_file = NULL;
    double cuts_drop = -1.0;          /* --cutsDropSlack S: a present cut of a cut-tightened file leaves when its slack exceeds S (< 0: none) */
    int bounds_max = -1;              /* separation of entry bounds lower <= X_pq <= upper (ours as well) */
    double bounds_lower = 0.0, bounds_upper = HUGE_VAL, bounds_minv = 1e-3;
    const char *bounds_file = NULL, *bounds_other = NULL; /* bounds_other: some --bounds* option other than --boundsMax was given */
    const char *topk_in = NULL, *topk_out = NULL, *topk_other = NULL; /* the k best entries per row of the primal (ours as well);
                                                                       * topk_other: some --topk* option other than --topkFile was given */
    int topk_k = 0, topk_smallest = 0, topk_diag = 0, topk_constrained = 0;
    lrd_topk *topk = NULL;
    for (int i = 2; i < argc; i += 2) {
        if (!strcmp(argv[i], "--topkSmallest") || !strcmp(argv[i], "--topkDiag") || !strcmp(argv[i], "--topkSkipConstrained")) {
            topk_other = argv[i]; /* (flags: no value follows) */
            if (argv[i][7] == 'm') topk_smallest = 1;
            else if (argv[i][6] == 'D') topk_diag = 1;
            else topk_constrained = 1;
            i -= 1;
            continue;
        }
        if (i + 1 >= argc) {
            fprintf(stderr, "option %s lacks a value\n", argv[i]);
            return 2;
        }
        if (!strcmp(argv[i], "--solutionFile")) {
            solution_file = argv[i + 1];
            continue;
        }
        if (!strcmp(argv[i], "--entriesFile")) { entries_in = argv[i + 1]; continue; }
        if (!strcmp(argv[i], "--entriesOut")) { entries_out = argv[i + 1]; continue; }
        if (!strcmp(argv[i], "--cutsFile")) { cuts_file = argv[i + 1]; continue; }
        if (!strcmp(argv[i], "--topkFile")) { topk_in = argv[i + 1]; continue; }
        if (!strcmp(argv[i], "--topkOut")) { topk_other = argv[i]; topk_out = argv[i + 1]; continue; }
        if (!strcmp(argv[i], "--topkCount")) {
            char *end = NULL;
            const long k = strtol(argv[i + 1], &end, 10);
            if (!end || end == argv[i + 1] || *end || k < 1 || k > 128) {
                fprintf(stderr, "bad value %s of %s (1 .. 128)\n", argv[i + 1], argv[i]);
                lrd_session_close(s);
                return 2;
            }
            topk_other = argv[i];
            topk_k = (int)k;
            continue;
        }
        if (!strcmp(argv[i], "--cutsMax") || !strcmp(argv[i], "--cutsMinViolation")) {
            char *end = NULL;
            const int is_max = argv[i][7] == 'a';
            const double t = is_max ? 0.0 : strtod(argv[i + 1], &end);
            const long k = is_max ? strtol(argv[i + 1], &end, 10) : 1;
            if (!end || end == argv[i + 1] || *end || !(t >= 0) || !(t < HUGE_VAL) || k < 1 || k > (1L << 20)) {
                fprintf(stderr, "bad value %s of %s\n", argv[i + 1], argv[i]);
                lrd_session_close(s);
                return 2;
            }
            if (is_max) cuts_max = (int)k;
            else { cuts_minv = t; cuts_minv_given = 1; }
            continue;
        }
        if (!strcmp(argv[i], "--cutsDropSlack")) {
            char *end = NULL;
            const double t = strtod(argv[i + 1], &end);
            if (!end || end == argv[i + 1] || *end || !(t >= 0) || !(t < HUGE_VAL)) {
                fprintf(stderr, "bad value %s of %s\n", argv[i + 1], argv[i]);
                lrd_session_close(s);
                return 2;
            }
            cuts_drop = t;
            continue;
        }
        if (!strcmp(argv[i], "--boundsFile")) { bounds_other = argv[i]; bounds_file = argv[i + 1]; continue; }
        if (!strcmp(argv[i], "--boundsMax") || !strcmp(argv[i], "--boundsLower") || !strcmp(argv[i], "--boundsUpper") ||
            !strcmp(argv[i], "--boundsMinViolation")) {
            char *end = NULL;
            const char w = argv[i][9] == 'a' ? 'K' : argv[i][9] == 'i' ? 'V' : argv[i][8]; /* K, L, U or V */
            const double t = w == 'K' ? 0.0 : strtod(argv[i + 1], &end);
            const long k = w == 'K' ? strtol(argv[i + 1], &end, 10) : 1;
            int bad = !end || end == argv[i + 1] || *end || t != t || k < 1 || k > (1L << 20);
            if (w == 'V') bad = bad || !(t >= 0) || !(t < HUGE_VAL);
            if (w == 'L') bad = bad || t == HUGE_VAL;   /* (-inf switches the class off) */
            if (w == 'U') bad = bad || t == -HUGE_VAL;
            if (bad) {
                fprintf(stderr, "bad value %s of %s\n", argv[i + 1], argv[i]);
                lrd_session_close(s);
                return 2;
            }
            if (w == 'K') bounds_max = (int)k;
            else {
                bounds_other = argv[i];
                if (w == 'L') bounds_lower = t;
                else if (w == 'U') bounds_upper = t;
                else bounds_minv = t;
            }
            continue;
        }
        int fam = -1;
        const char *opt = "";
        for (int f = 0; f < 4 && fam < 0 && !strncmp(argv[i], "--", 2); ++f) {
            const size_t len = strlen(ro[f].prefix);
            if (strncmp(argv[i] + 2, ro[f].prefix, len)) continue;
            opt = argv[i] + 2 + len;
            if (!strcmp(opt, "Trials") || !strcmp(opt, "Seed") || !strcmp(opt, "LocalSearch") || !strcmp(opt, "File") ||
                (f == KCUT && !strcmp(opt, "Parts")))
                fam = f;
        }
        if (fam >= 0) {
            const char w = opt[0]; /* T, S, L, F or P */
            if (ro[fam].gate && strcmp(argv[i], ro[fam].gate)) ro[fam].other = argv[i];
            if (w == 'F') { ro[fam].file = argv[i + 1]; continue; }
            char *end = NULL;
            const unsigned long long v = strtoull(argv[i + 1], &end, 10);
            int bad = !end || *end || argv[i + 1][0] == '-' || (w != 'S' && w != 'P' && v > 65536);
            if (ro[fam].strict) bad = bad || end == argv[i + 1] || (w == 'T' && v < 1) || (w == 'P' && (v < 2 || v > 64));
            if (bad) {
                fprintf(stderr, "bad value %s of %s\n", argv[i + 1], argv[i]);
                if (ro[fam].strict) lrd_session_close(s);
                return 2;
            }
            if (w == 'P') kcut_parts = (int)v;
            else if (w == 'T') ro[fam].trials = (int)v;
            else if (w == 'S') ro[fam].seed = v;
            else ro[fam].ls = (int)v;
            continue;
        }
        if (!strcmp(argv[i], "--compressTol") || !strcmp(argv[i], "--compressRank")) {
            char *end = NULL;
            const int is_tol = argv[i][10] == 'T';
            const double t = is_tol ? strtod(argv[i + 1], &end) : 0.0;
            const long kcap = is_tol ? 1 : strtol(argv[i + 1], &end, 10);
            if (!end || end == argv[i + 1] || *end || !(t >= 0) || !(t < HUGE_VAL) || kcap < 1 || kcap > 512) {
                fprintf(stderr, "bad value %s of %s\n", argv[i + 1], argv[i]);
                return 2;
            }
            if (is_tol) compress_tol = t;
            else compress_cap = (int)kcap;
            compress = 1;
            continue;
        }
        if (strncmp(argv[i], "--", 2) || lrd_session_set_param(s, argv[i] + 2, argv[i + 1])) {
            fprintf(stderr, "unknown option %s\n", argv[i]);
            return 2;
        }
    }
    if (entries_out && !entries_in) {
        fprintf(stderr, "--entriesOut needs --entriesFile\n");
        lrd_session_close(s);
        return 2;
    }
    if ((cuts_file || cuts_minv_given || cuts_drop >= 0) && cuts_max < 0) {
        fprintf(stderr, "%s needs --cutsMax\n", cuts_file ? "--cutsFile" : cuts_minv_given ? "--cutsMinViolation" : "--cutsDropSlack");
        lrd_session_close(s);
        return 2;
    }
    if (bounds_other && bounds_max < 0) {
        fprintf(stderr, "%s needs --boundsMax\n", bounds_other);
        lrd_session_close(s);
        return 2;
    }
    if (bounds_max > 0 && (bounds_lower > bounds_upper || (bounds_lower == -HUGE_VAL && bounds_upper == HUGE_VAL))) {
        fprintf(stderr, "bad value of --boundsLower and --boundsUpper: %g, %g (lower above upper, or both classes off)\n", bounds_lower,
                bounds_upper);
        lrd_session_close(s);
        return 2;
    }
    for (int f = KCUT; f <= BIS; ++f) {
        if (ro[f].other && (f == KCUT ? kcut_parts : ro[f].trials) == 0) {
            fprintf(stderr, "%s needs %s\n", ro[f].other, ro[f].gate);
            lrd_session_close(s);
            return 2;
        }
        if (f == KCUT && kcut_parts > 0 && (long)kcut_parts * ro[KCUT].trials > (1L << 20)) {
            fprintf(stderr, "bad value of --kcutParts and --kcutTrials: %d x %d is above 2^20\n", kcut_parts, ro[KCUT].trials);
            lrd_session_close(s);
            return 2;
        }
    }
    if (topk_other && !topk_in) {
        fprintf(stderr, "%s needs --topkFile\n", topk_other);
        lrd_session_close(s);
        return 2;
    }
    if (topk_in && topk_k == 0) {
        fprintf(stderr, "--topkFile needs --topkCount\n");
        lrd_session_close(s);
        return 2;
    }
    if (topk_in) { /* as the entry queries: refused before the backend is created */
        int bad = 0;
        const int qrc = lrd_topk_read(topk_in, &topk, &bad);
        if (qrc) {
            if (qrc == 1) fprintf(stderr, "lorads: cannot read the top-k query file %s\n", topk_in);
            else fprintf(stderr, "lorads: line %d of the top-k query file %s is malformed (blk row lo hi [skip ...], 1-based, lo <= hi)\n", bad, topk_in);
            lrd_session_close(s);
            return 2;
        }
        const lrd_problem *pr = lrd_session_problem(s);
        for (int e = 0; e < topk->count; ++e) {
            const int k = topk->blk[e];
            int out = k >= pr->nblk || pr->blk[k].is_lp || topk->row[e] >= pr->blk[k].n || topk->hi[e] > pr->blk[k].n;
            for (int64_t x = topk->skip_ptr[e]; !out && x < topk->skip_ptr[e + 1]; ++x) out = topk->skip_col[x] >= pr->blk[k].n;
            if (out) {
                fprintf(stderr, "lorads: query %d of %s (%d %d %d %d ...) is outside the problem or names the LP block\n", e + 1, topk_in, k + 1,
                        topk->row[e] + 1, topk->lo[e] + 1, topk->hi[e]);
                lrd_topk_free(topk);
                lrd_session_close(s);
                return 2;
            }
        }
        topk->k = topk_k; topk->smallest = topk_smallest; topk->include_diag = topk_diag; topk->skip_constrained = topk_constrained;
    }
    if (entries_in) { /* a bad query file is refused before the backend is created, let alone anything solved */
        int bad = 0;
        const int qrc = lrd_entries_read(entries_in, &queries, &bad);
        if (qrc) {
            if (qrc == 1) fprintf(stderr, "lorads: cannot read the query file %s\n", entries_in);
            else fprintf(stderr, "lorads: line %d of the query file %s is malformed (k i j [v], 1-based; every line with v or none)\n", bad, entries_in);
            lrd_topk_free(topk);
            lrd_session_close(s);
            return 2;
        }
        const lrd_problem *pr = lrd_session_problem(s);
        for (int64_t e = 0; e < queries->count; ++e) {
            const int k = queries->blk[e];
            if (k >= pr->nblk || queries->row[e] >= pr->blk[k].n || queries->col[e] >= pr->blk[k].n) {
                fprintf(stderr, "lorads: query %lld of %s (%d %d %d) is outside the problem\n", (long long)e + 1, entries_in, k + 1,
                        queries->row[e] + 1, queries->col[e] + 1);
                lrd_entries_free(queries);
                lrd_topk_free(topk);
                lrd_session_close(s);
                return 2;
            }
        }
    }
    lrd_session_prepare(s, 1, 0);
    char self[4096], lib[4200];
    ssize_t n = readlink("/proc/self/exe", self, sizeof self - 1);
    if (n <= 0) return 1;
    self[n] = 0;
    snprintf(lib, sizeof lib, "%s/liblorads_hip.so", dirname(self));
    lrd_backend be;
    if (lrd_hip_backend_create(lrd_session_problem(s), lrd_session_params(s)->lbfgsListLength, lib, &be)) {
        fprintf(stderr, "lorads: the HIP backend is required (no CPU fallback)\n");
        return 1;
    }
    if (lrd_session_attach(s, &be)) return 1;
    if (ro[RND].trials > 0 || cuts_max > 0) { /* applicability before any solving */
        lrd_rounding *none = NULL;
        const int rrc = lrd_session_round(s, 0, ro[RND].seed, ro[RND].ls, 0.0, &none);
        if (rrc) {
            fprintf(stderr, "lorads: %s needs a +-1-structured problem (see above); nothing was solved\n",
                    ro[RND].trials > 0 ? "--roundTrials" : "--cutsMax");
            lrd_topk_free(topk);
            lrd_session_close(s);
            return 2;
        }
    }
    if (kcut_parts > 0) { /* applicability before any solving */
        lrd_kcut *none = NULL;
        if (lrd_session_kcut(s, kcut_parts, 0, ro[KCUT].seed, ro[KCUT].ls, 0.0, 0, &none)) {
            fprintf(stderr, "lorads: --kcutParts needs a k-cut-structured problem (see above); nothing was solved\n");
            lrd_topk_free(topk);
            lrd_session_close(s);
            return 2;
        }
    }
    if (ro[STB].trials > 0) { /* applicability before any solving */
        lrd_stable *none = NULL;
        if (lrd_session_round_stable(s, 0, ro[STB].seed, ro[STB].ls, 0.0, 0, &none)) {
            fprintf(stderr, "lorads: --stableTrials needs a theta-structured problem (see above); nothing was solved\n");
            lrd_topk_free(topk);
            lrd_session_close(s);
            return 2;
        }
    }
    if (ro[BIS].trials > 0) { /* applicability before any solving */
        lrd_bisection *none = NULL;
        if (lrd_session_round_bisect(s, 0, ro[BIS].seed, ro[BIS].ls, 0.0, 0, &none)) {
            fprintf(stderr, "lorads: --bisectTrials needs a bisection-structured problem (see above); nothing was solved\n");
            lrd_topk_free(topk);
            lrd_session_close(s);
            return 2;
        }
    }
    const int rc = lrd_session_solve(s);
    if (rc != 0) {
        fprintf(stderr, "lorads: the solve failed (code %d): a backend call reported an error\n", rc);
        lrd_topk_free(topk);
        lrd_session_close(s);
        return 3;
    }
    double r[16], r2[4];
    lrd_session_results(s, r);
    lrd_session_results2(s, r2);
    static const char *why[] = {"but the status is unknown", "due to reaching `Official terminate criteria`",
                                "due to reaching `final terminate criteria`", "due to reaching `the maximum number of iterations`",
                                "since time limit"};
    printf("End Program %s:\n", why[(int)r[12] >= 0 && (int)r[12] <= 4 ? (int)r[12] : 0]);
    /* printRes layout (data/lorads_solver.c:908-922) */
    printf("-----------------------------------------------------------------------\n");
    printf("Objective function Value are:\n\t 1.Primal Objective:            : %10.6e\n\t 2.Dual Objective:              : %10.6e\n",
           r[0], r[1]);
    printf("Dimacs Error are:\n\t 1.Constraint Violation(1)      : %10.6e\n\t 2.Dual Infeasibility(1)        : %10.6e\n"
           "\t 3.Primal Dual Gap              : %10.6e\n\t 5.Constraint Violation(Inf)    : %10.6e\n"
           "\t 6.Dual Infeasibility(Inf)      : %10.6e\n", r[2], r2[0], r[3], r[15], r2[1]);
    printf("-----------------------------------------------------------------------\n");
    printf("phase 1: %f s, phase 2: %f s (%d ADMM iterations, %d CG iterations), dual infeasibility: %f s\n", r[10], r[11],
           (int)r[13], (int)r[14], r2[2]);
    if (compress) {
        lrd_spectral_report *x = NULL;
        if (lrd_session_compress(s, compress_tol, compress_cap, &x)) {
            fprintf(stderr, "lorads: the rank reduction failed\n");
            lrd_session_close(s);
            return 4;
        }
        printf("Rank reduction of the solution:\n");
        for (int k = 0; k < x->nblk; ++k) {
            const lrd_spectral_cone *q = &x->cone[k];
            if (q->is_lp) { printf("\t block %d: lp %d, left alone\n", k + 1, q->n); continue; }
            printf("\t block %d: sdp %d, rank %d -> %d (%d Jacobi sweeps), lambda_1 %.6e, lambda_%d %.6e, trace share lost %.3e, "
                   "||X - X_k||_F / ||X||_F %.3e\n", k + 1, q->n, q->rank_before, q->rank_after, q->sweeps, q->eig[0], q->rank_before,
                   q->eig[q->rank_before - 1], q->trace_lost, q->frob_lost);
        }
        printf("\t primal objective <C, X>         : %.10e -> %.10e\n\t err1 ||A(X) - b||_2 rel.        : %.6e -> %.6e\n",
               x->pobj_before, x->pobj_after, x->err1_before, x->err1_after);
        lrd_spectral_report_free(x);
    }
    if (queries) {
        if (lrd_session_entries(s, queries) || (entries_out && lrd_entries_write(entries_out, queries))) {
            fprintf(stderr, "lorads: the entry queries failed%s%s\n", entries_out ? " or cannot write " : "", entries_out ? entries_out : "");
            lrd_session_close(s);
            return 4;
        }
        printf("Entries of the primal X (%s): %lld positions%s%s\n", entries_in, (long long)queries->count, entries_out ? " -> " : "",
               entries_out ? entries_out : "");
        if (queries->has_ref) {
            const double c = queries->count > 0 ? (double)queries->count : 1.0;
            printf("\t against the reference values: RMSE %.17g, MAE %.17g, max %.17g\n", sqrt(queries->stats[0] / c), queries->stats[1] / c,
                   queries->stats[2]);
        }
        lrd_entries_free(queries);
    }
    if (topk) {
        char dflt[4096];
        snprintf(dflt, sizeof dflt, "%s.out", topk_in);
        const char *to = topk_out ? topk_out : dflt;
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        const int trc = lrd_session_topk(s, topk);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (trc || lrd_topk_write(to, topk)) {
            fprintf(stderr, "lorads: the top-k search failed or cannot write %s\n", to);
            lrd_topk_free(topk);
            lrd_session_close(s);
            return 4;
        }
        long long total = 0;
        for (int e = 0; e < topk->count; ++e) total += topk->found[e];
        printf("Top-k entries per row of the primal X (%s): %d queries, k %d, %lld found, %.6f s -> %s\n", topk_in, topk->count, topk->k,
               total, (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec), to);
        lrd_topk_free(topk);
    }
    if (cuts_max > 0) {
        lrd_cuts *x = NULL;
        if (lrd_session_triangle_cuts(s, cuts_minv, cuts_max, &x) || (cuts_file && (cuts_drop >= 0 ? lrd_session_write_tightened_drop(s, cuts_file, x, cuts_drop, 1e-8, NULL)
                                                                                                : lrd_session_write_tightened(s, cuts_file, x)))) {
            fprintf(stderr, "lorads: the separation failed%s%s\n", cuts_file ? " or cannot write " : "", cuts_file ? cuts_file : "");
            lrd_cuts_free(x);
            lrd_session_close(s);
            return 4;
        }
        long long total = 0;
        for (int k = 0; k < x->nblk; ++k) total += (long long)x->count[k];
        printf("Triangle inequalities violated by more than %g: %lld, kept %d, largest violation %.6e%s%s\n", cuts_minv, total, x->kept,
               x->kept > 0 ? x->viol[0] : 0.0, cuts_file ? " -> " : "", cuts_file ? cuts_file : "");
        lrd_cuts_free(x);
    }
    if (bounds_max > 0) {
        lrd_bounds *x = NULL;
        if (lrd_session_entry_bounds(s, bounds_lower, bounds_upper, bounds_minv, bounds_max, &x) ||
            (bounds_file && lrd_session_write_bounded(s, bounds_file, x))) {
            fprintf(stderr, "lorads: the separation of the entry bounds failed%s%s\n", bounds_file ? " or cannot write " : "",
                    bounds_file ? bounds_file : "");
            lrd_bounds_free(x);
            lrd_session_close(s);
            return 4;
        }
        long long total = 0;
        for (int k = 0; k < x->nblk; ++k) total += (long long)x->count[k];
        printf("Entry bounds [%g, %g] violated by more than %g: %lld, kept %d, largest violation %.6e, %d passes%s%s\n", bounds_lower,
               bounds_upper, bounds_minv, total, x->kept, x->kept > 0 ? x->viol[0] : 0.0, x->passes, bounds_file ? " -> " : "",
               bounds_file ? bounds_file : "");
        lrd_bounds_free(x);
    }
    if (solution_file) {
        lrd_solution *x = NULL;
        if (lrd_session_solution(s, 1e-8, &x) || lrd_solution_write(solution_file, x)) {
            fprintf(stderr, "lorads: cannot write the solution file %s\n", solution_file);
            lrd_solution_free(x);
            lrd_session_close(s);
            return 4;
        }
        printf("Certificate of the exported solution (%s):\n", solution_file);
        printf("\t primal objective <C, X>         : %.10e\n\t dual objective b.y               : %.10e\n", x->pobj, x->dobj);
        printf("\t err1 ||A(X) - b||_2 rel.        : %.6e\n\t err1 ||A(X) - b||_inf rel.      : %.6e\n", x->err1, x->err1_inf);
        printf("\t err2 (X = R R^T psd)            : %.6e\n\t err3 (S = C - A*(y))            : %.6e\n", x->err2, x->err3);
        printf("\t err4 lambda_min(S) rel.         : %.6e\n\t err5 gap rel.                   : %.6e\n", x->err4, x->err5);
        printf("\t err6 <X, S> rel.                : %.6e\n", x->err6);
        lrd_solution_free(x);
    }
    if (ro[RND].trials > 0) {
        lrd_rounding *x = NULL;
        if (lrd_session_round(s, ro[RND].trials, (uint64_t)ro[RND].seed, ro[RND].ls, 1e-8, &x) ||
            (ro[RND].file && lrd_rounding_write(ro[RND].file, x))) {
            fprintf(stderr, "lorads: the rounding failed%s%s\n", ro[RND].file ? " or cannot write " : "", ro[RND].file ? ro[RND].file : "");
            lrd_rounding_free(x);
            lrd_session_close(s);
            return 4;
        }
        printf("Hyperplane rounding (%d trials, seed %llu, %d local-search rounds%s%s):\n", x->head.trials, ro[RND].seed, x->head.rounds,
               ro[RND].file ? ", " : "", ro[RND].file ? ro[RND].file : "");
        printf("\t best trial                      : %d (before the local search: %d)\n", x->head.best, x->head.best0);
        printf("\t f = x^T C x before local search : %.10e\n\t f = x^T C x after local search  : %.10e\n", x->head.f_best0, x->head.f_best);
        printf("\t dual bound d                    : %.10e\n\t gap (f - d) / max(1, |d|)       : %.6e\n", x->head.bound, x->head.gap);
        if (x->nlp > 0) printf("\t triangle cuts in the problem     : %d (%d with a negative dual slack)\n", x->nlp, x->lp_neg);
        lrd_rounding_free(x);
    }
    if (kcut_parts > 0) {
        lrd_kcut *x = NULL;
        if (lrd_session_kcut(s, kcut_parts, ro[KCUT].trials, (uint64_t)ro[KCUT].seed, ro[KCUT].ls, 1e-8, 0, &x) ||
            (ro[KCUT].file && lrd_kcut_write(ro[KCUT].file, x))) {
            fprintf(stderr, "lorads: the rounding into parts failed%s%s\n", ro[KCUT].file ? " or cannot write " : "", ro[KCUT].file ? ro[KCUT].file : "");
            lrd_kcut_free(x);
            lrd_session_close(s);
            return 4;
        }
        printf("Rounding into %d parts (%d trials, seed %llu%s%s): best f %.10e, dual bound d %.10e, gap %.6e, %d local-search rounds\n",
               x->parts, x->head.trials, ro[KCUT].seed, ro[KCUT].file ? ", " : "", ro[KCUT].file ? ro[KCUT].file : "", x->head.f_best, x->head.bound, x->head.gap, x->head.rounds);
        lrd_kcut_free(x);
    }
    if (ro[STB].trials > 0) {
        lrd_stable *x = NULL;
        if (lrd_session_round_stable(s, ro[STB].trials, (uint64_t)ro[STB].seed, ro[STB].ls, 1e-8, 0, &x) ||
            (ro[STB].file && lrd_stable_write(ro[STB].file, x))) {
            fprintf(stderr, "lorads: the stable-set rounding failed%s%s\n", ro[STB].file ? " or cannot write " : "", ro[STB].file ? ro[STB].file : "");
            lrd_stable_free(x);
            lrd_session_close(s);
            return 4;
        }
        printf("Stable sets (%d trials, seed %llu%s%s): size", x->head.trials, ro[STB].seed, ro[STB].file ? ", " : "", ro[STB].file ? ro[STB].file : "");
        for (int k = 0; k < x->nblk; ++k) printf(" %d", x->cone[k].size);
        printf(", best f %.10e, dual bound d %.10e, gap %.6e, %d search rounds\n", x->head.f_best, x->head.bound, x->head.gap, x->head.rounds);
        lrd_stable_free(x);
    }
    if (ro[BIS].trials > 0) {
        lrd_bisection *x = NULL;
        if (lrd_session_round_bisect(s, ro[BIS].trials, (uint64_t)ro[BIS].seed, ro[BIS].ls, 1e-8, 0, &x) ||
            (ro[BIS].file && lrd_bisection_write(ro[BIS].file, x))) {
            fprintf(stderr, "lorads: the bisection rounding failed%s%s\n", ro[BIS].file ? " or cannot write " : "", ro[BIS].file ? ro[BIS].file : "");
            lrd_bisection_free(x);
            lrd_session_close(s);
            return 4;
        }
        printf("Bisection (%d trials, seed %llu%s%s): parts", x->head.trials, ro[BIS].seed, ro[BIS].file ? ", " : "", ro[BIS].file ? ro[BIS].file : "");
        for (int k = 0; k < x->nblk; ++k) printf(" %d+%d", x->cone[k].plus, x->cone[k].minus);
        printf(", best f %.10e, dual bound d %.10e, gap %.6e, %d search rounds\n", x->head.f_best, x->head.bound, x->head.gap, x->head.rounds);
        lrd_bisection_free(x);
    }
    lrd_session_close(s);
    return 0;
}
