// kcut.inc -- Frieze-Jerrum rounding of the factors into k parts and a 1-move local search (Max-k-Cut-type SDPs and the bounded
// problems lrd_session_write_bounded makes of them), included by lorads_hip.hip after rounding.inc.  DESIGN.md section 16.
//
// A context qualifies ("k-cut-structured") when every constraint without an LP entry is a_i X_k[p,p] = b_i with b_i / a_i > 0, one
// per diagonal position of every cone (t_p = sqrt(b_i / a_i), as rounding.inc), and every constraint with an LP entry is a bound row
// 2 a X_pq + c x_j = b: one off-diagonal SDP entry and one LP column that occurs nowhere else and has no objective.  For labels l_p
// in {0..k-1} the point X(l)_pq = t_p t_q (l_p = l_q), -t_p t_q / (k - 1) (otherwise) is PSD and meets every diagonal constraint.
// Per cone, trial and part a Gaussian g_a (rounding.inc's k_rnd_gauss, the part in bits 26..31 of the counter: part 0 is the +-1
// rounding's hyperplane); l_p = the lowest a that attains max_a R_p . g_a; f = sum_k <C_k, X(l_k)>; then a deterministic 1-move local
// search by colour classes of the cone's stored off-diagonal graph (rnd_colour).
//
// Labels: one byte per (row, trial) in blocks of 64 trials, lab[(w * n + p) * 64 + lane]: a wavefront of the field pass (lane = trial)
// reads a neighbour's 64 labels as one 64-byte segment.  Everything is read-only on the solver's state, as in rounding.inc: R is formed
// on the fly, the scratch is the feature's own (KCutScratch), launches go straight to the stream, every sum has one fixed order.
// The driver around the label and field kernels is rounding.inc's (round_begin, round_reserve, round_vectors, round_drive).

namespace {

constexpr int KCUT_CH = 16;            // parts whose sums h_a a walk of the row list holds at once (LDS, one column per thread)

// the whole score chain of one part over the rl columns in fours, ascending: mfma_fm_tile's steps -- the same operands (A's element
// times zero and a clamped load past rl) in the same order, so the same bits -- as postsolve.inc's mfma_chain issues them, with the
// operands of several steps in flight
__device__ __forceinline__ v4f64 kcut_chain(const double *__restrict__ U, const double *__restrict__ V, bool uv, size_t ao,
                                            const double *__restrict__ Ga, size_t K, int rl, int kk) {
    return mfma_chain((rl + 3) & ~3, [&](int k0, double &x, double &y) {
        const int k = k0 + kk, kc = k < rl ? k : 0;
        x = factor_ld(U, V, uv, ao + kc) * (k < rl ? 1.0 : 0.0);
        y = Ga[(size_t)kc * K];
    });
}

// Labels of 16 rows x 16 trials per wavefront on the FP64 matrix cores.  For a = 0 .. parts - 1 one chain of mfma_fm_tile's steps
// (kcut_chain) over the cone's own rl columns with B[kk][nn] = g_a[column kk][trial t0 + nn] (a 128-byte segment of G's row);
// result register q of lane (nn, kk) is the score of row p0 + kk + 4 q and trial t0 + nn, and the lane keeps its running maximum
// and the a that gave it (strict > in ascending a: the lowest a wins a tie).  No cross-lane work; rows past n and trials past K are
// clamped loads whose results are not stored (rows) or stored as label 0 (trials: the label blocks are whole, nobody reads their
// pad lanes into a result).
// Wavefronts of one trial tile are neighbours in the grid, so the tile's part of G stays in cache while the rows go by.
__global__ __launch_bounds__(TPB) void k_kcut_label(int n, int rl, int r, int K, int W, int parts, const double *__restrict__ U,
                                                    const double *__restrict__ V, int uv, const double *__restrict__ G,
                                                    unsigned char *__restrict__ lab) {
    const int l = threadIdx.x & 63, nn = l & 15, kk = l >> 4;
    const int nrt = (n + 15) / 16;
    const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TPB / 64) + (threadIdx.x >> 6)));
    if (gw >= nrt * W * 4) return;
    const int p0 = (gw % nrt) * 16, t = (gw / nrt) * 16 + nn, tc = t < K ? t : K - 1;
    const size_t ao = (size_t)(p0 + nn < n ? p0 + nn : n - 1) * r;
    double best[4] = {0.0, 0.0, 0.0, 0.0};
    int arg[4] = {0, 0, 0, 0};
    for (int a = 0; a < parts; ++a) {
        const double *Ga = G + (size_t)a * rl * K + tc;
        const v4f64 acc = kcut_chain(U, V, uv != 0, ao, Ga, (size_t)K, rl, kk);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (a == 0 || acc[q] > best[q]) { best[q] = acc[q]; arg[q] = a; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = p0 + kk + 4 * q;
        if (p < n) lab[((size_t)(t >> 6) * n + p) * 64 + (t & 63)] = (unsigned char)(t < K ? arg[q] : 0);
    }
}

// row p's list in its stored order: f(q, C_pq) for every stored position of the row, the diagonal included.  A sparse cone walks the
// union pattern's adjacency with C from cbase (adj_sval is not C on the slots a bound row touches); a dense-C cone walks the row of
// Cfull and passes over its zeros.
template <typename F>
__device__ __forceinline__ void kcut_walk(int p, int n, const int *__restrict__ adj_ptr, const int *__restrict__ adj_col,
                                          const int *__restrict__ adj_e, const double *__restrict__ cbase,
                                          const double *__restrict__ Cfull, int npad, F f) {
    if (Cfull) {
        const double *crow = Cfull + (size_t)p * npad;
        for (int q = 0; q < n; ++q) {
            const double cq = crow[q];
            if (cq != 0.0) f(q, cq);
        }
    } else {
        for (int s = adj_ptr[p]; s < adj_ptr[p + 1]; ++s) f(adj_col[s], cbase[adj_e[s]]);
    }
}

// The field pass, one wavefront per (row, block of 64 trials), lane = trial.
//   eval (rows == null): per-workgroup partials of sum_p t_p (C_pp t_p + (same_p - other_p / (k - 1))), same_p / other_p the sums of
//   C_pq t_q over the q != p of p's part / of the other parts, each in the row list's order; part[t * RND_STRIPS + strip].
//   local search: the rows of one colour class.  h_a = sum_{q != p, l_q = a} C_pq t_q, every h_a on its own in the row list's order
//   (KCUT_CH of them per walk, one LDS column per thread); a* = the lowest a that attains min_a h_a; the row moves to a* where
//   Delta = coef t_p (h_a* - h_lp) < -tau_p, tau_p = 2^-40 coef t_p sum_{q != p} |C_pq| t_q, coef = 2 k / (k - 1); a mover stores its
//   label and 1 to *flag.  No two rows of a class are adjacent: no row reads a label this launch writes, except across a zero of a
//   dense C, which kcut_walk passes over.
__global__ __launch_bounds__(TPB) void k_kcut_field(int nrows, const int *__restrict__ rows, int n, int K, int parts, double inv,
                                                    double coef, const int *__restrict__ adj_ptr, const int *__restrict__ adj_col,
                                                    const int *__restrict__ adj_e, const double *__restrict__ cbase,
                                                    const double *__restrict__ Cfull, int npad, const double *__restrict__ tv,
                                                    unsigned char *__restrict__ lab, double *__restrict__ part, int *__restrict__ flag) {
    __shared__ double sh[KCUT_CH][TPB];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int w = blockIdx.y, strip = blockIdx.x;
    const int t = w * 64 + lane;
    const bool valid = t < K;
    unsigned char *lw = lab + (size_t)w * n * 64 + lane;
    double acc = 0.0;
    for (int i = strip * (TPB / 64) + wv; i < nrows; i += gridDim.x * (TPB / 64)) {
        const int p = __builtin_amdgcn_readfirstlane(rows ? rows[i] : i);
        const int lp = lw[(size_t)p * 64];
        const double tp = tv[p];
        if (!rows) {
            double same = 0.0, other = 0.0, cpp = 0.0;
            kcut_walk(p, n, adj_ptr, adj_col, adj_e, cbase, Cfull, npad, [&](int q, double cq) {
                if (q == p) { cpp = cq; return; }
                const double v = cq * tv[q];
                if (lw[(size_t)q * 64] == lp) same += v; else other += v;
            });
            acc += tp * (cpp * tp + (same - other * inv));
            continue;
        }
        double hmin = INFINITY, hcur = 0.0, asum = 0.0;
        int amin = 0;
        for (int a0 = 0; a0 < parts; a0 += KCUT_CH) {
#pragma unroll
            for (int j = 0; j < KCUT_CH; ++j) sh[j][tid] = 0.0;
            kcut_walk(p, n, adj_ptr, adj_col, adj_e, cbase, Cfull, npad, [&](int q, double cq) {
                if (q == p) return;
                const double tq = tv[q];
                const unsigned j = (unsigned)((int)lw[(size_t)q * 64] - a0);
                if (j < (unsigned)KCUT_CH) sh[j][tid] += cq * tq;
                if (a0 == 0) asum += fabs(cq) * tq;
            });
            const int na = parts - a0 < KCUT_CH ? parts - a0 : KCUT_CH;
            for (int j = 0; j < na; ++j) {
                const double h = sh[j][tid];
                if (h < hmin) { hmin = h; amin = a0 + j; }
                if (a0 + j == lp) hcur = h;
            }
        }
        const double delta = coef * tp * (hmin - hcur), tau = 0x1p-40 * coef * tp * asum;
        if (valid && delta < -tau) { lw[(size_t)p * 64] = (unsigned char)amin; flag[0] = 1; }
    }
    if (rows) return;
    sh[0][tid] = acc;
    __syncthreads();
    if (wv == 0 && valid) part[(size_t)t * RND_STRIPS + strip] = ((sh[0][lane] + sh[0][64 + lane]) + sh[0][128 + lane]) + sh[0][192 + lane];
}

// ---- the constraint data as the applicability checks read it: read_constraints and blocks_admit_bound_rows of rounding.inc (shared
// with its check of a cut-tightened context and with stable.inc)
// entries of constraint E in the LP block lpk
inline int lp_entries(const std::vector<ConEnt> &E, int lpk) {
    int lp = 0;
    for (const ConEnt &e : E) lp += e.k == lpk;
    return lp;
}
// A constraint with an LP entry as the bound row 2 a X_pq + c x_j = b (what lrd_session_write_bounded appends): one off-diagonal
// cone entry and one LP column, neither coefficient zero.  "" and the row, or the reason it is none.
struct BoundRow { int i, k, p, q, j; double a, cc; };
std::string bound_row(int i, const std::vector<ConEnt> &E, int lpk, BoundRow &r) {
    char msg[256];
    int lp = 0, sdp = 0;
    const ConEnt *el = nullptr, *es = nullptr;
    for (const ConEnt &e : E) {
        if (e.k == lpk) { ++lp; el = &e; } else { ++sdp; es = &e; }
    }
    if (lp != 1) { snprintf(msg, sizeof msg, "constraint %d has %d LP entries", i + 1, lp); return msg; }
    if (sdp != 1) { snprintf(msg, sizeof msg, "constraint %d has an LP entry and %d cone entries", i + 1, sdp); return msg; }
    if (es->p == es->q) { snprintf(msg, sizeof msg, "constraint %d has an LP entry and a diagonal entry", i + 1); return msg; }
    if (el->a == 0.0 || es->a == 0.0) { snprintf(msg, sizeof msg, "constraint %d has a zero coefficient", i + 1); return msg; }
    r = {i, es->k, es->p, es->q, el->p, es->a, el->a};
    return "";
}
// every LP column in exactly one bound row and without an objective ("" or the reason)
std::string lp_columns_only_bound(const std::vector<int> &col_use, const std::vector<double> &cobj) {
    char msg[256];
    for (size_t j = 0; j < col_use.size(); ++j) {
        if (col_use[j] != 1) { snprintf(msg, sizeof msg, "LP column %d occurs in %d constraints", (int)j + 1, col_use[j]); return msg; }
        if (cobj[j] != 0.0) { snprintf(msg, sizeof msg, "LP column %d has an objective coefficient", (int)j + 1); return msg; }
    }
    return "";
}

// Applicability (once per context: the constraint data never changes).  Without an LP block it is rnd_check's answer and t; with one
// the constraint data is read back and checked here, and t and the bounds u_j of the LP columns are kept.
int kcut_check(lorads_hip_ctx *c) {
    KCutScratch &X = c->kcut;
    if (X.checked) return 0;
    if (rnd_check(c)) return 1;
    const RoundScratch &Rn = c->rnd;
    X.qualifies = false;
    X.why.clear();
    X.t = nullptr;
    X.lp_u.clear();
    int lpk = -1;
    const std::string blocks = blocks_admit_bound_rows(c, &lpk);
    if (lpk < 0) {
        X.qualifies = Rn.qualifies;
        X.why = Rn.why;
        X.t = Rn.t;
        X.checked = true;
        return 0;
    }
    char msg[256];
    X.why = blocks;
    if (!X.why.empty()) { X.checked = true; return 0; }
    ConData D;
    if (read_constraints(c, D)) return 1;
    const std::vector<double> &b = D.b;
    std::vector<double> th((size_t)Rn.t_off[c->nb], 0.0);
    const int nl = c->blk[lpk].n;
    std::vector<int> col_use((size_t)nl, 0);
    std::vector<std::vector<int>> cover((size_t)c->nb);
    for (int k = 0; k < c->nb; ++k) cover[k].assign((size_t)c->blk[k].n, 0);
    X.lp_u.assign((size_t)nl, 0.0);
    std::vector<BoundRow> brow;
    for (int i = 0; i < c->m && X.why.empty(); ++i) {
        const std::vector<ConEnt> &E = D.con[(size_t)i];
        if (lp_entries(E, lpk) == 0) {
            const int sdp = (int)E.size();
            const ConEnt *es = sdp ? &E.back() : nullptr;
            if (sdp != 1) { snprintf(msg, sizeof msg, "constraint %d has %d stored entries", i + 1, sdp); X.why = msg; break; }
            if (es->p != es->q) { snprintf(msg, sizeof msg, "constraint %d is not on a diagonal", i + 1); X.why = msg; break; }
            const double ratio = b[(size_t)i] / es->a;
            if (!(ratio > 0) || !std::isfinite(ratio)) {
                snprintf(msg, sizeof msg, "constraint %d has b / a = %g (not positive)", i + 1, ratio);
                X.why = msg;
                break;
            }
            cover[es->k][es->p]++;
            th[(size_t)Rn.t_off[es->k] + es->p] = std::sqrt(ratio);
        } else {
            BoundRow r;
            X.why = bound_row(i, E, lpk, r);
            if (!X.why.empty()) break;
            col_use[(size_t)r.j]++;
            brow.push_back(r);
        }
    }
    for (int k = 0; k < c->nb && X.why.empty(); ++k) {
        if (k == lpk) continue;
        for (int p = 0; p < c->blk[k].n && X.why.empty(); ++p)
            if (cover[k][p] != 1) {
                snprintf(msg, sizeof msg, "diagonal %d of cone %d is fixed by %d constraints", p + 1, k + 1, cover[k][p]);
                X.why = msg;
            }
    }
    if (X.why.empty()) X.why = lp_columns_only_bound(col_use, D.cobj);
    X.qualifies = X.why.empty();
    if (X.qualifies) {
        for (const BoundRow &r : brow) // x_j = (b - 2 a X_pq) / c and |X_pq| <= t_p t_q
            X.lp_u[(size_t)r.j] = (std::fabs(b[(size_t)r.i]) + 2.0 * std::fabs(r.a) * th[(size_t)Rn.t_off[r.k] + r.p] * th[(size_t)Rn.t_off[r.k] + r.q]) /
                                  std::fabs(r.cc);
        if (X.mem.upload(&X.t_own, th)) return 1;
        X.t = X.t_own;
    }
    X.checked = true;
    return 0;
}

const RoundFeature FT_KCUT{"round_kcut", "k-cut-structured", kcut_check, false};

} // namespace

extern "C" int lorads_hip_round_kcut(lorads_hip_ctx *c, int32_t src, int32_t parts, int32_t trials, uint64_t seed, int32_t max_rounds,
                                     double *obj, double *obj0, int32_t *best, int32_t *best0, uint8_t *label, int32_t *rounds,
                                     double *vectors, double *t, double *lp_upper) {
    if (const int rc = round_begin(c, FT_KCUT, c ? &c->kcut : nullptr, src, &parts, trials, max_rounds, obj)) return rc;
    KCutScratch &X = c->kcut;
    const std::vector<int> &off = c->rnd.t_off;
    if (t) { // t of the SDP cones, cone after cone
        size_t at = 0;
        for (int k = 0; k < c->nb; ++k) {
            const Block &B = c->blk[k];
            if (B.is_lp) continue;
            if (B.n) HC(hipMemcpyAsync(t + at, X.t + off[k], sizeof(double) * (size_t)B.n, hipMemcpyDeviceToHost, c->stream));
            at += (size_t)B.n;
        }
        HC(hipStreamSynchronize(c->stream));
    }
    if (lp_upper)
        for (size_t j = 0; j < X.lp_u.size(); ++j) lp_upper[j] = X.lp_u[j];
    if (trials == 0) return 0;
    const int K = trials, W = (K + 63) / 64;
    TrialScratch &T = X.trial;
    if (round_reserve(c, T, X.mem, K, parts, true) || X.lab.grow(X.mem, (size_t)off[c->nb] * W * 64) || (max_rounds > 0 && rnd_colour(c))) return 1;
    // vectors and labels
    if (round_vectors(c, T, K, parts, seed, false, vectors, [&](int k, const double *G) {
            const Block &B = c->blk[k];
            const FactorView F = factor_view(c, src, k);
            const size_t waves = (size_t)nblocks_for((size_t)B.n, 16) * W * 4;
            if (B.n) hipLaunchKernelGGL(k_kcut_label, dim3(nblocks_for(waves, TPB / 64)), dim3(TPB), 0, c->stream, B.n, B.rl, B.r, K, W, parts,
                                        F.U, F.V, F.uv, G, X.lab + (size_t)off[k] * W * 64);
            return 0;
        }))
        return 1;
    auto field = [&](int k, const int *rows, int nrows) {
        const Block &B = c->blk[k];
        hipLaunchKernelGGL(k_kcut_field, dim3(field_strips(rows, nrows), W), dim3(TPB), 0, c->stream, nrows, rows, B.n, K, parts,
                           1.0 / (parts - 1), 2.0 * parts / (parts - 1), (const int *)B.pu.adj_ptr, (const int *)B.pu.adj_col,
                           (const int *)B.pu.adj_e, (const double *)B.pu.cbase, (const double *)(B.dense_c ? B.Cfull : nullptr), B.npad,
                           (const double *)(X.t + off[k]), X.lab + (size_t)off[k] * W * 64, T.part.p, T.ctl);
    };
    int bt = 0;
    if (round_drive(c, K, max_rounds, T, field, RoundOut{obj, obj0, best, best0, rounds}, &bt)) return 1;
    if (label) { // the best trial's labels, SDP cone after SDP cone: its 64-trial block of every row, then the trial's byte
        const int w = bt / 64, l = bt % 64;
        std::vector<unsigned char> blkb;
        size_t at = 0;
        for (int k = 0; k < c->nb; ++k) {
            const Block &B = c->blk[k];
            if (B.is_lp) continue;
            blkb.resize((size_t)B.n * 64);
            if (B.n) HC(hipMemcpyAsync(blkb.data(), X.lab + (size_t)off[k] * W * 64 + (size_t)w * B.n * 64, blkb.size(), hipMemcpyDeviceToHost,
                                       c->stream));
            HC(hipStreamSynchronize(c->stream));
            for (int p = 0; p < B.n; ++p) label[at + p] = blkb[(size_t)p * 64 + l];
            at += (size_t)B.n;
        }
    }
    return 0;
}
