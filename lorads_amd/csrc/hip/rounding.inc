// rounding.inc -- hyperplane rounding and 1-flip local search of +-1-structured contexts (Max-Cut, weighted Max-Cut, +-1 QUBO
// relaxations and their scaled forms), included by lorads_hip.hip after solution.inc.  DESIGN.md section 11.
//
// A context qualifies when it has no LP block and every constraint is a_i X_k[p,p] = b_i with b_i / a_i > 0, one per diagonal
// position of every cone.  Then x = sigma o t (t_p = sqrt(b_i / a_i)) is feasible for every sigma in {+-1}^n.  Per cone and trial a
// Gaussian hyperplane g (counter-based: it depends on (seed, cone, trial, column) alone) gives sigma_p = sign(R_p . g); f = x^T C x;
// then a deterministic 1-flip local search by colour classes of C's off-diagonal graph.  A context whose one LP block holds the slacks
// of triangle cuts and nothing else qualifies too (rnd_check_tightened; DESIGN.md section 20): its field pass is k_rnd_field_cuts.
//
// Sign words: bit l of word sgn[w * n + p] is trial 64 w + l of row p (1: sigma = +1).  A wavefront works on one word (lane = trial),
// so the words of a row's neighbours are wave-uniform loads.  Everything is read-only on the solver's state: R is formed on the fly
// from U and V as the export forms it, the scratch is the feature's own (RoundScratch), launches go straight to the stream (never
// through LAUNCH, which would flush a waiting dual update), and every sum is reduced per workgroup and then in a fixed order.
//
// Shared with kcut.inc, stable.inc and bisect.inc (DESIGN.md sections 16, 18, 19): the Gaussian kernel k_rnd_gauss, the sign kernel,
// read_constraint_image, and the driver of a rounding call below the checks -- round_begin .. round_stored_trial.

namespace {

constexpr int RND_MAXK = 65536;   // trials per call
constexpr int KCUT_MAXPARTS = 64;      // parts of the rounding into k parts (kcut.inc; round_begin checks both)
constexpr int KCUT_MAXPROD = 1 << 20;  // its trials x parts
constexpr int RND_STRIPS = 256;   // row strips of the field pass: per-trial partials per cone (fixed: f's summation order is K's own)
constexpr int RND_RPW = 8;        // rows per wavefront of the sign pass (one load of G's column serves them all)

// splitmix64 of x: the output of the generator whose state was x before its step
__device__ __host__ __forceinline__ uint64_t rnd_sm(uint64_t x) {
    uint64_t z = x + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// G of cone `cone` (parts x rk x K, G[(a * rk + j) * K + t]): c = (cone << 32) | (a << 26) | (t << 10) | j, x = sm(seed ^ sm(2c)),
// y = sm(seed ^ sm(2c + 1)), u1 = ((x >> 11) + 1) 2^-53 in (0, 1], u2 = (y >> 11) 2^-53 in [0, 1), g = sqrt(-2 ln u1) cos(2 pi u2).
// The +-1 rounding's hyperplanes are parts = 1: part 0 of the rounding into k parts.
__global__ __launch_bounds__(TPB) void k_rnd_gauss(int rk, int K, int parts, int cone, uint64_t seed, double *__restrict__ G) {
    const size_t per = (size_t)rk * K, len = per * parts;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < len; i += (size_t)gridDim.x * TPB) {
        const uint64_t a = i / per, rem = i % per, j = rem / K, t = rem % K;
        const uint64_t ctr = ((uint64_t)cone << 32) | (a << 26) | (t << 10) | j;
        const uint64_t x = rnd_sm(seed ^ rnd_sm(2 * ctr)), y = rnd_sm(seed ^ rnd_sm(2 * ctr + 1));
        const double u1 = (double)((x >> 11) + 1) * 0x1p-53, u2 = (double)(y >> 11) * 0x1p-53;
        G[i] = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
    }
}

// sign words of RND_RPW rows and one word of trials per wavefront: s = R_p . g_t over the cone's own rk columns (R = (U + V) / 2 or R,
// row stride r), bit = s >= 0; lanes past K give 0 bits.  Wavefronts of one word are neighbours in the grid, so G's 64 columns of
// the word stay in cache while its rows go by; the rows of R are wave-uniform (scalar) loads.
__global__ __launch_bounds__(TPB) void k_rnd_sign(int n, int rk, int r, int K, int W, const double *__restrict__ U,
                                                  const double *__restrict__ V, int uv, const double *__restrict__ G,
                                                  unsigned long long *__restrict__ sgn) {
    const int lane = threadIdx.x & 63;
    const int nch = (n + RND_RPW - 1) / RND_RPW;
    const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TPB / 64) + (threadIdx.x >> 6)));
    if (gw >= nch * W) return;
    const int w = gw / nch, p0 = (gw % nch) * RND_RPW;
    const int t = w * 64 + lane;
    const bool valid = t < K;
    double s[RND_RPW];
#pragma unroll
    for (int i = 0; i < RND_RPW; ++i) s[i] = 0.0;
    for (int j = 0; j < rk; ++j) {
        const double g = valid ? G[(size_t)j * K + t] : 0.0;
#pragma unroll
        for (int i = 0; i < RND_RPW; ++i) {
            const int p = p0 + i < n ? p0 + i : n - 1;
            s[i] += factor_ld(U, V, uv != 0, (size_t)p * r + j) * g;
        }
    }
#pragma unroll
    for (int i = 0; i < RND_RPW; ++i) {
        const unsigned long long word = __ballot(valid && s[i] >= 0.0);
        if (lane == 0 && p0 + i < n) sgn[(size_t)w * n + p0 + i] = word;
    }
}

// The field pass, one wavefront per (row, word), lane = trial: h_p = sum_{q != p} C_pq x_q over p's row list in its stored order
// (the union pattern's adjacency; the dense row of a dense-C cone), x = sigma o t.
//   eval (rows == null): per-workgroup partials of sum_p x_p (h_p + C_pp x_p), part[t * RND_STRIPS + strip]
//   local search: the rows of one colour class; flip where Delta_p = -4 x_p h_p < -tau_p, tau_p = 2^-40 4 t_p sum_{q != p} |C_pq| t_q,
//   and raise *flag (every writer writes 1).  No two rows of a class are adjacent: no row reads a word this launch writes.
// The off-diagonal slots of a cone without cut rows are untouched by constraints, so adj_sval holds their C; C_pp comes from cbase.
// CUTS (k_rnd_field_cuts, a cut-tightened context: DESIGN.md section 20): the triangle rows touch off-diagonal slots, where adj_sval
// is no longer C, so every slot's C comes from cbase[adj_e[.]] as in kcut_walk; a cut position outside C's pattern has C = 0 there and
// adds a zero product, which changes no sum's bits.
template <bool CUTS>
__device__ __forceinline__ void rnd_field(int nrows, const int *__restrict__ rows, int n, int K, const int *__restrict__ adj_ptr,
                                          const int *__restrict__ adj_col, const int *__restrict__ adj_e,
                                          const double *__restrict__ adj_sval, const double *__restrict__ cbase,
                                          const double *__restrict__ Cfull, int npad, const double *__restrict__ tv,
                                          unsigned long long *__restrict__ sgn, double *__restrict__ part, int *__restrict__ flag) {
    __shared__ double sh[TPB];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int w = blockIdx.y, strip = blockIdx.x;
    const int t = w * 64 + lane;
    const bool valid = t < K;
    unsigned long long *sw = sgn + (size_t)w * n;
    double acc = 0.0;
    for (int i = strip * (TPB / 64) + wv; i < nrows; i += gridDim.x * (TPB / 64)) {
        const int p = __builtin_amdgcn_readfirstlane(rows ? rows[i] : i);
        double h = 0.0, a = 0.0, cpp = 0.0;
        if (Cfull) {
            const double *crow = Cfull + (size_t)p * npad;
            for (int q = 0; q < n; ++q) {
                const double cq = crow[q];
                if (q == p) { cpp = cq; continue; }
                const double tq = tv[q];
                h += cq * (((sw[q] >> lane) & 1ull) ? tq : -tq);
                a += fabs(cq) * tq;
            }
        } else {
            for (int k = adj_ptr[p]; k < adj_ptr[p + 1]; ++k) {
                const int q = adj_col[k];
                if (q == p) { cpp = cbase[adj_e[k]]; continue; }
                const double cq = CUTS ? cbase[adj_e[k]] : adj_sval[k], tq = tv[q];
                h += cq * (((sw[q] >> lane) & 1ull) ? tq : -tq);
                a += fabs(cq) * tq;
            }
        }
        const unsigned long long wp = sw[p];
        const double tp = tv[p];
        const double xp = ((wp >> lane) & 1ull) ? tp : -tp;
        if (!rows) {
            acc += xp * (h + cpp * xp);
        } else {
            const double delta = -4.0 * xp * h, tau = 0x1p-40 * 4.0 * tp * a;
            const unsigned long long fl = __ballot(valid && delta < -tau);
            if (lane == 0 && fl) { sw[p] = wp ^ fl; flag[0] = 1; }
        }
    }
    if (rows) return;
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (wv == 0 && valid) part[(size_t)t * RND_STRIPS + strip] = ((sh[lane] + sh[64 + lane]) + sh[128 + lane]) + sh[192 + lane];
}
#define RND_FIELD_ARGS                                                                                                                  \
    int nrows, const int *__restrict__ rows, int n, int K, const int *__restrict__ adj_ptr, const int *__restrict__ adj_col,           \
        const int *__restrict__ adj_e, const double *__restrict__ adj_sval, const double *__restrict__ cbase,                          \
        const double *__restrict__ Cfull, int npad, const double *__restrict__ tv, unsigned long long *__restrict__ sgn,               \
        double *__restrict__ part, int *__restrict__ flag
__global__ __launch_bounds__(TPB) void k_rnd_field(RND_FIELD_ARGS) {
    rnd_field<false>(nrows, rows, n, K, adj_ptr, adj_col, adj_e, adj_sval, cbase, Cfull, npad, tv, sgn, part, flag);
}
__global__ __launch_bounds__(TPB) void k_rnd_field_cuts(RND_FIELD_ARGS) {
    rnd_field<true>(nrows, rows, n, K, adj_ptr, adj_col, adj_e, adj_sval, cbase, Cfull, npad, tv, sgn, part, flag);
}
#undef RND_FIELD_ARGS

// f[t] (= or +=) sum of the strips' partials of trial t, in strip order
__global__ __launch_bounds__(TPB) void k_rnd_sum(int K, int nstrip, const double *__restrict__ part, double *__restrict__ f, int first) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= K) return;
    double s = 0.0;
    for (int b = 0; b < nstrip; ++b) s += part[(size_t)t * RND_STRIPS + b];
    f[t] = first ? s : f[t] + s;
}

// *best = argmin_t f[t], the lowest index on ties (one workgroup)
__global__ __launch_bounds__(TPB) void k_rnd_best(int K, const double *__restrict__ f, int *__restrict__ best) {
    __shared__ double sv[TPB];
    __shared__ int si[TPB];
    double v = INFINITY;
    int idx = K;
    for (int t = threadIdx.x; t < K; t += TPB)
        if (f[t] < v || idx == K) { v = f[t]; idx = t; }
    sv[threadIdx.x] = v; si[threadIdx.x] = idx;
    __syncthreads();
    for (int o = TPB / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double v2 = sv[threadIdx.x + o];
            const int i2 = si[threadIdx.x + o];
            if (i2 < K && (si[threadIdx.x] == K || v2 < sv[threadIdx.x] || (v2 == sv[threadIdx.x] && i2 < si[threadIdx.x]))) {
                sv[threadIdx.x] = v2; si[threadIdx.x] = i2;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *best = si[0];
}

// cone k's constraint image read back to the host: local constraint -> its global row (ri) and its entries (ap, ae, av) on the
// A-pattern (er, ec)
struct ConImage { std::vector<int> ri, ap, ae, er, ec; std::vector<double> av; };
int read_constraint_image(lorads_hip_ctx *c, int k, ConImage &m) {
    const Block &B = c->blk[k];
    m.ri.assign(B.nrow, 0); m.ap.assign(B.nrow + 1, 0); m.ae.assign(B.na, 0); m.er.assign(B.pa.ne, 0); m.ec.assign(B.pa.ne, 0);
    m.av.assign(B.na, 0.0);
    if (B.nrow) {
        HC(hipMemcpyAsync(m.ri.data(), B.row_idx, sizeof(int) * m.ri.size(), hipMemcpyDeviceToHost, c->stream));
        HC(hipMemcpyAsync(m.ap.data(), B.a_ptr, sizeof(int) * m.ap.size(), hipMemcpyDeviceToHost, c->stream));
    }
    if (B.na) {
        HC(hipMemcpyAsync(m.ae.data(), B.a_e, sizeof(int) * m.ae.size(), hipMemcpyDeviceToHost, c->stream));
        HC(hipMemcpyAsync(m.av.data(), B.a_val, sizeof(double) * m.av.size(), hipMemcpyDeviceToHost, c->stream));
    }
    if (B.pa.ne) {
        HC(hipMemcpyAsync(m.er.data(), B.pa.erow, sizeof(int) * m.er.size(), hipMemcpyDeviceToHost, c->stream));
        HC(hipMemcpyAsync(m.ec.data(), B.pa.ecol, sizeof(int) * m.ec.size(), hipMemcpyDeviceToHost, c->stream));
    }
    HC(hipStreamSynchronize(c->stream));
    return 0;
}

// Constraint gi's one stored entry a at (p, q) as the diagonal row a X[p,p] = b with b / a > 0 (shared with bisect.inc): "" and
// *t = sqrt(b / a), or the reason it is none (*t is then left as it was)
std::string diag_row(int gi, int p, int q, double a, double b, double *t) {
    char msg[256];
    if (p != q) { snprintf(msg, sizeof msg, "constraint %d is not on a diagonal", gi + 1); return msg; }
    const double ratio = b / a;
    if (!(ratio > 0) || !std::isfinite(ratio)) {
        snprintf(msg, sizeof msg, "constraint %d has b / a = %g (not positive)", gi + 1, ratio);
        return msg;
    }
    *t = std::sqrt(ratio);
    return "";
}

// ---- the constraint data as the applicability checks read it (shared with kcut.inc and stable.inc)
// every stored entry, constraint by constraint: (block, row, column, coefficient); b; the LP block's objective
struct ConEnt { int k, p, q; double a; };
struct ConData {
    std::vector<std::vector<ConEnt>> con;
    std::vector<double> b, cobj;
};
int read_constraints(lorads_hip_ctx *c, ConData &D) {
    D.con.assign((size_t)c->m, {});
    D.b.assign((size_t)c->m, 0.0);
    D.cobj.clear();
    if (c->m) HC(hipMemcpyAsync(D.b.data(), c->b, sizeof(double) * D.b.size(), hipMemcpyDeviceToHost, c->stream));
    for (int k = 0; k < c->nb; ++k) {
        const Block &B = c->blk[k];
        if (B.is_lp) { // (read_constraint_image below synchronises for this copy too)
            D.cobj.resize((size_t)B.n);
            if (B.n) HC(hipMemcpyAsync(D.cobj.data(), B.lp_cobj, sizeof(double) * D.cobj.size(), hipMemcpyDeviceToHost, c->stream));
        }
        ConImage m;
        if (read_constraint_image(c, k, m)) return 1;
        for (int i = 0; i < B.nrow; ++i)
            for (int s = m.ap[i]; s < m.ap[i + 1]; ++s) D.con[(size_t)m.ri[i]].push_back({k, m.er[m.ae[s]], m.ec[m.ae[s]], m.av[s]});
    }
    return 0;
}
// what holds before any constraint is looked at: at most one LP block, a cone, no dense constraint matrices ("" or the reason)
std::string blocks_admit_bound_rows(const lorads_hip_ctx *c, int *lpk) {
    char msg[256];
    int nlp = 0, nsdp = 0;
    *lpk = -1;
    for (int k = 0; k < c->nb; ++k) {
        if (c->blk[k].is_lp) { ++nlp; *lpk = k; } else ++nsdp;
    }
    if (nlp > 1) return "more than one LP block";
    if (nsdp == 0) return "no cone";
    for (int k = 0; k < c->nb; ++k)
        if (c->blk[k].dense_a) { snprintf(msg, sizeof msg, "cone %d stores dense constraint matrices", k + 1); return msg; }
    return "";
}

// rnd_check on a context with an LP block, lpk: the cut-tightened +-1 structure (DESIGN.md section 20) by the rule the host applies to
// the problem image (lorads_cut_rows.h: the same text, so the same first reason).  A context that qualifies leaves t, the sorted
// packed indices of every cone's cuts on the device (a row named twice once) and u_j of the slack columns; one that does not leaves
// its reason and allocates nothing.
int rnd_check_tightened(lorads_hip_ctx *c, int lpk, const std::string &blocks) {
    RoundScratch &X = c->rnd;
    const std::string lead = "block " + std::to_string(lpk + 1) + " is an LP block";
    X.checked = true;
    if (!blocks.empty()) { X.why = lead + ": " + blocks; return 0; }
    ConData D;
    if (read_constraints(c, D)) { X.checked = false; return 1; }
    std::vector<int> dim((size_t)c->nb), ptr((size_t)c->m + 1, 0);
    std::vector<lrd_cr_entry> ent;
    for (int k = 0; k < c->nb; ++k) dim[k] = c->blk[k].n;
    for (int i = 0; i < c->m; ++i) {
        for (const ConEnt &e : D.con[(size_t)i]) ent.push_back({e.k, e.p, e.q, e.a});
        ptr[(size_t)i + 1] = (int)ent.size();
    }
    std::vector<double> th((size_t)X.t_off[c->nb] + 1, 0.0), u((size_t)dim[lpk] + 1, 0.0);
    std::vector<lrd_cr_cut> cut((size_t)c->m + 1);
    int ncut = 0;
    char why[256];
    const lrd_cr_problem P{c->m, c->nb, lpk, dim.data(), ptr.data(), ent.data(), D.b.data(), D.cobj.data()};
    if (lrd_cr_check(&P, X.t_off.data(), th.data(), cut.data(), &ncut, u.data(), why, sizeof why)) {
        X.why = lead + " whose columns are not all triangle-cut slacks: " + why;
        return 0;
    }
    th.resize((size_t)X.t_off[c->nb]);
    u.resize((size_t)dim[lpk]);
    std::vector<std::vector<unsigned long long>> idx((size_t)c->nb);
    for (int e = 0; e < ncut; ++e) {
        const unsigned long long n = (unsigned long long)dim[cut[e].cone];
        idx[cut[e].cone].push_back((((unsigned long long)cut[e].p * n + cut[e].q) * n + cut[e].s) * 4ull + (unsigned long long)cut[e].cls);
    }
    X.present.assign((size_t)c->nb, nullptr);
    X.npresent.assign((size_t)c->nb, 0);
    for (int k = 0; k < c->nb; ++k) {
        std::sort(idx[k].begin(), idx[k].end());
        idx[k].erase(std::unique(idx[k].begin(), idx[k].end()), idx[k].end());
        X.npresent[k] = (int)idx[k].size();
        if (!idx[k].empty() && X.mem.upload(&X.present[k], idx[k])) { X.checked = false; return 1; }
    }
    if (X.mem.upload(&X.t, th)) { X.checked = false; return 1; }
    X.lpk = lpk;
    X.lp_u = u;
    X.qualifies = true;
    return 0;
}

// applicability (once per context: the constraint data never changes); t of every cone to the device
int rnd_check(lorads_hip_ctx *c) {
    RoundScratch &X = c->rnd;
    if (X.checked) return 0;
    X.qualifies = false;
    X.why.clear();
    X.t_off.assign(c->nb + 1, 0);
    for (int k = 0; k < c->nb; ++k) X.t_off[k + 1] = X.t_off[k] + c->blk[k].n;
    {
        int lpk = -1;
        const std::string blocks = blocks_admit_bound_rows(c, &lpk);
        if (lpk >= 0) return rnd_check_tightened(c, lpk, blocks);
    }
    std::vector<double> b((size_t)c->m), th((size_t)X.t_off[c->nb], 0.0);
    if (c->m) HC(hipMemcpyAsync(b.data(), c->b, sizeof(double) * b.size(), hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    std::vector<int> per_con((size_t)c->m, 0);
    char msg[256];
    for (int k = 0; k < c->nb && X.why.empty(); ++k) {
        const Block &B = c->blk[k];
        if (B.dense_a) { snprintf(msg, sizeof msg, "cone %d stores dense constraint matrices", k + 1); X.why = msg; break; }
        ConImage m;
        if (read_constraint_image(c, k, m)) return 1;
        const std::vector<int> &ri = m.ri, &ap = m.ap, &ae = m.ae, &er = m.er, &ec = m.ec;
        const std::vector<double> &av = m.av;
        std::vector<int> cover((size_t)B.n, 0);
        for (int i = 0; i < B.nrow && X.why.empty(); ++i) {
            const int gi = ri[i], cnt = ap[i + 1] - ap[i];
            per_con[gi] += cnt;
            if (cnt != 1) { snprintf(msg, sizeof msg, "constraint %d has %d entries on cone %d", gi + 1, cnt, k + 1); X.why = msg; break; }
            const int e = ae[ap[i]], p = er[e];
            X.why = diag_row(gi, er[e], ec[e], av[ap[i]], b[gi], &th[X.t_off[k] + p]);
            if (!X.why.empty()) break;
            cover[p]++;
        }
        for (int p = 0; p < B.n && X.why.empty(); ++p)
            if (cover[p] != 1) {
                snprintf(msg, sizeof msg, "diagonal %d of cone %d is fixed by %d constraints", p + 1, k + 1, cover[p]);
                X.why = msg;
            }
    }
    for (int i = 0; i < c->m && X.why.empty(); ++i)
        if (per_con[i] != 1) { snprintf(msg, sizeof msg, "constraint %d has %d stored entries", i + 1, per_con[i]); X.why = msg; }
    if (c->nb == 0 && X.why.empty()) X.why = "no cone";
    X.qualifies = X.why.empty();
    if (X.qualifies && X.mem.upload(&X.t, th)) return 1;
    X.checked = true;
    return 0;
}

// greedy colouring of every cone's off-diagonal graph of C in increasing vertex order (a vertex takes the smallest colour that none
// of its lower-numbered neighbours holds) and the class-sorted row list (class by class, rows ascending within a class)
int rnd_colour(lorads_hip_ctx *c) {
    RoundScratch &X = c->rnd;
    if (X.coloured) return 0;
    std::vector<int> all((size_t)X.t_off[c->nb]);
    X.cls_ptr.assign(c->nb, {});
    for (int k = 0; k < c->nb; ++k) {
        const Block &B = c->blk[k];
        const int n = B.n;
        std::vector<int> ptr, col;
        if (B.dense_c) {
            std::vector<double> cf((size_t)B.npad * B.npad);
            HC(hipMemcpyAsync(cf.data(), B.Cfull, sizeof(double) * cf.size(), hipMemcpyDeviceToHost, c->stream));
            HC(hipStreamSynchronize(c->stream));
            ptr.assign(n + 1, 0);
            for (int p = 0; p < n; ++p) {
                for (int q = 0; q < n; ++q)
                    if (q != p && cf[(size_t)p * B.npad + q] != 0.0) col.push_back(q);
                ptr[p + 1] = (int)col.size();
            }
        } else {
            ptr.resize(n + 1);
            col.resize(B.pu.nslot);
            HC(hipMemcpyAsync(ptr.data(), B.pu.adj_ptr, sizeof(int) * ptr.size(), hipMemcpyDeviceToHost, c->stream));
            if (B.pu.nslot) HC(hipMemcpyAsync(col.data(), B.pu.adj_col, sizeof(int) * col.size(), hipMemcpyDeviceToHost, c->stream));
            HC(hipStreamSynchronize(c->stream));
        }
        std::vector<int> colour((size_t)n, 0), seen;
        int ncol = 0;
        for (int p = 0; p < n; ++p) {
            for (int s = ptr[p]; s < ptr[p + 1]; ++s) {
                const int q = col[s];
                if (q < p) { if ((int)seen.size() <= colour[q]) seen.resize(colour[q] + 1, -1); seen[colour[q]] = p; }
            }
            int cp = 0;
            while (cp < (int)seen.size() && seen[cp] == p) ++cp;
            colour[p] = cp;
            ncol = std::max(ncol, cp + 1);
        }
        std::vector<int> &cp = X.cls_ptr[k];
        cp.assign(ncol + 1, 0);
        for (int p = 0; p < n; ++p) cp[colour[p] + 1]++;
        for (int i = 0; i < ncol; ++i) cp[i + 1] += cp[i];
        std::vector<int> fill(cp.begin(), cp.end() - 1);
        for (int p = 0; p < n; ++p) all[X.t_off[k] + fill[colour[p]]++] = p;
    }
    if (X.mem.upload(&X.cls_rows, all)) return 1;
    X.coloured = true;
    return 0;
}

// ---- the driver of a rounding call, shared by the four roundings (kcut.inc, stable.inc, bisect.inc): round_begin, round_reserve,
// round_vectors, round_signs, round_drive (the field-pass features) or trial_chunks (the one-trial-per-workgroup features), round_finish,
// round_stored_trial.  A feature supplies its check, its kernels and its per-cone outputs.

// what a feature calls itself: in its messages, the structure it asks for, and its once-per-context check.  (Plain functions only:
// hipcc gives the captureless lambdas of several namespace-scope initialisers one name on the host, and all of them call the first.)
struct RoundFeature {
    const char *name, *structured;
    int (*check)(lorads_hip_ctx *);
    bool terse;   // a bad `trials` is "bad argument" like every other bad argument (round_pm1), not a sentence of its own
};

// The head of every lorads_hip_round_*: 0 to go on, else the entry point's return code with the message set -- 1 a bad argument or a
// failed check, 3 a sharded context, 2 a context that lacks the feature's structure.  A: what the feature's check leaves (NULL with
// a NULL context, which is refused before it is looked at).  `parts`: round_kcut's (its range and the product's are looked at where
// that entry point always did), NULL for a feature without parts.
int round_begin(lorads_hip_ctx *c, const RoundFeature &ft, const Applies *A, int32_t src, const int32_t *parts, int32_t trials,
                int32_t max_rounds, const double *obj) {
    const std::string who = ft.name;
    spec_touch(c);
    if (postsolve_args(c, src, nullptr, ft.name, true)) return 1;
    if (parts && (*parts < 2 || *parts > KCUT_MAXPARTS)) return fail_msg(who + ": parts " + std::to_string(*parts) + " is outside [2, 64]");
    if (trials < 0 || trials > RND_MAXK)
        return fail_msg(ft.terse ? who + ": bad argument" : who + ": trials " + std::to_string(trials) + " is outside [0, 65536]");
    if (parts && (int64_t)trials * *parts > KCUT_MAXPROD)
        return fail_msg(who + ": trials x parts = " + std::to_string((int64_t)trials * *parts) + " is above 2^20");
    if (max_rounds < 0 || (trials > 0 && !obj)) return fail_msg(who + ": bad argument");
    if (postsolve_sharded(c, ft.name, "cannot be rounded")) return 3;
    if (ft.check(c)) return 1;
    if (!A->qualifies) {
        fail_msg(who + ": the context is not " + ft.structured + ": " + A->why);
        return 2;
    }
    return 0;
}

// the driver's buffers for K trials of `parts` vectors per cone (grown on demand, freed with the feature's pool `mem`): the field
// partials for a field-pass feature, the rounds per trial otherwise.  T.K <- K: call it behind the feature's own allocations.
int round_reserve(lorads_hip_ctx *c, TrialScratch &T, DevPool &mem, int K, int parts, bool field_pass) {
    size_t g = 0;
    for (auto &B : c->blk)
        if (!B.is_lp) g += (size_t)B.rl * K * parts;
    if (T.G.grow(mem, g) || (field_pass ? T.part.grow(mem, (size_t)K * RND_STRIPS) : T.nround.grow(mem, (size_t)K))) return 1;
    if (T.f.grow(mem, (size_t)K) || T.f0.grow(mem, (size_t)K)) return 1;
    if (!T.ctl && mem.alloc(&T.ctl, 4)) return 1;
    T.K = K;
    return 0;
}

// cone k's vectors at G (parts x rank x K)
void round_gauss(lorads_hip_ctx *c, int k, int K, int parts, uint64_t seed, double *G) {
    const size_t glen = (size_t)c->blk[k].rl * K * parts;
    if (glen) hipLaunchKernelGGL(k_rnd_gauss, dim3(std::min(grid1d(glen), 1024)), dim3(TPB), 0, c->stream, c->blk[k].rl, K, parts, k, seed, G);
}

// Every cone's vectors, cone after cone in T.G, each followed by `each(k, G)`: what the feature launches on cone k's vectors (0, or 1
// with the message set).  LP blocks are passed over, and with skip_empty the cones without a row.  `out` (may be NULL) <- all of them.
template <typename Each>
int round_vectors(lorads_hip_ctx *c, TrialScratch &T, int K, int parts, uint64_t seed, bool skip_empty, double *out, Each each) {
    size_t goff = 0;
    for (int k = 0; k < c->nb; ++k) {
        const Block &B = c->blk[k];
        if (B.is_lp || (skip_empty && B.n == 0)) continue;
        double *G = T.G + goff;
        round_gauss(c, k, K, parts, seed, G);
        if (each(k, (const double *)G)) return 1;
        goff += (size_t)B.rl * K * parts;
    }
    if (out && goff) HC(hipMemcpyAsync(out, T.G, sizeof(double) * goff, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

// cone k's sign words of the hyperplanes G, W words of 64 trials per row, at sgn
void round_signs(lorads_hip_ctx *c, int32_t src, int k, int K, int W, const double *G, unsigned long long *sgn) {
    const Block &B = c->blk[k];
    const FactorView F = factor_view(c, src, k);
    const size_t waves = (size_t)nblocks_for((size_t)B.n, RND_RPW) * W;
    hipLaunchKernelGGL(k_rnd_sign, dim3(nblocks_for(waves, TPB / 64)), dim3(TPB), 0, c->stream, B.n, B.rl, B.r, K, W, F.U, F.V, F.uv, G, sgn);
}

// Trials per chunk of a one-trial-per-workgroup feature whose chunk holds `elems` (trial, vertex) pairs of the largest cone (nmax
// rows): elems / nmax rounded down to a multiple of `multiple`, at least 16, at most K -- and at most LORADS_TRIAL_CHUNK, rounded up
// to the multiple, where a test sets it.  trial_chunks walks the chunks [t0, t1) of K trials (body: 0, or 1 with the message set).
inline int trial_chunk(const lorads_hip_ctx *c, int K, int nmax, size_t elems, int multiple) {
    size_t ch = std::max<size_t>(16, elems / nmax / multiple * multiple);
    if (c->opt.trial_chunk > 0) ch = std::min(ch, ((size_t)c->opt.trial_chunk + multiple - 1) / multiple * multiple);
    return (int)std::min<size_t>((size_t)K, ch);
}
template <typename Body>
int trial_chunks(int K, int CH, Body body) {
    for (int t0 = 0; t0 < K; t0 += CH)
        if (body(t0, std::min(K, t0 + CH))) return 1;
    return 0;
}

// workgroups along x of a field pass over nrows rows (rows == null: all of a cone's, the evaluation: f's summation order is K's own)
inline int field_strips(const int *rows, int nrows) {
    return rows ? std::max(1, std::min(RND_STRIPS, nblocks_for((size_t)nrows, TPB / 64))) : RND_STRIPS;
}

// where a rounding's results go: the entry point's arguments of these names (all but obj may be NULL)
struct RoundOut {
    double *obj, *obj0;
    int32_t *best, *best0, *rounds;
};

// The tail of every rounding: the best of f0 and of f (the lowest index on ties), then obj, obj0, best, best0 and rounds to `o`, behind
// one synchronisation that also covers the copies the feature enqueued before it.  rounds = host_rounds, what the host counted (the
// field-pass features), or with host_rounds < 0 the maximum of T.nround (the one-trial-per-workgroup features).  *trial <- the best
// trial after the search.
int round_finish(lorads_hip_ctx *c, int K, TrialScratch &T, const double *f, int host_rounds, const RoundOut &o, int *trial) {
    hipLaunchKernelGGL(k_rnd_best, dim3(1), dim3(TPB), 0, c->stream, K, (const double *)T.f0, T.ctl + 1);
    hipLaunchKernelGGL(k_rnd_best, dim3(1), dim3(TPB), 0, c->stream, K, f, T.ctl + 2);
    int bb[2] = {0, 0};
    std::vector<int> nr(host_rounds < 0 ? (size_t)K : 0);
    HC(hipMemcpyAsync(bb, T.ctl + 1, sizeof(int) * 2, hipMemcpyDeviceToHost, c->stream));
    HC(hipMemcpyAsync(o.obj, f, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
    if (o.obj0) HC(hipMemcpyAsync(o.obj0, T.f0, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
    if (host_rounds < 0) HC(hipMemcpyAsync(nr.data(), T.nround.p, sizeof(int) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    if (o.best) *o.best = bb[1];
    if (o.best0) *o.best0 = bb[0];
    if (o.rounds) *o.rounds = host_rounds < 0 ? *std::max_element(nr.begin(), nr.end()) : host_rounds;
    *trial = bb[1];
    return 0;
}

// What the two field-pass roundings do with their trials once the signs / labels stand.  `field(k, rows, nrows)` launches the feature's
// field kernel for cone k over nrows rows (rows == null: all of them, the evaluation; otherwise a colour class of the search), leaving
// its partials in T.part and its change flag in T.ctl[0].  LP blocks are passed over.  f0 of every trial (every cone's field pass, its
// strips added per trial in cone order); the local search, one host synchronisation per round (the flag decides whether another round
// runs); f; then round_finish.
template <typename Field>
int round_drive(lorads_hip_ctx *c, int K, int max_rounds, TrialScratch &T, Field field, const RoundOut &o, int *trial) {
    const RoundScratch &Rn = c->rnd;
    auto eval = [&](double *f) {
        bool first = true;
        for (int k = 0; k < c->nb; ++k) {
            if (c->blk[k].is_lp) continue;
            field(k, (const int *)nullptr, c->blk[k].n);
            hipLaunchKernelGGL(k_rnd_sum, dim3(nblocks_for((size_t)K, TPB)), dim3(TPB), 0, c->stream, K, (int)RND_STRIPS,
                               (const double *)T.part, f, (int)first);
            first = false;
        }
    };
    eval(T.f0);
    int nr = 0;
    for (int round = 0; round < max_rounds; ++round) {
        HC(hipMemsetAsync(T.ctl, 0, sizeof(int), c->stream));
        for (int k = 0; k < c->nb; ++k) {
            if (c->blk[k].is_lp) continue;
            const std::vector<int> &cp = Rn.cls_ptr[k];
            for (size_t cl = 0; cl + 1 < cp.size(); ++cl) field(k, (const int *)(Rn.cls_rows + Rn.t_off[k] + cp[cl]), cp[cl + 1] - cp[cl]);
        }
        int flag = 0;
        HC(hipMemcpyAsync(&flag, T.ctl, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HC(hipStreamSynchronize(c->stream));
        nr = round + 1;
        if (!flag) break;
    }
    if (nr > 0) eval(T.f);
    return round_finish(c, K, T, nr > 0 ? T.f : T.f0, nr, o, trial);
}

// The bytes of trial `trial` of the last call of a one-trial-per-workgroup feature, cone after cone, each decoded by `decode`: cone k's
// trials stand at store + v_off[k] * K, n bytes each (v_off: [nb + 1], a block without vertices has none).
template <typename Byte, typename Decode>
int round_stored_trial(lorads_hip_ctx *c, const char *who, const TrialScratch &T, const std::vector<int> &v_off, const Byte *store, int32_t trial,
                       Byte *out, Decode decode) {
    if (T.K == 0 || trial < 0 || trial >= T.K) return fail_msg(std::string(who) + ": trial " + std::to_string(trial) + " is outside the last call's");
    for (int k = 0; k < c->nb; ++k) {
        const size_t n = (size_t)(v_off[k + 1] - v_off[k]);
        if (n) HC(hipMemcpyAsync(out + v_off[k], store + (size_t)v_off[k] * T.K + (size_t)trial * n, n, hipMemcpyDeviceToHost, c->stream));
    }
    HC(hipStreamSynchronize(c->stream));
    for (int p = 0; p < v_off[c->nb]; ++p) out[p] = decode(out[p]);
    return 0;
}

const RoundFeature FT_PM1{"round_pm1", "+-1-structured", rnd_check, true};

} // namespace

extern "C" int lorads_hip_round_pm1(lorads_hip_ctx *c, int32_t src, int32_t trials, uint64_t seed, int32_t max_rounds, double *obj,
                                    double *obj0, int32_t *best, int32_t *best0, int8_t *sign, int32_t *rounds,
                                    double *hyperplanes) {
    if (const int rc = round_begin(c, FT_PM1, c ? &c->rnd : nullptr, src, nullptr, trials, max_rounds, obj)) return rc;
    RoundScratch &X = c->rnd;
    if (trials == 0) return 0;
    const int K = trials, W = (K + 63) / 64;
    TrialScratch &T = X.trial;
    if (round_reserve(c, T, X.mem, K, 1, true) || X.sgn.grow(X.mem, (size_t)X.t_off[c->nb] * W) || (max_rounds > 0 && rnd_colour(c))) return 1;
    // hyperplanes and sign words
    if (round_vectors(c, T, K, 1, seed, false, hyperplanes, [&](int k, const double *G) {
            round_signs(c, src, k, K, W, G, X.sgn + (size_t)X.t_off[k] * W);
            return 0;
        }))
        return 1;
    auto field = [&](int k, const int *rows, int nrows) {
        const Block &B = c->blk[k];
        hipLaunchKernelGGL(X.lpk >= 0 ? k_rnd_field_cuts : k_rnd_field, dim3(field_strips(rows, nrows), W), dim3(TPB), 0, c->stream, nrows, rows, B.n, K,
                           (const int *)B.pu.adj_ptr, (const int *)B.pu.adj_col, (const int *)B.pu.adj_e, (const double *)B.pu.adj_sval,
                           (const double *)B.pu.cbase, (const double *)(B.dense_c ? B.Cfull : nullptr), B.npad,
                           (const double *)(X.t + X.t_off[k]), X.sgn + (size_t)X.t_off[k] * W, T.part.p, T.ctl);
    };
    int bt = 0;
    if (round_drive(c, K, max_rounds, T, field, RoundOut{obj, obj0, best, best0, rounds}, &bt)) return 1;
    if (sign) { // the best trial's signs, cone after cone
        const int w = bt / 64, l = bt % 64;
        std::vector<unsigned long long> words;
        for (int k = 0; k < c->nb; ++k) {
            const int n = c->blk[k].n;
            if (c->blk[k].is_lp) { // (the slacks of a cut-tightened context have no sign: zeros)
                for (int p = 0; p < n; ++p) sign[X.t_off[k] + p] = 0;
                continue;
            }
            words.resize((size_t)n);
            if (n) HC(hipMemcpyAsync(words.data(), X.sgn + (size_t)X.t_off[k] * W + (size_t)w * n, sizeof(unsigned long long) * n,
                                     hipMemcpyDeviceToHost, c->stream));
            HC(hipStreamSynchronize(c->stream));
            for (int p = 0; p < n; ++p) sign[X.t_off[k] + p] = ((words[p] >> l) & 1ull) ? 1 : -1;
        }
    }
    return 0;
}
