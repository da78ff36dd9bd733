// bisect.inc -- balanced partitions read off the factors of a bisection-structured context (Min-/Max-Bisection and prescribed part
// sizes: the +-1 diagonal structure plus one sum row <11^T, X> = d^2 per cone), included by lorads_hip.hip after stable.inc.
// DESIGN.md section 19.
//
// A context qualifies ("bisection-structured") when it has no LP block and every cone k has the diagonal rows of rounding.inc -- one
// a_i X_k[p,p] = b_i with b_i / a_i > 0 per diagonal position, all t_p = sqrt(b_i / a_i) bit-equal: t_k -- and exactly one sum row:
// every position of the cone's lower triangle, all values bit-equal to one a != 0, no entry on another cone, b / (a t_k^2) the
// square of an integer d_k with 0 <= d_k <= n_k and d_k = n_k (mod 2).  Then x = t_k sigma with sum(sigma) = +-d_k is feasible.  The
// sum row sits in the sparse structures (n < 32 or LORADS_NO_DENSE_A) or in the dense store (Block::Adense); bis_check reads both.
//
// Per cone and trial the +-1 rounding's hyperplane and sign bits (k_rnd_gauss with parts = 1, k_rnd_sign: a trial depends on
// (seed, cone, trial) alone), then one workgroup owns one (cone, trial): the repair to sum(sigma) = +-d_k, f, the swap search,
// f again.  No workgroup waits for another.  Everything is read-only on the solver's state, as in rounding.inc: F is formed on the
// fly, the scratch is the feature's own (BisectScratch), launches go straight to the stream, every sum has one fixed order.  The driver
// around the search kernel is rounding.inc's (round_begin, round_reserve, round_vectors, round_signs, trial_chunks, round_finish,
// round_stored_trial).
//
// C comes from cbase through the union pattern's adjacency (kcut.inc's kcut_walk), never from adj_sval: with the sum row in the
// sparse structures a constraint touches every slot, so no slot's adj_sval is C.  A dense-C cone reads its row of Cfull.

namespace {

constexpr size_t BIS_CHUNK_ELEMS = (size_t)1 << 24; // (trial, vertex) pairs whose fields one chunk of trials holds on the slab path
constexpr size_t BIS_LDS_BYTES = 48 * 1024;         // a trial's state (9 n bytes) lives in the LDS where it fits this beside the scratch
constexpr int BIS_RED = 16;                         // doubles of reduction scratch at the head of the LDS
constexpr int BIS_REBUILD = 64;                     // accepted swaps between two rebuilds of h from the row lists
constexpr signed char BIS_MARK = 2;                 // bit 1 of a state byte: the vertex is in the row list being looked at (bit 0: sigma = +1)

// candidate (va, ia) wins over (vb, ib): an index >= n is no candidate; otherwise the lower value, the lower index on ties and
// wherever the values do not compare (written so that exactly one of two candidates wins whatever the values are)
__device__ __forceinline__ bool bis_wins(double va, int ia, double vb, int ib, int n) {
    if (ia >= n) return false;
    if (ib >= n) return true;
    return va < vb || (!(vb < va) && ia < ib);
}
__device__ __forceinline__ void bis_take(double &v, int &i, double v2, int i2, int n) {
    if (bis_wins(v2, i2, v, i, n)) { v = v2; i = i2; }
}
// the winner over the workgroup's candidates, in every thread (red: 4 doubles and 4 ints of LDS); ends behind a barrier
__device__ __forceinline__ void bis_argmin(double &v, int &i, int n, double *redv, int *redi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_xor(v, o);
        const int i2 = __shfl_xor(i, o);
        bis_take(v, i, v2, i2, n);
    }
    if ((threadIdx.x & 63) == 0) { redv[threadIdx.x >> 6] = v; redi[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = redv[0]; i = redi[0];
#pragma unroll
    for (int w = 1; w < TPB / 64; ++w) bis_take(v, i, redv[w], redi[w], n);
    __syncthreads();
}

// what a trial's workgroup works on
struct BisCone {
    int n;
    const int *adj_ptr, *adj_col, *adj_e;
    const double *cbase, *Cfull; // C on the union pattern / the dense C (null on a sparse cone)
    int npad;
    double t;
};

// row p's stored list, its positions dealt over the workgroup's threads: f(q, C_pq), the diagonal included
template <typename F>
__device__ __forceinline__ void bis_row(const BisCone &c, int p, F f) {
    if (c.Cfull) {
        const double *crow = c.Cfull + (size_t)p * c.npad;
        for (int q = threadIdx.x; q < c.n; q += TPB) {
            const double cq = crow[q];
            if (cq != 0.0) f(q, cq);
        }
    } else {
        for (int s = c.adj_ptr[p] + threadIdx.x; s < c.adj_ptr[p + 1]; s += TPB) f(c.adj_col[s], c.cbase[c.adj_e[s]]);
    }
}

__device__ __forceinline__ double bis_x(const BisCone &c, const signed char *x, int p) { return (x[p] & 1) ? c.t : -c.t; }

// h_p = sum_{q != p} C_pq x_q over p's row list in its stored order (a thread's rows ascending) and f = sum_p x_p (h_p + C_pp x_p)
// in block_sum's tree; ends behind a barrier
__device__ double bis_rebuild(const BisCone &c, const signed char *x, double *h, double *red) {
    double acc = 0.0;
    for (int p = threadIdx.x; p < c.n; p += TPB) {
        double hp = 0.0, cpp = 0.0;
        kcut_walk(p, c.n, c.adj_ptr, c.adj_col, c.adj_e, c.cbase, c.Cfull, c.npad, [&](int q, double cq) {
            if (q == p) cpp = cq; else hp += cq * bis_x(c, x, q);
        });
        h[p] = hp;
        const double xp = bis_x(c, x, p);
        acc += xp * (hp + cpp * xp);
    }
    return block_sum(acc, red);
}

// sigma_p <- -sigma_p and h_q += 2 C_pq x_p (the new x_p) over p's row list; ends behind a barrier
__device__ void bis_flip(const BisCone &c, signed char *x, double *h, int p) {
    if (threadIdx.x == 0) x[p] ^= 1;
    __syncthreads();
    const double two_xp = 2.0 * bis_x(c, x, p);
    bis_row(c, p, [&](int q, double cq) {
        if (q != p) h[q] += cq * two_xp;
    });
    __syncthreads();
}

// tau_p = 4 t^2 sum_{q != p} |C_pq|
__device__ double bis_tau(const BisCone &c, int p, double *red) {
    double a = 0.0;
    bis_row(c, p, [&](int q, double cq) {
        if (q != p) a += fabs(cq);
    });
    return 4.0 * c.t * c.t * block_sum(a, red);
}

// One order of a swap round, from the side `plus` (1: sigma = +1): p = argmin over that side of Delta_p = -4 x_p h_p, q = argmin over
// the other side of Delta_q + 8 C_pq x_p x_q with C_pq from p's row list (0 where nothing is stored: the vertices of the list are
// marked while the others are looked at), delta = the sum of the two.  An empty side: p or q = n and delta = +inf.
__device__ void bis_order(const BisCone &c, signed char *x, const double *h, int plus, int &p, int &q, double &delta, double *redv,
                          int *redi) {
    const int n = c.n;
    double v = INFINITY;
    int i = n;
    for (int u = threadIdx.x; u < n; u += TPB)
        if ((x[u] & 1) == plus) bis_take(v, i, -4.0 * bis_x(c, x, u) * h[u], u, n);
    bis_argmin(v, i, n, redv, redi);
    p = i; q = n; delta = INFINITY;
    if (p >= n) return; // (uniform: every thread holds the same p)
    const double dp = v, xp = bis_x(c, x, p);
    v = INFINITY; i = n;
    bis_row(c, p, [&](int u, double cq) {
        if (u == p) return;
        if ((x[u] & 1) != plus) {
            const double xu = bis_x(c, x, u);
            bis_take(v, i, -4.0 * xu * h[u] + 8.0 * cq * xp * xu, u, n);
        }
        x[u] |= BIS_MARK;
    });
    __syncthreads();
    for (int u = threadIdx.x; u < n; u += TPB)
        if ((x[u] & 1) != plus && !(x[u] & BIS_MARK)) bis_take(v, i, -4.0 * bis_x(c, x, u) * h[u], u, n);
    bis_argmin(v, i, n, redv, redi);
    bis_row(c, p, [&](int u, double) { x[u] &= ~BIS_MARK; });
    __syncthreads();
    q = i;
    if (q < n) delta = dp + v;
}

// One trial per workgroup (trial t0 + blockIdx.x of cone `kc`).  The hyperplane's signs, D = their sum; the repair: |D - target| / 2
// flips (target = +d where D >= 0, else -d) of the vertex of least Delta_p = -4 x_p h_p on the side in excess, the lowest index on
// ties; h rebuilt, f0; at most max_rounds rounds of the swap search -- orders A (from +1) and B (from -1), A unless Delta_B < Delta_A,
// the pair swapped where Delta < -2^-40 (tau_p + tau_q); the round that does not swap is the last and is counted --; h rebuilt, f.
// The state -- h (8 n bytes) and the sign bytes -- sits in the LDS (lds != 0) or h on the slab hs and the bytes in the trial's
// place of xs, where they end up in either case.  first: this cone is the context's first (f = instead of f +=).
__global__ __launch_bounds__(TPB) void k_bis_search(BisCone c, int d, int K, int t0, int kc, int first, int max_rounds, int lds,
                                                    const unsigned long long *__restrict__ sgn, signed char *xs, double *hs, double *f,
                                                    double *f0, int *imb, int *nround) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *red = (double *)smem, *redv = red + 4;
    int *redi = (int *)(red + 8);
    const int n = c.n, tid = threadIdx.x, t = t0 + blockIdx.x;
    signed char *xg = xs + (size_t)t * n;
    double *h = lds ? red + BIS_RED : hs + (size_t)blockIdx.x * n;
    signed char *x = lds ? (signed char *)(red + BIS_RED + n) : xg;
    const unsigned long long *sw = sgn + (size_t)(t >> 6) * n;
    double cnt = 0.0;
    for (int p = tid; p < n; p += TPB) {
        const signed char s = (signed char)((sw[p] >> (t & 63)) & 1ull);
        x[p] = s;
        cnt += s ? 1.0 : -1.0;
    }
    __syncthreads();
    const int D = (int)block_sum(cnt, red);
    const int target = D >= 0 ? d : -d;
    const int steps = (D > target ? D - target : target - D) / 2, side = D > target ? 1 : 0;
    if (steps > 0) bis_rebuild(c, x, h, red);
    for (int s = 0; s < steps; ++s) {
        double v = INFINITY;
        int i = n;
        for (int p = tid; p < n; p += TPB)
            if ((x[p] & 1) == side) bis_take(v, i, -4.0 * bis_x(c, x, p) * h[p], p, n);
        bis_argmin(v, i, n, redv, redi);
        if (i < n) bis_flip(c, x, h, i);
    }
    double val = bis_rebuild(c, x, h, red);
    if (tid == 0) f0[t] = first ? val : f0[t] + val;
    int rounds = 0, since = 0;
    while (rounds < max_rounds) {
        ++rounds;
        int pa, qa, pb, qb;
        double da, db;
        bis_order(c, x, h, 1, pa, qa, da, redv, redi);
        bis_order(c, x, h, 0, pb, qb, db, redv, redi);
        const bool useb = db < da;
        const int p = useb ? pb : pa, q = useb ? qb : qa;
        const double delta = useb ? db : da;
        if (p >= n || q >= n) break;
        const double tau = bis_tau(c, p, red) + bis_tau(c, q, red);
        if (!(delta < -0x1p-40 * tau)) break;
        bis_flip(c, x, h, p);
        bis_flip(c, x, h, q);
        if (++since == BIS_REBUILD) { bis_rebuild(c, x, h, red); since = 0; }
    }
    if (rounds > 0) val = bis_rebuild(c, x, h, red);
    if (lds)
        for (int p = tid; p < n; p += TPB) xg[p] = x[p];
    if (tid == 0) {
        f[t] = first ? val : f[t] + val;
        imb[(size_t)kc * K + t] = D;
        nround[t] = first || rounds > nround[t] ? rounds : nround[t];
    }
}

// Applicability (once per context: the constraint data never changes): t_k and d_k of every cone.  The cone's image is read back
// from the sparse structures (read_constraint_image) and, for the constraints kept there, from the dense store.
int bis_check(lorads_hip_ctx *c) {
    BisectScratch &X = c->bisect;
    if (X.checked) return 0;
    X.qualifies = false;
    X.why.clear();
    X.v_off.assign((size_t)c->nb + 1, 0);
    X.t.assign((size_t)c->nb, 0.0);
    X.d.assign((size_t)c->nb, 0);
    for (int k = 0; k < c->nb; ++k) X.v_off[k + 1] = X.v_off[k] + c->blk[k].n;
    std::vector<double> b((size_t)c->m);
    if (c->m) HC(hipMemcpyAsync(b.data(), c->b, sizeof(double) * b.size(), hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    std::vector<int> owner((size_t)c->m, -1);
    char msg[256];
    for (int k = 0; k < c->nb && X.why.empty(); ++k)
        if (c->blk[k].is_lp) { snprintf(msg, sizeof msg, "block %d is an LP block", k + 1); X.why = msg; }
    if (c->nb == 0 && X.why.empty()) X.why = "no cone";
    for (int k = 0; k < c->nb && X.why.empty(); ++k) {
        const Block &B = c->blk[k];
        const int n = B.n;
        const long long tri = (long long)n * (n + 1) / 2;
        ConImage m;
        if (read_constraint_image(c, k, m)) return 1;
        std::vector<int> dense_at((size_t)B.nrow, -1), cover((size_t)n, 0);
        if (B.dense_a)
            for (int j = 0; j < B.nd; ++j) dense_at[(size_t)B.d_con_h[(size_t)j]] = j;
        std::vector<double> th((size_t)n, 0.0), ad;
        std::vector<char> seen;
        int sum_row = -1;
        double sum_a = 0.0;
        for (int i = 0; i < B.nrow && X.why.empty(); ++i) {
            const int gi = m.ri[i], cnt = m.ap[i + 1] - m.ap[i];
            if (owner[gi] >= 0 && owner[gi] != k) { snprintf(msg, sizeof msg, "constraint %d touches more than one cone", gi + 1); X.why = msg; break; }
            owner[gi] = k;
            bool is_sum = false;
            double a = 0.0;
            if (dense_at[i] >= 0) { // the dense store: the full symmetric matrix, its lower triangle looked at
                const size_t msz = (size_t)B.npad * B.npad;
                ad.resize(msz);
                HC(hipMemcpyAsync(ad.data(), B.Adense + (size_t)dense_at[i] * msz, sizeof(double) * msz, hipMemcpyDeviceToHost, c->stream));
                HC(hipStreamSynchronize(c->stream));
                a = ad[0];
                is_sum = a != 0.0 && cnt == 0;
                for (int p = 0; p < n && is_sum; ++p)
                    for (int q = 0; q <= p && is_sum; ++q) is_sum = memcmp(&ad[(size_t)p * B.npad + q], &a, sizeof(double)) == 0;
            } else if (cnt == 1 && !(n == 1 && cover[0] == 1)) { // (a cone of one row: its first one-entry row is the diagonal row)
                const int e = m.ae[m.ap[i]], p = m.er[e];
                X.why = diag_row(gi, m.er[e], m.ec[e], m.av[m.ap[i]], b[gi], &th[p]);
                if (!X.why.empty()) break;
                cover[p]++;
                continue;
            } else if ((long long)cnt == tri && cnt > 0) { // the sparse structures: tri distinct positions of the lower triangle are all of it
                a = m.av[m.ap[i]];
                is_sum = a != 0.0;
                seen.assign((size_t)B.pa.ne, 0);
                for (int s = m.ap[i]; s < m.ap[i + 1] && is_sum; ++s) {
                    is_sum = !seen[(size_t)m.ae[s]] && memcmp(&m.av[s], &a, sizeof(double)) == 0;
                    seen[(size_t)m.ae[s]] = 1;
                }
            }
            if (!is_sum) {
                snprintf(msg, sizeof msg, "constraint %d is neither a diagonal row nor a sum row of cone %d", gi + 1, k + 1);
                X.why = msg;
                break;
            }
            if (sum_row >= 0) {
                snprintf(msg, sizeof msg, "cone %d has two sum rows (constraints %d and %d)", k + 1, sum_row + 1, gi + 1);
                X.why = msg;
                break;
            }
            sum_row = gi;
            sum_a = a;
        }
        for (int p = 0; p < n && X.why.empty(); ++p) {
            if (cover[p] != 1) {
                snprintf(msg, sizeof msg, "diagonal %d of cone %d is fixed by %d constraints", p + 1, k + 1, cover[p]);
                X.why = msg;
            } else if (memcmp(&th[p], &th[0], sizeof(double)) != 0) {
                snprintf(msg, sizeof msg, "cone %d has unequal diagonal values: t_%d = %.17g, t_1 = %.17g", k + 1, p + 1, th[p], th[0]);
                X.why = msg;
            }
        }
        if (!X.why.empty()) break;
        if (n == 0) { snprintf(msg, sizeof msg, "cone %d has no row", k + 1); X.why = msg; break; }
        if (sum_row < 0) { snprintf(msg, sizeof msg, "cone %d has no sum row", k + 1); X.why = msg; break; }
        const double q = b[sum_row] / (sum_a * th[0] * th[0]);
        const double dr = q >= 0 ? std::floor(std::sqrt(q) + 0.5) : -1.0;
        if (!std::isfinite(q) || !(dr >= 0) || !(std::fabs(q - dr * dr) <= 1e-9 * std::max(1.0, q)) || dr > n || (((int)dr ^ n) & 1)) {
            snprintf(msg, sizeof msg,
                     "the sum row of cone %d (constraint %d) has b / (a t^2) = %.17g: not d^2 for an integer 0 <= d <= n = %d with d = n (mod 2)",
                     k + 1, sum_row + 1, q, n);
            X.why = msg;
            break;
        }
        X.t[k] = th[0];
        X.d[k] = (int)dr;
    }
    for (int i = 0; i < c->m && X.why.empty(); ++i)
        if (owner[i] < 0) { snprintf(msg, sizeof msg, "constraint %d has no stored entry", i + 1); X.why = msg; }
    X.qualifies = X.why.empty();
    X.checked = true;
    return 0;
}

// does a trial's state of a cone of n rows live in the LDS (LORADS_BISECT_LDS=0 at creation: never, the slab path at every size)
inline bool bis_in_lds(const lorads_hip_ctx *c, int n) { return c->opt.bisect_lds && (size_t)BIS_RED * 8 + 9 * (size_t)n <= BIS_LDS_BYTES; }

const RoundFeature FT_BISECT{"round_bisect", "bisection-structured", bis_check, false};

} // namespace

// the signs of trial `trial` of the context's last lorads_hip_round_bisect call, cone after cone
extern "C" int lorads_hip_bisect_trial(lorads_hip_ctx *c, int32_t trial, int8_t *sign) {
    if (!c || !sign) return fail_msg("bisect_trial: bad argument");
    const BisectScratch &X = c->bisect;
    return round_stored_trial(c, "bisect_trial", X.trial, X.v_off, (const int8_t *)X.x.p, trial, sign,
                              [](int8_t s) { return (int8_t)((s & 1) ? 1 : -1); });
}

extern "C" int lorads_hip_round_bisect(lorads_hip_ctx *c, int32_t src, int32_t trials, uint64_t seed, int32_t max_rounds, double *obj,
                                       double *obj0, int32_t *best, int32_t *best0, int8_t *sign, int32_t *imbalance, int32_t *rounds,
                                       double *hyperplanes, double *t, int32_t *diff) {
    if (const int rc = round_begin(c, FT_BISECT, c ? &c->bisect : nullptr, src, nullptr, trials, max_rounds, obj)) return rc;
    BisectScratch &X = c->bisect;
    for (int k = 0; k < c->nb; ++k) {
        if (t) t[k] = X.t[k];
        if (diff) diff[k] = X.d[k];
    }
    if (trials == 0) return 0;
    const int K = trials, W = (K + 63) / 64, ntot = X.v_off[c->nb];
    int nmax = 1;
    bool slab = false;
    for (auto &B : c->blk) { nmax = std::max(nmax, B.n); slab = slab || !bis_in_lds(c, B.n); }
    const int CH = trial_chunk(c, K, nmax, BIS_CHUNK_ELEMS, 1);
    TrialScratch &R = X.trial;
    if (X.sgn.grow(X.mem, (size_t)ntot * W) || X.x.grow(X.mem, (size_t)ntot * K) || X.imb.grow(X.mem, (size_t)c->nb * K) ||
        (slab && X.h.grow(X.mem, (size_t)CH * nmax)) || round_reserve(c, R, X.mem, K, 1, false))
        return 1;
    if (round_vectors(c, R, K, 1, seed, false, hyperplanes, [&](int k, const double *G) {
            const Block &B = c->blk[k];
            round_signs(c, src, k, K, W, G, X.sgn + (size_t)X.v_off[k] * W);
            const bool lds = bis_in_lds(c, B.n);
            const size_t shm = (size_t)BIS_RED * 8 + (lds ? (((size_t)9 * B.n + 15) & ~(size_t)15) : 0);
            const BisCone bc{B.n, B.pu.adj_ptr, B.pu.adj_col, B.pu.adj_e, B.pu.cbase, B.dense_c ? B.Cfull : nullptr, B.npad, X.t[k]};
            trial_chunks(K, CH, [&](int t0, int t1) {
                hipLaunchKernelGGL(k_bis_search, dim3(t1 - t0), dim3(TPB), shm, c->stream, bc, X.d[k], K, t0, k, (int)(k == 0), (int)max_rounds,
                                   (int)lds, (const unsigned long long *)(X.sgn + (size_t)X.v_off[k] * W), X.x + (size_t)X.v_off[k] * K, X.h.p,
                                   R.f.p, R.f0.p, X.imb.p, R.nround.p);
                return 0;
            });
            HC(hipGetLastError());
            return 0;
        }))
        return 1;
    if (imbalance) HC(hipMemcpyAsync(imbalance, X.imb.p, sizeof(int) * (size_t)c->nb * K, hipMemcpyDeviceToHost, c->stream));
    int bt = 0;
    if (round_finish(c, K, R, R.f.p, -1, RoundOut{obj, obj0, best, best0, rounds}, &bt)) return 1;
    if (sign) return lorads_hip_bisect_trial(c, bt, sign);
    return 0;
}
