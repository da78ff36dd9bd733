// stable.inc -- stable sets read off the factors of a theta-structured context (Lovasz theta, Schrijver's theta' and what
// lrd_session_write_bounded makes of them), included by lorads_hip.hip after kcut.inc.  DESIGN.md section 18.
//
// A context qualifies ("theta-structured") when it has at most one LP block whose columns sit only in bound rows 2 a X_pq + c x_j = b
// (kcut.inc's bound_row), every SDP cone has exactly one trace row -- a I over all its n rows, a > 0, b > 0, touching no other cone:
// T = b / a -- and every other constraint that touches the cone is an edge row: one off-diagonal entry (p, q), b = 0.  The edge rows
// are the cone's graph.  For a stable set S of it X(S) = T 1_S 1_S^T / |S| is feasible and f = <C, X(S)>.
//
// Per cone and trial a priority per vertex: trial 0 takes |F_p|^2 = X_pp, trial t >= 1 takes F_p . g_t, g_t the +-1 rounding's
// hyperplane t (k_rnd_gauss, parts = 1) -- all projections of a cone one tall-skinny product on the FP64 matrix cores.  One workgroup
// owns one trial: the greedy set (the lexicographically first maximal stable set in the order priority descending, index ascending,
// as a parallel fixed point), f, the (1, 2)-swap search with the greedy completion behind every swap, f again.  No workgroup waits
// for another.  Everything is read-only on the solver's state, as in rounding.inc: F is formed on the fly, the scratch is the
// feature's own (StableScratch), launches go straight to the stream, every sum has one fixed order.  The driver around the kernels is
// rounding.inc's (round_begin, round_reserve, round_vectors, trial_chunks, round_finish, round_stored_trial).

namespace {

constexpr unsigned char STB_UND = 0, STB_IN = 1, STB_OUT = 2;
constexpr size_t STB_CHUNK_ELEMS = (size_t)1 << 24; // (trial, vertex) pairs whose scores and lists one chunk of trials holds

// trial 0's priorities: |F_p|^2 over the cone's own rl columns, ascending
__global__ __launch_bounds__(TPB) void k_stb_norm(int n, int rl, int r, const double *__restrict__ U, const double *__restrict__ V, int uv,
                                                  double *__restrict__ sc) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= n) return;
    double s = 0.0;
    for (int j = 0; j < rl; ++j) {
        const double f = factor_ld(U, V, uv != 0, (size_t)p * r + j);
        s += f * f;
    }
    sc[p] = s;
}

// Priorities of 16 rows x 16 trials per wavefront: mfma_fm_tile with B[kk][nn] = g[column kk][trial t0 + 16 tile + nn] (a 128-byte
// segment of G's row).  Result register q of lane (nn, kk) is row p0 + kk + 4 q, trial t0 + 16 tile + nn, stored at sc[trial - t0][row].
// Rows past n and trials past t1 are clamped loads whose results are not stored; trial 0 is k_stb_norm's.
__global__ __launch_bounds__(TPB) void k_stb_proj(int n, int rl, int r, int K, int t0, int t1, const double *__restrict__ U,
                                                  const double *__restrict__ V, int uv, const double *__restrict__ G,
                                                  double *__restrict__ sc) {
    const int l = threadIdx.x & 63, nn = l & 15, kk = l >> 4;
    const int nrt = (n + 15) / 16, ntt = (t1 - t0 + 15) / 16;
    const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TPB / 64) + (threadIdx.x >> 6)));
    if (gw >= nrt * ntt) return;
    const int p0 = (gw % nrt) * 16, t = t0 + (gw / nrt) * 16 + nn, tc = t < K ? t : K - 1;
    const size_t ao = (size_t)(p0 + nn < n ? p0 + nn : n - 1) * r;
    const double *Gt = G + tc;
    const v4f64 acc = mfma_fm_tile(U, V, uv != 0, ao, rl, kk, [&](int kc) { return Gt[(size_t)kc * K]; });
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = p0 + kk + 4 * q;
        if (p < n && t < t1 && t > 0) sc[(size_t)(t - t0) * n + p] = acc[q];
    }
}

// q comes before p in a trial's order: priority descending, index ascending (written so that exactly one of two vertices comes before
// the other whatever the values are)
__device__ __forceinline__ bool stb_before(double pq, int q, double pp, int p) { return pq > pp || (!(pq < pp) && q < p); }

// The greedy completion as a parallel fixed point on the undecided vertices of s: a vertex joins when every neighbour that comes
// before it is out, then an undecided vertex with a neighbour that is in leaves.  Every decision is the sequential greedy's, and a
// round decides at least the first undecided vertex: at most n + 1 rounds.  What a malformed order (priorities that are not numbers)
// leaves undecided is out.  Ends behind a barrier.
__device__ void stb_greedy(int n, const int *__restrict__ gp, const int *__restrict__ gc, const double *__restrict__ pi, unsigned char *s) {
    const int tid = threadIdx.x;
    for (int round = 0; round <= n; ++round) {
        for (int p = tid; p < n; p += TPB) {
            if (s[p] != STB_UND) continue;
            const double pp = pi[p];
            bool free = true;
            for (int e = gp[p]; e < gp[p + 1] && free; ++e) {
                const int q = gc[e];
                if (s[q] != STB_OUT && stb_before(pi[q], q, pp, p)) free = false;
            }
            if (free) s[p] = STB_IN;
        }
        __syncthreads();
        int und = 0;
        for (int p = tid; p < n; p += TPB) {
            if (s[p] != STB_UND) continue;
            bool hit = false;
            for (int e = gp[p]; e < gp[p + 1] && !hit; ++e) hit = s[gc[e]] == STB_IN;
            if (hit) s[p] = STB_OUT; else und = 1;
        }
        if (!__syncthreads_or(und)) return;
    }
    for (int p = tid; p < n; p += TPB)
        if (s[p] == STB_UND) s[p] = STB_OUT;
    __syncthreads();
}

// sum over the workgroup's threads in a fixed tree; every thread gets it
__device__ __forceinline__ double stb_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = TPB / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}

// |S| and f = (T / |S|) sum_{p in S} sum_{q in S} C_pq: a member's row sum over its stored row list in its stored order (kcut_walk),
// a thread's rows ascending, the threads in stb_sum's tree.  *size <- |S|.
__device__ double stb_value(int n, const unsigned char *s, const int *__restrict__ adj_ptr, const int *__restrict__ adj_col,
                            const int *__restrict__ adj_e, const double *__restrict__ cbase, const double *__restrict__ Cfull, int npad,
                            double T, double *red, int *size) {
    double acc = 0.0, cnt = 0.0;
    for (int p = threadIdx.x; p < n; p += TPB) {
        if (s[p] != STB_IN) continue;
        double row = 0.0;
        kcut_walk(p, n, adj_ptr, adj_col, adj_e, cbase, Cfull, npad, [&](int q, double cq) {
            if (s[q] == STB_IN) row += cq;
        });
        acc += row;
        cnt += 1.0;
    }
    const double tot = stb_sum(acc, red), sz = stb_sum(cnt, red);
    *size = (int)sz;
    return sz > 0.0 ? (T / sz) * tot : 0.0;
}

// is w a neighbour of u (the lists are ascending)
__device__ __forceinline__ bool stb_adjacent(const int *__restrict__ gp, const int *__restrict__ gc, int u, int w) {
    int lo = gp[u], hi = gp[u + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1, x = gc[mid];
        if (x == w) return true;
        if (x < w) lo = mid + 1; else hi = mid;
    }
    return false;
}

// One trial per workgroup (trial t0 + blockIdx.x of cone `kc`): the greedy set, f0, at most max_rounds rounds of the (1, 2)-swap
// search, f, |S| and the rounds run.  A round: own[u] = the one member next to u (tau(u) = 1; -1 otherwise); a member v is improvable
// when two of its neighbours u < w with own = v are not adjacent, its pair the lexicographically first such; the improvable v of least
// index leaves, its pair joins, and the vertices left without a member next to them are completed greedily.  The round that finds
// no improvable v is the last and is counted.  first: this cone is the context's first (f = instead of f +=).
__global__ __launch_bounds__(TPB) void k_stb_search(int n, int K, int t0, int kc, int first, int max_rounds, const int *__restrict__ gp,
                                                    const int *__restrict__ gc, const double *__restrict__ sc, unsigned char *st, int *own,
                                                    const int *__restrict__ adj_ptr, const int *__restrict__ adj_col,
                                                    const int *__restrict__ adj_e, const double *__restrict__ cbase,
                                                    const double *__restrict__ Cfull, int npad, double T, double *f, double *f0,
                                                    int *__restrict__ size, int *nround) {
    __shared__ double red[TPB];
    __shared__ int pick[3];
    const int tid = threadIdx.x, t = t0 + blockIdx.x;
    const double *pi = sc + (size_t)blockIdx.x * n;
    unsigned char *s = st + (size_t)t * n;
    int *ow = own + (size_t)blockIdx.x * n;
    for (int p = tid; p < n; p += TPB) s[p] = STB_UND;
    __syncthreads();
    stb_greedy(n, gp, gc, pi, s);
    int sz = 0;
    double v = stb_value(n, s, adj_ptr, adj_col, adj_e, cbase, Cfull, npad, T, red, &sz);
    if (tid == 0) f0[t] = first ? v : f0[t] + v;
    int rounds = 0;
    while (rounds < max_rounds) {
        ++rounds;
        if (tid == 0) pick[0] = n;
        for (int p = tid; p < n; p += TPB) {
            int cnt = 0, m = -1;
            if (s[p] != STB_IN)
                for (int e = gp[p]; e < gp[p + 1]; ++e) {
                    const int q = gc[e];
                    if (s[q] == STB_IN) { ++cnt; m = q; }
                }
            ow[p] = cnt == 1 ? m : -1;
        }
        __syncthreads();
        int mv = n, mu = 0, mw = 0;
        for (int x = tid; x < n && mv == n; x += TPB) {
            if (s[x] != STB_IN) continue;
            const int e1end = gp[x + 1];
            for (int e1 = gp[x]; e1 < e1end && mv == n; ++e1) {
                const int u = gc[e1];
                if (ow[u] != x) continue;
                for (int e2 = e1 + 1; e2 < e1end; ++e2) {
                    const int w = gc[e2];
                    if (ow[w] != x || stb_adjacent(gp, gc, u, w)) continue;
                    mv = x; mu = u; mw = w;
                    break;
                }
            }
        }
        if (mv < n) atomicMin(&pick[0], mv);
        __syncthreads();
        const int bv = pick[0];
        if (bv == n) break; // (uniform: every thread reads the same value behind the barrier)
        if (mv == bv) { pick[1] = mu; pick[2] = mw; }
        __syncthreads();
        if (tid == 0) { s[bv] = STB_OUT; s[pick[1]] = STB_IN; s[pick[2]] = STB_IN; }
        __syncthreads();
        for (int p = tid; p < n; p += TPB) {
            if (s[p] == STB_IN) continue;
            bool hit = false;
            for (int e = gp[p]; e < gp[p + 1] && !hit; ++e) hit = s[gc[e]] == STB_IN;
            s[p] = hit ? STB_OUT : STB_UND;
        }
        __syncthreads();
        stb_greedy(n, gp, gc, pi, s);
    }
    if (rounds > 0) v = stb_value(n, s, adj_ptr, adj_col, adj_e, cbase, Cfull, npad, T, red, &sz);
    if (tid == 0) {
        f[t] = first ? v : f[t] + v;
        size[(size_t)kc * K + t] = sz;
        nround[t] = first || rounds > nround[t] ? rounds : nround[t];
    }
}

// Applicability (once per context: the constraint data never changes): the trace row and the graph of every cone, the bounds u_j of
// the LP columns.  The graphs go to the device as CSR lists, both directions, ascending, an edge once however many rows name it.
int stb_check(lorads_hip_ctx *c) {
    StableScratch &X = c->stable;
    if (X.checked) return 0;
    X.qualifies = false;
    X.why.clear();
    X.lp_u.clear();
    X.T.assign((size_t)c->nb, 0.0);
    X.v_off.assign((size_t)c->nb + 1, 0);
    X.e_off.assign((size_t)c->nb + 1, 0);
    for (int k = 0; k < c->nb; ++k) X.v_off[k + 1] = X.v_off[k] + (c->blk[k].is_lp ? 0 : c->blk[k].n);
    int lpk = -1;
    X.why = blocks_admit_bound_rows(c, &lpk);
    if (!X.why.empty()) { X.checked = true; return 0; }
    ConData D;
    if (read_constraints(c, D)) return 1;
    char msg[256];
    const int nl = lpk >= 0 ? c->blk[lpk].n : 0;
    std::vector<int> col_use((size_t)nl, 0), trace_row((size_t)c->nb, -1);
    std::vector<BoundRow> brow;
    std::vector<std::vector<std::pair<int, int>>> edges((size_t)c->nb);
    for (int i = 0; i < c->m && X.why.empty(); ++i) {
        const std::vector<ConEnt> &E = D.con[(size_t)i];
        if (lpk >= 0 && lp_entries(E, lpk) > 0) {
            BoundRow r;
            X.why = bound_row(i, E, lpk, r);
            if (!X.why.empty()) break;
            col_use[(size_t)r.j]++;
            brow.push_back(r);
            continue;
        }
        if (E.empty()) { snprintf(msg, sizeof msg, "constraint %d has no stored entry", i + 1); X.why = msg; break; }
        const int k = E[0].k, n = c->blk[k].n;
        bool one_cone = true, all_diag = true, same_a = true;
        for (const ConEnt &e : E) {
            one_cone = one_cone && e.k == k;
            all_diag = all_diag && e.p == e.q;
            same_a = same_a && e.a == E[0].a;
        }
        if (!one_cone) { snprintf(msg, sizeof msg, "constraint %d touches more than one cone", i + 1); X.why = msg; break; }
        if (E.size() == 1 && !all_diag) { // an edge row
            if (D.b[(size_t)i] != 0.0) {
                snprintf(msg, sizeof msg, "constraint %d is an edge row with b = %g (not 0)", i + 1, D.b[(size_t)i]);
                X.why = msg;
                break;
            }
            edges[k].push_back({E[0].p, E[0].q});
            edges[k].push_back({E[0].q, E[0].p});
            continue;
        }
        if (!all_diag || !same_a || (int)E.size() != n) { // (the entries of a constraint are distinct positions: n diagonals are all of them)
            snprintf(msg, sizeof msg, "constraint %d is neither a trace row nor an edge row of cone %d", i + 1, k + 1);
            X.why = msg;
            break;
        }
        if (!(E[0].a > 0) || !(D.b[(size_t)i] > 0) || !std::isfinite(D.b[(size_t)i] / E[0].a)) {
            snprintf(msg, sizeof msg, "constraint %d is a trace row with a = %g, b = %g (not both positive)", i + 1, E[0].a, D.b[(size_t)i]);
            X.why = msg;
            break;
        }
        if (trace_row[k] >= 0) {
            snprintf(msg, sizeof msg, "cone %d has two trace rows (constraints %d and %d)", k + 1, trace_row[k] + 1, i + 1);
            X.why = msg;
            break;
        }
        trace_row[k] = i;
        X.T[k] = D.b[(size_t)i] / E[0].a;
    }
    for (int k = 0; k < c->nb && X.why.empty(); ++k)
        if (k != lpk && trace_row[k] < 0) { snprintf(msg, sizeof msg, "cone %d has no trace row", k + 1); X.why = msg; }
    if (X.why.empty()) X.why = lp_columns_only_bound(col_use, D.cobj);
    X.qualifies = X.why.empty();
    if (X.qualifies) {
        X.lp_u.assign((size_t)nl, 0.0);
        for (const BoundRow &r : brow) // x_j = (b - 2 a X_pq) / c and |X_pq| <= (X_pp + X_qq) / 2 <= T / 2
            X.lp_u[(size_t)r.j] = (std::fabs(2.0 * r.a) * X.T[r.k] / 2.0 + std::fabs(D.b[(size_t)r.i])) / std::fabs(r.cc);
        std::vector<int> ptr, col;
        for (int k = 0; k < c->nb; ++k) {
            X.e_off[k] = (long long)col.size();
            if (c->blk[k].is_lp) continue;
            std::vector<std::pair<int, int>> &e = edges[k];
            std::sort(e.begin(), e.end());
            e.erase(std::unique(e.begin(), e.end()), e.end());
            size_t at = 0;
            for (int p = 0; p < c->blk[k].n; ++p) {
                ptr.push_back((int)(col.size() - (size_t)X.e_off[k]));
                for (; at < e.size() && e[at].first == p; ++at) col.push_back(e[at].second);
            }
            ptr.push_back((int)(col.size() - (size_t)X.e_off[k]));
        }
        X.e_off[c->nb] = (long long)col.size();
        if (col.empty()) col.push_back(0);
        if (X.mem.upload(&X.g_ptr, ptr) || X.mem.upload(&X.g_col, col)) return 1;
    }
    X.checked = true;
    return 0;
}

// SDP cones before block k (the cone's index in the per-cone outputs)
inline int stb_cone_index(const lorads_hip_ctx *c, int k) {
    int kc = 0;
    for (int j = 0; j < k; ++j) kc += !c->blk[j].is_lp;
    return kc;
}

const RoundFeature FT_STABLE{"round_stable", "theta-structured", stb_check, false};

} // namespace

// the members of trial `trial` of the context's last lorads_hip_round_stable call (1: in the set), SDP cone after SDP cone
extern "C" int lorads_hip_stable_trial(lorads_hip_ctx *c, int32_t trial, uint8_t *member) {
    if (!c || !member) return fail_msg("stable_trial: bad argument");
    const StableScratch &X = c->stable;
    return round_stored_trial(c, "stable_trial", X.trial, X.v_off, (const uint8_t *)X.st.p, trial, member,
                              [](uint8_t s) { return (uint8_t)(s == STB_IN); });
}

extern "C" int lorads_hip_round_stable(lorads_hip_ctx *c, int32_t src, int32_t trials, uint64_t seed, int32_t max_rounds, double *obj,
                                       double *obj0, int32_t *best, int32_t *best0, uint8_t *member, int32_t *sizes, int32_t *rounds,
                                       double *scores, double *T) {
    if (const int rc = round_begin(c, FT_STABLE, c ? &c->stable : nullptr, src, nullptr, trials, max_rounds, obj)) return rc;
    StableScratch &X = c->stable;
    int ncone = 0;
    for (int k = 0; k < c->nb; ++k) ncone += !c->blk[k].is_lp;
    if (T) { // T_k of the SDP cones, then u_j of the LP columns
        int at = 0;
        for (int k = 0; k < c->nb; ++k)
            if (!c->blk[k].is_lp) T[at++] = X.T[k];
        for (size_t j = 0; j < X.lp_u.size(); ++j) T[at++] = X.lp_u[j];
    }
    if (trials == 0) return 0;
    const int K = trials, ntot = X.v_off[c->nb];
    int nmax = 1;
    for (auto &B : c->blk)
        if (!B.is_lp) nmax = std::max(nmax, B.n);
    const int CH = trial_chunk(c, K, nmax, STB_CHUNK_ELEMS, 16);
    TrialScratch &R = X.trial;
    if (X.sc.grow(X.mem, (size_t)CH * nmax) || X.own.grow(X.mem, (size_t)CH * nmax) || X.st.grow(X.mem, (size_t)ntot * K) ||
        X.size.grow(X.mem, (size_t)ncone * K) || round_reserve(c, R, X.mem, K, 1, false))
        return 1;
    bool first = true;
    if (round_vectors(c, R, K, 1, seed, true, nullptr, [&](int k, const double *G) {
            const Block &B = c->blk[k];
            const int kc = stb_cone_index(c, k);
            const FactorView F = factor_view(c, src, k);
            const int *gp = X.g_ptr + X.v_off[k] + kc, *gc = X.g_col + X.e_off[k];
            if (trial_chunks(K, CH, [&](int t0, int t1) {
                    const size_t waves = (size_t)nblocks_for((size_t)B.n, 16) * nblocks_for((size_t)(t1 - t0), 16);
                    hipLaunchKernelGGL(k_stb_proj, dim3(nblocks_for(waves, TPB / 64)), dim3(TPB), 0, c->stream, B.n, B.rl, B.r, K, t0, t1, F.U,
                                       F.V, F.uv, G, X.sc.p);
                    if (t0 == 0)
                        hipLaunchKernelGGL(k_stb_norm, dim3(nblocks_for((size_t)B.n, TPB)), dim3(TPB), 0, c->stream, B.n, B.rl, B.r, F.U, F.V,
                                           F.uv, X.sc.p);
                    hipLaunchKernelGGL(k_stb_search, dim3(t1 - t0), dim3(TPB), 0, c->stream, B.n, K, t0, kc, (int)first, (int)max_rounds, gp, gc,
                                       (const double *)X.sc.p, X.st + (size_t)X.v_off[k] * K, X.own.p, (const int *)B.pu.adj_ptr,
                                       (const int *)B.pu.adj_col, (const int *)B.pu.adj_e, (const double *)B.pu.cbase,
                                       (const double *)(B.dense_c ? B.Cfull : nullptr), B.npad, X.T[k], R.f.p, R.f0.p, X.size.p, R.nround.p);
                    HC(hipGetLastError());
                    if (scores) { // (the copy is in stream order: the next chunk's kernels write behind it)
                        HC(hipMemcpyAsync(scores + (size_t)X.v_off[k] * K + (size_t)t0 * B.n, X.sc.p, sizeof(double) * (size_t)(t1 - t0) * B.n,
                                          hipMemcpyDeviceToHost, c->stream));
                        HC(hipStreamSynchronize(c->stream));
                    }
                    return 0;
                }))
                return 1;
            first = false;
            return 0;
        }))
        return 1;
    if (first) return fail_msg("round_stable: no cone has a vertex");
    if (sizes) HC(hipMemcpyAsync(sizes, X.size.p, sizeof(int) * (size_t)ncone * K, hipMemcpyDeviceToHost, c->stream));
    int bt = 0;
    if (round_finish(c, K, R, R.f.p, -1, RoundOut{obj, obj0, best, best0, rounds}, &bt)) return 1;
    if (member) return lorads_hip_stable_trial(c, bt, member);
    return 0;
}
