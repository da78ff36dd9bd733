// kernels.inc -- every __global__ kernel of the backend (included by lorads_hip.hip inside its anonymous namespace).
// Sections: row/entry gather kernels, constraint kernels, CG scalars, lockstep (segmented) CG, LP block, vector kernels.
// ------------------------------------------------------------------ kernels
// Column slices: lane l of an LG-lane group owns columns (l + c*LG)*W .. +W-1 for c = 0..NS-1 (W = 2: one
// 16-byte load per step).  NS is a compile-time constant and every load is UNCONDITIONAL (the address is
// clamped into the row, the value masked afterwards): a per-element `if (j < r) load` makes hipcc branch
// around each load and wait vmcnt(0) per element, which serialises the gather (cdna_hip_programming.md 5, trap c).
template <int LG, bool V2, int NS>
struct Slice {
    static constexpr int W = V2 ? 2 : 1;
    __device__ static __forceinline__ void load(const double *__restrict__ row, int r, int lane, double (&v)[NS][W]) {
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            const int j = (lane + c * LG) * W;
            const bool ok = j < r;
            const int jc = ok ? j : 0;
            if (V2) {
                const double2 t = *(const double2 *)(row + jc);
                v[c][0] = ok ? t.x : 0.0;
                v[c][W - 1] = ok ? t.y : 0.0;
            } else {
                const double t = row[jc];
                v[c][0] = ok ? t : 0.0;
            }
        }
    }
    // the same loads without the mask: a slice beyond r holds the row's first columns.  For callers that mask the slice's results.
    __device__ static __forceinline__ void load_raw(const double *__restrict__ row, int r, int lane, double (&v)[NS][W]) {
        static_assert(V2, "the 16-byte form only");
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            const int j = (lane + c * LG) * W;
            const double2 t = *(const double2 *)(row + (j < r ? j : 0));
            v[c][0] = t.x;
            v[c][1] = t.y;
        }
    }
};

// Row outputs written THROUGH the L2 (`sc1`; DESIGN.md 4 item 11, LORADS_WT_STORES): a plain store leaves its line dirty in the
// XCD's L2 and the end-of-kernel release writes all of them back before the next kernel may start; a write-through store sends the
// line on at once, beside the rest of the kernel.  `wt` is wave-uniform (a bit of a kernel argument: one scalar branch), `off` the
// element offset from `p`.  The 16-byte form has no builtin with a 64-bit address, so it is one asm store; `s_nop 1` keeps the
// next instruction off its data registers until the store has read them.  hipcc does not count the asm store in vmcnt, so its later
// waits wait for more than it thinks, never for less.  No "memory" clobber (it would pin the gathers that follow behind the store):
// what orders the store against the loads of the same bytes is its data, which is computed from them -- NO KERNEL LOADS, IN THE SAME
// LAUNCH, BYTES IT STORED THIS WAY: k_front_cw writes out / rhs_out / contrib and reads none of them; the CG0 form of k_spmm_ell
// reads its rows of x and r before it forms what it stores there, and R is written only; the plain form writes `out` only.
__device__ __forceinline__ void store16(double *p, size_t off, double a, double b, bool wt) {
    if (wt) {
        typedef double d2v __attribute__((ext_vector_type(2)));
        const d2v v = {a, b};
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p + off), "v"(v));
    } else {
        *(double2 *)(p + off) = make_double2(a, b);
    }
}
__device__ __forceinline__ void store8(double *p, size_t off, double a, bool wt) {
    if (wt) __hip_atomic_store(p + off, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else p[off] = a;
}

// pair dot of one pattern entry, LG lanes: x_p.y_q + x_q.y_p (p != q) or x_p.y_p; all row loads issued first
template <int LG, bool V2, int NS>
__device__ __forceinline__ double pair_dot(const double *__restrict__ X, const double *__restrict__ Y, int p, int q, int r,
                                           int lane) {
    constexpr int W = V2 ? 2 : 1;
    double a[NS][W], b[NS][W], cc[NS][W], d[NS][W];
    Slice<LG, V2, NS>::load(X + (size_t)p * r, r, lane, a);
    Slice<LG, V2, NS>::load(Y + (size_t)q * r, r, lane, b);
    if (X == Y) { // same factor on both sides (every evaluation on R): the second product is the first one again --
                  // s1 + s1 is exactly what s1 + s2 gives, with half the row loads
        double s1 = 0.0;
#pragma unroll
        for (int c = 0; c < NS; ++c)
#pragma unroll
            for (int w = 0; w < W; ++w) s1 += a[c][w] * b[c][w];
        return p == q ? s1 : s1 + s1;
    }
    Slice<LG, V2, NS>::load(X + (size_t)q * r, r, lane, cc);
    Slice<LG, V2, NS>::load(Y + (size_t)p * r, r, lane, d);
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c)
#pragma unroll
        for (int w = 0; w < W; ++w) { s1 += a[c][w] * b[c][w]; s2 += cc[c][w] * d[c][w]; }
    return p == q ? s1 : s1 + s2;
}

// T_e = X_p.Y_q + X_q.Y_p  (p != q)   |   X_p.Y_p  (p == q); LG lanes share one pattern entry
template <int LG, bool V2, int NS>
__global__ __launch_bounds__(TPB) void k_pairdots(int ne, const int *__restrict__ erow, const int *__restrict__ ecol,
                                                  const double *__restrict__ X, const double *__restrict__ Y, int r,
                                                  double *__restrict__ T, Guard g) {
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const int e = (blockIdx.x * TPB + threadIdx.x) / LG, lane = threadIdx.x % LG;
    const bool act = e < ne;
    const int p = act ? erow[e] : 0, q = act ? ecol[e] : 0;
    double s = pair_dot<LG, V2, NS>(X, Y, p, q, r, lane);
    s = group_sum<LG>(s);
    if (GATE_OPEN && act && lane == 0) T[e] = s;
}

// Constraint values straight from the factors: w_i = sum_{entries e of A_i} a_e pairdot_e(X, Y), ONE WAVEFRONT PER
// CONSTRAINT (64 / LG entries in flight, LG lanes each), then the same bookkeeping as k_cv -- the pair-dot array T is
// never written.  w_out (may be null) additionally keeps the plain values (the operator's constraint weights).
struct ResArgs { // k_cw in an evaluation: residual partials (null b: off)
    const double *b, *lambda;
    double *part_v, *part_d;
};
// ONE = true: one entry per group and trip (64 / LG entries of the constraint in flight, nothing fetched twice) -- the
// form for fixed-width constraints that fit one trip (LG = 4, up to 16 entries: the headline's 10-entry constraints).
template <int LG, bool V2, int NS, bool ONE = false>
__global__ __launch_bounds__(TPB) void k_cw(int nrow, const int *__restrict__ a_ptr, const int *__restrict__ a_p,
                                            const double *__restrict__ a_val, const int *__restrict__ a_q,
                                            const double *__restrict__ X,
                                            const double *__restrict__ Y, int r, double scale, double *__restrict__ w_out,
                                            double *__restrict__ cv, int mode, const int *__restrict__ row_idx,
                                            double *__restrict__ vec, Guard g, int ell_w, InitArgs ia, ResArgs ra,
                                            Deferred d = Deferred{}) {
    // d.st != null (never together with ia.st): the convergence test of the solve this kernel waits for rides on it
    // (the evaluation's first kernel when the average has been left by the last update, see k_cg_update)
    __shared__ double sh[8];
    DefPriv dv{};
    if (d.st) dv = deferred_private(d);
    // ia.st != null: first kernel of a solve's iteration 0, the solve's start rides on it (see InitArgs).  Its partial sums
    // are fetched here, ahead of the kernel's own loads, and reduced over the workgroup only after the gathers: the two
    // latencies overlap
    const Gate gt = gate_load(ia.st ? Guard{nullptr, g.need} : g); // (a carried start replaces the solve's own word)
    double iv[2] = {0.0, 0.0};
    // (up to 1024 partials per sum: the eight loads are only ISSUED here and added up after the gathers)
    const bool ia_small = ia.st && ia.nrr <= 4 * TPB && ia.nb <= 4 * TPB;
    double ipr[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    if (ia_small) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = threadIdx.x + k * TPB;
            ipr[0][k] = ia.part_rr[j < ia.nrr ? j : 0];
            ipr[1][k] = ia.part_b[j < ia.nb ? j : 0];
        }
    } else if (ia.st) init_private(ia, iv);
    constexpr int GR = 64 / LG; // entry groups per wavefront
    const int i = (blockIdx.x * TPB + threadIdx.x) >> 6, lane64 = threadIdx.x & 63;
    const int grp = lane64 / LG, lane = lane64 % LG;
    const bool act = i < nrow;
    const int ic = act ? i : 0;
    // evaluation: the constraint's global index, b and lambda are requested now, beside the entry lists -- not after the
    // gathers, where they were two more dependent round trips at the kernel's tail
    int gi_pre = 0;
    double b_pre = 0.0, l_pre = 0.0;
    if (ra.b) { gi_pre = row_idx[ic]; b_pre = ra.b[gi_pre]; l_pre = ra.lambda[gi_pre]; }
    // ell_w > 0: the entry arrays are padded to ell_w per constraint (a = 0 in the padding) -- no row-pointer load
    // heads the dependent-load chain
    const int t0 = ell_w ? ic * ell_w : a_ptr[ic], t1 = !act ? t0 : ell_w ? t0 + ell_w : a_ptr[ic + 1];
    // two entries per group and trip: the (row, col, a) of both are fetched before the first row gather (rows and
    // columns are stored per constraint entry -- no detour through the pattern entry)
    double acc = 0.0;
    if (ONE) {
        for (int t = t0 + grp; t < t1; t += GR) {
            const int p0 = a_p[t], q0 = a_q[t];
            const double c0 = a_val[t];
            acc += c0 * pair_dot<LG, V2, NS>(X, Y, p0, q0, r, lane);
        }
    } else
    for (int t = t0 + grp; t < t1; t += 2 * GR) {
        const int tb = t + GR < t1 ? t + GR : t;
        const int p0 = a_p[t], q0 = a_q[t], p1 = a_p[tb], q1 = a_q[tb];
        const double c0 = a_val[t], c1 = t + GR < t1 ? a_val[tb] : 0.0;
        const double d0 = pair_dot<LG, V2, NS>(X, Y, p0, q0, r, lane);
        const double d1 = pair_dot<LG, V2, NS>(X, Y, p1, q1, r, lane);
        acc += c0 * d0;
        acc += c1 * d1;
    }
    const double s = wave_sum(acc);
    if (ia_small) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = threadIdx.x + k * TPB;
            iv[0] += j < ia.nrr ? ipr[0][k] : 0.0;
            iv[1] += j < ia.nb ? ipr[1][k] : 0.0;
        }
    }
    // with a solve's start on board: gated stage (-1) or converged at the initial residual (2) -> nothing to do
    const bool live = ia.st ? finish_init(ia, !(g.need && gt.vn == 0), iv, sh) == 0
                            : d.st ? !blocked_after(g, d, finish_deferred(d, dv, sh).done) : GATE_OPEN;
    if (live && act && lane64 == 0) {
        if (w_out) w_out[i] = s;
        if (vec) {
            const int gi = ra.b ? gi_pre : row_idx[i];
            if (mode == CV_SET) vec[gi] = s * scale;
            else if (mode == CV_ADD) vec[gi] += s * scale;
            else vec[gi] += s - cv[i];
        }
        if (cv) cv[i] = s;
    }
    if (ra.b) { // evaluation: the partials of sum (b - w)^2 and b.lambda ride along (as k_cv_res leaves them)
        double vd[2] = {0.0, 0.0};
        if (act && lane64 == 0) {
            const double bi = b_pre, t = bi - s * scale;
            vd[0] = t * t;
            vd[1] = bi * l_pre;
        }
        block_sum_n<2>(vd, sh);
        if (live && threadIdx.x == 0) { ra.part_v[blockIdx.x] = vd[0]; ra.part_d[blockIdx.x] = vd[1]; }
    }
}

// The evaluation of a single cone on the k_cw path in ONE launch (k_cw on (R, R) with its residual partials + k_obj before):
// workgroups [0, g_cw) are k_cw's -- one wavefront per fixed-width constraint, 4 lanes per entry: constrVal / constrValSum <-
// A(R R^T) (quirk Q1) and the partials of ||b - A(R R^T)||^2, b . lambda -- workgroups [g_cw, g_cw + g_obj) are k_obj's: the
// partials of <C, R R^T> over C's entries.  Neither half is bound by bandwidth alone at this size (11.9 and 7.6 us in
// situ for 32 + 90 MB of rows), so side by side they take little more than the longer one.  Same arithmetic, same partial
// slots as the two kernels (LORADS_FUSE_EVAL=0: those).  Carries a waiting convergence test like k_cw: every workgroup
// evaluates it, workgroup 0 (a k_cw workgroup) publishes the state.
template <int NS4, int NS>
__global__ __launch_bounds__(TPB) void k_eval_cw_obj(int nrow, int ell_w, const int *__restrict__ a_p, const double *__restrict__ a_val,
                                                     const int *__restrict__ a_q, const double *__restrict__ R, int r,
                                                     double *__restrict__ cv, const int *__restrict__ row_idx, double *__restrict__ vec,
                                                     ResArgs ra, int g_cw, int ne, const int *__restrict__ erow,
                                                     const int *__restrict__ ecol, const double *__restrict__ cval,
                                                     double *__restrict__ part_obj, Guard g, Deferred d) {
    __shared__ double sh[8];
    const Gate gt = gate_load(g);
    DefPriv dv{};
    if (d.st) dv = deferred_private(d);
    if ((int)blockIdx.x < g_cw) { // ---- k_cw<4, true, NS4, ONE> on (R, R), CV_SET, with the residual partials
        constexpr int LG = 4, GR = 16;
        const int i = (blockIdx.x * TPB + threadIdx.x) >> 6, lane64 = threadIdx.x & 63;
        const int grp = lane64 / LG, lane = lane64 % LG;
        const bool act = i < nrow;
        const int ic = act ? i : 0;
        const int gi = row_idx[ic];
        const double bi = ra.b[gi], li = ra.lambda[gi];
        const int t0 = ic * ell_w, t1 = act ? t0 + ell_w : t0;
        double acc = 0.0;
        for (int t = t0 + grp; t < t1; t += GR) {
            const int p0 = a_p[t], q0 = a_q[t];
            const double c0 = a_val[t];
            acc += c0 * pair_dot<LG, true, NS4>(R, R, p0, q0, r, lane);
        }
        const double s = wave_sum(acc);
        const bool live = d.st ? !blocked_after(g, d, finish_deferred(d, dv, sh).done) : GATE_OPEN;
        if (live && act && lane64 == 0) { vec[gi] = s * 1.0; cv[i] = s; }
        double vd[2] = {0.0, 0.0};
        if (act && lane64 == 0) {
            const double t = bi - s * 1.0;
            vd[0] = t * t;
            vd[1] = bi * li;
        }
        block_sum_n<2>(vd, sh);
        if (live && threadIdx.x == 0) { ra.part_v[blockIdx.x] = vd[0]; ra.part_d[blockIdx.x] = vd[1]; }
        return;
    }
    // ---- k_obj<8, true, NS> on (R, R)
    constexpr int LG = 8, per = TPB / LG;
    const int bid = blockIdx.x - g_cw, nblk = gridDim.x - g_cw;
    const int lane = threadIdx.x % LG;
    double sacc = 0.0;
    for (int e = bid * per + threadIdx.x / LG; e < ne; e += nblk * per)
        sacc += pair_dot<LG, true, NS>(R, R, erow[e], ecol[e], r, lane) * cval[e];
    const bool live = d.st ? !blocked_after(g, d, finish_deferred(d, dv, sh).done) : GATE_OPEN;
    const double t = block_sum(sacc, sh);
    if (live && threadIdx.x == 0) part_obj[bid] = t;
}

__global__ void k_fill(size_t len, double v, double *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) y[i] = v;
}

// Both pair dots of the line search from one visit of the four rows (ALMCalq12p12, lorads_alm.c:540-560):
// t1 = sym-pair(R, D), t2 = sym-pair(D, D), each summed exactly as pair_dot does.
template <int LG, bool V2, int NS>
__device__ __forceinline__ void pair_dot_rd(const double *__restrict__ R, const double *__restrict__ D, int p, int q, int r,
                                            int lane, double &t1, double &t2) {
    constexpr int W = V2 ? 2 : 1;
    double rp[NS][W], rq[NS][W], dp[NS][W], dq[NS][W];
    Slice<LG, V2, NS>::load(R + (size_t)p * r, r, lane, rp);
    Slice<LG, V2, NS>::load(D + (size_t)q * r, r, lane, dq);
    Slice<LG, V2, NS>::load(R + (size_t)q * r, r, lane, rq);
    Slice<LG, V2, NS>::load(D + (size_t)p * r, r, lane, dp);
    double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c)
#pragma unroll
        for (int w = 0; w < W; ++w) {
            a1 += rp[c][w] * dq[c][w]; a2 += rq[c][w] * dp[c][w];
            b1 += dp[c][w] * dq[c][w]; b2 += dq[c][w] * dp[c][w];
        }
    t1 = p == q ? a1 : a1 + a2;
    t2 = p == q ? b1 : b1 + b2;
}
template <int LG, bool V2, int NS>
__global__ __launch_bounds__(TPB) void k_pairdots_rd(int ne, const int *__restrict__ erow, const int *__restrict__ ecol,
                                                     const double *__restrict__ R, const double *__restrict__ D, int r,
                                                     double *__restrict__ T1, double *__restrict__ T2) {
    const int e = (blockIdx.x * TPB + threadIdx.x) / LG, lane = threadIdx.x % LG;
    const bool act = e < ne;
    const int p = act ? erow[e] : 0, q = act ? ecol[e] : 0;
    double t1, t2;
    pair_dot_rd<LG, V2, NS>(R, D, p, q, r, lane, t1, t2);
    t1 = group_sum<LG>(t1);
    t2 = group_sum<LG>(t2);
    if (act && lane == 0) { T1[e] = t1; T2[e] = t2; }
}
template <int LG, bool V2, int NS>
__global__ __launch_bounds__(TPB) void k_obj_rd(int ne, const int *__restrict__ erow, const int *__restrict__ ecol,
                                                const double *__restrict__ cval, const double *__restrict__ R,
                                                const double *__restrict__ D, int r, double *__restrict__ part1,
                                                double *__restrict__ part2) {
    __shared__ double sh[4];
    const int lane = threadIdx.x % LG, per = TPB / LG;
    double s1 = 0.0, s2 = 0.0;
    for (int e = blockIdx.x * per + threadIdx.x / LG; e < ne; e += gridDim.x * per) {
        double t1, t2;
        pair_dot_rd<LG, V2, NS>(R, D, erow[e], ecol[e], r, lane, t1, t2);
        s1 += t1 * cval[e];
        s2 += t2 * cval[e];
    }
    const double u1 = block_sum(s1, sh), u2 = block_sum(s2, sh);
    if (threadIdx.x == 0) { part1[blockIdx.x] = u1; part2[blockIdx.x] = u2; }
}
// q1 = 2 A(T1), q2 = A(T2) for a cone that sees every constraint (vec1/vec2 are SET); cv keeps the second one,
// as the two successive k_cv passes leave it.  The rows a workgroup owns also give its share of the seven
// line-search sums (see k_linesearch), so no kernel has to stream the m-vectors again.
__global__ __launch_bounds__(TPB) void k_cv_rd(int nrow, const int *__restrict__ a_ptr, const int *__restrict__ a_e,
                                               const double *__restrict__ a_val, const double *__restrict__ T1,
                                               const double *__restrict__ T2, double *__restrict__ cv,
                                               const int *__restrict__ row_idx, double *__restrict__ vec1,
                                               double *__restrict__ vec2, const double *__restrict__ b,
                                               const double *__restrict__ csum, const double *__restrict__ lambda,
                                               double *__restrict__ part, int pstride);
// out[b] = scale_b * sum(part_b), b = blockIdx.x in {0, 1}
__global__ __launch_bounds__(TPB) void k_finalize2(const double *__restrict__ part0, const double *__restrict__ part1, int n,
                                                   double scale0, double scale1, double *out) {
    __shared__ double sh[4];
    const double t = sum_partials(blockIdx.x ? part1 : part0, n, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = (blockIdx.x ? scale1 : scale0) * t;
}

// partial of sum_e c_e * pairdot_e  (objective <C, sym(X Y^T)>); grid-stride so that the grid stays small
template <int LG, bool V2, int NS>
__global__ __launch_bounds__(TPB) void k_obj(int ne, const int *__restrict__ erow, const int *__restrict__ ecol,
                                             const double *__restrict__ cval, const double *__restrict__ X,
                                             const double *__restrict__ Y, int r, double *__restrict__ part, Guard g,
                                             double *__restrict__ stage_tail = nullptr) {
    __shared__ double sh[4];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const int lane = threadIdx.x % LG, per = TPB / LG;
    double s = 0.0; // every lane keeps its own slice; the block sum adds the slices
    for (int e = blockIdx.x * per + threadIdx.x / LG; e < ne; e += gridDim.x * per)
        s += pair_dot<LG, V2, NS>(X, Y, erow[e], ecol[e], r, lane) * cval[e];
    const double t = block_sum(s, sh);
    if (GATE_OPEN && threadIdx.x == 0) part[blockIdx.x] = t;
    // sharded evaluation: the partials travel through the all-reduce themselves (part = stage_tail + 2); the two words in
    // front of them are [unused | "this rank's sweep is unfinished"], written whether or not the kernel is gated
    if (stage_tail && blockIdx.x == 0 && threadIdx.x == 0) {
        stage_tail[0] = 0.0;
        stage_tail[1] = GATE_OPEN ? 0.0 : 1.0;
    }
}

// w_i = sum_k a_k T[e_k]; 8 lanes per constraint.  `mode` says what happens to the running
// m-vector `vec` (constrValSum / q1 / q2): CV_SET vec[g] = scale w, CV_ADD vec[g] += scale w,
// CV_DELTA vec[g] += w - old (the subtract/recompute/add bookkeeping of LORADSUpdateSDPVar,
// lorads_alg_common.c:199-203); cv (compact constrVal[k]) gets w
__global__ __launch_bounds__(TPB) void k_cv(int nrow, const int *__restrict__ a_ptr, const int *__restrict__ a_e,
                                            const double *__restrict__ a_val, const double *__restrict__ T, double scale,
                                            double *__restrict__ cv, int mode, const int *__restrict__ row_idx,
                                            double *__restrict__ vec, Guard g) {
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const int i = (blockIdx.x * TPB + threadIdx.x) / 8, lane = threadIdx.x & 7;
    const bool act = i < nrow;
    double s = 0.0;
    if (act)
        for (int t = a_ptr[i] + lane; t < a_ptr[i + 1]; t += 8) s += a_val[t] * T[a_e[t]];
    s = group_sum<8>(s);
    if (GATE_OPEN && act && lane == 0) {
        if (vec) {
            const int gi = row_idx[i];
            if (mode == CV_SET) vec[gi] = s * scale;
            else if (mode == CV_ADD) vec[gi] += s * scale;
            else vec[gi] += s - cv[i];
        }
        if (cv) cv[i] = s;
    }
}

// the bookkeeping half of k_cw / k_cv when the constraint values w of the pair are already known (kept up to date by
// the CG updates): constrVal[k] <- w, constrValSum += w - old  (lorads_alg_common.c:199-203)
// drow != null (Max-Cut-type cones): w holds the row dots U_p . V_p and constraint i = da_i e_p e_p^T has the value da_i w[drow_i]
__global__ __launch_bounds__(TPB) void k_refresh_w(int nrow, const double *__restrict__ w, double *__restrict__ cv,
                                                   const int *__restrict__ row_idx, double *__restrict__ vec, Guard g,
                                                   Deferred d = Deferred{}, const int *__restrict__ drow = nullptr,
                                                   const double *__restrict__ da = nullptr) {
    __shared__ double sh[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x, ic = i < nrow ? i : 0;
    // the kernel's own operands first: they fly while a carried test is evaluated
    const double s = drow ? da[ic] * w[drow[ic]] : w[ic], old = cv[ic];
    const int gi = row_idx[ic];
    const double v = vec[gi];
    bool live;
    if (d.st) live = !blocked_after(g, d, run_deferred(d, sh).done);
    else live = !blocked(g);
    if (live && i < nrow) { vec[gi] = v + (s - old); cv[i] = s; }
}

struct WArgs {
    const double *w;      // W_COMPACT: compact weights [nrow]
    const double *csum;   // global m-vectors
    const double *b;
    const double *lambda;
    const double *cv;     // compact [nrow]
    const int *row_idx;
    DS rho;
    // W_ADMM with a dual update on board (lambda_out != null): the weights use lambda + rho_dual b - rho_dual csum
    // (LORADSUpdateDualVar, lorads_alg_common.c:319-332, exactly as k_dual_update forms it) and the owner pair of every
    // constraint (sign bit of its e_con word) stores that value to lambda_out -- a SECOND vector: other entries of
    // the constraint are still reading the old one
    double *lambda_out;
    DS rho_dual;
    // W_ADMM_V on a Max-Cut-type cone: w holds row dots, constraint i has the value da[i] * w[drow[i]]
    const int *drow;
    const double *da;
};
__device__ __forceinline__ double weight_of(int mode, const WArgs &a, int i) {
    if (mode == W_COMPACT) return a.w[i];
    const int g = a.row_idx ? a.row_idx[i] : i; // (null: the cone sees every constraint in file order -- one dependent load less)
    if (mode == W_ADMM_V) { // W_ADMM on top of the refresh k_refresh_w would have stored (same arithmetic, nothing written)
        const double s = a.drow ? a.da[i] * a.w[a.drow[i]] : a.w[i];
        const double cs = a.csum[g] + (s - a.cv[i]);
        return ((cs - a.b[g]) - s) * dsv(a.rho) - a.lambda[g];
    }
    if (mode == W_ADMM) {
        double lam = a.lambda[g];
        if (a.lambda_out) { // (uniform) the dual update of the previous iteration, not stored yet
            const double rd = dsv(a.rho_dual);
            const double l = lam + rd * a.b[g];
            lam = l + (-rd) * a.csum[g];
        }
        return ((a.csum[g] - a.b[g]) - a.cv[i]) * dsv(a.rho) - lam; // lorads_admm.c:432-445
    }
    if (mode == W_DUAL) return -a.lambda[g];                                            // data/lorads_solver.c:1011
    const double rho = dsv(a.rho);
    return (-a.lambda[g] - rho * a.b[g]) + rho * a.csum[g];                             // lorads_alm.c:22-26
}
// S_e = [cbase_e] + sum over the constraints touching e of weight_i * a
__global__ __launch_bounds__(TPB) void k_sval(int ne, const int *__restrict__ e_ptr, const int *__restrict__ e_con,
                                              const double *__restrict__ e_val, const double *__restrict__ cbase, int mode,
                                              WArgs wa, double *__restrict__ S, Guard g, CGState *reset, int nreset,
                                                   const double *__restrict__ w2 = nullptr, double *__restrict__ S2 = nullptr,
                                                   Deferred d = Deferred{}) {
    __shared__ double sh[4];
    // first kernel of a sweep: mark every later stage "not finished" (stage 0 itself is reset by its k_cg_init,
    // nothing before that reads it)
    if (reset && blockIdx.x == 0 && threadIdx.x < nreset) reset[threadIdx.x].done = 0;
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    DefPriv dv{};
    if (d.st) dv = deferred_private(d); // a carried convergence test (the V-solve's front after a virtual refresh)
    const int e = blockIdx.x * TPB + threadIdx.x;
    const bool act = e < ne;
    double s = 0.0, s2 = 0.0;
    if (act) {
        s = cbase ? cbase[e] : 0.0;
        for (int t = e_ptr[e]; t < e_ptr[e + 1]; ++t) {
            const int iw = e_con[t], i = iw & 0x7fffffff; // (sign bit: this pair stores the constraint's new multiplier)
            const double a = e_val[t];
            s += weight_of(mode, wa, i) * a;
            if (w2) s2 += w2[i] * a; // second image on the same pattern: sum_i w2_i A_i (the fused front's operator part)
            if (wa.lambda_out && iw < 0) { // (this kernel is then the ungated first kernel of a sweep)
                const int gI = wa.row_idx ? wa.row_idx[i] : i;
                const double rd = dsv(wa.rho_dual);
                const double l = wa.lambda[gI] + rd * wa.b[gI];
                wa.lambda_out[gI] = l + (-rd) * wa.csum[gI];
            }
        }
    }
    const bool live = d.st ? !blocked_after(g, d, finish_deferred(d, dv, sh).done) : GATE_OPEN;
    if (live && act) {
        if (w2) *(double2 *)(S2 + 2 * (size_t)e) = make_double2(s, s2); // both images side by side: ONE 16-byte gather per slot in k_spmm2<FRONT>
        else S[e] = s;
    }
}
// S = G T with G = A A^T over pattern entries (w = A T and S = A^T w in one pass); 8 lanes per entry so
// that the dependent (index -> T) loads of one Gram row are in flight together
__global__ __launch_bounds__(TPB) void k_sgram(int ne, const int *__restrict__ g_ptr, const int *__restrict__ g_col,
                                               const double *__restrict__ g_val, const double *__restrict__ T,
                                               double *__restrict__ S, Guard g) {
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const int e = (blockIdx.x * TPB + threadIdx.x) / 8, lane = threadIdx.x & 7;
    const bool act = e < ne;
    double s = 0.0;
    if (act)
        for (int t = g_ptr[e] + lane; t < g_ptr[e + 1]; t += 8) s += g_val[t] * T[g_col[t]];
    s = group_sum<8>(s);
    if (GATE_OPEN && act && lane == 0) S[e] = s;
}

// Y_p = epilogue( sum over the neighbours (q,e) of row p of S_e X_q ), LG lanes per row, + fused reduction.
// CW = true: the slot list is per (neighbour, constraint): adj_e holds the compact constraint index, S the constraint
// weights w and adj_a the coefficient a, so that the slot coefficient a * w[con] is formed without an S array.
template <int LG, bool V2, int NS, bool CW = false>
__global__ __launch_bounds__(TPB) void k_spmm(int n, const int *__restrict__ adj_ptr, const int *__restrict__ adj_col,
                                              const int *__restrict__ adj_e, const double *__restrict__ S,
                                              const double *__restrict__ X, int r, int mode, const double *__restrict__ xin,
                                              const double *__restrict__ rhs, DS rho_s, double *__restrict__ out,
                                              double *__restrict__ part, Guard g, const double *__restrict__ dense_add,
                                              const double *__restrict__ adj_a = nullptr) {
    __shared__ double sh[4];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const double rho = dsv(rho_s);
    constexpr int W = V2 ? 2 : 1;
    const int row = (blockIdx.x * TPB + threadIdx.x) / LG, lane = threadIdx.x % LG;
    const bool act = row < n;
    const int rowc = act ? row : 0;
    double acc[NS][W];
    // dense part of (C + sum_i w_i A_i) X, computed by k_dense_cx, when C is stored dense
    if (dense_add) Slice<LG, V2, NS>::load(dense_add + (size_t)rowc * r, r, lane, acc);
    else {
#pragma unroll
        for (int c = 0; c < NS; ++c)
#pragma unroll
            for (int w = 0; w < W; ++w) acc[c][w] = 0.0;
    }
    const int t0 = adj_ptr[rowc], t1 = act ? adj_ptr[rowc + 1] : t0;
    // epilogue operands are fetched up front: the kernel is bound by its chain of dependent loads
    // (row pointer -> neighbour index -> coefficient / neighbour row), not by bandwidth
    const size_t base = (size_t)rowc * r;
    double xi[NS][W], rh[NS][W];
    if (mode == OP_CG || mode == OP_RES) Slice<LG, V2, NS>::load(xin + base, r, lane, xi);
    if (mode == OP_RES) Slice<LG, V2, NS>::load(rhs + base, r, lane, rh);
    if (mode == OP_RHS) Slice<LG, V2, NS>::load(X + base, r, lane, xi);
    // 4 neighbours per trip: the 8 index loads, then the 4 coefficient and 4 row gathers are all issued
    // before the first use (out-of-range slots repeat the last neighbour with coefficient 0)
    for (int t = t0; t < t1; t += 4) {
        int q[4], e[4];
        double aa[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int tt = t + u < t1 ? t + u : t1 - 1;
            q[u] = adj_col[tt];
            e[u] = adj_e[tt];
            aa[u] = CW ? adj_a[tt] : 1.0;
        }
        double sc[4], v[4][NS][W];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            sc[u] = CW ? aa[u] * S[e[u]] : S[e[u]];
            Slice<LG, V2, NS>::load(X + (size_t)q[u] * r, r, lane, v[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double su = t + u < t1 ? sc[u] : 0.0;
#pragma unroll
            for (int c = 0; c < NS; ++c)
#pragma unroll
                for (int w = 0; w < W; ++w) acc[c][w] += su * v[u][c][w];
        }
    }
    double local = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const int j0 = (lane + c * LG) * W;
        double v[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const double a = acc[c][w];
            if (mode == OP_CG) { v[w] = xi[c][w] + a; local += xi[c][w] * v[w]; }
            else if (mode == OP_RES) { v[w] = rh[c][w] - (xi[c][w] + a); local += v[w] * v[w]; }
            else if (mode == OP_RHS) { v[w] = xi[c][w] - a / rho; local += fabs(v[w]); }
            else { v[w] = 2.0 * a; local += v[w] * v[w]; }
        }
        if (GATE_OPEN && act && j0 < r) {
            if (V2) *(double2 *)(out + base + j0) = make_double2(v[0], v[W - 1]);
            else out[base + j0] = v[0];
        }
    }
    const double t = block_sum(act ? local : 0.0, sh);
    if (GATE_OPEN && threadIdx.x == 0) part[blockIdx.x] = t;
}

// k_spmm (CW = false) with the neighbour list read eight slots at a time: lane l of a row's group fetches slot t + l
// (one coalesced load per array and trip instead of one broadcast load per slot) and the coefficient S[e] of its slot,
// the eight neighbour rows are gathered side by side, and the next trip's indices are requested before the current
// rows are consumed.  Slots are accumulated in list order, exactly as k_spmm does.
// FRONT = true is the whole front of a CG solve in one pass over the neighbour rows (mode is ignored):
//   rhs = X_p - (S X)_p / rho            (lorads_admm.c:432-463; part_b gets the partials of ||rhs||_1)
//   out = rhs - (xin_p + (S2 X)_p)       (initial residual, lorads_cgs.c:149-156; part gets the partials of ||out||^2)
// with S2 = sum_i w_i A_i on the same pattern -- one gather of X's rows feeds both sums.
template <int LG, bool V2, int NS, bool FRONT>
__global__ __launch_bounds__(TPB) void k_spmm2(int n, const int *__restrict__ adj_ptr, const int *__restrict__ adj_col,
                                               const int *__restrict__ adj_dyn, const double *__restrict__ adj_sval,
                                               const double *__restrict__ S,
                                               const double *__restrict__ S2, const double *__restrict__ X, int r, int mode,
                                               const double *__restrict__ xin, const double *__restrict__ rhs, DS rho_s,
                                               double *__restrict__ out, double *__restrict__ rhs_out,
                                               double *__restrict__ part, double *__restrict__ part_b, Guard g,
                                               const double *__restrict__ dense_add, const double *__restrict__ gd = nullptr,
                                               double *__restrict__ uv_out = nullptr, const int *__restrict__ rc_con = nullptr,
                                               int rc_w = 0, const double *__restrict__ rc_a = nullptr, WArgs wa = WArgs{},
                                               int wmode = 0, CGState *reset = nullptr, int nreset = 0, Deferred d = Deferred{}) {
    // FRONT on a Max-Cut-type cone with rc_con != null: NO coefficient pass (k_sval) before this kernel.  The only entries
    // whose coefficient changes are the diagonal ones of rows that hold constraints; the row forms its own
    // sum_i weight_i a_i from the m-vectors (weight_of, as k_sval did; rc_con: row -> constraints in fixed width rc_w, rc_a: a_i)
    // and adds it to the objective's part, which the list carries for every slot (adj_sval).  The kernel then also carries
    // what k_sval carried: the sweep's reset words, a waiting convergence test, the multipliers of a pending dual update.
    __shared__ double sh[8];
    if (FRONT && reset && blockIdx.x == 0 && threadIdx.x < nreset) reset[threadIdx.x].done = 0;
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const double rho = dsv(rho_s);
    DefPriv dv{};
    if (FRONT && d.st) dv = deferred_private(d);
    constexpr int W = V2 ? 2 : 1;
    // neighbour rows in flight per lane (register budget: three workgroups per CU at the headline shape NS = 3)
    constexpr int CH = FRONT ? (NS <= 1 ? 8 : NS <= 3 ? 4 : 2) : (NS <= 5 ? 4 : 2);
    const int row = (blockIdx.x * TPB + threadIdx.x) / LG, lane = threadIdx.x % LG, l8 = lane & 7;
    const bool act = row < n;
    const int rowc = act ? row : 0;
    const size_t base = (size_t)rowc * r;
    const int t0 = adj_ptr[rowc], t1 = act ? adj_ptr[rowc + 1] : t0;
    int tn = t0 + l8;
    int tc = tn < t1 ? tn : (t1 > 0 ? t1 - 1 : 0);
    int qn = adj_col[tc], en = adj_dyn[tc];
    double svn = adj_sval[tc];
    double acc[NS][W], acc2[FRONT ? NS : 1][W];
    if (dense_add) Slice<LG, V2, NS>::load(dense_add + base, r, lane, acc);
    else {
#pragma unroll
        for (int c = 0; c < NS; ++c)
#pragma unroll
            for (int w = 0; w < W; ++w) acc[c][w] = 0.0;
    }
    if (FRONT) {
#pragma unroll
        for (int c = 0; c < NS; ++c)
#pragma unroll
            for (int w = 0; w < W; ++w) acc2[c][w] = 0.0;
    }
    double xi[NS][W], rh[NS][W];
    double dyn_add = 0.0; // this row's sum_i weight_i a_i (on-the-fly form)
    const bool self_dot = FRONT && rc_con && wmode == W_ADMM_VS;
    if (FRONT && rc_con) {
        const int ci = (lane < rc_w && act) ? rc_con[(size_t)rowc * rc_w + lane] : -1;
        const int cic = ci >= 0 ? ci : 0;
        double wgt;
        if (self_dot) {
            // W_ADMM_VS (lockstep sweep): the refresh after the previous solves was not stored and no array holds the row dots either --
            // the row's own pair is fetched first and U_p . V_p formed as k_pairdots forms it; the weight is W_ADMM_V's
            Slice<LG, V2, NS>::load(X + base, r, lane, xi);
            Slice<LG, V2, NS>::load(xin + base, r, lane, rh);
            double d0 = 0.0;
#pragma unroll
            for (int c = 0; c < NS; ++c)
#pragma unroll
                for (int w = 0; w < W; ++w) d0 += xi[c][w] * rh[c][w];
            d0 = group_sum<LG>(d0);
            const int gI = wa.row_idx ? wa.row_idx[cic] : cic;
            const double sv0 = rc_a[cic] * d0;
            const double cs = wa.csum[gI] + (sv0 - wa.cv[cic]);
            wgt = (((cs - wa.b[gI]) - sv0) * dsv(wa.rho) - wa.lambda[gI]) * rc_a[cic];
        } else wgt = weight_of(wmode, wa, cic) * rc_a[cic];
        if (wa.lambda_out && ci >= 0) { // (this kernel is then the ungated first kernel of a sweep; every constraint sits in one row)
            const int gI = wa.row_idx ? wa.row_idx[cic] : cic;
            const double rd = dsv(wa.rho_dual);
            const double l = wa.lambda[gI] + rd * wa.b[gI];
            wa.lambda_out[gI] = l + (-rd) * wa.csum[gI];
        }
        dyn_add = group_sum<LG>(ci >= 0 ? wgt : 0.0);
    }
    if (FRONT) {
        if (!self_dot) {
            Slice<LG, V2, NS>::load(X + base, r, lane, xi);
            Slice<LG, V2, NS>::load(xin + base, r, lane, rh);
        }
    } else {
        if (mode == OP_CG || mode == OP_RES) Slice<LG, V2, NS>::load(xin + base, r, lane, xi);
        if (mode == OP_RES) Slice<LG, V2, NS>::load(rhs + base, r, lane, rh);
        if (mode == OP_RHS) Slice<LG, V2, NS>::load(X + base, r, lane, xi);
    }
    for (int t = t0; t < t1; t += 8) {
        // the slot's coefficient: entries no constraint touches carry theirs in the list itself (adj_sval, streamed);
        // only the others (adj_dyn >= 0: the entry's index) gather it -- the lanes of static slots all ask for word 0
        const int q = qn, e = en < 0 ? 0 : en;
        const bool mine = t + l8 < t1, dyn = en >= 0;
        const double sv = svn;
        double s1, s2 = 0.0;
        if (FRONT && S2) { // the two images interleaved (k_sval): one gather instead of two
            const double2 ss = *(const double2 *)(S2 + 2 * (size_t)e);
            s1 = dyn ? ss.x : sv; s2 = dyn ? ss.y : 0.0;
        } else if (FRONT && rc_con) s1 = dyn ? sv + dyn_add : sv; // (a changing entry of such a cone is the row's own diagonal)
        else s1 = dyn ? S[e] : sv;
        tn = t + 8 + l8;
        tc = tn < t1 ? tn : t1 - 1;
        qn = adj_col[tc];
        en = adj_dyn[tc];
        svn = adj_sval[tc];
#pragma unroll
        for (int u0 = 0; u0 < 8; u0 += CH) {
            if (u0 == 0 || t + u0 < t1) {
                double v[CH][NS][W];
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const int qq = __shfl(q, u0 + u, 8);
                    Slice<LG, V2, NS>::load(X + (size_t)qq * r, r, lane, v[u]);
                }
                if (u0 == 0) { s1 = mine ? s1 : 0.0; s2 = mine ? s2 : 0.0; }
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const double a1 = __shfl(s1, u0 + u, 8);
                    const double a2 = FRONT ? __shfl(s2, u0 + u, 8) : 0.0;
#pragma unroll
                    for (int c = 0; c < NS; ++c)
#pragma unroll
                        for (int w = 0; w < W; ++w) {
                            acc[c][w] += a1 * v[u][c][w];
                            if (FRONT) acc2[c][w] += a2 * v[u][c][w];
                        }
                }
            }
        }
    }
    const bool live_ = (FRONT && d.st) ? !blocked_after(g, d, finish_deferred(d, dv, sh).done) : GATE_OPEN;
    // FRONT on a Max-Cut-type cone (gd != null): the operator part of the residual is row-local, g_p (x_p . V_p) V_p
    // exactly as k_op_diag forms it -- no second image, no second sum
    double dd = 0.0;
    if (FRONT && gd) {
#pragma unroll
        for (int c = 0; c < NS; ++c)
#pragma unroll
            for (int w = 0; w < W; ++w) dd += rh[c][w] * xi[c][w];
        dd = group_sum<LG>(dd);
        if (uv_out && act && lane == 0 && live_) uv_out[rowc] = dd; // U_p . V_p, exact, at every front (see k_op_diag)
        dd *= gd[rowc];
    }
    double local = 0.0, local_b = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const int j0 = (lane + c * LG) * W;
        double v[W], vb[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const double a = acc[c][w];
            if (FRONT) {
                vb[w] = xi[c][w] - a / rho; local_b += fabs(vb[w]);
                const double opx = gd ? rh[c][w] + dd * xi[c][w] : rh[c][w] + acc2[c][w];
                v[w] = vb[w] - opx; local += v[w] * v[w];
            } else if (mode == OP_CG) { v[w] = xi[c][w] + a; local += xi[c][w] * v[w]; }
            else if (mode == OP_RES) { v[w] = rh[c][w] - (xi[c][w] + a); local += v[w] * v[w]; }
            else if (mode == OP_RHS) { v[w] = xi[c][w] - a / rho; local += fabs(v[w]); }
            else { v[w] = 2.0 * a; local += v[w] * v[w]; }
        }
        if (live_ && act && j0 < r) {
            if (V2) *(double2 *)(out + base + j0) = make_double2(v[0], v[W - 1]);
            else out[base + j0] = v[0];
            if (FRONT) {
                if (V2) *(double2 *)(rhs_out + base + j0) = make_double2(vb[0], vb[W - 1]);
                else rhs_out[base + j0] = vb[0];
            }
        }
    }
    if (FRONT) {
        double two[2] = {act ? local : 0.0, act ? local_b : 0.0};
        block_sum_n<2>(two, sh);
        if (live_ && threadIdx.x == 0) { part[blockIdx.x] = two[0]; part_b[blockIdx.x] = two[1]; }
    } else {
        const double t = block_sum(act ? local : 0.0, sh);
        if (live_ && threadIdx.x == 0) part[blockIdx.x] = t;
    }
}

// k_spmm<CW> with the slot list in a fixed-width layout (EW = 8 or 16 slots per row, the same (neighbour, constraint)
// order as the CSR list; rows with more slots finish from the CSR list).  Lane l of a row's group fetches slot l (and
// l + 8): ONE coalesced index load per array instead of one broadcast load per slot, no row pointer at the head of the
// chain, and the constraint weights of all slots are gathered side by side while the neighbour rows are already on
// their way: the dependent-load chain is index -> (weight | neighbour rows) for every row, whatever its slot count.
// Padding slots name the row itself (an L1 hit) with coefficient 0.  Slots are accumulated in list order, exactly as
// k_spmm<CW> does.  mode = OP_CG or OP_RES.
//
// CG0 = true: CG iteration 0 of a cone on the one-kernel-front path (Cg0Args), the update that k_cg_update would run next is
// done here, row by row.  alpha = rr / (p.Q) needs the global dot p.Q, but with p_0 = r_0 it is known before this kernel starts:
// k_wsum forms w_i = sum over the slots s of constraint i of a_s (p_row(s) . V_col(s)), this kernel forms
// Q_p = p_p + sum over the slots s of row p of a_s w_con(s) V_col(s), and regrouping the slots of sum_p p_p . Q_p by constraint gives
//   p.Q = ||p||^2 + ||w||^2 = rr + ||w||^2          (cg0_alpha; k_wsum leaves the partials of ||w||^2)
// So Q stays in registers: x_p += alpha p_p, the partials of ||r_0 - alpha Q||^2 go to `part` (r stored when store_r), the kept
// constraint values follow x (w_acc += alpha w_p, on the low thread ids), R = (U + V) / 2 when asked for -- also in the gated-off
// "solve already over" case, as k_cg_update does -- and workgroup 0 writes the shadow state.  The kernel gathers rows of the
// fixed factor X only and reads and writes its own rows of p (= r) and x: no workgroup reads what another one writes.
struct Cg0Args {
    const CGState *st;            // the solve's state (rr)
    const double *part_ww;        // k_wsum's partials of ||w||^2
    int nww;
    double *x, *r;                // the solve variable, the residual (= p_0, the kernel's xin)
    int store_r;
    double *w_acc;                // null: no recurrence of the constraint values
    const double *w_p;
    int nw;
    CGState *shadow;
    const double *avg_other;      // avg_out != null: R = (avg_other + x) / 2
    double *avg_out;
    int wt;                       // WT_* bits: which row outputs go through the L2 (store16; the plain form reads WT_OUT from here too)
};
// the update of one element, shared by k_cg_update and the CG0 form of k_spmm_ell (same arithmetic, same bits)
struct CgElem { double x, r; };
__device__ __forceinline__ CgElem cg_elem(double alpha, double p, double q, double x, double r) {
    return CgElem{x + alpha * p, r - alpha * q};
}
__device__ __forceinline__ double cg_avg(double other, double x) { return (other + x) / 2; }
__device__ __forceinline__ double cg_wacc(double wa, double alpha, double wp) { return wa + alpha * wp; }
// alpha of CG iteration 0 from ||r_0||^2 and the ||w||^2 partials (see Cg0Args): every kernel that forms it sums the same
// partials in the same order
__device__ __forceinline__ double cg0_alpha(double rr, double ww) { return rr / (rr + ww); }

template <int LG, bool V2, int NS, int EW, bool CG0 = false>
__global__ __launch_bounds__(TPB) void k_spmm_ell(int n, int rpw, const int *__restrict__ adj_ptr, const int *__restrict__ adj_col,
                                                  const int *__restrict__ adj_con, const double *__restrict__ adj_a,
                                                  const int *__restrict__ ell_col, const int *__restrict__ ell_con,
                                                  const double *__restrict__ ell_a, const double *__restrict__ wgt,
                                                  const double *__restrict__ X, int r, int mode,
                                                  const double *xin, const double *__restrict__ rhs,
                                                  double *__restrict__ out, double *__restrict__ part, Guard g,
                                                  Cg0Args u = Cg0Args{}) {
    // (xin is not __restrict__: in the CG0 form the kernel writes its rows back through u.r, after it has read them)
    __shared__ double sh[4];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    // CG0: the state's rr and this thread's share of the ||w||^2 partials travel with the gate words; so do the kept constraint
    // value and its increment of thread id `gid` (the first of the m-vector slice this thread updates)
    double rr = 0.0, ww = 0.0, wa0 = 0.0, wp0 = 0.0;
    const int gid = blockIdx.x * TPB + threadIdx.x;
    if (CG0) {
        rr = u.st->rr;
        ww = private_partials(u.part_ww, u.nww);
        if (u.w_acc) { const int iw = gid < u.nw ? gid : 0; wa0 = u.w_acc[iw]; wp0 = u.w_p[iw]; }
    }
    constexpr int W = V2 ? 2 : 1;
    constexpr int NH = EW / 8;             // index words per lane
    constexpr int CH = NS <= 5 ? 4 : 2; // neighbour rows gathered per step (a step is skipped when the group has no such slots: 4.5 slots per row on average at the headline; 8 per step was 10.1 us, 4: 9.1 us, 2: 9.4 us)
    // rpw rows per workgroup (row_deal; TPB / LG: every lane group holds one): a lane group beyond rpw is a row past n in every sense
    const int grp = threadIdx.x / LG, row = blockIdx.x * rpw + grp, lane = threadIdx.x % LG;
    const bool act = grp < rpw && row < n;
    const int rowc = act ? row : 0;
    const size_t base = (size_t)rowc * r;
    const size_t eb = (size_t)rowc * EW + (lane & 7);
    int qc[NH], kc[NH];
    double ac[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) { qc[h] = ell_col[eb + 8 * h]; kc[h] = ell_con[eb + 8 * h]; ac[h] = ell_a[eb + 8 * h]; }
    const int t0 = adj_ptr[rowc], t1r = adj_ptr[rowc + 1]; // (both words exist for every clamped row: no predicated load)
    const int t1 = act ? t1r : t0;                         // (an inactive group stays out of row 0's CSR tail)
    double xi[NS][W], rh[NS][W], acc[NS][W];
    Slice<LG, V2, NS>::load(xin + base, r, lane, xi);
    // (OP_CG: an L1 hit, never used; CG0: the row of x)
    Slice<LG, V2, NS>::load((CG0 ? (const double *)u.x : mode == OP_RES ? rhs : xin) + base, r, lane, rh);
#pragma unroll
    for (int c = 0; c < NS; ++c)
#pragma unroll
        for (int w = 0; w < W; ++w) acc[c][w] = 0.0;
    // the weight gathers are unconditional too (padding names constraint 0; its product is masked below): a predicated
    // load would put a branch and a full wait in front of the neighbour-row gathers
    double wv[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) wv[h] = wgt[kc[h]];
    const int cnt = act ? t1 - t0 : 0;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        if (h == 0 || cnt > 8 * h) { // (h > 0: only the groups that have such slots gather them)
#pragma unroll
            for (int u0 = 0; u0 < 8; u0 += CH) {
                if (u0 > 0 && cnt <= 8 * h + u0) continue; // (the group has no such slots: nothing to gather)
                double v[CH][NS][W];
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const int q = __shfl(qc[h], u0 + u, 8);
                    Slice<LG, V2, NS>::load(X + (size_t)q * r, r, lane, v[u]);
                }
                const double sch = (lane & 7) + 8 * h < cnt ? ac[h] * wv[h] : 0.0;
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const double su = __shfl(sch, u0 + u, 8);
#pragma unroll
                    for (int c = 0; c < NS; ++c)
#pragma unroll
                        for (int w = 0; w < W; ++w) acc[c][w] += su * v[u][c][w];
                }
            }
        }
    }
    // (slots per trip: four; two in the CG0 form, which holds the rows of x and r besides -- with four, hipcc kept the form at its
    // four wavefronts per SIMD by waiting for every load of the trip on its own, and the headline has one such row)
    constexpr int TU = CG0 ? 2 : 4;
    for (int t = t0 + EW; t < t1; t += TU) { // the rare row with more than EW slots: the rest of its CSR list
        int q[TU], e[TU];
        double aa[TU];
#pragma unroll
        for (int u = 0; u < TU; ++u) {
            const int tt = t + u < t1 ? t + u : t1 - 1;
            q[u] = adj_col[tt];
            e[u] = adj_con[tt];
            aa[u] = adj_a[tt];
        }
        double s4[TU], v[TU][NS][W];
#pragma unroll
        for (int u = 0; u < TU; ++u) {
            s4[u] = aa[u] * wgt[e[u]];
            Slice<LG, V2, NS>::load(X + (size_t)q[u] * r, r, lane, v[u]);
        }
#pragma unroll
        for (int u = 0; u < TU; ++u) {
            const double su = t + u < t1 ? s4[u] : 0.0;
#pragma unroll
            for (int c = 0; c < NS; ++c)
#pragma unroll
                for (int w = 0; w < W; ++w) acc[c][w] += su * v[u][c][w];
        }
    }
    if (CG0) {
        const double alpha = cg0_alpha(rr, block_sum(ww, sh));
        const bool open = GATE_OPEN;
        // gated off with the solve already over and the stage reached: the average alone, from the x that is there
        const bool avg_only = !open && gt.vs != 0 && !(g.need && gt.vn == 0);
        if (open && blockIdx.x == 0 && threadIdx.x == 0 && u.shadow) *u.shadow = *u.st; // the state the convergence test starts from
        if (open && u.w_acc && gid < u.nw) {
            u.w_acc[gid] = cg_wacc(wa0, alpha, wp0);
            for (int i = gid + gridDim.x * TPB; i < u.nw; i += gridDim.x * TPB) u.w_acc[i] = cg_wacc(u.w_acc[i], alpha, u.w_p[i]);
        }
        double local = 0.0;
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            const int j0 = (lane + c * LG) * W;
            double xo[W], ro[W];
#pragma unroll
            for (int w = 0; w < W; ++w) { // p_0 = r_0: xi is both p and r, rh is x, Q = p + acc
                const CgElem e = cg_elem(alpha, xi[c][w], xi[c][w] + acc[c][w], rh[c][w], xi[c][w]);
                xo[w] = e.x; ro[w] = e.r;
                local += e.r * e.r;
            }
            if (act && j0 < r) {
                if (open) {
                    if (V2) store16(u.x, base + j0, xo[0], xo[W - 1], u.wt & WT_CG0);
                    else store8(u.x, base + j0, xo[0], u.wt & WT_CG0);
                    if (u.store_r) { // (its row of r was read at the top: xi)
                        if (V2) store16(u.r, base + j0, ro[0], ro[W - 1], u.wt & WT_CG0);
                        else store8(u.r, base + j0, ro[0], u.wt & WT_CG0);
                    }
                }
                if (u.avg_out && (open || avg_only)) {
                    double ao[W];
#pragma unroll
                    for (int w = 0; w < W; ++w) ao[w] = open ? xo[w] : rh[c][w];
                    if (V2) {
                        const double2 o = *(const double2 *)(u.avg_other + base + j0);
                        store16(u.avg_out, base + j0, cg_avg(o.x, ao[0]), cg_avg(o.y, ao[W - 1]), u.wt & WT_AVG);
                    } else {
                        store8(u.avg_out, base + j0, cg_avg(u.avg_other[base + j0], ao[0]), u.wt & WT_AVG);
                    }
                }
            }
        }
        const double t = block_sum(act ? local : 0.0, sh);
        if (open && threadIdx.x == 0) part[blockIdx.x] = t;
        return;
    }
    double local = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const int j0 = (lane + c * LG) * W;
        double v[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const double a = acc[c][w];
            if (mode == OP_CG) { v[w] = xi[c][w] + a; local += xi[c][w] * v[w]; }
            else { v[w] = rh[c][w] - (xi[c][w] + a); local += v[w] * v[w]; }
        }
        if (GATE_OPEN && act && j0 < r) {
            if (V2) store16(out, base + j0, v[0], v[W - 1], u.wt & WT_OUT);
            else store8(out, base + j0, v[0], u.wt & WT_OUT);
        }
    }
    const double t = block_sum(act ? local : 0.0, sh);
    if (GATE_OPEN && threadIdx.x == 0) part[blockIdx.x] = t;
}

// ---- The front of a CG solve for cones on the k_cw path, in ONE kernel and WITHOUT a coefficient pass before it
// (k_sval + k_spmm2<FRONT> + the k_cw of iteration 0 in the older form; LORADS_FRONT_CW=0 restores that form):
//   rhs = X_p - ((C + sum_i M1_i A_i) X)_p / rho          (lorads_admm.c:432-463)
//   r0  = rhs - (xin_p + ((sum_i w_i A_i) X)_p)            (initial residual, lorads_cgs.c:149-156; w = A(sym(xin X^T)) kept in w_uv)
//   contrib[slot] = a (r0_p . X_q) for every slot (i, p, q) of row p  -> A(sym(r0 X^T))_i = sum of its slots' contributions,
//                                                                        which is the constraint weight vector of iteration 0's
//                                                                        operator application (p_0 = r_0): k_wsum adds them up
// C X runs over the objective's own adjacency (coefficients streamed with the list); the A part runs over the row's
// (neighbour, constraint, a) slot list of k_spmm_ell, the two coefficients a M1_i and a w_i formed on the fly from the m-vectors
// (csum, b, lambda, cv, w_uv: 40 KB each at the headline, cache-resident) while the neighbour rows are already on their way.
// `wmode` = W_ADMM | W_ADMM_V (weights as if the refresh after the previous solve had been stored, see enqueue_sweep);
// rho_dual != 0: the dual update of the previous iteration has not been stored yet, the weights use lambda + rho_dual (b - csum)
// (LORADSUpdateDualVar, lorads_alg_common.c:319-332; k_wsum stores it).  Carries the sweep's reset words and a waiting
// convergence test exactly as k_sval did.
struct FrontCwArgs {
    const int *fc_ptr, *fc_col;       // objective adjacency: row -> (neighbour, c)
    const double *fc_val;
    const int *sl_ptr;                // slot list, CSR pointer (slot s of row p has the global index sl_ptr[p] + s)
    const int *sl_col, *sl_con;       // CSR (rows with more than `EW` slots finish from here)
    const double *sl_a;
    const int *ell_col, *ell_con;     // the same list in fixed width EW
    const double *ell_a;
    const int *ell_dst, *sl_dst;      // where a slot's contribution goes: constraint-major, fixed width (k_wsum reads it as a stream)
    const double *csum, *b, *lambda, *cv, *w_uv;
    const int *row_idx;               // null: constraint i is global constraint i
    DS rho, rho_dual;
    int dual_on;                      // the dual update of the previous iteration has not been stored yet: weights from lambda + rho_dual (b - csum)
    int wmode;
    double *contrib;                  // [number of slots]
    CGState *reset;
    int nreset;
    int wt;                           // WT_* bits: which outputs go through the L2 (store16 / store8)
};
__device__ __forceinline__ void front_cw_weights(const FrontCwArgs &A, double rho, double rho_dual, int i, double a, double &c1, double &c2) {
    const int g = A.row_idx ? A.row_idx[i] : i;
    const double cs0 = A.csum[g], bb = A.b[g], lam0 = A.lambda[g], cvv = A.cv[i], wu = A.w_uv[i];
    double m1;
    if (A.wmode == W_ADMM_V) { // (as weight_of: W_ADMM on top of the refresh that was not stored)
        const double cs = cs0 + (wu - cvv);
        m1 = ((cs - bb) - wu) * rho - lam0;
    } else {
        double lam = lam0;
        if (A.dual_on) { const double l = lam0 + rho_dual * bb; lam = l + (-rho_dual) * cs0; }
        m1 = ((cs0 - bb) - cvv) * rho - lam;
    }
    c1 = a * m1;
    c2 = a * wu;
}
// The closing sums of an evaluation (gated like the evaluation itself) and the result hand-over behind them, one workgroup: the
// body of k_publish_final (see k_publish for the hand-over itself) and of workgroup 0 of k_front_cw's hand-over form.  sh: 12 doubles.
struct EvalFinalArgs {
    const double *part_v, *part_d, *obj_part;
    int np, nobj;
    double *out;
    Guard g;
};
__device__ __forceinline__ void publish_final(EvalFinalArgs fa, const unsigned long long *src, int nwords, unsigned long long *dst,
                                              unsigned long long *flag, unsigned long long *seq_dev, double *sh) {
    const unsigned long long seq = *seq_dev + 1; // (requested with everything else at the top)
    // the control block's words (written by earlier kernels) are requested at the top, beside the gate and the partial sums:
    // only the three scalars formed here change, and they go to the host mirror straight from registers -- no fence and
    // re-read between the sums and the hand-over.  (fa.out is words 0..2 of src: the evaluation's scalars.)
    constexpr int PW = 4;
    unsigned long long pre[PW];
#pragma unroll
    for (int k = 0; k < PW; ++k) {
        const int i = threadIdx.x + k * TPB;
        pre[k] = __builtin_nontemporal_load(src + (i < nwords ? i : 0));
    }
    const bool live = !blocked(fa.g);
    const double *const pp[3] = {fa.part_v, fa.part_d, fa.obj_part ? fa.obj_part : fa.part_v};
    const int nn[3] = {fa.np, fa.np, fa.obj_part ? fa.nobj : 0};
    double t3[3];
    private_partials_n<3>(pp, nn, t3); // (the three sets of loads fly together)
    block_sum_n<3>(t3, sh);
    const double v = t3[0], d = t3[1], o = t3[2];
    if (live && threadIdx.x == 0) { fa.out[0] = v; fa.out[1] = d; if (fa.obj_part) fa.out[2] = o; }
    const bool own = (const double *)src == fa.out; // the words being handed over start at the evaluation's scalars
#pragma unroll
    for (int k = 0; k < PW; ++k) {
        const int i = threadIdx.x + k * TPB;
        if (i >= nwords) continue;
        unsigned long long w = pre[k];
        if (live && own) {
            if (i == 0) w = (unsigned long long)__double_as_longlong(v);
            else if (i == 1) w = (unsigned long long)__double_as_longlong(d);
            else if (i == 2 && fa.obj_part) w = (unsigned long long)__double_as_longlong(o);
        }
        dst[i] = w;
    }
    if (!own || nwords > PW * TPB) { // (a hand-over that does not start at the scalars, or a very long one: the plain way)
        __threadfence();
        __syncthreads();
        for (int i = threadIdx.x; i < nwords; i += TPB) dst[i] = __builtin_nontemporal_load(src + i);
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        *seq_dev = seq;
        __atomic_store_n(flag, seq, __ATOMIC_RELEASE);
        __threadfence_system();
    }
}
// what the hand-over form of k_front_cw (HO) hands to publish_final: it travels beside the front's own arguments
struct HandoverArgs {
    EvalFinalArgs fa;
    const unsigned long long *src;
    unsigned long long *dst;
    int nwords;
    unsigned long long *flag, *seq_dev;
    // workgroups ahead of the row workgroups: always 1, and an argument on purpose.  With the constant hipcc schedules the row body
    // of the hand-over form apart from the plain form's (154 against 158 VGPRs at <3, 16, 4>, ten more `s_waitcnt vmcnt(0)`, loads
    // of the late-operand form waited for one by one) and the U front runs 0.7 us longer (profiles/r11_front_chain_ab.txt)
    int lead;
};
struct FrontCwHoArgs : FrontCwArgs { HandoverArgs ho; };
// KC = 4 (round 3; LORADS_FRONT_LDS=0: KC = 0): the rows of the first four slots, gathered for the A part, are parked in LDS
// (32 rows x 4 slots x NS x 128 bytes per workgroup: 48 KB at NS = 3, three workgroups per CU as the registers allow anyway) and the
// second visit takes them from there -- 53 % of the rows have no more than four slots, and the second gather of a slot row was a
// quarter of the kernel's L1 misses (profiles/r03_front_cw_counters.json).  The same lanes write and read a slot's row: no barrier.
// HO (the hand-over form: the next step's U front enqueued where the step's hand-over stood, see spec_front_enqueue): the grid has
// one workgroup more.  Workgroup 0 is the hand-over of k_publish_final (publish_final under its own gate in A.ho.fa) and returns:
// it is dispatched first, so the host sees the flag at the head of the front.  Workgroup b > 0 is row workgroup b - 1.  Nobody waits
// for anybody: the row workgroups read nothing the hand-over writes (the three scalars, the mirror, seq_dev) and write scratch alone.
// FC (LORADS_FRONT_CHAIN; either bit leaves the arithmetic as it is: the same products added in the same order):
//   FC_RAW   the neighbour rows are loaded without the mask of the slice beyond r (Slice::load_raw: no v_cndmask per loaded
//            register, no masked copy beside the loaded one); that slice of the right-hand side and of r0 is masked once, in the
//            epilogue, so every sum gets the same +0.0 from it as before
//   FC_LATE  the row's own operands (X_p, xin_p: nothing reads them before the epilogue) are requested behind the first slot batch
//            and arrive under the waits of the batches that follow -- 8 NS registers free while the objective is walked
template <int NB, class SL, bool RAW = false, int NS, int W>
__device__ __forceinline__ void front_gather(const double *__restrict__ X, int r, int lane, int q, int u0, double (&v)[NB][NS][W]) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if constexpr (RAW) SL::load_raw(X + (size_t)__shfl(q, u0 + u, 8) * r, r, lane, v[u]);
        else SL::load(X + (size_t)__shfl(q, u0 + u, 8) * r, r, lane, v[u]);
    }
}
template <int NB, int NS, int W>
__device__ __forceinline__ void front_fma2(double k1, double k2, int u0, const double (&v)[NB][NS][W], double (&acc)[NS][W], double (&acc2)[NS][W]) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const double s1 = __shfl(k1, u0 + u, 8), s2 = __shfl(k2, u0 + u, 8);
#pragma unroll
        for (int c = 0; c < NS; ++c)
#pragma unroll
            for (int w = 0; w < W; ++w) { acc[c][w] += s1 * v[u][c][w]; acc2[c][w] += s2 * v[u][c][w]; }
    }
}
// lane u0 + u of the group keeps r0 . v[u] in `mine`
template <int NB, int NS, int W>
__device__ __forceinline__ void front_dots(const double (&r0)[NS][W], const double (&v)[NB][NS][W], int u0, int l8, double &mine) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        double dsum = 0.0;
#pragma unroll
        for (int c = 0; c < NS; ++c)
#pragma unroll
            for (int w = 0; w < W; ++w) dsum += r0[c][w] * v[u][c][w];
        dsum = group_sum<8>(dsum);
        mine = l8 == u0 + u ? dsum : mine;
    }
}
template <int NS, int EW, int KC = 0, bool HO = false, int FC = 0>
__global__ __launch_bounds__(TPB) void k_front_cw(int n, int rpw, std::conditional_t<HO, FrontCwHoArgs, FrontCwArgs> A,
                                                  const double *__restrict__ X, int r,
                                                  const double *__restrict__ xin, double *__restrict__ out,
                                                  double *__restrict__ rhs_out, double *__restrict__ part,
                                                  double *__restrict__ part_b, Guard g, Deferred d) {
    constexpr int LG = 8, W = 2, NH = EW / 8;
    constexpr bool RAW = (FC & FC_RAW) != 0, LATE = (FC & FC_LATE) != 0;
    using SL = Slice<LG, true, NS>;
    __shared__ double sh[HO ? 12 : 8];
    extern __shared__ __attribute__((aligned(16))) double2 slotc[]; // [32 rows][KC slots][NS][8 lanes]
    unsigned wg = blockIdx.x; // the row workgroup
    if constexpr (HO) {
        if (blockIdx.x < (unsigned)A.ho.lead) { // (lead = 1, see HandoverArgs)
            if (blockIdx.x == 0) publish_final(A.ho.fa, A.ho.src, A.ho.nwords, A.ho.dst, A.ho.flag, A.ho.seq_dev, sh);
            return;
        }
        wg = blockIdx.x - A.ho.lead;
    }
    if (A.reset && wg == 0 && threadIdx.x < A.nreset) A.reset[threadIdx.x].done = 0;
    const Gate gt = gate_load(g);
    const double rho = dsv(A.rho), rho_dual = A.dual_on ? dsv(A.rho_dual) : 0.0;
    DefPriv dv{};
    if (d.st) dv = deferred_private(d);
    // rpw rows per workgroup (row_deal): a lane group beyond rpw is a row past n in every sense (the LDS park keeps its 32 places)
    const int grp = threadIdx.x / LG, row = wg * rpw + grp, lane = threadIdx.x % LG, l8 = lane & 7;
    const bool act = grp < rpw && row < n;
    const int rowc = act ? row : 0;
    const size_t base = (size_t)rowc * r;
    // level 1: the two lists' heads, this lane's slots, the row's own operands
    const int c0 = A.fc_ptr[rowc], c1e = act ? A.fc_ptr[rowc + 1] : c0;
    const int a0 = A.sl_ptr[rowc], a1r = A.sl_ptr[rowc + 1];
    const int a1 = act ? a1r : a0; // (an inactive group stays out of row 0's CSR tails, in both visits)
    const int cnt = a1 - a0;
    const size_t eb = (size_t)rowc * EW + l8;
    int qc[NH], kc[NH], dc[NH];
    double ac[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) { qc[h] = A.ell_col[eb + 8 * h]; kc[h] = A.ell_con[eb + 8 * h]; ac[h] = A.ell_a[eb + 8 * h]; dc[h] = A.ell_dst[eb + 8 * h]; }
    int tn = c0 + l8, tc = tn < c1e ? tn : (c1e > 0 ? c1e - 1 : 0);
    int qn = A.fc_col[tc];
    double svn = A.fc_val[tc];
    double xi[NS][W], rh[NS][W];
    if constexpr (!LATE) {
        SL::load(X + base, r, lane, xi);
        SL::load(xin + base, r, lane, rh);
    }
    // level 2 (beside the first neighbour rows): this lane's slot coefficients from the m-vectors
    double k1[NH], k2[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        front_cw_weights(A, rho, rho_dual, kc[h], ac[h], k1[h], k2[h]);
        const bool mine = l8 + 8 * h < cnt; // (padding slots name constraint 0 with a = 0: masked, whatever its weights are)
        k1[h] = mine ? k1[h] : 0.0;
        k2[h] = mine ? k2[h] : 0.0;
    }
    double acc[NS][W], acc2[NS][W];
#pragma unroll
    for (int c = 0; c < NS; ++c)
#pragma unroll
        for (int w = 0; w < W; ++w) { acc[c][w] = 0.0; acc2[c][w] = 0.0; }
    // ---- C X: eight list slots per trip (lane l8 holds slot t + l8), four neighbour rows in flight
    for (int t = c0; t < c1e; t += 8) {
        const int q = qn;
        const double sv = t + l8 < c1e ? svn : 0.0;
        tn = t + 8 + l8;
        tc = tn < c1e ? tn : c1e - 1;
        qn = A.fc_col[tc];
        svn = A.fc_val[tc];
#pragma unroll
        for (int u0 = 0; u0 < 8; u0 += 4) {
            if (u0 == 0 || t + u0 < c1e) {
                double v[4][NS][W];
                front_gather<4, SL, RAW>(X, r, lane, q, u0, v);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double a1c = __shfl(sv, u0 + u, 8);
#pragma unroll
                    for (int c = 0; c < NS; ++c)
#pragma unroll
                        for (int w = 0; w < W; ++w) acc[c][w] += a1c * v[u][c][w];
                }
            }
        }
    }
    // ---- the A part: the row's slots, two coefficients per slot
    { // slots 0..3 (every row: padding names the row itself, coefficient 0)
        double v[4][NS][W];
        front_gather<4, SL, RAW>(X, r, lane, qc[0], 0, v);
        if constexpr (LATE) {
            SL::load(X + base, r, lane, xi);
            SL::load(xin + base, r, lane, rh);
        }
        if constexpr (KC > 0) { // park the rows for the second visit
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int c = 0; c < NS; ++c)
                    slotc[(((threadIdx.x >> 3) * KC + u) * NS + c) * 8 + l8] = make_double2(v[u][c][0], v[u][c][1]);
        }
        front_fma2<4>(k1[0], k2[0], 0, v, acc, acc2);
    }
    if (cnt > 4) { // slots 4..7
        double v[4][NS][W];
        front_gather<4, SL, RAW>(X, r, lane, qc[0], 4, v);
        front_fma2<4>(k1[0], k2[0], 4, v, acc, acc2);
    }
#pragma unroll
    for (int h = 1; h < NH; ++h) {
        if (cnt > 8 * h) {
#pragma unroll
            for (int u0 = 0; u0 < 8; u0 += 4) {
                if (u0 > 0 && cnt <= 8 * h + u0) continue;
                double v[4][NS][W];
                front_gather<4, SL, RAW>(X, r, lane, qc[h], u0, v);
                front_fma2<4>(k1[h], k2[h], u0, v, acc, acc2);
            }
        }
    }
    for (int t = a0 + EW; t < a1; ++t) { // the rare row with more than EW slots: the rest of its CSR list, one slot at a time
        double s1, s2, v[NS][W];
        front_cw_weights(A, rho, rho_dual, A.sl_con[t], A.sl_a[t], s1, s2);
        if constexpr (RAW) SL::load_raw(X + (size_t)A.sl_col[t] * r, r, lane, v);
        else SL::load(X + (size_t)A.sl_col[t] * r, r, lane, v);
#pragma unroll
        for (int c = 0; c < NS; ++c)
#pragma unroll
            for (int w = 0; w < W; ++w) { acc[c][w] += s1 * v[c][w]; acc2[c][w] += s2 * v[c][w]; }
    }
    // ---- epilogue: right-hand side, initial residual, their partial norms
    const bool live = d.st ? !blocked_after(g, d, finish_deferred(d, dv, sh).done) : GATE_OPEN;
    double r0[NS][W];
    double local = 0.0, local_b = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const int j0 = (lane + c * LG) * W;
        double vb[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            vb[w] = xi[c][w] - acc[c][w] / rho;
            r0[c][w] = vb[w] - (rh[c][w] + acc2[c][w]);
            if constexpr (RAW) { // (the neighbour rows came unmasked: a slice beyond r is masked here, once)
                vb[w] = j0 < r ? vb[w] : 0.0;
                r0[c][w] = j0 < r ? r0[c][w] : 0.0;
            }
            local_b += fabs(vb[w]);
            local += r0[c][w] * r0[c][w];
        }
        if (live && act && j0 < r) {
            store16(out, base + j0, r0[c][0], r0[c][1], A.wt & WT_R0);
            store16(rhs_out, base + j0, vb[0], vb[1], A.wt & WT_RHS);
        }
    }
    // ---- second visit of the row's slots: contributions of the constraint values of (r0, X)
    // (A.contrib == null -- measurement only, lorads_hip_ubench -- leaves the visit out: what it costs is the difference)
    // (inactive groups are clamped to row 0: their lanes must not write row 0's tail contributions, which row 0's own lanes
    // write -- a1 = a0 for them, see above)
    const int cnt2 = A.contrib ? cnt : 0;
    const int a1b = A.contrib ? a1 : a0;
    if (cnt2 > 0) { // slots 0..7 (a lane's contribution does not depend on the order its neighbours' are formed in)
        double mine = 0.0;
        if constexpr (KC > 0) { // slots 0..3 parked by the first visit
            double v[4][NS][W];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int c = 0; c < NS; ++c) {
                    const double2 t = slotc[(((threadIdx.x >> 3) * KC + u) * NS + c) * 8 + l8];
                    v[u][c][0] = t.x; v[u][c][1] = t.y;
                }
            front_dots<4>(r0, v, 0, l8, mine);
            if (cnt2 > 4) {
                front_gather<4, SL, RAW>(X, r, lane, qc[0], 4, v);
                front_dots<4>(r0, v, 4, l8, mine);
            }
        } else {
#pragma unroll
            for (int u0 = 0; u0 < 8; u0 += 4) {
                if (u0 > 0 && cnt2 <= u0) continue;
                double v[4][NS][W];
                front_gather<4, SL, RAW>(X, r, lane, qc[0], u0, v);
                front_dots<4>(r0, v, u0, l8, mine);
            }
        }
        if (live && l8 < cnt2) store8(A.contrib, (size_t)dc[0], ac[0] * mine, A.wt & WT_CONTRIB);
    }
#pragma unroll
    for (int h = 1; h < NH; ++h) {
        if (cnt2 > 8 * h) {
            double mine = 0.0;
#pragma unroll
            for (int u0 = 0; u0 < 8; u0 += 4) {
                if (u0 > 0 && cnt2 <= 8 * h + u0) continue;
                double v[4][NS][W];
                front_gather<4, SL, RAW>(X, r, lane, qc[h], u0, v);
                front_dots<4>(r0, v, u0, l8, mine);
            }
            if (live && l8 + 8 * h < cnt2) store8(A.contrib, (size_t)dc[h], ac[h] * mine, A.wt & WT_CONTRIB);
        }
    }
    for (int t = a0 + EW; t < a1b; ++t) {
        double v[NS][W], dsum = 0.0;
        SL::load(X + (size_t)A.sl_col[t] * r, r, lane, v);
#pragma unroll
        for (int c = 0; c < NS; ++c)
#pragma unroll
            for (int w = 0; w < W; ++w) dsum += r0[c][w] * v[c][w];
        dsum = group_sum<LG>(dsum);
        if (live && l8 == 0) store8(A.contrib, (size_t)A.sl_dst[t], A.sl_a[t] * dsum, A.wt & WT_CONTRIB);
    }
    double two[2] = {act ? local : 0.0, act ? local_b : 0.0};
    block_sum_n<2>(two, sh);
    if (live && threadIdx.x == 0) { part[wg] = two[0]; part_b[wg] = two[1]; }
}

// w_i = sum of the contributions k_front_cw left for constraint i's slots: constraint-major, fixed width cw (padding holds 0),
// 8 lanes per constraint, lane l adds entries l, l + 8, ... in that order and the lanes are combined by the same butterfly
// every time (deterministic).  The first kernel of iteration 0: the solve's start rides on it (InitArgs, as on k_cw), and --
// first solve of a sweep -- it stores the multipliers of the dual update the front has already used (rho_dual != 0): all m_all of them.
// part_ww != null: workgroup b also writes part_ww[b] = sum of w_i^2 over its constraints (fixed order), see Cg0Args.
__global__ __launch_bounds__(TPB) void k_wsum(int nrow, int cw, const double *__restrict__ contrib, double *__restrict__ w_out, Guard g,
                                              InitArgs ia, int dual_on, DS rho_dual_s, int m_all,
                                              const double *__restrict__ b, const double *__restrict__ csum,
                                              double *__restrict__ lambda, double *__restrict__ part_ww = nullptr,
                                              CGState *reset = nullptr, int nreset = 0) {
    __shared__ double sh[8];
    // (behind a front that was enqueued ahead of its step, see spec_front_enqueue: the sweep's reset words, which that front left alone)
    if (reset && blockIdx.x == 0 && threadIdx.x < nreset) reset[threadIdx.x].done = 0;
    const Gate gt = gate_load(ia.st ? Guard{nullptr, g.need} : g);
    double iv[2] = {0.0, 0.0};
    if (ia.st) init_private(ia, iv);
    const int i = (blockIdx.x * TPB + threadIdx.x) / 8, lane = threadIdx.x & 7;
    const bool act = i < nrow;
    const int ic = act ? i : 0;
    const double *cp = contrib + (size_t)ic * cw;
    double s = 0.0;
    for (int t = lane; t < cw; t += 32) { // (four loads per trip in flight)
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = cp[t + 8 * u < cw ? t + 8 * u : lane];
#pragma unroll
        for (int u = 0; u < 4; ++u) s += t + 8 * u < cw ? v[u] : 0.0;
    }
    s = group_sum<8>(s);
    if (dual_on) { // (ungated: the front has used these multipliers whatever this solve does)
        const double rho_dual = dsv(rho_dual_s);
        // every entry of the (replicated) multiplier vector, not just this cone's constraints: k_dual_update's pass
        for (int gi = blockIdx.x * TPB + threadIdx.x; gi < m_all; gi += gridDim.x * TPB) {
            const double l = lambda[gi] + rho_dual * b[gi];
            lambda[gi] = l + (-rho_dual) * csum[gi];
        }
    }
    const bool live = ia.st ? finish_init(ia, !(g.need && gt.vn == 0), iv, sh) == 0 : GATE_OPEN;
    if (live && act && lane == 0) w_out[i] = s;
    if (part_ww) { // this workgroup's constraints' share of ||w||^2, for alpha of iteration 0 (cg0_alpha)
        const double t = block_sum(act && lane == 0 ? s * s : 0.0, sh);
        if (live && threadIdx.x == 0) part_ww[blockIdx.x] = t;
    }
}

// Max-Cut-type cones (every A_i = a_i e_p e_p^T): the whole operator is row-local,
//   out_p = x_p + g_p (x_p . V_p) V_p,  g_p = sum_i a_i^2  -> one pass over x and V
// DirArgs (kind != 0): the operator is row-local, so the direction update that precedes it in a CG iteration
// (lorads_cgs.c:217-228: p = r + beta p; after a restart p = 2 r) is done here, row by row, instead of by a k_cg_dir launch:
// the row of p is formed, stored, and used as the operator's input.  beta comes from the carried convergence test or from
// the state; after a restart workgroup 0 also writes the restart's two scalars (rr = ||true residual||^2, beta = 1).
// Lockstep sweep (tile_cone != null): workgroup b works on rows of cone tile_cone[b] (row tiles never straddle a cone), the
// state is st[2 cone + half], and a cone whose solve has finished keeps its direction (as k_cg_dir_seg leaves it alone).
__device__ __forceinline__ double wave_partials(const double *part, int n); // (defined with the lockstep sweep's kernels)
struct DirArgs {
    int kind;            // 0 | DIR_BETA | DIR_RESTART
    const double *rvec;  // r
    double *pvec;        // p (in: old direction, out: new direction)
    CGState *st;
    const double *rs_part; // DIR_RESTART, one cone: partials of the true residual's norm
    int rs_np;
    const int *tile_cone;
    int half;
    // Lockstep sweep, seg_part != null: the convergence test of the iteration BEFORE this application (k_cg_check_seg's CHK_ITER for
    // iteration seg_k - 1) rides here.  Every workgroup redoes its own cone's test from the update's partial sums (same sums, same
    // order: one wavefront's wave_partials) and takes beta and "done" from it; the cone's first row tile writes the state.  The old
    // r.r is read from slot (seg_k - 1) & 1, the new one goes to slot seg_k & 1 (see SegArgs): no workgroup reads a word another
    // one writes, except `done` -- and a reader that sees the new `done` skips the cone exactly as its own test would have told it.
    const double *seg_part;
    const int4 *seg_info; // per row tile: {cone, its chunk partials [y, z), first tile of the cone?}
    double *seg_rr_alt;
    DS seg_tol, seg_maxit;
    int seg_k;
    // Lockstep sweep, kind == 0 with seg_part != null: that test alone rides (the application is the k % 20 == 0 restart's residual,
    // which comes right behind iteration k's test; a cone the test finishes needs no residual).
    // Lockstep sweep, DIR_RESTART with rs_seg != null: the restart's two scalars (k_cg_check_seg's CHK_RESTART: r.r = ||true residual||^2
    // from the residual pass's row-tile partials, beta = 1) are written by the cone's first row tile -- nobody in this kernel reads
    // them (p = 2 r after a restart), the update that follows does.  row0 / rpw: the cone's row tiles.
    const double *rs_seg;
    const int *seg_row0;
    int seg_rpw;
    // Lockstep sweep, iteration 0's application (kind == 0) with init_rr != null: the start of every cone's solve (k_cg_init_seg) rides
    // here.  Every workgroup sums its own cone's partials of ||r_0||^2 and ||rhs||_1 (the front's row-tile partials: same sums, one
    // wavefront's wave_partials) and skips a cone that is converged at once; the cone's first row tile writes the state, workgroup 0
    // re-arms the phase words.  Nothing of the old state is read, and the phase's own skip word -- still set from the previous ADMM
    // iteration -- is not looked at (as with a carried start of a single cone, InitArgs).
    const double *init_rr, *init_b;
    DS init_tol;
    int *init_pd;
};
template <int LG, bool V2, int NS>
__global__ __launch_bounds__(TPB) void k_op_diag(int n, const double *__restrict__ gd, const double *__restrict__ V, int r,
                                                 int mode, const double *xin, const double *__restrict__ rhs,
                                                 double *__restrict__ out, double *__restrict__ part, Guard g, Carry cy,
                                                 DirArgs da, double *__restrict__ dot_out) {
    __shared__ double sh[8];
    // a carried solve start (iteration 0's operator) or convergence test (the k = 0 restart's residual, or the test in
    // front of a fused direction update) replaces the solve's own gate word: its loads go out first
    const Gate gt = gate_load((cy.ia.st || da.init_rr) ? Guard{nullptr, g.need} : g);
    double iv[2] = {0.0, 0.0};
    DefPriv dv{};
    if (cy.ia.st) init_private(cy.ia, iv);
    if (cy.d.st) dv = deferred_private(cy.d);
    CGState *stp = da.st;
    bool dir_on = da.kind != 0;
    bool seg_carried = false;
    double beta_seg = 1.0;
    if (da.init_rr) { // the start of this row tile's cone (see DirArgs)
        const int cone = da.tile_cone[blockIdx.x];
        const int tb = da.seg_row0[cone] / da.seg_rpw, te = da.seg_row0[cone + 1] / da.seg_rpw;
        const double a = wave_partials(da.init_rr + tb, te - tb), b = wave_partials(da.init_b + tb, te - tb);
        const int done = sqrt(a) / b < dsv(da.init_tol) ? 2 : 0;
        if (threadIdx.x == 0 && !gate_blocked(g, gt)) {
            if ((int)blockIdx.x == tb) {
                CGState *st = da.st + 2 * cone + da.half;
                st->rr = a; st->bnorm = b; st->beta = 0.0; st->iter = 0; st->nan = 0; st->pad = 1; // pad = "started"
                st->done = done;
                if (da.half == 0) { da.st[2 * cone + 1].done = 0; da.st[2 * cone + 1].pad = 0; }
            }
            if (blockIdx.x == 0) { // (k_cg_init_seg publishes "every cone converged at once" here; the per-cone words say the same to every kernel that follows)
                if (da.half == 0) da.init_pd[1] = 0;
                da.init_pd[da.half] = 0;
            }
        }
        if (done) return; // converged at once: nothing of this application is ever read
    }
    if (da.tile_cone && da.seg_part) { // the previous iteration's convergence test of this cone (see DirArgs)
        seg_carried = true;
        const int4 ti = da.seg_info[blockIdx.x]; // {cone, first and one-past-last chunk partial of the cone, "first row tile of the cone"}
        stp = da.st + 2 * ti.x + da.half;
        const int done0 = stp->done, it = stp->iter;
        const double bn = stp->bnorm;
        const int idx = 2 * ti.x + da.half;
        const double rr_old = ((da.seg_k - 1) & 1) ? da.seg_rr_alt[idx] : stp->rr;
        const double a = wave_partials(da.seg_part + ti.y, ti.z - ti.y);
        int done_new = done0;
        if (done0 == 0) {
            if (sqrt(a) / bn < dsv(da.seg_tol)) done_new = 1;
            else if (da.seg_k >= (int)dsv(da.seg_maxit)) done_new = 3;
        }
        beta_seg = a / rr_old;
        dir_on = done_new == 0;
        if (ti.w && threadIdx.x == 0 && done0 == 0 && !gate_blocked(g, gt)) { // (as k_cg_check_seg: a gated phase tests nothing)
            stp->iter = it + 1;
            if (a != a) stp->nan = 1;
            stp->beta = beta_seg;
            if (da.seg_k & 1) da.seg_rr_alt[idx] = a;
            else stp->rr = a;
            if (done_new) stp->done = done_new;
        }
        if (!dir_on) return; // a finished cone: nothing of this application is ever read -- its rows are not even fetched
    } else if (da.kind && da.tile_cone) {
        const int cone = da.tile_cone[blockIdx.x];
        stp = da.st + 2 * cone + da.half;
        dir_on = stp->done == 0;
        if (da.kind == DIR_RESTART && da.rs_seg) {
            const int tb = da.seg_row0[cone] / da.seg_rpw, te = da.seg_row0[cone + 1] / da.seg_rpw;
            if ((int)blockIdx.x == tb && dir_on) { // the cone's first row tile: CHK_RESTART of this cone (same sum: one wavefront's wave_partials)
                const double a = wave_partials(da.rs_seg + tb, te - tb);
                if (threadIdx.x == 0 && !gate_blocked(g, gt)) {
                    if (da.seg_k & 1) da.seg_rr_alt[2 * cone + da.half] = a;
                    else stp->rr = a;
                    stp->beta = 1.0;
                }
            }
        }
    }
    const double beta_plain = (da.kind == DIR_BETA && !cy.d.st && !seg_carried) ? stp->beta : 1.0;
    double a_rs = 0.0;
    if (da.kind == DIR_RESTART && da.rs_part && blockIdx.x == 0) a_rs = sum_partials(da.rs_part, da.rs_np, sh);
    constexpr int W = V2 ? 2 : 1;
    const int row = (blockIdx.x * TPB + threadIdx.x) / LG, lane = threadIdx.x % LG;
    const bool act = row < n;
    const int rowc = act ? row : 0;
    const size_t base = (size_t)rowc * r;
    double xv[NS][W], vv[NS][W], rh[NS][W], po[NS][W];
    Slice<LG, V2, NS>::load((da.kind ? da.rvec : xin) + base, r, lane, xv); // (fused direction: the row of r)
    Slice<LG, V2, NS>::load(V + base, r, lane, vv);
    if (mode == OP_RES) Slice<LG, V2, NS>::load(rhs + base, r, lane, rh);
    if (da.kind == DIR_BETA || (da.kind && da.tile_cone)) Slice<LG, V2, NS>::load(da.pvec + base, r, lane, po);
    const double gr = gd[rowc];
    bool live;
    double beta = seg_carried ? beta_seg : beta_plain;
    if (cy.ia.st) live = finish_init(cy.ia, !(g.need && gt.vn == 0), iv, sh) == 0;
    else if (cy.d.st) {
        const DefOut o = finish_deferred(cy.d, dv, sh);
        live = !blocked_after(g, cy.d, o.done);
        beta = o.beta;
    } else live = GATE_OPEN;
    if (da.kind) { // this row of the new direction: formed, stored, and the operator's input
        if (live && da.kind == DIR_RESTART && da.rs_part && blockIdx.x == 0 && threadIdx.x == 0) { da.st->rr = a_rs; da.st->beta = 1.0; }
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            const int j0 = (lane + c * LG) * W;
#pragma unroll
            for (int w = 0; w < W; ++w)
                xv[c][w] = !dir_on ? po[c][w] : da.kind == DIR_RESTART ? xv[c][w] + xv[c][w] : fma(beta, po[c][w], xv[c][w]); // (as k_cg_dir)
            if (live && dir_on && act && j0 < r) {
                if (V2) *(double2 *)(da.pvec + base + j0) = make_double2(xv[c][0], xv[c][W - 1]);
                else da.pvec[base + j0] = xv[c][0];
            }
        }
    }
    double d = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c)
#pragma unroll
        for (int w = 0; w < W; ++w) d += xv[c][w] * vv[c][w];
    d = group_sum<LG>(d);
    // the row's x . V itself (may be null): for x = a CG direction the increment of U_p . V_p per unit step, for x = the
    // solve variable that dot itself -- what the constraint refresh of a Max-Cut cone is made of (constr_by_recurrence)
    if (dot_out && live && act && lane == 0) dot_out[rowc] = d;
    d *= gr;
    double local = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const int j0 = (lane + c * LG) * W;
        double v[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            v[w] = xv[c][w] + d * vv[c][w];
            if (mode == OP_CG) local += xv[c][w] * v[w];
            else { v[w] = rh[c][w] - v[w]; local += v[w] * v[w]; }
        }
        if (live && act && j0 < r) {
            if (V2) *(double2 *)(out + base + j0) = make_double2(v[0], v[W - 1]);
            else out[base + j0] = v[0];
        }
    }
    const double t = block_sum(act ? local : 0.0, sh);
    if (live && threadIdx.x == 0) part[blockIdx.x] = t;
}

// Cones whose constraints each hold ONE pattern entry (matrix completion: A_k = a (e_i e_j^T + e_j e_i^T)/2 ...):
// w_i = a_i T_e and S_e = (sum_i a_i^2) T_e = ge_e T_e stay entry-local, so the whole operator is one row-centric pass
//   out_p = x_p + sum_{(q,e) adjacent to p} ge_e (x_p.V_q + x_q.V_p) V_q        (q = p: ge_e (x_p.V_p) V_p)
// -- no T, no S, no second and third kernel.  Every entry is visited from both of its rows (the pair dot is formed
// twice); what it saves is two launches and the 4-rows-per-entry gather of the pair-dot kernel.
template <int LG, bool V2, int NS>
__global__ __launch_bounds__(TPB) void k_op_entry(int n, const int *__restrict__ adj_ptr, const int *__restrict__ adj_col,
                                                  const int *__restrict__ adj_e, const double *__restrict__ ge,
                                                  const double *__restrict__ V, int r, int mode, const double *__restrict__ xin,
                                                  const double *__restrict__ rhs, double *__restrict__ out,
                                                  double *__restrict__ part, Guard g) {
    __shared__ double sh[4];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    constexpr int W = V2 ? 2 : 1;
    const int row = (blockIdx.x * TPB + threadIdx.x) / LG, lane = threadIdx.x % LG;
    const bool act = row < n;
    const int rowc = act ? row : 0;
    const size_t base = (size_t)rowc * r;
    const int t0 = adj_ptr[rowc], t1 = act ? adj_ptr[rowc + 1] : t0;
    double xp[NS][W], vp[NS][W], rh[NS][W], acc[NS][W];
    Slice<LG, V2, NS>::load(xin + base, r, lane, xp);
    Slice<LG, V2, NS>::load(V + base, r, lane, vp);
    if (mode == OP_RES) Slice<LG, V2, NS>::load(rhs + base, r, lane, rh);
#pragma unroll
    for (int c = 0; c < NS; ++c)
#pragma unroll
        for (int w = 0; w < W; ++w) acc[c][w] = 0.0;
    for (int t = t0; t < t1; t += 2) { // two neighbours per trip: 4 row gathers in flight
        int q[2], e[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int tt = t + u < t1 ? t + u : t1 - 1;
            q[u] = adj_col[tt];
            e[u] = adj_e[tt];
        }
        double gc[2], xq[2][NS][W], vq[2][NS][W];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            gc[u] = ge[e[u]];
            Slice<LG, V2, NS>::load(xin + (size_t)q[u] * r, r, lane, xq[u]);
            Slice<LG, V2, NS>::load(V + (size_t)q[u] * r, r, lane, vq[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            double s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int c = 0; c < NS; ++c)
#pragma unroll
                for (int w = 0; w < W; ++w) { s1 += xp[c][w] * vq[u][c][w]; s2 += xq[u][c][w] * vp[c][w]; }
            double td = q[u] == rowc ? s1 : s1 + s2;
            td = group_sum<LG>(td);
            const double su = t + u < t1 ? gc[u] * td : 0.0;
#pragma unroll
            for (int c = 0; c < NS; ++c)
#pragma unroll
                for (int w = 0; w < W; ++w) acc[c][w] += su * vq[u][c][w];
        }
    }
    double local = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const int j0 = (lane + c * LG) * W;
        double v[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            v[w] = xp[c][w] + acc[c][w];
            if (mode == OP_CG) local += xp[c][w] * v[w];
            else { v[w] = rh[c][w] - v[w]; local += v[w] * v[w]; }
        }
        if (GATE_OPEN && act && j0 < r) {
            if (V2) *(double2 *)(out + base + j0) = make_double2(v[0], v[W - 1]);
            else out[base + j0] = v[0];
        }
    }
    const double t = block_sum(act ? local : 0.0, sh);
    if (GATE_OPEN && threadIdx.x == 0) part[blockIdx.x] = t;
}

// The same operator when the entry graph is BIPARTITE (matrix completion: every entry couples a row of the left factor block with
// a row of the right one).  k_op_entry forms every entry's pair dot twice, once from each of its rows: 2 gathered rows per slot, 4
// per entry.  Here the rows of one colour (SIDE 0) do that work once -- gather x_q and V_q, form su = ge (x_p.V_q + x_q.V_p), use
// it AND leave it in we[e] -- and the rows of the other colour (SIDE 1, a second launch) only gather V_p and read su: 3 gathered
// rows per entry instead of 4, nothing streamed twice (every row belongs to exactly one launch).  Rows come from a list
// (rows[0..nrows)); diagonal entries are row-local on either side.  Partial sums: part[part0 + workgroup].
template <int LG, bool V2, int NS, int SIDE>
__global__ __launch_bounds__(TPB) void k_op_entry_bip(int nrows, const int *__restrict__ rows, const int *__restrict__ adj_ptr,
                                                      const int *__restrict__ adj_col, const int *__restrict__ adj_e,
                                                      const double *__restrict__ ge, double *__restrict__ we,
                                                      const double *__restrict__ V, int r, int mode, const double *__restrict__ xin,
                                                      const double *__restrict__ rhs, double *__restrict__ out,
                                                      double *__restrict__ part, int part0, Guard g) {
    __shared__ double sh[4];
    const Gate gt = gate_load(g);
    constexpr int W = V2 ? 2 : 1;
    const int idx = (blockIdx.x * TPB + threadIdx.x) / LG, lane = threadIdx.x % LG;
    const bool act = idx < nrows;
    const int rowc = rows[act ? idx : 0];
    const size_t base = (size_t)rowc * r;
    const int t0 = adj_ptr[rowc], t1 = act ? adj_ptr[rowc + 1] : t0;
    double xp[NS][W], vp[NS][W], rh[NS][W], acc[NS][W];
    Slice<LG, V2, NS>::load(xin + base, r, lane, xp);
    if (SIDE == 0) Slice<LG, V2, NS>::load(V + base, r, lane, vp); // (SIDE 1 meets its own V row only as the "neighbour" of a diagonal entry)
    if (mode == OP_RES) Slice<LG, V2, NS>::load(rhs + base, r, lane, rh);
#pragma unroll
    for (int c = 0; c < NS; ++c)
#pragma unroll
        for (int w = 0; w < W; ++w) acc[c][w] = 0.0;
    const bool open = GATE_OPEN;
    constexpr int TR = 2; // neighbours per trip (four on SIDE 1, i.e. four row gathers in flight there too, was no faster: 68.3 against 66.7 us)
    for (int t = t0; t < t1; t += TR) {
        int q[TR], e[TR];
#pragma unroll
        for (int u = 0; u < TR; ++u) {
            const int tt = t + u < t1 ? t + u : t1 - 1;
            q[u] = adj_col[tt];
            e[u] = adj_e[tt];
        }
        double gc[TR], xq[SIDE == 0 ? TR : 1][NS][W], vq[TR][NS][W];
#pragma unroll
        for (int u = 0; u < TR; ++u) {
            // SIDE 1: the other colour has left ge (x_p.V_q + x_q.V_p) in we[e]; a diagonal entry's is formed here
            gc[u] = (SIDE == 1 && q[u] != rowc) ? we[e[u]] : ge[e[u]];
            if (SIDE == 0) Slice<LG, V2, NS>::load(xin + (size_t)q[u] * r, r, lane, xq[SIDE == 0 ? u : 0]);
            Slice<LG, V2, NS>::load(V + (size_t)q[u] * r, r, lane, vq[u]);
        }
#pragma unroll
        for (int u = 0; u < TR; ++u) {
            double su;
            if (SIDE == 0 || q[u] == rowc) {
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int c = 0; c < NS; ++c)
#pragma unroll
                    for (int w = 0; w < W; ++w) {
                        s1 += xp[c][w] * vq[u][c][w];
                        if (SIDE == 0) s2 += xq[SIDE == 0 ? u : 0][c][w] * vp[c][w];
                    }
                double td = q[u] == rowc ? s1 : s1 + s2;
                td = group_sum<LG>(td);
                su = gc[u] * td;
                if (SIDE == 0 && open && act && lane == 0 && t + u < t1 && q[u] != rowc) we[e[u]] = su;
            } else {
                su = gc[u];
            }
            if (!(t + u < t1)) su = 0.0;
#pragma unroll
            for (int c = 0; c < NS; ++c)
#pragma unroll
                for (int w = 0; w < W; ++w) acc[c][w] += su * vq[u][c][w];
        }
    }
    double local = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const int j0 = (lane + c * LG) * W;
        double v[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            v[w] = xp[c][w] + acc[c][w];
            if (mode == OP_CG) local += xp[c][w] * v[w];
            else { v[w] = rh[c][w] - v[w]; local += v[w] * v[w]; }
        }
        if (open && act && j0 < r) {
            if (V2) *(double2 *)(out + base + j0) = make_double2(v[0], v[W - 1]);
            else out[base + j0] = v[0];
        }
    }
    const double t = block_sum(act ? local : 0.0, sh);
    if (open && threadIdx.x == 0) part[part0 + blockIdx.x] = t;
}

// Dense objective matrix: W = C X with C dense symmetric (n_pad x n_pad row-major, zero padded) and X n x r
// row-major -- the reference's dense branch (unpack + dsymm, lorads_sdp_data.c:646-671) -- on the FP64 matrix
// cores: v_mfma_f64_16x16x4_f64, split-K over workgroups so that the grid fills 256 CUs, the partial results summed in a fixed
// order by k_sum_slabs.  (Round 1's form -- C as the MFMA A operand, 64 rows of C per workgroup, X staged through LDS: 2.2 TB/s at
// n = 4096 -- lost to the form below in round 2 and was retired with its switch LORADS_DENSE_B in round 4.)
typedef double v4f64 __attribute__((ext_vector_type(4)));
// W = C X for a dense symmetric C: C is read as the MFMA **B** operand.
// W^T = X^T C for symmetric C, so D[m = column j of X][n = row i of W] = sum_k X[k][j] C[k][i]: the lanes that supply
// B[k][n] for one k are 16 consecutive lanes reading 16 consecutive 16-byte pieces of ROW k of C -- 256 contiguous bytes per
// k, four such rows per wavefront instruction, straight from global memory with no LDS stage (the first form reads C as the A
// operand: 16 rows x 64 scattered bytes per instruction).  A lane's double2 feeds two accumulator tiles (even / odd columns of
// a 32-column block).  X rows (A operand, 128 contiguous bytes per k) come from L1/L2: n x r is about 1 MB.
// Workgroup = 4 wavefronts on the SAME 32 output rows, each on a quarter of the workgroup's K range; their accumulators are
// added in wave order through LDS (deterministic), so the slab count -- and the slab traffic -- is a quarter of the K split.
// REM (0..4): columns beyond the NT full tiles that do NOT get a matrix-core tile of their own (a 16-column tile for 2 columns is
// 14/16 wasted MFMA time, and at r = 34 the kernel is bound by the matrix pipe once C streams well): they are accumulated by
// plain FMAs from the same C values (each lane multiplies its two C entries with the k-row's X value of the column) and the four
// k-groups of a wavefront are added by shuffles at the end.
template <int NT, int UN = 4, int REM = 0> // NT column tiles of 16 + REM single columns; UN k-steps of 4 rows in flight per trip
__global__ __launch_bounds__(TPB) void k_dense_cx_b(int n, int npad, int krange, const double *__restrict__ Cf,
                                                    const double *__restrict__ X, int r, double *__restrict__ Wpart, Guard g, int col0) {
    // col0: first column of X / W this launch covers (ranks above 128 take several launches of up to 8 column tiles)
    constexpr int NTA = NT > 0 ? NT : 1, RA = REM > 0 ? REM : 1;
    __shared__ double red[3][NTA][2][4][64]; // accumulators of waves 1..3
    __shared__ double redr[3][RA][2][64];
    const Gate gt = gate_load(g);
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, nn = l & 15, kk = l >> 4;
    const int i0 = blockIdx.x * 32;                 // this workgroup's 32 output rows (= columns of C)
    const int kq = krange / 4;                      // (krange is a multiple of 64: see dense_cx)
    const int kbeg = blockIdx.y * krange + wave * kq;
    v4f64 acc[NTA][2];
    double accr[RA][2];
#pragma unroll
    for (int t = 0; t < NTA; ++t) { acc[t][0] = (v4f64){0.0, 0.0, 0.0, 0.0}; acc[t][1] = (v4f64){0.0, 0.0, 0.0, 0.0}; }
#pragma unroll
    for (int j = 0; j < RA; ++j) { accr[j][0] = 0.0; accr[j][1] = 0.0; }
    int colc[NTA];
    double colm[NTA];
#pragma unroll
    for (int ct = 0; ct < NTA; ++ct) {
        const int col = col0 + 16 * ct + nn;
        colc[ct] = (col < r && ct < NT) ? col : 0;
        colm[ct] = (col < r && ct < NT) ? 1.0 : 0.0;
    }
    const int rc0 = col0 + 16 * NT; // first single column
    const double *cp = Cf + (size_t)(kbeg + kk) * npad + i0 + 2 * nn;
    // (a software-pipelined form -- trip t + 1's loads issued before trip t's MFMAs, two register sets -- was slower: 43.6 vs
    // 39.0 us at n = 4096, r = 34; so was UN = 8, and more workgroups: 1024 or 2048 instead of 512 changed nothing)
    for (int k0 = 0; k0 < kq; k0 += 4 * UN) {
        double2 cb[UN];
        double xa[UN][NTA], xr[UN][RA];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            cb[u] = *(const double2 *)(cp + (size_t)(k0 + 4 * u) * npad);
            const int krow = kbeg + k0 + 4 * u + kk;
            const size_t xo = (size_t)(krow < n ? krow : 0) * r; // (rows beyond n: C is zero there, X must stay in bounds)
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) xa[u][ct] = X[xo + colc[ct]] * colm[ct];
#pragma unroll
            for (int j = 0; j < REM; ++j) xr[u][j] = X[xo + (rc0 + j < r ? rc0 + j : 0)];
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                acc[ct][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u][ct], cb[u].x, acc[ct][0], 0, 0, 0);
                acc[ct][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u][ct], cb[u].y, acc[ct][1], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < REM; ++j) { accr[j][0] += xr[u][j] * cb[u].x; accr[j][1] += xr[u][j] * cb[u].y; }
        }
    }
    // the four k-groups of the wavefront hold partial sums of the single columns for the same output rows: add them (fixed order)
#pragma unroll
    for (int j = 0; j < REM; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double v = accr[j][h];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            accr[j][h] = v;
        }
    if (wave > 0) {
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int q = 0; q < 4; ++q) red[wave - 1][ct][h][q][l] = acc[ct][h][q];
#pragma unroll
        for (int j = 0; j < REM; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) redr[wave - 1][j][h][l] = accr[j][h];
    }
    __syncthreads();
    if (wave != 0 || !GATE_OPEN) return;
    double *Wo = Wpart + (size_t)blockIdx.y * n * r;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double v = acc[ct][h][q];
                v += red[0][ct][h][q][l]; v += red[1][ct][h][q][l]; v += red[2][ct][h][q][l];
                const int col = col0 + 16 * ct + kk + 4 * q, row = i0 + 2 * nn + h; // D[m = kk + 4 q][n = nn] of tile (ct, h)
                if (row < n && col < r) Wo[(size_t)row * r + col] = v;
            }
#pragma unroll
    for (int j = 0; j < REM; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double v = accr[j][h];
            v += redr[0][j][h][l]; v += redr[1][j][h][l]; v += redr[2][j][h][l];
            const int col = rc0 + j, row = i0 + 2 * nn + h;
            if (kk == 0 && row < n && col < r) Wo[(size_t)row * r + col] = v;
        }
}
// ---- dense constraint matrices (Block::dense_a): their part of A and A^* through the dense GEMM
// mu_j = weight of dense constraint j in the combination that is being formed (`mode` as k_sval's: W_COMPACT takes wa.w)
__global__ void k_dense_mu(int nd, const int *__restrict__ d_con, int mode, WArgs wa, double sign, double *__restrict__ mu, Guard g) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nd || blocked(g)) return;
    mu[j] = sign * weight_of(mode, wa, d_con[j]);
}
// S = [C] + sum_j mu_j A_j on the full npad x npad matrices (streaming; the GEMM then runs on S)
__global__ void k_dense_combine(size_t len, int nd, const double *__restrict__ A, const double *__restrict__ mu,
                                const double *__restrict__ Cf, double *__restrict__ S, Guard g) {
    if (blocked(g)) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) {
        double v = Cf ? Cf[i] : 0.0;
        for (int j = 0; j < nd; ++j) v += mu[j] * A[(size_t)j * len + i];
        S[i] = v;
    }
}
// the value s = <X, A_j Y> of dense constraint i = d_con[j] (dot partials in `part`) joins what the sparse pass has left: that
// pass saw the constraint with no entries (value 0), so whatever its mode the fix is additive: vec[g] += scale s, cv[i] += s
__global__ __launch_bounds__(TPB) void k_dense_cv_fix(const double *__restrict__ part, int np, int i, double scale, double *__restrict__ cv,
                                                      const int *__restrict__ row_idx, double *__restrict__ vec, Guard g) {
    __shared__ double sh[4];
    const Gate gt = gate_load(g);
    const double s = sum_partials(part, np, sh);
    if (!GATE_OPEN || threadIdx.x != 0) return;
    if (vec) vec[row_idx[i]] += s * scale;
    if (cv) cv[i] += s;
}
// ---- dense constraint matrices with the products W_j = A_j Y kept for the length of a CG solve (Y, the fixed factor, does not change):
// <A_j, sym(X Y^T)> = <X, W_j> is a dot, and (sum_j mu_j A_j) Y = sum_j mu_j W_j a combination -- no GEMM per operator application
// (the reference forms dsyr2k + a packed dot per application, data/lorads_sdp_data.c:698-732; the uncached form here nd + 1 GEMMs).
// workgroup j: s = <X, W_j> (fixed order: strided per thread, then the workgroup sum), then k_dense_cv_fix's bookkeeping
__global__ __launch_bounds__(TPB) void k_dense_dots_fix(size_t len, const double *__restrict__ X, const double *__restrict__ Wj,
                                                        const int *__restrict__ d_con, double scale, double *__restrict__ cv,
                                                        const int *__restrict__ row_idx, double *__restrict__ vec, Guard g) {
    __shared__ double sh[4];
    const Gate gt = gate_load(g);
    const double *__restrict__ W = Wj + (size_t)blockIdx.x * len;
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < len; i += 4 * TPB) { // (four loads per operand and trip in flight)
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const size_t k = i + (size_t)u * TPB, kc = k < len ? k : i; a[u] = X[kc]; b[u] = W[kc]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += i + (size_t)u * TPB < len ? a[u] * b[u] : 0.0;
    }
    const double s = block_sum(acc, sh);
    if (!GATE_OPEN || threadIdx.x != 0) return;
    const int i = d_con[blockIdx.x];
    if (vec) vec[row_idx[i]] += s * scale;
    if (cv) cv[i] += s;
}
// out = [Wc] + sum_j mu_j W_j
__global__ void k_dense_lincomb(size_t len, int nd, const double *__restrict__ Wj, const double *__restrict__ mu,
                                const double *__restrict__ Wc, double *__restrict__ out, Guard g) {
    if (blocked(g)) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) {
        double v = Wc ? Wc[i] : 0.0;
        for (int j = 0; j < nd; ++j) v += mu[j] * Wj[(size_t)j * len + i];
        out[i] = v;
    }
}
// W = sum of the split-K slabs, fixed order
__global__ void k_sum_slabs(size_t len, int ks, const double *__restrict__ part, double *__restrict__ W, Guard g) {
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) {
        double v = part[i];
        for (int k = 1; k < ks; ++k) v += part[(size_t)k * len + i];
        if (GATE_OPEN) W[i] = v;
    }
}

// start of CGSolve (lorads_cgs.c:115,149-172): ||b||_1 and the initial residual norm from partials; every
// workgroup recomputes the two sums (same order -> same value), workgroup 0 publishes the state; p = r
// (one workgroup; the direction of iteration 0 is r itself -- its tail is always the k = 0 restart, which
// sets p = 2 r_true without reading the old p -- so no p = r copy is made)
__global__ __launch_bounds__(TPB) void k_cg_init(CGState *st, const double *__restrict__ part_rr, int nrr,
                                                 const double *__restrict__ part_b, int nb, DS tol, Guard g,
                                                 CGState *shadow = nullptr) {
    __shared__ double sh[8];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const double *const pp[2] = {part_rr, part_b};
    const int nn[2] = {nrr, nb};
    double ab[2];
    private_partials_n<2>(pp, nn, ab);
    block_sum_n<2>(ab, sh);
    const double a = ab[0], b = ab[1];
    const bool conv = sqrt(a) / b < dsv(tol);
    if (!GATE_OPEN || threadIdx.x != 0) return;
    st->rr = a; st->bnorm = b; st->beta = 0.0; st->iter = 0; st->nan = 0; st->pad = 0;
    st->done = conv ? 2 : 0;
    if (shadow) *shadow = *st; // (see Deferred)
}

// x += alpha p, r -= alpha Q, partial ||r||^2; alpha = rr / (p.Q) from device scalars (lorads_cgs.c:181-189)
// w_acc (may be null): the constraint values of the pair (x, V) follow x by linearity, w_acc += alpha * A(sym(p V^T)) with
// the operator's own w_p = A(sym(p V^T)) -- see constr_by_recurrence in sweep.inc
// VEC = true: the four vectors as double2 (len even, 16-byte aligned): half the memory instructions
template <bool VEC>
__global__ __launch_bounds__(TPB) void k_cg_update(size_t len, const CGState *st, const double *__restrict__ part_pq, int npq,
                                                   double *__restrict__ x, double *r, const double *p,
                                                   const double *__restrict__ Q, double *__restrict__ part_rr, Guard g,
                                                   double *__restrict__ w_acc, const double *__restrict__ w_p, int nw,
                                                   CGState *shadow = nullptr, int store_r = 1,
                                                   const double *__restrict__ avg_other = nullptr, double *__restrict__ avg_out = nullptr,
                                                   int tile = 0, int tile_w = 0, const double *__restrict__ part_ww = nullptr,
                                                   int nww = 0) {
    // tile > 0 (row-local operators: Max-Cut-type cones): workgroup b owns elements [b tile, (b + 1) tile) -- the rows of k_op_diag's
    // (and the front's, and k_eval_diag's) workgroup b, tile_w of them.  Workgroups go to the eight XCDs round robin by number, so
    // what this kernel reads (p, Q, r, x) was written by the same-numbered workgroup of the kernel before it ON THE SAME XCD, and
    // what it writes is read there again: the CG iteration's vectors stay in the XCD's own L2 instead of crossing the fabric at
    // every kernel boundary (a kernel replayed back to back ran 15-100 % faster than inside the iteration for that reason,
    // profiles/r02_tried_and_dropped.txt).  tile = 0: grid-stride over the whole vector.
    // store_r = 0: the new residual is only summed, not stored -- the iteration's tail is a restart that recomputes r from
    // scratch (k % 20 == 0, lorads_cgs.c:195-216), and a finished solve never reads it again.
    // avg_out != null: the last update of a sweep that an evaluation follows also leaves R = (U + V) / 2 (averageUV,
    // lorads_admm.c:310-323: k_average's pass, saved) -- from the new x when this update runs, from the x that is there when
    // the solve had finished before it; the evaluation is gated on the solve's state either way.
    __shared__ double sh[4];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const double rr = st->rr; // issued before the partial sums so that the loads overlap
    // the operands of this thread's first PF elements too: threads own a few elements each, and the partial sums below
    // are a dependent chain of their own
    constexpr int PF = 4, EW = VEC ? 2 : 1;
    using T = typename std::conditional<VEC, double2, double>::type;
    const size_t ne_all = len / EW;
    const size_t tl = (size_t)tile / EW; // (tile is even whenever VEC is chosen: a multiple of 32 rows)
    const size_t ebeg = tile ? (size_t)blockIdx.x * tl : 0;
    const size_t ne = tile ? (ebeg + tl < ne_all ? ebeg + tl : ne_all) : ne_all;
    const size_t i0 = tile ? ebeg + threadIdx.x : (size_t)blockIdx.x * TPB + threadIdx.x, stride = tile ? (size_t)TPB : (size_t)gridDim.x * TPB;
    T pv[PF], qv[PF], xv[PF], rv[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const size_t i = i0 + u * stride, ic = i < ne ? i : (ebeg < ne_all ? ebeg : 0);
        pv[u] = ((const T *)p)[ic]; qv[u] = ((const T *)Q)[ic]; xv[u] = ((const T *)x)[ic]; rv[u] = ((const T *)r)[ic];
    }
    // (tile mode: thread t < tile_w owns the row dot of the tile's row t; otherwise the first element index doubles as the w index)
    const size_t iw0 = tile ? (size_t)blockIdx.x * tile_w + threadIdx.x : i0;
    const bool hasw = w_acc && iw0 < (size_t)nw && (!tile || (int)threadIdx.x < tile_w);
    const size_t iw = hasw ? iw0 : 0;
    const double wa0 = w_acc ? w_acc[iw] : 0.0, wp0 = w_acc ? w_p[iw] : 0.0;
    // part_ww != null: iteration 0 of a cone whose k_wsum has left the partials of ||w||^2 -- alpha by the rule of the CG0 form of
    // k_spmm_ell (cg0_alpha), whichever of the two kernels runs the update
    const double alpha = part_ww ? cg0_alpha(rr, sum_partials(part_ww, nww, sh)) : rr / sum_partials(part_pq, npq, sh);
    if (!GATE_OPEN) {
        if (avg_out && gt.vs != 0 && !(g.need && gt.vn == 0)) { // solve over before this update, stage reached: the average alone
            for (size_t i = i0; i < ne; i += stride) {
                const T a = ((const T *)avg_other)[i], b = ((const T *)x)[i];
                if constexpr (VEC) ((double2 *)avg_out)[i] = make_double2(cg_avg(a.x, b.x), cg_avg(a.y, b.y));
                else avg_out[i] = cg_avg(a, b);
            }
        }
        return;
    }
    if (shadow && blockIdx.x == 0 && threadIdx.x == 0) *shadow = *st; // the state the convergence test will start from
    if (hasw) {
        w_acc[iw0] = cg_wacc(wa0, alpha, wp0);
        if (!tile)
            for (size_t i = i0 + stride; i < (size_t)nw; i += stride) w_acc[i] = cg_wacc(w_acc[i], alpha, w_p[i]);
    }
    double local = 0.0;
    auto one = [&](size_t i, const T &pe, const T &qe, const T &xe, const T &re) { // p may alias r (iteration 0): read before written
        if constexpr (VEC) {
            const CgElem ex = cg_elem(alpha, pe.x, qe.x, xe.x, re.x), ey = cg_elem(alpha, pe.y, qe.y, xe.y, re.y);
            ((double2 *)x)[i] = make_double2(ex.x, ey.x);
            if (store_r) ((double2 *)r)[i] = make_double2(ex.r, ey.r);
            local += ex.r * ex.r;
            local += ey.r * ey.r;
            if (avg_out) {
                const double2 o = ((const double2 *)avg_other)[i];
                ((double2 *)avg_out)[i] = make_double2(cg_avg(o.x, ex.x), cg_avg(o.y, ey.x));
            }
        } else {
            const CgElem e = cg_elem(alpha, pe, qe, xe, re);
            x[i] = e.x;
            if (store_r) r[i] = e.r;
            local += e.r * e.r;
            if (avg_out) avg_out[i] = cg_avg(avg_other[i], e.x);
        }
    };
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const size_t i = i0 + u * stride;
        if (i < ne) one(i, pv[u], qv[u], xv[u], rv[u]);
    }
    for (size_t i = i0 + PF * stride; i < ne; i += stride) {
        const T pe = ((const T *)p)[i], qe = ((const T *)Q)[i], xe = ((const T *)x)[i], re = ((const T *)r)[i];
        one(i, pe, qe, xe, re);
    }
    const double t = block_sum(local, sh);
    if (threadIdx.x == 0) part_rr[blockIdx.x] = t;
}

// scalar bookkeeping of CGSolve, one workgroup
__global__ __launch_bounds__(TPB) void k_cg_check(CGState *st, int kind, const double *__restrict__ part_a, int na, DS tol_s,
                                                  DS maxiter_s, Guard g) {
    __shared__ double sh[4];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const double tol = dsv(tol_s);
    const int maxiter = (int)dsv(maxiter_s);
    const double rr_old = st->rr, bnorm = st->bnorm; // issued before the partial sums: the loads overlap
    const int it = st->iter;
    const double a = sum_partials(part_a, na, sh);
    if (!GATE_OPEN || threadIdx.x != 0) return;
    if (kind == CHK_ITER) { // lorads_cgs.c:189-194, :217-224
        st->iter = it + 1;
        if (a != a) st->nan = 1;
        st->beta = a / rr_old;
        st->rr = a;
        if (sqrt(a) / bnorm < tol) st->done = 1;
        else if (it + 1 >= maxiter) st->done = 3;
    } else { // restart: true residual, then beta = qTrNew/qTr = 1 (:195-221)
        st->rr = a;
        st->beta = 1.0;
    }
}

__global__ __launch_bounds__(TPB) void k_cg_dir(size_t len, CGState *st, int kind, const double *__restrict__ r,
                                                double *__restrict__ p, Guard g, Deferred d = Deferred{},
                                                const double *__restrict__ rs_part = nullptr, int rs_np = 0) {
    __shared__ double sh[4];
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const size_t ic = i0 < len ? i0 : 0;
    const double r0 = r[ic], p0 = p[ic]; // fetched while the gate / a carried test is evaluated
    // rs_part != null (DIR_RESTART): the bookkeeping of the restart (k_cg_check, CHK_RESTART: rr = ||true residual||^2,
    // beta = 1; lorads_cgs.c:195-221) is done here by workgroup 0 -- nobody in this kernel reads those two words
    double a_rs = 0.0;
    if (rs_part && blockIdx.x == 0) a_rs = sum_partials(rs_part, rs_np, sh);
    double beta;
    if (d.st) { // the convergence test of the iteration just finished rides on this kernel
        const DefOut o = run_deferred(d, sh);
        if (blocked_after(g, d, o.done)) return;
        beta = o.beta;
    } else {
        if (blocked(g)) return;
        beta = kind == DIR_RESTART ? 1.0 : st->beta;
    }
    if (rs_part && blockIdx.x == 0 && threadIdx.x == 0) { st->rr = a_rs; st->beta = 1.0; }
    // (the multiply-add is spelled out so that k_op_diag's fused form of this update rounds the same way)
    if (i0 < len) p[i0] = kind == DIR_RESTART ? r0 + r0 : fma(beta, p0, r0);
    for (size_t i = i0 + stride; i < len; i += stride) {
        const double rv = r[i];
        p[i] = kind == DIR_RESTART ? rv + rv : fma(beta, p[i], rv);
    }
}

// ---- CG of MANY cones in lockstep on the merged block-diagonal cone (block-separable constraints, equal rank).
// The gather kernels run once for all cones; what stays per cone are the scalars of CGSolve (alpha, beta, norms,
// stopping): SegArgs maps workgroups to cones.  row0[k] = first (padded) row of cone k, a multiple of 32, so the
// per-workgroup partials of the row kernels never straddle two cones: cone k owns tiles [row0[k]/rpw, row0[k+1]/rpw).
// The vector kernels run over chunks of SEG_CH elements, chunk j of the launch belongs to cone vt_seg[j] and starts
// at element vt_e0[j]; cone k owns chunk partials [vt0[k], vt0[k+1]).  State of (cone k, half) is st[2k + half].
// phase_done[half] != 0 <=> every cone's solve of that half has finished (uniform gate for the gather kernels).
constexpr int SEG_CH = 2048;
struct SegArgs {
    const int *row0, *vt0, *vt_seg;
    const long long *vt_e0;
    CGState *st;
    int *phase_done;
    int half, ncones, rpw, r;
    // Where a cone's r.r lives: slot 0 = its state word, slot 1 = rr_alt[state index].  With the convergence test carried by the
    // next operator kernel (see DirArgs.seg_part) the test of iteration k reads slot k & 1 and writes slot (k + 1) & 1, so that the
    // workgroups that still read the old value never race with the one that writes the new; otherwise both are slot 0.
    double *rr_alt;
    int slot_rd, slot_wr;
};
__device__ __forceinline__ double seg_rr_load(const SegArgs &sa, int idx, int slot) { return slot ? sa.rr_alt[idx] : sa.st[idx].rr; }
__device__ __forceinline__ void seg_rr_store(const SegArgs &sa, int idx, int slot, double v) {
    if (slot) sa.rr_alt[idx] = v;
    else sa.st[idx].rr = v;
}
// (four loads per lane and trip, unconditional: see private_partials)
__device__ __forceinline__ double wave_partials(const double *part, int n) { // whole wavefront, result in every lane
    double v = 0.0;
    for (int i = threadIdx.x & 63; i < n; i += 256) {
        double t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = i + 64 * k;
            t[k] = part[j < n ? j : i];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v += (i + 64 * k < n) ? t[k] : 0.0;
    }
    return wave_sum(v);
}
// the same sums over partials that OTHER workgroups of the running kernel have written (they live in other XCDs' L2s until
// released): loads at agent scope
__device__ __forceinline__ double wave_partials_coherent(const double *part, int n) {
    double v = 0.0;
    for (int i = threadIdx.x & 63; i < n; i += 256) {
        double t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = i + 64 * k;
            t[k] = __hip_atomic_load(part + (j < n ? j : i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v += (i + 64 * k < n) ? t[k] : 0.0;
    }
    return wave_sum(v);
}
// all cones finished? (after a barrier that follows the state writes)
__device__ __forceinline__ void publish_phase_done(const SegArgs &sa, int *flag_sh) {
    if (threadIdx.x == 0) *flag_sh = 1;
    __syncthreads();
    for (int k = threadIdx.x; k < sa.ncones; k += blockDim.x)
        if (sa.st[2 * k + sa.half].done == 0) *flag_sh = 0;
    __syncthreads();
    if (threadIdx.x == 0) sa.phase_done[sa.half] = *flag_sh;
}
// k_cg_init for every cone (one workgroup, one wavefront per cone in turn); the U half also re-arms the V half
// (SEG_TPB = 1024 threads: sixteen wavefronts work on sixteen cones side by side -- each cone is a chain of dependent
// loads, bounds -> partials -> state, and four wavefronts walking through sixteen cones in turn took 6-9 us)
constexpr int SEG_TPB = 1024;
__global__ __launch_bounds__(SEG_TPB) void k_cg_init_seg(SegArgs sa, const double *__restrict__ part_rr,
                                                         const double *__restrict__ part_b, DS tol_s, Guard g) {
    __shared__ int flag;
    const double tol = dsv(tol_s);
    if (blocked(g)) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = wave; k < sa.ncones; k += blockDim.x / 64) {
        const int tb = sa.row0[k] / sa.rpw, te = sa.row0[k + 1] / sa.rpw;
        const double a = wave_partials(part_rr + tb, te - tb), b = wave_partials(part_b + tb, te - tb);
        if (lane == 0) {
            CGState *st = sa.st + 2 * k + sa.half;
            st->rr = a; st->bnorm = b; st->beta = 0.0; st->iter = 0; st->nan = 0; st->pad = 1; // pad = "started"
            st->done = sqrt(a) / b < tol ? 2 : 0;
            if (sa.half == 0) { sa.st[2 * k + 1].done = 0; sa.st[2 * k + 1].pad = 0; }
        }
    }
    __threadfence_block();
    if (sa.half == 0 && threadIdx.x == 0) sa.phase_done[1] = 0;
    publish_phase_done(sa, &flag);
}
// k_cg_update per chunk with the alpha of the chunk's cone
// (rounds 2-3 also carried the convergence test on this kernel's last workgroup to finish -- an arrival counter; bit-for-bit and
// slower, profiles/r02_tried_and_dropped.txt 5 -- retired in round 4 with its switch LORADS_SEG_LASTBLOCK)
__global__ __launch_bounds__(TPB) void k_cg_update_seg(SegArgs sa, const double *__restrict__ part_pq, double *__restrict__ x,
                                                       double *r, const double *p, const double *__restrict__ Q,
                                                       double *__restrict__ part_rr, Guard g) {
    __shared__ double sh[4];
    const Gate gt = gate_load(g);
    const int k = sa.vt_seg[blockIdx.x];
    const long long e0 = sa.vt_e0[blockIdx.x];
    const CGState *st = sa.st + 2 * k + sa.half;
    const int done = st->done;
    const int tb = sa.row0[k] / sa.rpw, te = sa.row0[k + 1] / sa.rpw;
    const double rr = seg_rr_load(sa, 2 * k + sa.half, sa.slot_rd);
    const long long eend = (long long)sa.row0[k + 1] * sa.r;
    const long long e1 = e0 + SEG_CH < eend ? e0 + SEG_CH : eend;
    // the chunk's operands are requested before alpha is known (the partial sums are a dependent chain of their own);
    // p may alias r (iteration 0): everything is read before anything is written
    constexpr int PER = SEG_CH / TPB;
    double pv[PER], qv[PER], xv[PER], rv[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const long long i = e0 + threadIdx.x + (long long)u * TPB, ic = i < e1 ? i : e0;
        pv[u] = p[ic]; qv[u] = Q[ic]; xv[u] = x[ic]; rv[u] = r[ic];
    }
    const double pq = sum_partials(part_pq + tb, te - tb, sh);
    const double alpha = rr / pq;
    const bool live = GATE_OPEN && done == 0;
    if (!live) return;
    double local = 0.0;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const long long i = e0 + threadIdx.x + (long long)u * TPB;
        if (i < e1) {
            x[i] = xv[u] + alpha * pv[u];
            const double t = rv[u] - alpha * qv[u];
            r[i] = t;
            local += t * t;
        }
    }
    const double t = block_sum(local, sh);
    if (threadIdx.x == 0) part_rr[blockIdx.x] = t;
}
// k_cg_check for every cone (one workgroup); part: chunk partials (CHK_ITER) or row-tile partials (CHK_RESTART)
__global__ __launch_bounds__(SEG_TPB) void k_cg_check_seg(SegArgs sa, int kind, const double *__restrict__ part, DS tol_s,
                                                          DS maxiter_s, Guard g) {
    __shared__ int flag;
    const double tol = dsv(tol_s);
    const int maxiter = (int)dsv(maxiter_s);
    if (blocked(g)) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = wave; k < sa.ncones; k += blockDim.x / 64) {
        CGState *st = sa.st + 2 * k + sa.half;
        // the cone's state and bounds are requested together, before the partial sums
        const int done0 = st->done, it = st->iter;
        const double rr_old = seg_rr_load(sa, 2 * k + sa.half, sa.slot_rd), bnorm = st->bnorm;
        int lo, hi;
        if (kind == CHK_ITER) { lo = sa.vt0[k]; hi = sa.vt0[k + 1]; }
        else { lo = sa.row0[k] / sa.rpw; hi = sa.row0[k + 1] / sa.rpw; }
        if (done0 != 0) continue; // uniform per wavefront
        const double a = wave_partials(part + lo, hi - lo);
        if (lane == 0) {
            if (kind == CHK_ITER) {
                st->iter = it + 1;
                if (a != a) st->nan = 1;
                st->beta = a / rr_old;
                seg_rr_store(sa, 2 * k + sa.half, sa.slot_wr, a);
                if (sqrt(a) / bnorm < tol) st->done = 1;
                else if (it + 1 >= maxiter) st->done = 3;
            } else {
                seg_rr_store(sa, 2 * k + sa.half, sa.slot_wr, a);
                st->beta = 1.0;
            }
        }
    }
    __threadfence_block();
    publish_phase_done(sa, &flag);
}
__global__ __launch_bounds__(TPB) void k_cg_dir_seg(SegArgs sa, int kind, const double *__restrict__ r, double *__restrict__ p,
                                                    Guard g) {
    const Gate gt = gate_load(g);
    const int k = sa.vt_seg[blockIdx.x];
    const long long e0 = sa.vt_e0[blockIdx.x];
    const CGState *st = sa.st + 2 * k + sa.half;
    const int done = st->done;
    const double beta = st->beta;
    const long long eend = (long long)sa.row0[k + 1] * sa.r;
    const long long e1 = e0 + SEG_CH < eend ? e0 + SEG_CH : eend;
    constexpr int PER = SEG_CH / TPB;
    double rv[PER], pv[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) { // all operands of the chunk in flight together
        const long long i = e0 + threadIdx.x + (long long)u * TPB, ic = i < e1 ? i : e0;
        rv[u] = r[ic]; pv[u] = p[ic];
    }
    if (!GATE_OPEN || done != 0) return;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const long long i = e0 + threadIdx.x + (long long)u * TPB;
        if (i < e1) p[i] = kind == DIR_RESTART ? rv[u] + rv[u] : fma(beta, pv[u], rv[u]);
    }
}

// 1.0 when the gate word says "not finished" (this rank missed its speculation), else 0.0 -- rides on the all-reduce
__global__ void k_miss_flag(const int *need, double *out) { *out = (need && *need == 0) ? 1.0 : 0.0; }
// [objective part | miss flag] behind the staged constraint sums (one workgroup): stage_tail[0] = the sum of the
// objective partials (or the scalar several local cones accumulated into), stage_tail[1] = 1 when this rank's sweep
// is unfinished (then everything it staged is stale, and the flag says so)
__global__ __launch_bounds__(TPB) void k_stage_tail(const double *__restrict__ obj_part, int nobj, const double *obj_scalar,
                                                    const int *need, double *stage_tail) {
    __shared__ double sh[4];
    const double t = obj_part ? sum_partials(obj_part, nobj, sh) : *obj_scalar;
    if (threadIdx.x == 0) {
        stage_tail[0] = t;
        stage_tail[1] = (need && *need == 0) ? 1.0 : 0.0;
    }
}
// after the all-reduce: commit the staged sums (unless some rank missed), the partials of ||b - csum||^2 and
// b.lambda over whatever constrValSum now holds, and the two reduced scalars
// nobj > 0: the objective came through the all-reduce as nobj partials behind the two tail words (summed here by
// workgroup 0), and the staged sums are zeroed once read -- the next evaluation adds into them without a k_zero launch
__global__ __launch_bounds__(TPB) void k_commit_eval(int m, double *__restrict__ stage, double *__restrict__ csum,
                                                     const double *__restrict__ b, const double *__restrict__ lambda,
                                                     double *__restrict__ part_v, double *__restrict__ part_d, double *scal,
                                                     int nobj) {
    __shared__ double sh[8];
    const bool ok = stage[m + 1] == 0.0;
    double obj = stage[m];
    if (nobj > 0 && blockIdx.x == 0) obj = sum_partials(stage + m + 2, nobj, sh);
    double vd[2] = {0.0, 0.0};
    for (int i = blockIdx.x * TPB + threadIdx.x; i < m; i += gridDim.x * TPB) {
        double cs;
        if (ok) { cs = stage[i]; csum[i] = cs; }
        else cs = csum[i];
        if (nobj > 0) stage[i] = 0.0;
        const double t = b[i] - cs;
        vd[0] += t * t;
        vd[1] += b[i] * lambda[i];
    }
    block_sum_n<2>(vd, sh);
    if (threadIdx.x == 0) {
        part_v[blockIdx.x] = vd[0];
        part_d[blockIdx.x] = vd[1];
        if (blockIdx.x == 0) { scal[2] = obj; scal[5] = stage[m + 1]; }
    }
}
// constrValSum <- the all-reduced staging vector, unless some rank reported a miss (stage[m+1] = number of such ranks):
// then every rank keeps its constrValSum -- the unfinished sweeps still need it -- and the evaluation is repeated
__global__ void k_commit_csum(int m, const double *__restrict__ stage, double *__restrict__ csum) {
    if (stage[m + 1] != 0.0) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) csum[i] = stage[i];
}

// ---- LP block (one diagonal cone, rank 1, lorads_hip_block.is_lp).  In phase 1 and in every evaluation it runs
// through the generic cone kernels.  The ADMM update is the reference's closed form, column by column in file order
// (LORADSUpdateLPVarOne, lorads_admm.c:595-629; bookkeeping lorads_alg_common.c:236-246):
//   m1_k = rho (csum[g_k] - cvLP_k - b[g_k]) - lambda[g_k],  w = c + sum_k m1_k a_k,
//   u <- (-(w v - rho v) / rho) / (1 + ||a||^2 v^2),  cvLP_k <- a_k u v (csum follows),  then the same for v.
// Columns that share no constraint row do not see each other, so the sweep is LEVEL-SCHEDULED: level(j) =
// 1 + max level of the earlier columns sharing a row with j; columns of one level are updated in parallel, levels in
// order -- exactly the sequential result.  Slack-type blocks (every column alone in its row) are one level.
struct LpArgs {
    int ncols, nlev;
    const int *lvl_ptr, *lvl_cols, *ptr, *grow; // level -> columns; column -> entries; entry -> global constraint
    const double *a, *nrm2sq, *cobj;
    double *cv, *U, *V, *csum;
    const double *b, *lambda;
    DS rho;
};
__device__ __forceinline__ double lp_new_value(const LpArgs &A, int col, double fixed) {
    const double rho = dsv(A.rho);
    double w = A.cobj[col];
    for (int t = A.ptr[col]; t < A.ptr[col + 1]; ++t) {
        const int g = A.grow[t];
        double m1 = A.b[g];
        m1 *= -1.0;
        m1 += A.csum[g];
        m1 += -1.0 * A.cv[t];
        m1 *= rho;
        m1 += -1.0 * A.lambda[g];
        w += m1 * A.a[t];
    }
    double M2 = w * fixed;
    M2 = M2 - rho * fixed;
    const double blin = -1.0 * M2 / rho;
    return blin / (1 + A.nrm2sq[col] * fixed * fixed);
}
__device__ __forceinline__ void lp_refresh(const LpArgs &A, int col, double uv) {
    for (int t = A.ptr[col]; t < A.ptr[col + 1]; ++t) {
        const int g = A.grow[t];
        double cs = A.csum[g] + -1.0 * A.cv[t];
        const double nv = A.a[t] * uv;
        A.cv[t] = nv;
        A.csum[g] = cs + nv;
    }
}
__device__ __forceinline__ void lp_column(const LpArgs &A, int col) {
    const double u = lp_new_value(A, col, A.V[col]);
    A.U[col] = u;
    lp_refresh(A, col, u * A.V[col]);
    const double v = lp_new_value(A, col, u);
    A.V[col] = v;
    lp_refresh(A, col, u * v);
}
// one workgroup walks the levels; done words of the block's two stages are set at the end
__global__ __launch_bounds__(TPB) void k_lp_sweep(LpArgs A, CGState *st, Guard g) {
    if (blocked(g)) return;
    for (int lev = 0; lev < A.nlev; ++lev) {
        for (int i = A.lvl_ptr[lev] + threadIdx.x; i < A.lvl_ptr[lev + 1]; i += TPB) lp_column(A, A.lvl_cols[i]);
        __threadfence_block();
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        st[0].iter = 0; st[0].nan = 0; st[0].pad = 1; st[0].done = 1;
        st[1].iter = 0; st[1].nan = 0; st[1].pad = 1; st[1].done = 1;
    }
}
// single level: every column independent, many workgroups; the done words are set by k_lp_done afterwards
__global__ __launch_bounds__(TPB) void k_lp_sweep_flat(LpArgs A, Guard g) {
    if (blocked(g)) return;
    const int col = blockIdx.x * TPB + threadIdx.x;
    if (col < A.ncols) lp_column(A, col);
}
__global__ void k_lp_done(CGState *st, Guard g) {
    if (blocked(g)) return;
    st[0].iter = 0; st[0].nan = 0; st[0].pad = 1; st[0].done = 1;
    st[1].iter = 0; st[1].nan = 0; st[1].pad = 1; st[1].done = 1;
}
// constrValLP: cv_t = a_t x_col y_col for every stored entry (lp_cone_AUV, data/lorads_lp_conic.c:172-175)
__global__ void k_lp_cv(int ncols, const int *__restrict__ ptr, const double *__restrict__ a, const double *__restrict__ X,
                        const double *__restrict__ Y, double *__restrict__ cv, Guard g) {
    if (blocked(g)) return;
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= ncols) return;
    const double uv = X[col] * Y[col];
    for (int t = ptr[col]; t < ptr[col + 1]; ++t) cv[t] = a[t] * uv;
}
// sum over the columns of |min(c - sum_k lambda a, 0)| (data/lorads_solver.c:1015-1023), one workgroup
__global__ __launch_bounds__(TPB) void k_lp_dual(int ncols, const int *__restrict__ ptr, const int *__restrict__ grow,
                                                 const double *__restrict__ a, const double *__restrict__ cobj,
                                                 const double *__restrict__ lambda, double *out) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int col = threadIdx.x; col < ncols; col += TPB) {
        double w = cobj[col];
        for (int t = ptr[col]; t < ptr[col + 1]; ++t) w += -lambda[grow[t]] * a[t];
        acc += fabs(w < 0.0 ? w : 0.0);
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) *out = acc;
}

// Result hand-over without hipStreamSynchronize: one workgroup copies `nwords` 8-byte words of the control block into
// host-mapped pinned memory, fences at system scope and then publishes a sequence number the host spins on.  Cuts the
// per-iteration wake-up latency of an interrupt-driven stream synchronisation (and the separate copy kernel).
// The sequence number is a DEVICE counter (seq_dev, bumped by every hand-over; the host counts along): the kernel's arguments are
// the same for every hand-over, so a captured launch chain that ends in one can be replayed as it is.
__global__ __launch_bounds__(TPB) void k_publish(const unsigned long long *__restrict__ src, int nwords, unsigned long long *dst,
                                                 unsigned long long *flag, unsigned long long *seq_dev) {
    const unsigned long long seq = *seq_dev + 1;
    for (int i = threadIdx.x; i < nwords; i += TPB) dst[i] = src[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        *seq_dev = seq;
        __atomic_store_n(flag, seq, __ATOMIC_RELEASE);
        __threadfence_system();
    }
}

// k_eval_final and k_publish in one launch: the closing sums of an evaluation (gated like the evaluation itself) are
// written to the device scalars and the control block then goes to the host mirror in the same workgroup (publish_final, above
// k_front_cw, whose hand-over form runs the same body in a workgroup of its own)
__global__ __launch_bounds__(TPB) void k_publish_final(EvalFinalArgs fa, const unsigned long long *src, int nwords,
                                                       unsigned long long *dst, unsigned long long *flag, unsigned long long *seq_dev) {
    __shared__ double sh[12];
    publish_final(fa, src, nwords, dst, flag, seq_dev, sh);
}
// the hand-over that follows the all-reduce of separable shards: k_sep_commit (the reduced scalars into the control block) and
// k_publish in one launch -- the sharded iteration's chain is one kernel shorter
struct SepExtra;
__global__ __launch_bounds__(TPB) void k_publish_sep(const double *buf, double *scal, int with_obj, int nex, double *ex0, double *ex1,
                                                     double *ex2, double *ex3, const unsigned long long *src, int nwords,
                                                     unsigned long long *dst, unsigned long long *flag, unsigned long long *seq_dev) {
    const unsigned long long seq = *seq_dev + 1;
    if (threadIdx.x == 0) {
        scal[0] = buf[0];
        scal[1] = buf[1];
        if (with_obj) scal[2] = buf[2];
        scal[5] = buf[3];
        double *const ex[4] = {ex0, ex1, ex2, ex3};
        for (int k = 0; k < nex; ++k) *ex[k] = buf[4 + k];
    }
    __threadfence();
    __syncthreads();
    for (int i = threadIdx.x; i < nwords; i += TPB) dst[i] = __builtin_nontemporal_load(src + i);
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        *seq_dev = seq;
        __atomic_store_n(flag, seq, __ATOMIC_RELEASE);
        __threadfence_system();
    }
}
// the step parameters of a replayed launch chain (see DS): written only when they change
__global__ void k_set_par(double *par, double v0, double v1, double v2, double v3, int mask) {
    if (mask & 1) par[0] = v0;
    if (mask & 2) par[1] = v1;
    if (mask & 4) par[2] = v2;
    if (mask & 8) par[3] = v3;
}

// ---- small vector kernels
__global__ __launch_bounds__(TPB) void k_average(size_t len, const double *__restrict__ u, const double *__restrict__ v,
                                                 double *__restrict__ out, Guard g, Deferred d = Deferred{}) {
    __shared__ double sh[4];
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    // 16-byte accesses when the three vectors allow it (even length, 16-byte aligned: uniform test)
    const bool v2 = (len & 1) == 0 && (((uintptr_t)u | (uintptr_t)v | (uintptr_t)out) & 15) == 0;
    if (v2) {
        const size_t n2 = len / 2, ic = i0 < n2 ? i0 : 0;
        const double2 a0 = ((const double2 *)u)[ic], b0 = ((const double2 *)v)[ic]; // fetched while a carried test is evaluated
        if (d.st) {
            if (blocked_after(g, d, run_deferred(d, sh).done)) return;
        } else if (blocked(g)) return;
        if (i0 < n2) ((double2 *)out)[i0] = make_double2((a0.x + b0.x) / 2, (a0.y + b0.y) / 2);
        for (size_t i = i0 + stride; i < n2; i += stride) {
            const double2 a = ((const double2 *)u)[i], b = ((const double2 *)v)[i];
            ((double2 *)out)[i] = make_double2((a.x + b.x) / 2, (a.y + b.y) / 2);
        }
        return;
    }
    const size_t ic = i0 < len ? i0 : 0;
    const double u0 = u[ic], v0 = v[ic]; // fetched while a carried test is evaluated
    if (d.st) { // the last convergence test of the sweep rides on the evaluation's first kernel
        if (blocked_after(g, d, run_deferred(d, sh).done)) return;
    } else if (blocked(g)) return;
    if (i0 < len) out[i0] = (u0 + v0) / 2;
    for (size_t i = i0 + stride; i < len; i += stride) out[i] = (u[i] + v[i]) / 2;
}
// The evaluation's first half for a Max-Cut-type cone (every A_i = a_i e_p e_p^T) in one row pass: R_p = (U_p + V_p) / 2
// (averageUV, lorads_admm.c:310-323), the constraint values a_i ||R_p||^2 of the row's constraints (LORADSInitConstrVal on
// (R, R): constrVal <- , constrValSum <-; quirk Q1) and the partials of ||b - A(R R^T)||^2 and b . lambda -- k_average +
// k_pairdots + k_cv_res in the older form.  rc_con: row -> its constraints, fixed width rc_w (-1 = none).  ||R_p||^2 is summed
// as k_pairdots sums it.  Carries a waiting convergence test as k_average did.
template <int LG, bool V2, int NS>
__global__ __launch_bounds__(TPB) void k_eval_diag(int n, const double *__restrict__ U, const double *__restrict__ V,
                                                   double *__restrict__ R, int r, int rc_w, const int *__restrict__ rc_con,
                                                   const double *__restrict__ da, const int *__restrict__ row_idx,
                                                   double *__restrict__ cv, double *__restrict__ vec, const double *__restrict__ b,
                                                   const double *__restrict__ lambda, double *__restrict__ part_v,
                                                   double *__restrict__ part_d, Guard g, Deferred d) {
    __shared__ double sh[8];
    constexpr int W = V2 ? 2 : 1;
    const Gate gt = gate_load(g);
    DefPriv dv{};
    if (d.st) dv = deferred_private(d);
    const int row = (blockIdx.x * TPB + threadIdx.x) / LG, lane = threadIdx.x % LG;
    const bool act = row < n;
    const int rowc = act ? row : 0;
    const size_t base = (size_t)rowc * r;
    double u[NS][W], v[NS][W];
    Slice<LG, V2, NS>::load(U + base, r, lane, u);
    Slice<LG, V2, NS>::load(V + base, r, lane, v);
    const int ci = (lane < rc_w && act) ? rc_con[(size_t)rowc * rc_w + lane] : -1; // this lane's constraint of the row
    const int cic = ci >= 0 ? ci : 0;
    const int gi = row_idx ? row_idx[cic] : cic;
    const double ai = da[cic], bi = b[gi], li = lambda[gi];
    const bool live = d.st ? !blocked_after(g, d, finish_deferred(d, dv, sh).done) : GATE_OPEN;
    double rn = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const int j0 = (lane + c * LG) * W;
        double a[W];
#pragma unroll
        for (int w = 0; w < W; ++w) { a[w] = (u[c][w] + v[c][w]) / 2; rn += a[w] * a[w]; }
        if (live && act && j0 < r) {
            if (V2) *(double2 *)(R + base + j0) = make_double2(a[0], a[W - 1]);
            else R[base + j0] = a[0];
        }
    }
    rn = group_sum<LG>(rn);
    double vd[2] = {0.0, 0.0};
    if (ci >= 0) {
        const double s = ai * rn, t = bi - s;
        if (live) { vec[gi] = s; cv[ci] = s; }
        vd[0] = t * t;
        vd[1] = bi * li;
    }
    block_sum_n<2>(vd, sh);
    if (live && threadIdx.x == 0) { part_v[blockIdx.x] = vd[0]; part_d[blockIdx.x] = vd[1]; }
}
// rank growth (AUG_RANK, data/lorads_solver.c:806-906; lpRandomDiag :776-786) on a row-major n x r factor: row i keeps its r_old
// entries; of the new columns, column j holds dv = 1/sqrt(rr) in row j for j < rr = min(n, r_new - r_old), zeros elsewhere
// (r_old, r_new: the ranks; s_old, s_new: the row strides -- the ranks rounded up to even, the extra column zero)
__global__ void k_grow_rank(size_t len, int r_old, int s_old, int r_new, int s_new, const double *__restrict__ src, double *__restrict__ dst,
                            int rr, double dv) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / (size_t)s_new;
        const int col = (int)(i - row * (size_t)s_new);
        dst[i] = col < r_old ? src[row * (size_t)s_old + col]
                             : ((col < r_new && (size_t)(col - r_old) == row && (int)row < rr) ? dv : 0.0);
    }
}
__global__ void k_zero(size_t len, double *__restrict__ y, Guard g) {
    if (blocked(g)) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) y[i] = 0.0;
}
__global__ void k_axpy(size_t len, double a, const double *__restrict__ x, double *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x)
        y[i] += a * x[i];
}
__global__ void k_axpy_dev(size_t len, const double *coef, const double *__restrict__ x, double *__restrict__ y) {
    const double a = *coef;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x)
        y[i] += a * x[i];
}
__global__ void k_scale_copy(size_t len, double a, const double *__restrict__ x, double *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x)
        y[i] = a * x[i];
}
__global__ void k_scale(size_t len, double a, double *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) y[i] *= a;
}
// s = tau*D, y += G  (setlbfgsHisTwo)
__global__ void k_his_two(size_t len, double tau, const double *__restrict__ D, const double *__restrict__ G,
                          double *__restrict__ s, double *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) {
        s[i] = tau * D[i];
        y[i] += G[i];
    }
}
// D = -G when <D,G> >= 0 (LBFGSDirectionUseGrad)
__global__ void k_use_grad(size_t len, const double *ip, const double *__restrict__ G, double *__restrict__ D) {
    if (!(*ip >= 0)) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x)
        D[i] = -G[i];
}
__global__ __launch_bounds__(TPB) void k_dot(size_t len, const double *__restrict__ x, const double *__restrict__ y,
                                             double *__restrict__ part, Guard g) {
    __shared__ double sh[4];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    double local = 0.0;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < len; i += (size_t)gridDim.x * TPB) local += x[i] * y[i];
    const double t = block_sum(local, sh);
    if (GATE_OPEN && threadIdx.x == 0) part[blockIdx.x] = t;
}
// out (= or +=) scale * sum(part)
__global__ __launch_bounds__(TPB) void k_finalize(const double *__restrict__ part, int n, double scale, int accumulate,
                                                  double *out, Guard g) {
    __shared__ double sh[4];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const double t = sum_partials(part, n, sh);
    if (GATE_OPEN && threadIdx.x == 0) *out = accumulate ? *out + scale * t : scale * t;
}
// One stage of the L-BFGS two-loop recursion (lorads_alm.c:230-391) per launch:
//   [coefficient from the previous stage's dot partials]  ->  q += coef * ax  ->  partials of <dv, q>.
// Every workgroup re-sums the previous partials in the order k_finalize uses, so all of them see the same
// coefficient and the arithmetic is that of the k_dot / k_finalize / k_scalar_op / k_axpy_dev chain it replaces.
// ab = {alpha, beta} of the history node the coefficient belongs to.  dout != nullptr: last stage, D = -q and
// the partials are those of <D, dv> (dv = Grad).
enum { ST_FIRST = 0, ST_ALPHA = 1, ST_W = 2 };
__global__ __launch_bounds__(TPB) void k_lbfgs_stage(size_t len, int op, const double *__restrict__ prev_part, int nprev,
                                                     double *ab, const double *__restrict__ ax, double *q,
                                                     const double *__restrict__ qsrc, const double *__restrict__ dv,
                                                     double *__restrict__ part_out, double *__restrict__ dout) {
    __shared__ double sh[4];
    // this thread's first PF element pairs are requested before the previous stage's partials are summed (the sum is a
    // dependent chain of its own: loads, two barriers)
    constexpr int PF = 4;
    const size_t gid0 = (size_t)blockIdx.x * TPB + threadIdx.x, stride0 = (size_t)gridDim.x * TPB, n20 = len / 2;
    const double2 *q20 = (const double2 *)(op == ST_FIRST ? qsrc : q), *ax20 = (const double2 *)ax, *dv20 = (const double2 *)dv;
    double2 pq[PF], pdv[PF], pax[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const size_t i = gid0 + u * stride0, ic = i < n20 ? i : 0;
        pq[u] = q20[ic]; pdv[u] = dv20[ic];
        pax[u] = op == ST_FIRST ? pq[u] : ax20[ic];
    }
    double coef = 0.0;
    if (op != ST_FIRST) {
        const double dot = sum_partials(prev_part, nprev, sh);
        if (op == ST_ALPHA) {
            const double alpha = ab[1] * dot;
            coef = -1 * alpha;
            if (blockIdx.x == 0 && threadIdx.x == 0) ab[0] = alpha;
        } else {
            coef = ab[0] - ab[1] * dot;
        }
    }
    double local = 0.0;
    auto one = [&](double qi, double axi, double dvi, double &store) { // one element of the stage
        const double v = op == ST_FIRST ? qi : qi + coef * axi;
        if (dout) { store = -1.0 * v; local += store * dvi; }
        else { store = v; local += dvi * v; }
    };
    // 16-byte accesses: these stages only stream (3 vectors in, 1 out)
    const size_t gid = (size_t)blockIdx.x * TPB + threadIdx.x, stride = (size_t)gridDim.x * TPB, n2 = len / 2;
    const double2 *q2 = (const double2 *)(op == ST_FIRST ? qsrc : q), *ax2 = (const double2 *)ax, *dv2 = (const double2 *)dv;
    double2 *o2 = (double2 *)(dout ? dout : q);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const size_t i = gid + u * stride;
        if (i < n2) {
            double2 st;
            one(pq[u].x, pax[u].x, pdv[u].x, st.x);
            one(pq[u].y, pax[u].y, pdv[u].y, st.y);
            o2[i] = st;
        }
    }
    for (size_t i = gid + PF * stride; i < n2; i += stride) {
        const double2 qv = q2[i], dvv = dv2[i];
        const double2 axv = op == ST_FIRST ? qv : ax2[i];
        double2 st;
        one(qv.x, axv.x, dvv.x, st.x);
        one(qv.y, axv.y, dvv.y, st.y);
        o2[i] = st;
    }
    if ((len & 1) && gid == 0) {
        const size_t i = len - 1;
        double st;
        one(op == ST_FIRST ? qsrc[i] : q[i], op == ST_FIRST ? 0.0 : ax[i], dv[i], st);
        (dout ? dout : q)[i] = st;
    }
    const double t = block_sum(local, sh);
    if (threadIdx.x == 0) part_out[blockIdx.x] = t;
}
// D = -G when <D,G> >= 0 (LBFGSDirectionUseGrad), <D,G> given as partials
__global__ __launch_bounds__(TPB) void k_use_grad_p(size_t len, const double *__restrict__ part, int npart,
                                                    const double *__restrict__ G, double *__restrict__ D) {
    __shared__ double sh[4];
    const double ip = sum_partials(part, npart, sh);
    if (!(ip >= 0)) return;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < len; i += (size_t)gridDim.x * TPB) D[i] = -G[i];
}
// s = tau*D, y += G (setlbfgsHisTwo) and the partials of <y, s>
__global__ __launch_bounds__(TPB) void k_his_two_dot(size_t len, double tau, const double *__restrict__ D,
                                                     const double *__restrict__ G, double *__restrict__ s,
                                                     double *__restrict__ y, double *__restrict__ part) {
    __shared__ double sh[4];
    double local = 0.0;
    const size_t gid = (size_t)blockIdx.x * TPB + threadIdx.x, stride = (size_t)gridDim.x * TPB, n2 = len / 2;
    for (size_t i = gid; i < n2; i += stride) {
        const double2 d = ((const double2 *)D)[i], gg = ((const double2 *)G)[i], yo = ((const double2 *)y)[i];
        double2 si, yi;
        si.x = tau * d.x; yi.x = yo.x + gg.x;
        si.y = tau * d.y; yi.y = yo.y + gg.y;
        ((double2 *)s)[i] = si;
        ((double2 *)y)[i] = yi;
        local += yi.x * si.x;
        local += yi.y * si.y;
    }
    if ((len & 1) && gid == 0) {
        const size_t i = len - 1;
        const double si = tau * D[i], yi = y[i] + G[i];
        s[i] = si;
        y[i] = yi;
        local += yi * si;
    }
    const double t = block_sum(local, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}
// beta = 1 / sum(part)
__global__ __launch_bounds__(TPB) void k_finalize_beta(const double *__restrict__ part, int n, double *beta) {
    __shared__ double sh[4];
    const double t = sum_partials(part, n, sh);
    if (threadIdx.x == 0) *beta = 1.0 / t;
}
enum { SOP_ALPHA = 0, SOP_W = 1, SOP_BETA = 2 };
// scalar algebra of the two-loop recursion
__global__ void k_scalar_op(int op, const double *dot, double *alpha, double *beta, double *coef) {
    if (op == SOP_ALPHA) { *alpha = *beta * *dot; *coef = -1 * *alpha; }
    else if (op == SOP_W) { *coef = *alpha - *beta * *dot; }
    else { *beta = 1.0 / *dot; }
}
// partials of sum (b-csum)^2 and b.lambda over the m constraints (primalInfeasibility, LORADSCalDualObj) when no
// constraint-value kernel could produce them on the way (cones that share constraints)
__global__ __launch_bounds__(TPB) void k_eval_part(int m, const double *__restrict__ b, const double *__restrict__ csum,
                                                   const double *__restrict__ lambda, double *__restrict__ part_v,
                                                   double *__restrict__ part_d, Guard g) {
    __shared__ double sh[8];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    double vd[2] = {0.0, 0.0};
    for (int i = blockIdx.x * TPB + threadIdx.x; i < m; i += gridDim.x * TPB) {
        const double t = b[i] - csum[i];
        vd[0] += t * t;
        vd[1] += b[i] * lambda[i];
    }
    block_sum_n<2>(vd, sh);
    if (GATE_OPEN && threadIdx.x == 0) { part_v[blockIdx.x] = vd[0]; part_d[blockIdx.x] = vd[1]; }
}
// cv_i = w_i = sum_k a_k T[e_k] and vec[g_i] = w_i for a cone that sees every constraint (k_cv with CV_SET, scale 1),
// plus the partials of sum (b - w)^2 and b.lambda over the rows this workgroup owns
__global__ __launch_bounds__(TPB) void k_cv_res(int nrow, const int *__restrict__ a_ptr, const int *__restrict__ a_e,
                                                const double *__restrict__ a_val, const double *__restrict__ T,
                                                double *__restrict__ cv, const int *__restrict__ row_idx, double *__restrict__ vec,
                                                const double *__restrict__ b, const double *__restrict__ lambda,
                                                double *__restrict__ part_v, double *__restrict__ part_d, Guard g) {
    __shared__ double sh[8];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const int lane = threadIdx.x & 7, per = TPB / 8;
    double vd[2] = {0.0, 0.0};
    for (int i0 = blockIdx.x * per; i0 < nrow; i0 += gridDim.x * per) {
        const int i = i0 + threadIdx.x / 8;
        const bool act = i < nrow;
        double s = 0.0;
        if (act)
            for (int t = a_ptr[i] + lane; t < a_ptr[i + 1]; t += 8) s += a_val[t] * T[a_e[t]];
        s = group_sum<8>(s);
        if (act && lane == 0) {
            const int gi = row_idx[i];
            const double w = s * 1.0, bi = b[gi], t = bi - w;
            if (GATE_OPEN) { vec[gi] = w; cv[i] = s; }
            vd[0] += t * t;
            vd[1] += bi * lambda[gi];
        }
    }
    block_sum_n<2>(vd, sh);
    if (GATE_OPEN && threadIdx.x == 0) { part_v[blockIdx.x] = vd[0]; part_d[blockIdx.x] = vd[1]; }
}
// one workgroup: out[0] = sum (b-csum)^2, out[1] = b.lambda from their partials, out[2] = <C, R R^T> (one cone, one rank)
__global__ __launch_bounds__(TPB) void k_eval_final(const double *__restrict__ part_v, const double *__restrict__ part_d, int np,
                                                    double *out, Guard g, const double *__restrict__ obj_part, int nobj) {
    __shared__ double sh[12];
    const Gate gt = gate_load(g); // (both gate words requested now, looked at where GATE_OPEN first appears)
    const double *const pp[3] = {part_v, part_d, obj_part ? obj_part : part_v};
    const int nn[3] = {np, np, obj_part ? nobj : 0};
    double t3[3];
    private_partials_n<3>(pp, nn, t3);
    block_sum_n<3>(t3, sh);
    const double v = t3[0], d = t3[1], o = t3[2];
    if (GATE_OPEN && threadIdx.x == 0) { out[0] = v; out[1] = d; if (obj_part) out[2] = o; }
}

struct SepExtra { int n; double *p[4]; }; // device scalars that share the evaluation's all-reduce (separable shards)
// ---- L-BFGS direction in GRAM FORM (sharded cones).  The two-loop recursion (lorads_alm.c:230-391) takes 2 nn + 1 dots, each
// against a vector the previous dot's result has just changed: 2 nn + 1 collectives in a row when the vectors are dealt over ranks.
// Every vector it touches is a combination of V = {Grad, y_t, s_t (t = newest .. oldest)}, so all its dots are combinations of the
// (2 nn + 1)^2 products V_a.V_b: ONE pass over the vectors forms them (k_gram), ONE all-reduce sums them over the ranks, one thread
// runs the recursion on the coefficients (k_lbfgs_coef; also LBFGSDirUseGrad's test, :469-489), one pass forms D (k_lincomb).
// Same arithmetic up to the order of the sums.
constexpr int GRAM_MAXV = 11; // history <= 5
struct GramVecs { const double *v[GRAM_MAXV]; };
struct GramPlan { int nn; int node[5]; }; // ring nodes, newest -> oldest
template <int NV>
__global__ __launch_bounds__(TPB) void k_gram(size_t len, GramVecs gv, double *__restrict__ part) { // part[pair][workgroup]
    constexpr int NP = NV * (NV + 1) / 2;
    __shared__ double sh[NP * 4];
    double acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = 0.0;
    // 16-byte loads, two trips' operands in flight (the vectors are the flat factor arrays: even length, 16-byte aligned whenever
    // every cone's n r is even; uniform test).  One 8-byte element per trip ran at 2.8 TB/s.
    bool v2 = (len & 1) == 0;
#pragma unroll
    for (int a = 0; a < NV; ++a) v2 = v2 && (((uintptr_t)gv.v[a]) & 15) == 0;
    const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, stride = (size_t)gridDim.x * TPB;
    if (v2) {
        const size_t n2 = len / 2;
        for (size_t i = tid; i < n2; i += 2 * stride) {
            const size_t j = i + stride, jc = j < n2 ? j : i;
            double2 x[NV], y[NV];
#pragma unroll
            for (int a = 0; a < NV; ++a) { x[a] = ((const double2 *)gv.v[a])[i]; y[a] = ((const double2 *)gv.v[a])[jc]; }
            if (j >= n2) {
#pragma unroll
                for (int a = 0; a < NV; ++a) y[a] = make_double2(0.0, 0.0);
            }
            int p = 0;
#pragma unroll
            for (int a = 0; a < NV; ++a)
#pragma unroll
                for (int b = a; b < NV; ++b) {
                    acc[p] = fma(x[a].x, x[b].x, acc[p]); acc[p] = fma(x[a].y, x[b].y, acc[p]);
                    acc[p] = fma(y[a].x, y[b].x, acc[p]); acc[p] = fma(y[a].y, y[b].y, acc[p]);
                    ++p;
                }
        }
    } else
    for (size_t i = tid; i < len; i += stride) {
        double x[NV];
#pragma unroll
        for (int a = 0; a < NV; ++a) x[a] = gv.v[a][i];
        int p = 0;
#pragma unroll
        for (int a = 0; a < NV; ++a)
#pragma unroll
            for (int b = a; b < NV; ++b) { acc[p] = fma(x[a], x[b], acc[p]); ++p; }
    }
    block_sum_n<NP>(acc, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int p = 0; p < NP; ++p) part[(size_t)p * gridDim.x + blockIdx.x] = acc[p];
    }
}
// the recursion on coefficients (one thread).  q = sum_k a_k V_k starts as Grad; coef = the coefficients of D = -q, or of -Grad when
// D.Grad >= 0 (LBFGSDirUseGrad).  alpha_t is left in ring_ab as the sequential form leaves it.
__device__ __forceinline__ void lbfgs_coef_body(const GramPlan &pl, const double *gram, double *ring_ab, double *__restrict__ coef) {
    const int nn = pl.nn, nv = 2 * nn + 1;
    double a[GRAM_MAXV];
    for (int k = 0; k < nv; ++k) a[k] = k == 0 ? 1.0 : 0.0;
#define GRAM_AT(i_, j_) gram[((i_) < (j_) ? (i_) : (j_)) * nv - ((i_) < (j_) ? (i_) : (j_)) * (((i_) < (j_) ? (i_) : (j_)) - 1) / 2 + ((i_) < (j_) ? (j_) - (i_) : (i_) - (j_))]
    for (int t = 0; t < nn; ++t) { // newest -> oldest: alpha = beta s.q, q -= alpha y
        const int is = 1 + nn + t, iy = 1 + t, node = pl.node[t];
        double dot = 0.0;
        for (int k = 0; k < nv; ++k) dot += a[k] * GRAM_AT(is, k);
        const double alpha = ring_ab[2 * node + 1] * dot;
        ring_ab[2 * node] = alpha;
        a[iy] += -1 * alpha;
    }
    for (int t = nn - 1; t >= 0; --t) { // oldest -> newest: q += (alpha - beta y.q) s
        const int is = 1 + nn + t, iy = 1 + t, node = pl.node[t];
        double dot = 0.0;
        for (int k = 0; k < nv; ++k) dot += a[k] * GRAM_AT(iy, k);
        a[is] += ring_ab[2 * node] - ring_ab[2 * node + 1] * dot;
    }
    double ip = 0.0; // D.Grad = -q.Grad
    for (int k = 0; k < nv; ++k) ip -= a[k] * GRAM_AT(0, k);
#undef GRAM_AT
    const bool use_grad = ip >= 0;
    for (int k = 0; k < nv; ++k) coef[k] = use_grad ? (k == 0 ? -1.0 : 0.0) : -a[k];
}
// the products' sums: wavefront w adds up pairs w, w + 4, ... (one wave sum each; the four wavefronts side by side -- 15 block sums
// one after the other took 11.5 us at the headline).  coef != null (one rank: nothing to sum over ranks in between): the recursion on
// coefficients follows in the same launch, from the sums held in LDS.
__global__ __launch_bounds__(TPB) void k_gram_final(const double *__restrict__ part, int npair, int g, double *__restrict__ gram,
                                                    GramPlan pl, double *ring_ab, double *__restrict__ coef) {
    __shared__ double sg[GRAM_MAXV * (GRAM_MAXV + 1) / 2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int p = wave; p < npair; p += TPB / 64) {
        const double t = wave_partials(part + (size_t)p * g, g);
        if (lane == 0) { gram[p] = t; sg[p] = t; }
    }
    if (!coef) return;
    __syncthreads();
    if (threadIdx.x == 0) lbfgs_coef_body(pl, sg, ring_ab, coef);
}
__global__ void k_lbfgs_coef(GramPlan pl, const double *__restrict__ gram, double *ring_ab, double *__restrict__ coef) {
    lbfgs_coef_body(pl, gram, ring_ab, coef);
}
template <int NV>
__global__ __launch_bounds__(TPB) void k_lincomb(size_t len, GramVecs gv, const double *__restrict__ coef, double *__restrict__ D) {
    double cf[NV];
#pragma unroll
    for (int a = 0; a < NV; ++a) cf[a] = coef[a];
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < len; i += (size_t)gridDim.x * TPB) {
        double x[NV];
#pragma unroll
        for (int a = 0; a < NV; ++a) x[a] = gv.v[a][i];
        double d = 0.0;
#pragma unroll
        for (int a = 0; a < NV; ++a) d = fma(cf[a], x[a], d);
        D[i] = d;
    }
}

// Separable shards (lorads_hip_set_separable): k_eval_final's sums, staged for the all-reduce of four scalars.  A rank whose gate is
// shut (its sweep missed the speculation: nothing of this evaluation ran) sends zeros and buf[3] = 1.
__global__ __launch_bounds__(TPB) void k_sep_stage(const double *__restrict__ part_v, const double *__restrict__ part_d, int np,
                                                   const double *__restrict__ obj_part, int nobj, const double *scal, Guard g,
                                                   int with_obj, double *buf, SepExtra ex) {
    __shared__ double sh[12];
    const Gate gt = gate_load(g);
    const double *const pp[3] = {part_v, part_d, obj_part ? obj_part : part_v};
    const int nn[3] = {np, np, obj_part ? nobj : 0};
    double t3[3];
    private_partials_n<3>(pp, nn, t3);
    block_sum_n<3>(t3, sh);
    if (threadIdx.x == 0) {
        const bool open = GATE_OPEN;
        buf[0] = open ? t3[0] : 0.0;
        buf[1] = open ? t3[1] : 0.0;
        buf[2] = (open && with_obj) ? (obj_part ? t3[2] : scal[2]) : 0.0; // (several cones: k_finalize has summed into scal[2])
        buf[3] = open ? 0.0 : 1.0;
        for (int k = 0; k < ex.n; ++k) buf[4 + k] = *ex.p[k]; // (local scalars of the caller that ride on the same collective)
    }
}
// k_sep_stage for ranks whose HOSTS sum the scalars (lorads_hip_set_scalar_exchange): the same four local numbers, left in the
// control block (loc = scal + SX_WORD) for the hand-over kernel that follows
__global__ __launch_bounds__(TPB) void k_sep_stage_local(const double *__restrict__ part_v, const double *__restrict__ part_d, int np,
                                                         const double *__restrict__ obj_part, int nobj, const double *scal, Guard g,
                                                         int with_obj, double *loc) {
    __shared__ double sh[12];
    const Gate gt = gate_load(g);
    const double *const pp[3] = {part_v, part_d, obj_part ? obj_part : part_v};
    const int nn[3] = {np, np, obj_part ? nobj : 0};
    double t3[3];
    private_partials_n<3>(pp, nn, t3);
    block_sum_n<3>(t3, sh);
    if (threadIdx.x == 0) {
        const bool open = GATE_OPEN;
        loc[0] = open ? t3[0] : 0.0;
        loc[1] = open ? t3[1] : 0.0;
        loc[2] = (open && with_obj) ? (obj_part ? t3[2] : scal[2]) : 0.0;
        loc[3] = open ? 0.0 : 1.0;
    }
}
__global__ void k_fill_from(size_t len, const double *src, double *__restrict__ dst) {
    const double v = *src;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) dst[i] = v;
}
__global__ void k_sep_commit(const double *buf, double *scal, int with_obj, SepExtra ex) {
    if (threadIdx.x != 0) return;
    scal[0] = buf[0];
    scal[1] = buf[1];
    if (with_obj) scal[2] = buf[2];
    scal[5] = buf[3];
    for (int k = 0; k < ex.n; ++k) *ex.p[k] = buf[4 + k];
}
// phase-1 step with the line-search result: y_head = -Grad (setAsNegGrad), R += tau D (ALMupdateVar) and
// constrValSum += tau q1 + tau^2 q2 (lorads_alm.c:583-598,619-648,1122-1124) in one pass
// sd.ptr != null (Block::sv_direct: every touched entry of the union pattern belongs to ONE constraint): the thread that steps a
// constraint's constrValSum also forms its weight (-lambda - rho b) + rho constrValSum (lorads_alm.c:22-26, as weight_of forms it) and
// writes the coefficients cbase + weight a of the constraint's entries (as k_sval forms them): k_sval is not launched
struct SvDirect {
    const int *ptr, *e;
    const double *a, *cbase;
    double *S;
    const int *row_idx;
    const double *b, *lambda;
    double rho;
    int nrow;
};
__global__ __launch_bounds__(TPB) void k_alm_update(size_t len, double tau, const double *__restrict__ G,
                                                    const double *__restrict__ D, double *__restrict__ y, double *__restrict__ R,
                                                    int m, const double *__restrict__ q1, const double *__restrict__ q2,
                                                    double *__restrict__ csum, SvDirect sd) {
    const size_t gid = (size_t)blockIdx.x * TPB + threadIdx.x, stride = (size_t)gridDim.x * TPB;
    const size_t n2 = len / 2;
    for (size_t i = gid; i < n2; i += stride) {
        const double2 gg = ((const double2 *)G)[i], d = ((const double2 *)D)[i];
        double2 rr = ((double2 *)R)[i], yy;
        yy.x = -1.0 * gg.x; yy.y = -1.0 * gg.y;
        rr.x += tau * d.x; rr.y += tau * d.y;
        ((double2 *)y)[i] = yy;
        ((double2 *)R)[i] = rr;
    }
    if ((len & 1) && gid == 0) {
        y[len - 1] = -1.0 * G[len - 1];
        R[len - 1] += tau * D[len - 1];
    }
    if (sd.ptr) { // (the cone sees every constraint once: its local constraints are a permutation of the m global ones)
        for (size_t i = gid; i < (size_t)sd.nrow; i += stride) {
            const int g = sd.row_idx[i];
            const double cs = csum[g] + tau * q1[g];
            const double cs2 = cs + (tau * tau) * q2[g];
            csum[g] = cs2;
            const double rho = sd.rho;
            const double w = (-sd.lambda[g] - rho * sd.b[g]) + rho * cs2;
            for (int t = sd.ptr[i]; t < sd.ptr[i + 1]; ++t) {
                const int e = sd.e[t];
                double s = sd.cbase[e];
                s += w * sd.a[t];
                sd.S[e] = s;
            }
        }
        return;
    }
    for (size_t i = gid; i < (size_t)m; i += stride) {
        const double cs = csum[i] + tau * q1[i];
        csum[i] = cs + (tau * tau) * q2[i];
    }
}
// one workgroup closes the inner iteration: lagNormSq, beta of the new history pair, primal residual and b.lambda,
// all from partials
__global__ __launch_bounds__(TPB) void k_alm_tail(const double *__restrict__ lag_part, int nlag, double *lag_out,
                                                  const double *__restrict__ ys_part, int nys, double *beta_out,
                                                  const double *__restrict__ part_v, const double *__restrict__ part_d, int np,
                                                  double *out) {
    __shared__ double sh[16];
    const double *const pp[4] = {lag_part, ys_part, part_v, part_d};
    const int nn[4] = {nlag, nys, np, np};
    double t4[4];
    private_partials_n<4>(pp, nn, t4); // (the four sets of loads fly together; each sum as sum_partials takes it)
    block_sum_n<4>(t4, sh);
    const double lag = t4[0], ys = t4[1], v = t4[2], d = t4[3];
    if (threadIdx.x == 0) { *lag_out = 1.0 * lag; if (nys > 0) *beta_out = 1.0 / ys; out[0] = v; out[1] = d; } // (nys == 0: the pair's beta has been formed elsewhere)
}
// lambda += rho b - rho csum
__global__ void k_dual_update(int m, DS rho_s, const double *__restrict__ b, const double *__restrict__ csum,
                              double *__restrict__ lambda) {
    const double rho = dsv(rho_s);
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) { double l = lambda[i] + rho * b[i]; lambda[i] = l + (-rho) * csum[i]; }
}
// csum += tau q1 + tau^2 q2
__global__ void k_csum_step(int m, double tau, const double *__restrict__ q1, const double *__restrict__ q2,
                            double *__restrict__ csum) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) { double c = csum[i] + tau * q1[i]; csum[i] = c + (tau * tau) * q2[i]; }
}
// Line search sums (lorads_alm.c:164-172).  With q0 = (b - csum) + lambda / rho the five dots are
//   ||q2||^2, q1.q2, ||q1||^2, q0.q2, q0.q1;  the rho-free pieces are accumulated as SEVEN partial sums per workgroup
//   {q2.q2, q1.q2, q1.q1, (b-csum).q2, lambda.q2, (b-csum).q1, lambda.q1}  (slot k at part + k * pstride, pstride = the capacity of a partial-sum slot)
// either by the kernel that produces q1, q2 (k_cv_rd) or by k_linesearch_part; k_linesearch adds them up.
constexpr int LS_NSUM = 7;
__device__ __forceinline__ void ls_accumulate(double (&s)[LS_NSUM], double a1, double a2, double bc, double lam) {
    s[0] += a2 * a2; s[1] += a1 * a2; s[2] += a1 * a1; s[3] += bc * a2; s[4] += lam * a2; s[5] += bc * a1; s[6] += lam * a1;
}
__global__ __launch_bounds__(TPB) void k_cv_rd(int nrow, const int *__restrict__ a_ptr, const int *__restrict__ a_e,
                                               const double *__restrict__ a_val, const double *__restrict__ T1,
                                               const double *__restrict__ T2, double *__restrict__ cv,
                                               const int *__restrict__ row_idx, double *__restrict__ vec1,
                                               double *__restrict__ vec2, const double *__restrict__ b,
                                               const double *__restrict__ csum, const double *__restrict__ lambda,
                                               double *__restrict__ part, int pstride) {
    __shared__ double sh[4 * LS_NSUM];
    const int lane = threadIdx.x & 7, per = TPB / 8;
    double acc[LS_NSUM] = {0, 0, 0, 0, 0, 0, 0};
    for (int i0 = blockIdx.x * per; i0 < nrow; i0 += gridDim.x * per) {
        const int i = i0 + threadIdx.x / 8;
        const bool act = i < nrow;
        double s1 = 0.0, s2 = 0.0;
        if (act)
            for (int t = a_ptr[i] + lane; t < a_ptr[i + 1]; t += 8) {
                const int e = a_e[t];
                const double a = a_val[t];
                s1 += a * T1[e];
                s2 += a * T2[e];
            }
        s1 = group_sum<8>(s1);
        s2 = group_sum<8>(s2);
        if (act && lane == 0) {
            const int gi = row_idx[i];
            const double a1 = s1 * 2.0, a2 = s2 * 1.0;
            vec1[gi] = a1;
            vec2[gi] = a2;
            cv[i] = s2;
            ls_accumulate(acc, a1, a2, b[gi] - csum[gi], lambda[gi]);
        }
    }
    block_sum_n<LS_NSUM>(acc, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < LS_NSUM; ++k) part[(size_t)k * pstride + blockIdx.x] = acc[k];
}
__global__ __launch_bounds__(TPB) void k_linesearch_part(int m, const double *__restrict__ b, const double *__restrict__ csum,
                                                         const double *__restrict__ lambda, const double *__restrict__ q1,
                                                         const double *__restrict__ q2, double *__restrict__ part, int pstride) {
    __shared__ double sh[4 * LS_NSUM];
    double s[LS_NSUM] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = blockIdx.x * TPB + threadIdx.x; i < m; i += gridDim.x * TPB) ls_accumulate(s, q1[i], q2[i], b[i] - csum[i], lambda[i]);
    block_sum_n<LS_NSUM>(s, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < LS_NSUM; ++k) part[(size_t)k * pstride + blockIdx.x] = s[k];
}
// one workgroup: out[0..4] = the five dots, out[5], out[6] = p1, p2 -- taken from the q12 tail or, when the objective
// partials are handed over (fused step), summed here and stored in both places
__global__ __launch_bounds__(TPB) void k_linesearch(int m, double rinv, const double *__restrict__ part, int np, double *q12,
                                                    double *__restrict__ out, const double *__restrict__ part1,
                                                    const double *__restrict__ part2, int npart, int pstride) {
    __shared__ double sh[4 * (LS_NSUM + 2)];
    // all nine sets of partials are requested together and reduced with one barrier pair (each sum as sum_partials takes it)
    const double *pp[LS_NSUM + 2];
    int nn[LS_NSUM + 2];
    double t[LS_NSUM + 2];
#pragma unroll
    for (int k = 0; k < LS_NSUM; ++k) { pp[k] = part + (size_t)k * pstride; nn[k] = np; }
    pp[LS_NSUM] = part1 ? part1 : part; nn[LS_NSUM] = part1 ? npart : 0;
    pp[LS_NSUM + 1] = part1 ? part2 : part; nn[LS_NSUM + 1] = part1 ? npart : 0;
    {
        const double *const(&ppc)[LS_NSUM + 2] = pp;
        const int(&nnc)[LS_NSUM + 2] = nn;
        private_partials_n<LS_NSUM + 2>(ppc, nnc, t);
    }
    block_sum_n<LS_NSUM + 2>(t, sh);
    if (part1) {
        if (threadIdx.x == 0) {
            out[5] = q12[2 * (size_t)m] = 2.0 * t[LS_NSUM];
            out[6] = q12[2 * (size_t)m + 1] = 1.0 * t[LS_NSUM + 1];
        }
    } else if (threadIdx.x == 0) {
        out[5] = q12[2 * (size_t)m];
        out[6] = q12[2 * (size_t)m + 1];
    }
    const double *s = t;
    if (threadIdx.x == 0) {
        out[0] = s[0]; out[1] = s[1]; out[2] = s[2];
        out[3] = s[3] + rinv * s[4];
        out[4] = s[5] + rinv * s[6];
    }
}

