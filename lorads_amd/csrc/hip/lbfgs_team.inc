// lbfgs_team.inc -- the L-BFGS part of a phase-1 inner iteration as ONE launch (single rank, history length <= 2).
//
// Reference: setlbfgsHisTwo + LBFGSDirection + LBFGSDirectionUseGrad (src_semi/lorads_alg/lorads_alm.c:230-391,469-489,540-560):
//   s_new = tau D, y_new = y_new + Grad (y_new holds -Grad_old), beta_new = 1 / <y_new, s_new>;
//   q = Grad;  newest -> oldest: alpha_i = beta_i <s_i, q>, q -= alpha_i y_i;  oldest -> newest: q += (alpha_i - beta_i <y_i, q>) s_i;
//   D = -q;  D = -Grad if <D, Grad> >= 0.
// Launch by launch (lorads_hip_set_lbfgs_his_two + lorads_hip_lbfgs_direction) that is k_his_two_dot, 2 nn + 1 launches of
// k_lbfgs_stage and k_use_grad_p: 2 nn + 3 launches whose vectors (q, the history) go through memory 27 times at nn = 2, each launch
// waiting for the previous one's global sum.  Here a team of resident workgroups keeps q and the NEW pair (s, y) -- which it has just
// formed -- in registers, streams only the older pair, and takes the 2 nn + 1 global sums as in-kernel all-reduces (persist.inc:
// team_allreduce, the same tagged granules, bounded spins, placement check): 10 vector passes instead of 27, one launch instead of
// 2 nn + 3.  Per element the same operations in the same order as k_his_two_dot / k_lbfgs_stage / k_use_grad_p (the dots are summed
// in another order: 1e-16 of their scale).  Everything in memory is left as the launch-by-launch form leaves it (s, y, D, alpha,
// beta), so the two forms can be mixed call by call (tests/test_lbfgs_team.py).

struct LTArgs {
    size_t n2;                 // vector length in pairs of doubles
    double tau;
    const double *G;           // the gradient at the new point
    double *D;                 // in: the step's direction; out: the next direction
    double *s1, *y1;           // the new history pair (y1 holds -Grad_old on entry)
    const double *s2, *y2;     // the older pair (nn == 2)
    double *ab1, *ab2;         // {alpha, beta} of the two nodes
    int nn;                    // pairs the direction uses: 1 or 2
    const PMap *wg_map;
    unsigned long long *slA, *slF, *slX, *slB;
    int G_team, nsub;
    unsigned int tag0;
    int *abort_flag;
    int allow_l2;
    double *abort_out;         // 1.0 if the team gave up, else 0.0 (read with the iteration's scalars)
};

// 16 bytes of a vector through a buffer descriptor: ONE 32-bit offset register per thread serves all of its slices (the slice is the
// scalar offset), and a slice past the end reads zeros / stores nothing by the descriptor's range check -- no masks, no 64-bit
// address per slice and vector (which at 8 slices cost more registers than the data)
__device__ __forceinline__ double2 lt_ld(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
    const pk_d2 t = __builtin_bit_cast(pk_d2, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, (int)soff, 0));
    double2 r;
    r.x = t.x; r.y = t.y;
    return r;
}
__device__ __forceinline__ void lt_st(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, double2 v) {
    pk_d2 t;
    t.x = v.x; t.y = v.y;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(pk_v4u, t), rs, (int)voff, (int)soff, 0);
}

template <int NP>
__global__ __launch_bounds__(TPB) void k_lbfgs_team(LTArgs A) {
    __shared__ double sh[68];
    const PMap mp = A.wg_map[blockIdx.x];
    PTeam T;
    T.slA = A.slA; T.slF = A.slF; T.slX = A.slX; T.slB = A.slB;
    T.G = A.G_team; T.wl = mp.wl; T.si = mp.si; T.ssz = mp.ssz; T.sid = mp.sid; T.nsub = A.nsub; T.soff = mp.soff;
    T.tag = A.tag0; T.abort_flag = A.abort_flag; T.l2 = 0;
    T.dead = __hip_atomic_load(A.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ? 1 : 0;
    const int xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 7; // hwreg(HW_REG_XCC_ID, 0, 4): see k_admm_diag
    const double dplace = (double)((xcc - mp.cls) & 7);
    const unsigned vbytes = (unsigned)(A.n2 * 16);
    const __amdgpu_buffer_rsrc_t rG = __builtin_amdgcn_make_buffer_rsrc((void *)A.G, 0, vbytes, 0x00020000),
                                 rD = __builtin_amdgcn_make_buffer_rsrc((void *)A.D, 0, vbytes, 0x00020000),
                                 rS1 = __builtin_amdgcn_make_buffer_rsrc((void *)A.s1, 0, vbytes, 0x00020000),
                                 rY1 = __builtin_amdgcn_make_buffer_rsrc((void *)A.y1, 0, vbytes, 0x00020000),
                                 rS2 = __builtin_amdgcn_make_buffer_rsrc((void *)A.s2, 0, vbytes, 0x00020000),
                                 rY2 = __builtin_amdgcn_make_buffer_rsrc((void *)A.y2, 0, vbytes, 0x00020000);
    // this thread's slices: pairs (block * NP + u) * TPB + thread, u < NP; a block whose pairs lie past the end asks past the range
    const unsigned long long first = ((unsigned long long)blockIdx.x * NP * TPB + threadIdx.x) * 16ull;
    const unsigned voff = first < vbytes ? (unsigned)first : vbytes; // (+ slice offset: past the range, never wrapping: see lteam_build)
    constexpr unsigned SL = TPB * 16u; // bytes between a thread's slices
    const double tau = A.tau;
    double2 q[NP], s1[NP], y1[NP];
    // ---- the new pair (setlbfgsHisTwo) and the first dot of the recursion, <s_new, Grad>
    double two[4] = {0.0, 0.0, threadIdx.x == 0 ? dplace : 0.0, threadIdx.x == 0 ? dplace * dplace : 0.0};
    // (the loads of UB slices fly together; more at once would cost the registers that keep every workgroup of the team resident)
    constexpr int UB = NP <= 4 ? NP : 2;
#pragma unroll
    for (int u0 = 0; u0 < NP; u0 += UB) {
        double2 d[UB], g[UB], yo[UB];
#pragma unroll
        for (int v = 0; v < UB; ++v) {
            d[v] = lt_ld(rD, voff, (u0 + v) * SL); g[v] = lt_ld(rG, voff, (u0 + v) * SL); yo[v] = lt_ld(rY1, voff, (u0 + v) * SL);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int v = 0; v < UB; ++v) {
            const int u = u0 + v;
            double2 si, yi;
            si.x = tau * d[v].x; yi.x = yo[v].x + g[v].x;
            si.y = tau * d[v].y; yi.y = yo[v].y + g[v].y;
            lt_st(rS1, voff, u * SL, si);
            lt_st(rY1, voff, u * SL, yi);
            two[0] += yi.x * si.x;
            two[0] += yi.y * si.y;
            two[1] += si.x * g[v].x;
            two[1] += si.y * g[v].y;
            s1[u] = si; y1[u] = yi; q[u] = g[v];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    team_allreduce<4>(T, two, sh, false);
    if (A.allow_l2 && T.G > 1 && (double)T.G * two[3] == two[2] * two[2]) T.l2 = 1; // every workgroup where round-robin dealing puts it
    const double beta1 = 1.0 / two[0];
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    if (writer) A.ab1[1] = beta1;
    double dot = two[1];
    // ---- first loop, newest -> oldest
    const double alpha1 = beta1 * dot;
    if (writer) A.ab1[0] = alpha1;
    double alpha2 = 0.0, beta2 = 0.0;
    {
        const double coef = -1 * alpha1;
        double one[1] = {0.0};
        if (A.nn == 2) { // q -= alpha_1 y_1, then <s_2, q>
#pragma unroll
            for (int u0 = 0; u0 < NP; u0 += UB) {
                double2 dv[UB];
#pragma unroll
                for (int v = 0; v < UB; ++v) dv[v] = lt_ld(rS2, voff, (u0 + v) * SL);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int v = 0; v < UB; ++v) {
                    const int u = u0 + v;
                    q[u].x = q[u].x + coef * y1[u].x;
                    q[u].y = q[u].y + coef * y1[u].y;
                    one[0] += dv[v].x * q[u].x;
                    one[0] += dv[v].y * q[u].y;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else { // nn == 1: q -= alpha_1 y_1, then <y_1, q>
#pragma unroll
            for (int u = 0; u < NP; ++u) {
                q[u].x = q[u].x + coef * y1[u].x;
                q[u].y = q[u].y + coef * y1[u].y;
                one[0] += y1[u].x * q[u].x;
                one[0] += y1[u].y * q[u].y;
            }
        }
        team_allreduce<1>(T, one, sh, false);
        dot = one[0];
    }
    if (A.nn == 2) {
        beta2 = A.ab2[1];
        alpha2 = beta2 * dot;
        if (writer) A.ab2[0] = alpha2;
        { // q -= alpha_2 y_2, then <y_2, q>
            const double coef = -1 * alpha2;
            double one[1] = {0.0};
#pragma unroll
            for (int u0 = 0; u0 < NP; u0 += UB) {
                double2 ax[UB];
#pragma unroll
                for (int v = 0; v < UB; ++v) ax[v] = lt_ld(rY2, voff, (u0 + v) * SL);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int v = 0; v < UB; ++v) {
                    const int u = u0 + v;
                    q[u].x = q[u].x + coef * ax[v].x;
                    q[u].y = q[u].y + coef * ax[v].y;
                    one[0] += ax[v].x * q[u].x;
                    one[0] += ax[v].y * q[u].y;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            team_allreduce<1>(T, one, sh, false);
            dot = one[0];
        }
        { // second loop, oldest first: q += (alpha_2 - beta_2 <y_2, q>) s_2, then <y_1, q>
            const double coef = alpha2 - beta2 * dot;
            double one[1] = {0.0};
#pragma unroll
            for (int u0 = 0; u0 < NP; u0 += UB) {
                double2 ax[UB];
#pragma unroll
                for (int v = 0; v < UB; ++v) ax[v] = lt_ld(rS2, voff, (u0 + v) * SL);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int v = 0; v < UB; ++v) {
                    const int u = u0 + v;
                    q[u].x = q[u].x + coef * ax[v].x;
                    q[u].y = q[u].y + coef * ax[v].y;
                    one[0] += y1[u].x * q[u].x;
                    one[0] += y1[u].y * q[u].y;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            team_allreduce<1>(T, one, sh, false);
            dot = one[0];
        }
    }
    // ---- the newest pair closes the second loop: q += (alpha_1 - beta_1 <y_1, q>) s_1, D = -q, <D, Grad>
    {
        const double coef = alpha1 - beta1 * dot;
        double one[1] = {0.0};
#pragma unroll
        for (int u0 = 0; u0 < NP; u0 += UB) {
            double2 g[UB];
#pragma unroll
            for (int v = 0; v < UB; ++v) g[v] = lt_ld(rG, voff, (u0 + v) * SL);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int v = 0; v < UB; ++v) {
                const int u = u0 + v;
                const double vx = q[u].x + coef * s1[u].x, vy = q[u].y + coef * s1[u].y;
                q[u].x = -1.0 * vx; // (q becomes D)
                q[u].y = -1.0 * vy;
                one[0] += q[u].x * g[v].x;
                one[0] += q[u].y * g[v].y;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        team_allreduce<1>(T, one, sh, false);
        dot = one[0];
    }
    if (dot >= 0) { // (LBFGSDirectionUseGrad: rare; the gradient is read once more)
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const double2 g = lt_ld(rG, voff, u * SL);
            q[u].x = -g.x; q[u].y = -g.y;
        }
    }
#pragma unroll
    for (int u = 0; u < NP; ++u) lt_st(rD, voff, u * SL, q[u]);
    if (writer) *A.abort_out = T.dead ? 1.0 : 0.0;
}

// ---- the rest of the fused inner iteration around that launch (single rank, one sparse cone that sees every constraint).  Once the
// next direction D exists BEFORE the step's residual is taken, the step's A(R R^T) and the next line search's A(sym(R D^T)),
// A(D D^T) can share every visit: one pass over the constraint pattern for the three pair dots, one pass over the constraints for
// the three constraint values (k_pairdots + k_pairdots_rd and k_cv_res + k_cv_rd in the launch-by-launch form), and ONE closing
// workgroup for all the sums and the hand-over (k_alm_tail + k_linesearch + k_publish).
// T0 = sym-pair(R, R), T1 = sym-pair(R, D), T2 = sym-pair(D, D), each summed exactly as pair_dot / pair_dot_rd sum them
struct CvFold { // k_pairdots_rrd doing k_cv_res_rd's work for cones whose constraints have one entry each (null e_ptr: off)
    const int *e_ptr, *e_con;      // pattern entry -> its constraints (local index; sign bit: owner mark), coefficient
    const double *e_val;
    const int *row_idx;
    double *cv, *csum, *q1, *q2;
    const double *b, *lambda;
    double *part_v, *part_d, *part_ls;
    int pstride;
};
// (the first g1 workgroups; the others take k_obj_rd's part, the objective's pair sums p1, p2 of the same line search -- the two
// passes read the same factors and neither needs the other: one launch)
template <int LG, bool V2, int NS>
__global__ __launch_bounds__(TPB) void k_pairdots_rrd(int ne, const int *__restrict__ erow, const int *__restrict__ ecol,
                                                      const double *__restrict__ R, const double *__restrict__ D, int r,
                                                      double *__restrict__ T0, double *__restrict__ T1, double *__restrict__ T2, int g1,
                                                      int nc, const int *__restrict__ c_row, const int *__restrict__ c_col,
                                                      const double *__restrict__ c_val, double *__restrict__ part1,
                                                      double *__restrict__ part2, CvFold cf) {
    constexpr int W = V2 ? 2 : 1;
    if ((int)blockIdx.x >= g1) { // k_obj_rd on the remaining workgroups
        __shared__ double sh[4];
        const int lane = threadIdx.x % LG, per = TPB / LG, bid = blockIdx.x - g1, nblk = gridDim.x - g1;
        double s1 = 0.0, s2 = 0.0;
        for (int e = bid * per + threadIdx.x / LG; e < nc; e += nblk * per) {
            double t1, t2;
            pair_dot_rd<LG, V2, NS>(R, D, c_row[e], c_col[e], r, lane, t1, t2);
            s1 += t1 * c_val[e];
            s2 += t2 * c_val[e];
        }
        const double u1 = block_sum(s1, sh), u2 = block_sum(s2, sh);
        if (threadIdx.x == 0) { part1[bid] = u1; part2[bid] = u2; }
        return;
    }
    const int e = (blockIdx.x * TPB + threadIdx.x) / LG, lane = threadIdx.x % LG;
    const bool act = e < ne;
    const int p = act ? erow[e] : 0, q = act ? ecol[e] : 0;
    double rp[NS][W], rq[NS][W], dp[NS][W], dq[NS][W];
    Slice<LG, V2, NS>::load(R + (size_t)p * r, r, lane, rp);
    Slice<LG, V2, NS>::load(D + (size_t)q * r, r, lane, dq);
    Slice<LG, V2, NS>::load(R + (size_t)q * r, r, lane, rq);
    Slice<LG, V2, NS>::load(D + (size_t)p * r, r, lane, dp);
    double c1 = 0.0, c2 = 0.0, a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int c = 0; c < NS; ++c)
#pragma unroll
        for (int w = 0; w < W; ++w) {
            c1 += rp[c][w] * rq[c][w]; c2 += rq[c][w] * rp[c][w];
            a1 += rp[c][w] * dq[c][w]; a2 += rq[c][w] * dp[c][w];
            b1 += dp[c][w] * dq[c][w]; b2 += dq[c][w] * dp[c][w];
        }
    double t0 = p == q ? c1 : c1 + c2, t1 = p == q ? a1 : a1 + a2, t2 = p == q ? b1 : b1 + b2;
    t0 = group_sum<LG>(t0);
    t1 = group_sum<LG>(t1);
    t2 = group_sum<LG>(t2);
    if (!cf.e_ptr) {
        if (act && lane == 0) { T0[e] = t0; T1[e] = t1; T2[e] = t2; }
        return;
    }
    // Every constraint of the cone has exactly ONE entry (Max-Cut-type and single-entry cones): k_cv_res_rd's pass over the
    // constraints is bookkeeping of this entry's three values -- done here, by the lane that holds them, for the entry's constraints
    // (s = 0 + a T: the value k_cv_res_rd forms for a constraint with one entry, bit for bit); the pair-dot arrays are never written
    __shared__ double sh9[4 * (LS_NSUM + 2)];
    double acc[LS_NSUM + 2] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (act && lane == 0) {
        for (int t = cf.e_ptr[e]; t < cf.e_ptr[e + 1]; ++t) {
            const int i = cf.e_con[t] & 0x7fffffff;
            const double a = cf.e_val[t];
            const double s0 = a * t0, s1 = a * t1, s2 = a * t2;
            const int gi = cf.row_idx[i];
            const double w = s0 * 1.0, bi = cf.b[gi], lam = cf.lambda[gi], tt = bi - w;
            const double a1 = s1 * 2.0, a2 = s2 * 1.0;
            cf.csum[gi] = w;
            cf.q1[gi] = a1;
            cf.q2[gi] = a2;
            cf.cv[i] = s2;
            double ls[LS_NSUM] = {acc[0], acc[1], acc[2], acc[3], acc[4], acc[5], acc[6]};
            ls_accumulate(ls, a1, a2, tt, lam);
#pragma unroll
            for (int k = 0; k < LS_NSUM; ++k) acc[k] = ls[k];
            acc[LS_NSUM] += tt * tt;
            acc[LS_NSUM + 1] += bi * lam;
        }
    }
    block_sum_n<LS_NSUM + 2>(acc, sh9);
    if (threadIdx.x == 0) {
        for (int k = 0; k < LS_NSUM; ++k) cf.part_ls[(size_t)k * cf.pstride + blockIdx.x] = acc[k];
        cf.part_v[blockIdx.x] = acc[LS_NSUM];
        cf.part_d[blockIdx.x] = acc[LS_NSUM + 1];
    }
}
// per constraint: constrValSum_i = cv... = sum a T0 (k_cv_res: the step's A(R R^T), its residual partials), q1_i = 2 sum a T1,
// q2_i = sum a T2 (k_cv_rd: cv keeps the last one; the seven line-search partials, which see the NEW constrValSum)
__global__ __launch_bounds__(TPB) void k_cv_res_rd(int nrow, const int *__restrict__ a_ptr, const int *__restrict__ a_e,
                                                   const double *__restrict__ a_val, const double *__restrict__ T0,
                                                   const double *__restrict__ T1, const double *__restrict__ T2, double *__restrict__ cv,
                                                   const int *__restrict__ row_idx, double *__restrict__ csum, double *__restrict__ q1,
                                                   double *__restrict__ q2, const double *__restrict__ b, const double *__restrict__ lambda,
                                                   double *__restrict__ part_v, double *__restrict__ part_d, double *__restrict__ part_ls,
                                                   int pstride) {
    __shared__ double sh[4 * (LS_NSUM + 2)];
    const int lane = threadIdx.x & 7, per = TPB / 8;
    double acc[LS_NSUM + 2] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // the seven line-search sums, then sum (b - w)^2 and b.lambda
    for (int i0 = blockIdx.x * per; i0 < nrow; i0 += gridDim.x * per) {
        const int i = i0 + threadIdx.x / 8;
        const bool act = i < nrow;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (act)
            for (int t = a_ptr[i] + lane; t < a_ptr[i + 1]; t += 8) {
                const int e = a_e[t];
                const double a = a_val[t];
                s0 += a * T0[e];
                s1 += a * T1[e];
                s2 += a * T2[e];
            }
        s0 = group_sum<8>(s0);
        s1 = group_sum<8>(s1);
        s2 = group_sum<8>(s2);
        if (act && lane == 0) {
            const int gi = row_idx[i];
            const double w = s0 * 1.0, bi = b[gi], lam = lambda[gi], t = bi - w;
            const double a1 = s1 * 2.0, a2 = s2 * 1.0;
            csum[gi] = w;
            q1[gi] = a1;
            q2[gi] = a2;
            cv[i] = s2;
            double ls[LS_NSUM] = {acc[0], acc[1], acc[2], acc[3], acc[4], acc[5], acc[6]};
            ls_accumulate(ls, a1, a2, t, lam);
#pragma unroll
            for (int k = 0; k < LS_NSUM; ++k) acc[k] = ls[k];
            acc[LS_NSUM] += t * t;
            acc[LS_NSUM + 1] += bi * lam;
        }
    }
    block_sum_n<LS_NSUM + 2>(acc, sh);
    if (threadIdx.x == 0) {
        for (int k = 0; k < LS_NSUM; ++k) part_ls[(size_t)k * pstride + blockIdx.x] = acc[k];
        part_v[blockIdx.x] = acc[LS_NSUM];
        part_d[blockIdx.x] = acc[LS_NSUM + 1];
    }
}
// one workgroup closes the fused inner iteration: ||Grad||^2 (scal[8]), the residual sums (scal[0], scal[1]), the line search's five
// dots and p1, p2 (scal[16..22], q12's tail) -- k_alm_tail and k_linesearch, each sum taken as sum_partials takes it -- and then
// the hand-over of k_publish
struct AlmCloseArgs {
    const double *lag_part; int nlag;
    const double *part_v, *part_d; int nres;
    const double *part_ls; int nls, pstride;
    const double *obj1, *obj2; int nobj;
    double rinv;
    double *scal, *q12_tail;
};
__global__ __launch_bounds__(TPB) void k_alm_close(AlmCloseArgs a, const unsigned long long *__restrict__ src, int nwords,
                                                   unsigned long long *dst, unsigned long long *flag, unsigned long long *seq_dev) {
    __shared__ double sh[4 * (LS_NSUM + 5)];
    __shared__ double shv[10];
    constexpr int NA = LS_NSUM + 5;
    // (src = the control block from word 0 = the device scalars, nwords <= TPB: a word per thread, requested at the top; the ten
    // scalars formed here go to the host mirror straight from LDS -- no fence and re-read between the sums and the hand-over)
    const unsigned long long seq = *seq_dev + 1;
    const unsigned long long pre = __builtin_nontemporal_load(src + ((int)threadIdx.x < nwords ? (int)threadIdx.x : 0));
    const double *pp[NA];
    int nn[NA];
    double t[NA];
#pragma unroll
    for (int k = 0; k < LS_NSUM; ++k) { pp[k] = a.part_ls + (size_t)k * a.pstride; nn[k] = a.nls; }
    pp[LS_NSUM] = a.obj1; nn[LS_NSUM] = a.nobj;
    pp[LS_NSUM + 1] = a.obj2; nn[LS_NSUM + 1] = a.nobj;
    pp[LS_NSUM + 2] = a.lag_part; nn[LS_NSUM + 2] = a.nlag;
    pp[LS_NSUM + 3] = a.part_v; nn[LS_NSUM + 3] = a.nres;
    pp[LS_NSUM + 4] = a.part_d; nn[LS_NSUM + 4] = a.nres;
    {
        const double *const(&ppc)[NA] = pp;
        const int(&nnc)[NA] = nn;
        private_partials_n<NA>(ppc, nnc, t);
    }
    block_sum_n<NA>(t, sh);
    if (threadIdx.x == 0) {
        double *out = a.scal + 16;
        double v[10];
        v[0] = t[LS_NSUM + 3];            // scal[0]: sum (b - A(R R^T))^2
        v[1] = t[LS_NSUM + 4];            // scal[1]: b.lambda
        v[2] = 1.0 * t[LS_NSUM + 2];      // scal[8]: ||Grad||^2
        v[3] = t[0]; v[4] = t[1]; v[5] = t[2];
        v[6] = t[3] + a.rinv * t[4];
        v[7] = t[5] + a.rinv * t[6];
        v[8] = 2.0 * t[LS_NSUM];          // p1
        v[9] = 1.0 * t[LS_NSUM + 1];      // p2
        a.scal[0] = v[0]; a.scal[1] = v[1]; a.scal[8] = v[2];
#pragma unroll
        for (int k = 0; k < 7; ++k) out[k] = v[3 + k];
        a.q12_tail[0] = v[8]; a.q12_tail[1] = v[9];
#pragma unroll
        for (int k = 0; k < 10; ++k) shv[k] = v[k];
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i < nwords) {
        unsigned long long w = pre;
        const int k = i == 0 ? 0 : i == 1 ? 1 : i == 8 ? 2 : (i >= 16 && i <= 22) ? i - 13 : -1;
        if (k >= 0) w = (unsigned long long)__double_as_longlong(shv[k]);
        dst[i] = w;
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        *seq_dev = seq;
        __atomic_store_n(flag, seq, __ATOMIC_RELEASE);
        __threadfence_system();
    }
}

struct LTeamPlan {
    bool valid = false, failed = false;
    size_t len = 0;
    int np = 0, grid = 0, nsub = 0;
    PMap *d_map = nullptr;
    unsigned long long *gran = nullptr;
    size_t gran_words = 0, offA = 0, offF = 0, offX = 0, offB = 0;
    int *abort_flag = nullptr;
    unsigned int tag = 0;
    long long launches = 0;
    double *t0 = nullptr;      // sym-pair(R, R) of the fused iteration's pattern pass (k_pairdots_rrd), t0_len entries
    size_t t0_len = 0;
    DevPool mem;
    void release() {
        mem.release();
        d_map = nullptr; gran = nullptr; abort_flag = nullptr; t0 = nullptr; t0_len = 0;
        valid = false;
    }
};

typedef void (*lt_kernel_t)(LTArgs);
inline lt_kernel_t lt_kernel(int np) {
    switch (np) {
    case 1: return k_lbfgs_team<1>;
    case 2: return k_lbfgs_team<2>;
    case 3: return k_lbfgs_team<3>;
    case 4: return k_lbfgs_team<4>;
    case 6: return k_lbfgs_team<6>;
    case 8: return k_lbfgs_team<8>;
    case 12: return k_lbfgs_team<12>;
    }
    return nullptr;
}

int lteam_build(lorads_hip_ctx *c) {
    LTeamPlan &P = *c->lteam;
    P.release();
    P.len = c->all_elem;
    if ((c->all_elem & 1) || c->all_elem * 8 >= (size_t)0xfff00000u) { P.failed = true; return 0; } // (pairs; 32-bit buffer offsets + slice offsets)
    const size_t n2 = c->all_elem / 2;
    int dev = 0, ncu_dev = 0;
    HC(hipGetDevice(&dev));
    HC(hipDeviceGetAttribute(&ncu_dev, hipDeviceAttributeMultiprocessorCount, dev)); // (hipGetDeviceProperties takes milliseconds)
    // Pairs per thread and vector: the fewest workgroups that still put one on most compute units -- what a launch costs is its five
    // all-reduces, which grow with the team (rand20000: 131 workgroups 114.8 us per inner iteration, 782: 119.9; matcomp50000: 489
    // workgroups 221.6 us, 977: 227.3; profiles/r04_lteam_np.txt); small vectors: one pair per thread
    const int cand[7] = {12, 8, 6, 4, 3, 2, 1};
    const int force_np = opt_lbfgs_team_np(); // (measurements)
    for (int ci = 0; ci < 7 && !P.valid; ++ci) {
        const int np = cand[ci];
        if (force_np && np != force_np) continue;
        const size_t g = (n2 + (size_t)TPB * np - 1) / ((size_t)TPB * np);
        if (g < 1 || g > (size_t)PK_GMAX) continue;
        if (!force_np && np > 1 && g < 128) continue;
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)lt_kernel(np), TPB, 0) != hipSuccess) { (void)hipGetLastError(); continue; }
        if ((long long)g > (long long)std::min(occ, 4) * ncu_dev) continue; // (every workgroup resident, see persist_build)
        P.np = np; P.grid = (int)g; P.valid = true;
    }
    if (!P.valid) { P.failed = true; return 0; }
    // one team; its sub-teams: the workgroups of one residue class mod 8, in block order (persist_build)
    const int G = P.grid;
    std::vector<PMap> map(G);
    std::vector<std::vector<int>> mem(8);
    for (int b = 0; b < G; ++b) mem[b % 8].push_back(b);
    int sid = 0, soff = 0;
    for (int x = 0; x < 8; ++x) {
        if (mem[x].empty()) continue;
        for (size_t i = 0; i < mem[x].size(); ++i) map[mem[x][i]] = PMap{0, mem[x][i], (int)i, (int)mem[x].size(), sid, soff, x, 0};
        soff += (int)mem[x].size();
        ++sid;
    }
    P.nsub = sid;
    size_t words = 0;
    P.offA = words; words += (size_t)2 * (G + (G + 63) / 64) * PK_SLOTW;
    P.offF = words; words += (size_t)2 * G * PK_SLOTW;
    P.offX = words; words += (size_t)2 * 8 * PK_SLOTW;
    P.offB = words; words += (size_t)2 * 8 * PK_SLOTW;
    if (P.mem.alloc(&P.gran, words) || P.mem.alloc(&P.abort_flag, 1)) return 1;
    P.gran_words = words;
    HC(hipMemset(P.gran, 0, sizeof(unsigned long long) * words));
    HC(hipMemset(P.abort_flag, 0, sizeof(int)));
    if (P.mem.upload(&P.d_map, map)) return 1;
    P.tag = 0;
    if (opt_verbose())
        fprintf(stderr, "lorads_hip: one-launch L-BFGS direction: %d workgroups, %d pairs of doubles per thread and vector\n", P.grid, P.np);
    return 0;
}

// the fused tail's third pair-dot array (0: ready)
int lteam_scratch(lorads_hip_ctx *c, size_t ne) {
    LTeamPlan &P = *c->lteam;
    if (P.t0 && P.t0_len >= ne) return 0;
    P.mem.free(P.t0);
    P.t0_len = 0;
    if (P.mem.alloc(&P.t0, ne)) return 1;
    P.t0_len = ne;
    return 0;
}

// may this inner iteration's history update + next direction run as the one launch?
bool lteam_ready(lorads_hip_ctx *c, int next_inner) {
    if (!c->lteam || !c->opt.lbfgs_team || c->ar || c->L > 2 || next_inner < 1) return false;
    LTeamPlan &P = *c->lteam;
    if ((P.valid || P.failed) && P.len != c->all_elem) { P.release(); P.failed = false; }
    if (P.failed) return false;
    if (!P.valid && lteam_build(c)) { P.failed = true; return false; }
    return P.valid;
}

// setlbfgsHisTwo(tau) and LBFGSDirection(next_inner) in one launch; c->head still names the node that takes the new pair
int launch_lbfgs_team(lorads_hip_ctx *c, double tau, int next_inner) {
    LTeamPlan &P = *c->lteam;
    if (P.tag > 0xffffffffu - 64u) { // (tags about to wrap: start over on a clean slate)
        HC(hipMemsetAsync(P.gran, 0, sizeof(unsigned long long) * P.gran_words, c->stream));
        P.tag = 0;
    }
    const int node1 = c->head, node2 = (c->head - 1 + c->L) % c->L;
    LTArgs A{};
    A.n2 = c->all_elem / 2; A.tau = tau; A.G = c->G; A.D = c->U;
    A.s1 = c->ring[node1].s; A.y1 = c->ring[node1].y;
    A.s2 = c->ring[node2].s; A.y2 = c->ring[node2].y;
    A.ab1 = c->ring_ab + 2 * node1; A.ab2 = c->ring_ab + 2 * node2;
    A.nn = next_inner <= c->L - 1 ? next_inner : c->L;
    A.wg_map = P.d_map;
    A.slA = P.gran + P.offA; A.slF = P.gran + P.offF; A.slX = P.gran + P.offX; A.slB = P.gran + P.offB;
    A.G_team = P.grid; A.nsub = P.nsub; A.tag0 = P.tag; A.abort_flag = P.abort_flag;
    A.allow_l2 = c->opt.persist_l2 ? 1 : 0;
    A.abort_out = c->scal + 7;
    P.tag += 16;
    P.launches++;
    if (c->shared_gpu_fd >= 0) flock(c->shared_gpu_fd, LOCK_EX); // (several processes on one card: see run_sweep_persist)
    ++c->n_launch;
    hipLaunchKernelGGL(lt_kernel(P.np), dim3(P.grid), dim3(TPB), 0, c->stream, A);
    if (c->shared_gpu_fd >= 0) {
        (void)hipStreamSynchronize(c->stream);
        flock(c->shared_gpu_fd, LOCK_UN);
    }
    c->merged.t_uv_valid = false;
    for (auto &B : c->blk) B.t_uv_valid = false; // U is overwritten by the direction D
    return 0;
}
