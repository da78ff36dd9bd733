// solution.inc -- export of the primal-dual point and its DIMACS certificate, included by lorads_hip.hip after lanczos.inc.
//
// The exported point (DESIGN.md "Exporting a solution"): X_k = R_k R_k^T per cone with R = (U + V) / 2 (phase 2) or R itself
// (phase 1), x_j = r_j^2 on the LP block, the multipliers lambda (with a dual update still waiting for a carrier applied to a COPY)
// and S_k = C_k - sum_i lambda_i A_ik.  Everything here is read-only on the solver's state: R is formed on the fly from the rows of
// U and V, the slack goes to scratch of its own (never B.pu.S, which the ADMM / ALM kernels write and read), and every launch goes
// straight to the stream -- not through LAUNCH, which would flush a pending dual update into the state.  All sums are per-workgroup
// partials added in a fixed order by one workgroup: two calls on the same state give the same bits.

namespace {

// d = R_p . R_q (this lane's share), R = (U + V) / 2 formed as k_average forms it (uv) or R = U; 8 lanes per pair, 16-byte row loads
// when the rank and the base pointers allow them
__device__ __forceinline__ double cert_row_dot(const double *__restrict__ U, const double *__restrict__ V, bool uv, bool v2, int p, int q,
                                               int r, int lane) {
    double s = 0.0;
    if (v2) {
        const double2 *up = (const double2 *)(U + (size_t)p * r), *uq = (const double2 *)(U + (size_t)q * r);
        const double2 *vp = (const double2 *)(V + (size_t)p * r), *vq = (const double2 *)(V + (size_t)q * r);
        for (int j = lane; j < r / 2; j += 8) {
            const double2 a = factor_ld(up, vp, uv, j), b = factor_ld(uq, vq, uv, j);
            s += a.x * b.x;
            s += a.y * b.y;
        }
    } else {
        for (int j = lane; j < r; j += 8) s += factor_ld(U, V, uv, (size_t)p * r + j) * factor_ld(U, V, uv, (size_t)q * r + j);
    }
    return s;
}

// Over the entries e = (p, q) of a pattern: d_e = <E_pq + E_qp (p != q) | E_pp, R R^T>, i.e. R_p.R_q, twice off the diagonal (the
// convention of k_pairdots).  dout (may be null) keeps d; cw / sw (may be null) weight it into the two sums <C, X>, <S, X>, whose
// per-workgroup partials go to part[blockIdx] and part[gridDim + blockIdx].  Grid-stride over the entries (bounded grid).
__global__ __launch_bounds__(TPB) void k_cert_pat(int ne, const int *__restrict__ erow, const int *__restrict__ ecol,
                                                  const double *__restrict__ U, const double *__restrict__ V, int uv, int r,
                                                  double *__restrict__ dout, const double *__restrict__ cw,
                                                  const double *__restrict__ sw, double *__restrict__ part) {
    __shared__ double sh[4];
    const int lane = threadIdx.x & 7;
    const bool v2 = (r % 2) == 0 && (((uintptr_t)U | (uintptr_t)V) & 15) == 0;
    double ac = 0.0, as = 0.0;
    const int step = gridDim.x * (TPB / 8);
    for (int e = blockIdx.x * (TPB / 8) + threadIdx.x / 8; e < ne; e += step) { // (uniform over the entry's 8 lanes)
        const int p = erow[e], q = ecol[e];
        double s = group_sum<8>(cert_row_dot(U, V, uv != 0, v2, p, q, r, lane));
        const double d = p == q ? s : 2.0 * s;
        if (lane == 0) {
            if (dout) dout[e] = d;
            if (cw) ac += cw[e] * d;
            if (sw) as += sw[e] * d;
        }
    }
    if (!part) return;
    ac = block_sum(ac, sh);
    as = block_sum(as, sh);
    if (threadIdx.x == 0) { part[blockIdx.x] = ac; part[gridDim.x + blockIdx.x] = as; }
}

// A_k(X_k) of a cone's constraints from the pair values d on its A-pattern, added to the global m-vector ax (each constraint is one
// group's: no two writers; the cones run one after the other)
__global__ __launch_bounds__(TPB) void k_cert_cv(int nrow, const int *__restrict__ a_ptr, const int *__restrict__ a_e,
                                                 const double *__restrict__ a_val, const double *__restrict__ d,
                                                 const int *__restrict__ row_idx, double *__restrict__ ax) {
    const int i = (blockIdx.x * TPB + threadIdx.x) / 8, lane = threadIdx.x & 7;
    const bool act = i < nrow;
    double s = 0.0;
    if (act)
        for (int t = a_ptr[i] + lane; t < a_ptr[i + 1]; t += 8) s += a_val[t] * d[a_e[t]];
    s = group_sum<8>(s);
    if (act && lane == 0) ax[row_idx[i]] += s;
}

// G = R R^T on the full npad x npad square of a dense-storage cone (zero outside n x n)
__global__ __launch_bounds__(TPB) void k_cert_gram(int n, int npad, const double *__restrict__ U, const double *__restrict__ V, int uv,
                                                   int r, double *__restrict__ G) {
    const size_t len = (size_t)npad * npad;
    for (size_t t = (size_t)blockIdx.x * TPB + threadIdx.x; t < len; t += (size_t)gridDim.x * TPB) {
        const int p = (int)(t / npad), q = (int)(t % npad);
        double s = 0.0;
        if (p < n && q < n)
            for (int j = 0; j < r; ++j) s += factor_ld(U, V, uv != 0, (size_t)p * r + j) * factor_ld(U, V, uv != 0, (size_t)q * r + j);
        G[t] = s;
    }
}

// per-workgroup partials of a . b (grid-stride)
__global__ __launch_bounds__(TPB) void k_cert_dot(size_t len, const double *__restrict__ a, const double *__restrict__ b,
                                                  double *__restrict__ part) {
    __shared__ double sh[4];
    double s = 0.0;
    for (size_t t = (size_t)blockIdx.x * TPB + threadIdx.x; t < len; t += (size_t)gridDim.x * TPB) s += a[t] * b[t];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// dst[idx ? idx[i] : i] += sum of np partials (one workgroup, fixed order)
__global__ __launch_bounds__(TPB) void k_cert_fin(const double *__restrict__ part, int np, double *__restrict__ dst,
                                                  const int *__restrict__ idx, int i) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int t = threadIdx.x; t < np; t += TPB) s += part[t];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) dst[idx ? idx[i] : i] += s;
}

// one workgroup: ax <- A(X) - b in place; acc[2..5] = { ||A(X) - b||_2^2, ||A(X) - b||_inf, ||b||_inf, b . lambda }
__global__ __launch_bounds__(TPB) void k_cert_close(int m, double *__restrict__ ax, const double *__restrict__ b,
                                                    const double *__restrict__ lam, double *__restrict__ acc) {
    __shared__ double sh[4];
    double s2 = 0.0, rinf = 0.0, binf = 0.0, bl = 0.0;
    for (int i = threadIdx.x; i < m; i += TPB) {
        const double res = ax[i] - b[i];
        ax[i] = res;
        s2 += res * res;
        rinf = fmax(rinf, fabs(res));
        binf = fmax(binf, fabs(b[i]));
        bl += b[i] * lam[i];
    }
    s2 = block_sum(s2, sh);
    bl = block_sum(bl, sh);
    rinf = block_max(rinf, sh);
    binf = block_max(binf, sh);
    if (threadIdx.x == 0) { acc[2] = s2; acc[3] = rinf; acc[4] = binf; acc[5] = bl; }
}

// *out = min(v[0..n)) (one workgroup)
__global__ __launch_bounds__(TPB) void k_cert_min(int n, const double *__restrict__ v, double *__restrict__ out) {
    __shared__ double sh[4];
    double s = INFINITY;
    for (int t = threadIdx.x; t < n; t += TPB) s = fmin(s, v[t]);
    s = block_min(s, sh);
    if (threadIdx.x == 0) *out = s;
}

constexpr int CERT_GRID = 1024; // workgroups of the pattern pass (bounded: its partials fit the scratch)
constexpr int CERT_ACC = 16;    // accumulators in front of the per-cone minima of LP blocks

// scratch of the export, allocated on first use (CertScratch::release frees it with the context)
int cert_alloc(lorads_hip_ctx *c) {
    CertScratch &X = c->cert;
    if (X.ready) return 0;
    size_t s_tot = 0, sd_tot = 0, ne_max = 0, na_max = 0, g_max = 0, nd_max = 0;
    X.s_off.assign(c->nb, 0);
    X.sd_off.assign(c->nb, 0);
    for (int k = 0; k < c->nb; ++k) {
        const Block &B = c->blk[k];
        X.s_off[k] = s_tot;
        s_tot += (size_t)B.pu.ne;
        ne_max = std::max(ne_max, (size_t)B.pu.ne);
        na_max = std::max(na_max, (size_t)B.pa.ne);
        if (B.dense_a || B.dense_c) g_max = std::max(g_max, (size_t)B.npad * B.npad);
        X.sd_off[k] = sd_tot;
        if (B.dense_a) { sd_tot += (size_t)B.npad * B.npad; nd_max = std::max(nd_max, (size_t)B.nd); }
    }
    if (X.mem.alloc(&X.lam, (size_t)c->m) || X.mem.alloc(&X.ax, (size_t)c->m) || X.mem.alloc(&X.S, s_tot) || X.mem.alloc(&X.d, ne_max) ||
        X.mem.alloc(&X.dA, na_max) || X.mem.alloc(&X.G, g_max) || X.mem.alloc(&X.Sd, sd_tot) || X.mem.alloc(&X.mu, nd_max) ||
        X.mem.alloc(&X.part, (size_t)2 * CERT_GRID) || X.mem.alloc(&X.acc, (size_t)CERT_ACC + c->nb)) {
        X.release();
        return 1;
    }
    X.ready = true;
    return 0;
}

// the multipliers the next iteration will use: lambda, with a dual update that waits for a carrier applied (as k_dual_update applies
// it) to the copy -- the state keeps waiting
void cert_lambda(lorads_hip_ctx *c) {
    if (c->m == 0) return;
    hipMemcpyAsync(c->cert.lam, c->lambda, sizeof(double) * (size_t)c->m, hipMemcpyDeviceToDevice, c->stream);
    if (c->pend.dual_owed())
        hipLaunchKernelGGL(k_dual_update, dim3(nblocks_for((size_t)c->m, TPB)), dim3(TPB), 0, c->stream, c->m,
                           ds_rho_dual(c, c->pend.dual_rho_value()), (const double *)c->b, (const double *)c->csum, c->cert.lam);
}

// S_k = C_k - sum_i lambda_i A_ik into the scratch: the union pattern's values (k_sval, W_DUAL) and, on a cone with dense constraint
// matrices, the dense share [C] - sum_j lambda_j A_j
void cert_slack(lorads_hip_ctx *c, int k) {
    Block &B = c->blk[k];
    CertScratch &X = c->cert;
    WArgs wa{};
    wa.lambda = X.lam; wa.row_idx = B.row_idx;
    if (B.pu.ne > 0)
        hipLaunchKernelGGL(k_sval, dim3(nblocks_for((size_t)B.pu.ne, TPB)), dim3(TPB), 0, c->stream, B.pu.ne, (const int *)B.pu.e_ptr,
                           (const int *)B.pu.e_con, (const double *)B.pu.e_val, (const double *)B.pu.cbase, (int)W_DUAL, wa,
                           X.S + X.s_off[k], NOGUARD, (CGState *)nullptr, 0, (const double *)nullptr, (double *)nullptr, Deferred{});
    if (B.dense_a) {
        const size_t msz = (size_t)B.npad * B.npad;
        hipLaunchKernelGGL(k_dense_mu, dim3(nblocks_for((size_t)B.nd, TPB)), dim3(TPB), 0, c->stream, B.nd, (const int *)B.d_con,
                           (int)W_DUAL, wa, 1.0, X.mu, NOGUARD);
        hipLaunchKernelGGL(k_dense_combine, dim3(grid1d(msz)), dim3(TPB), 0, c->stream, msz, B.nd, (const double *)B.Adense,
                           (const double *)X.mu, (const double *)(B.dense_c ? B.Cfull : nullptr), X.Sd + X.sd_off[k], NOGUARD);
    }
}
// the dense share of S (null: none)
const double *cert_dense_slack(lorads_hip_ctx *c, int k) {
    const Block &B = c->blk[k];
    return B.dense_a ? c->cert.Sd + c->cert.sd_off[k] : B.dense_c ? B.Cfull : nullptr;
}

// dst[idx ? idx[i] : i] += a . b over len doubles
void cert_dot_into(lorads_hip_ctx *c, size_t len, const double *a, const double *b, double *dst, const int *idx, int i) {
    const int g = std::min(grid1d(len), 256);
    hipLaunchKernelGGL(k_cert_dot, dim3(g), dim3(TPB), 0, c->stream, len, a, b, c->cert.part);
    hipLaunchKernelGGL(k_cert_fin, dim3(1), dim3(TPB), 0, c->stream, (const double *)c->cert.part, g, dst, idx, i);
}

} // namespace

extern "C" int lorads_hip_certificate(lorads_hip_ctx *c, int32_t src, double tol, int32_t ncv, int32_t max_restarts,
                                      double out[LORADS_HIP_CERT_N], double *lam_min, double *residual,
                                      double *lambda) {
    spec_touch(c);
    if (postsolve_args(c, src, nullptr, "certificate", true)) return 1;
    if (!out || (tol > 0 && ncv < 2)) return fail_msg("certificate: bad argument");
    if (postsolve_sharded(c, "certificate", "cannot export a solution") || cert_alloc(c)) return 1;
    CertScratch &X = c->cert;
    cert_lambda(c);
    HC(hipMemsetAsync(X.ax, 0, sizeof(double) * (size_t)std::max(c->m, 1), c->stream));
    HC(hipMemsetAsync(X.acc, 0, sizeof(double) * ((size_t)CERT_ACC + c->nb), c->stream));
    for (int k = 0; k < c->nb; ++k) {
        Block &B = c->blk[k];
        const FactorView F = factor_view(c, src, k);
        cert_slack(c, k);
        if (B.pu.ne > 0) { // <C, X> and <S, X> over the union pattern (d_e kept in the scratch)
            const int g = std::min(nblocks_for((size_t)B.pu.ne, TPB / 8), CERT_GRID);
            hipLaunchKernelGGL(k_cert_pat, dim3(g), dim3(TPB), 0, c->stream, B.pu.ne, (const int *)B.pu.erow, (const int *)B.pu.ecol, F.U, F.V,
                               F.uv, B.r, X.d, (const double *)B.pu.cbase, (const double *)(X.S + X.s_off[k]), X.part);
            hipLaunchKernelGGL(k_cert_fin, dim3(1), dim3(TPB), 0, c->stream, (const double *)X.part, g, X.acc, (const int *)nullptr, 0);
            hipLaunchKernelGGL(k_cert_fin, dim3(1), dim3(TPB), 0, c->stream, (const double *)(X.part + g), g, X.acc, (const int *)nullptr, 1);
        }
        if (B.pa.ne > 0 && B.nrow > 0) { // A_k(X_k) by constraint over the A-pattern
            const int g = std::min(nblocks_for((size_t)B.pa.ne, TPB / 8), CERT_GRID);
            hipLaunchKernelGGL(k_cert_pat, dim3(g), dim3(TPB), 0, c->stream, B.pa.ne, (const int *)B.pa.erow, (const int *)B.pa.ecol, F.U, F.V,
                               F.uv, B.r, X.dA, (const double *)nullptr, (const double *)nullptr, (double *)nullptr);
            hipLaunchKernelGGL(k_cert_cv, dim3(nblocks_for((size_t)B.nrow, TPB / 8)), dim3(TPB), 0, c->stream, B.nrow, (const int *)B.a_ptr,
                               (const int *)B.a_e, (const double *)B.a_val, (const double *)X.dA, (const int *)B.row_idx, X.ax);
        }
        if (B.dense_a || B.dense_c) { // the dense shares through G = R R^T
            const size_t msz = (size_t)B.npad * B.npad;
            hipLaunchKernelGGL(k_cert_gram, dim3(grid1d(msz)), dim3(TPB), 0, c->stream, B.n, B.npad, F.U, F.V, F.uv, B.r, X.G);
            if (B.dense_c) cert_dot_into(c, msz, B.Cfull, X.G, X.acc, nullptr, 0);
            cert_dot_into(c, msz, cert_dense_slack(c, k), X.G, X.acc, nullptr, 1);
            for (int j = 0; j < B.nd; ++j)
                cert_dot_into(c, msz, B.Adense + (size_t)j * msz, X.G, X.ax, B.row_idx, B.d_con_h[j]);
        }
        if (B.is_lp && B.pu.ne > 0) // lambda_min of the LP block: min_j s_j over the pattern (a column outside it has s_j = 0)
            hipLaunchKernelGGL(k_cert_min, dim3(1), dim3(TPB), 0, c->stream, B.pu.ne, (const double *)(X.S + X.s_off[k]), X.acc + CERT_ACC + k);
    }
    hipLaunchKernelGGL(k_cert_close, dim3(1), dim3(TPB), 0, c->stream, c->m, X.ax, (const double *)c->b, (const double *)X.lam, X.acc);
    std::vector<double> acc((size_t)CERT_ACC + c->nb);
    HC(hipMemcpyAsync(acc.data(), X.acc, sizeof(double) * acc.size(), hipMemcpyDeviceToHost, c->stream));
    if (lambda && c->m) HC(hipMemcpyAsync(lambda, X.lam, sizeof(double) * (size_t)c->m, hipMemcpyDeviceToHost, c->stream));
    if (residual && c->m) HC(hipMemcpyAsync(residual, X.ax, sizeof(double) * (size_t)c->m, hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    // lambda_min per cone: Lanczos on the scratch slack (tol <= 0: not computed, NaN)
    std::vector<double> th((size_t)c->nb, std::nan(""));
    int nmv = 0;
    for (int k = 0; k < c->nb && tol > 0; ++k) {
        Block &B = c->blk[k];
        if (B.is_lp) {
            th[k] = B.pu.ne > 0 ? acc[CERT_ACC + k] : 0.0;
            if (B.pu.ne < B.n) th[k] = std::min(th[k], 0.0);
            continue;
        }
        if (lanczos_min_eig(c, c->stream, nullptr, B, tol, ncv, max_restarts, &th[k], &nmv, X.S + X.s_off[k], cert_dense_slack(c, k)))
            return 1;
    }
    double lmin = tol > 0 ? INFINITY : std::nan("");
    for (int k = 0; k < c->nb && tol > 0; ++k) lmin = std::min(lmin, th[k]);
    if (lam_min)
        for (int k = 0; k < c->nb; ++k) lam_min[k] = th[k];
    out[0] = std::sqrt(acc[2]) / (1 + c->b_nrm1);
    out[1] = acc[3] / (1 + acc[4]);
    out[2] = acc[0];
    out[3] = acc[5];
    out[4] = acc[1];
    out[5] = lmin;
    out[6] = (double)nmv;
    out[7] = std::sqrt(acc[2]);
    out[8] = acc[3];
    out[9] = acc[4];
    return 0;
}

extern "C" int lorads_hip_get_slack(lorads_hip_ctx *c, int32_t k, int64_t *nnz, int32_t *row, int32_t *col, double *val) {
    spec_touch(c);
    if (!c || !nnz || k < 0 || k >= c->nb) return fail_msg("get_slack: bad argument");
    if (postsolve_sharded(c, "get_slack", "cannot export a solution")) return 1;
    Block &B = c->blk[k];
    const bool dense = B.dense_a || B.dense_c;
    const int64_t cnt = B.is_lp ? B.n : dense ? (int64_t)B.n * (B.n + 1) / 2 : B.pu.ne;
    if (!row || !col || !val) { *nnz = cnt; return 0; }
    if (cert_alloc(c)) return 1;
    CertScratch &X = c->cert;
    cert_lambda(c);
    cert_slack(c, k);
    std::vector<int> er((size_t)B.pu.ne), ec((size_t)B.pu.ne);
    std::vector<double> sv((size_t)B.pu.ne), sd;
    if (B.pu.ne) {
        HC(hipMemcpyAsync(er.data(), B.pu.erow, sizeof(int) * er.size(), hipMemcpyDeviceToHost, c->stream));
        HC(hipMemcpyAsync(ec.data(), B.pu.ecol, sizeof(int) * ec.size(), hipMemcpyDeviceToHost, c->stream));
        HC(hipMemcpyAsync(sv.data(), X.S + X.s_off[k], sizeof(double) * sv.size(), hipMemcpyDeviceToHost, c->stream));
    }
    if (dense) {
        sd.resize((size_t)B.npad * B.npad);
        HC(hipMemcpyAsync(sd.data(), cert_dense_slack(c, k), sizeof(double) * sd.size(), hipMemcpyDeviceToHost, c->stream));
    }
    HC(hipStreamSynchronize(c->stream));
    if (B.is_lp) { // one (j, j) entry per column; a column outside the pattern has s_j = 0
        for (int j = 0; j < B.n; ++j) { row[j] = col[j] = j; val[j] = 0.0; }
        for (int e = 0; e < B.pu.ne; ++e) val[er[e]] = sv[e];
    } else if (dense) { // the whole lower triangle, column by column: dense share + the pattern's
        std::vector<int64_t> at((size_t)B.n + 1, 0); // first slot of column q
        for (int q = 0; q < B.n; ++q) at[q + 1] = at[q] + (B.n - q);
        for (int q = 0; q < B.n; ++q)
            for (int p = q; p < B.n; ++p) {
                const int64_t t = at[q] + (p - q);
                row[t] = p; col[t] = q; val[t] = sd[(size_t)p * B.npad + q];
            }
        for (int e = 0; e < B.pu.ne; ++e) val[at[ec[e]] + (er[e] - ec[e])] += sv[e];
    } else {
        for (int e = 0; e < B.pu.ne; ++e) { row[e] = er[e]; col[e] = ec[e]; val[e] = sv[e]; }
    }
    *nnz = cnt;
    return 0;
}
