// spectral.inc -- spectrum of the solution factors and their reduction to a lower rank, included by lorads_hip.hip after rounding.inc.
//
// Per SDP cone (DESIGN.md section 12): F = R, or (U + V) / 2 formed as k_average forms it, at the cone's OWN rank rl (no pad column,
// no common-rank columns); G = F^T F (rl x rl) = Q Lambda Q^T with lambda_1 >= lambda_2 >= ... (ties: lower original index first).
// The non-zero eigenvalues of X = F F^T are those of G, F Q has mutually orthogonal columns of squared norm lambda_j, and its first
// k columns are the best rank-k approximation of X.
//   k_spec_gram + k_spec_gram_sum   G on the FP64 matrix cores (postsolve.inc: mfma_strip_tile): row strips give partial Grams, a
//                                   second stage adds them in strip order (no float atomics: same state, same bits)
//   k_spec_jacobi                   one workgroup per cone: cyclic Jacobi in the round-robin ordering, then the sort
//   k_spec_rotate                   F' = F Q[:, :k] on the matrix cores (mfma_fm_tile), written to the new R, U and V alike
// lorads_hip_spectrum is read-only on the solver's state: the scratch is the feature's own (SpecScratch) and every launch goes
// straight to the stream (never through LAUNCH, which would flush a pending dual update into the state).

namespace {

constexpr int SPEC_MAXR = 512;        // largest rank (as lorads_hip_resize_rank)
constexpr int SPEC_SWEEPS = 30;       // sweeps after which a Jacobi run that still rotates is an error
constexpr int SPEC_JT = 1024;         // threads of k_spec_jacobi's workgroup
constexpr int SPEC_LDS_M = 96;        // largest order whose G and Q live in LDS: 2 m (m + 1) 8 bytes = 145.5 KB of the 160 KB
constexpr int SPEC_MAX_STRIPS = 256;
constexpr size_t SPEC_PART_CAP = (size_t)4 << 20; // doubles of Gram partials (32 MB): fewer strips at large rl
constexpr size_t SPEC_W_CAP = (size_t)3 << 20;    // doubles of G, Q, eigenvalues and sorted Q per k_spec_jacobi launch (24 MB): cones
                                                  // beyond it go to a further launch (one cone of order 512 takes 0.79 M)

// Partial Gram of one row strip and one tile pair I <= J (blockIdx.y): mfma_strip_tile with A[m][k] = F[row k][16 I + m] (F transposed)
// and B[k][n] = F[row k][16 J + n], segments of the same row.  Columns >= rl and rows >= n are clamped loads times zero.
__global__ __launch_bounds__(TPB) void k_spec_gram(int n, int rl, int r, int rows_per_strip, int npairs, const double *__restrict__ U,
                                                   const double *__restrict__ V, int uv, double *__restrict__ part) {
    const int nn = threadIdx.x & 15;
    const int T = (rl + 15) / 16;
    int I = 0, pi = blockIdx.y;
    while (pi >= T - I) { pi -= T - I; ++I; }
    const int J = I + pi;
    const int ca = 16 * I + nn, cb = 16 * J + nn;
    const int cac = ca < rl ? ca : 0, cbc = cb < rl ? cb : 0;
    const double ma = ca < rl ? 1.0 : 0.0, mb = cb < rl ? 1.0 : 0.0;
    mfma_strip_tile(n, rows_per_strip, npairs, part, [=](size_t row, double mr, double &a, double &b) {
        const size_t o = row * r;
        a = factor_ld(U, V, uv != 0, o + cac) * (ma * mr);
        b = factor_ld(U, V, uv != 0, o + cbc) * mb;
    });
}

// G (m x m, m = rl rounded up to even) = the strips' partial Grams added in strip order; tile pair I < J mirrored into (J, I)
__global__ __launch_bounds__(TPB) void k_spec_gram_sum(int rl, int m, int strips, int npairs, const double *__restrict__ part,
                                                       double *__restrict__ G) {
    const int T = (rl + 15) / 16;
    int I = 0, pi = blockIdx.x;
    while (pi >= T - I) { pi -= T - I; ++I; }
    const int J = I + pi;
    double v = 0.0;
    for (int s = 0; s < strips; ++s) v += part[((size_t)s * npairs + blockIdx.x) * 256 + threadIdx.x];
    const int gi = 16 * I + (int)(threadIdx.x >> 4), gj = 16 * J + (int)(threadIdx.x & 15);
    if (gi < m && gj < m) {
        G[(size_t)gi * m + gj] = v;
        if (I != J) G[(size_t)gj * m + gi] = v;
    }
}

// Cyclic Jacobi of one cone's G in the round-robin ("circle") ordering: m - 1 steps of m / 2 disjoint plane rotations per sweep.  All
// rotations of a step are computed from the matrix as the step found it (phase 0), then applied to the columns of G and Q (phase A)
// and to the rows of G (phase B).  A rotation is skipped when |g_pq| <= 2^-53 ||G||_F: an ABSOLUTE threshold (the relative one never
// settles on rank-deficient Grams, and the absolute accuracy is all a Gram with n u lambda_1 of rounding in it can give).  The pad
// index of an odd rl has a zero row and column: every rotation with it is skipped and it stays out of the sort.  The run ends with
// the first sweep that rotates nothing; SPEC_SWEEPS sweeps without one leave info[1] = 1, a factor that is not finite info[1] = 2.
template <bool LDS>
__device__ void spec_jacobi_body(const SpecCone C, double *__restrict__ W, int *__restrict__ info, double *dyn, double *cs, double *sn,
                                 int *pp, int *qq, int *perm, double *red, int *nrot) {
    const int m = C.m, rl = C.rl, h = m / 2, tid = threadIdx.x, nt = blockDim.x;
    double *Gg = W + C.g_off, *Qg = Gg + (size_t)m * m;
    const int ld = LDS ? m + 1 : m;
    double *G = LDS ? dyn : Gg, *Q = LDS ? dyn + (size_t)m * ld : Qg;
    double ss = 0.0;
    for (int w = tid; w < m * m; w += nt) {
        const int i = w / m, j = w % m;
        const double g = Gg[w];
        if (LDS) G[i * ld + j] = g;
        Q[i * ld + j] = i == j ? 1.0 : 0.0;
        ss += g * g;
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    ss = 0.0;
    for (int w = 0; w < nt / 64; ++w) ss += red[w];
    const double thr = 0x1p-53 * sqrt(ss);
    for (int j = tid; j < rl; j += nt) perm[j] = j; // (every entry defined whatever the diagonal holds)
    // a NaN or an infinity anywhere in the factor reaches ||G||_F: nothing is rotated and info[1] = 2 says so
    const bool finite = ss <= 0x1p1023;
    int sweeps = 0, left = 1;
    while (finite && sweeps < SPEC_SWEEPS && left) {
        if (tid == 0) *nrot = 0;
        __syncthreads();
        for (int step = 0; step < m - 1; ++step) {
            for (int i = tid; i < h; i += nt) {
                int a = m - 1, b = step;
                if (i > 0) { a = (step + i) % (m - 1); b = (step - i + (m - 1)) % (m - 1); }
                const int p = a < b ? a : b, q = a < b ? b : a;
                const double gpq = G[p * ld + q];
                double c = 1.0, s = 0.0;
                if (fabs(gpq) > thr) {
                    const double tau = (G[q * ld + q] - G[p * ld + p]) / (2.0 * gpq);
                    const double t = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                    atomicAdd(nrot, 1);
                }
                cs[i] = c; sn[i] = s; pp[i] = p; qq[i] = q;
            }
            __syncthreads();
            for (int w = tid; w < h * m; w += nt) { // columns p, q of G and Q
                const int i = w % h, row = w / h;
                const double s = sn[i];
                if (s == 0.0) continue;
                const double c = cs[i];
                const int p = row * ld + pp[i], q = row * ld + qq[i];
                const double gp = G[p], gq = G[q], xp = Q[p], xq = Q[q];
                G[p] = c * gp - s * gq; G[q] = s * gp + c * gq;
                Q[p] = c * xp - s * xq; Q[q] = s * xp + c * xq;
            }
            __syncthreads();
            for (int w = tid; w < h * m; w += nt) { // rows p, q of G
                const int i = w / m, col = w % m;
                const double s = sn[i];
                if (s == 0.0) continue;
                const double c = cs[i];
                const int p = pp[i] * ld + col, q = qq[i] * ld + col;
                const double gp = G[p], gq = G[q];
                G[p] = c * gp - s * gq; G[q] = s * gp + c * gq;
            }
            __syncthreads();
        }
        left = *nrot;
        ++sweeps;
        __syncthreads();
    }
    // eigenvalues descending (ties: lower original index first) with their columns
    for (int j = tid; j < rl; j += nt) {
        const double d = G[j * ld + j];
        int rk = 0;
        for (int i = 0; i < rl; ++i) {
            const double e = G[i * ld + i];
            rk += (e > d || (e == d && i < j)) ? 1 : 0;
        }
        if (finite) { perm[rk] = j; W[C.e_off + rk] = d; }
        else W[C.e_off + j] = d;
    }
    __syncthreads();
    for (int w = tid; w < rl * rl; w += nt) {
        const int i = w % rl, j = w / rl;
        W[C.q_off + w] = Q[i * ld + perm[j]];
    }
    if (tid == 0) { info[0] = sweeps; info[1] = !finite ? 2 : left ? 1 : 0; }
}

__global__ __launch_bounds__(SPEC_JT) void k_spec_jacobi(const SpecCone *__restrict__ cones, double *__restrict__ W, int *__restrict__ info) {
    extern __shared__ double spec_dyn[];
    __shared__ double cs[SPEC_MAXR / 2], sn[SPEC_MAXR / 2], red[SPEC_JT / 64];
    __shared__ int pp[SPEC_MAXR / 2], qq[SPEC_MAXR / 2], perm[SPEC_MAXR], nrot;
    const SpecCone C = cones[blockIdx.x];
    if (C.m <= SPEC_LDS_M) spec_jacobi_body<true>(C, W, info + 2 * blockIdx.x, spec_dyn, cs, sn, pp, qq, perm, red, &nrot);
    else spec_jacobi_body<false>(C, W, info + 2 * blockIdx.x, spec_dyn, cs, sn, pp, qq, perm, red, &nrot);
}

// F' = F Q[:, :knew] into the new factor arrays (row stride rnew; columns >= knew stay as alloc_factors zeroed them).  A wavefront
// takes 16 rows and, 16 columns j0 at a time, mfma_fm_tile with M[k][n] = Q[k][j0 + n] (Qs column-major rl x rl; columns >= knew: a
// clamped load times zero).
__global__ __launch_bounds__(TPB) void k_spec_rotate(int n, int rl, int r, int knew, int rnew, const double *__restrict__ U,
                                                     const double *__restrict__ V, int uv, const double *__restrict__ Qs,
                                                     double *__restrict__ oR, double *__restrict__ oU, double *__restrict__ oV) {
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, nn = l & 15, kk = l >> 4;
    const int row0 = (blockIdx.x * (TPB / 64) + wave) * 16;
    if (row0 >= n) return;
    const size_t ao = (size_t)(row0 + nn < n ? row0 + nn : n - 1) * r;
    for (int j0 = 0; j0 < knew; j0 += 16) {
        const int jb = j0 + nn;
        const size_t bo = (size_t)(jb < knew ? jb : 0) * rl;
        const double mb = jb < knew ? 1.0 : 0.0;
        const v4f64 acc = mfma_fm_tile(U, V, uv != 0, ao, rl, kk, [=](int k) { return Qs[bo + k] * mb; });
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = row0 + kk + 4 * q;
            if (row < n && jb < knew) {
                const size_t o = (size_t)row * rnew + jb;
                oR[o] = acc[q]; oU[o] = acc[q]; oV[o] = acc[q];
            }
        }
    }
}

inline int spec_m(int rl) { return (rl + 1) & ~1; }
inline size_t spec_w_need(int rl) { const size_t m = (size_t)spec_m(rl); return 2 * m * m + (size_t)rl + (size_t)rl * rl; }

// Gram + Jacobi of the SDP cones [k0, k1) (one k_spec_jacobi launch) of the factor arrays F (a view of whole arrays: offset 0) with the
// cones' CURRENT shapes `off`, `r`, `rl`; eigenvalues, sweep counts and (q != null) eigenvectors to the host arrays at the cones' places.
// The sorted eigenvectors of cone k stay in the scratch at W + qoff[k] until the next call.
int spec_run(lorads_hip_ctx *c, const FactorView &F, int k0, int k1, const std::vector<size_t> &off,
             const std::vector<int> &r, const std::vector<int> &rl, double *eig, double *q, int32_t *sweeps,
             std::vector<size_t> &qoff) {
    SpecScratch &X = c->spectral;
    std::vector<SpecCone> cones;
    std::vector<int> which;
    size_t need = 0, part_need = 1;
    int lds_m = 0;
    for (int k = k0; k < k1; ++k) {
        if (c->blk[k].is_lp) continue;
        const int m = spec_m(rl[k]);
        SpecCone C;
        C.rl = rl[k]; C.m = m; C.g_off = (long long)need; C.e_off = C.g_off + 2ll * m * m; C.q_off = C.e_off + rl[k];
        need += spec_w_need(rl[k]);
        qoff[k] = (size_t)C.q_off;
        cones.push_back(C);
        which.push_back(k);
        if (m <= SPEC_LDS_M) lds_m = std::max(lds_m, m);
    }
    if (cones.empty()) return 0;
    // strips of every cone: rows_per_strip a multiple of 64, the partials of one cone within SPEC_PART_CAP
    std::vector<int> strips(cones.size()), rps(cones.size()), npairs(cones.size());
    for (size_t i = 0; i < cones.size(); ++i) {
        const int n = c->blk[which[i]].n, T = (cones[i].rl + 15) / 16;
        npairs[i] = T * (T + 1) / 2;
        const int smax = (int)std::max<size_t>(1, std::min<size_t>(SPEC_MAX_STRIPS, SPEC_PART_CAP / ((size_t)npairs[i] * 256)));
        row_strips(n, smax, strips[i], rps[i]);
        part_need = std::max(part_need, (size_t)strips[i] * npairs[i] * 256);
    }
    if (X.part.grow(X.mem, part_need) || X.W.grow(X.mem, need)) return 1;
    if (X.cones.grow(X.mem, cones.size()) || X.info.grow(X.mem, 2 * cones.size())) return 1;
    const int lds = (int)(sizeof(double) * 2 * (size_t)lds_m * (lds_m + 1));
    // (the attribute belongs to the kernel on the current device, not to a context: set before every launch, to the most it can ask for)
    HC(hipFuncSetAttribute((const void *)k_spec_jacobi, hipFuncAttributeMaxDynamicSharedMemorySize,
                           (int)(sizeof(double) * 2 * SPEC_LDS_M * (SPEC_LDS_M + 1))));
    for (size_t i = 0; i < cones.size(); ++i) {
        const Block &B = c->blk[which[i]];
        const int k = which[i];
        if (B.n == 0) { // (no rows: G = 0)
            HC(hipMemsetAsync(X.W + cones[i].g_off, 0, sizeof(double) * (size_t)cones[i].m * cones[i].m, c->stream));
            continue;
        }
        hipLaunchKernelGGL(k_spec_gram, dim3(strips[i], npairs[i]), dim3(TPB), 0, c->stream, B.n, rl[k], r[k], rps[i], npairs[i], F.U + off[k],
                           F.V + off[k], F.uv, X.part);
        hipLaunchKernelGGL(k_spec_gram_sum, dim3(npairs[i]), dim3(TPB), 0, c->stream, rl[k], cones[i].m, strips[i], npairs[i],
                           (const double *)X.part, X.W + cones[i].g_off);
    }
    HC(hipMemcpyAsync(X.cones, cones.data(), sizeof(SpecCone) * cones.size(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_spec_jacobi, dim3((unsigned)cones.size()), dim3(SPEC_JT), (size_t)lds, c->stream, (const SpecCone *)X.cones, X.W, X.info);
    HC(hipGetLastError());
    std::vector<int> info(2 * cones.size());
    HC(hipMemcpyAsync(info.data(), X.info, sizeof(int) * info.size(), hipMemcpyDeviceToHost, c->stream));
    size_t eo = 0;
    for (int k = 0; k < k0; ++k) eo += c->blk[k].is_lp ? 0 : (size_t)rl[k];
    size_t qo = 0;
    for (int k = 0; k < k0; ++k) qo += c->blk[k].is_lp ? 0 : (size_t)rl[k] * rl[k];
    for (size_t i = 0; i < cones.size(); ++i) {
        const size_t n1 = (size_t)cones[i].rl;
        if (eig) HC(hipMemcpyAsync(eig + eo, X.W + cones[i].e_off, sizeof(double) * n1, hipMemcpyDeviceToHost, c->stream));
        if (q) HC(hipMemcpyAsync(q + qo, X.W + cones[i].q_off, sizeof(double) * n1 * n1, hipMemcpyDeviceToHost, c->stream));
        eo += n1; qo += n1 * n1;
    }
    HC(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < cones.size(); ++i) {
        if (sweeps) sweeps[which[i]] = info[2 * i];
        if (info[2 * i + 1] == 2) {
            fail_msg("spectrum: the factor of cone " + std::to_string(which[i]) + " holds a value that is not finite");
            return 4;
        }
        if (info[2 * i + 1]) {
            fail_msg("spectrum: the Jacobi iteration of cone " + std::to_string(which[i]) + " (order " + std::to_string(cones[i].rl) +
                     ") still rotates after " + std::to_string(SPEC_SWEEPS) + " sweeps");
            return 4;
        }
    }
    return 0;
}

// the launches the cones are dealt to: consecutive cones while their G, Q and results fit SPEC_W_CAP
std::vector<std::pair<int, int>> spec_batches(const lorads_hip_ctx *c) {
    std::vector<std::pair<int, int>> out;
    int k0 = 0;
    size_t need = 0;
    for (int k = 0; k < c->nb; ++k) {
        const size_t w = c->blk[k].is_lp ? 0 : spec_w_need(c->blk[k].rl);
        if (need > 0 && need + w > SPEC_W_CAP) { out.push_back({k0, k}); k0 = k; need = 0; }
        need += w;
    }
    out.push_back({k0, c->nb});
    return out;
}

void spec_shapes(const lorads_hip_ctx *c, std::vector<size_t> &off, std::vector<int> &r, std::vector<int> &rl) {
    off.resize(c->nb); r.resize(c->nb); rl.resize(c->nb);
    for (int k = 0; k < c->nb; ++k) { off[k] = c->blk[k].off; r[k] = c->blk[k].r; rl[k] = c->blk[k].rl; }
}

} // namespace

extern "C" int lorads_hip_spectrum(lorads_hip_ctx *c, int32_t src, double *eig, double *q, int32_t *sweeps) {
    spec_touch(c);
    if (postsolve_args(c, src, nullptr, "spectrum", true)) return 1;
    if (!eig) return fail_msg("spectrum: bad argument");
    if (postsolve_sharded(c, "spectrum", "are not supported")) return 3;
    const FactorView F = factor_view(src, c->R, c->U, c->V, 0);
    std::vector<size_t> off, qoff(c->nb, 0);
    std::vector<int> r, rl;
    spec_shapes(c, off, r, rl);
    if (sweeps) for (int k = 0; k < c->nb; ++k) sweeps[k] = 0;
    for (auto &b : spec_batches(c)) {
        const int rc = spec_run(c, F, b.first, b.second, off, r, rl, eig, q, sweeps, qoff);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int lorads_hip_compress_rank(lorads_hip_ctx *c, int32_t src, const int32_t *nr, double *eig) {
    spec_touch(c);
    if (postsolve_args(c, src, nullptr, "compress_rank", true)) return 1;
    if (!nr) return fail_msg("compress_rank: bad argument");
    if (postsolve_sharded(c, "compress_rank", "are not supported")) return 3;
    // (refuse before anything is touched: a refused call leaves host and device at the old ranks and the old bits)
    for (int k = 0; k < c->nb; ++k) {
        const Block &B = c->blk[k];
        if (B.is_lp ? nr[k] != 1 : (nr[k] < 1 || nr[k] > B.rl)) return fail_msg("compress_rank: bad rank");
        const int nd = dev_rank(c, nr[k], B.is_lp);
        if (nblocks_for((size_t)B.n, TPB / lg_for(nd)) > c->maxpart)
            return fail_msg("compress_rank: cone dimension too large for the partial-sum slots at this rank");
    }
    std::vector<size_t> off_old, qoff(c->nb, 0);
    std::vector<int> r_old, rl_old;
    spec_shapes(c, off_old, r_old, rl_old);
    const auto batches = spec_batches(c);
    std::vector<double> ev;
    size_t ne = 0;
    for (int k = 0; k < c->nb; ++k) ne += c->blk[k].is_lp ? 0 : (size_t)rl_old[k];
    ev.resize(std::max<size_t>(ne, 1));
    // every cone's eigen-solve before the state is touched: one that does not converge is a refusal too
    for (auto &b : batches) {
        const int rc = spec_run(c, factor_view(src, c->R, c->U, c->V, 0), b.first, b.second, off_old, r_old, rl_old, ev.data(), nullptr,
                                nullptr, qoff);
        if (rc) return rc;
    }
    c->pend.flush(c);
    persist_touch(c);
    double *old[3] = {c->R, c->U, c->V};
    DevPool old_mem; // the old arrays live until the kernels below have read them, and go on every way out
    old_mem.swap(c->factor_mem);
    free_factors(c);
    invalidate_t(c);
    for (int k = 0; k < c->nb; ++k) { c->blk[k].rl = nr[k]; c->blk[k].r = dev_rank(c, nr[k], c->blk[k].is_lp); }
    common_rank(c);
    refresh_merged(c);
    if (alloc_factors(c)) return 1; // (every new array zero: pad columns, pad rows, Grad, the L-BFGS ring)
    const FactorView Fo = factor_view(src, old[0], old[1], old[2], 0);
    for (auto &b : batches) {
        // (several launches: the eigenvectors of this one are formed again -- the same bits -- since the scratch holds one launch's)
        if (batches.size() > 1) {
            const int rc = spec_run(c, Fo, b.first, b.second, off_old, r_old, rl_old, nullptr, nullptr, nullptr, qoff);
            if (rc) return rc;
        }
        for (int k = b.first; k < b.second; ++k) {
            const Block &B = c->blk[k];
            if (B.is_lp) { // the LP block is left alone: its three vectors are carried over as they are
                for (int a = 0; a < 3 && B.n; ++a)
                    HC(hipMemcpyAsync((a == 0 ? c->R : a == 1 ? c->U : c->V) + B.off, old[a] + off_old[k], sizeof(double) * (size_t)B.n * B.r,
                                      hipMemcpyDeviceToDevice, c->stream));
                continue;
            }
            if (B.n == 0) continue;
            hipLaunchKernelGGL(k_spec_rotate, dim3(nblocks_for((size_t)B.n, 16 * (TPB / 64))), dim3(TPB), 0, c->stream, B.n, rl_old[k], r_old[k],
                               B.rl, B.r, Fo.U + off_old[k], Fo.V + off_old[k], Fo.uv, (const double *)(c->spectral.W + qoff[k]), c->R + B.off,
                               c->U + B.off, c->V + B.off);
        }
    }
    HC(hipMemsetAsync(c->ring_ab, 0, sizeof(double) * (size_t)2 * c->L, c->stream));
    HC(hipStreamSynchronize(c->stream)); // (the old arrays are read by the kernels above)
    if (eig) std::copy(ev.begin(), ev.begin() + (long)ne, eig);
    return 0;
}
