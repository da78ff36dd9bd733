// lanczos.inc -- dual infeasibility of the current multipliers (SURVEY.md 8f3), included by lorads_hip.hip.
//
// Replaces calculate_dual_infeasibility_solver (data/lorads_solver.c:1007-1037) + dual_infeasible
// (data/lorads_sdp_conic.c:1286-1349): per cone the slack S_k = C_k - sum_i lambda_i A_ik is assembled on the
// union pattern (addObjCoeff + sdpDataWSum with -lambda) and its smallest eigenvalue is found with a Lanczos
// process whose only contact with S is y = S x -- the same gather kernel shape as the rest of the path, r = 1.
// The reference hands this to ARPACK (dsaupd/dseupd: which = "SA", nev = 1, ncv = 40, tol = 1e-2, <= 600
// restarts); here it is a thick-restart Lanczos with full (twice-applied classical Gram-Schmidt)
// re-orthogonalisation, the same subspace size, the same stopping rule |beta_m y_m| <= tol max(eps^(2/3), |theta|)
// and the same restart budget.  Basis, matvec and orthogonalisation live on the device; the (<= 41)^2 projected
// matrix is diagonalised on the host (cyclic Jacobi).  Round 4: the recurrence's scalars stay on the device (k_lz_close: alpha_j,
// beta_j, the running norm of T, the breakdown test; k_scale_to takes 1 / beta_j from there), so a whole sweep of up to ncv steps is
// enqueued without a host round trip and the host reads the coefficients back ONCE PER RESTART (round 3: one copy and one
// hipStreamSynchronize per step -- more than the solve itself on rand4000).

namespace {

// y = S x over a symmetric pattern (row p gathers its neighbours), 8 lanes per row
__global__ __launch_bounds__(TPB) void k_spmv(int n, const int *__restrict__ adj_ptr, const int *__restrict__ adj_col,
                                              const int *__restrict__ adj_e, const double *__restrict__ S,
                                              const double *__restrict__ x, double *__restrict__ y,
                                              const double *__restrict__ dense_add) {
    const int p = (blockIdx.x * TPB + threadIdx.x) / 8, lane = threadIdx.x & 7;
    const bool act = p < n;
    const int pp = act ? p : n - 1;
    double s = 0.0;
    for (int t = adj_ptr[pp] + lane; t < adj_ptr[pp + 1]; t += 8) s += S[adj_e[t]] * x[adj_col[t]];
    s = group_sum<8>(s);
    if (act && lane == 0) y[p] = s + (dense_add ? dense_add[p] : 0.0);
}
// y = C x for the dense objective (npad x npad row-major, zero padded), one wavefront per row
__global__ __launch_bounds__(TPB) void k_dense_mv(int n, int npad, const double *__restrict__ C, const double *__restrict__ x,
                                                  double *__restrict__ y) {
    const int row = (blockIdx.x * TPB + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (row >= n) return; // uniform per wavefront
    double s = 0.0;
    for (int q = lane; q < n; q += 64) s += C[(size_t)row * npad + q] * x[q];
    s = wave_sum(s);
    if (lane == 0) y[row] = s;
}
// h_j = <V_j, w>, one workgroup per basis vector (deterministic order)
__global__ __launch_bounds__(TPB) void k_basis_dots(int n, const double *__restrict__ V, const double *__restrict__ w,
                                                    double *__restrict__ h) {
    __shared__ double sh[4];
    const double *v = V + (size_t)blockIdx.x * n;
    double s = 0.0;
    // (eight element pairs requested per trip, added in the order of the plain loop: one workgroup streams a whole basis vector, and
    // one load per trip made that a chain of n / 256 dependent round trips -- 40 us per call at n = 20000)
    for (int i = threadIdx.x; i < n; i += 8 * TPB) {
        double a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int k = i + u * TPB, kc = k < n ? k : i; a[u] = v[kc]; b[u] = w[kc]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) s += i + u * TPB < n ? a[u] * b[u] : 0.0;
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) h[blockIdx.x] = s;
}
// w -= sum_j h_j V_j
__global__ __launch_bounds__(TPB) void k_basis_sub(int n, const double *__restrict__ V, int ncols, const double *__restrict__ h,
                                                   double *__restrict__ w) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double s = w[i];
    for (int j0 = 0; j0 < ncols; j0 += 8) { // (eight columns requested per trip, subtracted in the order of the plain loop)
        double v[8], hj[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int j = j0 + u < ncols ? j0 + u : j0; v[u] = V[(size_t)j * n + i]; hj[u] = h[j]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) if (j0 + u < ncols) s -= hj[u] * v[u];
    }
    w[i] = s;
}
__global__ __launch_bounds__(TPB) void k_scale_to(int n, const double *__restrict__ w, double a, double *__restrict__ dst) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) dst[i] = a * w[i];
}
// The scalar end of Lanczos step j on the device: alpha_j = h1_j + h2_j (the two Gram-Schmidt passes), beta_j = ||w||, the running
// max |T| and the breakdown test (beta_j negligible: invariant subspace, the sweep ends at j).  ab = [alpha_0..m | beta_0..m | tnorm |
// breakdown step or -1]; a sweep that has broken down does nothing more.
__global__ void k_lz_close(int j, int m, const double *__restrict__ h1, const double *__restrict__ h2, const double *__restrict__ nr2,
                           double *__restrict__ ab) {
    if (ab[2 * (m + 1) + 1] >= 0.0) return;
    const double alpha = h1[j] + h2[j], beta = sqrt(fmax(0.0, nr2[0]));
    ab[j] = alpha;
    ab[(m + 1) + j] = beta;
    const double tn = fmax(ab[2 * (m + 1)], fmax(fabs(alpha), beta));
    ab[2 * (m + 1)] = tn;
    if (!(beta > 1e-13 * fmax(tn, 1e-300))) ab[2 * (m + 1) + 1] = (double)j; // (also taken by a NaN: the host reports it)
}
// v_{j+1} = w / beta_j (zeros once the sweep has broken down: the remaining steps of the enqueued sweep then work on nothing)
__global__ __launch_bounds__(TPB) void k_scale_to_dev(int n, const double *__restrict__ w, const double *__restrict__ ab, int j, int m,
                                                      double *__restrict__ dst) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const bool broke = ab[2 * (m + 1) + 1] >= 0.0;
    const double a = 1.0 / ab[(m + 1) + j];
    dst[i] = broke ? 0.0 : a * w[i];
}
// Vout[:, c] = V[:, 0:m] Y[:, c], c < k  (Ritz vectors kept across a restart)
__global__ __launch_bounds__(TPB) void k_basis_rotate(int n, const double *__restrict__ V, int m, const double *__restrict__ Y,
                                                      int k, double *__restrict__ Vout) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < k; ++c) {
        double s = 0.0;
        for (int j = 0; j < m; ++j) s += V[(size_t)j * n + i] * Y[(size_t)c * m + j];
        Vout[(size_t)c * n + i] = s;
    }
}

// eigen-decomposition of a small symmetric matrix (row-major m x m, destroyed): cyclic Jacobi, ascending order;
// Y column-major (eigenvector c at Y[c*m ...]).  The rotations are applied in Rutishauser's form: the diagonal moves by t a_pq (the
// corrections of a sweep are summed apart and added once), the rotated entry is set to zero, the others move by s (x -+ tau y), and an
// entry below the rounding of both its diagonals is dropped.  The eigenvalues then carry a few eps ||A|| of rounding whatever m is:
// a rotation written out as two matrix products loses about m eps ||A|| (5e-14 relative at m = 40), and a thick restart carries
// theta into the next projected matrix, so that with a small subspace and hundreds of restarts the loss adds up.
void small_sym_eig(int m, std::vector<double> &A, std::vector<double> &theta, std::vector<double> &Y) {
    Y.assign((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) Y[(size_t)i * m + i] = 1.0;
    std::vector<double> d(m), d0(m), z(m, 0.0);
    for (int i = 0; i < m; ++i) d[i] = d0[i] = A[(size_t)i * m + i];
    auto rot = [&](double s, double tau, size_t x, size_t y) {
        const double g = A[x], h = A[y];
        A[x] = g - s * (h + g * tau);
        A[y] = h + s * (g - h * tau);
    };
    for (int sweep = 0; sweep < 60; ++sweep) {
        double sm = 0.0;
        for (int p = 0; p < m - 1; ++p)
            for (int q = p + 1; q < m; ++q) sm += std::fabs(A[(size_t)p * m + q]);
        if (sm == 0.0) break;
        const double tresh = sweep < 3 ? 0.2 * sm / ((double)m * m) : 0.0;
        for (int p = 0; p < m - 1; ++p)
            for (int q = p + 1; q < m; ++q) {
                double &apq = A[(size_t)p * m + q];
                const double g = 100.0 * std::fabs(apq);
                if (sweep > 3 && std::fabs(d[p]) + g == std::fabs(d[p]) && std::fabs(d[q]) + g == std::fabs(d[q])) { apq = 0.0; continue; }
                if (!(std::fabs(apq) > tresh)) continue;
                double h = d[q] - d[p], t;
                if (std::fabs(h) + g == std::fabs(h)) t = apq / h;
                else {
                    const double th = 0.5 * h / apq;
                    t = 1.0 / (std::fabs(th) + std::sqrt(1.0 + th * th));
                    if (th < 0.0) t = -t;
                }
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = t * cs, tau = sn / (1.0 + cs);
                h = t * apq;
                z[p] -= h; z[q] += h;
                d[p] -= h; d[q] += h;
                apq = 0.0;
                for (int j = 0; j < p; ++j) rot(sn, tau, (size_t)j * m + p, (size_t)j * m + q);         // (upper triangle only)
                for (int j = p + 1; j < q; ++j) rot(sn, tau, (size_t)p * m + j, (size_t)j * m + q);
                for (int j = q + 1; j < m; ++j) rot(sn, tau, (size_t)p * m + j, (size_t)q * m + j);
                for (int j = 0; j < m; ++j) { // eigenvectors are stored as rows of Y^T here: Y[c*m + j]
                    const double yp = Y[(size_t)p * m + j], yq = Y[(size_t)q * m + j];
                    Y[(size_t)p * m + j] = yp - sn * (yq + yp * tau);
                    Y[(size_t)q * m + j] = yq + sn * (yp - yq * tau);
                }
            }
        for (int i = 0; i < m; ++i) { d0[i] += z[i]; d[i] = d0[i]; z[i] = 0.0; }
    }
    for (int i = 0; i < m; ++i) A[(size_t)i * m + i] = d[i];
    std::vector<int> ord(m);
    for (int i = 0; i < m; ++i) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](int a, int b) { return A[(size_t)a * m + a] < A[(size_t)b * m + b]; });
    theta.resize(m);
    std::vector<double> Ys((size_t)m * m);
    for (int c = 0; c < m; ++c) {
        theta[c] = A[(size_t)ord[c] * m + ord[c]];
        std::copy(Y.begin() + (size_t)ord[c] * m, Y.begin() + (size_t)(ord[c] + 1) * m, Ys.begin() + (size_t)c * m);
    }
    Y.swap(Ys);
}

struct LanczosBufs {
    double *V = nullptr, *V2 = nullptr, *w = nullptr, *h = nullptr, *Yd = nullptr, *dtmp = nullptr;
};

// Every cone's eigen-solve is independent of the others: they run on their own streams (one host thread each, see
// lorads_hip_dual_infeasibility), so everything here is launched on an explicit stream.
#define LAUNCH_ON(st, kern, grid, ...) hipLaunchKernelGGL(kern, dim3(grid), dim3(TPB), 0, st, __VA_ARGS__)

// y = (C - sum_i lambda_i A_i) x of cone B; S holds the W_DUAL assembly on the union pattern and Sd (dense-storage cones) the dense
// share of the slack, npad x npad
void slack_matvec(hipStream_t st, Block &B, const double *x, double *y, double *dtmp, const double *S, const double *Sd) {
    const bool dn = B.dense_c || B.dense_a;
    if (dn) LAUNCH_ON(st, k_dense_mv, nblocks_for((size_t)B.n, TPB / 64), B.n, B.npad, Sd, x, dtmp);
    LAUNCH_ON(st, k_spmv, nblocks_for((size_t)B.n, TPB / 8), B.n, B.pu.adj_ptr, B.pu.adj_col, B.pu.adj_e, S, x, y,
              dn ? dtmp : (const double *)nullptr);
}

// S_given / Sd_given null: the slack of the context's multipliers is assembled into B.pu.S (and B.Sfull); otherwise the caller has
// assembled it there (the solution export's own scratch, solution.inc) and nothing of the cone is written
int lanczos_min_eig(lorads_hip_ctx *c, hipStream_t st, double *pinned, Block &B, double tol, int ncv, int max_restart,
                    double *theta_out, int *matvecs, const double *S_given = nullptr, const double *Sd_given = nullptr) {
    const int n = B.n, m = std::max(1, std::min(ncv, n)), keep_max = 8;
    DevPool mem; // this solve's scratch (a worker thread's own pool): gone on every way out
    LanczosBufs lb;
    if (mem.alloc(&lb.V, (size_t)n * (m + 1)) || mem.alloc(&lb.V2, (size_t)n * (keep_max + 1)) || mem.alloc(&lb.w, (size_t)n) ||
        mem.alloc(&lb.h, (size_t)2 * (m + 1) + 1) || mem.alloc(&lb.Yd, (size_t)m * keep_max) || mem.alloc(&lb.dtmp, (size_t)n))
        return 1;
    // S on the union pattern: C_e - sum_i lambda_i a  (data/lorads_solver.c:1027-1029)
    WArgs wa{};
    wa.lambda = c->lambda; wa.row_idx = B.row_idx;
    const double *Smv = S_given ? S_given : B.pu.S;
    // (dense constraint matrices: the dense share [C] - sum_j lambda_j A_j, formed once before the iterations)
    const double *Sdmv = S_given ? Sd_given : B.dense_a ? B.Sfull : B.Cfull;
    if (!S_given && B.pu.ne > 0)
        LAUNCH_ON(st, k_sval, nblocks_for((size_t)B.pu.ne, TPB), B.pu.ne, B.pu.e_ptr, B.pu.e_con, B.pu.e_val, B.pu.cbase, (int)W_DUAL, wa,
                  B.pu.S, NOGUARD, (CGState *)nullptr, 0);
    if (!S_given && B.dense_a) { // the dense constraints' share of the slack: [C_dense] - sum_j lambda_j A_j
        const size_t msz = (size_t)B.npad * B.npad;
        hipLaunchKernelGGL(k_dense_mu, dim3(nblocks_for((size_t)B.nd, TPB)), dim3(TPB), 0, st, B.nd, (const int *)B.d_con, (int)W_DUAL, wa, 1.0,
                           B.d_mu, NOGUARD);
        hipLaunchKernelGGL(k_dense_combine, dim3(grid1d(msz)), dim3(TPB), 0, st, msz, B.nd, (const double *)B.Adense, (const double *)B.d_mu,
                           (const double *)(B.dense_c ? B.Cfull : nullptr), B.Sfull, NOGUARD);
    }
    // start vector: fixed pseudo-random direction (ARPACK draws its own; any vector with a component along the
    // wanted eigenvector serves)
    {
        std::vector<double> v0((size_t)n);
        uint64_t s = 0x9E3779B97F4A7C15ull;
        double nr = 0.0;
        for (int i = 0; i < n; ++i) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            v0[i] = ((double)(s >> 11) / 9007199254740992.0) * 2.0 - 1.0;
            nr += v0[i] * v0[i];
        }
        nr = 1.0 / std::sqrt(nr);
        for (auto &x : v0) x *= nr;
        HC(hipMemcpyAsync(lb.V, v0.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
        HC(hipStreamSynchronize(st));
    }
    std::vector<double> T((size_t)m * m, 0.0), theta, Y, Tw;
    const size_t nhh = (size_t)2 * (m + 1) + 2;
    std::vector<double> hh_own(pinned ? 0 : nhh);
    double *hh = pinned ? pinned : hh_own.data(); // pinned (<= LZ_PINNED doubles): the read-back copy is a true async copy
    const double eps23 = std::pow(2.220446049250313e-16, 2.0 / 3.0);
    const int gn = nblocks_for((size_t)n, TPB);
    int k = 0, nmv = 0;
    double tnorm = 0.0;
    double *ab = nullptr; // (device) the sweep's coefficients, see k_lz_close
    if (mem.alloc(&ab, (size_t)2 * (m + 1) + 2)) return 1;
    {
        std::vector<double> z((size_t)2 * (m + 1) + 2, 0.0);
        z[(size_t)2 * (m + 1) + 1] = -1.0;
        HC(hipMemcpyAsync(ab, z.data(), sizeof(double) * z.size(), hipMemcpyHostToDevice, st));
        HC(hipStreamSynchronize(st));
    }
    for (int restart = 0;; ++restart) {
        int mm = m;
        bool breakdown = false;
        double beta = 0.0;
        // the whole sweep j = k .. m - 1 goes to the stream; ONE read-back at its end
        for (int j = k; j < m; ++j) {
            const double *vj = lb.V + (size_t)j * n;
            slack_matvec(st, B, vj, lb.w, lb.dtmp, Smv, Sdmv);
            double *h1 = lb.h, *h2 = lb.h + (m + 1), *nr2 = lb.h + 2 * (m + 1);
            LAUNCH_ON(st, k_basis_dots, j + 1, n, lb.V, lb.w, h1);
            LAUNCH_ON(st, k_basis_sub, gn, n, lb.V, j + 1, h1, lb.w);
            LAUNCH_ON(st, k_basis_dots, j + 1, n, lb.V, lb.w, h2);
            LAUNCH_ON(st, k_basis_sub, gn, n, lb.V, j + 1, h2, lb.w);
            LAUNCH_ON(st, k_basis_dots, 1, n, lb.w, lb.w, nr2);
            hipLaunchKernelGGL(k_lz_close, dim3(1), dim3(1), 0, st, j, m, (const double *)h1, (const double *)h2, (const double *)nr2, ab);
            LAUNCH_ON(st, k_scale_to_dev, gn, n, lb.w, (const double *)ab, j, m, lb.V + (size_t)(j + 1) * n);
        }
        HC(hipMemcpyAsync(hh, ab, sizeof(double) * ((size_t)2 * (m + 1) + 2), hipMemcpyDeviceToHost, st));
        HC(hipStreamSynchronize(st));
        const int jb = (int)hh[(size_t)2 * (m + 1) + 1];
        const int jend = jb >= 0 ? jb : m - 1;
        nmv += jend - k + 1;
        tnorm = hh[(size_t)2 * (m + 1)];
        for (int j = k; j <= jend; ++j) {
            const double alpha = hh[j];
            beta = hh[(size_t)(m + 1) + j];
            if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail_msg("dual_infeasibility: non-finite Lanczos coefficient");
            T[(size_t)j * m + j] = alpha;
            if (j == jb) { // invariant subspace: the Ritz values are exact
                mm = j + 1;
                breakdown = true;
                break;
            }
            if (j + 1 < m) T[(size_t)j * m + j + 1] = T[(size_t)(j + 1) * m + j] = beta;
        }
        if (jb >= 0) { // (re-arm the flag for the next sweep -- there is none after a breakdown, but keep the buffer consistent)
            const double minus1 = -1.0;
            HC(hipMemcpyAsync(ab + (size_t)2 * (m + 1) + 1, &minus1, sizeof(double), hipMemcpyHostToDevice, st));
            HC(hipStreamSynchronize(st));
        }
        Tw.assign((size_t)mm * mm, 0.0);
        for (int i = 0; i < mm; ++i)
            for (int j = 0; j < mm; ++j) Tw[(size_t)i * mm + j] = T[(size_t)i * m + j];
        small_sym_eig(mm, Tw, theta, Y);
        const double res = breakdown ? 0.0 : std::fabs(beta * Y[(size_t)0 * mm + (mm - 1)]);
        if (breakdown || res <= tol * std::max(eps23, std::fabs(theta[0])) || restart >= max_restart || mm < 2) {
            *theta_out = theta[0];
            if (matvecs) *matvecs += nmv;
            return 0;
        }
        // thick restart: keep the lowest Ritz vectors, continue from the residual direction
        const int keep = std::min(keep_max, mm - 1);
        HC(hipMemcpyAsync(lb.Yd, Y.data(), sizeof(double) * (size_t)mm * keep, hipMemcpyHostToDevice, st));
        LAUNCH_ON(st, k_basis_rotate, gn, n, lb.V, mm, lb.Yd, keep, lb.V2);
        HC(hipMemcpyAsync(lb.V2 + (size_t)keep * n, lb.V + (size_t)mm * n, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
        HC(hipMemcpyAsync(lb.V, lb.V2, sizeof(double) * (size_t)n * (keep + 1), hipMemcpyDeviceToDevice, st));
        HC(hipStreamSynchronize(st)); // Y (host) is re-used below
        std::fill(T.begin(), T.end(), 0.0);
        for (int i = 0; i < keep; ++i) {
            T[(size_t)i * m + i] = theta[i];
            T[(size_t)i * m + keep] = T[(size_t)keep * m + i] = beta * Y[(size_t)i * mm + (mm - 1)];
        }
        k = keep;
    }
}

} // namespace

extern "C" int lorads_hip_dual_infeasibility(lorads_hip_ctx *c, double tol, int32_t ncv, int32_t max_restarts, double *sum_neg,
                                             double *lam_min, int32_t *matvecs) {
    spec_touch(c);
    if (!c || !sum_neg || ncv < 2 || tol <= 0) return fail_msg("dual_infeasibility: bad argument");
    c->pend.flush(c); // (a dual update still waiting for a carrier: the multipliers must be final here)
    double acc = 0.0;
    std::vector<int> cones;
    std::vector<double> th((size_t)std::max(c->nb, 1), 0.0);
    for (int kb = 0; kb < c->nb; ++kb) {
        Block &B = c->blk[kb];
        if (B.is_lp) { // every LP column is its own 1 x 1 cone (data/lorads_solver.c:1015-1023): no eigen-solve
            hipLaunchKernelGGL(k_lp_dual, dim3(1), dim3(TPB), 0, c->stream, B.n, B.lp_ptr, B.lp_grow, B.lp_a, B.lp_cobj, c->lambda,
                               c->scal + 6);
            double v = 0.0;
            if (read_scalars(c, 6, 1, &v)) return 1;
            acc += v;
            continue;
        }
        cones.push_back(kb);
    }
    // SDP cones: independent eigen-solves.  Several cones -> a few host threads, each with its own stream, pull cones
    // from a shared counter: the small kernels of different cones overlap on the device and so do the host waits.
    int nthr = (int)std::min<size_t>(cones.size(), 8);
    nthr = opt_lanczos_threads(nthr);
    const bool pin_ok = (size_t)2 * (std::min<int>(ncv, 1 << 20) + 1) + 2 <= LZ_PINNED;
    while ((int)c->lz_workers.size() < nthr) { // worker streams + pinned read-back buffers are created once and kept
        const bool own_stream = !c->lz_workers.empty() || nthr > 1;
        c->lz_workers.emplace_back(); // (first, so that whatever is created below has its owner)
        LzWorker &w = c->lz_workers.back();
        if (own_stream) HC(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
        if (c->mem.alloc_pinned(&w.pinned, LZ_PINNED, hipHostMallocDefault)) return 1;
    }
    std::atomic<int> next{0}, failed{0}, nmv_tot{0};
    std::mutex err_mu;
    std::string err_text;
    int dev = 0;
    HC(hipGetDevice(&dev));
    HC(hipStreamSynchronize(c->stream)); // lambda and the patterns are final before other streams read them
    auto worker = [&](hipStream_t st, double *pinned) {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= (int)cones.size() || failed.load()) return;
            int nmv = 0;
            if (lanczos_min_eig(c, st, pin_ok ? pinned : nullptr, c->blk[cones[i]], tol, ncv, max_restarts, &th[cones[i]], &nmv)) {
                std::lock_guard<std::mutex> lk(err_mu);
                if (!failed.exchange(1)) err_text = g_err;
                return;
            }
            nmv_tot.fetch_add(nmv);
        }
    };
    if (nthr <= 1) {
        if (!cones.empty()) worker(c->stream, c->lz_workers[0].pinned);
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < nthr; ++t)
            pool.emplace_back([&, dev, t]() {
                if (hipSetDevice(dev) != hipSuccess) {
                    std::lock_guard<std::mutex> lk(err_mu);
                    if (!failed.exchange(1)) err_text = "dual_infeasibility: hipSetDevice failed in a worker thread";
                    return;
                }
                hipStream_t st = c->lz_workers[t].stream ? c->lz_workers[t].stream : c->stream;
                worker(st, c->lz_workers[t].pinned);
                hipStreamSynchronize(st);
            });
        for (auto &t : pool) t.join();
    }
    if (failed.load()) return fail_msg(err_text.empty() ? "dual_infeasibility failed" : err_text);
    for (int kb : cones) acc += std::fabs(std::min(th[kb], 0.0)); // data/lorads_solver.c:1032
    if (lam_min)
        for (int kb = 0; kb < c->nb; ++kb) lam_min[kb] = th[kb];
    *sum_neg = acc;
    if (matvecs) *matvecs = nmv_tot.load();
    return 0;
}
