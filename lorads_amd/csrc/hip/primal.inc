// primal.inc -- entries of the primal X = F F^T and its products with a block of vectors, included by lorads_hip.hip after spectral.inc.
//
// Per SDP cone (DESIGN.md section 13): F = R, or (U + V) / 2 formed as k_average forms it, at the cone's own rank rl (pad and
// common-rank columns are zero: walked or skipped, the value is the same); X = F F^T in the file's units, never formed.  On the LP block
// X = diag(f_j^2).
//   k_primal_entries + k_primal_stats_close   val_e = F_row . F_col by one 8-lane group per entry (16-byte row loads, PRIMAL_EPG entries
//                                             of a group in flight); with reference values the four statistics ride along as
//                                             per-workgroup partials, closed in order by one workgroup
//   k_primal_ftb + k_primal_ftb_sum           T = F^T B on the FP64 matrix cores (postsolve.inc: mfma_strip_tile): row strips give
//                                             partial tiles, added in strip order
//   k_primal_ft                               Y = F T (mfma_fm_tile: a wavefront takes 16 rows, 128-byte row segments out)
//   k_primal_lp                               Y = diag(f^2) B on the LP block
// Both entry points are read-only on the solver's state: the scratch is the feature's own (PrimalScratch), every launch goes straight
// to the stream (never through LAUNCH, which would flush a pending dual update into the state).  No float atomics: every sum is a
// fixed sequence of partials, chunks and panels in order -- the same state and arguments give the same bits.

namespace {

constexpr int PRIMAL_EPG = 4;                          // entries one 8-lane group has in flight
constexpr int PRIMAL_EPW = (TPB / 8) * PRIMAL_EPG;     // entries per workgroup (LORADS_HIP_PRIMAL_EPW)
constexpr int PRIMAL_PW = 16;                          // columns of a panel of B and Y: one MFMA tile, one 128-byte row segment
constexpr int PRIMAL_ROWS = 1 << 16;                   // rows of a panel held on the device at a time
constexpr int PRIMAL_MAX_STRIPS = 256;                 // strips of a row panel (row_strips)
constexpr int PRIMAL_MAXR = 512;                       // largest rank (as lorads_hip_resize_rank)
static_assert(PRIMAL_EPW == LORADS_HIP_PRIMAL_EPW, "the header states the entries per workgroup");
static_assert(LORADS_HIP_PRIMAL_CHUNK % PRIMAL_EPW == 0, "a chunk is whole workgroups");

// val_e = F_p . F_q for the entries of one chunk.  Entry e of the workgroup's PRIMAL_EPW belongs to group e % 32 (neighbouring groups
// read neighbouring indices and write neighbouring values).  The indices of all PRIMAL_EPG entries are fetched first, then per step of
// 8 x 16 bytes the row pieces of all of them, before the first product.  Entries past the count are the last entry again (clamped),
// never stored and selected out of the statistics; double2 indices past the row's end are element 0 times zero.  Each lane sums its
// products a.x b.x, a.y b.y in column order and the eight lanes are added by a butterfly: the sequence is the same with p and q
// swapped and every product commutes, so val(p, q) and val(q, p) are the same bits.  diag: the LP block, X = diag(f^2).
// With ref the workgroup's partials {sum d^2, sum |d|, max |d|, sum ref^2} (d = val - ref; entries in order within a group, groups in
// order) go to part[4 blockIdx ..].
template <bool UV>
__global__ __launch_bounds__(TPB) void k_primal_entries(int cnt, const int *__restrict__ row, const int *__restrict__ col,
                                                        const double *__restrict__ U, const double *__restrict__ V, int r, int diag,
                                                        double *__restrict__ val, const double *__restrict__ ref,
                                                        double *__restrict__ part) {
    __shared__ double sh[TPB / 8][4];
    const int g = threadIdx.x >> 3, lane = threadIdx.x & 7;
    const bool v2 = (r % 2) == 0 && (((uintptr_t)U | (uintptr_t)V) & 15) == 0;
    int p[PRIMAL_EPG], q[PRIMAL_EPG], ec[PRIMAL_EPG];
    bool act[PRIMAL_EPG];
#pragma unroll
    for (int t = 0; t < PRIMAL_EPG; ++t) {
        const int e = blockIdx.x * PRIMAL_EPW + t * (TPB / 8) + g;
        act[t] = e < cnt;
        ec[t] = act[t] ? e : cnt - 1;
        p[t] = row[ec[t]];
        q[t] = col[ec[t]];
    }
    double s[PRIMAL_EPG];
#pragma unroll
    for (int t = 0; t < PRIMAL_EPG; ++t) s[t] = 0.0;
    if (v2) {
        const int h = r / 2;
        for (int j0 = 0; j0 < h; j0 += 8) {
            const int j = j0 + lane, jc = j < h ? j : 0;
            const double m = j < h ? 1.0 : 0.0;
            double2 a[PRIMAL_EPG], b[PRIMAL_EPG];
#pragma unroll
            for (int t = 0; t < PRIMAL_EPG; ++t) {
                a[t] = factor_ld((const double2 *)(U + (size_t)p[t] * r), (const double2 *)(V + (size_t)p[t] * r), UV, jc);
                b[t] = factor_ld((const double2 *)(U + (size_t)q[t] * r), (const double2 *)(V + (size_t)q[t] * r), UV, jc);
            }
#pragma unroll
            for (int t = 0; t < PRIMAL_EPG; ++t) {
                s[t] += (a[t].x * b[t].x) * m;
                s[t] += (a[t].y * b[t].y) * m;
            }
        }
    } else {
        for (int j0 = 0; j0 < r; j0 += 8) {
            const int j = j0 + lane, jc = j < r ? j : 0;
            const double m = j < r ? 1.0 : 0.0;
#pragma unroll
            for (int t = 0; t < PRIMAL_EPG; ++t) {
                s[t] += (factor_ld(U, V, UV, (size_t)p[t] * r + jc) * factor_ld(U, V, UV, (size_t)q[t] * r + jc)) * m;
            }
        }
    }
    double st[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < PRIMAL_EPG; ++t) {
        double v = group_sum<8>(s[t]);
        v = (diag && p[t] != q[t]) ? 0.0 : v;
        if (lane == 0) {
            if (val && act[t]) val[ec[t]] = v;
            if (ref) {
                const double rf = act[t] ? ref[ec[t]] : 0.0;
                const double d = act[t] ? fabs(v - rf) : 0.0;
                st[0] += d * d; st[1] += d; st[2] = fmax(st[2], d); st[3] += rf * rf;
            }
        }
    }
    if (!ref) return; // (uniform)
    if (lane == 0) {
#pragma unroll
        for (int w = 0; w < 4; ++w) sh[g][w] = st[w];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int w = threadIdx.x;
        double v = 0.0;
        for (int i = 0; i < TPB / 8; ++i) v = w == 2 ? fmax(v, sh[i][w]) : v + sh[i][w];
        part[4 * (size_t)blockIdx.x + w] = v;
    }
}

// acc[0..3] <- acc combined with the nb workgroup partials of one chunk: thread t folds its run of consecutive workgroups in order,
// then four threads fold the 256 runs in order (one workgroup)
__global__ __launch_bounds__(TPB) void k_primal_stats_close(int nb, const double *__restrict__ part, double *__restrict__ acc) {
    __shared__ double sh[4][TPB];
    const int per = (nb + TPB - 1) / TPB, b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = b0; b < b1; ++b) {
        st[0] += part[4 * (size_t)b]; st[1] += part[4 * (size_t)b + 1];
        st[2] = fmax(st[2], part[4 * (size_t)b + 2]); st[3] += part[4 * (size_t)b + 3];
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) sh[w][threadIdx.x] = st[w];
    __syncthreads();
    if (threadIdx.x < 4) {
        const int w = threadIdx.x;
        double v = acc[w];
        for (int i = 0; i < TPB; ++i) v = w == 2 ? fmax(v, sh[w][i]) : v + sh[w][i];
        acc[w] = v;
    }
}

// Partial tile of T = F^T B of one row strip (blockIdx.x) and one 16-row tile I of T (blockIdx.y): mfma_strip_tile with A[m][k] =
// F[row k][16 I + m] (F transposed) and B[k][n] = Bp[row k][n] (the panel, row-major 16 wide: a 128-byte segment too).  Columns >= rl
// and rows >= n are clamped loads times zero.  Column nn of D is made of column nn of Bp alone.
__global__ __launch_bounds__(TPB) void k_primal_ftb(int n, int rl, int r, int rows_per_strip, int ntile, const double *__restrict__ U,
                                                    const double *__restrict__ V, int uv, const double *__restrict__ Bp,
                                                    double *__restrict__ part) {
    const int nn = threadIdx.x & 15;
    const int ca = 16 * blockIdx.y + nn, cac = ca < rl ? ca : 0;
    const double ma = ca < rl ? 1.0 : 0.0;
    mfma_strip_tile(n, rows_per_strip, ntile, part, [=](size_t row, double mr, double &a, double &b) {
        a = factor_ld(U, V, uv != 0, row * r + cac) * (ma * mr);
        b = Bp[row * PRIMAL_PW + nn] * mr;
    });
}

// T (16 ntile x 16, row-major) = [T +] the strips' partial tiles added in strip order (first: the row panel that opens the sum)
__global__ __launch_bounds__(TPB) void k_primal_ftb_sum(int strips, int ntile, int first, const double *__restrict__ part,
                                                        double *__restrict__ T) {
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    double v = first ? 0.0 : T[o];
    for (int s = 0; s < strips; ++s) v += part[((size_t)s * ntile + blockIdx.x) * 256 + threadIdx.x];
    T[o] = v;
}

// Yp (rows x 16, row-major) = F T.  A wavefront takes 16 rows: mfma_fm_tile with M = T (T's rows >= rl are zero, as F's columns there
// count for zero).
__global__ __launch_bounds__(TPB) void k_primal_ft(int n, int rl, int r, const double *__restrict__ U, const double *__restrict__ V, int uv,
                                                   const double *__restrict__ T, double *__restrict__ Yp) {
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, nn = l & 15, kk = l >> 4;
    const int row0 = (blockIdx.x * (TPB / 64) + wave) * 16;
    if (row0 >= n) return; // (wave-uniform)
    const size_t ao = (size_t)(row0 + nn < n ? row0 + nn : n - 1) * r;
    const v4f64 acc = mfma_fm_tile(U, V, uv != 0, ao, rl, kk, [=](int k) { return T[(size_t)k * PRIMAL_PW + nn]; });
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int rw = row0 + kk + 4 * q;
        if (rw < n) Yp[(size_t)rw * PRIMAL_PW + nn] = acc[q];
    }
}

// LP block: Yp[i][j] = f_i^2 Bp[i][j] (f: column 0 of the block's rows of stride r)
__global__ __launch_bounds__(TPB) void k_primal_lp(size_t len, int r, const double *__restrict__ U, const double *__restrict__ V, int uv,
                                                   const double *__restrict__ Bp, double *__restrict__ Yp) {
    for (size_t t = (size_t)blockIdx.x * TPB + threadIdx.x; t < len; t += (size_t)gridDim.x * TPB) {
        const double f = factor_ld(U, V, uv != 0, (t / PRIMAL_PW) * r);
        Yp[t] = (f * f) * Bp[t];
    }
}

} // namespace

extern "C" int lorads_hip_primal_entries(lorads_hip_ctx *c, int32_t src, int32_t blk, int64_t count, const int32_t *row, const int32_t *col,
                                         double *val, const double *ref, double stats[4]) {
    spec_touch(c);
    if (postsolve_args(c, src, &blk, "primal_entries", false)) return 1;
    if (count < 0) return fail_msg("primal_entries: count " + std::to_string((long long)count) + " is negative");
    if (count > 0 && (!row || !col)) return fail_msg("primal_entries: row and col must not be NULL");
    if (!val && !ref && count > 0) return fail_msg("primal_entries: val may be NULL only when ref is given");
    if ((ref != nullptr) != (stats != nullptr))
        return fail_msg("primal_entries: stats must be given with ref and only with it");
    if (postsolve_sharded(c, "primal_entries", "are not supported")) return 3;
    const Block &K = c->blk[blk];
    for (int64_t e = 0; e < count; ++e) { // (no index reaches a kernel before every one has been looked at)
        if (row[e] < 0 || row[e] >= K.n)
            return fail_msg("primal_entries: row[" + std::to_string((long long)e) + "] = " + std::to_string(row[e]) + " is outside [0, " + std::to_string(K.n) + ")");
        if (col[e] < 0 || col[e] >= K.n)
            return fail_msg("primal_entries: col[" + std::to_string((long long)e) + "] = " + std::to_string(col[e]) + " is outside [0, " + std::to_string(K.n) + ")");
    }
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0.0;
    if (count == 0) return 0;
    PrimalScratch &X = c->primal;
    const size_t cap = (size_t)std::min<int64_t>(count, LORADS_HIP_PRIMAL_CHUNK);
    if (X.row.grow(X.mem, cap) || X.col.grow(X.mem, cap) || X.val.grow(X.mem, cap)) return 1;
    if (ref && (X.ref.grow(X.mem, cap) || X.part.grow(X.mem, 4 * (size_t)nblocks_for(cap, PRIMAL_EPW)))) return 1;
    if (!X.acc && X.mem.alloc(&X.acc, 4)) return 1;
    const FactorView F = factor_view(c, src, blk);
    if (ref) HC(hipMemsetAsync(X.acc, 0, sizeof(double) * 4, c->stream));
    for (int64_t e0 = 0; e0 < count; e0 += LORADS_HIP_PRIMAL_CHUNK) {
        const int cnt = (int)std::min<int64_t>(count - e0, LORADS_HIP_PRIMAL_CHUNK), grid = nblocks_for((size_t)cnt, PRIMAL_EPW);
        HC(hipMemcpyAsync(X.row, row + e0, sizeof(int) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
        HC(hipMemcpyAsync(X.col, col + e0, sizeof(int) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
        if (ref) HC(hipMemcpyAsync(X.ref, ref + e0, sizeof(double) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
        if (F.uv)
            hipLaunchKernelGGL(k_primal_entries<true>, dim3(grid), dim3(TPB), 0, c->stream, cnt, (const int *)X.row, (const int *)X.col, F.U, F.V,
                               K.r, K.is_lp ? 1 : 0, X.val, ref ? (const double *)X.ref : nullptr, X.part);
        else
            hipLaunchKernelGGL(k_primal_entries<false>, dim3(grid), dim3(TPB), 0, c->stream, cnt, (const int *)X.row, (const int *)X.col, F.U, F.V,
                               K.r, K.is_lp ? 1 : 0, X.val, ref ? (const double *)X.ref : nullptr, X.part);
        if (ref) hipLaunchKernelGGL(k_primal_stats_close, dim3(1), dim3(TPB), 0, c->stream, grid, (const double *)X.part, X.acc);
        HC(hipGetLastError());
        if (val) HC(hipMemcpyAsync(val + e0, X.val, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
    }
    if (ref) HC(hipMemcpyAsync(stats, X.acc, sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int lorads_hip_primal_apply(lorads_hip_ctx *c, int32_t src, int32_t blk, int32_t ncols, const double *B, double *Y, double *T) {
    spec_touch(c);
    if (postsolve_args(c, src, &blk, "primal_apply", false)) return 1;
    if (ncols < 1 || ncols > 1024) return fail_msg("primal_apply: ncols " + std::to_string(ncols) + " is outside [1, 1024]");
    if (!B || !Y) return fail_msg("primal_apply: B and Y must not be NULL");
    if (c->blk[blk].is_lp && T) return fail_msg("primal_apply: the LP block has no factor: T must be NULL");
    if (postsolve_sharded(c, "primal_apply", "are not supported")) return 3;
    const Block &K = c->blk[blk];
    const int n = K.n, rl = K.rl;
    if (n == 0) return 0;
    if (!K.is_lp && rl > PRIMAL_MAXR) return fail_msg("primal_apply: rank above 512");
    PrimalScratch &X = c->primal;
    const int rcap = std::min(n, PRIMAL_ROWS), ntile = K.is_lp ? 1 : (rl + 15) / 16;
    int smax = 0, rps0 = 0;
    row_strips(rcap, PRIMAL_MAX_STRIPS, smax, rps0);
    if (X.bp.grow(X.mem, (size_t)rcap * PRIMAL_PW) || X.yp.grow(X.mem, (size_t)rcap * PRIMAL_PW)) return 1;
    if (!K.is_lp && (X.tpart.grow(X.mem, (size_t)smax * ntile * 256) || X.t.grow(X.mem, (size_t)ntile * 256))) return 1;
    const FactorView F = factor_view(c, src, blk);
    std::vector<double> hb((size_t)rcap * PRIMAL_PW), ht((size_t)ntile * 256);
    // one row panel of one column panel of B, row-major 16 wide (columns past ncols: zero), to the device
    auto send_b = [&](int c0, int pw, int r0, int rows) -> int {
        for (int i0 = 0; i0 < rows; i0 += 32) // (32 rows at a time: both sides of the transposition stay in the cache)
            for (int j = 0; j < PRIMAL_PW; ++j)
                for (int i = i0; i < std::min(rows, i0 + 32); ++i) hb[(size_t)i * PRIMAL_PW + j] = j < pw ? B[(size_t)(c0 + j) * n + r0 + i] : 0.0;
        HC(hipMemcpyAsync(X.bp, hb.data(), sizeof(double) * (size_t)rows * PRIMAL_PW, hipMemcpyHostToDevice, c->stream));
        return 0;
    };
    auto fetch_y = [&](int c0, int pw, int r0, int rows) -> int {
        HC(hipMemcpyAsync(hb.data(), X.yp, sizeof(double) * (size_t)rows * PRIMAL_PW, hipMemcpyDeviceToHost, c->stream));
        HC(hipStreamSynchronize(c->stream));
        for (int i0 = 0; i0 < rows; i0 += 32)
            for (int j = 0; j < pw; ++j)
                for (int i = i0; i < std::min(rows, i0 + 32); ++i) Y[(size_t)(c0 + j) * n + r0 + i] = hb[(size_t)i * PRIMAL_PW + j];
        return 0;
    };
    for (int c0 = 0; c0 < ncols; c0 += PRIMAL_PW) {
        const int pw = std::min(PRIMAL_PW, ncols - c0);
        if (K.is_lp) {
            for (int r0 = 0; r0 < n; r0 += PRIMAL_ROWS) {
                const int rows = std::min(PRIMAL_ROWS, n - r0);
                if (send_b(c0, pw, r0, rows)) return 1;
                hipLaunchKernelGGL(k_primal_lp, dim3(std::min(4096, nblocks_for((size_t)rows * PRIMAL_PW, TPB))), dim3(TPB), 0, c->stream,
                                   (size_t)rows * PRIMAL_PW, K.r, F.U + (size_t)r0 * K.r, F.V + (size_t)r0 * K.r, F.uv, (const double *)X.bp, X.yp);
                HC(hipGetLastError());
                if (fetch_y(c0, pw, r0, rows)) return 1;
            }
            continue;
        }
        for (int r0 = 0; r0 < n; r0 += PRIMAL_ROWS) { // T = F^T B: row panels in order
            const int rows = std::min(PRIMAL_ROWS, n - r0);
            int strips, rps;
            row_strips(rows, PRIMAL_MAX_STRIPS, strips, rps);
            if (send_b(c0, pw, r0, rows)) return 1;
            hipLaunchKernelGGL(k_primal_ftb, dim3(strips, ntile), dim3(TPB), 0, c->stream, rows, rl, K.r, rps, ntile, F.U + (size_t)r0 * K.r,
                               F.V + (size_t)r0 * K.r, F.uv, (const double *)X.bp, X.tpart);
            hipLaunchKernelGGL(k_primal_ftb_sum, dim3(ntile), dim3(TPB), 0, c->stream, strips, ntile, r0 == 0 ? 1 : 0, (const double *)X.tpart, X.t);
            HC(hipGetLastError());
            HC(hipStreamSynchronize(c->stream)); // (the staging array is packed anew)
        }
        if (T) {
            HC(hipMemcpyAsync(ht.data(), X.t, sizeof(double) * ht.size(), hipMemcpyDeviceToHost, c->stream));
            HC(hipStreamSynchronize(c->stream));
            for (int j = 0; j < pw; ++j)
                for (int k = 0; k < rl; ++k) T[(size_t)(c0 + j) * rl + k] = ht[(size_t)k * PRIMAL_PW + j];
        }
        for (int r0 = 0; r0 < n; r0 += PRIMAL_ROWS) { // Y = F T
            const int rows = std::min(PRIMAL_ROWS, n - r0);
            hipLaunchKernelGGL(k_primal_ft, dim3(nblocks_for((size_t)rows, 16 * (TPB / 64))), dim3(TPB), 0, c->stream, rows, rl, K.r,
                               F.U + (size_t)r0 * K.r, F.V + (size_t)r0 * K.r, F.uv, (const double *)X.t, X.yp);
            HC(hipGetLastError());
            if (fetch_y(c0, pw, r0, rows)) return 1;
        }
    }
    return 0;
}
