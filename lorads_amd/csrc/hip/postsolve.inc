// postsolve.inc -- what the post-solve entry points share, included by lorads_hip.hip after lanczos.inc and before the first of them:
// solution.inc, rounding.inc, kcut.inc, stable.inc, bisect.inc, spectral.inc, primal.inc, cuts.inc, bounds.inc and topk.inc (DESIGN.md sections 10 to 19).  All of them read the solution
// factors and none is run by a solve.
//   FactorView / factor_view, factor_ld   which arrays make up F for a `src`, and F's elements on the device
//   mfma_strip_tile, mfma_fm_tile         the two FP64 matrix-core tile bodies, with the operand layout written down once
//   row_strips                            the row strips of the first of them
//   mfma_chain, packed_dot                the prefetching chain of MFMA steps over a row's columns; on two rows of a packed factor
//   k_pack_factor / pack_factor           F (and t) zero-padded to whole tiles of rows and whole steps of 4 columns
//   postsolve_args, postsolve_sharded     the argument checks and the sharded refusal, in the calling feature's words
// The four roundings share more than this file: the driver of a rounding call -- round_begin, round_reserve, round_vectors, round_signs,
// round_drive, trial_chunk(s), round_finish, round_stored_trial -- is in rounding.inc, behind the kernels it launches.
// (DevBuf, the grown scratch buffer of their scratch structs, sits with those structs in lorads_hip.hip: they are members of the
// context, which is defined long before this file is read.)

namespace {

// The factor F of the cones for a `src`: F = R (RR: both pointers name R), or F = (U + V) / 2 (UV), never stored.
struct FactorView { const double *U, *V; int uv; };
// from explicit arrays (lorads_hip_compress_rank reads the ones it has just replaced) at an offset / of block blk of the context
inline FactorView factor_view(int32_t src, const double *R, const double *U, const double *V, size_t off) {
    const int uv = src == LORADS_HIP_PAIR_UV;
    return {(uv ? U : R) + off, (uv ? V : R) + off, uv};
}
inline FactorView factor_view(const lorads_hip_ctx *c, int32_t src, int blk) { return factor_view(src, c->R, c->U, c->V, c->blk[blk].off); }

// F[i] (and, for 16-byte row loads, the pair F[2 i], F[2 i + 1]): the average is formed as k_average forms it, per component
__device__ __forceinline__ double factor_ld(const double *__restrict__ U, const double *__restrict__ V, bool uv, size_t i) {
    double a = U[i];
    if (uv) a = (a + V[i]) / 2;
    return a;
}
__device__ __forceinline__ double2 factor_ld(const double2 *__restrict__ U, const double2 *__restrict__ V, bool uv, size_t i) {
    double2 a = U[i];
    if (uv) { const double2 v = V[i]; a = make_double2((a.x + v.x) / 2, (a.y + v.y) / 2); }
    return a;
}

// ------------------------------------------------------------------ the FP64 matrix-core tiles
// v_mfma_f64_16x16x4_f64 computes D (16 x 16) += A (16 x 4) B (4 x 16) per wavefront.  Lane l = (nn = l & 15, kk = l >> 4) supplies
// ONE element of each operand, A[nn][kk] and B[kk][nn], and holds D[kk + 4 q][nn] in register q of its four (the FP64 result map: not
// the FP32 one).  Both tile bodies below feed it so that a lane's two operands come from one row of the matrices in memory, and
// mask by multiplying a clamped load with zero, never by branching.  (cuts.inc: cut_tile, bounds.inc: k_bnd_enum, topk.inc: k_topk_scan, kcut.inc: k_kcut_label and kernels.inc: k_dense_cx_b use the same
// layout on operands of their own.)

// Partial tile of F^T B over one row strip: the 16 x 16 tile D[m][n] = sum over the strip's rows k of A[m][k] B[k][n], where row k of
// the strip gives A[.][k] (a 128-byte segment of F's row, transposed) and B[k][.] (another segment of that row, or of a panel's).
// Workgroup blockIdx.x takes strip blockIdx.x of `rows_per_strip` rows (a multiple of 64: row_strips), its four wavefronts a quarter
// each, four rows per MFMA: lane (nn, kk) asks `load(row, mr, a, b)` for A[nn][row] and B[row][nn] of row kk of the four -- `row`
// clamped to 0 and mr = 0.0 past n, mr = 1.0 otherwise; which masks multiply which operand is the loader's business.  The four
// wavefronts' tiles are added in wave order through LDS and wave 0 stores the tile row-major, D[m][n] at 16 m + n of the 256 doubles
// of [strip blockIdx.x][tile blockIdx.y] of `part` (ntile tiles per strip).
template <typename Load>
__device__ __forceinline__ void mfma_strip_tile(int n, int rows_per_strip, int ntile, double *__restrict__ part, Load load) {
    __shared__ double red[3][4][64];
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, nn = l & 15, kk = l >> 4;
    const int q4 = rows_per_strip / 4; // (a multiple of 16)
    const int rbeg = blockIdx.x * rows_per_strip + wave * q4;
    v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < q4; k0 += 16) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = rbeg + k0 + 4 * u + kk;
            const bool ok = row < n;
            load((size_t)(ok ? row : 0), ok ? 1.0 : 0.0, a[u], b[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave - 1][q][l] = acc[q];
    }
    __syncthreads();
    if (wave != 0) return;
    double *out = part + ((size_t)blockIdx.x * ntile + blockIdx.y) * 256;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double v = acc[q];
        v += red[0][q][l]; v += red[1][q][l]; v += red[2][q][l];
        out[(kk + 4 * q) * 16 + nn] = v; // D[m = kk + 4 q][n = nn]
    }
}

// strips of `rows` rows for mfma_strip_tile: rows_per_strip a multiple of 64, at most smax strips (a function of the two alone)
inline void row_strips(int rows, int smax, int &strips, int &rps) {
    const int s = std::max(1, std::min(smax, nblocks_for((size_t)rows, 256)));
    rps = std::max(64, (nblocks_for((size_t)rows, s) + 63) & ~63);
    strips = std::max(1, nblocks_for((size_t)rows, rps));
}

// F M for the 16 rows of one wavefront and 16 columns of M: A[m][k] = F[row m][k0 + k], B[k][n] = M[k0 + k][n] in steps k0 of four
// columns of F up to rl.  Lane (nn, kk) reads F at ao + k, ao the start of ITS row nn (clamped by the caller), and asks `load_b(k)`
// for M[k][nn]; k >= rl is k = 0 with A's element times zero.  The lane's result register q is D[kk + 4 q][nn]: row kk + 4 q of
// the sixteen, column nn -- 128-byte row segments on the way out.
template <typename LoadB>
__device__ __forceinline__ v4f64 mfma_fm_tile(const double *__restrict__ U, const double *__restrict__ V, bool uv, size_t ao, int rl,
                                              int kk, LoadB load_b) {
    v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < rl; k0 += 4) {
        const int k = k0 + kk, kc = k < rl ? k : 0;
        const double a = factor_ld(U, V, uv, ao + kc) * (k < rl ? 1.0 : 0.0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, load_b(kc), acc, 0, 0, 0);
    }
    return acc;
}

// N steps of a chain from column k0 on: the operands of all N are asked for before the first step waits for its own
template <int N, typename Load>
__device__ __forceinline__ v4f64 mfma_steps(int k0, v4f64 d, Load load) {
    double x[N], y[N];
#pragma unroll
    for (int u = 0; u < N; ++u) load(k0 + 4 * u, x[u], y[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) d = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u], y[u], d, 0, 0, 0);
    return d;
}
// One chain of steps over rl4 columns (a multiple of 4) in fours, ascending: `load(k0, x, y)` supplies the lane's two operands of the
// step at column k0.  Eight, four, two steps and one at a time: the same chain as a loop of single steps, with more loads in flight.
template <typename Load>
__device__ __forceinline__ v4f64 mfma_chain(int rl4, Load load) {
    v4f64 d = (v4f64){0.0, 0.0, 0.0, 0.0};
    int k0 = 0;
    for (; k0 + 32 <= rl4; k0 += 32) d = mfma_steps<8>(k0, d, load);
    if (k0 + 16 <= rl4) { d = mfma_steps<4>(k0, d, load); k0 += 16; }
    if (k0 + 8 <= rl4) { d = mfma_steps<2>(k0, d, load); k0 += 8; }
    if (k0 < rl4) d = mfma_steps<1>(k0, d, load);
    return d;
}
// the chain on two rows of packed, padded matrices (A and B at the lane's column kk of its rows): nothing to clamp
__device__ __forceinline__ v4f64 packed_dot(const double *__restrict__ A, const double *__restrict__ B, int rl4) {
    return mfma_chain(rl4, [&](int k0, double &x, double &y) { x = A[k0]; y = B[k0]; });
}

// ------------------------------------------------------------------ the packed factor
// Fp (npad x rl4, row-major) <- F, the average of U and V formed once, zero past its n rows and rl columns; with t, tp (npad) <- t
// padded with ones
__global__ __launch_bounds__(TPB) void k_pack_factor(int n, int npad, int rl, int rl4, int r, const double *__restrict__ U,
                                                     const double *__restrict__ V, int uv, const double *__restrict__ t,
                                                     double *__restrict__ Fp, double *__restrict__ tp) {
    const size_t len = (size_t)npad * rl4;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < len; i += (size_t)gridDim.x * TPB) {
        const size_t row = i / rl4, j = i % rl4;
        Fp[i] = (row < (size_t)n && j < (size_t)rl) ? factor_ld(U, V, uv != 0, row * r + j) : 0.0;
        if (t && j == 0) tp[row] = row < (size_t)n ? t[row] : 1.0;
    }
}
// block blk's factor for src, packed to npad rows and rl4 = its rank rounded up to a multiple of 4 columns (t == nullptr: no tp)
int pack_factor(lorads_hip_ctx *c, int32_t src, int blk, int npad, const double *t, double *Fp, double *tp) {
    const Block &B = c->blk[blk];
    const int rl4 = (B.rl + 3) & ~3;
    const FactorView F = factor_view(c, src, blk);
    hipLaunchKernelGGL(k_pack_factor, dim3(std::min(grid1d((size_t)npad * rl4), 1024)), dim3(TPB), 0, c->stream, B.n, npad, B.rl, rl4, B.r,
                       F.U, F.V, F.uv, t, Fp, tp);
    HC(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ checks and refusals (0, or 1 with the message set)
// c, src and -- where the entry point takes one (blk != nullptr) -- the block.  The wording is the feature's: the `terse` entry points
// answer "<what>: bad argument" (one line for all their arguments), the others say which argument it is.
int postsolve_args(const lorads_hip_ctx *c, int32_t src, const int32_t *blk, const char *what, bool terse) {
    const bool src_ok = src == LORADS_HIP_PAIR_RR || src == LORADS_HIP_PAIR_UV;
    if (terse) return c && src_ok ? 0 : fail_msg(std::string(what) + ": bad argument");
    if (!c) return fail_msg(std::string(what) + ": no context");
    if (!src_ok) return fail_msg(std::string(what) + ": src " + std::to_string(src) + " is neither RR nor UV");
    if (blk && (*blk < 0 || *blk >= c->nb))
        return fail_msg(std::string(what) + ": block " + std::to_string(*blk) + " is outside [0, " + std::to_string(c->nb) + ")");
    return 0;
}
// sharded contexts (world > 1): "<what>: sharded contexts (world > 1) <cannot>".  The code it is refused with is the caller's (3; the
// export's is 1).
int postsolve_sharded(const lorads_hip_ctx *c, const char *what, const char *cannot) {
    if (!(c->ar || c->sep || c->sx)) return 0;
    return fail_msg(std::string(what) + ": sharded contexts (world > 1) " + cannot);
}

} // namespace
