// bounds.inc -- separation of entry bounds on the primal X = F F^T, included by lorads_hip.hip after cuts.inc.  DESIGN.md section 15.
//
// Per SDP cone: F as lorads_hip_certificate takes it for src, at the cone's own rank.  Every pair p < q has two inequalities,
//   class 0:  X_pq >= lower,  v = lower - X_pq        class 1:  X_pq <= upper,  v = X_pq - upper
// and v > min_violation is a violation; an infinite bound gives v = -inf: the class is off with no test of its own.  X_pq is one chain
// of v_mfma_f64_16x16x4_f64 steps (postsolve.inc: packed_dot) over the columns in fours with row p as the A operand and row q as the
// B operand (as cut_tile forms F_x . F_y), then one subtraction: its bits depend on the two rows alone and every pass reproduces them.  All n (n - 1) of them
// are enumerated and never stored:
//   k_pack_factor (postsolve.inc)   F (the average of U and V formed once), zero-padded to whole tiles of BND_T rows and whole
//                steps of 4 columns
//   k_bnd_enum   workgroup (I, c) keeps rows of tile I of the packed F in LDS and walks the tiles J = I + BND_ITERS c ... (at most
//                BND_ITERS of them): the 32 x 32 tile of X on the FP64 matrix cores, one 16 x 16 quarter per wavefront, every thread
//                then tests the four entries it holds.  The three modes of select.inc.
// The key of a (pair, class) is 128 bits: the bit pattern of v above the complement of (p n + q) 2 + class -- "v descending, then p,
// q, class ascending"; the selection is select.inc's.  Read-only on the solver's state: the scratch is the feature's own
// (BoundScratch), launches go straight to the stream (never through LAUNCH).  No float atomics and no waiting between workgroups;
// the integer atomics of the counts, the histograms and the emit cursor commute, and the emitted keys are sorted, so the same state
// and arguments give the same bits.

namespace {

constexpr int BND_T = 32;                 // rows of a tile
constexpr int BND_ITERS = 16;             // tiles J one workgroup walks at most, as CUT_ITERS caps k_cut_enum
constexpr int BND_LDS_COLS = 128;         // the I strip sits in LDS up to this many (padded) columns: 32 x 129 doubles = 33 KB beside the
                                          // 16 KB histogram; wider factors read the strip through the caches like the J rows
constexpr int BND_MAXN = 1 << 24;         // tiles / BND_ITERS fits the grid's second dimension; (p n + q) 2 + class stays below 2^49
static_assert(TPB == 256, "k_bnd_enum maps four wavefronts onto the quarters of a tile");
static_assert((BND_MAXN / BND_T + BND_ITERS - 1) / BND_ITERS <= 65535, "grid.y");

struct BndArgs {
    int n, nt, rl4, mode, shift, width, in_lds;
    double lower, upper, minv;
    unsigned long long khi, klo;          // (these and mode, shift, width, minv, ctl, hist, ohi, olo, cap: select.inc's fields)
    const double *Fp;
    unsigned long long *ctl, *hist, *ohi, *olo;
    unsigned long long cap;
};

// The enumeration.  Wavefront w forms the quarter (w >> 1, w & 1) of the tile X[I][J] as D = F_I F_J^T in steps of four columns (the
// operand layout of postsolve.inc's tiles: lane (nn, kk) supplies row nn, column k0 + kk of both and holds D[kk + 4 g][nn]: row
// kk + 4 g of I's sixteen, row nn of J's), both operands rows of the packed, padded F with nothing to clamp.  Padding rows produce no
// pair: p < q < n is tested per entry.
__global__ __launch_bounds__(TPB) void k_bnd_enum(BndArgs a) {
    extern __shared__ double strip[];     // [BND_T][rl4 + 1] when a.in_lds
    __shared__ unsigned hist[CUT_BINS];
    __shared__ unsigned long long total;
    const int I = blockIdx.x, J0 = I + (int)blockIdx.y * BND_ITERS;
    if (J0 >= a.nt) return; // (the whole workgroup: no tile J is its own)
    const int J1 = min(a.nt, J0 + BND_ITERS), rl4 = a.rl4, ld = rl4 + 1;
    select_begin(a, hist, &total);
    if (a.in_lds)
        for (int i = threadIdx.x; i < BND_T * rl4; i += TPB) {
            const int row = i / rl4, k = i - row * rl4;
            strip[row * ld + k] = a.Fp[(size_t)(I * BND_T + row) * rl4 + k];
        }
    __syncthreads();
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, nn = l & 15, kk = l >> 4;
    const int la0 = 16 * (wave >> 1), lb0 = 16 * (wave & 1);
    const double *ga = a.Fp + (size_t)(I * BND_T + la0 + nn) * rl4 + kk;
    const double *sa = strip + (la0 + nn) * ld + kk;
    const unsigned long long n = (unsigned long long)a.n;
    SelAcc acc;
    for (int J = J0; J < J1; ++J) {
        const double *fb = a.Fp + (size_t)(J * BND_T + lb0 + nn) * rl4 + kk;
        const v4f64 d = a.in_lds ? packed_dot(sa, fb, rl4) : packed_dot(ga, fb, rl4);
        const int q = J * BND_T + lb0 + nn;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int p = I * BND_T + la0 + kk + 4 * g;
            if (!(p < q && q < a.n)) continue;
            const unsigned long long index = ((unsigned long long)p * n + (unsigned long long)q) * 2ull;
            select_item(a, a.lower - d[g], index, hist, acc);
            select_item(a, d[g] - a.upper, index + 1, hist, acc);
        }
    }
    // the selection's epilogue (select.inc): the same lines as k_cut_enum's
    if (a.mode == 2) return;
    if (acc.cur_n) atomicAdd(&hist[acc.cur_bin], acc.cur_n);
    if (a.mode == 0 && acc.cnt) atomicAdd(&total, acc.cnt);
    __syncthreads();
    if (a.mode == 0 && threadIdx.x == 0 && total) atomicAdd(a.ctl, total);
    for (int b = threadIdx.x; b < CUT_BINS; b += TPB)
        if (hist[b]) atomicAdd(a.hist + b, (unsigned long long)hist[b]);
}

int bnd_launch(lorads_hip_ctx *c, const BndArgs &a) {
    const size_t lds = a.in_lds ? sizeof(double) * BND_T * (size_t)(a.rl4 + 1) : 0;
    hipLaunchKernelGGL(k_bnd_enum, dim3((unsigned)a.nt, (unsigned)nblocks_for((size_t)a.nt, BND_ITERS)), dim3(TPB), lds, c->stream, a);
    HC(hipGetLastError());
    return 0;
}

} // namespace

extern "C" int lorads_hip_entry_bounds(lorads_hip_ctx *c, int32_t src, int32_t blk, double lower, double upper, double min_violation,
                                       int32_t max_cuts, int64_t *count, int32_t *p, int32_t *q, int8_t *cls, double *viol, int32_t *kept,
                                       int32_t *passes) {
    spec_touch(c);
    if (postsolve_args(c, src, &blk, "entry_bounds", false)) return 1;
    if (c->blk[blk].is_lp) return fail_msg("entry_bounds: block " + std::to_string(blk) + " is the LP block");
    if (select_check_range("entry_bounds", min_violation, max_cuts)) return 1;
    if (std::isnan(lower) || std::isnan(upper)) return fail_msg("entry_bounds: a bound is NaN");
    if (lower > upper) return fail_msg("entry_bounds: lower is above upper");
    if (lower == -INFINITY && upper == INFINITY) return fail_msg("entry_bounds: both classes are off (lower = -inf and upper = +inf)");
    if (lower == INFINITY || upper == -INFINITY) return fail_msg("entry_bounds: a bound is infinite on the wrong side");
    if (select_check_outputs("entry_bounds", "p, q, cls, viol and kept", max_cuts, count, p && q && cls && viol && kept)) return 1;
    if (c->blk[blk].n > BND_MAXN) return fail_msg("entry_bounds: cone dimension above 2^24");
    if (postsolve_sharded(c, "entry_bounds", "are not supported")) return 3;
    *count = 0;
    if (kept) *kept = 0;
    if (passes) *passes = 0;
    const Block &B = c->blk[blk];
    const int n = B.n;
    if (n < 2) return 0;
    BoundScratch &X = c->bounds;
    const int nt = nblocks_for((size_t)n, BND_T), npad = nt * BND_T, rl4 = (B.rl + 3) & ~3;
    BndArgs a{};
    if (X.Fp.grow(X.mem, (size_t)npad * rl4) || select_reserve(X.sel, X.mem, max_cuts, min_violation, a)) return 1;
    if (pack_factor(c, src, blk, npad, nullptr, X.Fp, nullptr)) return 1;
    a.n = n; a.nt = nt; a.rl4 = rl4;
    a.in_lds = rl4 <= BND_LDS_COLS;
    a.lower = lower; a.upper = upper;
    a.Fp = X.Fp;
    std::vector<unsigned long long> khi, klo;
    if (select_largest(c, "entry_bounds", max_cuts, a, [&] { return bnd_launch(c, a); }, count, passes, khi, klo))
        return 1;
    for (size_t e = 0; e < khi.size(); ++e) {
        unsigned long long idx = select_unpack(khi[e], klo[e], viol[e]);
        cls[e] = (int8_t)(idx & 1); idx >>= 1;
        q[e] = (int32_t)(idx % (unsigned long long)n);
        p[e] = (int32_t)(idx / (unsigned long long)n);
    }
    if (kept) *kept = (int32_t)khi.size();
    return 0;
}
