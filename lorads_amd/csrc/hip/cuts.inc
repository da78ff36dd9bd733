// cuts.inc -- separation of the triangle inequalities of +-1-structured contexts, included by lorads_hip.hip after primal.inc.
// DESIGN.md section 14.
//
// Per SDP cone: F as lorads_hip_certificate takes it for src, at the cone's own rank; rho_xy = (F_x . F_y) / (t_x t_y) with t of
// rounding.inc (rnd_check); for p < q < s and a = rho_pq, b = rho_ps, c = rho_qs the four violations are
//   v0 = (-1 - a) - (b + c)   v1 = (-1 - a) + (b + c)   v2 = (-1 + a) - (b - c)   v3 = (-1 + a) + (b - c)
// in exactly this order of operations.  All 4 C(n, 3) of them are enumerated and never stored:
//   k_pack_factor  (postsolve.inc) F (the average of U and V formed once) and t, zero-padded to whole tiles of CUT_T rows and whole
//                  steps of 4 columns
//   k_cut_enum     one workgroup per pair J <= K of row tiles keeps the tile rho[J][K] in LDS and walks the tiles I <= J: the tiles
//                  rho[I][J] and rho[I][K] on the FP64 matrix cores, then the workgroup's CUT_T^3 triples: a gate on the largest
//                  of the four v per triple, the triples that pass queued and handled densely.  Three modes:
//                  0 counts the pairs with v > min_violation and histograms the top digit of their keys, 1 histograms one digit of
//                  the keys under a prefix, 2 emits the keys at or above a threshold
// The key of a (triple, class) pair is 128 bits: the bit pattern of v (positive, so the patterns order as the values do) above the
// complement of ((p n + q) n + s) 4 + class -- larger keys come earlier in "v descending, then p, q, s, class ascending", and no two
// pairs share a key.  The selection is select.inc's radix select on the key (shared with bounds.inc): ties of v are told apart by
// the digits of the index, so any number of them is handled exactly.  Every pass enumerates anew (v is the same bits every time).
// On a cut-tightened context (DESIGN.md section 20) the pairs that are rows already are passed over: k_cut_enum<CutArgsPresent>.
// Read-only on the solver's state: the scratch is the feature's own (CutScratch), launches go straight to the stream (never through
// LAUNCH).  No float atomics; the integer atomics of the counts, the histograms and the emit cursor commute, and the emitted keys are
// sorted, so the same state and arguments give the same bits.

namespace {

constexpr int CUT_T = 32;                 // rows of a tile: 3 tiles of rho take 25 KB of LDS, the histogram 16 KB, the queue 8 KB
constexpr int CUT_LD = CUT_T + 1;
constexpr int CUT_QUEUE = 4096;           // triples of one tile triple (of 32768) queued in LDS for the dense pass
constexpr int CUT_MAXN = 1 << 20;         // the packed index ((p n + q) n + s) 4 + class stays below 2^62
constexpr int CUT_ITERS = 16;              // tiles I one workgroup walks at most (its 32-bit LDS bins hold 2^32 / 2^17 of them)
static_assert(CUT_T == 32, "k_cut_enum keeps one bit per s of a tile in a 32-bit word");
static_assert(TPB == 256, "k_cut_enum maps 256 threads onto a tile");

struct CutArgs {
    int n, rl4, mode, shift, width;
    double minv;
    unsigned long long khi, klo;          // (these and mode, shift, width, minv, ctl, hist, ohi, olo, cap: select.inc's fields)
    const double *Fp, *tp;
    unsigned long long *ctl, *hist, *ohi, *olo;
    unsigned long long cap;
};

// The arguments of the enumeration on a cone of a cut-tightened context (DESIGN.md section 20) that holds cuts: the sorted packed
// indices of the (triple, class) pairs that are rows of the problem already.  k_cut_enum<CutArgsPresent> passes over them in cut_handle,
// the dense pass, alone: the gate and the tiles are k_cut_enum<CutArgs>'s, which a cone without cuts launches as it always did.
struct CutArgsPresent : CutArgs {
    const unsigned long long *present;
    int npresent;
};
template <typename A> constexpr bool cut_excludes = false;
template <> constexpr bool cut_excludes<CutArgsPresent> = true;

// is `key` in the ascending list [0, n)?  (a binary search on the whole 64-bit packed index: past 2^32 for n > 1024)
__device__ __forceinline__ bool cut_listed(const unsigned long long *__restrict__ list, int n, unsigned long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && list[lo] == key;
}

// out <- the tile rho[A][B] (transposed: out[b][a]): wavefront w forms the 16 x 16 quarter (w >> 1, w & 1) as D = F_A F_B^T in steps of
// four columns (the operand layout of postsolve.inc's tiles: lane (nn, kk) supplies row nn, column k0 + kk of both and holds
// D[kk + 4 q][nn]; not mfma_fm_tile itself: both operands are rows of the packed, padded F, with nothing to clamp or mask), then
// divides by t_x t_y.  An entry's value depends on its two rows alone, not on the tile or the quarter it is formed in.
__device__ __forceinline__ void cut_tile(const CutArgs &a, int A, int B, double (*out)[CUT_LD], bool transposed) {
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, nn = l & 15, kk = l >> 4;
    const int la0 = 16 * (wave >> 1), lb0 = 16 * (wave & 1);
    const double *fa = a.Fp + (size_t)(A * CUT_T + la0 + nn) * a.rl4 + kk;
    const double *fb = a.Fp + (size_t)(B * CUT_T + lb0 + nn) * a.rl4 + kk;
    v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < a.rl4; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[k0], fb[k0], acc, 0, 0, 0);
    const double tb = a.tp[B * CUT_T + lb0 + nn];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int la = la0 + kk + 4 * q, lb = lb0 + nn;
        const double rho = acc[q] / (a.tp[A * CUT_T + la] * tb);
        if (transposed) out[lb][la] = rho; else out[la][lb] = rho;
    }
}

// One triple with a violated class, by its code (i << 10) | (j << 5) | sl inside the tiles at hand: the four v again from the same
// three rho in the same order of operations (the same bits as the gate saw), every class with v > min_violation counted, binned or
// emitted -- unless the problem holds it as a row already (CutArgsPresent).
template <typename A>
__device__ __forceinline__ void cut_handle(const A &a, unsigned code, int I, int J, int K, const double (*pq)[CUT_LD],
                                           const double (*ps)[CUT_LD], const double (*qs)[CUT_LD], unsigned *hist, SelAcc &acc) {
    const int i = code >> 10, j = (code >> 5) & 31, sl = code & 31;
    const double ra = pq[i][j], rb = ps[i][sl], rc = qs[sl][j];
    const double am = -1.0 - ra, ap = -1.0 + ra, sm = rb + rc, df = rb - rc;
    const double v[4] = {am - sm, am + sm, ap - df, ap + df};
    const unsigned long long n = (unsigned long long)a.n;
    const unsigned long long base = (((unsigned long long)(I * CUT_T + i) * n + (unsigned long long)(J * CUT_T + j)) * n +
                                     (unsigned long long)(K * CUT_T + sl)) * 4ull;
#pragma unroll
    for (int cl = 0; cl < 4; ++cl) { // (must match select.inc's select_item)
        if (!(v[cl] > a.minv)) continue;
        if constexpr (cut_excludes<A>)
            if (cut_listed(a.present, a.npresent, base + cl)) continue;
        const unsigned long long hi = (unsigned long long)__double_as_longlong(v[cl]), lo = ~(base + cl);
        if (a.mode == 2) {
            if (hi > a.khi || (hi == a.khi && lo >= a.klo)) {
                const unsigned long long slot = atomicAdd(a.ctl + 1, 1ull);
                if (slot < a.cap) { a.ohi[slot] = hi; a.olo[slot] = lo; }
            }
            continue;
        }
        ++acc.cnt;
        if (a.mode == 1 && !cut_same_prefix(hi, lo, a.khi, a.klo, a.shift + a.width)) continue;
        const int bin = (int)cut_digit(hi, lo, a.shift, a.width);
        if (bin != acc.cur_bin) {
            if (acc.cur_n) atomicAdd(&hist[acc.cur_bin], acc.cur_n);
            acc.cur_bin = bin; acc.cur_n = 0;
        }
        ++acc.cur_n;
    }
}

// The enumeration.  Thread (j = t & 31, ig = t >> 5) owns column q = 32 J + j and the rows p = 32 I + ig + 8 m, m < 4, whose rho_pq it
// keeps in registers as -1 - rho and -1 + rho (-inf where p < q < n fails: nothing passes the gate).  Per s it reads rho_qs once and
// rho_ps four times (two addresses per wavefront) and tests the gate max(v0, v1, v2, v3) = max((-1 - a) + |b + c|, (-1 + a) + |b - c|)
// > min_violation -- the same bits as the larger v (rounding is monotone and symmetric) -- into one bit per triple: no branch in the
// loop.  The few triples that pass are then queued in LDS by their code (one cursor step per thread) and handled by all threads,
// densely; what the queue cannot hold is handled on the spot.
template <typename A>
__global__ __launch_bounds__(TPB) void k_cut_enum(A a) {
    __shared__ double pq[CUT_T][CUT_LD], ps[CUT_T][CUT_LD], qs[CUT_T][CUT_LD]; // rho[p][q], rho[p][s], rho[q][s] as qs[s][q]
    __shared__ unsigned hist[CUT_BINS];
    __shared__ unsigned short queue[CUT_QUEUE];
    __shared__ unsigned qn;
    __shared__ unsigned long long total;
    // the pair J <= K of this workgroup: blockIdx.x = K (K + 1) / 2 + J
    const long long pi = blockIdx.x;
    long long Kl = (long long)((sqrt(8.0 * (double)pi + 1.0) - 1.0) / 2.0);
    while (Kl * (Kl + 1) / 2 > pi) --Kl;
    while ((Kl + 1) * (Kl + 2) / 2 <= pi) ++Kl;
    const int K = (int)Kl, J = (int)(pi - Kl * (Kl + 1) / 2);
    if ((int)blockIdx.y > J) return; // (the whole workgroup: no tile I is its own)
    select_begin(a, hist, &total);
    cut_tile(a, J, K, qs, true);
    const int n = a.n, j = threadIdx.x & 31, ig = threadIdx.x >> 5;
    const int q = J * CUT_T + j;
    const int s_lo = J == K ? j + 1 : 0, s_hi = min(CUT_T, n - K * CUT_T);
    const double minv = a.minv;
    SelAcc acc;
    for (int I = blockIdx.y; I <= J; I += gridDim.y) {
        __syncthreads();
        if (threadIdx.x == 0) qn = 0;
        cut_tile(a, I, J, pq, false);
        cut_tile(a, I, K, ps, false);
        __syncthreads();
        double am[CUT_T / 8], ap[CUT_T / 8];
#pragma unroll
        for (int m = 0; m < CUT_T / 8; ++m) {
            const int i = ig + 8 * m;
            const bool ok = q < n && (I < J || i < j);
            const double ra = pq[i][j];
            am[m] = ok ? -1.0 - ra : -INFINITY;
            ap[m] = ok ? -1.0 + ra : -INFINITY;
        }
        unsigned hit[CUT_T / 8];   // bit sl of hit[m]: the triple (ig + 8 m, j, sl) passes the gate
#pragma unroll
        for (int m = 0; m < CUT_T / 8; ++m) hit[m] = 0;
#pragma unroll 4
        for (int sl = 0; sl < s_hi; ++sl) {
            const double rc = qs[sl][j];
            const bool sok = sl >= s_lo;
#pragma unroll
            for (int m = 0; m < CUT_T / 8; ++m) {
                const double rb = ps[ig + 8 * m][sl];
                const double sm = rb + rc, df = rb - rc;
                hit[m] |= (unsigned)(sok && fmax(am[m] + fabs(sm), ap[m] + fabs(df)) > minv) << sl;
            }
        }
        const unsigned nh = __popc(hit[0]) + __popc(hit[1]) + __popc(hit[2]) + __popc(hit[3]);
        if (nh) {
            unsigned slot = atomicAdd(&qn, nh);
#pragma unroll
            for (int m = 0; m < CUT_T / 8; ++m)
                for (unsigned h = hit[m]; h; h &= h - 1, ++slot) {
                    const unsigned code = ((unsigned)(ig + 8 * m) << 10) | ((unsigned)j << 5) | (unsigned)(__ffs(h) - 1);
                    if (slot < CUT_QUEUE) queue[slot] = (unsigned short)code;
                    else cut_handle(a, code, I, J, K, pq, ps, qs, hist, acc);
                }
        }
        __syncthreads();
        const unsigned nq = min(qn, (unsigned)CUT_QUEUE);
        for (unsigned e = threadIdx.x; e < nq; e += TPB) cut_handle(a, queue[e], I, J, K, pq, ps, qs, hist, acc);
    }
    // the selection's epilogue (select.inc): the same lines as k_bnd_enum's
    if (a.mode == 2) return;
    if (acc.cur_n) atomicAdd(&hist[acc.cur_bin], acc.cur_n);
    if (a.mode == 0 && acc.cnt) atomicAdd(&total, acc.cnt);
    __syncthreads();
    if (a.mode == 0 && threadIdx.x == 0 && total) atomicAdd(a.ctl, total);
    for (int b = threadIdx.x; b < CUT_BINS; b += TPB)
        if (hist[b]) atomicAdd(a.hist + b, (unsigned long long)hist[b]);
}

template <typename A>
int cut_launch(lorads_hip_ctx *c, const A &a, int nt) {
    const long long npairs = (long long)nt * (nt + 1) / 2;
    // tiles I are dealt over blockIdx.y: at most CUT_ITERS per workgroup (the longest workgroups would otherwise run nt of them while
    // the device drains), and enough workgroups for a small cone
    const int split = (int)std::max<long long>(nblocks_for((size_t)nt, CUT_ITERS), std::min<long long>(nt, (2048 + npairs - 1) / npairs));
    hipLaunchKernelGGL(k_cut_enum<A>, dim3((unsigned)npairs, (unsigned)split), dim3(TPB), 0, c->stream, a);
    HC(hipGetLastError());
    return 0;
}

} // namespace

extern "C" int lorads_hip_triangle_cuts(lorads_hip_ctx *c, int32_t src, int32_t blk, double min_violation, int32_t max_cuts, int64_t *count,
                                        int32_t *p, int32_t *q, int32_t *s, int8_t *cls, double *viol, int32_t *kept, int32_t *passes) {
    spec_touch(c);
    if (postsolve_args(c, src, &blk, "triangle_cuts", false)) return 1;
    if (c->blk[blk].is_lp) return fail_msg("triangle_cuts: block " + std::to_string(blk) + " is the LP block");
    if (select_check_range("triangle_cuts", min_violation, max_cuts)) return 1;
    if (select_check_outputs("triangle_cuts", "p, q, s, cls, viol and kept", max_cuts, count, p && q && s && cls && viol && kept)) return 1;
    if (postsolve_sharded(c, "triangle_cuts", "are not supported")) return 3;
    if (rnd_check(c)) return 1;
    if (!c->rnd.qualifies) {
        fail_msg("triangle_cuts: the context is not +-1-structured: " + c->rnd.why);
        return 2;
    }
    *count = 0;
    if (kept) *kept = 0;
    if (passes) *passes = 0;
    const Block &B = c->blk[blk];
    const int n = B.n;
    if (n < 3) return 0;
    if (n > CUT_MAXN) return fail_msg("triangle_cuts: cone dimension above 2^20");
    CutScratch &X = c->cuts;
    const int nt = nblocks_for((size_t)n, CUT_T), npad = nt * CUT_T, rl4 = (B.rl + 3) & ~3;
    CutArgsPresent a{};
    if (X.Fp.grow(X.mem, (size_t)npad * rl4) || X.tp.grow(X.mem, (size_t)npad)) return 1;
    if (select_reserve(X.sel, X.mem, max_cuts, min_violation, a)) return 1;
    if (pack_factor(c, src, blk, npad, c->rnd.t + c->rnd.t_off[blk], X.Fp, X.tp)) return 1;
    a.n = n; a.rl4 = rl4;
    a.Fp = X.Fp; a.tp = X.tp;
    a.npresent = c->rnd.lpk >= 0 ? c->rnd.npresent[blk] : 0;
    a.present = a.npresent ? c->rnd.present[blk] : nullptr;
    std::vector<unsigned long long> khi, klo;
    if (select_largest(c, "triangle_cuts", max_cuts, a, [&] { return a.npresent ? cut_launch(c, a, nt) : cut_launch(c, static_cast<const CutArgs &>(a), nt); }, count, passes, khi, klo))
        return 1;
    const size_t want = khi.size();
    if (want == 0) return 0;
    for (size_t e = 0; e < (size_t)want; ++e) {
        unsigned long long idx = select_unpack(khi[e], klo[e], viol[e]);
        cls[e] = (int8_t)(idx & 3); idx >>= 2;
        s[e] = (int32_t)(idx % (unsigned long long)n); idx /= (unsigned long long)n;
        q[e] = (int32_t)(idx % (unsigned long long)n);
        p[e] = (int32_t)(idx / (unsigned long long)n);
    }
    *kept = (int32_t)want;
    return 0;
}
