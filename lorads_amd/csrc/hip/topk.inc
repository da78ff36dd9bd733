// topk.inc -- the k best entries per row of the primal X = F F^T, included by lorads_hip.hip after bounds.inc.  DESIGN.md section 17.
//
// Per SDP cone: F as lorads_hip_certificate takes it for src, at the cone's own rank.  For a query row p the candidates are the
// columns q of a window [col_lo, col_hi), minus q = p (unless include_diag), minus the query's skip list, minus every q whose X_pq
// is NaN.  X_pq is one chain of v_mfma_f64_16x16x4_f64 steps over the columns in fours, ascending, with the query row as the A
// operand and the candidate row as the B operand, both rows of the packed, zero-padded F of k_pack_factor (packed_dot's chain): its bits
// depend on the two rows alone, never on the window, k, the tile position or the other queries.  The chain starts from +0.0, so it
// never ends in -0.0: the value read back from a key (below) is the chain's own bits.
//   k_topk_gather  the query rows of the packed F, gathered into a packed query matrix of the same column padding
//   k_topk_scan    workgroup (I, s) owns the TOPK_T query rows of tile I and run s of the window's steps of TOPK_STEP columns: the
//                  16 x 64 tile of X on the FP64 matrix cores (one 16 x 16 per wavefront, the query strip in LDS up to
//                  TOPK_LDS_COLS columns), then every lane tests the four entries it holds against its row's threshold
//   k_topk_merge   when the window was split: one workgroup per query tile merges the runs' lists, (B - k) / k runs at a time
// The order is "X_pq descending (smallest: ascending), q ascending".  The key of a candidate is 64 bits of value -- the bits of
// v + 0.0 (so the two zeros are one value) mapped so that unsigned order is numeric order, complemented as a whole for `smallest`:
// the key is flipped, never the double -- above the column, compared ascending.  No valid key is 0 (NaN is no candidate), which is
// the pad.  No two candidates of one query share (key, column).
//
// Determinism.  A row of a workgroup keeps a buffer of TOPK_B (key, column) pairs in LDS and a threshold, the k-th best pair seen at
// the last prune (before the first: everything passes).  A lane whose candidate beats the threshold -- and, only then, is not in the
// query's sorted skip list -- appends it through an LDS cursor; the order of arrival is the hardware's.  Whether to prune is the result of the step's one barrier
// (the OR of the lanes' flags), so all 256 threads take the same decisions.  Before a step could overflow
// a row (cursor above TOPK_B - TOPK_STEP) the workgroup sorts that row with a bitonic network, keeps the best k and raises the
// threshold.  Since the pairs are unique and totally ordered, "the best k of a set" is a function of the set alone: whatever the
// arrival order, the buffer after a prune holds the same pairs in the same (sorted) places, every candidate dropped is beaten by k
// others of its row, and the final list is the best k of all candidates.  The same holds for the merge of the runs' lists: the best k
// of the union of the runs' best k.  So the same state and arguments give the same bytes, split or not.
// Read-only on the solver's state: scratch of its own (TopkScratch), launches straight to the stream (never through LAUNCH), LDS
// integer atomics only, no waiting between workgroups.

namespace {

constexpr int TOPK_T = 16;                // query rows of a tile (the A operand of all four wavefronts)
constexpr int TOPK_STEP = 64;             // columns of a step: 16 per wavefront
constexpr int TOPK_KMAX = 128;
constexpr int TOPK_LDS_COLS = 112;        // the query strip sits in LDS up to this many (padded) columns: 16 x 113 doubles = 14 KB beside
                                          // the 48 KB of the buffers at TOPK_B = 256; wider factors read it through the caches
constexpr int TOPK_MINSTEPS = 2;          // steps a run has at least: a window is split into runs of no fewer than 128 columns
constexpr int TOPK_MAXRUNS = 32;          // runs of a window at most: the merge walks them in sequence, (B - k) / k per pass, and a workgroup alone on
                                          // a CU walks a step in about 3 us -- beyond 32 runs the merge costs more than the longer runs (section 17)
constexpr int TOPK_BATCH = 16384;         // queries of one batch: 1024 tiles, at which nothing is split on any card up to 512 CUs
constexpr size_t TOPK_SKIP_BATCH = (size_t)1 << 22; // skip columns of one batch (a single query's de-duplicated list, at most n, may exceed it)
static_assert(TPB == 256, "k_topk_scan maps four wavefronts onto the four 16-column quarters of a step");

// rows' buffer capacity: room for the k kept and at least one step's appends after a prune
inline int topk_cap(int k) { return k <= 32 ? 128 : 256; }

struct TopkArgs {
    int nq, n, rl4, k, B, smallest, diag, in_lds;
    int lo, hi;                           // the window
    int step0, nsteps, sps, splits;       // first step of the window (columns step0 * 64 ...), its steps, steps per run, runs
    const double *Fp, *Qp;                // packed F [npad][rl4], packed queries [nqpad][rl4]
    const int *row;                       // [nq] the queries' own rows
    const long long *sptr;                // [nq + 1] or NULL
    const int *scol;                      // sorted, de-duplicated per query
    unsigned long long *pkey;             // runs' lists [nq][splits][k] (splits > 1)
    int *pcol, *pcnt;                     // [nq][splits][k], [nq][splits]
    int *idx, *found;                     // results [nq][k], [nq]
    double *val;
};

__device__ __forceinline__ unsigned long long topk_key(double v, int smallest) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);
    const unsigned long long key = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return smallest ? ~key : key;
}
__device__ __forceinline__ double topk_value(unsigned long long key, int smallest) {
    if (smallest) key = ~key;
    const unsigned long long b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
    return __longlong_as_double((long long)b);
}
// is (key a, column ca) before (b, cb) in the order?
__device__ __forceinline__ bool topk_before(unsigned long long a, unsigned ca, unsigned long long b, unsigned cb) {
    return a > b || (a == b && ca < cb);
}

// what a workgroup keeps per row of its query tile
struct TopkRows {
    unsigned long long *key;              // [TOPK_T][B]
    unsigned *col;                        // [TOPK_T][B]
    int *cur;                             // [TOPK_T] entries in the buffer
    unsigned long long *tkey;             // [TOPK_T] the threshold
    unsigned *tcol;
};

// Rows whose bit is set in `mask` (the same in every thread): pad to B, sort best first, keep the best k, set the threshold once k
// are held.  All 256 threads; barriers inside, the last one at the end.
__device__ void topk_prune(const TopkRows &R, int B, int k, unsigned mask) {
    for (int r = 0; r < TOPK_T; ++r) {
        if (!(mask >> r & 1)) continue;
        const int cnt = min(R.cur[r], B);
        for (int i = threadIdx.x; i < B; i += TPB)
            if (i >= cnt) { R.key[r * B + i] = 0; R.col[r * B + i] = 0xffffffffu; }
    }
    __syncthreads();
    for (int kk = 2; kk <= B; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int r = 0; r < TOPK_T; ++r) {
                if (!(mask >> r & 1)) continue;
                for (int i = threadIdx.x; i < B; i += TPB) {
                    const int l = i ^ j;
                    if (l <= i) continue;
                    const unsigned long long a = R.key[r * B + i], b = R.key[r * B + l];
                    const unsigned ca = R.col[r * B + i], cb = R.col[r * B + l];
                    const bool a_first = topk_before(a, ca, b, cb);
                    if ((i & kk) == 0 ? !a_first : a_first) {
                        R.key[r * B + i] = b; R.col[r * B + i] = cb;
                        R.key[r * B + l] = a; R.col[r * B + l] = ca;
                    }
                }
            }
            __syncthreads();
        }
    if (threadIdx.x < TOPK_T && (mask >> threadIdx.x & 1)) {
        const int r = threadIdx.x;
        int cnt = min(min(R.cur[r], B), k);
        while (cnt > 0 && R.key[r * B + cnt - 1] == 0) --cnt; // (pads the merge brought along: they sort last and count for nothing)
        R.cur[r] = cnt;
        if (cnt == k) { R.tkey[r] = R.key[r * B + k - 1]; R.tcol[r] = R.col[r * B + k - 1]; }
    }
    __syncthreads();
}

// the rows' sorted lists go out: as results (pkey == NULL) or as run `s` of the partial lists
__device__ void topk_emit(const TopkArgs &a, const TopkRows &R, int I, int s) {
    for (int e = threadIdx.x; e < TOPK_T * a.k; e += TPB) {
        const int r = e / a.k, j = e - r * a.k, qi = I * TOPK_T + r;
        if (qi >= a.nq) continue;
        const bool have = j < R.cur[r];
        const unsigned long long key = R.key[r * a.B + j];
        const unsigned col = R.col[r * a.B + j];
        if (s < 0) {
            a.idx[(size_t)qi * a.k + j] = have ? (int)col : -1;
            a.val[(size_t)qi * a.k + j] = have ? topk_value(key, a.smallest) : 0.0;
            if (j == 0) a.found[qi] = R.cur[r];
        } else {
            const size_t at = ((size_t)qi * a.splits + s) * a.k + j;
            if (have) { a.pkey[at] = key; a.pcol[at] = (int)col; }
            if (j == 0) a.pcnt[(size_t)qi * a.splits + s] = R.cur[r];
        }
    }
}

__device__ __forceinline__ bool topk_skipped(const TopkArgs &a, int qi, int col) {
    if (!a.sptr) return false;
    long long lo = a.sptr[qi], hi = a.sptr[qi + 1];
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        const int c = a.scol[mid];
        if (c == col) return true;
        if (c < col) lo = mid + 1; else hi = mid;
    }
    return false;
}

// dynamic LDS of both kernels: the keys, the strip (scan, in_lds), the columns
inline size_t topk_lds(int B, int rl4, int in_lds) {
    return sizeof(unsigned long long) * TOPK_T * (size_t)B + (in_lds ? sizeof(double) * TOPK_T * (size_t)(rl4 + 1) : 0) +
           sizeof(unsigned) * TOPK_T * (size_t)B;
}

__global__ __launch_bounds__(TPB) void k_topk_gather(int nq, int nqpad, int rl4, const int *__restrict__ row,
                                                     const double *__restrict__ Fp, double *__restrict__ Qp) {
    const size_t len = (size_t)nqpad * rl4;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < len; i += (size_t)gridDim.x * TPB) {
        const size_t q = i / rl4, j = i % rl4;
        Qp[i] = q < (size_t)nq ? Fp[(size_t)row[q] * rl4 + j] : 0.0;
    }
}

// The scan.  Wavefront w forms D = Q_I F_J^T for the 16 columns J = c0 + 16 w ... of the step (the operand layout of postsolve.inc's
// tiles: lane (nn, kk) supplies query row nn and candidate row nn at column k0 + kk and holds D[kk + 4 g][nn]: query kk + 4 g of the
// tile, candidate nn of the sixteen).  Both operands are rows of padded matrices with nothing to clamp; queries past nq, columns
// outside the window and rows past n produce no candidate: tested per entry, no branch around the MFMAs.
__global__ __launch_bounds__(TPB) void k_topk_scan(TopkArgs a) {
    extern __shared__ unsigned long long topk_sh[];
    __shared__ int cur[TOPK_T], qrow[TOPK_T];
    __shared__ unsigned long long tkey[TOPK_T];
    __shared__ unsigned tcol[TOPK_T];
    const int I = blockIdx.x, s = blockIdx.y, B = a.B, rl4 = a.rl4, ld = rl4 + 1;
    double *strip = (double *)(topk_sh + TOPK_T * B);
    TopkRows R{topk_sh, (unsigned *)(strip + (a.in_lds ? TOPK_T * ld : 0)), cur, tkey, tcol};
    if (threadIdx.x < TOPK_T) {
        const int qi = I * TOPK_T + threadIdx.x;
        cur[threadIdx.x] = 0; tkey[threadIdx.x] = 0; tcol[threadIdx.x] = 0xffffffffu;
        qrow[threadIdx.x] = (qi < a.nq && !a.diag) ? a.row[qi] : -1;
    }
    if (a.in_lds)
        for (int i = threadIdx.x; i < TOPK_T * rl4; i += TPB) {
            const int r = i / rl4, k = i - r * rl4;
            strip[r * ld + k] = a.Qp[(size_t)(I * TOPK_T + r) * rl4 + k];
        }
    __syncthreads();
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, nn = l & 15, kk = l >> 4;
    const double *ga = a.Qp + (size_t)(I * TOPK_T + nn) * rl4 + kk;
    const double *sa = strip + nn * ld + kk;
    const int t0 = a.step0 + s * a.sps, t1 = min(a.step0 + a.nsteps, t0 + a.sps);
    for (int t = t0; t < t1; ++t) {
        const int q = t * TOPK_STEP + 16 * wave + nn;     // (below npad: the packed F has whole steps of rows)
        const double *fb = a.Fp + (size_t)q * rl4 + kk;
        const v4f64 d = a.in_lds ? packed_dot(sa, fb, rl4) : packed_dot(ga, fb, rl4);
        const bool col_ok = q >= a.lo && q < a.hi;
        int near_full = 0;                                // did an append of this lane leave its row within a step of B?
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int r = kk + 4 * g, qi = I * TOPK_T + r;
            const double v = d[g];
            if (!(col_ok && qi < a.nq && v == v && q != qrow[r])) continue;
            const unsigned long long key = topk_key(v, a.smallest);
            if (!topk_before(key, (unsigned)q, tkey[r], tcol[r])) continue;
            if (topk_skipped(a, qi, q)) continue;
            const int slot = atomicAdd(&cur[r], 1);       // (below B: a row above B - TOPK_STEP was pruned before this step)
            if (slot < B) { R.key[r * B + slot] = key; R.col[r * B + slot] = (unsigned)q; }
            near_full |= slot + 1 > B - TOPK_STEP;
        }
        // one barrier per step, which also carries the decision: the OR over the workgroup of the lanes' own flags is the barrier's
        // result, the same value in all 256 threads by construction -- no flag in LDS that a later step could write while an earlier
        // one is still being read.  Without a prune nobody reads cur[] before the next barrier; with one, all do, then wait, then sort.
        if (__syncthreads_or(near_full)) {
            unsigned mask = 0;
            for (int r = 0; r < TOPK_T; ++r) mask |= (cur[r] > B - TOPK_STEP ? 1u : 0u) << r;
            __syncthreads();
            topk_prune(R, B, a.k, mask);
        }
    }
    unsigned mask = 0;
    for (int r = 0; r < TOPK_T; ++r) mask |= (cur[r] > 0 ? 1u : 0u) << r;
    __syncthreads();
    topk_prune(R, B, a.k, mask);
    topk_emit(a, R, I, a.splits > 1 ? s : -1);
}

// The merge: the runs' lists of a query tile through the same buffers and the same prune, as many runs at a time as fit beside the k
// kept: run c of a pass goes to the fixed place cur + c k of its row, the slots past its count padded (key 0: no candidate's).
__global__ __launch_bounds__(TPB) void k_topk_merge(TopkArgs a) {
    extern __shared__ unsigned long long topk_sh[];
    __shared__ int cur[TOPK_T];
    __shared__ unsigned long long tkey[TOPK_T];
    __shared__ unsigned tcol[TOPK_T];
    const int I = blockIdx.x, B = a.B, k = a.k, C = max(1, (B - k) / k);
    TopkRows R{topk_sh, (unsigned *)(topk_sh + TOPK_T * B), cur, tkey, tcol};
    if (threadIdx.x < TOPK_T) cur[threadIdx.x] = 0;
    __syncthreads();
    for (int s0 = 0; s0 < a.splits; s0 += C) {
        const int nc = min(C, a.splits - s0), span = nc * k;
        unsigned mask = 0;
        for (int r = 0; r < TOPK_T; ++r) mask |= (cur[r] + span > B ? 1u : 0u) << r;
        __syncthreads();
        if (mask) topk_prune(R, B, k, mask); // (to at most k: k + span <= B)
        for (int e = threadIdx.x; e < TOPK_T * span; e += TPB) {
            const int r = e / span, rem = e - r * span, c = rem / k, j = rem - c * k, qi = I * TOPK_T + r;
            if (qi >= a.nq) continue;
            const size_t ls = (size_t)qi * a.splits + s0 + c;
            const bool have = j < a.pcnt[ls];
            R.key[r * B + cur[r] + rem] = have ? a.pkey[ls * k + j] : 0ull;
            R.col[r * B + cur[r] + rem] = have ? (unsigned)a.pcol[ls * k + j] : 0xffffffffu;
        }
        __syncthreads();
        if (threadIdx.x < TOPK_T && I * TOPK_T + (int)threadIdx.x < a.nq) cur[threadIdx.x] += span;
        __syncthreads();
    }
    unsigned mask = 0;
    for (int r = 0; r < TOPK_T; ++r) mask |= (cur[r] > 0 ? 1u : 0u) << r;
    __syncthreads();
    topk_prune(R, B, k, mask);
    topk_emit(a, R, I, -1);
}

} // namespace

extern "C" int lorads_hip_primal_topk(lorads_hip_ctx *c, int32_t src, int32_t blk, int32_t nq, const int32_t *row, int32_t col_lo,
                                      int32_t col_hi, int32_t k, int32_t smallest, int32_t include_diag, const int64_t *skip_ptr,
                                      const int32_t *skip_col, int32_t *idx, double *val, int32_t *found) {
    spec_touch(c);
    const std::string w = "primal_topk: ";
    if (postsolve_args(c, src, &blk, "primal_topk", false)) return 1;
    if (c->blk[blk].is_lp) { fail_msg(w + "block " + std::to_string(blk) + " is the LP block: X is diagonal there, there are no rows to rank"); return 2; }
    const Block &B = c->blk[blk];
    const int n = B.n;
    if (nq < 0) return fail_msg(w + "nq " + std::to_string(nq) + " is negative");
    if (nq > 0 && !row) return fail_msg(w + "row must not be NULL when nq > 0");
    for (int i = 0; i < nq; ++i)
        if (row[i] < 0 || row[i] >= n)
            return fail_msg(w + "query " + std::to_string(i) + ": row " + std::to_string(row[i]) + " is outside [0, " + std::to_string(n) + ")");
    if (!(0 <= col_lo && col_lo <= col_hi && col_hi <= n))
        return fail_msg(w + "the window [" + std::to_string(col_lo) + ", " + std::to_string(col_hi) + ") is not within 0 <= lo <= hi <= " + std::to_string(n));
    if (k < 1 || k > TOPK_KMAX) return fail_msg(w + "k " + std::to_string(k) + " is outside [1, 128]");
    if (smallest != 0 && smallest != 1) return fail_msg(w + "smallest " + std::to_string(smallest) + " is neither 0 nor 1");
    if (include_diag != 0 && include_diag != 1) return fail_msg(w + "include_diag " + std::to_string(include_diag) + " is neither 0 nor 1");
    if ((skip_ptr == nullptr) != (skip_col == nullptr)) return fail_msg(w + "skip_ptr and skip_col: both or neither must be NULL");
    if (skip_ptr) {
        if (skip_ptr[0] != 0) return fail_msg(w + "skip_ptr does not start at 0");
        for (int i = 0; i < nq; ++i)
            if (skip_ptr[i + 1] < skip_ptr[i]) return fail_msg(w + "skip_ptr decreases at query " + std::to_string(i));
        for (int64_t e = 0; e < skip_ptr[nq]; ++e)
            if (skip_col[e] < 0 || skip_col[e] >= n)
                return fail_msg(w + "skip column " + std::to_string(skip_col[e]) + " (entry " + std::to_string(e) + ") is outside [0, " + std::to_string(n) + ")");
    }
    if (nq > 0 && (!idx || !val || !found)) return fail_msg(w + "idx, val and found must not be NULL when nq > 0");
    if (postsolve_sharded(c, "primal_topk", "are not supported")) return 3;
    for (int i = 0; i < nq; ++i) found[i] = 0;
    for (size_t e = 0; e < (size_t)nq * k; ++e) { idx[e] = -1; val[e] = 0.0; }
    if (nq == 0 || col_lo == col_hi) return 0;

    // the skip lists, sorted and de-duplicated per query (entries outside the window stay: they match no candidate)
    std::vector<long long> sp;
    std::vector<int> sc;
    if (skip_ptr) {
        sp.assign((size_t)nq + 1, 0);
        sc.reserve((size_t)skip_ptr[nq]);
        for (int i = 0; i < nq; ++i) {
            const size_t at = sc.size();
            sc.insert(sc.end(), skip_col + skip_ptr[i], skip_col + skip_ptr[i + 1]);
            std::sort(sc.begin() + (long)at, sc.end());
            sc.erase(std::unique(sc.begin() + (long)at, sc.end()), sc.end());
            sp[(size_t)i + 1] = (long long)sc.size();
        }
    }
    TopkScratch &X = c->topk;
    if (X.ncu == 0) {
        int dev = 0;
        HC(hipGetDevice(&dev));
        HC(hipDeviceGetAttribute(&X.ncu, hipDeviceAttributeMultiprocessorCount, dev));
    }
    const int rl4 = (B.rl + 3) & ~3, npad = nblocks_for((size_t)n, TOPK_STEP) * TOPK_STEP;
    if (X.Fp.grow(X.mem, (size_t)npad * rl4)) return 1;
    if (pack_factor(c, src, blk, npad, nullptr, X.Fp, nullptr)) return 1;
    TopkArgs a{};
    a.n = n; a.rl4 = rl4; a.k = k; a.B = topk_cap(k); a.smallest = smallest; a.diag = include_diag;
    a.in_lds = rl4 <= TOPK_LDS_COLS;
    a.lo = col_lo; a.hi = col_hi;
    a.step0 = col_lo / TOPK_STEP;
    a.nsteps = nblocks_for((size_t)col_hi, TOPK_STEP) - a.step0;
    a.Fp = X.Fp;
    for (int q0 = 0; q0 < nq;) {
        // a batch: at most TOPK_BATCH queries and, beyond its first query, TOPK_SKIP_BATCH skip columns
        int nb = std::min(nq - q0, TOPK_BATCH);
        if (skip_ptr) {
            int m = 1;
            while (m < nb && (size_t)(sp[(size_t)q0 + m + 1] - sp[(size_t)q0]) <= TOPK_SKIP_BATCH) ++m;
            nb = m;
        }
        const int qt = nblocks_for((size_t)nb, TOPK_T), nqpad = qt * TOPK_T;
        // the window is split only while the query tiles alone leave the card short of two workgroups per CU
        int splits = std::max(1, std::min({nblocks_for((size_t)2 * X.ncu, qt), a.nsteps / TOPK_MINSTEPS, TOPK_MAXRUNS}));
        a.sps = nblocks_for((size_t)a.nsteps, splits);
        a.splits = splits = nblocks_for((size_t)a.nsteps, a.sps);
        a.nq = nb;
        const size_t nsk = skip_ptr ? (size_t)(sp[(size_t)q0 + nb] - sp[(size_t)q0]) : 0;
        if (X.row.grow(X.mem, (size_t)nb) || X.Qp.grow(X.mem, (size_t)nqpad * rl4) || X.idx.grow(X.mem, (size_t)nb * k) ||
            X.val.grow(X.mem, (size_t)nb * k) || X.found.grow(X.mem, (size_t)nb))
            return 1;
        if (skip_ptr && (X.sptr.grow(X.mem, (size_t)nb + 1) || X.scol.grow(X.mem, nsk))) return 1;
        if (splits > 1 && (X.pkey.grow(X.mem, (size_t)nb * splits * k) || X.pcol.grow(X.mem, (size_t)nb * splits * k) ||
                           X.pcnt.grow(X.mem, (size_t)nb * splits)))
            return 1;
        HC(hipMemcpyAsync(X.row.p, row + q0, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, c->stream));
        std::vector<long long> spb;
        if (skip_ptr) {
            spb.resize((size_t)nb + 1);
            for (int i = 0; i <= nb; ++i) spb[(size_t)i] = sp[(size_t)q0 + i] - sp[(size_t)q0];
            HC(hipMemcpyAsync(X.sptr.p, spb.data(), sizeof(long long) * spb.size(), hipMemcpyHostToDevice, c->stream));
            if (nsk) HC(hipMemcpyAsync(X.scol.p, sc.data() + sp[(size_t)q0], sizeof(int) * nsk, hipMemcpyHostToDevice, c->stream));
        }
        a.Qp = X.Qp; a.row = X.row;
        a.sptr = skip_ptr ? X.sptr.p : nullptr; a.scol = X.scol;
        a.pkey = X.pkey; a.pcol = X.pcol; a.pcnt = X.pcnt;
        a.idx = X.idx; a.val = X.val; a.found = X.found;
        hipLaunchKernelGGL(k_topk_gather, dim3(std::min(grid1d((size_t)nqpad * rl4), 1024)), dim3(TPB), 0, c->stream, nb, nqpad, rl4,
                           (const int *)X.row.p, (const double *)X.Fp.p, X.Qp.p);
        HC(hipGetLastError());
        hipLaunchKernelGGL(k_topk_scan, dim3((unsigned)qt, (unsigned)splits), dim3(TPB), topk_lds(a.B, rl4, a.in_lds), c->stream, a);
        HC(hipGetLastError());
        if (splits > 1) {
            hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)qt), dim3(TPB), topk_lds(a.B, rl4, 0), c->stream, a);
            HC(hipGetLastError());
        }
        HC(hipMemcpyAsync(idx + (size_t)q0 * k, X.idx.p, sizeof(int) * (size_t)nb * k, hipMemcpyDeviceToHost, c->stream));
        HC(hipMemcpyAsync(val + (size_t)q0 * k, X.val.p, sizeof(double) * (size_t)nb * k, hipMemcpyDeviceToHost, c->stream));
        HC(hipMemcpyAsync(found + q0, X.found.p, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
        HC(hipStreamSynchronize(c->stream)); // (spb and the scratch are the next batch's)
        q0 += nb;
    }
    return 0;
}
