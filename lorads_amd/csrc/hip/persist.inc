// persist.inc -- ONE launch per ADMM iteration for contexts whose cones are all of Max-Cut type (every A_i = a e_p e_p^T) with
// block-separable constraints (included by lorads_hip.hip inside its anonymous namespace, after sweep.inc).
//
// Reference path: LORADSUpdateSDPVar (lorads_alg/lorads_alg_common.c:187-215) = per cone LORADSUpdateSDPVarOne for U, constraint
// refresh, the same for V (lorads_alg/lorads_admm.c:428-480), each a CGSolve (linalg/lorads_cgs.c:81-240) on the operator
// linSysProduct (lorads_admm.c:376-391); then calObj_admm + LORADSCalDualObj + updateDimacsADMM (lorads_admm.c:79-81,310-337,
// lorads_alg_common.c:282-290), with the dual update of the previous iteration (lorads_alg_common.c:319-332) on board.
//
// Why: launch by launch such an iteration is 20-200 dependent kernels of ~3.5-5 us each whatever the cone's size (DESIGN 7, size
// sweep: 0.09-0.10 ms per iteration for every cone below n ~ 10000).  For these cones the CG operator is ROW-LOCAL,
//   (I + A_V^* A_V) x |_p = x_p + g_p (x_p . V_p) V_p ,   g_p = sum of a_i^2 over the constraints of row p,
// so a whole CG solve needs other rows only through its global dots.  Here every cone is solved by a TEAM of workgroups that stays
// resident for the whole iteration: a workgroup owns a tile of rows and keeps V_p, x_p, r_p, p_p of its rows in REGISTERS (rhs_p in
// LDS) from the solve's front to its last update; HBM sees the front's gather of neighbour rows and the final store.  The only
// cross-workgroup traffic inside a solve is the all-reduce of one or two scalars per step (team_allreduce below: tagged 8-byte
// granules written and polled with agent-scope accesses, every workgroup re-sums the same partials in the same order, so all of
// them take the same decisions -- alpha, beta, the stopping test of lorads_cgs.c:191, the k % 20 restart of :195-211 -- without a
// leader).  Teams are independent of each other: no lockstep between cones, no equal-rank condition (VERDICT r3 #1, #6).
//
// Hand-off rules followed (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement & inter-workgroup visibility"): bytes that cross
// workgroups inside the launch are stored with sc1 (write-through) stores, every storing wave drains (s_waitcnt vmcnt(0)) before
// its workgroup's barrier, and the workgroup publishes its granule only behind that barrier.  Granules (8-byte {half a double, tag}
// words) are read with sc1 loads; factor rows -- gathered by the next front, R rows by the objective -- with plain loads behind one
// agent-scope acquire per workgroup after the team barrier (pk_acquire).  Nothing depends on where a workgroup was placed.  Every spin is bounded (PK_TIMEOUT_TICKS of the
// 100 MHz clock): a team that cannot complete sets the abort word, everybody leaves, the host reports the failure.
// Residency: the grid is sized by the occupancy query (<= 2 workgroups per CU); the workgroups of a team are consecutive blocks.

constexpr int PK_KMAX = 5;     // doubles per all-reduce at most; granules of one parity: [PK_KMAX][len] pairs of 8-byte words, packed (a
                               // workgroup reads 16 contiguous bytes per lane and value)
constexpr int PK_SLOTW = 2 * PK_KMAX; // 8-byte words per slot and parity
constexpr int PK_GMAX = 1024;  // workgroups per team at most
constexpr int PK_TAGS_PER_LAUNCH = 16384; // tags a launch may use (2 (2 maxit + maxit / 20 + 4) + 8 must stay below)
constexpr unsigned long long PK_TIMEOUT_TICKS = 400000000ull; // 4 s of the 100 MHz clock

typedef unsigned int pk_v4u __attribute__((ext_vector_type(4)));
typedef double pk_d2 __attribute__((ext_vector_type(2)));

// Granule regions of a team (each [2 parities][PK_KMAX][len] pairs of {tag, half a double} words):
//   A  len G + ceil(G / 64): the placement-independent exchange (every store and load agent-scope): all workgroups, in one step
//      up to 64 of them, else sub-teams of 64 + their first members
//   F  len G: sub-team exchange through the XCD's L2 (plain stores, L1-bypassing loads) -- the sub-team = the team's workgroups on
//      blocks of one residue class mod 8, used only after the launch has VERIFIED that they sit on one XCD (see team_allreduce)
//   X  len 8: the sub-teams' first members among themselves (agent-scope)       B  len 8: first member -> its sub-team (L2)
struct PCone {
    int n, r, rows_k, G;       // rows, row stride (even), rows per 8-lane group (<= ROWS), workgroups of the team
    int rc_w, nc, st0, nsub;   // constraints per row (fixed width), unused, index of the cone's first CG state, sub-teams
    unsigned long long off;    // element offset of the cone in the flat factor arrays
    const int *adj_ptr, *adj_col, *adj_dyn;
    const double *adj_sval;
    const int *rc_con;
    const double *diag_a, *gdiag;
    const int *row_idx;        // null: the cone sees every constraint in file order
    double *cv;
    unsigned long long *slA, *slF, *slX, *slB;
};
struct PMap { int cone, wl, si, ssz, sid, soff, cls, pad; }; // block -> {cone (-1: idle), index in the team, index in / size of / number of
                                                              // its sub-team, first F slot of the sub-team, block number mod 8}
struct PArgs {
    const PCone *cones;
    const PMap *wg_map;
    int ncones;
    double *U, *V, *R;
    unsigned int fbytes;       // bytes of a flat factor array (buffer range)
    double *csum;
    const double *b;
    double *lambda;
    double rho, tol, rho_dual;
    int maxit, dual_on, with_eval;
    CGState *st;
    unsigned int tag0;
    double *team_out;          // [ncones][4]
    unsigned long long *arrive, arrive_target;
    int *abort_flag;
    // hand-over (the last team to arrive): publish = 1 control block -> pinned mirror + sequence number; 0: nothing (the caller
    // enqueues its own hand-over); loc_word >= 0: the evaluation's local sums also go to scal[loc_word .. +4) (separable shards)
    int publish, loc_word;
    double *scal, *sepbuf;
    unsigned long long *ctrl_src, *ctrl_dst;
    int nwords;
    unsigned long long *flag, *seq_dev;
    unsigned long long *stamps; // null, or [16] ticks of team 0's leader at its phase boundaries (bench)
    int allow_l2;               // 0: never the L2 forms (LORADS_PERSIST_L2=0)
    // The objective's part of the fronts' gathers, (C X)_p = sum_q c_pq X_q, depends on the factor gathered and on nothing else, and
    // the evaluation needs <C, R R^T> = sum_p R_p . ((C U)_p + (C V)_p) / 2 (R = (U + V) / 2): (C U) is what the V front has just
    // gathered, so the evaluation gathers V instead of R -- and (C V) is exactly what the NEXT iteration's U front would gather
    // again.  cv_out: the evaluation leaves (C V) in CX; cv_in: the U front reads its rows back instead of gathering (the host
    // knows whether V has been touched in between).  Two gathers per iteration instead of three.
    double *CX;
    int cv_in, cv_out;
};

struct PTeam {
    unsigned long long *slA, *slF, *slX, *slB;
    int G, wl, si, ssz, sid, nsub, soff;
    unsigned int tag;
    int *abort_flag;
    int dead; // (uniform over the workgroup)
    int l2;   // this launch has verified the placement: sub-team exchanges go through the XCD's L2
};

__device__ __forceinline__ pk_d2 pk_ld16(__amdgpu_buffer_rsrc_t rs, unsigned off) {
    return __builtin_bit_cast(pk_d2, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0)); // plain (L1 / L2): see pk_acquire
}
__device__ __forceinline__ void pk_st16(__amdgpu_buffer_rsrc_t rs, unsigned off, double a, double b, bool wt) {
    pk_d2 v;
    v.x = a; v.y = b;
    if (wt) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(pk_v4u, v), rs, (int)off, 0, 16); // aux 16 = sc1: written through
    else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(pk_v4u, v), rs, (int)off, 0, 0);      // stays in the XCD's L2
}
// what a workgroup does between the team barrier that follows the other workgroups' sc1 stores of factor rows and its own plain
// loads of those rows: one lane's agent-scope acquire (this CU's L1 is invalidated), its wait, the workgroup's barrier
// (MI355X_MICROARCH.md, valid consumer form: poll -> ONE agent acquire -> s_waitcnt vmcnt(0) -> __syncthreads() -> plain loads)
// A pointer that came out of memory (the PCone table) is a generic pointer to the compiler: loads through it are flat_load, which
// return out of order and count on the LDS counter too -- every wait behind one becomes vmcnt(0) + lgkmcnt(0), and a gather's row
// loads get serialised behind the next trip's index loads.  These say what the pointers are: global memory.
template <class T> __device__ __forceinline__ T pk_gld(const T *p, size_t i) {
    typedef const T __attribute__((address_space(1))) *G;
    return ((G)p)[i];
}
template <class T> __device__ __forceinline__ void pk_gst(T *p, size_t i, T v) {
    typedef T __attribute__((address_space(1))) *G;
    ((G)p)[i] = v;
}
__device__ __forceinline__ void pk_acquire() {
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
}
// one factor row (byte offset row0 inside the buffer), the lane's column slices; inactive: zeros
template <int NS>
__device__ __forceinline__ void pk_load_row(__amdgpu_buffer_rsrc_t rs, unsigned row0, int r, int lane, bool act, double (&v)[NS][2]) {
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const int j = (lane + c * 8) * 2;
        // (a slice that does not exist asks beyond the buffer's range and the hardware answers 0: nothing looks at the loaded value
        // before its real consumer, so a batch of loads stays a batch)
        const pk_d2 t = pk_ld16(rs, (j < r && act) ? row0 + (unsigned)j * 8u : 0x7ffffff0u);
        v[c][0] = t.x;
        v[c][1] = t.y;
    }
}
template <int NS>
__device__ __forceinline__ void pk_store_row(__amdgpu_buffer_rsrc_t rs, unsigned row0, int r, int lane, bool act, const double (&v)[NS][2], bool wt) {
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const int j = (lane + c * 8) * 2;
        if (act && j < r) pk_st16(rs, row0 + (unsigned)j * 8u, v[c][0], v[c][1], wt);
    }
}
// Sums over 8 lanes / the wavefront on the DPP path (two 32-bit moves + one add per step; __shfl_xor on a double is two
// ds_bpermute round trips per step, ~0.3 us per wave sum, and a CG iteration has half a dozen of them on its critical path).
// Every lane ends with the same bits (each step adds the same two partial sums in either order).
template <int CTRL>
__device__ __forceinline__ double pk_dpp(double v) {
    const long long b = __double_as_longlong(v);
    int lo = (int)b, hi = (int)(b >> 32);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double pk_readlane(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double pk_sum8(double v) { // lanes 8 k .. 8 k + 7 (all 64 lanes active)
    v += pk_dpp<0xB1>(v);  // quad_perm [1,0,3,2]
    v += pk_dpp<0x4E>(v);  // quad_perm [2,3,0,1]
    v += pk_dpp<0x141>(v); // row_half_mirror
    return v;
}
__device__ __forceinline__ double pk_sum64(double v) { // (all 64 lanes active)
    v = pk_sum8(v);
    v += pk_dpp<0x140>(v); // row_mirror: the row's two halves
    return (pk_readlane(v, 0) + pk_readlane(v, 16)) + (pk_readlane(v, 32) + pk_readlane(v, 48));
}
// a workgroup's resident rows to LDS and back ([ROWS][NS][TPB] 16-byte words: consecutive threads, consecutive words)
template <int NS, int ROWS>
__device__ __forceinline__ void pk_park(pk_d2 *l, const double (&v)[ROWS][NS][2]) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
        for (int c = 0; c < NS; ++c) { pk_d2 t; t.x = v[j][c][0]; t.y = v[j][c][1]; l[(j * NS + c) * TPB + threadIdx.x] = t; }
}
template <int NS, int ROWS>
__device__ __forceinline__ void pk_unpark(const pk_d2 *l, double (&v)[ROWS][NS][2]) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
        for (int c = 0; c < NS; ++c) { const pk_d2 t = l[(j * NS + c) * TPB + threadIdx.x]; v[j][c][0] = t.x; v[j][c][1] = t.y; }
}
__device__ __forceinline__ unsigned long long pk_ticks() { return wall_clock64(); } // the constant 100 MHz counter

// Granule traffic of wave 0.  A slot region of one parity: [K][len] pairs of {tag, half a double} 8-byte words; every word carries
// its own tag, so a reader needs no ordering between the words.  l2 = false: agent-scope stores and loads (written through to
// memory, read past L1 and a possibly stale L2 line: valid wherever the workgroups sit).  l2 = true: plain stores (they stay in
// the XCD's L2) and the same L1-bypassing loads, which that L2 serves -- valid between workgroups of ONE XCD only.
template <int K>
__device__ __forceinline__ void pk_publish(unsigned long long *base, int len, int idx, unsigned tag, int wl, const double (&s)[K], bool l2) {
    if (wl < 2 * K) {
        const int k = wl >> 1;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(s[k]);
        const unsigned long long half = (wl & 1) ? (bits & 0xffffffffull) : (bits >> 32);
        unsigned long long *p = base + ((size_t)k * len + idx) * 2 + (wl & 1);
        const unsigned long long word = ((unsigned long long)tag << 32) | half;
        if (l2) __hip_atomic_store(p, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_store(p, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// lane l collects slots first + l, first + l + 64, ... (< first + cnt) as they arrive; s <- their sum, lanes in butterfly order (the
// same bits in every workgroup that collects the same slots).  Returns non-zero if the team has given up: every spin is bounded.
template <int K>
__device__ __forceinline__ int pk_collect(PTeam &T, const unsigned long long *base, int len, int first, int cnt, unsigned tag, int wl,
                                          double (&s)[K]) {
    int bad = 0;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int g = first + wl; g < first + cnt && !bad; g += 64) {
        unsigned lo[2 * K];
        unsigned long long t0 = 0;
        for (unsigned spins = 0;; ++spins) {
            bool ok = true;
#pragma unroll
            for (int w = 0; w < 2 * K; ++w) {
                const unsigned long long word = __hip_atomic_load(base + ((size_t)(w >> 1) * len + g) * 2 + (w & 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = ok && (unsigned)(word >> 32) == tag;
                lo[w] = (unsigned)word;
            }
            if (ok) break;
            __builtin_amdgcn_s_sleep(1);
            if ((spins & 63u) == 63u) { // every so often: has somebody given up, or is it time to?
                if (__hip_atomic_load(T.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { bad = 1; break; }
                const unsigned long long now = pk_ticks();
                if (t0 == 0) t0 = now;
                else if (now - t0 > PK_TIMEOUT_TICKS) {
                    __hip_atomic_store(T.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    bad = 1;
                    break;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += __longlong_as_double((long long)(((unsigned long long)lo[2 * k] << 32) | lo[2 * k + 1]));
    }
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = pk_sum64(acc[k]);
    return __any(bad) ? 1 : 0;
}

// All-reduce of K doubles over the team, result in every thread of every workgroup, the same bits everywhere.  Two workgroup
// barriers per call: the waves leave their sums in LDS; wave 0 adds them, exchanges granules with the team and leaves the result in
// LDS.  sh: 64 doubles + 2 ints behind them, used in halves by call parity (a call never writes what the previous call's readers
// may still be reading).  drain: this workgroup has stores in flight that other workgroups read after this call.
// The exchange, by what the launch knows about its placement:
//   T.l2 == 0 (always the launch's first call): region A, agent scope -- one step for teams of up to 64 workgroups, else sub-teams
//     of 64 and then their first members' sums, published by each sub-team's first member and collected by everybody;
//   T.l2 == 1: the sub-team (one XCD, verified) exchanges through its L2 (region F); with several sub-teams their first members
//     exchange the sub-team sums at agent scope (region X: at most eight pollers on those lines) and hand the total back to their
//     sub-team through the L2 (region B).  Every first member adds the same sub-team sums in the same order.
template <int K>
__device__ __forceinline__ void team_allreduce(PTeam &T, double (&v)[K], double *sh, bool drain) {
    static_assert(K <= PK_KMAX, "slot too small");
    if (drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int wave = threadIdx.x >> 6, wl = threadIdx.x & 63;
    const unsigned tag = ++T.tag; // (every thread counts along)
    double *shp = sh + (tag & 1u) * 32;
    int *shd = (int *)(sh + 64);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = pk_sum64(v[k]);
        if (wl == 0) shp[k * 4 + wave] = v[k];
    }
    __syncthreads();
    if (wave == 0) {
        double s[K];
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] = (shp[k * 4] + shp[k * 4 + 1]) + (shp[k * 4 + 2] + shp[k * 4 + 3]);
        int bad = 0;
        if (T.G > 1 && !T.dead) {
            const size_t par = tag & 1u;
            if (T.l2) {
                unsigned long long *bF = T.slF + par * T.G * PK_SLOTW;
                pk_publish<K>(bF, T.G, T.soff + T.si, tag, wl, s, true);
                bad = pk_collect<K>(T, bF, T.G, T.soff, T.ssz, tag, wl, s);
                if (T.nsub > 1 && !bad) {
                    unsigned long long *bX = T.slX + par * 8 * PK_SLOTW, *bB = T.slB + par * 8 * PK_SLOTW;
                    if (T.si == 0) {
                        pk_publish<K>(bX, 8, T.sid, tag, wl, s, false);
                        bad = pk_collect<K>(T, bX, 8, 0, T.nsub, tag, wl, s);
                        if (!bad) pk_publish<K>(bB, 8, T.sid, tag, wl, s, true);
                    } else {
                        bad = pk_collect<K>(T, bB, 8, T.sid, 1, tag, wl, s);
                    }
                }
            } else {
                const int n64 = (T.G + 63) >> 6, sb = T.wl >> 6, g0 = sb << 6, sz = T.G - g0 < 64 ? T.G - g0 : 64, nA = T.G + n64;
                unsigned long long *bA = T.slA + par * nA * PK_SLOTW;
                pk_publish<K>(bA, nA, T.wl, tag, wl, s, false);
                bad = pk_collect<K>(T, bA, nA, g0, sz, tag, wl, s);
                if (n64 > 1 && !bad) {
                    if ((T.wl & 63) == 0) pk_publish<K>(bA, nA, T.G + sb, tag, wl, s, false);
                    bad = pk_collect<K>(T, bA, nA, T.G, n64, tag, wl, s);
                }
            }
        }
        if (wl == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) shp[24 + k] = s[k];
            shd[tag & 1u] = bad;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = shp[24 + k];
    if (shd[tag & 1u]) T.dead = 1;
}

// What a lane group keeps about its rows for the length of the launch (ROWS <= 2; otherwise fetched again in front of each use):
// the adjacency row's start and length, this lane's slot of its first trip, the lane's constraint of the row (-1: none), that
// constraint's index in the m-vectors and its coefficient.  All static data of the cone: the three gathers and the three weight
// computations of an iteration start two to three dependent memory round trips later without it.
template <int ROWS>
struct PRowInfo {
    int t0[ROWS], len[ROWS], q0[ROWS], ci[ROWS], gI[ROWS];
    double sv0[ROWS], ai[ROWS];
};
template <int ROWS>
__device__ __forceinline__ void pk_row_info(const PCone &C, const int (&row)[ROWS], const bool (&act)[ROWS], int lane, PRowInfo<ROWS> &I) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int rowc = act[j] ? row[j] : 0;
        I.t0[j] = pk_gld(C.adj_ptr, rowc);
        I.len[j] = act[j] ? pk_gld(C.adj_ptr, rowc + 1) - I.t0[j] : 0;
        I.ci[j] = (lane < C.rc_w && act[j]) ? pk_gld(C.rc_con, (size_t)rowc * C.rc_w + lane) : -1;
    }
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        int tc = lane < I.len[j] ? I.t0[j] + lane : I.t0[j] + I.len[j] - 1;
        tc = tc < 0 ? 0 : tc;
        I.q0[j] = pk_gld(C.adj_col, tc);
        I.sv0[j] = pk_gld(C.adj_sval, tc);
        const int cic = I.ci[j] >= 0 ? I.ci[j] : 0;
        I.gI[j] = C.row_idx ? pk_gld(C.row_idx, cic) : cic;
        I.ai[j] = pk_gld(C.diag_a, cic);
    }
}

// acc[j] = sum over the adjacency slots of row j of c_slot * X_q -- the OBJECTIVE's part of (C + sum_i w_i A_i) X, the list carries
// its coefficients -- for ALL the lane group's rows at once (X: the buffer rs, cone base byte offset cb).  (The constraints' part of
// a Max-Cut-type cone sits on the row's own diagonal: the caller adds (sum_i w_i a_i) X_p from the row it holds.)  Eight slots per
// trip and row (lane l holds slot l: one coalesced index load per array and trip, the next trip's requested before this one's rows
// are consumed), CHR neighbour rows of EVERY row in flight together: the dependent chain of a gather is (trips x 8 / CHR batches),
// whatever the number of rows a lane group owns.  A row that has run out of slots rides along with coefficient 0 on its last
// neighbour.
template <int NS, int ROWS>
__device__ __forceinline__ void pk_gather(__amdgpu_buffer_rsrc_t rs, unsigned cb, int r, const PCone &C, const PRowInfo<ROWS> &I, int lane,
                                          double (&acc)[ROWS][NS][2]) {
    // neighbour rows in flight per lane in all (what the compiler fits without spilling next to the rows parked in LDS; deeper batches
    // were measured and are no faster: 16 at two rows per lane group took the 2-cone shard's fronts from 16.9 to 18.5 us)
    constexpr int CHT = NS <= 2 ? 8 : NS == 3 ? (ROWS == 1 ? 4 : 8) : NS == 4 ? (ROWS == 1 ? 8 : 4) : 2;
    constexpr int CHR = CHT / ROWS >= 1 ? CHT / ROWS : 1;
    int qn[ROWS];
    double svn[ROWS];
    int lmax = 0;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        lmax = I.len[j] > lmax ? I.len[j] : lmax;
        qn[j] = I.q0[j]; svn[j] = I.sv0[j];
#pragma unroll
        for (int c = 0; c < NS; ++c) { acc[j][c][0] = 0.0; acc[j][c][1] = 0.0; }
    }
    const unsigned rb = (unsigned)r * 8u;
    for (int off = 0; off < lmax; off += 8) {
        int q[ROWS];
        double s1[ROWS];
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            q[j] = qn[j];
            s1[j] = off + lane < I.len[j] ? svn[j] : 0.0;
            const int tn = off + 8 + lane;
            int tc = tn < I.len[j] ? I.t0[j] + tn : I.t0[j] + I.len[j] - 1;
            tc = tc < 0 ? 0 : tc;
            qn[j] = pk_gld(C.adj_col, tc); svn[j] = pk_gld(C.adj_sval, tc);
        }
#pragma unroll
        for (int u0 = 0; u0 < 8; u0 += CHR) {
            if (u0 == 0 || off + u0 < lmax) {
                double v[ROWS][CHR][NS][2];
#pragma unroll
                for (int j = 0; j < ROWS; ++j)
#pragma unroll
                    for (int u = 0; u < CHR; ++u) {
                        const int qq = __shfl(q[j], u0 + u, 8);
                        pk_load_row<NS>(rs, cb + (unsigned)qq * rb, r, lane, true, v[j][u]);
                    }
                // (nothing crosses this line: the batch's loads are ALL requested before the first of them is consumed -- left to
                // itself the scheduler has been seen to issue them one by one between the multiply-adds, one memory round trip each)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < ROWS; ++j)
#pragma unroll
                    for (int u = 0; u < CHR; ++u) {
                        const double a1 = __shfl(s1[j], u0 + u, 8);
#pragma unroll
                        for (int c = 0; c < NS; ++c) { acc[j][c][0] += a1 * v[j][u][c][0]; acc[j][c][1] += a1 * v[j][u][c][1]; }
                    }
            }
        }
    }
}

__device__ __forceinline__ void pk_store_state(CGState *st, double rr, double bnorm, double beta, int done, int iter, int nan) {
    unsigned long long *w = (unsigned long long *)st; // {rr, bnorm, beta, {done, iter}, {nan, pad}}
    __hip_atomic_store(w + 0, (unsigned long long)__double_as_longlong(rr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 1, (unsigned long long)__double_as_longlong(bnorm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 2, (unsigned long long)__double_as_longlong(beta), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 3, ((unsigned long long)(unsigned)iter << 32) | (unsigned)done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 4, (unsigned long long)(unsigned)nan | (1ull << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int NS, int ROWS>
__global__ __launch_bounds__(TPB, 2) void k_admm_diag(PArgs A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    pk_d2 *rhs_l = (pk_d2 *)lds;                          // [ROWS][NS][TPB]: the solve's right-hand side
    pk_d2 *park_l = rhs_l + ROWS * NS * TPB;              // [ROWS][NS][TPB]: where resident rows wait while a gather runs
    double *sh = lds + 4 * ROWS * NS * TPB;               // 64 + 2 ints (team_allreduce)
    int *shi = (int *)(sh + 66);                          // 4
    const PMap mp = A.wg_map[blockIdx.x];
    if (mp.cone < 0) return;
    const PCone C = A.cones[mp.cone];
    PTeam T;
    T.slA = C.slA; T.slF = C.slF; T.slX = C.slX; T.slB = C.slB;
    T.G = C.G; T.wl = mp.wl; T.si = mp.si; T.ssz = mp.ssz; T.sid = mp.sid; T.nsub = C.nsub; T.soff = mp.soff;
    T.tag = A.tag0; T.abort_flag = A.abort_flag; T.l2 = 0;
    T.dead = __hip_atomic_load(A.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ? 1 : 0; // (uniform: one word)
    // Which XCD is this?  Blocks are dealt to the XCDs round robin (observed, not promised), so block b should sit on XCD (b + d) mod 8
    // for ONE d of the launch.  Every workgroup brings its own d to the launch's first all-reduce (agent scope, placement-independent):
    // if all of the team's agree, the workgroups of one residue class mod 8 share an XCD and its L2, and from then on their granules
    // (and, where the team is a single class, their factor rows) go through that L2.  If not: nothing changes but the speed.
    const int xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 7; // hwreg(HW_REG_XCC_ID, 0, 4)
    const double dplace = (double)((xcc - mp.cls) & 7);
    bool rows_l2 = false; // the team's factor rows stay in the XCD's L2 (plain stores) instead of being written through
    const int grp = threadIdx.x >> 3, lane = threadIdx.x & 7;
    const int r = C.r;
    const unsigned rb = (unsigned)r * 8u, cb = (unsigned)(C.off * 8ull);
    const __amdgpu_buffer_rsrc_t rsU = __builtin_amdgcn_make_buffer_rsrc((void *)A.U, 0, A.fbytes, 0x00020000),
                                 rsV = __builtin_amdgcn_make_buffer_rsrc((void *)A.V, 0, A.fbytes, 0x00020000),
                                 rsR = __builtin_amdgcn_make_buffer_rsrc((void *)A.R, 0, A.fbytes, 0x00020000),
                                 rsC = __builtin_amdgcn_make_buffer_rsrc((void *)A.CX, 0, A.CX ? A.fbytes : 0, 0x00020000);
    const bool stamp = A.stamps && mp.cone == 0 && mp.wl == 0 && threadIdx.x == 0;
    int nstamp = 0;
    if (stamp) A.stamps[nstamp++] = pk_ticks();
    int row[ROWS];
    bool act[ROWS];
    double gd[ROWS];
    double fx[ROWS][NS][2], xv[ROWS][NS][2]; // the fixed factor and the solve variable of the running half: (V, U), then (U, V)
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        row[j] = (T.wl * C.rows_k + j) * 32 + grp;
        act[j] = j < C.rows_k && row[j] < C.n;
        const int rc = act[j] ? row[j] : 0;
        gd[j] = act[j] ? pk_gld(C.gdiag, rc) : 0.0;
        pk_load_row<NS>(rsV, cb + (unsigned)rc * rb, r, lane, act[j], fx[j]);
        pk_load_row<NS>(rsU, cb + (unsigned)rc * rb, r, lane, act[j], xv[j]);
    }
    // (a lane group with more than two rows has no registers to spare for this: its copy is fetched again in front of each use)
    constexpr bool KEEP = ROWS <= 2;
    PRowInfo<ROWS> I;
    pk_row_info<ROWS>(C, row, act, lane, I);
    const double rho = A.rho, tol = A.tol;

#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        const __amdgpu_buffer_rsrc_t rsF = half == 0 ? rsV : rsU, rsX = half == 0 ? rsU : rsV;
        double rv[ROWS][NS][2], pv[ROWS][NS][2];
        // ---- front: rhs = F - (C + sum_i M1_i A_i) F / rho (lorads_admm.c:432-463), r0 = rhs - (x + g (x.F) F) (lorads_cgs.c:149-156)
        // (the front's all-reduce also carries p_0 . Q_0 of iteration 0: p_0 = r_0 is known before anybody knows whether the solve runs)
        double three0[3] = {0.0, 0.0, 0.0};
        double dq[ROWS];
        double dyn_add[ROWS];
        if (!KEEP) pk_row_info<ROWS>(C, row, act, lane, I);
        // the rows' sum_i weight_i a_i, weight_i = rho (constrValSum - constrVal_k - b)_i - lambda_i (:432-445), formed as weight_of forms
        // it; the operands are requested here and used behind the gather
        double w_cs[ROWS], w_bb[ROWS], w_cv[ROWS], w_lam[ROWS];
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int cic = I.ci[j] >= 0 ? I.ci[j] : 0;
            w_cs[j] = A.csum[I.gI[j]]; w_bb[j] = A.b[I.gI[j]]; w_lam[j] = A.lambda[I.gI[j]]; w_cv[j] = pk_gld((const double *)C.cv, cic);
        }
        // While the gather runs nobody needs the resident rows: they wait in LDS (x in the right-hand side's place, which the
        // epilogue below fills only after reading x back) and the gather has the registers for rows in flight.  (The compiler is
        // told nothing about the detour: the clobber keeps it from carrying the values across in registers after all.)
        double accA[ROWS][NS][2];
        const bool carried = half == 0 && A.cv_in != 0; // (C V)_p of these rows was left behind by the previous launch's evaluation
        pk_park<NS, ROWS>(rhs_l, xv);
        pk_park<NS, ROWS>(park_l, fx);
        asm volatile("" ::: "memory");
        {
            PRowInfo<ROWS> Ig = I; // (carried: rows of length 0 -- the gather has nothing to do, its code stays what it is)
#pragma unroll
            for (int j = 0; j < ROWS; ++j) Ig.len[j] = carried ? 0 : I.len[j];
            pk_gather<NS, ROWS>(rsF, cb, r, C, Ig, lane, accA);
        }
        asm volatile("" ::: "memory");
        pk_unpark<NS, ROWS>(rhs_l, xv);
        pk_unpark<NS, ROWS>(park_l, fx);
        if (carried) {
#pragma unroll
            for (int j = 0; j < ROWS; ++j) pk_load_row<NS>(rsC, cb + (unsigned)(act[j] ? row[j] : 0) * rb, r, lane, act[j], accA[j]);
        }
        // (C U)_p waits for the evaluation where the fixed factor waited a moment ago (nobody parks anything during the solve)
        if (half == 1 && A.cv_out) pk_park<NS, ROWS>(park_l, accA);
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            double lm = w_lam[j];
            if (half == 0 && A.dual_on) { // LORADSUpdateDualVar of the previous iteration (lorads_alg_common.c:319-332), as k_dual_update forms it
                const double l = lm + A.rho_dual * w_bb[j];
                lm = l + (-A.rho_dual) * w_cs[j];
                if (I.ci[j] >= 0) A.lambda[I.gI[j]] = lm;
            }
            const double wgt = (((w_cs[j] - w_bb[j]) - w_cv[j]) * rho - lm) * I.ai[j];
            dyn_add[j] = pk_sum8(I.ci[j] >= 0 ? wgt : 0.0);
#pragma unroll
            for (int c = 0; c < NS; ++c) { // the constraints' part: (sum_i weight_i a_i) F_p on the row's own diagonal
                accA[j][c][0] = fma(dyn_add[j], fx[j][c][0], accA[j][c][0]);
                accA[j][c][1] = fma(dyn_add[j], fx[j][c][1], accA[j][c][1]);
            }
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const double (&acc)[NS][2] = accA[j];
            double dd = 0.0;
#pragma unroll
            for (int c = 0; c < NS; ++c) dd += xv[j][c][0] * fx[j][c][0] + xv[j][c][1] * fx[j][c][1];
            dd = pk_sum8(dd) * gd[j];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                pk_d2 vb;
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    const double b0 = fx[j][c][w] - acc[c][w] / rho;
                    three0[1] += fabs(b0);
                    const double opx = xv[j][c][w] + dd * fx[j][c][w];
                    const double r0 = b0 - opx;
                    three0[0] += r0 * r0;
                    rv[j][c][w] = r0;
                    pv[j][c][w] = r0; // p_0 = r_0 (lorads_cgs.c:163-166)
                    if (w == 0) vb.x = b0; else vb.y = b0;
                }
                rhs_l[(j * NS + c) * TPB + threadIdx.x] = vb;
            }
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < NS; ++c) d += pv[j][c][0] * fx[j][c][0] + pv[j][c][1] * fx[j][c][1];
            d = pk_sum8(d) * gd[j];
            dq[j] = d;
#pragma unroll
            for (int c = 0; c < NS; ++c)
#pragma unroll
                for (int w = 0; w < 2; ++w) three0[2] += pv[j][c][w] * (pv[j][c][w] + d * fx[j][c][w]); // p . Q, Q = p + g (p.F) F
        }
        if (half == 0) { // the launch's first all-reduce: also the placement words (thread 0 of every workgroup: d and d^2)
            double five[5] = {three0[0], three0[1], three0[2], threadIdx.x == 0 ? dplace : 0.0, threadIdx.x == 0 ? dplace * dplace : 0.0};
            team_allreduce<5>(T, five, sh, false);
            three0[0] = five[0]; three0[1] = five[1]; three0[2] = five[2];
            // all d equal  <=>  G sum d^2 == (sum d)^2  (small integers: exact)
            if (A.allow_l2 && T.G > 1 && (double)T.G * five[4] == five[3] * five[3]) { T.l2 = 1; rows_l2 = T.nsub == 1; }
            if (stamp) A.stamps[15] = 1ull | (T.l2 ? 2ull : 0ull) | (rows_l2 ? 4ull : 0ull); // (what this launch decided, for the tests)
        } else team_allreduce<3>(T, three0, sh, false);
        if (stamp && nstamp < 15) A.stamps[nstamp++] = pk_ticks();
        double rr = three0[0], beta = 0.0, pq = three0[2];
        const double bnorm = three0[1];
        int done = sqrt(rr) / bnorm < tol ? 2 : 0, iter = 0, nan = 0; // (lorads_cgs.c:156-160)
        // ---- CG iterations (lorads_cgs.c:174-234)
        for (int k = 0; !done && !T.dead; ++k) {
            if (k > 0) {
                double one[1] = {0.0};
#pragma unroll
                for (int j = 0; j < ROWS; ++j) {
                    double d = 0.0;
#pragma unroll
                    for (int c = 0; c < NS; ++c) d += pv[j][c][0] * fx[j][c][0] + pv[j][c][1] * fx[j][c][1];
                    d = pk_sum8(d) * gd[j];
                    dq[j] = d;
#pragma unroll
                    for (int c = 0; c < NS; ++c)
#pragma unroll
                        for (int w = 0; w < 2; ++w) one[0] += pv[j][c][w] * (pv[j][c][w] + d * fx[j][c][w]);
                }
                team_allreduce<1>(T, one, sh, false);
                pq = one[0];
            }
            const double alpha = rr / pq; // (:181-183)
            const bool restart = k % 20 == 0;
            double two[2] = {0.0, 0.0};
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
#pragma unroll
                for (int c = 0; c < NS; ++c)
#pragma unroll
                    for (int w = 0; w < 2; ++w) {
                        xv[j][c][w] = xv[j][c][w] + alpha * pv[j][c][w];                                // (:185)
                        const double t = rv[j][c][w] - alpha * (pv[j][c][w] + dq[j] * fx[j][c][w]);   // (:188)
                        rv[j][c][w] = t;
                        two[0] += t * t;
                    }
                if (restart) {
                    // k % 20 == 0: should the solve go on, it restarts from the true residual rhs - (x + g (x.F) F) (:195-211).  Its norm
                    // travels with the stopping test's sum -- the residual carried so far is not read again either way
                    double d = 0.0;
#pragma unroll
                    for (int c = 0; c < NS; ++c) d += xv[j][c][0] * fx[j][c][0] + xv[j][c][1] * fx[j][c][1];
                    d = pk_sum8(d) * gd[j];
#pragma unroll
                    for (int c = 0; c < NS; ++c) {
                        const pk_d2 rh = rhs_l[(j * NS + c) * TPB + threadIdx.x];
#pragma unroll
                        for (int w = 0; w < 2; ++w) {
                            const double t = (w == 0 ? rh.x : rh.y) - (xv[j][c][w] + d * fx[j][c][w]);
                            rv[j][c][w] = t;
                            two[1] += t * t;
                        }
                    }
                }
            }
            if (restart) team_allreduce<2>(T, two, sh, false);
            else { double one[1] = {two[0]}; team_allreduce<1>(T, one, sh, false); two[0] = one[0]; }
            const double a = two[0];
            iter = k + 1;
            if (a != a) nan = 1;
            beta = a / rr;
            rr = a;
            done = sqrt(a) / bnorm < tol ? 1 : (iter >= A.maxit ? 3 : 0); // (:189-194)
            if (done) break;
            if (restart) { // beta = qTrNew / qTr = 1 after a restart: p = 2 r (:212-221)
                rr = two[1];
                beta = 1.0;
#pragma unroll
                for (int j = 0; j < ROWS; ++j)
#pragma unroll
                    for (int c = 0; c < NS; ++c)
#pragma unroll
                        for (int w = 0; w < 2; ++w) pv[j][c][w] = rv[j][c][w] + rv[j][c][w];
            } else {
#pragma unroll
                for (int j = 0; j < ROWS; ++j)
#pragma unroll
                    for (int c = 0; c < NS; ++c)
#pragma unroll
                        for (int w = 0; w < 2; ++w) pv[j][c][w] = fma(beta, pv[j][c][w], rv[j][c][w]); // (:217-221)
            }
        }
        if (stamp && nstamp < 15) A.stamps[nstamp++] = pk_ticks();
        if (!KEEP) pk_row_info<ROWS>(C, row, act, lane, I);
        // ---- the solve's result: the new rows of x (read by the other workgroups' next gather), the constraint refresh
        //      constrVal_k <- A_k(sym(U V^T)), constrValSum += new - old (lorads_alg_common.c:199-203), the solve's state
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int rc = act[j] ? row[j] : 0;
            if (done != 2) pk_store_row<NS>(rsX, cb + (unsigned)rc * rb, r, lane, act[j], xv[j], !rows_l2);
            double dd = 0.0;
#pragma unroll
            for (int c = 0; c < NS; ++c) dd += xv[j][c][0] * fx[j][c][0] + xv[j][c][1] * fx[j][c][1];
            dd = pk_sum8(dd);
            const int ci = I.ci[j];
            if (ci >= 0 && !(half == 1 && A.with_eval)) { // (dead before an evaluation: it overwrites both vectors, quirk Q1)
                const int gI = I.gI[j];
                const double s = I.ai[j] * dd, old = pk_gld((const double *)C.cv, ci);
                A.csum[gI] = A.csum[gI] + (s - old);
                pk_gst(C.cv, ci, s);
            }
        }
        if (T.wl == 0 && threadIdx.x == 0) pk_store_state(A.st + C.st0 + half, rr, bnorm, beta, done, iter, nan);
        if (half == 0) {
            // every row of U must be in memory before anybody's V front gathers it
            double z[1] = {0.0};
            team_allreduce<1>(T, z, sh, true);
            pk_acquire();
#pragma unroll
            for (int j = 0; j < ROWS; ++j)
#pragma unroll
                for (int c = 0; c < NS; ++c)
#pragma unroll
                    for (int w = 0; w < 2; ++w) { const double t = fx[j][c][w]; fx[j][c][w] = xv[j][c][w]; xv[j][c][w] = t; }
        }
    }
    // here fx = U, xv = V
    double three[3] = {0.0, 0.0, 0.0};
    if (A.with_eval) {
        // ---- evaluation: R = (U + V) / 2 (averageUV, lorads_admm.c:310-323), constrVal <- A(R R^T), constrValSum <- (quirk Q1),
        //      partials of ||b - A(R R^T)||^2 and b.lambda (lorads_alg_common.c:250-258,282-290,334-340), <C, R R^T> (lorads_admm.c:325-337)
        double av[ROWS][NS][2];
        if (!KEEP) pk_row_info<ROWS>(C, row, act, lane, I);
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int rc = act[j] ? row[j] : 0;
            double rn = 0.0;
#pragma unroll
            for (int c = 0; c < NS; ++c)
#pragma unroll
                for (int w = 0; w < 2; ++w) { av[j][c][w] = (fx[j][c][w] + xv[j][c][w]) / 2; rn += av[j][c][w] * av[j][c][w]; }
            pk_store_row<NS>(rsR, cb + (unsigned)rc * rb, r, lane, act[j], av[j], !rows_l2);
            rn = pk_sum8(rn);
            const int ci = I.ci[j];
            if (ci >= 0) {
                const int gI = I.gI[j];
                const double bi = A.b[gI], s = I.ai[j] * rn, t = bi - s;
                A.csum[gI] = s;
                pk_gst(C.cv, ci, s);
                three[0] += t * t;
                three[1] += bi * A.lambda[gI];
            }
        }
        { // every row of R in memory before the objective's gather
            double z[1] = {0.0};
            team_allreduce<1>(T, z, sh, true);
            pk_acquire();
        }
        { // <C, R R^T> = sum_p R_p . (C R)_p.  cv_out: (C R)_p = ((C U)_p + (C V)_p) / 2 with (C U) kept from the V front, so V is gathered
          // (in memory since the V solve's stores; the barrier above covers them) and (C V) stays behind for the next launch;
          // otherwise R itself is gathered ((x + x) / 2 = x: one expression for both)
            double accA[ROWS][NS][2];
            pk_park<NS, ROWS>(rhs_l, av); // (the right-hand side is dead; park_l may hold (C U))
            asm volatile("" ::: "memory");
            pk_gather<NS, ROWS>(A.cv_out ? rsV : rsR, cb, r, C, I, lane, accA);
            asm volatile("" ::: "memory");
            pk_unpark<NS, ROWS>(rhs_l, av);
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                if (A.cv_out) pk_store_row<NS>(rsC, cb + (unsigned)(act[j] ? row[j] : 0) * rb, r, lane, act[j], accA[j], false); // (read by this workgroup's next launch)
#pragma unroll
                for (int c = 0; c < NS; ++c) {
                    const pk_d2 cu = park_l[(j * NS + c) * TPB + threadIdx.x];
                    const double o0 = A.cv_out ? cu.x : accA[j][c][0], o1 = A.cv_out ? cu.y : accA[j][c][1];
                    three[2] += av[j][c][0] * ((o0 + accA[j][c][0]) / 2) + av[j][c][1] * ((o1 + accA[j][c][1]) / 2);
                }
            }
        }
        team_allreduce<3>(T, three, sh, false);
    }
    if (stamp && nstamp < 15) A.stamps[nstamp++] = pk_ticks();
    if (T.wl != 0) return;
    // ---- the team reports; the last team to arrive sums the teams' numbers in cone order and hands everything over
    if (threadIdx.x == 0) {
        unsigned long long *o = (unsigned long long *)(A.team_out + 4 * (size_t)mp.cone);
        __hip_atomic_store(o + 0, (unsigned long long)__double_as_longlong(three[0]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 1, (unsigned long long)__double_as_longlong(three[1]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 2, (unsigned long long)__double_as_longlong(three[2]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long old = __hip_atomic_fetch_add(A.arrive, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        shi[0] = old + 1 == A.arrive_target ? 1 : 0;
    }
    __syncthreads();
    if (!shi[0]) return;
    double tot[3] = {0.0, 0.0, 0.0};
    if (threadIdx.x == 0) {
        for (int k = 0; k < A.ncones; ++k) {
            const unsigned long long *o = (const unsigned long long *)(A.team_out + 4 * (size_t)k);
#pragma unroll
            for (int q = 0; q < 3; ++q)
                tot[q] += __longlong_as_double((long long)__hip_atomic_load(o + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
        const int ab = __hip_atomic_load(A.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (A.with_eval) { A.scal[0] = tot[0]; A.scal[1] = tot[1]; A.scal[2] = tot[2]; }
        A.scal[7] = ab ? 1.0 : 0.0;
        if (A.loc_word >= 0) { A.scal[A.loc_word] = tot[0]; A.scal[A.loc_word + 1] = tot[1]; A.scal[A.loc_word + 2] = A.with_eval ? tot[2] : 0.0; A.scal[A.loc_word + 3] = 0.0; }
        if (A.sepbuf) { A.sepbuf[0] = tot[0]; A.sepbuf[1] = tot[1]; A.sepbuf[2] = A.with_eval ? tot[2] : 0.0; A.sepbuf[3] = 0.0; }
        sh[0] = tot[0]; sh[1] = tot[1]; sh[2] = tot[2]; sh[3] = ab ? 1.0 : 0.0;
    }
    __syncthreads();
    if (stamp && nstamp < 15) A.stamps[nstamp++] = pk_ticks();
    if (!A.publish) return;
    const unsigned long long seq = *A.seq_dev + 1;
    for (int i = threadIdx.x; i < A.nwords; i += TPB) {
        unsigned long long w = __hip_atomic_load(A.ctrl_src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (A.with_eval && i < 3) w = (unsigned long long)__double_as_longlong(sh[i]);
        if (i == 7) w = (unsigned long long)__double_as_longlong(sh[3]);
        if (A.loc_word >= 0 && i >= A.loc_word && i < A.loc_word + 4)
            w = (unsigned long long)__double_as_longlong(i - A.loc_word < 3 ? ((i - A.loc_word == 2 && !A.with_eval) ? 0.0 : sh[i - A.loc_word]) : 0.0);
        A.ctrl_dst[i] = w;
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        *A.seq_dev = seq;
        __atomic_store_n(A.flag, seq, __ATOMIC_RELEASE);
        __threadfence_system();
    }
}

// ------------------------------------------------------------------ host side
struct PersistPlan {
    bool valid = false, failed = false;
    int ns = 0, rows = 0, grid = 0, occ = 0, ncu = 0;
    int g_max = 0, nsub_max = 0, ssz_max = 0; // largest team, most sub-teams of a team, largest sub-team (lorads_hip_persist_plan)
    bool xcd_map = false;      // every team on the blocks of one residue class mod 8 (one XCD under round-robin placement: speed only)
    size_t lds = 0;
    std::vector<int> sig;      // what the plan was built for: {n, r} of every cone
    PCone *d_cones = nullptr;
    PMap *d_map = nullptr;
    unsigned long long *gran = nullptr;
    size_t gran_words = 0;
    double *team_out = nullptr;
    unsigned long long *arrive = nullptr;
    unsigned long long launches = 0;
    unsigned int tag = 0;
    int *abort_flag = nullptr;
    unsigned long long *stamps = nullptr, *h_stamps = nullptr;
    double *cx = nullptr;      // (C V)_p of every row, from one launch's evaluation to the next launch's U front
    bool cx_ok = false;        // ... and whether it still belongs to the V in memory (persist_touch: every writer of V or C clears it)
    DevPool mem;
    void release() {
        mem.release();
        d_cones = nullptr; d_map = nullptr; gran = nullptr; team_out = nullptr; arrive = nullptr; abort_flag = nullptr; stamps = nullptr; h_stamps = nullptr;
        cx = nullptr; cx_ok = false;
        valid = false;
    }
};

typedef void (*pk_kernel_t)(PArgs);
pk_kernel_t pk_kernel(int ns, int rows) {
#define PKK(NSV, RV) if (ns == NSV && rows == RV) return k_admm_diag<NSV, RV>
    PKK(1, 1); PKK(1, 2); PKK(1, 4); PKK(2, 1); PKK(2, 2); PKK(2, 4); PKK(3, 1); PKK(3, 2); PKK(4, 1); PKK(4, 2);
    PKK(5, 1); PKK(6, 1); PKK(7, 1); PKK(8, 1);
#undef PKK
    return nullptr;
}
inline size_t pk_lds_bytes(int ns, int rows) { return sizeof(double) * ((size_t)4 * rows * ns * TPB + 66) + 16; }

// may this context's ADMM iteration run as the one-launch form at all?
bool persist_eligible(const lorads_hip_ctx *c) {
    if (!c->opt.persist || c->nb < 1 || c->m <= 0 || shard_vec(c)) return false;
    if (c->nb > 1 && !c->merged_ok) return false; // (merged_ok <=> no LP block, no dense cone, every constraint in exactly one cone)
    long long nrow = 0;
    for (const auto &B : c->blk) {
        if (!B.diag_only || B.rc_w <= 0 || B.dense_c || B.dense_a || B.is_lp || B.pu.ne <= 0 || B.n <= 0 || (B.r & 1) || B.r > 128) return false;
        nrow += B.nrow;
    }
    if (nrow != c->m) return false; // (a constraint no cone holds would miss its share of the residual)
    if (c->all_elem * 8 >= (size_t)0x7ffffff0u) return false; // (32-bit buffer offsets; pk_load_row's out-of-range address)
    return true;
}

int persist_build(lorads_hip_ctx *c) {
    PersistPlan &P = *c->persist;
    P.release();
    P.sig.clear();
    for (const auto &B : c->blk) { P.sig.push_back(B.n); P.sig.push_back(B.r); }
    int ns = 1;
    for (const auto &B : c->blk) ns = std::max(ns, (B.r + 15) / 16);
    int dev = 0, ncu_dev = 0;
    HC(hipGetDevice(&dev));
    HC(hipDeviceGetAttribute(&ncu_dev, hipDeviceAttributeMultiprocessorCount, dev)); // (hipGetDeviceProperties takes milliseconds)
    const int force_rows = c->opt.persist_rows; // (LORADS_PERSIST_ROWS: measurements and tests)
    const int cand[3] = {1, 2, 4};
    for (int ci = 0; ci < 3 && !P.valid; ++ci) {
        const int rows = cand[ci];
        if (force_rows && rows != force_rows) continue;
        pk_kernel_t kern = pk_kernel(ns, rows);
        if (!kern) continue;
        const size_t lds = pk_lds_bytes(ns, rows);
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)kern, TPB, lds) != hipSuccess) { (void)hipGetLastError(); continue; }
        // (256-thread blocks at .sgpr_count ~100: the hardware admits six per CU, MI355X_MICROARCH.md "Residency and cooperative launch")
        const int cap = std::min(occ, 4) * ncu_dev;
        long long total = 0;
        bool ok = true;
        for (const auto &B : c->blk) {
            const int G = nblocks_for((size_t)B.n, 32 * rows);
            ok = ok && G <= PK_GMAX;
            total += G;
        }
        if (!ok || total > cap) continue;
        P.ns = ns; P.rows = rows; P.grid = (int)total; P.lds = lds; P.occ = std::min(occ, 4); P.ncu = ncu_dev;
        P.valid = true;
    }
    if (!P.valid) { P.failed = true; return 0; }
    std::vector<PCone> cones(c->nb);
    std::vector<std::pair<int, int>> blocks; // block -> (cone, index in the team); (-1, 0): idle
    for (int k = 0; k < c->nb; ++k) {
        const Block &B = c->blk[k];
        PCone &C = cones[k];
        C.n = B.n; C.r = B.r; C.rows_k = P.rows; C.G = nblocks_for((size_t)B.n, 32 * P.rows);
        C.rc_w = B.rc_w; C.nc = B.nc; C.st0 = 2 * k; C.nsub = 1;
        C.off = B.off;
        C.adj_ptr = B.pu.adj_ptr; C.adj_col = B.pu.adj_col; C.adj_dyn = B.pu.adj_dyn; C.adj_sval = B.pu.adj_sval;
        C.rc_con = B.rc_con; C.diag_a = B.diag_a; C.gdiag = B.gdiag; C.row_idx = B.row_idx_identity ? nullptr : B.row_idx;
        C.cv = B.cv;
        for (int g = 0; g < C.G; ++g) blocks.push_back({k, g});
    }
    { // Teams to XCDs.  Blocks are dealt to the eight XCDs round robin by number (observed, not promised: it buys speed, nothing
      // else depends on it), so the blocks {x + 8 s} share XCD x and its L2.  A team whose workgroups all sit there gathers its
      // cone's factor rows -- stored by the team itself a moment ago -- out of ONE 4 MB L2 that holds just the cones of that XCD
      // (cfg4: two cones of 576 KB per factor) instead of every XCD fetching every cone's rows, and exchanges its granules
      // through that L2.  Possible when every team fits the CUs of one XCD and the teams can be dealt so that no XCD is overbooked
      // (largest first to the emptiest XCD); otherwise the blocks are dealt team by team and a team's workgroups of one residue
      // class mod 8 form its sub-teams (LORADS_PERSIST_MAP=linear forces that)
        const int cap_x = P.occ * (P.ncu / 8);
        std::vector<int> order(c->nb), load(8, 0), xcd_of(c->nb, 0);
        for (int k = 0; k < c->nb; ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cones[a].G > cones[b].G; });
        bool ok = !c->opt.persist_linear && P.ncu % 8 == 0;
        for (int k : order) {
            int x = 0;
            for (int y = 1; y < 8; ++y) if (load[y] < load[x]) x = y;
            xcd_of[k] = x;
            load[x] += cones[k].G;
            ok = ok && load[x] <= cap_x;
        }
        P.xcd_map = ok;
        if (ok) {
            int depth = 0;
            for (int x = 0; x < 8; ++x) depth = std::max(depth, load[x]);
            blocks.assign((size_t)8 * depth, {-1, 0});
            std::vector<int> fill(8, 0);
            for (int k = 0; k < c->nb; ++k) // (cone order within an XCD: the order of the file)
                for (int g = 0; g < cones[k].G; ++g) blocks[(size_t)8 * (fill[xcd_of[k]]++) + xcd_of[k]] = {k, g};
        }
        P.grid = (int)blocks.size();
    }
    // sub-teams: a team's workgroups by residue class of their block number, in block order
    std::vector<PMap> map(blocks.size());
    {
        std::vector<std::vector<std::vector<int>>> cls_members(c->nb, std::vector<std::vector<int>>(8));
        for (size_t b = 0; b < blocks.size(); ++b)
            if (blocks[b].first >= 0) cls_members[blocks[b].first][b % 8].push_back((int)b);
        for (size_t b = 0; b < blocks.size(); ++b) map[b] = PMap{-1, 0, 0, 0, 0, 0, (int)(b % 8), 0};
        P.g_max = 0; P.nsub_max = 0; P.ssz_max = 0;
        for (int k = 0; k < c->nb; ++k) {
            int sid = 0, soff = 0;
            for (int x = 0; x < 8; ++x) {
                const auto &mem = cls_members[k][x];
                if (mem.empty()) continue;
                for (size_t i = 0; i < mem.size(); ++i)
                    map[mem[i]] = PMap{k, blocks[mem[i]].second, (int)i, (int)mem.size(), sid, soff, (int)(mem[i] % 8), 0};
                soff += (int)mem.size();
                ++sid;
                P.ssz_max = std::max(P.ssz_max, (int)mem.size());
            }
            cones[k].nsub = sid;
            P.g_max = std::max(P.g_max, cones[k].G);
            P.nsub_max = std::max(P.nsub_max, sid);
        }
    }
    size_t words = 0;
    std::vector<size_t> offA(c->nb), offF(c->nb), offX(c->nb), offB(c->nb);
    for (int k = 0; k < c->nb; ++k) {
        const int G = cones[k].G;
        offA[k] = words; words += (size_t)2 * (G + (G + 63) / 64) * PK_SLOTW;
        offF[k] = words; words += (size_t)2 * G * PK_SLOTW;
        offX[k] = words; words += (size_t)2 * 8 * PK_SLOTW;
        offB[k] = words; words += (size_t)2 * 8 * PK_SLOTW;
    }
    if (P.mem.alloc(&P.gran, words) || P.mem.alloc(&P.team_out, (size_t)4 * c->nb) || P.mem.alloc(&P.arrive, 1) || P.mem.alloc(&P.abort_flag, 1) || P.mem.alloc(&P.stamps, 16)) return 1;
    if (c->opt.persist_carry && P.mem.alloc(&P.cx, c->all_elem)) return 1;
    P.cx_ok = false;
    P.gran_words = words;
    HC(hipMemset(P.gran, 0, sizeof(unsigned long long) * std::max<size_t>(words, 1)));
    HC(hipMemset(P.team_out, 0, sizeof(double) * 4 * (size_t)c->nb));
    HC(hipMemset(P.arrive, 0, sizeof(unsigned long long)));
    HC(hipMemset(P.abort_flag, 0, sizeof(int)));
    HC(hipMemset(P.stamps, 0, sizeof(unsigned long long) * 16));
    if (P.mem.alloc_pinned(&P.h_stamps, 16, hipHostMallocDefault)) return 1;
    for (int k = 0; k < c->nb; ++k) { cones[k].slA = P.gran + offA[k]; cones[k].slF = P.gran + offF[k]; cones[k].slX = P.gran + offX[k]; cones[k].slB = P.gran + offB[k]; }
    if (P.mem.upload(&P.d_cones, cones) || P.mem.upload(&P.d_map, map)) return 1;
    P.launches = 0;
    P.tag = 0;
    if (opt_verbose())
        fprintf(stderr, "lorads_hip: one-launch ADMM iteration: %d cone(s), %d workgroups (%s), %d row(s) per lane group, column steps %d, %zu bytes of LDS\n",
                c->nb, P.grid, P.xcd_map ? "every team on one XCD's blocks" : "dealt team by team", P.rows, P.ns, P.lds);
    return 0;
}

// is the one-launch form ready for this call (builds the plan on first use and after a rank change)
bool persist_ready(lorads_hip_ctx *c, int maxit) {
    if (!c->persist || !persist_eligible(c)) return false;
    if (maxit < 1 || 2ll * (2ll * maxit + maxit / 20 + 4) + 8 >= PK_TAGS_PER_LAUNCH) return false;
    PersistPlan &P = *c->persist;
    std::vector<int> sig;
    for (const auto &B : c->blk) { sig.push_back(B.n); sig.push_back(B.r); }
    if ((P.valid || P.failed) && sig != P.sig) { P.release(); P.failed = false; }
    if (P.failed) return false;
    if (!P.valid && persist_build(c)) { P.failed = true; return false; }
    return P.valid;
}

int run_sweep_persist(lorads_hip_ctx *c, double rho, double tol, int maxit, bool with_eval) {
    PersistPlan &P = *c->persist;
    // the dual update of the previous iteration rides on the U front (the rows store their constraints' new multipliers in place)
    const bool dual_on = c->pend.dual_owed_unused();
    const double rho_dual = dual_on ? c->pend.take_dual() : c->pend.dual_rho_value();
    c->pend.flush(c);
    flush_final(c);
    c->avg_folded = false;
    if (P.tag > 0xffffffffu - 4u * PK_TAGS_PER_LAUNCH) { // (tags about to wrap: start over on a clean slate)
        HC(hipMemsetAsync(P.gran, 0, sizeof(unsigned long long) * std::max<size_t>(P.gran_words, 1), c->stream));
        P.tag = 0;
    }
    const bool sep = c->ar && c->sep;
    const bool host_sum = sep && c->sx && with_eval;   // the ranks' hosts sum the four scalars after the hand-over
    const bool dev_sum = sep && with_eval && !host_sum; // ... or the all-reduce hook does, on the stream, before the hand-over
    PArgs A{};
    A.cones = P.d_cones; A.wg_map = P.d_map; A.ncones = c->nb;
    A.U = c->U; A.V = c->V; A.R = c->R; A.fbytes = (unsigned int)(c->all_elem * 8);
    A.csum = c->csum; A.b = c->b; A.lambda = c->lambda;
    A.rho = rho; A.tol = tol; A.rho_dual = rho_dual; A.maxit = maxit; A.dual_on = dual_on ? 1 : 0; A.with_eval = with_eval ? 1 : 0;
    A.st = c->st; A.tag0 = P.tag; A.team_out = P.team_out; A.arrive = P.arrive; A.arrive_target = (P.launches + 1) * (unsigned long long)c->nb;
    A.abort_flag = P.abort_flag;
    A.publish = dev_sum ? 0 : 1;
    A.loc_word = host_sum ? SX_WORD : -1;
    A.scal = c->scal; A.sepbuf = dev_sum ? c->sepbuf : nullptr;
    A.ctrl_src = (unsigned long long *)c->ctrl; A.ctrl_dst = (unsigned long long *)c->h_ctrl_dev; A.nwords = (int)state_words(c);
    A.flag = c->h_flag_dev; A.seq_dev = c->seq_dev;
    A.stamps = c->persist_stamps ? P.stamps : nullptr;
    A.allow_l2 = c->opt.persist_l2 ? 1 : 0;
    A.CX = P.cx; A.cv_in = (P.cx && P.cx_ok) ? 1 : 0; A.cv_out = (P.cx && with_eval) ? 1 : 0;
    P.cx_ok = false; // (V changes in this launch; true again below once the launch has left the new (C V) behind and has been seen to complete)
    P.tag += PK_TAGS_PER_LAUNCH;
    P.launches++;
    // Several PROCESSES on one card (the one-GPU rehearsals of the sharded path, never a deployment: one process per GPU): two such
    // launches side by side could each hold part of the compute units and wait for the rest for ever -- well, for PK_TIMEOUT_TICKS.
    // LORADS_SHARED_GPU=1: the launches of the processes on this card take turns (an advisory lock on a file named after the device
    // -- held for the launch alone, never across anything that waits for another rank)
    if (c->shared_gpu_fd >= 0) flock(c->shared_gpu_fd, LOCK_EX);
    // a profiling window (lorads_hip_profile, target 0) times this launch -- the whole iteration -- between two events
    const bool samp = c->prof && c->prof_target == 0 && c->prof_every < (1 << 20) && (c->n_persist % c->prof_every == 0) &&
                      c->ev_next + 2 <= c->ev_pool.size();
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (samp) { e0 = c->ev_pool[c->ev_next++]; e1 = c->ev_pool[c->ev_next++]; hipEventRecord(e0, c->stream); }
    ++c->n_launch;
    hipLaunchKernelGGL(pk_kernel(P.ns, P.rows), dim3(P.grid), dim3(TPB), P.lds, c->stream, A);
    if (samp) { hipEventRecord(e1, c->stream); c->timed_mv.push_back({e0, e1}); }
    if (c->shared_gpu_fd >= 0) {
        (void)hipStreamSynchronize(c->stream);
        flock(c->shared_gpu_fd, LOCK_UN);
    }
    c->merged.t_uv_valid = false; // (nothing the launch-by-launch form keeps between sweeps is kept here)
    for (auto &B : c->blk) { B.t_uv_valid = false; B.wj_for = nullptr; B.w0_ready = false; }
    if (dev_sum) {
        if (allreduce_dev(c, c->sepbuf, 4)) return 1;
        c->pend.post_sep(1, SepExtra{});
        if (enqueue_publish(c, 0, state_words(c))) return 1;
    } else {
        ++c->pub_seq;
        if (host_sum) { c->sx_pending = true; c->sx_with_obj = 1; }
    }
    if (wait_publish(c)) return 1;
    if (c->h_scal[7] != 0.0) {
        P.failed = true; // (not again in this context)
        return fail_msg("one-launch ADMM iteration: a team of workgroups did not complete (are other processes holding the GPU's compute units?); "
                        "LORADS_PERSIST=0 selects the launch-by-launch form");
    }
    // Sharded cones: a rank that runs its sweep launch by launch (cones of another kind) may have missed its speculation; then EVERY
    // rank evaluates once more so that all enter the second collective (run_sweep's protocol: the reduced scalars carry the count)
    if (with_eval && c->ar && c->h_scal[5] > 0.5) {
        if (enqueue_eval(c, LORADS_HIP_PAIR_UV, nullptr)) return 1;
        if (read_states(c)) return 1;
    }
    for (int stg = 0; stg < 2 * c->nb; ++stg) { // operator applications, for the counters of lorads_hip_profile_read
        const CGState &h = c->h_st[stg];
        c->n_matvec += 1 + (h.done == 2 ? 0 : h.iter + (h.iter > 1 ? (h.iter - 2) / 20 + 1 : 0));
    }
    c->n_sweeps++;
    c->n_persist++;
    P.cx_ok = A.cv_out != 0;
    return 0;
}

// V (or the objective's coefficients) is about to be written by somebody else than the one-launch iteration
inline void persist_touch(lorads_hip_ctx *c) { if (c->persist) c->persist->cx_ok = false; }
