// sweep.inc -- launch helpers, the CG operator, one speculative CG solve, the ADMM sweeps (cone by cone and lockstep), the
// evaluation and the result hand-over (included by lorads_hip.hip inside its anonymous namespace).
// ---- launch helpers
// (an empty grid -- a cone without constraints, an empty pattern -- is simply nothing to do, not a refused launch)
// Scalar steps waiting for a carrier kernel (class Pending): whoever can carry them takes them BEFORE its LAUNCH; any other
// launch first sends them off as the one-workgroup kernels they replace.
#define LAUNCH_LDS(kern, grid, lds, ...)                                                             \
    do {                                                                                             \
        const int grid__ = (int)(grid);                                                              \
        if (c->pend.must_flush()) c->pend.flush(c);                                                  \
        if (grid__ > 0) { ++c->n_launch; hipLaunchKernelGGL(kern, dim3(grid__), dim3(TPB), (size_t)(lds), c->stream, __VA_ARGS__); } \
    } while (0)
#define LAUNCH(kern, grid, ...) LAUNCH_LDS(kern, grid, 0, __VA_ARGS__)
#include "pending.inc"

// (LG, V2, NS) for a rank: 8 lanes x 16-byte loads when r is even and <= 128, else 8/32/64 lanes x 8-byte loads
struct Shape {
    int lg, v2, ns;
};
inline Shape shape_for(int r) {
    Shape s;
    s.v2 = use_v2(r);
    s.lg = lg_for(r);
    const int w = s.v2 ? 2 : 1;
    s.ns = (r + s.lg * w - 1) / (s.lg * w);
    return s;
}
#define NS_SWITCH(LGV, V2V, ns, ...)                                     \
    switch (ns) {                                                        \
    case 1: { constexpr int LG_ = LGV; constexpr bool V2_ = V2V; constexpr int NS_ = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int LG_ = LGV; constexpr bool V2_ = V2V; constexpr int NS_ = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int LG_ = LGV; constexpr bool V2_ = V2V; constexpr int NS_ = 3; __VA_ARGS__; } break; \
    case 4: { constexpr int LG_ = LGV; constexpr bool V2_ = V2V; constexpr int NS_ = 4; __VA_ARGS__; } break; \
    case 5: { constexpr int LG_ = LGV; constexpr bool V2_ = V2V; constexpr int NS_ = 5; __VA_ARGS__; } break; \
    case 6: { constexpr int LG_ = LGV; constexpr bool V2_ = V2V; constexpr int NS_ = 6; __VA_ARGS__; } break; \
    case 7: { constexpr int LG_ = LGV; constexpr bool V2_ = V2V; constexpr int NS_ = 7; __VA_ARGS__; } break; \
    default: { constexpr int LG_ = LGV; constexpr bool V2_ = V2V; constexpr int NS_ = 8; __VA_ARGS__; } break; \
    }
#define SHAPE_DISPATCH(sh, ...)                                   \
    do {                                                          \
        if ((sh).v2) { NS_SWITCH(8, true, (sh).ns, __VA_ARGS__) }        \
        else if ((sh).lg == 8) { NS_SWITCH(8, false, (sh).ns, __VA_ARGS__) } \
        else if ((sh).lg == 32) { NS_SWITCH(32, false, (sh).ns, __VA_ARGS__) } \
        else { NS_SWITCH(64, false, (sh).ns, __VA_ARGS__) }              \
    } while (0)

void pairdots(lorads_hip_ctx *c, const Pattern &P, const double *X, const double *Y, int r, double *T, Guard g) {
    if (P.ne == 0) return;
    const Shape sh = shape_for(r);
    const int grid = nblocks_for((size_t)P.ne, TPB / sh.lg);
    SHAPE_DISPATCH(sh, LAUNCH((k_pairdots<LG_, V2_, NS_>), grid, P.ne, P.erow, P.ecol, X, Y, r, T, g));
}
// returns the number of partials written
int spmm(lorads_hip_ctx *c, const Block &B, const Pattern &P, const double *X, int mode, const double *xin, const double *rhs,
         double rho, double *out, double *part, Guard g, const double *dense_add = nullptr) {
    const Shape sh = shape_for(B.r);
    const int grid = nblocks_for((size_t)B.n, TPB / sh.lg);
    SHAPE_DISPATCH(sh, LAUNCH((k_spmm2<LG_, V2_, NS_, false>), grid, B.n, P.adj_ptr, P.adj_col, P.adj_dyn, P.adj_sval, P.S, (const double *)nullptr, X,
                              B.r, mode, xin, rhs, ds_rho(c, rho), out, (double *)nullptr, part, (double *)nullptr, g, dense_add));
    return grid;
}
// the front of a CG solve in one pass (k_spmm2<FRONT>): rhs_out = X - (S X)/rho, out = rhs_out - (xin + S2 X);
// part <- partials of ||out||^2, part_b <- partials of ||rhs_out||_1; returns their number
struct DiagOnFly { // Max-Cut-type cone: the front forms its changing coefficients itself (no k_sval before it), see k_spmm2
    bool on = false;
    WArgs wa{};
    int wmode = 0;
    CGState *reset = nullptr;
    int nreset = 0;
    Deferred d{};
};
int spmm_front(lorads_hip_ctx *c, const Block &B, const Pattern &P, const double *X, const double *xin, double rho, double *rhs_out,
               double *out, double *part, double *part_b, Guard g, const DiagOnFly &of = DiagOnFly{}) {
    const Shape sh = shape_for(B.r);
    const int grid = nblocks_for((size_t)B.n, TPB / sh.lg);
    if (of.on) {
        SHAPE_DISPATCH(sh, LAUNCH((k_spmm2<LG_, V2_, NS_, true>), grid, B.n, P.adj_ptr, P.adj_col, P.adj_dyn, P.adj_sval, P.S,
                                  (const double *)nullptr, X, B.r, 0, xin, (const double *)nullptr, ds_rho(c, rho), out, rhs_out, part, part_b, g,
                                  (const double *)nullptr, (const double *)B.gdiag, B.w_uv, (const int *)B.rc_con, B.rc_w,
                                  (const double *)B.diag_a, of.wa, of.wmode, of.reset, of.nreset, of.d));
        return grid;
    }
    SHAPE_DISPATCH(sh, LAUNCH((k_spmm2<LG_, V2_, NS_, true>), grid, B.n, P.adj_ptr, P.adj_col, P.adj_dyn, P.adj_sval, P.S,
                              (const double *)(B.diag_only ? nullptr : P.S2), X, B.r, 0, xin, (const double *)nullptr, ds_rho(c, rho), out, rhs_out,
                              part, part_b, g, (const double *)nullptr, (const double *)(B.diag_only ? B.gdiag : nullptr),
                              B.diag_only ? B.w_uv : (double *)nullptr));
    return grid;
}
// rows per workgroup and grid of k_front_cw and of k_spmm_ell at 8 lanes per row on cone B: fixed for the context's life (see
// row_deal and Options::row_deal).  The merged lockstep cone keeps 32 rows; so does a forced deal whose grid would not
// fit a partial-sum slot.
RowDeal row_deal_of(const lorads_hip_ctx *c, const Block &B) {
    const size_t n = (size_t)std::max(B.n, 0);
    if (c->opt.row_deal == 0 || &B == &c->merged) return RowDeal{32, nblocks_for(n, 32)};
    if (c->opt.row_deal > 0) {
        const int rpw = nblocks_for(n, c->opt.row_deal) <= c->maxpart ? c->opt.row_deal : 32;
        return RowDeal{rpw, nblocks_for(n, rpw)};
    }
    return row_deal(n, c->row_deal_cus);
}
// epilogue(x + sum over (neighbour, constraint) slots of a w_i V_q): the operator's SpMM with the coefficients formed
// from the constraint weights w
// cg0 != null: CG iteration 0's update folded in (the CG0 form of k_spmm_ell: 16-byte rows, mode OP_CG, out unused, `part`
// receives the partials of the new residual's norm)
int spmm_cw(lorads_hip_ctx *c, const Block &B, const double *w, const double *X, int mode, const double *xin, const double *rhs,
            double *out, double *part, Guard g, const Cg0Args *cg0 = nullptr) {
    const Shape sh = shape_for(B.r);
    const int grid = nblocks_for((size_t)B.n, TPB / sh.lg);
    // k_spmm_ell: rows per workgroup and grid together -- at 8 lanes per row the rows dealt over the compute units, else TPB / lg rows
    const RowDeal rd = sh.lg == 8 ? row_deal_of(c, B) : RowDeal{TPB / sh.lg, grid};
    if (cg0) {
        if (!B.cell_w || !sh.v2 || mode != OP_CG) { c->launch_err = "CG iteration 0 in the operator: no kernel form for this cone"; return 0; }
        if (B.cell_w == 8) {
            NS_SWITCH(8, true, sh.ns, LAUNCH((k_spmm_ell<LG_, V2_, NS_, 8, true>), rd.grid, B.n, rd.rpw, B.cadj_ptr, B.cadj_col, B.cadj_con, B.cadj_a,
                                             B.cell_col, B.cell_con, B.cell_a, w, X, B.r, mode, xin, rhs, (double *)nullptr, part, g, *cg0))
        } else {
            NS_SWITCH(8, true, sh.ns, LAUNCH((k_spmm_ell<LG_, V2_, NS_, 16, true>), rd.grid, B.n, rd.rpw, B.cadj_ptr, B.cadj_col, B.cadj_con, B.cadj_a,
                                             B.cell_col, B.cell_con, B.cell_a, w, X, B.r, mode, xin, rhs, (double *)nullptr, part, g, *cg0))
        }
        return rd.grid;
    }
    if (B.cell_w && (mode == OP_CG || mode == OP_RES)) {
        Cg0Args wo{}; // (the plain form reads its store mask from here and nothing else)
        wo.wt = c->opt.wt_stores;
        if (B.cell_w == 8)
            SHAPE_DISPATCH(sh, LAUNCH((k_spmm_ell<LG_, V2_, NS_, 8>), rd.grid, B.n, rd.rpw, B.cadj_ptr, B.cadj_col, B.cadj_con, B.cadj_a, B.cell_col,
                                      B.cell_con, B.cell_a, w, X, B.r, mode, xin, rhs, out, part, g, wo));
        else
            SHAPE_DISPATCH(sh, LAUNCH((k_spmm_ell<LG_, V2_, NS_, 16>), rd.grid, B.n, rd.rpw, B.cadj_ptr, B.cadj_col, B.cadj_con, B.cadj_a, B.cell_col,
                                      B.cell_con, B.cell_a, w, X, B.r, mode, xin, rhs, out, part, g, wo));
        return rd.grid;
    }
    SHAPE_DISPATCH(sh, LAUNCH((k_spmm<LG_, V2_, NS_, true>), grid, B.n, B.cadj_ptr, B.cadj_col, B.cadj_con, w, X, B.r, mode, xin, rhs,
                              0.0, out, part, g, (const double *)nullptr, B.cadj_a));
    return grid;
}
bool cw_quad(lorads_hip_ctx *c, const Block &B) {
    return c->opt.cw_quad && use_v2(B.r) && B.r <= 48 && B.ca_ell > 8 && B.ca_ell <= 16;
}
// w_i = A_i(sym(X Y^T)) for every constraint of the cone + k_cv's bookkeeping, without the pair-dot array
int cw(lorads_hip_ctx *c, const Block &B, const double *X, const double *Y, double scale, double *w_out, double *cv, int mode,
       double *vec, Guard g, ResArgs ra = ResArgs{}) {
    if (B.nrow == 0) return 0;
    const Shape sh = shape_for(B.r);
    const int grid = nblocks_for((size_t)B.nrow, TPB / 64);
    // a waiting start rides on this kernel if it is the solve's own first, a waiting test if this kernel waits for its solve
    const InitArgs ia = c->pend.take_init_on(g);
    const Deferred d = c->pend.take_check_behind(g);
    if (cw_quad(c, B)) { // 4 lanes per entry: a whole fixed-width constraint of 9..16 entries in one trip
        const int ns4 = (B.r + 7) / 8;
        NS_SWITCH(4, true, ns4, LAUNCH((k_cw<LG_, V2_, NS_, true>), grid, B.nrow, B.a_ptr, B.ca_row, B.ca_val, B.ca_col, X, Y, B.r,
                                       scale, w_out, cv, mode, B.row_idx, vec, g, B.ca_ell, ia, ra, d));
        return grid;
    }
    SHAPE_DISPATCH(sh, LAUNCH((k_cw<LG_, V2_, NS_>), grid, B.nrow, B.a_ptr, B.ca_row, B.ca_val, B.ca_col, X, Y, B.r, scale,
                              w_out, cv, mode, B.row_idx, vec, g, B.ca_ell, ia, ra, d));
    return grid;
}
// the tiles of one k_dense_cx_b launch that starts at column col0 of a rank-r factor: up to 8 column tiles of 16 on the matrix cores;
// a last tile that would hold 1..4 columns is not given to them: those columns run on plain FMAs (REM)
struct DenseTiles { int nt, rem; };
static inline DenseTiles dense_tiles(int r, int col0, bool use_rem) {
    const int cols = std::min(r - col0, 128);
    DenseTiles t{(cols + 15) / 16, 0};
    if (cols % 16 >= 1 && cols % 16 <= 4 && t.nt >= 2 && use_rem) { t.rem = cols % 16; t.nt -= 1; }
    return t;
}
// W = C X on the matrix cores (dense objective only)
int dense_cx(lorads_hip_ctx *c, const Block &B, const double *X, double *W, Guard g, const double *M = nullptr) {
    c->pend.flush(c);
    if (!M) M = B.Cfull; // (the dense objective; else: a dense constraint matrix or a combination of them)
    if (B.ksplit_b <= 0) return 1; // (n_pad is a multiple of 64: never)
    { // C as the MFMA B operand, K split inside the workgroup (see k_dense_cx_b)
        const int gx = B.npad / 32, ks = B.ksplit_b, krange = B.npad / ks;
        double *dst = ks == 1 ? W : B.Wpart;
        for (int col0 = 0; col0 < B.r; col0 += 128) { // (up to 8 column tiles of 16 per launch)
            const DenseTiles tl = dense_tiles(B.r, col0, c->opt.dense_rem);
            const int nt = tl.nt, rem = tl.rem;
#define DCXB(NTV, RV) hipLaunchKernelGGL((k_dense_cx_b<NTV, 4, RV>), dim3(gx, ks), dim3(TPB), 0, c->stream, B.n, B.npad, krange, M, X, B.r, dst, g, col0)
#define DCXR(NTV)                                  \
    switch (rem) {                                 \
    case 1: DCXB(NTV, 1); break;                   \
    case 2: DCXB(NTV, 2); break;                   \
    case 3: DCXB(NTV, 3); break;                   \
    case 4: DCXB(NTV, 4); break;                   \
    default: DCXB(NTV, 0); break;                  \
    }
            switch (nt) {
            case 1: DCXR(1); break;
            case 2: DCXR(2); break;
            case 3: DCXR(3); break;
            case 4: DCXR(4); break;
            case 5: DCXR(5); break;
            case 6: DCXR(6); break;
            case 7: DCXR(7); break;
            default: DCXR(8); break;
            }
#undef DCXR
#undef DCXB
        }
        if (ks > 1) {
            const size_t len = (size_t)B.n * B.r;
            LAUNCH(k_sum_slabs, grid1d(len), len, ks, B.Wpart, W, g);
        }
        return 0;
    }
}
// ---- dense constraint matrices (Block::dense_a)
// their constraint values <A_j, sym(X Y^T)> = <X, A_j Y>: one GEMM + one dot per dense constraint, added to what the sparse pass
// (which saw these constraints empty) has left in cv / vec
// W_j = A_j Y for every dense constraint (and C Y for a dense objective), kept while Y -- the fixed factor of a CG solve -- stands
void dense_cache_fill(lorads_hip_ctx *c, Block &B, const double *Y, Guard g) {
    if (!B.dense_a || !B.Wj || !c->opt.dense_cache) return;
    const size_t len = (size_t)B.n * B.r, msz = (size_t)B.npad * B.npad;
    for (int j = 0; j < B.nd; ++j)
        if (dense_cx(c, B, Y, B.Wj + (size_t)j * len, g, B.Adense + (size_t)j * msz)) { c->launch_err = "dense GEMM: no kernel form for this rank"; return; }
    if (B.dense_c && dense_cx(c, B, Y, B.Wc, g, B.Cfull)) { c->launch_err = "dense GEMM: no kernel form for this rank"; return; }
    B.wj_for = Y;
}
void dense_constr_fix(lorads_hip_ctx *c, const Block &B, const double *X, const double *Y, double scale, double *cv, double *vec, Guard g) {
    if (!B.dense_a) return;
    if (B.wj_for && (B.wj_for == Y || B.wj_for == X)) { // <A_j, sym(X Y^T)> = <X, A_j Y> = <Y, A_j X>: one dot per constraint, one launch
        const size_t len = (size_t)B.n * B.r;
        LAUNCH(k_dense_dots_fix, B.nd, len, B.wj_for == Y ? X : Y, (const double *)B.Wj, (const int *)B.d_con, scale, cv, (const int *)B.row_idx, vec, g);
        return;
    }
    const size_t len = (size_t)B.n * B.r, msz = (size_t)B.npad * B.npad;
    const std::vector<int> &dcon = B.d_con_h;
    for (int j = 0; j < B.nd; ++j) {
        if (dense_cx(c, B, Y, B.Wd, g, B.Adense + (size_t)j * msz)) c->launch_err = "dense GEMM: no kernel form for this rank";
        const int gd = grid1d(len);
        LAUNCH(k_dot, gd, len, X, (const double *)B.Wd, part_slot(c, 17), g);
        LAUNCH(k_dense_cv_fix, 1, (const double *)part_slot(c, 17), gd, dcon[(size_t)j], scale, cv, (const int *)B.row_idx, vec, g);
    }
}
// B.Wd = ([C] + sum_j mu_j A_j) X with mu_j = sign * weight of dense constraint j under (`wmode`, wa): the dense part of every
// (C + sum_i mu_i A_i) X product of such a cone (its sparse part runs over the union pattern as ever)
void dense_part(lorads_hip_ctx *c, const Block &B, const double *X, int wmode, const WArgs &wa, double sign, bool with_c, Guard g) {
    const double *M = B.Cfull;
    if (B.dense_a && B.wj_for == X) { // the products are there: a combination of n x r arrays instead of matrices and a GEMM
        const size_t len = (size_t)B.n * B.r;
        LAUNCH(k_dense_mu, nblocks_for((size_t)B.nd, TPB), B.nd, (const int *)B.d_con, wmode, wa, sign, B.d_mu, g);
        LAUNCH(k_dense_lincomb, grid1d(len), len, B.nd, (const double *)B.Wj, (const double *)B.d_mu,
               (const double *)((with_c && B.dense_c) ? B.Wc : nullptr), B.Wd, g);
        return;
    }
    if (B.dense_a) {
        const size_t msz = (size_t)B.npad * B.npad;
        LAUNCH(k_dense_mu, nblocks_for((size_t)B.nd, TPB), B.nd, (const int *)B.d_con, wmode, wa, sign, B.d_mu, g);
        LAUNCH(k_dense_combine, grid1d(msz), msz, B.nd, (const double *)B.Adense, (const double *)B.d_mu,
               (const double *)((with_c && B.dense_c) ? B.Cfull : nullptr), B.Sfull, g);
        M = B.Sfull;
    }
    if (dense_cx(c, B, X, B.Wd, g, M)) c->launch_err = "dense GEMM: no kernel form for this rank";
}

int op_diag(lorads_hip_ctx *c, const Block &B, const double *V, int mode, const double *xin, const double *rhs, double *out,
            double *part, Guard g, double *dot_out = nullptr) {
    const Shape sh = shape_for(B.r);
    const int grid = nblocks_for((size_t)B.n, TPB / sh.lg);
    // a waiting solve start rides on the solve's first operator application, a waiting convergence test on the
    // residual of the k = 0 restart (both carry the solve's own gate)
    Carry cy{};
    cy.ia = c->pend.take_init_on(g);
    if (!cy.ia.st) cy.d = c->pend.take_check_on(g);
    // a waiting direction update whose output is this application's input is formed here, row by row (see take_on_op_diag)
    const DirArgs da = c->pend.take_on_op_diag(c, mode, xin, g, TPB / sh.lg);
    SHAPE_DISPATCH(sh, LAUNCH((k_op_diag<LG_, V2_, NS_>), grid, B.n, B.gdiag, V, B.r, mode, xin, rhs, out, part, g, cy, da, dot_out));
    return grid;
}
int op_entry(lorads_hip_ctx *c, const Block &B, const double *V, int mode, const double *xin, const double *rhs, double *out,
             double *part, Guard g) {
    const Shape sh = shape_for(B.r);
    if (B.bip_rows[0] && c->opt.entry_bip) { // bipartite entry graph: 3 gathered rows per entry instead of 4 (see k_op_entry_bip)
        const int g0 = nblocks_for((size_t)B.bip_n[0], TPB / sh.lg), g1 = nblocks_for((size_t)B.bip_n[1], TPB / sh.lg);
        if (g0 + g1 <= c->maxpart) {
            SHAPE_DISPATCH(sh, LAUNCH((k_op_entry_bip<LG_, V2_, NS_, 0>), g0, B.bip_n[0], (const int *)B.bip_rows[0], B.pa.adj_ptr, B.pa.adj_col,
                                      B.pa.adj_e, B.gentry, B.bip_we, V, B.r, mode, xin, rhs, out, part, 0, g));
            SHAPE_DISPATCH(sh, LAUNCH((k_op_entry_bip<LG_, V2_, NS_, 1>), g1, B.bip_n[1], (const int *)B.bip_rows[1], B.pa.adj_ptr, B.pa.adj_col,
                                      B.pa.adj_e, B.gentry, B.bip_we, V, B.r, mode, xin, rhs, out, part, g0, g));
            return g0 + g1;
        }
    }
    const int grid = nblocks_for((size_t)B.n, TPB / sh.lg);
    // (a variant that reads the neighbour list eight slots at a time and keeps four neighbours' row pairs in flight ran
    // at the same 83 us at r = 44 and 8 % slower at r = 60: the kernel moves 0.3-0.45 GB of short random rows per launch
    // out of the Infinity Cache at 3.9-4.3 TB/s whatever the issue order -- ubench variant 100)
    // (nor does the order of the rows matter: rows by descending neighbour count -- equal trips for the eight rows of a
    // wavefront -- ran at the same 83 / 108 us, and made the solve front 1 us slower)
    SHAPE_DISPATCH(sh, LAUNCH((k_op_entry<LG_, V2_, NS_>), grid, B.n, B.pa.adj_ptr, B.pa.adj_col, B.pa.adj_e, B.gentry, V, B.r, mode, xin,
                              rhs, out, part, g));
    return grid;
}
int obj_partials(lorads_hip_ctx *c, const Block &B, const double *X, const double *Y, double *part, Guard g,
                 double *stage_tail = nullptr) {
    if (B.nc == 0) return 0;
    if (B.dense_c) { // <C, sym(X Y^T)> = sum_p X_p . (C Y)_p for symmetric C
        if (dense_cx(c, B, Y, B.Wd, g)) c->launch_err = "dense GEMM: no kernel form for this rank";
        const size_t len = (size_t)B.n * B.r;
        const int grid = grid1d(len);
        LAUNCH(k_dot, grid, len, X, B.Wd, part, g);
        return grid;
    }
    const Shape sh = shape_for(B.r);
    // (2048 workgroups: 7.0 us against 8.4 with 1024 and 7.7 with 4096 at the headline, ubench 10/13/14.  Partials that travel
    // through the all-reduce: always 2048 of them -- the collective has the same length on every rank, whatever its cone's size)
    const int grid = stage_tail ? 2048 : std::min(nblocks_for((size_t)B.nc, TPB / sh.lg), 2048);
    SHAPE_DISPATCH(sh, LAUNCH((k_obj<LG_, V2_, NS_>), grid, B.nc, B.c_row, B.c_col, B.c_val, X, Y, B.r, part, g, stage_tail));
    return grid;
}

// cv = A_k(sym(X Y^T))   (LORADSInitConstrVal, lorads_alg_common.c:71-76) and, per `mode`, the running m-vector
// T(U,V) is kept in B.T (and reused by the next solve's initial residual, whose pair dots are the same
// numbers); every other pair goes through B.T2
void constr_val(lorads_hip_ctx *c, Block &B, const double *X, const double *Y, double scale, double *cv, int mode, double *vec,
                Guard g) {
    if (B.nrow == 0) return;
    const bool uv = (X == c->U + B.off && Y == c->V + B.off);
    if (B.use_cw) { // one kernel, no pair-dot array; for (U, V) the values are kept as the operator's weights
        cw(c, B, X, Y, scale, uv ? B.w_uv : (double *)nullptr, cv, mode, vec, g);
        if (uv) B.t_uv_valid = true;
        return;
    }
    double *T = uv ? B.T : B.T2;
    pairdots(c, B.pa, X, Y, B.r, T, g);
    if (uv) B.t_uv_valid = true;
    LAUNCH(k_cv, nblocks_for((size_t)B.nrow, TPB / 8), B.nrow, B.a_ptr, B.a_e, B.a_val, T, scale, cv, mode, B.row_idx, vec, g);
    dense_constr_fix(c, B, X, Y, scale, cv, vec, g); // (dense constraint matrices: their values join the sparse pass's)
}
void sval(lorads_hip_ctx *c, const Pattern &P, bool with_c, int mode, const WArgs &wa, Guard g, CGState *reset = nullptr,
          int nreset = 0, const double *w2 = nullptr, const int *econ = nullptr) {
    if (P.ne == 0 && !reset) return;
    // a waiting convergence test whose gate is this kernel's gate rides on it (the V-solve's front after a virtual refresh)
    const Deferred d = c->pend.take_check_behind(g);
    LAUNCH(k_sval, std::max(1, nblocks_for((size_t)P.ne, TPB)), P.ne, P.e_ptr, econ ? econ : P.e_con, P.e_val,
           with_c ? P.cbase : nullptr, mode, wa, P.S, g, reset, nreset, w2, w2 ? P.S2 : (double *)nullptr, d);
}

// the constraint weights of iteration 0's operator application from the contributions k_front_cw has left (see there)
// (part_ww != null: also the partials of ||w||^2, one per workgroup, see Cg0Args)
int wsum(lorads_hip_ctx *c, Block &B, Guard g, double *part_ww = nullptr) {
    const InitArgs ia = c->pend.take_init_on(g);
    double rho_dual = 0.0;
    const int dual_on = c->pend.take_dual_used(&rho_dual) ? 1 : 0; // this kernel stores the multipliers
    const int grid = nblocks_for((size_t)B.nrow, TPB / 8);
    // (behind an adopted front: the sweep's reset words, see spec_front_adopt)
    CGState *reset = c->spec.reset;
    const int nreset = c->spec.nreset;
    c->spec.reset = nullptr; c->spec.nreset = 0;
    LAUNCH(k_wsum, grid, B.nrow, B.cs_w, (const double *)B.w_contrib, B.w_op, g, ia, dual_on, ds_rho_dual(c, rho_dual), c->m, (const double *)c->b,
           (const double *)c->csum, c->lambda, part_ww, reset, nreset);
    return grid;
}

// one application of the CG operator  out = epilogue(x + (sum_i <A_i, sym(x V^T)> A_i) V)
// (linSysProduct, lorads_admm.c:376-391); returns #partials in `part`
// (iteration 0 of a cone on the one-kernel-front path, see solve_iter_body: part_ww receives k_wsum's partials of ||w||^2,
// cg0 != null folds the iteration's update into the operator kernel)
int apply_operator(lorads_hip_ctx *c, Block &B, const double *V, const double *x, int mode, const double *rhs, double *out,
                   double *part, Guard g, double *part_ww = nullptr, const Cg0Args *cg0 = nullptr) {
    // (prof_every >= 2^20: count applications, time none -- such a window is replayed like any other, see graph_ok)
    // A timed application runs exactly what an untimed one runs (iteration 0 of a k_cw cone: k_wsum + k_spmm_ell with the solve's
    // start on board; a fused direction update stays fused): the events bracket the launches, they do not change them.
    const bool samp = c->prof && c->prof_target == 0 && c->prof_every < (1 << 20) && (c->n_matvec % c->prof_every == 0) &&
                      c->ev_next + 3 <= c->ev_pool.size();
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    if (samp) {
        e0 = c->ev_pool[c->ev_next++]; e1 = c->ev_pool[c->ev_next++];
        hipEventRecord(e0, c->stream);
    }
    int grid;
    if (B.diag_only) {
        // the row dots x_p . V_p ride along: for a CG direction into w_op, for the solve variable (exact) into w_uv
        const bool is_uv = (x == c->U + B.off && V == c->V + B.off) || (x == c->V + B.off && V == c->U + B.off);
        double *dots = !B.w_op ? (double *)nullptr : (mode == OP_CG && !is_uv) ? B.w_op : (mode == OP_RES && is_uv) ? B.w_uv : (double *)nullptr;
        grid = op_diag(c, B, V, mode, x, rhs, out, part, g, dots);
        if (dots && dots == B.w_uv) B.t_uv_valid = true; // (under the caveat of solve_iter_tail: the kernel is gated)
    } else if (B.entry_only) {
        grid = op_entry(c, B, V, mode, x, rhs, out, part, g);
    } else if (B.use_cw) {
        // x and V are this cone's (U,V) in either order and B.w_uv already holds A(sym(U V^T))
        const bool is_uv = (x == c->U + B.off && V == c->V + B.off) || (x == c->V + B.off && V == c->U + B.off);
        const double *w = B.w_uv;
        if (B.w0_ready && mode == OP_CG && x == c->cr + B.off) {
            // iteration 0 (p_0 = r_0) right behind k_front_cw: the constraint values of (r_0, V) are the sums of the
            // contributions the front has left -- no gather pass
            wsum(c, B, g, part_ww);
            w = B.w_op;
            B.t_uv_valid = false;
        } else if (!(is_uv && B.t_uv_valid)) {
            cw(c, B, x, V, 1.0, is_uv ? B.w_uv : B.w_op, (double *)nullptr, (int)CV_SET, (double *)nullptr, g);
            w = is_uv ? B.w_uv : B.w_op;
            B.t_uv_valid = is_uv;
        }
        B.w0_ready = false;
        // (no event between the two kernels of an application: a marker there would keep them from running back to back,
        // which is how they run when nobody is watching)
        grid = spmm_cw(c, B, w, V, mode, x, rhs, out, part, g, cg0);
    } else {
        // x and V are this cone's (U,V) in either order and B.T already holds their pair dots
        const bool is_uv = (x == c->U + B.off && V == c->V + B.off) || (x == c->V + B.off && V == c->U + B.off);
        if (!(is_uv && B.t_uv_valid)) {
            pairdots(c, B.pa, x, V, B.r, B.T, g);
            B.t_uv_valid = is_uv;
        }
        if (B.has_gram) {
            LAUNCH(k_sgram, nblocks_for((size_t)B.pa.ne, TPB / 8), B.pa.ne, B.g_ptr, B.g_col, B.g_val, B.T, B.pa.S, g);
        } else {
            LAUNCH(k_cv, nblocks_for((size_t)B.nrow, TPB / 8), B.nrow, B.a_ptr, B.a_e, B.a_val, B.T, 1.0, B.wtmp, (int)CV_SET,
                   B.row_idx, (double *)nullptr, g);
            dense_constr_fix(c, B, x, V, 1.0, B.wtmp, (double *)nullptr, g); // w_i = <x, A_i V> of the dense constraints
            WArgs wa{};
            wa.w = B.wtmp;
            sval(c, B.pa, false, W_COMPACT, wa, g);
            if (B.dense_a) dense_part(c, B, V, W_COMPACT, wa, 1.0, false, g); // (sum over the dense constraints of w_i A_i) V -> B.Wd
        }
        if (samp) { e2 = c->ev_pool[c->ev_next++]; hipEventRecord(e2, c->stream); }
        grid = spmm(c, B, B.pa, V, mode, x, rhs, 0.0, out, part, g, B.dense_a ? B.Wd : (const double *)nullptr);
    }
    if (samp) {
        hipEventRecord(e1, c->stream);
        c->timed_mv.push_back({e0, e1});
        if (e2) c->timed_sp.push_back({e2, e1});
    }
    c->n_matvec++;
    return grid;
}

void drain_events(lorads_hip_ctx *c) {
    for (auto &pr : c->timed_mv) {
        float ms = 0;
        hipEventSynchronize(pr.second);
        hipEventElapsedTime(&ms, pr.first, pr.second);
        c->ms_samp += ms; c->n_samp++;
        c->samp_ms.push_back(ms);
    }
    for (auto &pr : c->timed_sp) {
        float ms = 0;
        hipEventElapsedTime(&ms, pr.first, pr.second);
        c->ms_samp_spmm += ms; c->n_samp_spmm++;
    }
    c->timed_mv.clear();
    c->timed_sp.clear();
    c->ev_next = 0;
}

// Constraint values of (U, V) by recurrence.  Inside a CG solve on x (V fixed) every update x += alpha p moves
// A(sym(x V^T)) by alpha A(sym(p V^T)), and A(sym(p V^T)) is exactly what the operator has just computed for that p
// (k_cw's output w_op).  So the constraint refresh after a solve (LORADSInitConstrVal, lorads_alg_common.c:199-203: a full
// gather pass over the factors in the reference and in k_cw) needs no pass at all: k_cg_update keeps w_uv current, and
// the refresh is the m-vector bookkeeping alone (k_refresh_w).  Same numbers up to rounding (the reference's own CG
// carries its residual the same way, r -= alpha Q); every 32nd sweep recomputes w_uv from the factors so that rounding
// cannot pile up over a long run.  LORADS_EXACT_REFRESH=1 switches the recurrence off (tests compare the two).
// Max-Cut-type cones do the same with row dots: w_uv[p] = U_p . V_p (left exact by every front and every residual on the
// solve variable), w_op[p] = p_p . V_p from k_op_diag, and constraint i = a_i e_p e_p^T has the value a_i w_uv[p].
bool constr_by_recurrence(lorads_hip_ctx *c, const Block &B) {
    return (B.use_cw || (B.diag_only && B.w_uv && B.w_op && B.diag_row)) && !c->opt.exact_refresh && &B != &c->merged;
}

// k_cw cones and Max-Cut-type cones with a sparse objective build the right-hand side and the initial residual of a solve in one kernel
// (LORADS_SPLIT_FRONT=1: the two separate passes, for tests and comparisons)
bool fused_front(lorads_hip_ctx *c, const Block &B) {
    return ((B.use_cw && B.pu.S2) || B.diag_only) && !B.dense_c && !B.dense_a && !c->opt.split_front && B.pu.ne > 0;
}

// cones on the k_cw path with 16-byte row accesses take the one-kernel front (LORADS_FRONT_CW=0: k_sval + k_spmm2<FRONT>)
bool front_cw_ok(lorads_hip_ctx *c, const Block &B) {
    return c->opt.front_cw && B.front_cw && fused_front(c, B) && B.use_cw && B.cell_w && use_v2(B.r) && &B != &c->merged;
}

// profiling target 1: the front of a solve (its main kernel) between two events, one front in `prof_every`
struct FrontSample {
    lorads_hip_ctx *c;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit FrontSample(lorads_hip_ctx *c_) : c(c_) {
        const bool samp = c->prof && c->prof_target == 1 && c->prof_every < (1 << 20) && (c->n_front % c->prof_every == 0) &&
                          c->ev_next + 2 <= c->ev_pool.size();
        c->n_front++;
        if (samp) { e0 = c->ev_pool[c->ev_next++]; e1 = c->ev_pool[c->ev_next++]; hipEventRecord(e0, c->stream); }
    }
    void done() { if (e0) { hipEventRecord(e1, c->stream); c->timed_mv.push_back({e0, e1}); } }
};

// ---- one CG solve, split so that it can be enqueued speculatively and resumed
struct Solve {
    Block *B;
    double *x;
    const double *V;
    CGState *st;
    Guard front;   // gate of everything before the iterations ({nullptr, need = previous solve done})
    size_t len;
    int gv;
    int tile = 0, tile_w = 0; // k_cg_update on the operator's own row tiles (see there)
};

// the one-kernel front (k_front_cw): its argument pack for weights of mode `wmode` at `rho`, no dual update on board ...
FrontCwArgs front_cw_args(lorads_hip_ctx *c, const Block &B, double rho, int wmode) {
    FrontCwArgs A{};
    A.fc_ptr = B.fc_ptr; A.fc_col = B.fc_col; A.fc_val = B.fc_val; A.sl_ptr = B.cadj_ptr; A.sl_col = B.cadj_col; A.sl_con = B.cadj_con;
    A.sl_a = B.cadj_a; A.ell_col = B.cell_col; A.ell_con = B.cell_con; A.ell_a = B.cell_a; A.ell_dst = B.cell_dst; A.sl_dst = B.cadj_dst; A.csum = c->csum; A.b = c->b;
    A.lambda = c->lambda; A.cv = B.cv; A.w_uv = B.w_uv; A.row_idx = B.row_idx_identity ? nullptr : B.row_idx; A.rho = ds_rho(c, rho);
    A.wmode = wmode;
    A.contrib = B.w_contrib;
    A.wt = c->opt.wt_stores;
    return A;
}
// ... and its launch for the solve `s` under gate `g`; returns its grid (= the number of partials it leaves in slots 18 and 1)
// `ho`: the hand-over form -- one workgroup more, which hands the step's results over as k_publish_final would (not among the partials)
int launch_front_cw(lorads_hip_ctx *c, const Solve &s, const FrontCwArgs &A, Guard g, Deferred d, const HandoverArgs *ho = nullptr) {
    Block &B = *s.B;
    double *r = c->cr + B.off, *rhs = c->rhs + B.off;
    double *pA = part_slot(c, 18), *pB = part_slot(c, 1);
    const RowDeal rd = row_deal_of(c, B);
    const int grid = rd.grid;
    const int ns = (B.r + 15) / 16;
    // (LAUNCH would send a virtual dual update off as its own kernel: this launch is the one that uses it)
    const bool keep = c->pend.set_dual_used(false);
    FrontSample fs(c);
    FrontCwHoArgs AH{};
    // (the hand-over form: `lead` workgroups ahead of the row workgroups, in the grid and in the kernel's argument alike)
    const int lead = ho ? 1 : 0;
    if (ho) { static_cast<FrontCwArgs &>(AH) = A; AH.ho = *ho; AH.ho.lead = lead; }
    // (LORADS_FRONT_CHAIN: the cuts belong to the form with the LDS park, the one they were measured on -- see k_front_cw)
    const int fc = c->opt.front_chain & FC_ALL;
#define FC_SWITCH(...)                                             \
    do { switch (fc) {                                             \
    case 0: { constexpr int FC_ = 0; __VA_ARGS__; } break;         \
    case 1: { constexpr int FC_ = 1; __VA_ARGS__; } break;         \
    case 2: { constexpr int FC_ = 2; __VA_ARGS__; } break;         \
    default: { constexpr int FC_ = 3; __VA_ARGS__; } break;        \
    } } while (0)
#define FCW(EWV, HO, AV) NS_SWITCH(8, true, ns, LAUNCH((k_front_cw<NS_, EWV, 0, HO>), grid + lead, B.n, rd.rpw, AV, s.V, B.r, (const double *)s.x, r, rhs, pA, pB, g, d))
    // (r <= 48: the first four slot rows are parked in LDS for the second visit, see k_front_cw; 48 KB per workgroup at most)
#define FCWL(NSV, EWV, HO, AV) FC_SWITCH(LAUNCH_LDS((k_front_cw<NSV, EWV, 4, HO, FC_>), grid + lead, sizeof(double2) * 32 * 4 * NSV * 8, B.n, rd.rpw, AV, s.V, B.r, (const double *)s.x, r, rhs, pA, pB, g, d))
#define FRONT(HO, AV)                                                                                                    \
    if (c->opt.front_lds && ns <= 3) {                                                                                   \
        if (B.cell_w == 8) { if (ns == 1) FCWL(1, 8, HO, AV); else if (ns == 2) FCWL(2, 8, HO, AV); else FCWL(3, 8, HO, AV); }     \
        else { if (ns == 1) FCWL(1, 16, HO, AV); else if (ns == 2) FCWL(2, 16, HO, AV); else FCWL(3, 16, HO, AV); }                \
    } else if (B.cell_w == 8) { FCW(8, HO, AV) } else { FCW(16, HO, AV) }
    if (ho) { FRONT(true, AH) } else { FRONT(false, A) }
#undef FRONT
#undef FCWL
#undef FCW
#undef FC_SWITCH
    fs.done();
    c->pend.set_dual_used(keep);
    return grid;
}
// the host-side state behind a one-kernel front: its launch, or the adoption of one that was enqueued ahead of its step
void front_cw_started(lorads_hip_ctx *c, const Solve &s, int grid, double tol) {
    s.B->w0_ready = true;
    c->pend.post_init(c, s.st, part_slot(c, 18), grid, part_slot(c, 1), grid, tol, s.front);
}
// may the U front of a fresh sweep take a waiting dual update along?  (see solve_front)
bool front_carries_dual(const lorads_hip_ctx *c, const Solve &s, int wmode) {
    return c->pend.dual_rides(s.front) && wmode == W_ADMM && c->nb == 1;
}
bool spec_front_adopt(lorads_hip_ctx *c, const Solve &s, double rho, double tol, CGState *reset, int nreset);

// rhs = V - (C + sum_i M1_i A_i) V / rho, initial residual, state  (lorads_admm.c:432-463, lorads_cgs.c:115,149-172)
void solve_front(lorads_hip_ctx *c, const Solve &s, double rho, double tol, CGState *reset = nullptr, int nreset = 0) {
    Block &B = *s.B;
    double *r = c->cr + B.off, *p = c->cp + B.off, *rhs = c->rhs + B.off;
    // Slots: ||r_0||^2 partials go to slot 18, NOT to slot 0 where the operator of iteration 0 writes its p.Q partials -- when
    // the solve's start rides on that very kernel (k_op_diag), some of its workgroups would still be summing the slot
    // while others already overwrite it (seen once in eight runs on a two-workgroup cone; certain on grids larger than
    // the device holds at once)
    double *pA = part_slot(c, 18), *pB = part_slot(c, 1);
    WArgs wa{};
    wa.csum = c->csum; wa.b = c->b; wa.lambda = c->lambda; wa.cv = B.cv; wa.row_idx = B.row_idx_identity ? nullptr : B.row_idx; wa.rho = ds_rho(c, rho);
    B.w0_ready = false;
    if (front_cw_ok(c, B)) {
        // the whole front in ONE kernel, coefficients formed on the fly (k_front_cw): no k_sval before it, and iteration 0's
        // constraint weights come out of it as per-slot contributions (k_wsum instead of k_cw)
        if (!B.t_uv_valid) { // (x, V) is this cone's (U, V) in either order
            cw(c, B, s.x, s.V, 1.0, B.w_uv, (double *)nullptr, (int)CV_SET, (double *)nullptr, s.front);
            B.t_uv_valid = true;
        }
        if (spec_front_adopt(c, s, rho, tol, reset, nreset)) return;
        FrontCwArgs A = front_cw_args(c, B, rho, c->virt_refresh ? W_ADMM_V : W_ADMM);
        c->virt_refresh = false;
        A.reset = reset; A.nreset = nreset;
        // a dual update that is still waiting is used on the fly by the ungated first kernel of the sweep of a cone that sees
        // every constraint, and stored by the k_wsum that follows (or by k_dual_update if anything else comes first)
        // (sharded: the cone sees its own constraints only -- the front needs no others -- and k_wsum updates the whole vector)
        if (front_carries_dual(c, s, A.wmode)) {
            A.rho_dual = ds_rho_dual(c, c->pend.use_dual());
            A.dual_on = 1;
        }
        // a waiting convergence test whose gate is this kernel's gate rides on it (the V-solve's front after a virtual refresh)
        const Deferred d = c->pend.take_check_behind(s.front);
        front_cw_started(c, s, launch_front_cw(c, s, A, s.front, d), tol);
        return;
    }
    if (fused_front(c, B)) {
        // one pass over V's rows gives the right-hand side AND the initial residual: the operator part of the residual,
        // (sum_i w_i A_i) V with w = A(sym(x V^T)), rides on the same neighbour rows as (C + sum_i M1_i A_i) V
        if (B.use_cw && !B.t_uv_valid) { // (x, V) is this cone's (U, V) in either order
            cw(c, B, s.x, s.V, 1.0, B.w_uv, (double *)nullptr, (int)CV_SET, (double *)nullptr, s.front);
            B.t_uv_valid = true;
        }
        int wmode = W_ADMM;
        if (c->virt_refresh && (B.use_cw || B.diag_only)) { // (see enqueue_sweep)
            wmode = W_ADMM_V;
            wa.w = B.w_uv;
            if (B.diag_only) { wa.drow = B.diag_row; wa.da = B.diag_a; }
        }
        c->virt_refresh = false;
        // a dual update that is still waiting rides on this kernel when it is the ungated first kernel of the sweep of a
        // cone that sees every constraint: the multipliers are read from lambda, the updated ones go to lambda_alt (owner
        // pairs), and the two vectors swap for everything enqueued from here on
        const bool carry_dual = c->pend.dual_rides(s.front) && wmode == W_ADMM && B.pu.e_con_own && B.nrow == c->m && B.pu.n_owned == c->m && c->nb == 1;
        const int *econ = B.pu.e_con;
        if (carry_dual) {
            wa.lambda_out = c->lambda_alt;
            wa.rho_dual = ds_rho_dual(c, c->pend.take_dual());
            econ = B.pu.e_con_own;
        }
        // Max-Cut-type cone with its rows' constraint lists: no coefficient pass, the front forms the diagonal coefficients itself
        const bool onfly = B.diag_only && B.rc_w > 0 && B.w_uv && c->opt.front_diag && &B != &c->merged; // (with or without a dual update on board)
        DiagOnFly of{};
        if (onfly) {
            of.on = true; of.wa = wa; of.wmode = wmode; of.reset = reset; of.nreset = nreset;
            of.d = c->pend.take_check_behind(s.front);
        } else {
            sval(c, B.pu, true, wmode, wa, s.front, reset, nreset, B.use_cw ? B.w_uv : (const double *)nullptr, econ);
        }
        FrontSample fs(c);
        const int nf = spmm_front(c, B, B.pu, s.V, s.x, rho, rhs, r, pA, pB, s.front, of);
        fs.done();
        if (carry_dual) std::swap(c->lambda, c->lambda_alt);
        if (B.diag_only && B.w_uv) B.t_uv_valid = true; // (the front has left the row dots U_p . V_p)
        c->pend.post_init(c, s.st, pA, nf, pB, nf, tol, s.front); // the solve's start rides on the first kernel of iteration 0 (or goes off on its own)
        return;
    }
    sval(c, B.pu, true, W_ADMM, wa, s.front, reset, nreset);
    if (B.dense_a && B.wj_for != s.V) dense_cache_fill(c, B, s.V, s.front); // (the fixed factor of this solve: nd GEMMs once, none per application)
    if (B.dense_c || B.dense_a) dense_part(c, B, s.V, W_ADMM, wa, 1.0, true, s.front);
    const int nb1 = spmm(c, B, B.pu, s.V, OP_RHS, nullptr, nullptr, rho, rhs, pB, s.front, (B.dense_c || B.dense_a) ? B.Wd : nullptr);
    const int na = apply_operator(c, B, s.V, s.x, OP_RES, rhs, r, pA, s.front);
    c->pend.post_init(c, s.st, pA, na, pB, nb1, tol, s.front);
}
// CG iteration 0 of this cone takes alpha = rr / (rr + ||w||^2) (cg0_alpha, see Cg0Args) when its operator application runs
// k_wsum: the w that k_wsum leaves must be exactly the w that k_spmm_ell applies -- one cone on the k_front_cw path (not the
// merged lockstep cone, no dense constraint part, fixed-width slot list), its k_wsum grid within one partial-sum slot.  A sharded
// cone qualifies as well: its solve's operator is built from the rank's own slot lists alone, which k_wsum and k_spmm_ell share.
bool cg0_rule(lorads_hip_ctx *c, const Block &B) {
    return front_cw_ok(c, B) && B.nrow > 0 && nblocks_for((size_t)B.nrow, TPB / 8) <= c->maxpart;
}
// body of CG iteration k up to and including the convergence test (lorads_cgs.c:180-194)
void solve_iter_body(lorads_hip_ctx *c, const Solve &s, int k, double tol, int maxit, bool fold_avg = false) {
    Block &B = *s.B;
    double *r = c->cr + B.off, *p = k == 0 ? c->cr + B.off : c->cp + B.off, *Q = c->cQ + B.off; // p_0 = r_0
    double *pA = part_slot(c, 0), *pC = part_slot(c, 2);
    const Guard g{&s.st->done, s.front.need};
    const bool rec = constr_by_recurrence(c, B) && B.t_uv_valid; // (valid since the front's initial residual)
    // the update below moves x by alpha p: w_op = A(sym(p V^T)) from the operator  =>  A(sym(x V^T)) += alpha w_op
    const int nw = !rec ? 0 : B.diag_only ? B.n : B.nrow; // (row dots for Max-Cut-type cones, constraint values otherwise)
    const bool v2 = (s.len & 1) == 0 && (((uintptr_t)s.x | (uintptr_t)r | (uintptr_t)p | (uintptr_t)Q) & 15) == 0;
    // the residual of an iteration whose tail is a restart is recomputed there: summed here, not stored
    const int store_r = (k % 20 != 0 || !c->opt.lazy_scalars) ? 1 : 0;
    // R = (U + V) / 2 left by this update when it is the last one enqueued before an evaluation (x = V, the other factor = U)
    const double *avg_other = fold_avg ? s.V : (const double *)nullptr;
    double *avg_out = fold_avg ? c->R + B.off : (double *)nullptr;
    if (fold_avg) c->avg_folded = true;
    const bool v2_avg = v2 && (!fold_avg || (((uintptr_t)avg_other | (uintptr_t)avg_out) & 15) == 0);
    // iteration 0 right behind the one-kernel front (its weights come out of k_wsum, see apply_operator): alpha from ||w||^2, and
    // the update inside k_spmm_ell (LORADS_FUSE_CG0=0: k_cg_update with the same alpha)
    const bool rule0 = k == 0 && B.w0_ready && cg0_rule(c, B);
    double *pW = rule0 ? part_slot(c, 20) : (double *)nullptr;
    const int nww = rule0 ? nblocks_for((size_t)B.nrow, TPB / 8) : 0;
    const bool fuse0 = rule0 && c->opt.fuse_cg0 && v2_avg;
    Cg0Args u{};
    u.wt = c->opt.wt_stores;
    if (fuse0) {
        u.st = s.st; u.part_ww = pW; u.nww = nww; u.x = s.x; u.r = r; u.store_r = store_r;
        u.w_acc = rec ? B.w_uv : (double *)nullptr; u.w_p = B.w_op; u.nw = nw; u.shadow = shadow_of(c, s.st);
        u.avg_other = avg_other; u.avg_out = avg_out;
    }
    // (fused: the operator kernel leaves the partials of the new residual's norm in pC, there are as many as it has workgroups)
    const int npq = apply_operator(c, B, s.V, p, OP_CG, nullptr, Q, fuse0 ? pC : pA, g, pW, fuse0 ? &u : (const Cg0Args *)nullptr);
    int nrr = npq;
    if (!fuse0) {
        if (v2_avg)
            LAUNCH(k_cg_update<true>, s.gv, s.len, s.st, pA, npq, s.x, r, p, Q, pC, g, rec ? B.w_uv : (double *)nullptr,
                   (const double *)B.w_op, nw, shadow_of(c, s.st), store_r, avg_other, avg_out, s.tile, s.tile_w, (const double *)pW, nww);
        else
            LAUNCH(k_cg_update<false>, s.gv, s.len, s.st, pA, npq, s.x, r, p, Q, pC, g, rec ? B.w_uv : (double *)nullptr,
                   (const double *)B.w_op, nw, shadow_of(c, s.st), store_r, avg_other, avg_out, s.tile, s.tile_w, (const double *)pW, nww);
        nrr = s.gv;
    }
    B.t_uv_valid = rec; // x (= U or V) moved: the kept values moved with it, or are stale
    if (B.wj_for == s.x) B.wj_for = nullptr; // (... and so are products kept for x as a fixed factor)
    c->merged.t_uv_valid = false;
    c->pend.post_check(c, s.st, pC, nrr, tol, maxit, g); // the convergence test rides on the next kernel if that kernel can carry it
}
// tail of CG iteration k: restart with the true residual when k % 20 == 0 (incl. k = 0), new direction (:195-228)
// `runs_for_sure`: the host has seen this solve unfinished and nothing is enqueued between that observation and this
// tail (first kernels of a resume)
void solve_iter_tail(lorads_hip_ctx *c, const Solve &s, int k, double tol, int maxit, bool runs_for_sure = false) {
    Block &B = *s.B;
    double *r = c->cr + B.off, *p = c->cp + B.off, *rhs = c->rhs + B.off;
    double *pA = part_slot(c, 19); // (the restart's residual partials: not the slot the next operator application writes, see solve_front)
    const Guard g{&s.st->done, s.front.need};
    if (k % 20 == 0) {
        const bool was_valid = B.t_uv_valid;
        if (k > 0) B.t_uv_valid = false; // a restart past iteration 0 recomputes the pair's constraint values from the factors
        const int nr = apply_operator(c, B, s.V, s.x, OP_RES, rhs, r, pA, g);
        // The recomputation is gated like every kernel of the solve: if the solve has finished by then it does not run.
        // Harmless when the kept values were valid (they still are); but values that were stale before (resume after a
        // speculation miss) must not be taken for fresh on the strength of a kernel that may have been skipped.
        if (!was_valid && !runs_for_sure) B.t_uv_valid = false;
        if (c->opt.lazy_scalars && B.diag_only && c->opt.fuse_dir) { // p = 2 r is formed by the next operator application itself
            c->pend.post_dir(Pending::Dir{DIR_RESTART, s.st, r, p, s.len, s.gv, pA, nr, g});
        } else if (c->opt.lazy_scalars) { // the restart's two scalars are written by workgroup 0 of the direction kernel
            LAUNCH(k_cg_dir, s.gv, s.len, s.st, (int)DIR_RESTART, r, p, g, Deferred{}, (const double *)pA, nr);
        } else {
            LAUNCH(k_cg_check, 1, s.st, (int)CHK_RESTART, pA, nr, ds_tol(c, tol), ds_maxit(c, maxit), g);
            LAUNCH(k_cg_dir, s.gv, s.len, s.st, (int)DIR_RESTART, r, p, g);
        }
    } else if (c->opt.lazy_scalars && B.diag_only && c->opt.fuse_dir) {
        // p = r + beta p is formed by the next operator application itself (and the waiting test rides on it too)
        c->pend.post_dir(Pending::Dir{DIR_BETA, s.st, r, p, s.len, s.gv, nullptr, 0, g});
    } else {
        const Deferred d = c->pend.take_check_of(s.st);
        LAUNCH(k_cg_dir, s.gv, s.len, s.st, (int)DIR_BETA, r, p, g, d);
    }
}
// iterations [k0, k1): bodies, with tails between them (the tail of the last one is left to a resume)
void solve_iters(lorads_hip_ctx *c, const Solve &s, int k0, int k1, double tol, int maxit, bool fold_avg_last = false) {
    for (int k = k0; k < k1; ++k) {
        if (k > k0) solve_iter_tail(c, s, k - 1, tol, maxit);
        solve_iter_body(c, s, k, tol, maxit, fold_avg_last && k == k1 - 1);
    }
}
// constrVal[k] <- A_k(sym(U V^T)) and constrValSum += new - old (lorads_alg_common.c:199-203)
void refresh_after_solve(lorads_hip_ctx *c, Block &B, const int *need) {
    if (constr_by_recurrence(c, B) && B.t_uv_valid && B.nrow > 0) { // w_uv already is A(sym(U V^T)): bookkeeping only
        const Deferred d = c->pend.take_check_behind(Guard{nullptr, need});
        LAUNCH(k_refresh_w, nblocks_for((size_t)B.nrow, TPB), B.nrow, (const double *)B.w_uv, B.cv, B.row_idx, c->csum,
               Guard{nullptr, need}, d, B.diag_only ? (const int *)B.diag_row : (const int *)nullptr,
               B.diag_only ? (const double *)B.diag_a : (const double *)nullptr);
        return;
    }
    constr_val(c, B, c->U + B.off, c->V + B.off, 1.0, B.cv, CV_DELTA, c->csum, Guard{nullptr, need});
}

void flush_final(lorads_hip_ctx *c);
bool spec_front_enqueue(lorads_hip_ctx *c, double rho, const HandoverArgs *ho = nullptr);
// hand [word0, word0 + nwords) of the control block over to its pinned mirror: the kernel that copies the words and publishes the
// next sequence number (the last kernel of every launch chain that is replayed as a graph) ...
// `front_rho`: the next step's U front may be enqueued behind this hand-over (run_sweep), at that rho.  Where the hand-over is the
// evaluation's (k_publish_final) over the usual words, that front's launch carries it as one more workgroup
// (LORADS_HANDOVER_ON_FRONT=0: never) and *front_carried says so; every other hand-over is a launch of its own, as ever.
int enqueue_publish(lorads_hip_ctx *c, size_t word0, size_t nwords, const double *front_rho = nullptr, bool *front_carried = nullptr) {
    if (c->sx_pending && (word0 > SX_WORD || word0 + nwords < SX_WORD + 4)) { // the staged local sums travel with this hand-over
        const size_t w1 = std::max(word0 + nwords, (size_t)SX_WORD + 4);
        word0 = std::min(word0, (size_t)SX_WORD);
        nwords = w1 - word0;
    }
    int sep_with_obj = 0;
    SepExtra ex{};
    const bool sep = !c->final_pending && c->pend.take_sep(4, &sep_with_obj, &ex); // (taken by this hand-over)
    c->pend.flush(c);
    ++c->pub_seq;
    if (sep) {
        LAUNCH(k_publish_sep, 1, (const double *)c->sepbuf, c->scal, sep_with_obj, ex.n, ex.p[0], ex.p[1], ex.p[2],
               ex.p[3], (const unsigned long long *)c->ctrl + word0, (int)nwords, (unsigned long long *)c->h_ctrl_dev + word0,
               c->h_flag_dev, c->seq_dev);
    } else if (c->final_pending) {
        const HandoverArgs H{c->final_args, (const unsigned long long *)c->ctrl + word0, (unsigned long long *)c->h_ctrl_dev + word0,
                             (int)nwords, c->h_flag_dev, c->seq_dev, 0}; // (lead: set by launch_front_cw with the grid)
        const bool own = (const double *)H.src == H.fa.out; // (as k_publish_final sees it)
        if (front_rho && c->opt.handover_on_front && own && spec_front_enqueue(c, *front_rho, &H)) {
            *front_carried = true;
            c->final_pending = false;
            ++c->n_handover_front;
            return 0;
        }
        LAUNCH(k_publish_final, 1, H.fa, H.src, H.nwords, H.dst, H.flag, H.seq_dev);
        c->final_pending = false;
    } else {
        LAUNCH(k_publish, 1, (const unsigned long long *)c->ctrl + word0, (int)nwords, (unsigned long long *)c->h_ctrl_dev + word0,
               c->h_flag_dev, c->seq_dev);
    }
    ++c->n_handover_alone;
    return 0;
}
// separable shards with a scalar exchange: the hand-over has brought this rank's LOCAL sums of the evaluation; the ranks' hosts sum
// them now and the mirror gets what k_sep_commit would have written (the device's copy keeps the local numbers: nothing on the
// device reads them)
int sx_exchange(lorads_hip_ctx *c) {
    if (!c->sx_pending) return 0;
    c->sx_pending = false;
    double v[4] = {c->h_scal[SX_WORD], c->h_scal[SX_WORD + 1], c->h_scal[SX_WORD + 2], c->h_scal[SX_WORD + 3]};
    if (!c->sx || c->sx(c->sx_user, v, 4)) return fail_msg("scalar exchange of separable shards failed (a rank that never arrived?)");
    c->n_sx++;
    c->h_scal[0] = v[0];
    c->h_scal[1] = v[1];
    if (c->sx_with_obj) c->h_scal[2] = v[2];
    c->h_scal[5] = v[3];
    return 0;
}
// ... and the wait for it
int wait_publish(lorads_hip_ctx *c) {
    const unsigned long long seq = c->pub_seq;
    if (c->launch_err) { const char *e = c->launch_err; c->launch_err = nullptr; hipStreamSynchronize(c->stream); return fail_msg(e); } // (a step that could not be enqueued: its results mean nothing)
    { // a launch that was refused (bad configuration, lost device) never publishes: say so instead of spinning
        hipError_t le = hipGetLastError();
        if (le != hipSuccess) return fail("kernel launch", le);
    }
    volatile unsigned long long *f = c->h_flag;
    // wall-clock bound on the wait (LORADS_HANDOVER_TIMEOUT_S, default 300): a collective on the stream that a peer never
    // enters (a rank that left the loop, a dead process) keeps hipStreamQuery at NotReady for ever -- report it instead
    const double limit_s = opt_handover_timeout_s();
    std::chrono::steady_clock::time_point t0;
    bool timing = false;
    for (unsigned long spins = 0;; ++spins) {
        if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == seq) return sx_exchange(c);
        if ((spins & 0xfffff) == 0xfffff) { // every ~million spins: is the stream still alive?
            hipError_t q = hipStreamQuery(c->stream);
            if (q == hipSuccess) { // everything ran: the flag must be there
                if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == seq) return sx_exchange(c);
                HC(hipStreamSynchronize(c->stream));
                if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == seq) return sx_exchange(c);
                return fail_msg("result hand-over: sequence number not published");
            }
            if (q != hipErrorNotReady) return fail("hipStreamQuery", q);
            if (!timing) { t0 = std::chrono::steady_clock::now(); timing = true; }
            else if (limit_s > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s)
                return fail_msg("result hand-over: the stream did not finish within LORADS_HANDOVER_TIMEOUT_S (a collective "
                                "that not every rank entered?)");
        }
    }
}
// copy [word0, word0 + nwords) of the control block to its pinned mirror and wait for it
int publish_and_wait(lorads_hip_ctx *c, size_t word0, size_t nwords) {
    if (enqueue_publish(c, word0, nwords)) return 1;
    return wait_publish(c);
}
size_t state_words(const lorads_hip_ctx *c) { return (64 * sizeof(double) + sizeof(CGState) * (size_t)(2 * c->nb)) / 8; }
int read_states(lorads_hip_ctx *c) { return publish_and_wait(c, 0, state_words(c)); }

Solve make_solve(lorads_hip_ctx *c, int k, int half, const int *need) {
    Block &B = c->blk[k];
    Solve s;
    s.B = &B;
    s.x = (half == 0 ? c->U : c->V) + B.off;
    s.V = (half == 0 ? c->V : c->U) + B.off;
    s.st = c->st + 2 * k + half;
    s.front = Guard{nullptr, need};
    s.len = (size_t)B.n * B.r;
    s.gv = std::min(grid1d(s.len), 512); // (512 workgroups stream fastest: ubench variants 6-9, profiles/r01_ubench.txt; their partials are re-summed by the next kernel)
    if (B.diag_only && c->opt.tile_update) { // row-local operator: the update works on the operator's row tiles (same workgroup -> same XCD)
        const int rows = TPB / shape_for(B.r).lg, g = nblocks_for((size_t)B.n, rows);
        if (g <= c->maxpart && rows * B.r >= TPB / 2) { s.gv = g; s.tile = rows * B.r; s.tile_w = rows; }
    }
    return s;
}

// ---- the U front of the NEXT ADMM step, enqueued behind this step's hand-over (LORADS_SPEC_FRONT, DESIGN.md 4)
// Between the hand-over kernel and the next step's first kernel the GPU waits for the host: the flag's way to the host, the caller's
// stop decisions, update_dual_var, the next enqueue.  The next step's U front reads U, V, csum, cv, w_uv, b, lambda, rho and the
// dual step -- all final once the evaluation has run -- and writes scratch alone (cr, rhs, w_contrib, partial slots 18 and 1; the
// dual update it forms on the fly is stored later, by k_wsum).  So it is enqueued now, on the guess that the host goes on as
// lrd_admm_optimize does between two steps: update_dual_var(rho), admm_step(rho).  Anything else (spec_touch) leaves its output unused.
// May this step, whose sweep and evaluation are about to be enqueued, be followed by such a front?
bool spec_front_ok(lorads_hip_ctx *c) {
    if (!c->opt.spec_front || c->ar || c->nb != 1 || !c->opt.lazy_scalars || !c->lambda_alt) return false;
    if (c->prof && c->prof_every < (1 << 20)) return false; // (a window that times launches between events: nothing runs differently in it)
    return front_cw_ok(c, c->blk[0]) && !c->blk[0].is_lp;
}
// `ho`: this step's hand-over, not launched yet, rides on the front's launch (see enqueue_publish).  Returns whether a front went off.
bool spec_front_enqueue(lorads_hip_ctx *c, double rho, const HandoverArgs *ho) {
    Block &B = c->blk[0];
    if (!B.t_uv_valid || c->pend.dual_owed()) return false;
    const Solve s = make_solve(c, 0, 0, nullptr);
    FrontCwArgs A = front_cw_args(c, B, rho, W_ADMM);
    A.dual_on = 1;
    A.rho_dual = ds_rho_dual(c, rho);
    // gated like the evaluation: if this step's V-solve missed its speculation the resume still needs cr and rhs, and a blocked
    // front writes nothing.  No reset words: they would shut the very gate it waits at (the k_wsum behind it takes them).
    // (with the hand-over on board: its workgroup has its own gate, the evaluation's, and publishes whether or not the rows write)
    launch_front_cw(c, s, A, Guard{nullptr, &c->st[2 * c->nb - 1].done}, Deferred{}, ho);
    c->spec.live = true; c->spec.dual_seen = false;
    c->spec.rho = rho; c->spec.rho_dual = rho; c->spec.wmode = W_ADMM; c->spec.epoch = c->spec_epoch;
    ++c->n_spec_enq;
    return true;
}
// stage 0 of a fresh sweep: take the front that is already there instead of launching one?
bool spec_front_adopt(lorads_hip_ctx *c, const Solve &s, double rho, double tol, CGState *reset, int nreset) {
    if (!c->spec.live) return false;
    c->spec.live = false;
    Block &B = *s.B;
    const bool ok = s.st == c->st && reset && !c->par_mode && c->spec.epoch == c->spec_epoch && memcmp(&rho, &c->spec.rho, sizeof(double)) == 0 &&
                    c->spec.dual_seen && c->pend.dual_owed_at(c->spec.rho_dual) && !c->virt_refresh &&
                    c->spec.wmode == W_ADMM && front_carries_dual(c, s, W_ADMM) && B.t_uv_valid && c->opt.lazy_scalars &&
                    B.spec[0] >= 1; // (iteration 0 is enqueued: its k_wsum is the next launch and takes the reset words)
    if (!ok) { ++c->n_spec_discard; return false; }
    ++c->n_spec_adopt;
    c->pend.use_dual();
    c->virt_refresh = false;
    c->spec.reset = reset; c->spec.nreset = nreset;
    c->n_front++; // (as the launch would have counted it)
    front_cw_started(c, s, row_deal_of(c, B).grid, tol);
    return true;
}

// the LP block's ADMM update (see k_lp_sweep); st = the block's two stage states
void enqueue_lp_sweep(lorads_hip_ctx *c, Block &B, double rho, CGState *st, Guard g) {
    c->pend.flush(c);
    LpArgs A;
    A.ncols = B.n; A.nlev = B.lp_nlev; A.lvl_ptr = B.lp_lvl_ptr; A.lvl_cols = B.lp_lvl_cols; A.ptr = B.lp_ptr; A.grow = B.lp_grow;
    A.a = B.lp_a; A.nrm2sq = B.lp_nrm2sq; A.cobj = B.lp_cobj; A.cv = B.lp_cv; A.U = c->U + B.off; A.V = c->V + B.off;
    A.csum = c->csum; A.b = c->b; A.lambda = c->lambda; A.rho = ds_rho(c, rho);
    B.t_uv_valid = false;
    if (B.lp_nlev <= 1) {
        LAUNCH(k_lp_sweep_flat, nblocks_for((size_t)B.n, TPB), A, g);
        hipLaunchKernelGGL(k_lp_done, dim3(1), dim3(1), 0, c->stream, st, g);
    } else {
        LAUNCH(k_lp_sweep, 1, A, st, g);
    }
}
// constrValLP of the LP block from the pair (X, Y)
void lp_col_values(lorads_hip_ctx *c, Block &B, const double *X, const double *Y, Guard g) {
    if (!B.is_lp || B.n == 0) return;
    LAUNCH(k_lp_cv, nblocks_for((size_t)B.n, TPB), B.n, B.lp_ptr, B.lp_a, X + B.off, Y + B.off, B.lp_cv, g);
}

// LORADSUpdateSDPVar (lorads_alg_common.c:187-215) for all cones of this context, enqueued speculatively
// from stage `first` (stage = 2*cone + half); `resume_iter` >= 0 resumes that stage's CG after that many
// completed iterations
void enqueue_sweep(lorads_hip_ctx *c, int first, int resume_iter, double rho, double tol, int maxit, bool eval_follows) {
    c->virt_refresh = false;
    for (int stg = first; stg < 2 * c->nb; ++stg) {
        const int k = stg / 2, half = stg % 2;
        const int *need = stg == 0 ? nullptr : &c->st[stg - 1].done;
        Solve s = make_solve(c, k, half, need);
        Block &B = *s.B;
        if (B.is_lp) { // both halves of every column in one go at the block's first stage; never a speculation miss
            if (half == 0) enqueue_lp_sweep(c, B, rho, c->st + stg, Guard{nullptr, need});
            continue;
        }
        if (stg == first && resume_iter >= 0) {
            const int more = std::max(2, std::min(resume_iter, 16));
            if (resume_iter > 0) solve_iter_tail(c, s, resume_iter - 1, tol, maxit, true);
            solve_iters(c, s, resume_iter, std::min(resume_iter + more, maxit), tol, maxit);
        } else {
            // a fresh sweep marks every later stage "not finished" in its very first kernel
            const bool fresh0 = stg == 0 && resume_iter < 0 && 2 * c->nb - 1 <= TPB;
            solve_front(c, s, rho, tol, fresh0 ? c->st + 1 : nullptr, fresh0 ? 2 * c->nb - 1 : 0);
            // the sweep's very last update also leaves the average the evaluation starts from (one cone on the k_cw path: its
            // evaluation's first kernel can carry the convergence test k_average used to carry); LORADS_FOLD_AVG=0: k_average
            // (sharded cones too: the evaluation's first constraint kernel is this cone's k_cw there as well, and whatever comes
            // first sends a waiting test off as its own launch if it cannot carry it)
            const bool fold = eval_follows && stg == 2 * c->nb - 1 && c->nb == 1 && B.use_cw && c->opt.lazy_scalars &&
                              c->opt.fold_avg && B.nrow > 0 && nblocks_for((size_t)B.nrow, TPB / 64) <= c->maxpart;
            solve_iters(c, s, 0, std::min(B.spec[half], maxit), tol, maxit, fold);
        }
        if (eval_follows && stg == 2 * c->nb - 1) {
            // the evaluation that follows overwrites constrVal / constrValSum with A(R R^T) (Q1): after the very last
            // solve only the pair dots are kept (the next sweep's first residual re-uses them)
            if (B.use_cw) {
                const bool exact_now = (c->n_sweeps % 32) == 31; // (see constr_by_recurrence)
                if (!(constr_by_recurrence(c, B) && B.t_uv_valid) || exact_now)
                    cw(c, B, c->U + B.off, c->V + B.off, 1.0, B.w_uv, (double *)nullptr, (int)CV_SET, (double *)nullptr,
                       Guard{nullptr, &s.st->done});
                B.t_uv_valid = true;
            } else if (!B.diag_only && !B.entry_only) { // (those operators never read the pair dots)
                pairdots(c, B.pa, c->U + B.off, c->V + B.off, B.r, B.T, Guard{nullptr, &s.st->done});
                B.t_uv_valid = true;
            }
        } else if (eval_follows && c->nb == 1 && stg == 0 && c->opt.lazy_scalars && constr_by_recurrence(c, B) && B.t_uv_valid &&
                   fused_front(c, B) && (B.use_cw || B.diag_only)) {
            // One cone, evaluation at the end of the sweep: what the refresh after the U-solve would store (constrVal <- w_uv,
            // constrValSum += w_uv - old) has ONE reader, the weights of the V-solve's front -- the evaluation overwrites both
            // vectors (Q1).  The front forms its weights from w_uv directly (W_ADMM_V, same arithmetic) and nothing is
            // stored: no k_refresh_w launch, and the waiting convergence test rides on the front's k_sval instead.
            c->virt_refresh = true;
        } else {
            if (stg == 2 * c->nb - 1 && (c->n_sweeps % 32) == 31) B.t_uv_valid = false; // the same cadence without an evaluation
            refresh_after_solve(c, B, &s.st->done);
        }
    }
}

// after a sync: first stage >= first whose solve is not finished, or -1
int first_unfinished(lorads_hip_ctx *c, int first) {
    for (int stg = first; stg < 2 * c->nb; ++stg)
        if (c->h_st[stg].done == 0) return stg;
    return -1;
}

// objective + DIMACS refresh (calObj_admm + LORADSCalDualObj + updateDimacsADMM, lorads_admm.c:79-81):
// R = (U+V)/2 (pair UV), constrVal <- A(R R^T), constrValSum, then scal[0..2] = {||b-sum||^2, b.lambda, <C,RR^T>}
void flush_final(lorads_hip_ctx *c) { // closing sums of an earlier evaluation that no hand-over has picked up yet
    if (!c->final_pending) return;
    const EvalFinalArgs &fa = c->final_args;
    LAUNCH(k_eval_final, 1, fa.part_v, fa.part_d, fa.np, fa.out, fa.g, fa.obj_part, fa.nobj);
    c->final_pending = false;
}
int enqueue_eval(lorads_hip_ctx *c, int pair, const int *need, bool with_obj = true) {
    flush_final(c);
    const Guard g{nullptr, need};
    const bool vec = shard_vec(c); // (separable shards evaluate as a single GPU does and sum four scalars at the end)
    // one Max-Cut-type cone that sees every constraint: average, constraint values and residual partials in ONE row kernel
    // (the only cone, or the merged block-diagonal cone of a lockstep sweep: its rows, constraints and constrVal array are the
    // concatenation of the cones')
    Block *Dc = solo(c);
    Block *D1 = (pair == LORADS_HIP_PAIR_UV && !vec && c->opt.eval_diag && Dc && Dc->diag_only && Dc->rc_w > 0 && Dc->nrow == c->m &&
                 c->m > 0 && Dc->w_uv && !c->avg_folded && !Dc->dense_c) ? Dc : nullptr;
    if (D1) {
        // (k_eval_diag below carries a waiting test and forms R itself)
    } else if (pair == LORADS_HIP_PAIR_UV && c->avg_folded && need) {
        c->avg_folded = false; // the sweep's last update has left R (see solve_iter_body); a waiting test rides on the next kernel
    } else if (pair == LORADS_HIP_PAIR_UV) {
        c->avg_folded = false;
        const Deferred d = c->pend.take_check_behind(g);
        LAUNCH(k_average, grid1d(c->all_elem), c->all_elem, c->U, c->V, c->R, g, d);
    }
    Block *S1 = solo(c);
    if (S1 && (S1->nrow != c->m || S1->dense_c)) S1 = c->nb == 1 ? S1 : nullptr;
    const bool single = (S1 && S1->nrow == c->m) || (c->nb == 1 && c->blk[0].nrow == c->m);
    bool any_dense_a = false;
    for (auto &B0 : c->blk) any_dense_a = any_dense_a || B0.dense_a;
    // the constraint-value kernel also delivers the residual partials (not with dense constraint matrices: their values join later)
    const bool fold_res = single && !vec && c->m > 0 && !any_dense_a;
    c->ls_np = 0;
    // sharded cones: the local sums go to a staging vector, are all-reduced there and committed to constrValSum only
    // if no rank reported a speculation miss (an unfinished sweep still needs the old constrValSum)
    double *dst = vec ? c->cstage : c->csum;
    std::vector<Block *> cones;
    if (S1) cones.push_back(S1);
    else for (auto &B0 : c->blk) cones.push_back(&B0);
    // One local cone (the block-per-GPU layout): the objective partials travel through the all-reduce themselves, behind
    // the two tail words k_obj writes, and k_commit_eval leaves the staged sums zeroed for the next evaluation -- three
    // launches fewer around the collective (no k_zero, no k_stage_tail)
    // (the length of the collective must be the same on every rank: the ranks agree once -- one host-side sum through the hook --
    // that each of them holds one such cone; a deal that leaves some rank two cones takes the general form everywhere)
    if (vec && c->ar_fast_all < 0) {
        double v[2] = {(c->nb == 1 && !c->blk[0].dense_c && c->blk[0].nc > 0 && !c->blk[0].is_lp) ? 1.0 : 0.0, 1.0};
        c->pend.flush(c);
        HC(hipStreamSynchronize(c->stream));
        if (c->ar(c->ar_user, v, 2, 0)) return fail_msg("allreduce hook failed");
        c->ar_fast_all = v[0] == v[1] ? 1 : 0;
    }
    const bool ar_fast = vec && with_obj && c->ar_fast_all == 1 && cones.size() == 1;
    if ((!single || vec) && !(ar_fast && c->stage_clean)) LAUNCH(k_zero, grid1d((size_t)c->m), (size_t)c->m, dst, g);
    bool first_obj = true;
    const bool fold_obj = (c->nb == 1 || S1) && !vec; // the final kernel sums the objective partials itself
    int nobj = 0, nres = 0;
    for (Block *bp : cones) {
        Block &B = *bp;
        if (D1 == &B && fold_res) {
            const Deferred d = c->pend.take_check_behind(g);
            const Shape sh = shape_for(B.r);
            nres = nblocks_for((size_t)B.n, TPB / sh.lg);
            SHAPE_DISPATCH(sh, LAUNCH((k_eval_diag<LG_, V2_, NS_>), nres, B.n, (const double *)(c->U + B.off), (const double *)(c->V + B.off),
                                      c->R + B.off, B.r, B.rc_w, (const int *)B.rc_con, (const double *)B.diag_a,
                                      B.row_idx_identity ? (const int *)nullptr : (const int *)B.row_idx, B.cv, c->csum,
                                      (const double *)c->b, (const double *)c->lambda, part_slot(c, 8), part_slot(c, 9), g, d));
        } else if (fold_res && B.use_cw && with_obj && fold_obj && c->opt.fuse_eval && cw_quad(c, B) && B.nc > 0 && !B.dense_c &&
                   nblocks_for((size_t)B.nrow, TPB / 64) <= c->maxpart) {
            // constraint values + residual partials AND the objective partials in one launch (k_eval_cw_obj)
            const Deferred d = c->pend.take_check_behind(g);
            nres = nblocks_for((size_t)B.nrow, TPB / 64);
            nobj = std::min(nblocks_for((size_t)B.nc, TPB / 8), 2048);
            const int ns4 = (B.r + 7) / 8, ns = (B.r + 15) / 16;
            const ResArgs ra{c->b, c->lambda, part_slot(c, 8), part_slot(c, 9)};
#define EVF(A4, A8) LAUNCH((k_eval_cw_obj<A4, A8>), nres + nobj, B.nrow, B.ca_ell, (const int *)B.ca_row, (const double *)B.ca_val, (const int *)B.ca_col, \
                           (const double *)(c->R + B.off), B.r, B.cv, (const int *)B.row_idx, c->csum, ra, nres, B.nc, (const int *)B.c_row,           \
                           (const int *)B.c_col, (const double *)B.c_val, part_slot(c, 4), g, d)
            switch (ns4) {
            case 1: EVF(1, 1); break;
            case 2: EVF(2, 1); break;
            case 3: EVF(3, 2); break;
            case 4: EVF(4, 2); break;
            case 5: EVF(5, 3); break;
            default: EVF(6, 3); break;
            }
#undef EVF
            (void)ns;
            lp_col_values(c, B, c->R, c->R, g);
            continue; // (objective partials are in slot 4: the closing kernel sums them, as with fold_obj)
        } else if (fold_res && B.use_cw && nblocks_for((size_t)B.nrow, TPB / 64) <= c->maxpart) {
            // constraint values straight from the factors, residual partials on the same launch (one kernel instead of two)
            nres = cw(c, B, c->R + B.off, c->R + B.off, 1.0, (double *)nullptr, B.cv, (int)CV_SET, c->csum, g,
                      ResArgs{c->b, c->lambda, part_slot(c, 8), part_slot(c, 9)});
        } else if (fold_res) {
            pairdots(c, B.pa, c->R + B.off, c->R + B.off, B.r, B.T2, g);
            nres = std::min(nblocks_for((size_t)B.nrow, TPB / 8), 2048);
            LAUNCH(k_cv_res, nres, B.nrow, B.a_ptr, B.a_e, B.a_val, B.T2, B.cv, B.row_idx, c->csum, c->b, c->lambda, part_slot(c, 8),
                   part_slot(c, 9), g);
        } else {
            constr_val(c, B, c->R + B.off, c->R + B.off, 1.0, B.cv, (single && !vec) ? CV_SET : CV_ADD, dst, g);
        }
        lp_col_values(c, B, c->R, c->R, g); // primalInfeasibilityLP re-initialises constrValLP too (:260-262)
        if (!with_obj) continue; // DIMACS refresh alone (lorads_alg_common.c:250-290) does not touch the objective
        const int go = obj_partials(c, B, c->R + B.off, c->R + B.off, ar_fast ? dst + c->m + 2 : part_slot(c, 4), g,
                                    ar_fast ? dst + c->m : (double *)nullptr);
        if (fold_obj || (vec && cones.size() == 1)) { nobj = go; continue; } // a later kernel sums the partials
        if (go) { LAUNCH(k_finalize, 1, part_slot(c, 4), go, 1.0, first_obj ? 0 : 1, c->scal + 2, g); first_obj = false; }
    }
    if (with_obj && first_obj && nobj == 0) LAUNCH(k_zero, 1, (size_t)1, c->scal + 2, g);
    if (vec) { // sharded cones: ONE all-reduce of [constrValSum | objective part | "I missed my speculation"]
        const bool obj_from_part = with_obj && cones.size() == 1 && nobj > 0;
        if (!ar_fast)
            LAUNCH(k_stage_tail, 1, obj_from_part ? part_slot(c, 4) : (const double *)nullptr, nobj, c->scal + 2, need, dst + c->m);
        c->pend.flush(c);
        if (allreduce_dev(c, dst, c->m + 2 + (ar_fast ? nobj : 0))) return 1;
        nres = std::max(1, std::min(grid1d((size_t)c->m), 256));
        LAUNCH(k_commit_eval, nres, c->m, dst, c->csum, c->b, c->lambda, part_slot(c, 8), part_slot(c, 9), c->scal,
               ar_fast ? nobj : 0);
        c->stage_clean = ar_fast;
    } else if (!fold_res) {
        nres = std::min(grid1d((size_t)c->m), 1024);
        LAUNCH(k_eval_part, nres, c->m, c->b, c->csum, c->lambda, part_slot(c, 8), part_slot(c, 9), g);
    }
    // the closing sums ride on the result hand-over that follows every evaluation (k_publish_final); without the
    // hand-over kernel they are a launch of their own
    const double *op = (fold_obj && nobj > 0) ? part_slot(c, 4) : (const double *)nullptr;
    if (c->ar && c->sep) {
        // separable shards: the closing sums now (not on the hand-over), then ONE all-reduce of {||b - csum||^2, b.lambda, <C,RR^T>,
        // "my sweep is unfinished"} -- a rank whose gate is shut sends zeros and the flag; k_sep_commit leaves the sums in scal[0..2]
        // and the number of such ranks in scal[5], where run_sweep looks for it (as after k_commit_eval)
        const SepExtra ex = c->sep_extra; // (phase 1: ||Grad||^2 and y.s of the step ride along, see lorads_hip_alm_step)
        c->sep_extra = SepExtra{};
        if (c->sx && ex.n == 0) {
            // the ranks' hosts sum them after the hand-over (lorads_hip_set_scalar_exchange): no collective on the stream
            LAUNCH(k_sep_stage_local, 1, part_slot(c, 8), part_slot(c, 9), nres, op, nobj, (const double *)c->scal, g, with_obj ? 1 : 0, c->scal + SX_WORD);
            c->sx_pending = true; c->sx_with_obj = with_obj ? 1 : 0;
            return 0;
        }
        LAUNCH(k_sep_stage, 1, part_slot(c, 8), part_slot(c, 9), nres, op, nobj, (const double *)c->scal, g, with_obj ? 1 : 0, c->sepbuf, ex);
        c->pend.flush(c);
        if (allreduce_dev(c, c->sepbuf, 4 + ex.n)) return 1;
        // (the commit of the reduced scalars rides on the hand-over that follows; flush_pending sends it off on its own otherwise)
        c->pend.post_sep(with_obj ? 1 : 0, ex);
        return 0;
    }
    c->final_args = EvalFinalArgs{part_slot(c, 8), part_slot(c, 9), op, nres, nobj, c->scal, g};
    c->final_pending = true;
    return 0;
}

int read_scalars_at(lorads_hip_ctx *c, const double *dptr, int count, double *out) {
    c->pend.flush(c);
    flush_final(c);
    if (c->launch_err) { const char *e = c->launch_err; c->launch_err = nullptr; hipStreamSynchronize(c->stream); return fail_msg(e); }
    HC(hipMemcpyAsync(c->h_scal + 32, dptr, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    memcpy(out, c->h_scal + 32, sizeof(double) * (size_t)count);
    return 0;
}
int read_scalars(lorads_hip_ctx *c, int first, int count, double *out) { // scal[first .. first+count)
    if (publish_and_wait(c, (size_t)first, (size_t)count)) return 1;
    memcpy(out, c->h_scal + first, sizeof(double) * (size_t)count);
    return 0;
}

// flat dot -> device scalar slot (+ cross-rank sum)
int dot_to_slot(lorads_hip_ctx *c, const double *x, const double *y, int slot, bool reduce = true) {
    int g = grid1d(c->all_elem);
    LAUNCH(k_dot, g, c->all_elem, x, y, part_slot(c, 3), NOGUARD);
    LAUNCH(k_finalize, 1, part_slot(c, 3), g, 1.0, 0, c->scal + slot, NOGUARD);
    return reduce ? allreduce_dev(c, c->scal + slot, 1) : 0; // (!reduce: the caller sends the local sum along with another collective)
}

// collect the sweep results after all stages are finished
int finish_sweep(lorads_hip_ctx *c, int *iters) {
    int tot = 0;
    for (int stg = 0; stg < 2 * c->nb; ++stg) {
        Block &B = c->blk[stg / 2];
        const CGState &h = c->h_st[stg];
        if (h.nan) fprintf(stderr, "lorads_hip: NaN residual in CG (cone %d)\n", stg / 2);
        if (h.done != 2) B.cg_iter_last = h.iter; // an immediate exit leaves the stale count (reference quirk)
        tot += B.cg_iter_last;
        // Speculation for the next sweep: the largest count of the last `spec_window` sweeps.  A solve that needs one iteration
        // more than was enqueued costs a host round trip (the GPU idles for ~20-30 us); an iteration enqueued in vain costs its
        // kernels' immediate exits (~2 us each).  Where the counts wander by one from sweep to sweep (Max-Cut: 5, 6, 5, 5, 6)
        // the previous count alone missed every few sweeps; where they are constant (the headline: 1) nothing changes.
        B.spec_hist[stg % 2][B.spec_pos % c->opt.spec_window] = h.done == 2 ? 0 : h.iter;
        int mx = 0;
        for (int k = 0; k < c->opt.spec_window; ++k) mx = std::max(mx, B.spec_hist[stg % 2][k]);
        B.spec[stg % 2] = mx;
        if (stg % 2 == 1) B.spec_pos++;
        c->n_cg_it += (h.done == 2 ? 0 : h.iter);
        c->n_solves++;
    }
    *iters = tot;
    return 0;
}

// ---- lockstep sweep over all cones on the merged cone (see SegArgs).  Phase 0 = all U-solves, phase 1 = all V-solves;
// every kernel of a phase is gated on phase_done[] -- skip when the phase is over, wait while the previous one is not.
// one wavefront per cone in the per-cone scalar kernels, up to sixteen side by side
int seg_threads(lorads_hip_ctx *c) { return 64 * std::max(1, std::min(c->nb, SEG_TPB / 64)); }
// the lockstep sweep's convergence tests ride on the next operator kernel (Max-Cut-type merged cone with the fused direction update;
// LORADS_SEG_CARRY=0: k_cg_check_seg after every update)
bool seg_carry(lorads_hip_ctx *c) {
    return c->merged.diag_only && c->opt.lazy_scalars && c->opt.fuse_dir && c->seg_tile_cone && c->seg_tile_info && c->opt.seg_carry && c->seg_rr_alt;
}
// k: the lockstep iteration the kernel belongs to (see SegArgs: which slot holds r.r)
SegArgs seg_args(lorads_hip_ctx *c, int half, int k) {
    SegArgs sa;
    sa.row0 = c->seg_row0; sa.vt0 = c->seg_vt0; sa.vt_seg = c->seg_vt_seg; sa.vt_e0 = c->seg_vt_e0; sa.st = c->st;
    sa.phase_done = c->phase_done; sa.half = half; sa.ncones = c->nb; sa.rpw = TPB / shape_for(c->merged.r).lg; sa.r = c->merged.r;
    const bool carry = seg_carry(c);
    sa.rr_alt = c->seg_rr_alt; sa.slot_rd = carry ? (k & 1) : 0; sa.slot_wr = carry ? ((k + 1) & 1) : 0;
    return sa;
}
void batched_body(lorads_hip_ctx *c, int half, int k, double tol, int maxit) {
    Block &M = c->merged;
    const double *Vfix = half == 0 ? c->V : c->U;
    double *x = half == 0 ? c->U : c->V;
    double *r = c->cr, *p = k == 0 ? c->cr : c->cp, *Q = c->cQ; // p_0 = r_0
    double *pA = part_slot(c, 0), *pC = part_slot(c, 2);
    const Guard g{&c->phase_done[half], half ? &c->phase_done[0] : nullptr};
    const SegArgs sa = seg_args(c, half, k);
    apply_operator(c, M, Vfix, p, OP_CG, nullptr, Q, pA, g);
    LAUNCH(k_cg_update_seg, c->seg_nvt, sa, pA, x, r, p, Q, pC, g);
    M.t_uv_valid = false;
    for (auto &B0 : c->blk) B0.t_uv_valid = false;
    if (seg_carry(c)) { // the test waits for the next operator kernel (batched_tail), or for flush_segchk
        c->pend.post_segchk(Pending::SegChk{true, half, k, pC, tol, maxit});
        return;
    }
    SEG_LAUNCH(k_cg_check_seg, sa, (int)CHK_ITER, pC, ds_tol(c, tol), ds_maxit(c, maxit), g);
}
void batched_tail(lorads_hip_ctx *c, int half, int k, double tol, int maxit) {
    Block &M = c->merged;
    const double *Vfix = half == 0 ? c->V : c->U;
    double *x = half == 0 ? c->U : c->V;
    const Guard g{&c->phase_done[half], half ? &c->phase_done[0] : nullptr};
    const SegArgs sa = seg_args(c, half, k);
    // Max-Cut-type merged cone: the direction update is formed by the operator application that follows (k_op_diag, DirArgs)
    const bool fuse = M.diag_only && c->opt.lazy_scalars && c->opt.fuse_dir && c->seg_tile_cone;
    // (iteration k's waiting test rides along with p = r + beta p -- its tolerance and limit are this call's, batched_iters gives an
    // iteration's body and tail the same -- and a riding restart's two scalars, rs_seg, with p = 2 r)
    auto defer_dir = [&](int kind, const double *rs_seg = nullptr) {
        const double *chk_part = kind == DIR_BETA ? c->pend.take_segchk_part(half, k) : (const double *)nullptr;
        c->pend.post_dir(Pending::Dir{kind, c->st, c->cr, c->cp, 0, 0, nullptr, 0, g, true, half, chk_part, tol, maxit, k, rs_seg});
    };
    if (k % 20 != 0 && !fuse) c->pend.flush_segchk(c);
    if (k % 20 == 0) {
        // (the restart recomputes the residual of the cones that are still running: their test comes first -- on the residual pass
        // itself when the test was waiting for an operator kernel anyway, and the restart's two scalars on the operator that follows)
        const bool ride = fuse && seg_carry(c) && c->opt.seg_carry_restart && c->seg_row0;
        if (!(ride && c->pend.segchk_rides_res(half, k))) c->pend.flush_segchk(c);
        // (riding: the residual's partials go to a slot of their own -- the operator kernel that sums them writes slot 0, p.Ap, itself)
        double *p_res = ride ? part_slot(c, 19) : part_slot(c, 0);
        apply_operator(c, M, Vfix, x, OP_RES, c->rhs, c->cr, p_res, g);
        c->pend.flush_segchk(c); // (not taken: cannot happen on this path; kept in order of safety, not of arithmetic)
        if (ride) {
            defer_dir(DIR_RESTART, p_res);
        } else {
            SEG_LAUNCH(k_cg_check_seg, sa, (int)CHK_RESTART, part_slot(c, 0), ds_tol(c, tol), ds_maxit(c, maxit), g);
            if (fuse) defer_dir(DIR_RESTART);
            else LAUNCH(k_cg_dir_seg, c->seg_nvt, sa, (int)DIR_RESTART, c->cr, c->cp, g);
        }
    } else {
        if (fuse) defer_dir(DIR_BETA);
        else LAUNCH(k_cg_dir_seg, c->seg_nvt, sa, (int)DIR_BETA, c->cr, c->cp, g);
    }
}
void batched_iters(lorads_hip_ctx *c, int half, int k0, int k1, double tol, int maxit) {
    for (int k = k0; k < k1; ++k) {
        if (k > k0) batched_tail(c, half, k - 1, tol, maxit);
        batched_body(c, half, k, tol, maxit);
    }
    c->pend.flush_segchk(c); // (the last enqueued iteration's test: the hand-over, the other phase and a resume read the states)
}
// returns the number of lockstep iterations enqueued so far for `phase` (for a later resume)
void enqueue_batched(lorads_hip_ctx *c, int phase, int resume, double rho, double tol, int maxit, int launched[2],
                     bool eval_follows) {
    Block &M = c->merged;
    // Max-Cut-type merged cone with an evaluation at the end of the sweep: what the refresh after the U-solves would store (constrVal,
    // constrValSum) has one reader, the weights of the V-solves' front -- the evaluation overwrites both vectors (Q1).  That front
    // forms U_p . V_p itself and its weights as if the refresh had been stored (W_ADMM_VS): no k_pairdots, no k_cv.
    const bool onfly_front = M.diag_only && M.rc_w > 0 && M.w_uv && c->opt.front_diag && !c->opt.split_front && M.pu.ne > 0;
    bool virt = false;
    for (int half = phase; half < 2; ++half) {
        const double *Vfix = half == 0 ? c->V : c->U;
        double *x = half == 0 ? c->U : c->V;
        if (half == phase && resume >= 0) {
            const int more = std::max(2, std::min(resume, 16));
            if (resume > 0) batched_tail(c, half, resume - 1, tol, maxit);
            const int k1 = std::min(resume + more, maxit);
            batched_iters(c, half, resume, k1, tol, maxit);
            launched[half] = k1;
        } else {
            const Guard front{nullptr, half ? &c->phase_done[0] : nullptr};
            // the start of the cones' solves rides on iteration 0's operator kernel (op_diag) when there is one: its partials of ||r_0||^2
            // then live in a slot of their own -- that kernel writes slot 0 (p.Ap) while its other workgroups still read them
            const int k1 = std::min(std::max(c->spec_b[half], 0), maxit);
            const bool carry_init = k1 > 0 && M.diag_only && seg_carry(c) && c->opt.seg_carry_init && c->seg_row0;
            double *p_rr0 = carry_init ? part_slot(c, 18) : part_slot(c, 0);
            WArgs wa{};
            wa.csum = c->csum; wa.b = c->b; wa.lambda = c->lambda; wa.cv = M.cv; wa.row_idx = M.row_idx_identity ? nullptr : M.row_idx; wa.rho = ds_rho(c, rho);
            if (onfly_front) {
                // Max-Cut-type merged cone: right-hand side AND initial residual of all cones in ONE kernel, the diagonal
                // coefficients formed on the fly (no k_sval, no separate residual pass): same row tiles, same partial slots
                DiagOnFly of{};
                of.on = true; of.wa = wa; of.wmode = (half == 1 && virt) ? W_ADMM_VS : W_ADMM;
                // a dual update that is still waiting rides on the sweep's ungated first kernel, as on a single cone's front (solve_front):
                // every constraint sits in one row of the merged cone, the updated multipliers go to lambda_alt and the vectors swap
                const bool carry_dual = c->pend.dual_rides(front, true) && half == 0 && M.nrow == c->m && c->m > 0 && c->lambda_alt && c->opt.seg_carry_dual;
                if (carry_dual) {
                    of.wa.lambda_out = c->lambda_alt;
                    of.wa.rho_dual = ds_rho_dual(c, c->pend.take_dual());
                }
                spmm_front(c, M, M.pu, Vfix, x, rho, c->rhs, c->cr, p_rr0, part_slot(c, 1), front, of);
                if (carry_dual) std::swap(c->lambda, c->lambda_alt);
            } else {
                sval(c, M.pu, true, W_ADMM, wa, front);
                spmm(c, M, M.pu, Vfix, OP_RHS, nullptr, nullptr, rho, c->rhs, part_slot(c, 1), front);
                apply_operator(c, M, Vfix, x, OP_RES, c->rhs, c->cr, p_rr0, front);
            }
            if (carry_init) { c->pend.flush(c); c->pend.post_seginit(Pending::SegInit{true, half, tol, front, p_rr0, part_slot(c, 1)}); }
            else SEG_LAUNCH(k_cg_init_seg, seg_args(c, half), p_rr0, part_slot(c, 1), ds_tol(c, tol), front);
            batched_iters(c, half, 0, k1, tol, maxit);
            launched[half] = k1;
        }
        // constrVal <- A(sym(U V^T)), constrValSum += new - old for every cone at once
        if (eval_follows && half == 1) { // dead before the evaluation (see enqueue_sweep): keep the pair dots only
            if (M.use_cw) {
                cw(c, M, c->U, c->V, 1.0, M.w_uv, (double *)nullptr, (int)CV_SET, (double *)nullptr,
                   Guard{nullptr, &c->phase_done[half]});
                M.t_uv_valid = true;
            } else if (!M.diag_only && !M.entry_only) {
                pairdots(c, M.pa, c->U, c->V, M.r, M.T, Guard{nullptr, &c->phase_done[half]});
                M.t_uv_valid = true;
            }
        } else if (eval_follows && half == 0 && onfly_front && c->opt.seg_virt) {
            virt = true; // (nothing stored: see above)
        } else {
            constr_val(c, M, c->U, c->V, 1.0, M.cv, CV_DELTA, c->csum, Guard{nullptr, &c->phase_done[half]});
        }
    }
}
#include "graph.inc"

// while a sweep is enqueued the step parameters are referred to by address when the chain may be replayed (see DS)
struct ParMode {
    lorads_hip_ctx *c;
    ParMode(lorads_hip_ctx *c_, bool on) : c(c_) { c->par_mode = on; }
    ~ParMode() { c->par_mode = false; }
};
int run_sweep_batched(lorads_hip_ctx *c, double rho, double tol, int maxit, bool with_eval) {
    int phase = 0, resume = -1, launched[2] = {0, 0};
    bool first_pass = true, any_missed = false;
    // (the lockstep sweep's long chains -- ~200 launches per iteration on cfg4 -- run no faster replayed than enqueued while the
    // GPU works, 0.288 against 0.279 ms per iteration: replayed only on request, LORADS_GRAPH=2)
    const bool graph = c->opt.graph_batched && graph_this_step(c, rho, tol, maxit);
    if (graph && set_step_params(c, rho, tol, maxit)) return 1;
    ParMode pm(c, graph);
    for (;;) {
        // the evaluation rides along speculatively; with sharded cones only in the first pass (see run_sweep)
        const bool eval_now = with_eval && (!c->ar || first_pass);
        auto enq = [&]() -> int {
            enqueue_batched(c, phase, resume, rho, tol, maxit, launched, with_eval);
            if (eval_now && enqueue_eval(c, LORADS_HIP_PAIR_UV, &c->phase_done[1])) return 1;
            return enqueue_publish(c, 0, state_words(c));
        };
        if (graph && first_pass) {
            std::vector<uint64_t> key{2, (uint64_t)with_eval, (uint64_t)maxit};
            if (graph_step(c, key, enq)) return 1;
            // (a replay has not run enqueue_batched: what it would have left in `launched` follows from the speculation)
            launched[0] = std::min(std::max(c->spec_b[0], 0), maxit);
            launched[1] = std::min(std::max(c->spec_b[1], 0), maxit);
        } else if (enq()) return 1;
        if (wait_publish(c)) return 1;
        if (eval_now && c->ar) any_missed = c->h_scal[5] > 0.5;
        first_pass = false;
        bool u_done = true, v_done = true;
        for (int k = 0; k < c->nb; ++k) {
            u_done = u_done && c->h_st[2 * k].done != 0;
            v_done = v_done && c->h_st[2 * k + 1].pad == 1 && c->h_st[2 * k + 1].done != 0;
        }
        if (u_done && v_done) break;
        c->n_resume++;
        c->merged.t_uv_valid = false; // kernels after the miss did not run: recompute
        if (!u_done) { phase = 0; resume = launched[0]; }
        else { phase = 1; resume = c->h_st[1].pad == 1 ? launched[1] : -1; }
    }
    // speculation for the next ADMM iteration: what the slowest cone needed
    for (int half = 0; half < 2; ++half) {
        int mx = 0;
        for (int k = 0; k < c->nb; ++k) {
            const CGState &h = c->h_st[2 * k + half];
            if (h.done != 2) mx = std::max(mx, h.iter);
        }
        c->spec_b_hist[half][c->spec_b_pos % c->opt.spec_window] = mx;
        int mw = 0;
        for (int k = 0; k < c->opt.spec_window; ++k) mw = std::max(mw, c->spec_b_hist[half][k]);
        c->spec_b[half] = mw; // (as in finish_sweep: the largest of the last few sweeps)
        if (half == 1) c->spec_b_pos++;
    }
    if (with_eval && c->ar && any_missed) { // some rank missed: every rank evaluates again, now with finished sweeps
        if (enqueue_eval(c, LORADS_HIP_PAIR_UV, nullptr)) return 1;
        if (read_states(c)) return 1;
    }
    return 0;
}

bool persist_ready(lorads_hip_ctx *c, int maxit);
int run_sweep_persist(lorads_hip_ctx *c, double rho, double tol, int maxit, bool with_eval);
int run_sweep(lorads_hip_ctx *c, double rho, double tol, int maxit, bool with_eval) {
    // every cone of Max-Cut type with separable constraints: the whole iteration is ONE launch (persist.inc)
    if (persist_ready(c, maxit)) { spec_touch(c); return run_sweep_persist(c, rho, tol, maxit, with_eval); }
    persist_touch(c);
    // (no cross-rank sum inside the sweep: with sharded cones the lockstep form works unchanged)
    if (c->has_merged && !opt_no_batch()) { spec_touch(c); return run_sweep_batched(c, rho, tol, maxit, with_eval); }
    int first = 0, resume = -1;
    bool first_pass = true, any_missed = false, front_carried = false; // (front_carried: the hand-over went with the next step's U front)
    const bool graph = graph_this_step(c, rho, tol, maxit);
    if (graph && set_step_params(c, rho, tol, maxit)) return 1;
    ParMode pm(c, graph);
    if (graph || maxit < 1) spec_touch(c); // (a replayed chain has its own front)
    // an admm_step that is enqueued launch by launch: the next step's U front goes behind its hand-over (see spec_front_enqueue)
    const bool spec = with_eval && !graph && spec_front_ok(c);
    for (;;) {
        // With sharded cones the evaluation contains the all-reduce, a collective every rank must enter the same
        // number of times, whatever its own speculation did.  Every rank enters it once in the first pass, and the
        // reduced vector carries one extra word: how many ranks missed.  If any did, every rank finishes its sweep
        // and all enter the collective once more.  No miss anywhere (the common case): one host synchronisation.
        const bool eval_now = with_eval && (!c->ar || first_pass);
        auto enq = [&]() -> int {
            // every stage starts "not finished": a stage whose predecessor misses its speculation must stay
            // blocked (and block its successors) instead of seeing last iteration's done word
            if (first_pass && 2 * c->nb - 1 > TPB) HC(hipMemsetAsync(c->st, 0, sizeof(CGState) * (size_t)(2 * c->nb), c->stream));
            enqueue_sweep(c, first, resume, rho, tol, maxit, with_eval);
            if (eval_now && enqueue_eval(c, LORADS_HIP_PAIR_UV, c->nb ? &c->st[2 * c->nb - 1].done : nullptr)) return 1;
            return enqueue_publish(c, 0, state_words(c), spec && first_pass ? &rho : nullptr, &front_carried);
        };
        if (graph && first_pass) {
            std::vector<uint64_t> key{1, (uint64_t)with_eval, (uint64_t)maxit, (uint64_t)((c->n_sweeps % 32) == 31)};
            if (graph_step(c, key, enq)) return 1;
        } else if (enq()) return 1;
        if (spec && first_pass && !front_carried) spec_front_enqueue(c, rho);
        if (wait_publish(c)) return 1;
        if (eval_now && c->ar) any_missed = c->h_scal[5] > 0.5;
        const int stg = first_unfinished(c, first);
        if (first_pass && c->spec.live && stg >= 0) { c->spec.live = false; ++c->n_spec_blocked; } // (its gate was shut: it wrote nothing)
        first_pass = false;
        if (stg < 0) break;
        first = stg;
        resume = c->h_st[stg].iter;
        c->n_resume++;
        c->merged.t_uv_valid = false;
        for (auto &B : c->blk) { B.t_uv_valid = false; B.w0_ready = false; B.wj_for = nullptr; } // kernels after the miss did not run: recompute
    }
    if (with_eval && c->ar && any_missed) {
        if (enqueue_eval(c, LORADS_HIP_PAIR_UV, nullptr)) return 1;
        if (read_states(c)) return 1;
    }
    c->n_sweeps++;
    return 0;
}

