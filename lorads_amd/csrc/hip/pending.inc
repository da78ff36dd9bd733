// pending.inc -- the scalar steps that wait for a carrier kernel: what of class Pending (lorads_hip.hip, beside the context)
// needs the context -- posting with LORADS_LAZY_SCALARS=0, k_op_diag's carry, the flush.  Included by sweep.inc behind LAUNCH.
SegArgs seg_args(lorads_hip_ctx *c, int half, int k = 0);
int seg_threads(lorads_hip_ctx *c);
CGState *shadow_of(lorads_hip_ctx *c, CGState *st) { return c->st_shadow + (st - c->st); }
// a per-cone scalar kernel of the lockstep sweep as a launch of its own, one wavefront per cone (not counted in n_launch), and the
// same behind everything that waits
#define SEG_RAW(kern, ...) hipLaunchKernelGGL(kern, dim3(1), dim3(seg_threads(c)), 0, c->stream, __VA_ARGS__)
#define SEG_LAUNCH(kern, ...) do { c->pend.flush(c); SEG_RAW(kern, __VA_ARGS__); } while (0)

void Pending::post_init(lorads_hip_ctx *c, CGState *st, const double *part_rr, int nrr, const double *part_b, int nb, double tol, Guard front) {
    if (c->opt.lazy_scalars) { // rides on the first kernel of iteration 0 if that kernel can carry it (k_op_diag, k_cw, k_wsum)
        init = InitArgs{st, shadow_of(c, st), part_rr, part_b, nrr, nb, ds_tol(c, tol)};
        init_g = front;
    } else {
        LAUNCH(k_cg_init, 1, st, part_rr, nrr, part_b, nb, ds_tol(c, tol), front, shadow_of(c, st));
    }
}
void Pending::post_check(lorads_hip_ctx *c, CGState *st, const double *part, int np, double tol, int maxit, Guard g) {
    if (c->opt.lazy_scalars) { // rides on the next kernel if that kernel can carry it
        chk = Deferred{st, shadow_of(c, st), part, np, ds_maxit(c, maxit), ds_tol(c, tol), g.need};
        chk_g = g;
    } else {
        LAUNCH(k_cg_check, 1, st, (int)CHK_ITER, part, np, ds_tol(c, tol), ds_maxit(c, maxit), g);
    }
}

// k_op_diag carries a direction update of the same solve whose output is this application's input; or the lockstep solves'
// start, on iteration 0's application; or a lockstep test marked for the restart's residual pass
DirArgs Pending::take_on_op_diag(lorads_hip_ctx *c, int mode, const double *xin, const Guard &g, int rows) {
    const bool quiet = !init.st && !chk.st;
    if (dir.kind && quiet && mode == OP_CG && xin == dir.p && g.skip == dir.g.skip && g.need == dir.g.need) {
        const Dir d = std::exchange(dir, Dir{});
        return DirArgs{d.kind, d.r, d.p, d.st, d.rs_part, d.rs_np, d.seg ? c->seg_tile_cone : (const int *)nullptr, d.half,
                       d.seg ? d.chk_part : (const double *)nullptr, (const int4 *)c->seg_tile_info, c->seg_rr_alt, ds_tol(c, d.chk_tol),
                       ds_maxit(c, d.chk_maxit), d.chk_k + 1, d.seg ? d.rs_seg : (const double *)nullptr, (const int *)c->seg_row0, rows};
    }
    if (seginit.on && mode == OP_CG && xin == c->cr && quiet && !dir.kind && g.need == seginit.front.need) { // (DirArgs, kind 0)
        const SegInit pi = std::exchange(seginit, SegInit{});
        return DirArgs{0, nullptr, nullptr, c->st, nullptr, 0, c->seg_tile_cone, pi.half, nullptr, (const int4 *)c->seg_tile_info, c->seg_rr_alt,
                       DS(0.0), DS(0.0), 0, nullptr, (const int *)c->seg_row0, rows, pi.part_rr, pi.part_b, ds_tol(c, pi.tol), c->phase_done};
    }
    if (segchk.on && segchk.ride_res && mode == OP_RES && quiet && !dir.kind) { // (DirArgs, kind 0)
        const SegChk pc = std::exchange(segchk, SegChk{});
        return DirArgs{0, nullptr, nullptr, c->st, nullptr, 0, c->seg_tile_cone, pc.half, pc.part, (const int4 *)c->seg_tile_info, c->seg_rr_alt,
                       ds_tol(c, pc.tol), ds_maxit(c, pc.maxit), pc.k + 1, nullptr, (const int *)c->seg_row0, rows};
    }
    return DirArgs{};
}
void Pending::flush(lorads_hip_ctx *c) {
    const auto dual_update = [&] { hipLaunchKernelGGL(k_dual_update, dim3(nblocks_for((size_t)c->m, TPB)), dim3(TPB), 0, c->stream, c->m, ds_rho_dual(c, dual_rho), c->b, c->csum, c->lambda); };
    if (sep) { // the reduced scalars of separable shards wait for the hand-over (k_publish_sep); anything else first: their own launch
        sep = false;
        hipLaunchKernelGGL(k_sep_commit, dim3(1), dim3(1), 0, c->stream, (const double *)c->sepbuf, c->scal, sep_with_obj, sep_ex);
    }
    if (dual_virtual) { dual_virtual = false; dual_update(); } // k_front_cw has formed its weights from the updated multipliers; nobody has stored them yet
    if (dual) { dual = false; dual_update(); }                 // first: everything else may read the multipliers
    if (seginit.on) { // the lockstep solves' start that no operator kernel has taken
        const SegInit pi = std::exchange(seginit, SegInit{});
        SEG_RAW(k_cg_init_seg, seg_args(c, pi.half), pi.part_rr, pi.part_b, ds_tol(c, pi.tol), pi.front);
    }
    if (init.st) {
        const InitArgs ia = std::exchange(init, InitArgs{});
        hipLaunchKernelGGL(k_cg_init, dim3(1), dim3(TPB), 0, c->stream, ia.st, ia.part_rr, ia.nrr, ia.part_b, ia.nb, ia.tol, init_g, ia.shadow);
    }
    if (chk.st) {
        const Deferred d = take_check(true);
        hipLaunchKernelGGL(k_cg_check, dim3(1), dim3(TPB), 0, c->stream, d.st, (int)CHK_ITER, d.part, d.np, d.tol, d.maxit, chk_g);
    }
    if (dir.kind) { // (after the test: the direction needs its beta)
        const Dir pd = std::exchange(dir, Dir{});
        if (pd.seg) {
            if (pd.chk_part) // the convergence test that was to ride on the next operator kernel: its own launch after all
                SEG_RAW(k_cg_check_seg, seg_args(c, pd.half, pd.chk_k), (int)CHK_ITER, pd.chk_part, ds_tol(c, pd.chk_tol), ds_maxit(c, pd.chk_maxit), pd.g);
            if (pd.rs_seg) // likewise the restart's scalars
                SEG_RAW(k_cg_check_seg, seg_args(c, pd.half, pd.chk_k), (int)CHK_RESTART, pd.rs_seg, ds_tol(c, pd.chk_tol), ds_maxit(c, pd.chk_maxit), pd.g);
            hipLaunchKernelGGL(k_cg_dir_seg, dim3(c->seg_nvt), dim3(TPB), 0, c->stream, seg_args(c, pd.half), pd.kind, (const double *)pd.r, pd.p, pd.g);
        } else {
            hipLaunchKernelGGL(k_cg_dir, dim3(pd.gv), dim3(TPB), 0, c->stream, pd.len, pd.st, pd.kind, (const double *)pd.r, pd.p, pd.g,
                               Deferred{}, pd.rs_part, pd.rs_np);
        }
    }
}
// a convergence test of the lockstep sweep that nothing has carried: its own launch
void Pending::flush_segchk(lorads_hip_ctx *c) {
    if (!segchk.on) return;
    const SegChk pc = std::exchange(segchk, SegChk{});
    const Guard g{&c->phase_done[pc.half], pc.half ? &c->phase_done[0] : nullptr};
    SEG_LAUNCH(k_cg_check_seg, seg_args(c, pc.half, pc.k), (int)CHK_ITER, pc.part, ds_tol(c, pc.tol), ds_maxit(c, pc.maxit), g);
}
