// options.inc -- every LORADS_* environment switch of the HIP backend: its name, its parse rule (the helper its line calls) and its
// default.  Host-only C++17, no HIP header, no word about lorads_hip_ctx: a plain host compiler builds it alone
// (tests/options_probe.cpp).  A new switch is one field of Options and one line of read_options(); DESIGN.md 8a names its test.
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdlib>

namespace {

// which row outputs of k_front_cw and k_spmm_ell are written through the L2 (store16 in kernels.inc, LORADS_WT_STORES)
enum { WT_R0 = 1, WT_RHS = 2, WT_CONTRIB = 4, WT_CG0 = 8, WT_AVG = 16, WT_OUT = 32, WT_ALL = 63,
       WT_DEFAULT = WT_R0 | WT_RHS | WT_CG0 | WT_AVG }; // (measured at the headline: profiles/r08_write_through_ab.txt)
// the cuts in k_front_cw's chain of dependent loads (see there, LORADS_FRONT_CHAIN)
enum { FC_RAW = 1, FC_LATE = 2, FC_ALL = 3, FC_DEFAULT = FC_ALL }; // (measured at the headline: profiles/r11_front_chain_ab.txt)

inline bool env_on(const char *name) { const char *v = getenv(name); return !(v && v[0] == '0'); } // on unless the value starts with '0' (unset, empty: on)
inline bool env_set(const char *name) { const char *v = getenv(name); return v && v[0] == '1'; }   // off unless the value starts with '1'
inline bool env_present(const char *name) { return getenv(name) != nullptr; }                      // on when the variable is there, whatever it holds ("0", "")
// atoi of the value clamped to [lo, hi]; `unset` when the variable is not there (or, where asked for, empty)
inline int env_int(const char *name, int unset, int lo, int hi, bool empty_is_unset = false) {
    const char *v = getenv(name);
    return (!v || (empty_is_unset && !v[0])) ? unset : std::max(lo, std::min(hi, atoi(v)));
}

// the switches read when a context is created (ctx_init, once, before the first cone is built); nothing writes them afterwards
struct Options {
    bool pad_rank = true; // odd ranks run as the next even rank with a zero column (LORADS_PAD_ODD_RANK=0: as they are)
    bool dev_presolve = true;   // pattern work of the pre-solve on the device (presolve.inc; LORADS_DEV_PRESOLVE=0: host)
    bool presolve_check = false; // LORADS_PRESOLVE_CHECK=1: build every device pattern on the host too and compare
    size_t dev_presolve_min = (size_t)1 << 15; // stored entries below which a pattern is built on the host (LORADS_DEV_PRESOLVE_MIN)
    bool dense_a = true;      // dense constraint matrices stored full (LORADS_NO_DENSE_A: they stay in the sparse structures)
    bool ell = true;          // constraints of (nearly) equal size in a fixed-width layout (LORADS_NO_ELL: CSR)
    bool slot_ell = true;     // fixed-width image of the slot list for k_spmm_ell (LORADS_NO_SLOT_ELL: CSR)
    bool merge = true;        // all cones as ONE block-diagonal cone where the structure allows it (LORADS_NO_MERGE: no merged view)
    int op_cw = -1;           // LORADS_OP_CW: the constraint-wise operator by its own rule (-1), forced off (0) or on (1) (tests / comparisons)
    bool graph = true;                   // LORADS_GRAPH=0: every iteration enqueued launch by launch
    bool graph_batched = false;          // LORADS_GRAPH=2: the lockstep sweep of a merged cone is replayed too
    bool graph_forced = false;           // LORADS_GRAPH=1 or 2: replay whatever the size (default: small cones only, see graph_ok)
    bool persist = true;                 // teams of resident workgroups, one launch per ADMM iteration (LORADS_PERSIST=0: off)
    bool shared_gpu = false;             // LORADS_SHARED_GPU=1: lock file of the device (several processes on one card take turns, see run_sweep_persist)
    bool persist_carry = true;           // the evaluation leaves (C V) for the next iteration's U front (LORADS_PERSIST_CARRY=0: every front gathers)
    bool persist_l2 = true;              // granules / rows of workgroups verified to share an XCD go through its L2 (LORADS_PERSIST_L2=0: always written through)
    int persist_rows = 0;                // LORADS_PERSIST_ROWS=1|2|4: only that many rows per lane group (0: the first that fits; measurements and tests)
    bool persist_linear = false;         // LORADS_PERSIST_MAP=linear: blocks dealt team by team even where every team fits one XCD
    bool lbfgs_team = true;              // setlbfgsHisTwo + LBFGSDirection as one launch of resident workgroups (LORADS_LBFGS_TEAM=0: launch by launch)
    bool alm_sval_direct = true;         // ... and k_alm_update writes the entries' coefficients where Block::sv_direct holds (LORADS_ALM_SVAL_DIRECT=0: k_sval)
    bool alm_fold_cv = true;             // ... where every constraint has one entry the pattern pass does the constraint pass's work (LORADS_ALM_FOLD_CV=0)
    bool alm_fused_tail = true;          // ... and, behind it, shared passes for A(R R^T), q1, q2 and one closing workgroup (LORADS_ALM_FUSED_TAIL=0)
    bool gram = true;         // LORADS_LBFGS_GRAM=0: sharded direction by the sequential recursion, one collective per dot
    bool gram_single = false; // LORADS_LBFGS_GRAM=2: the Gram-form direction on a single GPU as well
    bool entry_bip = true; // single-entry cones with a bipartite entry graph: k_op_entry_bip x 2 (LORADS_ENTRY_BIP=0: k_op_entry)
    bool fuse_dir = true; // Max-Cut-type cones: the direction update inside the operator kernel (LORADS_FUSE_DIR=0: k_cg_dir)
    bool cw_quad = true;  // k_cw with 4 lanes per entry where it applies (LORADS_CW_QUAD=0: 8 lanes)
    bool fuse_eval = true; // single cone on the k_cw path: constraint values and objective partials in one launch (LORADS_FUSE_EVAL=0)
    bool dense_rem = true; // dense GEMM: 1..4 columns beyond the full tiles on plain FMAs instead of a tile of their own (LORADS_DENSE_REM=0)
    bool dense_cache = true; // dense constraint matrices: A_j V kept for the length of a CG solve (LORADS_DENSE_CACHE=0: nd + 1 GEMMs per application)
    bool front_diag = true; // Max-Cut-type cones: the front forms its diagonal coefficients itself, no k_sval (LORADS_FRONT_DIAG=0)
    bool eval_diag = true; // Max-Cut-type cones: k_eval_diag instead of k_average + k_pairdots + k_cv_res (LORADS_EVAL_DIAG=0)
    bool fold_avg = true; // the sweep's last k_cg_update also forms R = (U + V) / 2 (LORADS_FOLD_AVG=0: k_average)
    bool tile_update = true; // Max-Cut-type cones: k_cg_update on the row tiles of k_op_diag (LORADS_TILE_UPDATE=0: grid-stride over the flat vector)
    bool front_lds = true; // k_front_cw parks the first four slot rows in LDS for its second visit (LORADS_FRONT_LDS=0: gathered again)
    bool front_cw = true; // k_front_cw + k_wsum instead of k_sval + k_spmm2<FRONT> + iteration 0's k_cw (LORADS_FRONT_CW=0: the latter)
    bool fuse_cg0 = true; // CG iteration 0 of a front_cw_ok cone: the update inside k_spmm_ell (LORADS_FUSE_CG0=0: k_cg_update)
    // rows per workgroup of k_front_cw and k_spmm_ell (row_deal; LORADS_ROW_DEAL): -1 the rule, 0 always 32 (the launches as they
    // were), 1..32 that many for every cone (tests).  pretend_cus: LORADS_ROW_DEAL_CUS pretends another count of compute units for
    // the rule to deal over than the device's (tests only; 0: the device's own; what holds is lorads_hip_ctx::row_deal_cus)
    int row_deal = -1, pretend_cus = 0;
    // which row outputs of those two kernels are stored through the L2 (WT_* bits, store16 in kernels.inc; LORADS_WT_STORES: a bit
    // mask, 0 = plain stores everywhere; DESIGN.md 4 item 11)
    int wt_stores = WT_DEFAULT;
    // the cuts in the solve front's chain of dependent loads (FC_* bits, k_front_cw; LORADS_FRONT_CHAIN: a bit mask, 0 = the front
    // without them; DESIGN.md 4 item 12)
    int front_chain = FC_DEFAULT;
    // The U front of the NEXT ADMM step, enqueued behind this step's hand-over while the host still waits for it (sweep.inc:
    // spec_front_enqueue / spec_front_adopt).  LORADS_SPEC_FRONT=0: off
    bool spec_front = true;
    // ... and that front's launch carries the step's hand-over as one more workgroup instead of following k_publish_final (sweep.inc:
    // enqueue_publish; k_front_cw's hand-over form).  LORADS_HANDOVER_ON_FRONT=0: two launches
    bool handover_on_front = true;
    int spec_window = 4;                      // sweeps looked back at (LORADS_SPEC_WINDOW, 1 = the previous sweep's count alone)
    bool exact_refresh = false, split_front = false; // test knobs: see constr_by_recurrence, fused_front
    bool lazy_scalars = true; // LORADS_LAZY_SCALARS=0: every scalar step as its own launch
    bool seg_carry_init = true; // (LORADS_SEG_CARRY_INIT=0: k_cg_init_seg as a launch of its own)
    bool seg_virt = true; // Max-Cut-type merged cone, evaluation at the end: the refresh after the U-solves is not stored, the V front forms its weights from U_p.V_p itself (LORADS_SEG_VIRT=0: k_pairdots + k_cv)
    bool seg_carry_dual = true; // a waiting dual update rides on the U front of the merged cone (LORADS_SEG_CARRY_DUAL=0: k_dual_update)
    bool seg_carry_restart = true; // the k % 20 == 0 restart's test and scalars ride on its two operator kernels (LORADS_SEG_CARRY_RESTART=0)
    bool seg_carry = true;    // LORADS_SEG_CARRY=0: k_cg_check_seg after every update of the lockstep sweep
    int trial_chunk = 0;     // stable-set and bisection rounding: at most this many trials per chunk (LORADS_TRIAL_CHUNK=n, tests only: the chunk loop at sizes a test can afford; 0: the chunk rule alone)
    bool bisect_lds = true;  // bisection rounding: a trial's state in the LDS where it fits (LORADS_BISECT_LDS=0: the device-memory slab at every size, the path of cones too large for the LDS)
};

inline Options read_options() {
    Options o;
    o.pad_rank = env_on("LORADS_PAD_ODD_RANK");
    o.dev_presolve = env_on("LORADS_DEV_PRESOLVE");
    o.presolve_check = env_set("LORADS_PRESOLVE_CHECK");
    if (const char *v = getenv("LORADS_DEV_PRESOLVE_MIN")) o.dev_presolve_min = (size_t)std::max(0ll, atoll(v));
    o.dense_a = !env_present("LORADS_NO_DENSE_A");
    o.ell = !env_present("LORADS_NO_ELL");
    o.slot_ell = !env_present("LORADS_NO_SLOT_ELL");
    o.merge = !env_present("LORADS_NO_MERGE");
    if (const char *v = getenv("LORADS_OP_CW")) o.op_cw = v[0] == '1'; // (the empty string forces off)
    if (const char *v = getenv("LORADS_GRAPH")) { o.graph = v[0] != '0'; o.graph_batched = v[0] == '2'; o.graph_forced = v[0] == '1' || v[0] == '2'; }
    o.persist = env_on("LORADS_PERSIST");
    o.shared_gpu = env_set("LORADS_SHARED_GPU");
    o.persist_carry = env_on("LORADS_PERSIST_CARRY");
    o.persist_l2 = env_on("LORADS_PERSIST_L2");
    o.persist_rows = env_int("LORADS_PERSIST_ROWS", 0, INT_MIN, INT_MAX);
    if (const char *v = getenv("LORADS_PERSIST_MAP")) o.persist_linear = v[0] == 'l';
    o.lbfgs_team = env_on("LORADS_LBFGS_TEAM");
    o.alm_sval_direct = env_on("LORADS_ALM_SVAL_DIRECT");
    o.alm_fold_cv = env_on("LORADS_ALM_FOLD_CV");
    o.alm_fused_tail = env_on("LORADS_ALM_FUSED_TAIL");
    if (const char *v = getenv("LORADS_LBFGS_GRAM")) { o.gram = v[0] != '0'; o.gram_single = v[0] == '2'; }
    o.entry_bip = env_on("LORADS_ENTRY_BIP");
    o.fuse_dir = env_on("LORADS_FUSE_DIR");
    o.cw_quad = env_on("LORADS_CW_QUAD");
    o.fuse_eval = env_on("LORADS_FUSE_EVAL");
    o.dense_rem = env_on("LORADS_DENSE_REM");
    o.dense_cache = env_on("LORADS_DENSE_CACHE");
    o.front_diag = env_on("LORADS_FRONT_DIAG");
    o.eval_diag = env_on("LORADS_EVAL_DIAG");
    o.fold_avg = env_on("LORADS_FOLD_AVG");
    o.tile_update = env_on("LORADS_TILE_UPDATE");
    o.front_lds = env_on("LORADS_FRONT_LDS");
    o.front_cw = env_on("LORADS_FRONT_CW");
    o.fuse_cg0 = env_on("LORADS_FUSE_CG0");
    if (const char *v = getenv("LORADS_ROW_DEAL")) o.row_deal = (!v[0] || v[0] == 'a') ? -1 : std::max(0, std::min(32, atoi(v)));
    o.pretend_cus = env_int("LORADS_ROW_DEAL_CUS", 0, 1, INT_MAX);
    o.wt_stores = env_int("LORADS_WT_STORES", WT_DEFAULT, INT_MIN, INT_MAX, true) & WT_ALL;
    o.front_chain = env_int("LORADS_FRONT_CHAIN", FC_DEFAULT, INT_MIN, INT_MAX, true) & FC_ALL;
    o.spec_front = env_on("LORADS_SPEC_FRONT");
    o.handover_on_front = env_on("LORADS_HANDOVER_ON_FRONT");
    o.spec_window = env_int("LORADS_SPEC_WINDOW", 4, 1, 8);
    o.exact_refresh = env_set("LORADS_EXACT_REFRESH");
    o.split_front = env_set("LORADS_SPLIT_FRONT");
    o.lazy_scalars = env_on("LORADS_LAZY_SCALARS");
    o.seg_carry_init = env_on("LORADS_SEG_CARRY_INIT");
    o.seg_virt = env_on("LORADS_SEG_VIRT");
    o.seg_carry_dual = env_on("LORADS_SEG_CARRY_DUAL");
    o.seg_carry_restart = env_on("LORADS_SEG_CARRY_RESTART");
    o.seg_carry = env_on("LORADS_SEG_CARRY");
    o.trial_chunk = env_int("LORADS_TRIAL_CHUNK", 0, 0, INT_MAX);
    o.bisect_lds = env_on("LORADS_BISECT_LDS");
    return o;
}

// the switches read after creation, each at the moment named
inline bool opt_no_batch() { return env_present("LORADS_NO_BATCH"); }      // every sweep: cone by cone although the context has a merged cone
inline bool opt_common_rank() { return env_on("LORADS_COMMON_RANK"); }     // every common_rank call (creation, resize_rank, the spectral rank reduction): 0 leaves each cone its own rank
inline int opt_lanczos_threads(int n) { return env_int("LORADS_LANCZOS_THREADS", n, 1, n); } // every eigen-solve call: at most that many of the call's `n` host threads, at least one
inline int opt_lbfgs_team_np() { return env_int("LORADS_LBFGS_TEAM_NP", 0, INT_MIN, INT_MAX); } // when phase 1's team plan is built: pairs of doubles per thread and vector forced (measurements; 0: the rule)
// once per process, at first use: wall-clock bound in seconds on the wait for a hand-over (0 or less: none)
inline double opt_handover_timeout_s() { static const char *const v = getenv("LORADS_HANDOVER_TIMEOUT_S"); static const double s = v ? atof(v) : 300.0; return s; }
// at each message and in StageTimer: 0 quiet, 1 the messages (the variable is there, whatever it holds), 2 build_block's stage times too (a leading '2')
inline int opt_verbose() { const char *v = getenv("LORADS_HIP_VERBOSE"); return !v ? 0 : (v[0] == '2' ? 2 : 1); }

} // namespace
