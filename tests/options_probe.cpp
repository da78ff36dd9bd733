// options_probe.cpp -- what lorads_amd/csrc/hip/options.inc reads from the environment, one `field=value` line per switch
// (tests/test_options.py compiles this with the host compiler and runs it under chosen environments).
#include <cstdio>

#include "options.inc"

int main() {
    const Options o = read_options();
#define P(field) printf(#field "=%lld\n", (long long)o.field)
    P(pad_rank); P(dev_presolve); P(presolve_check); P(dev_presolve_min);
    P(dense_a); P(ell); P(slot_ell); P(merge); P(op_cw);
    P(graph); P(graph_batched); P(graph_forced);
    P(persist); P(shared_gpu); P(persist_carry); P(persist_l2); P(persist_rows); P(persist_linear);
    P(lbfgs_team); P(alm_sval_direct); P(alm_fold_cv); P(alm_fused_tail); P(gram); P(gram_single);
    P(entry_bip); P(fuse_dir); P(cw_quad); P(fuse_eval); P(dense_rem); P(dense_cache); P(front_diag); P(eval_diag);
    P(fold_avg); P(tile_update); P(front_lds); P(front_cw); P(fuse_cg0);
    P(row_deal); P(pretend_cus); P(wt_stores); P(front_chain);
    P(spec_front); P(handover_on_front); P(spec_window); P(exact_refresh); P(split_front); P(lazy_scalars);
    P(seg_carry_init); P(seg_virt); P(seg_carry_dual); P(seg_carry_restart); P(seg_carry);
    P(trial_chunk); P(bisect_lds);
#undef P
    // the switches read after creation
    printf("no_batch=%d\n", (int)opt_no_batch());
    printf("common_rank=%d\n", (int)opt_common_rank());
    printf("lanczos_threads_of_4=%d\n", opt_lanczos_threads(4));
    printf("lbfgs_team_np=%d\n", opt_lbfgs_team_np());
    printf("handover_timeout_s=%g\n", opt_handover_timeout_s());
    printf("verbose=%d\n", opt_verbose());
    return 0;
}
