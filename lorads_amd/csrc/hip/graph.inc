// graph.inc -- replay of captured launch chains (hipGraph); included by sweep.inc in front of the sweeps' drivers.
//
// Below n ~ 20000 an ADMM iteration is bound by the host's launch rate, not by the GPU (profiles/r02_size_sweep.txt: 0.114-0.122 ms
// per iteration from n = 2500 to 20000 while the kernels shrink several-fold).  The enqueue of an iteration is a pure function of
// a little host-side state (which scalar steps are waiting for a carrier, which kept constraint values are valid, the speculated
// CG iteration counts, which of the two multiplier vectors is current) -- every decision inside the iteration is taken on the
// device (struct Guard).  So the chain is captured once per such state (hipStreamBeginCapture) and replayed with ONE
// hipGraphLaunch; the values that change from iteration to iteration without changing the chain -- rho, the CG tolerance, the
// iteration limit, the hand-over's sequence number -- live in device memory (struct DS, k_publish's counter).  A replay restores
// the host-side state the captured enqueue left behind.  A speculation miss resumes launch by launch, as before.
// LORADS_GRAPH=0 switches the replay off (tests compare the two bit for bit).
struct MutSnap { // the host-side state an enqueue reads and writes
    Pending pend; // (saved whole; Pending::restore puts back the part an enqueue changes)
    bool virt_refresh, avg_folded, final_pending, stage_clean, merged_t_uv;
    EvalFinalArgs final_args;
    double *lambda, *lambda_alt;
    int ls_np, head;
    std::vector<unsigned char> blk; // per cone: bit 0 t_uv_valid, bit 1 w0_ready
    std::vector<const double *> wj_for; // per cone: the factor its kept dense products belong to
};
struct GraphEntry {
    hipGraphExec_t exec = nullptr;
    MutSnap after;
    long d_matvec = 0;
    unsigned long long d_seq = 0;
};
struct GraphCache {
    std::map<std::vector<uint64_t>, GraphEntry> map;
    std::map<std::vector<uint64_t>, int> seen; // how often a state has come up without a captured chain
    long n_capture = 0, n_replay = 0;
};
void graph_cache_clear(lorads_hip_ctx *c) {
    if (!c->graphs) return;
    for (auto &kv : c->graphs->map)
        if (kv.second.exec) hipGraphExecDestroy(kv.second.exec);
    c->graphs->map.clear();
    c->graphs->seen.clear();
}
void graph_cache_free(lorads_hip_ctx *c) {
    graph_cache_clear(c);
    delete c->graphs;
    c->graphs = nullptr;
}
MutSnap snap_take(const lorads_hip_ctx *c) {
    MutSnap s;
    s.pend = c->pend;
    s.virt_refresh = c->virt_refresh; s.avg_folded = c->avg_folded;
    s.final_pending = c->final_pending; s.stage_clean = c->stage_clean; s.merged_t_uv = c->merged.t_uv_valid;
    s.final_args = c->final_args;
    s.lambda = c->lambda; s.lambda_alt = c->lambda_alt;
    s.ls_np = c->ls_np; s.head = c->head;
    s.blk.resize(c->blk.size());
    for (size_t k = 0; k < c->blk.size(); ++k) s.blk[k] = (unsigned char)((c->blk[k].t_uv_valid ? 1 : 0) | (c->blk[k].w0_ready ? 2 : 0));
    s.wj_for.resize(c->blk.size());
    for (size_t k = 0; k < c->blk.size(); ++k) s.wj_for[k] = c->blk[k].wj_for;
    return s;
}
void snap_put(lorads_hip_ctx *c, const MutSnap &s) {
    c->pend.restore(s.pend);
    c->virt_refresh = s.virt_refresh; c->avg_folded = s.avg_folded;
    c->final_pending = s.final_pending; c->stage_clean = s.stage_clean; c->merged.t_uv_valid = s.merged_t_uv;
    c->final_args = s.final_args;
    c->lambda = s.lambda; c->lambda_alt = s.lambda_alt;
    c->ls_np = s.ls_np; c->head = s.head;
    for (size_t k = 0; k < c->blk.size() && k < s.blk.size(); ++k) {
        c->blk[k].t_uv_valid = (s.blk[k] & 1) != 0;
        c->blk[k].w0_ready = (s.blk[k] & 2) != 0;
        c->blk[k].wj_for = s.wj_for[k];
    }
}
void snap_key(const lorads_hip_ctx *c, const MutSnap &s, std::vector<uint64_t> &key) {
    key.push_back((uint64_t)s.pend.dual_owed_unused() | (uint64_t)s.virt_refresh << 1 | (uint64_t)s.avg_folded << 2 | (uint64_t)s.stage_clean << 3 |
                  (uint64_t)s.merged_t_uv << 4 | (uint64_t)c->has_merged << 5);
    key.push_back((uint64_t)(uintptr_t)s.lambda);
    key.push_back((uint64_t)(uintptr_t)s.lambda_alt);
    key.push_back((uint64_t)s.head);
    for (size_t k = 0; k < c->blk.size(); ++k)
        key.push_back((uint64_t)s.blk[k] | (uint64_t)(uint32_t)c->blk[k].spec[0] << 8 | (uint64_t)(uint32_t)c->blk[k].spec[1] << 32);
    for (size_t k = 0; k < c->blk.size(); ++k)
        if (c->blk[k].dense_a) key.push_back((uint64_t)(uintptr_t)s.wj_for[k]);
    key.push_back((uint64_t)(uint32_t)c->spec_b[0] | (uint64_t)(uint32_t)c->spec_b[1] << 32);
}
// (a profiling window that times operator applications puts events between the launches: launch by launch)
// Default (no LORADS_GRAPH in the environment): only contexts whose factors hold at most 2^18 elements replay -- n = 5000 at r = 40.
// Above that the iteration is bound by its kernels, a replay is no faster than the enqueue it replaces (profiles/r03_size_sweep.txt:
// 0.1048 vs 0.1044 ms at n = 10000) and capturing a chain costs a short run more than it can give back (the driver's 20-step window at
// the headline: 0.128 ms per step with replay, 0.124-0.125 without).
bool graph_ok(const lorads_hip_ctx *c) {
    if (!c->opt.graph || c->graph_capture_failed || (c->prof && c->prof_every < (1 << 20)) || c->ar) return false;
    return c->opt.graph_forced || c->all_elem <= ((size_t)1 << 18);
}

// the step parameters on the device (see DS): one tiny launch, and only for the words that changed
int step_params_mask(const lorads_hip_ctx *c, const double (&v)[4]) {
    int mask = 0;
    for (int k = 0; k < 4; ++k) {
        if (k == 2 && !c->pend.dual_owed()) continue; // (nobody reads it)
        if (!((c->par_valid >> k) & 1) || memcmp(&v[k], &c->par_h[k], sizeof(double)) != 0) mask |= 1 << k;
    }
    return mask;
}
// Replay this step?  A step whose parameters differ from the device's costs one more (tiny, dependent) launch in front of the
// replayed chain; when they change step after step -- the CG tolerance follows the primal infeasibility once that is below 1e-6,
// lorads_admm.c:76 -- the chain is enqueued launch by launch with its parameters by value instead, which is as fast as a replay
// wherever the GPU is the bound (Max-Cut n = 20000: 0.157 ms per iteration against 0.162 with a k_set_par per iteration).
bool graph_this_step(lorads_hip_ctx *c, double rho, double tol, int maxit) {
    if (!graph_ok(c)) return false;
    const double v[3] = {rho, tol, (double)maxit};
    const bool changed = c->par_req_valid && memcmp(v, c->par_req, sizeof(v)) != 0; // (against the previous step's request)
    memcpy(c->par_req, v, sizeof(v));
    c->par_req_valid = true;
    const bool hot = changed && c->par_changed_last;
    c->par_changed_last = changed;
    return !hot;
}
int set_step_params(lorads_hip_ctx *c, double rho, double tol, int maxit) {
    const double v[4] = {rho, tol, c->pend.dual_rho_value(), (double)maxit};
    const int mask = step_params_mask(c, v);
    if (!mask) return 0;
    hipLaunchKernelGGL(k_set_par, dim3(1), dim3(1), 0, c->stream, c->par, v[0], v[1], v[2], v[3], mask);
    for (int k = 0; k < 4; ++k)
        if ((mask >> k) & 1) { c->par_h[k] = v[k]; c->par_valid |= 1 << k; }
    return 0;
}

// Run `enqueue` (which ends in a hand-over kernel, not in a wait) either launch by launch or -- when the host-side state allows --
// as a captured chain: replayed if the same state has been seen before, captured, instantiated and launched otherwise.
// `key` arrives with whatever of the call's own arguments shapes the chain.
template <class F>
int graph_step(lorads_hip_ctx *c, std::vector<uint64_t> &key, F &&enqueue) {
    const MutSnap before = snap_take(c);
    // nothing but a dual update may be waiting when a step is replayed (see Pending; every entry point that reads results has flushed the rest anyway)
    if (!before.pend.at_rest_for_replay() || before.final_pending) return enqueue();
    if (!c->graphs) c->graphs = new GraphCache();
    snap_key(c, before, key);
    auto it = c->graphs->map.find(key);
    if (it != c->graphs->map.end()) {
        const GraphEntry &e = it->second;
        HC(hipGraphLaunch(e.exec, c->stream));
        snap_put(c, e.after);
        c->n_matvec += e.d_matvec;
        c->pub_seq += e.d_seq;
        c->graphs->n_replay++;
        return 0;
    }
    // capturing and instantiating a chain costs about a millisecond: only a state that comes up a second time is worth it (several
    // cones whose speculated CG counts wander independently produce states that never return)
    if (c->graphs->seen.size() >= 4096) c->graphs->seen.clear();
    if (++c->graphs->seen[key] < 2) return enqueue();
    if (c->graphs->map.size() >= 256) graph_cache_clear(c); // (start over)
    const long mv0 = c->n_matvec;
    const unsigned long long seq0 = c->pub_seq;
    auto give_up = [&](hipGraph_t g) { // capture is not available for this chain: launch by launch from now on
        if (g) hipGraphDestroy(g);
        (void)hipGetLastError();
        c->graph_capture_failed = true;
        snap_put(c, before);
        c->n_matvec = mv0;
        c->pub_seq = seq0;
        if (opt_verbose()) fprintf(stderr, "lorads_hip: graph capture failed, launching step by step\n");
        return enqueue();
    };
    if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return give_up(nullptr);
    const int rc = enqueue();
    hipGraph_t g = nullptr;
    const hipError_t e1 = hipStreamEndCapture(c->stream, &g);
    if (rc) { // nothing of the captured chain has run: the host-side state the enqueue advanced goes back with it (as in give_up)
        if (g) hipGraphDestroy(g);
        snap_put(c, before);
        c->n_matvec = mv0;
        c->pub_seq = seq0;
        return rc;
    }
    if (e1 != hipSuccess || !g) return give_up(g);
    GraphEntry ent;
    if (hipGraphInstantiate(&ent.exec, g, nullptr, nullptr, 0) != hipSuccess) return give_up(g);
    hipGraphDestroy(g);
    ent.after = snap_take(c);
    ent.d_matvec = c->n_matvec - mv0;
    ent.d_seq = c->pub_seq - seq0;
    HC(hipGraphLaunch(ent.exec, c->stream));
    c->graphs->map.emplace(key, std::move(ent));
    c->graphs->n_capture++;
    return 0;
}
