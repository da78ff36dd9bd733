// build.inc -- host-side construction of a cone's device image: patterns, adjacency, Gram, operator variants, the merged
// block-diagonal cone, factor allocation (included by lorads_hip.hip inside its anonymous namespace).
// ---- pattern construction (host, once per context)
struct HostPattern {
    std::vector<int> erow, ecol;
    std::vector<int> e_ptr, e_con;
    std::vector<double> e_val;
    std::vector<int> adj_ptr, adj_col, adj_e;
};
#include "presolve.inc"

void unique_positions(const std::vector<std::pair<int, int>> &pos, std::vector<std::pair<int, int>> &uniq,
                      std::vector<int> &index) {
    std::vector<int> order(pos.size());
    for (size_t i = 0; i < pos.size(); ++i) order[i] = (int)i;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        if (pos[a].second != pos[b].second) return pos[a].second < pos[b].second; // by column, then row
        if (pos[a].first != pos[b].first) return pos[a].first < pos[b].first;
        return a < b;
    });
    uniq.clear();
    index.assign(pos.size(), -1);
    for (size_t k = 0; k < order.size(); ++k) {
        int i = order[k];
        if (uniq.empty() || uniq.back() != pos[i]) uniq.push_back(pos[i]);
        index[i] = (int)uniq.size() - 1;
    }
}

void build_adjacency(int n, const std::vector<std::pair<int, int>> &uniq, HostPattern &hp) {
    hp.erow.resize(uniq.size());
    hp.ecol.resize(uniq.size());
    std::vector<int> deg(n + 1, 0);
    for (size_t e = 0; e < uniq.size(); ++e) {
        hp.erow[e] = uniq[e].first;
        hp.ecol[e] = uniq[e].second;
        deg[uniq[e].first + 1]++;
        if (uniq[e].first != uniq[e].second) deg[uniq[e].second + 1]++;
    }
    hp.adj_ptr.assign(n + 1, 0);
    for (int i = 0; i < n; ++i) hp.adj_ptr[i + 1] = hp.adj_ptr[i] + deg[i + 1];
    hp.adj_col.resize(hp.adj_ptr[n]);
    hp.adj_e.resize(hp.adj_ptr[n]);
    std::vector<int> fill(hp.adj_ptr.begin(), hp.adj_ptr.end() - 1);
    for (size_t e = 0; e < uniq.size(); ++e) {
        int p = uniq[e].first, q = uniq[e].second;
        hp.adj_col[fill[p]] = q; hp.adj_e[fill[p]] = (int)e; fill[p]++;
        if (p != q) { hp.adj_col[fill[q]] = p; hp.adj_e[fill[q]] = (int)e; fill[q]++; }
    }
    // neighbours in ascending row order: fixed summation order and better locality
    for (int i = 0; i < n; ++i) {
        int s = hp.adj_ptr[i], t = hp.adj_ptr[i + 1];
        std::vector<std::pair<int, int>> tmp(t - s);
        for (int k = s; k < t; ++k) tmp[k - s] = {hp.adj_col[k], hp.adj_e[k]};
        std::sort(tmp.begin(), tmp.end());
        for (int k = s; k < t; ++k) { hp.adj_col[k] = tmp[k - s].first; hp.adj_e[k] = tmp[k - s].second; }
    }
}

// transpose of the constraint CSR over pattern entries
void build_transpose(int ne, int nrow, const int *a_ptr, const std::vector<int> &a_e, const double *a_val, HostPattern &hp) {
    hp.e_ptr.assign(ne + 1, 0);
    int na = a_ptr[nrow];
    for (int t = 0; t < na; ++t) hp.e_ptr[a_e[t] + 1]++;
    for (int e = 0; e < ne; ++e) hp.e_ptr[e + 1] += hp.e_ptr[e];
    hp.e_con.resize(na);
    hp.e_val.resize(na);
    std::vector<int> fill(hp.e_ptr.begin(), hp.e_ptr.end() - 1);
    for (int i = 0; i < nrow; ++i)
        for (int t = a_ptr[i]; t < a_ptr[i + 1]; ++t) {
            int e = a_e[t];
            hp.e_con[fill[e]] = i;
            hp.e_val[fill[e]] = a_val[t];
            fill[e]++;
        }
}

int upload_pattern(DevPool &M, Pattern &P, const HostPattern &hp, const std::vector<double> *cbase) {
    P.ne = (int)hp.erow.size();
    if (M.upload(&P.erow, hp.erow) || M.upload(&P.ecol, hp.ecol) || M.upload(&P.e_ptr, hp.e_ptr) || M.upload(&P.e_con, hp.e_con) ||
        M.upload(&P.e_val, hp.e_val) || M.upload(&P.adj_ptr, hp.adj_ptr) || M.upload(&P.adj_col, hp.adj_col) ||
        M.upload(&P.adj_e, hp.adj_e))
        return 1;
    if (M.alloc(&P.S, (size_t)P.ne)) return 1;
    if (cbase && M.upload(&P.cbase, *cbase)) return 1;
    { // one (entry, constraint) pair per constraint marked as the constraint's owner (see WArgs::lambda_out)
        int nrow = 0;
        for (int i : hp.e_con) nrow = std::max(nrow, i + 1);
        std::vector<char> seen((size_t)nrow, 0);
        std::vector<int> own(hp.e_con);
        int marked = 0;
        for (size_t t = 0; t < own.size(); ++t)
            if (!seen[own[t]]) { seen[own[t]] = 1; own[t] |= (int)0x80000000; ++marked; }
        P.n_owned = marked;
        if (M.upload(&P.e_con_own, own)) return 1;
    }
    // per slot: is the entry's coefficient static (no constraint touches it: C alone) or does it change with the weights
    P.nslot = (int)hp.adj_e.size();
    std::vector<int> dyn(hp.adj_e.size());
    std::vector<double> sval(hp.adj_e.size(), 0.0);
    for (size_t k = 0; k < hp.adj_e.size(); ++k) {
        const int e = hp.adj_e[k];
        sval[k] = cbase ? (*cbase)[e] : 0.0; // (the objective's part of every slot: read for static slots, and by the on-the-fly front of Max-Cut-type cones for the others too)
        dyn[k] = hp.e_ptr[e + 1] > hp.e_ptr[e] ? e : -1;
    }
    if (M.upload(&P.adj_dyn, dyn) || M.upload(&P.adj_sval, sval)) return 1;
    return 0;
}

// G = A A^T over pattern entries, when sum_i nnz_i^2 stays small
int build_gram(DevPool &M, Block &B, const lorads_hip_block &hb, const std::vector<int> &a_e, int ne) {
    double tot = 0;
    for (int i = 0; i < hb.nrow; ++i) { double k = hb.a_ptr[i + 1] - hb.a_ptr[i]; tot += k * k; }
    if (tot > std::max(64.0 * B.na, 1.0e6) || tot > 2.0e8) return 0;
    std::vector<std::pair<uint64_t, double>> tri;
    tri.reserve((size_t)tot);
    for (int i = 0; i < hb.nrow; ++i)
        for (int t1 = hb.a_ptr[i]; t1 < hb.a_ptr[i + 1]; ++t1)
            for (int t2 = hb.a_ptr[i]; t2 < hb.a_ptr[i + 1]; ++t2)
                tri.push_back({((uint64_t)a_e[t1] << 32) | (uint32_t)a_e[t2], hb.a_val[t1] * hb.a_val[t2]});
    std::stable_sort(tri.begin(), tri.end(), [](const std::pair<uint64_t, double> &x, const std::pair<uint64_t, double> &y) {
        return x.first < y.first;
    });
    std::vector<int> g_ptr(ne + 1, 0), g_col;
    std::vector<double> g_val;
    for (size_t k = 0; k < tri.size(); ++k) {
        if (k > 0 && tri[k].first == tri[k - 1].first) { g_val.back() += tri[k].second; continue; }
        g_col.push_back((int)(tri[k].first & 0xffffffffu));
        g_val.push_back(tri[k].second);
        g_ptr[(int)(tri[k].first >> 32) + 1]++;
    }
    for (int e = 0; e < ne; ++e) g_ptr[e + 1] += g_ptr[e];
    if (M.upload(&B.g_ptr, g_ptr) || M.upload(&B.g_col, g_col) || M.upload(&B.g_val, g_val)) return 1;
    B.has_gram = true;
    return 0;
}

// stage timing of build_block (LORADS_HIP_VERBOSE=2)
struct StageTimer {
    bool on;
    std::chrono::steady_clock::time_point t0;
    StageTimer() : on(opt_verbose() == 2), t0(std::chrono::steady_clock::now()) {}
    void lap(const char *what) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "lorads_hip:   build %-34s %8.2f ms\n", what, 1e3 * std::chrono::duration<double>(t1 - t0).count());
        t0 = t1;
    }
};
// One sparsity pattern: unique positions, the entry -> position map, adjacency, transpose of the constraint CSR (entries [0, na)
// of `pos` are the constraints' in CSR order).  On the device above LORADS_DEV_PRESOLVE_MIN stored entries (presolve.inc), on the
// host below; LORADS_PRESOLVE_CHECK=1 builds both and refuses any difference.
int make_pattern(lorads_hip_ctx *c, const std::vector<std::pair<int, int>> &pos, int dim, int nrow, const int *a_ptr, int na,
                 const double *a_val, std::vector<std::pair<int, int>> &uniq, std::vector<int> &index, HostPattern &hp, StageTimer &tm,
                 const char *what) {
    bool dev = c->opt.dev_presolve && pos.size() >= c->opt.dev_presolve_min && dim > 0 && pos.size() <= (size_t)INT32_MAX / 2;
    if (dev) {
        if (dev_pattern(c, pos, dim, nrow, a_ptr, na, a_val, uniq, index, hp)) {
            // (no room for the sorts' scratch next to a problem that fills the HBM, or a failed launch: the host builds the same arrays)
            (void)hipGetLastError();
            g_err.clear();
            uniq.clear(); index.clear(); hp = HostPattern{};
            dev = false;
            tm.lap((std::string(what) + " (device pre-solve gave up: host construction)").c_str());
        } else {
            c->n_dev_patterns++;
            tm.lap((std::string(what) + " (device: unique, adjacency, transpose)").c_str());
            if (!c->opt.presolve_check) return 0;
        }
    }
    std::vector<std::pair<int, int>> uniq_h;
    std::vector<int> index_h;
    HostPattern hp_h;
    unique_positions(pos, uniq_h, index_h);
    build_adjacency(dim, uniq_h, hp_h);
    std::vector<int> a_e(index_h.begin(), index_h.begin() + na);
    build_transpose((int)uniq_h.size(), nrow, a_ptr, a_e, a_val, hp_h);
    tm.lap((std::string(what) + " (host: unique, adjacency, transpose)").c_str());
    if (dev) {
        c->n_checked_patterns++;
        if (uniq != uniq_h || index != index_h || hp.erow != hp_h.erow || hp.ecol != hp_h.ecol || hp.e_ptr != hp_h.e_ptr || hp.e_con != hp_h.e_con ||
            hp.e_val != hp_h.e_val || hp.adj_ptr != hp_h.adj_ptr || hp.adj_col != hp_h.adj_col || hp.adj_e != hp_h.adj_e)
            return fail_msg(std::string("device pre-solve: ") + what + " differs from the host construction");
        return 0;
    }
    uniq.swap(uniq_h); index.swap(index_h);
    hp = std::move(hp_h);
    return 0;
}
int build_block(lorads_hip_ctx *c, Block &B, const lorads_hip_block &hb_in) {
    StageTimer tm;
    DevPool &M = c->mem;
    // Dense constraint matrices first (the reference's rule for a dense coefficient, data/lorads_sdp_data.c:820): they leave the
    // sparse structures -- the rest of this function sees their rows of the constraint CSR empty -- and are stored full.
    lorads_hip_block hbf = hb_in;
    std::vector<int> f_ptr, f_row, f_col, dcon;
    std::vector<double> f_val;
    // The dense store only where it pays.  The reference's rule alone (nnz > 0.1 n(n+1)/2) calls almost every constraint of a SMALL
    // cone dense (n <= 3: any entry; n = 10: six entries), and each would get a 64 x 64 matrix of its own, three launches per operator
    // application, and switch the cone's fast paths off: below n = 32 -- and when the matrices would not fit 8 GB -- such constraints
    // stay in the sparse structures (same sums in another order).
    if (!hb_in.is_lp && hb_in.n >= 32) {
        const double thr = 0.1 * (double)((int64_t)hb_in.n * (hb_in.n + 1) / 2);
        for (int i = 0; i < hb_in.nrow; ++i)
            if ((double)(hb_in.a_ptr[i + 1] - hb_in.a_ptr[i]) > thr) dcon.push_back(i);
        const double npad_d = (double)((hb_in.n + 63) / 64 * 64);
        if ((double)dcon.size() * npad_d * npad_d * 8.0 > 8e9) dcon.clear();
    }
    if (!dcon.empty() && c->opt.dense_a) {
        const int npad = (hb_in.n + 63) / 64 * 64;
        std::vector<double> ad((size_t)dcon.size() * npad * npad, 0.0);
        std::vector<char> isd((size_t)hb_in.nrow, 0);
        for (size_t j = 0; j < dcon.size(); ++j) {
            const int i = dcon[j];
            isd[i] = 1;
            double *M = ad.data() + j * (size_t)npad * npad;
            for (int t = hb_in.a_ptr[i]; t < hb_in.a_ptr[i + 1]; ++t) {
                const int p = hb_in.a_row[t], q = hb_in.a_col[t];
                if (p < q || q < 0 || p >= hb_in.n) return fail_msg("A entry out of range / not lower-triangular");
                M[(size_t)p * npad + q] += hb_in.a_val[t];
                if (p != q) M[(size_t)q * npad + p] += hb_in.a_val[t];
            }
        }
        f_ptr.assign(1, 0);
        for (int i = 0; i < hb_in.nrow; ++i) {
            if (!isd[i])
                for (int t = hb_in.a_ptr[i]; t < hb_in.a_ptr[i + 1]; ++t) {
                    f_row.push_back(hb_in.a_row[t]); f_col.push_back(hb_in.a_col[t]); f_val.push_back(hb_in.a_val[t]);
                }
            f_ptr.push_back((int)f_row.size());
        }
        hbf.a_ptr = f_ptr.data(); hbf.a_row = f_row.data(); hbf.a_col = f_col.data(); hbf.a_val = f_val.data();
        if (M.upload(&B.d_con, dcon) || M.upload(&B.Adense, ad) || M.alloc(&B.Sfull, (size_t)npad * npad) || M.alloc(&B.d_mu, dcon.size())) return 1;
        B.dense_a = true;
        B.nd = (int)dcon.size();
        B.d_con_h = dcon;
    }
    const lorads_hip_block &hb = hbf;
    B.n = hb.n; B.rl = hb.rank; B.r = dev_rank(c, hb.rank, hb.is_lp != 0); B.nrow = hb.nrow; B.na = hb.a_ptr[hb.nrow]; B.nc = hb.c_nnz;
    if (B.r > 512) return fail_msg("rank > 512 is not supported by the row kernels");
    if (nblocks_for((size_t)B.n, TPB / lg_for(B.r)) > c->maxpart)
        return fail_msg("cone dimension too large for the partial-sum slots of this build");
    std::vector<std::pair<int, int>> posA(B.na), posU;
    for (int t = 0; t < B.na; ++t) {
        if (hb.a_row[t] < hb.a_col[t] || hb.a_col[t] < 0 || hb.a_row[t] >= hb.n) return fail_msg("A entry out of range / not lower-triangular");
        posA[t] = {hb.a_row[t], hb.a_col[t]};
    }
    for (int t = 0; t < B.nc; ++t)
        if (hb.c_row[t] < hb.c_col[t] || hb.c_col[t] < 0 || hb.c_row[t] >= hb.n) return fail_msg("C entry out of range / not lower-triangular");
    for (int i = 0; i < hb.nrow; ++i)
        if (hb.row_idx[i] < 0 || hb.row_idx[i] >= c->m) return fail_msg("constraint index out of range");
    // A-pattern
    std::vector<std::pair<int, int>> uniqA;
    std::vector<int> a_e;
    HostPattern hpA;
    if (make_pattern(c, posA, B.n, hb.nrow, hb.a_ptr, B.na, hb.a_val, uniqA, a_e, hpA, tm, "A-pattern")) return 1;
    if (upload_pattern(M, B.pa, hpA, nullptr)) return 1;
    tm.lap("upload A-pattern");
    // dense objective (the reference's rule for a dense coefficient, lorads_sdp_data.c:818-821)
    B.dense_c = !hb.is_lp && (double)B.nc > 0.1 * (double)((int64_t)B.n * (B.n + 1) / 2);
    if (B.dense_c || B.dense_a) {
        B.npad = (B.n + 63) / 64 * 64;
        // k_dense_cx_b: workgroups of 32 output rows, four wavefronts each on a quarter of the workgroup's K range
        // (a multiple of 16 rows per wavefront); K is split over workgroups until the grid holds >= 512 of them
        if (B.npad % 64 == 0) {
            B.ksplit_b = 1;
            while (B.ksplit_b < 16 && (B.npad / 32) * B.ksplit_b < 512 && (B.npad / (2 * B.ksplit_b)) % 64 == 0) B.ksplit_b *= 2;
            if ((B.npad / B.ksplit_b) % 64 != 0) B.ksplit_b = 0;
        }
        if (B.dense_c) {
            std::vector<double> cf((size_t)B.npad * B.npad, 0.0);
            for (int t = 0; t < B.nc; ++t) {
                cf[(size_t)hb.c_row[t] * B.npad + hb.c_col[t]] += hb.c_val[t];
                if (hb.c_row[t] != hb.c_col[t]) cf[(size_t)hb.c_col[t] * B.npad + hb.c_row[t]] += hb.c_val[t];
            }
            if (M.upload(&B.Cfull, cf)) return 1;
        }
    }
    // union pattern C u A (A only when C is dense: the dense part is added by k_dense_cx)
    posU = posA;
    for (int t = 0; t < B.nc && !B.dense_c; ++t) posU.push_back({hb.c_row[t], hb.c_col[t]});
    std::vector<std::pair<int, int>> uniqU;
    std::vector<int> u_idx;
    HostPattern hpU;
    if (make_pattern(c, posU, B.n, hb.nrow, hb.a_ptr, B.na, hb.a_val, uniqU, u_idx, hpU, tm, "union pattern")) return 1;
    std::vector<double> cbase(uniqU.size(), 0.0);
    for (int t = 0; t < B.nc && !B.dense_c; ++t) cbase[u_idx[B.na + t]] += hb.c_val[t];
    if (upload_pattern(M, B.pu, hpU, &cbase)) return 1;
    tm.lap("upload union pattern");
    { // constraint -> its entries of the union pattern, where every touched entry belongs to one constraint (Block::sv_direct)
        bool direct = hb.nrow > 0 && !B.dense_c && !hpU.e_ptr.empty();
        for (size_t e = 0; e + 1 < hpU.e_ptr.size() && direct; ++e) direct = hpU.e_ptr[e + 1] - hpU.e_ptr[e] <= 1;
        if (direct) {
            std::vector<int> cnt((size_t)hb.nrow + 1, 0);
            for (int i : hpU.e_con) ++cnt[(size_t)i + 1];
            for (int i = 0; i < hb.nrow; ++i) cnt[(size_t)i + 1] += cnt[i];
            std::vector<int> se(hpU.e_con.size());
            std::vector<double> sa(hpU.e_con.size());
            std::vector<int> fill(cnt.begin(), cnt.end() - 1);
            for (size_t e = 0; e + 1 < hpU.e_ptr.size(); ++e)
                for (int t = hpU.e_ptr[e]; t < hpU.e_ptr[e + 1]; ++t) {
                    const int i = hpU.e_con[t], k = fill[i]++;
                    se[k] = (int)e;
                    sa[k] = hpU.e_val[t];
                }
            if (M.upload(&B.sv_ptr, cnt) || M.upload(&B.sv_e, se) || M.upload(&B.sv_a, sa)) return 1;
            // (entries no constraint touches are never written by that path and never read through Pattern::adj_dyn; they hold C all the same)
            HC(hipMemcpy(B.pu.S, B.pu.cbase, sizeof(double) * (size_t)B.pu.ne, hipMemcpyDeviceToDevice));
        }
        B.sv_direct = direct;
    }
    // constraint CSR + misc
    std::vector<int> v_rowidx(hb.row_idx, hb.row_idx + hb.nrow), v_aptr(hb.a_ptr, hb.a_ptr + hb.nrow + 1);
    B.row_idx_identity = hb.nrow > 0;
    for (int i = 0; i < hb.nrow && B.row_idx_identity; ++i) B.row_idx_identity = hb.row_idx[i] == i;
    std::vector<double> v_aval(hb.a_val, hb.a_val + B.na), v_cval(hb.c_val, hb.c_val + B.nc);
    std::vector<int> v_crow(hb.c_row, hb.c_row + B.nc), v_ccol(hb.c_col, hb.c_col + B.nc);
    if (M.upload(&B.row_idx, v_rowidx) || M.upload(&B.a_ptr, v_aptr) || M.upload(&B.a_e, a_e) || M.upload(&B.a_val, v_aval) ||
        M.upload(&B.c_row, v_crow) || M.upload(&B.c_col, v_ccol) || M.upload(&B.c_val, v_cval))
        return 1;
    if (M.alloc(&B.T, (size_t)B.pa.ne) || M.alloc(&B.T2, (size_t)B.pa.ne) || M.alloc(&B.cv, (size_t)B.nrow) || M.alloc(&B.wtmp, (size_t)B.nrow)) return 1;
    HC(hipMemset(B.cv, 0, sizeof(double) * (size_t)std::max(B.nrow, 1)));
    // Max-Cut fast path
    bool diag = B.nrow > 0 && !B.dense_a; // (a cone with dense constraint matrices takes the general path everywhere)
    std::vector<double> gd(B.n, 0.0);
    for (int i = 0; i < hb.nrow && diag; ++i) {
        if (hb.a_ptr[i + 1] - hb.a_ptr[i] != 1) { diag = false; break; }
        int t = hb.a_ptr[i];
        if (hb.a_row[t] != hb.a_col[t]) { diag = false; break; }
        gd[hb.a_row[t]] += hb.a_val[t] * hb.a_val[t];
    }
    B.diag_only = diag;
    if (diag && M.upload(&B.gdiag, gd)) return 1;
    if (diag) { // per constraint (row, coefficient) and the two row-dot vectors of constr_by_recurrence
        std::vector<int> drow(hb.nrow);
        std::vector<double> dav(hb.nrow);
        for (int i = 0; i < hb.nrow; ++i) { drow[i] = hb.a_row[hb.a_ptr[i]]; dav[i] = hb.a_val[hb.a_ptr[i]]; }
        if (M.upload(&B.diag_row, drow) || M.upload(&B.diag_a, dav) || M.alloc(&B.w_uv, (size_t)B.n) || M.alloc(&B.w_op, (size_t)B.n)) return 1;
        { // row -> its constraints in fixed width (k_eval_diag); Max-Cut: exactly one per row
            std::vector<int> cntr(B.n, 0);
            for (int i = 0; i < hb.nrow; ++i) cntr[drow[i]]++;
            int w = 1;
            for (int p = 0; p < B.n; ++p) w = std::max(w, cntr[p]);
            if (w <= 8) {
                std::vector<int> rc((size_t)B.n * w, -1), fillr(B.n, 0);
                for (int i = 0; i < hb.nrow; ++i) rc[(size_t)drow[i] * w + fillr[drow[i]]++] = i;
                if (M.upload(&B.rc_con, rc)) return 1;
                B.rc_w = w;
            }
        }
    }
    bool single_entry = !diag && B.nrow > 0 && !B.dense_a;
    for (int i = 0; i < hb.nrow && single_entry; ++i) single_entry = hb.a_ptr[i + 1] - hb.a_ptr[i] == 1;
    if (single_entry) {
        std::vector<double> gev((size_t)B.pa.ne, 0.0);
        for (int i = 0; i < hb.nrow; ++i) gev[a_e[hb.a_ptr[i]]] += hb.a_val[hb.a_ptr[i]] * hb.a_val[hb.a_ptr[i]];
        if (M.upload(&B.gentry, gev)) return 1;
        B.entry_only = true;
        // two-colouring of the entry graph (matrix completion: left factor rows / right factor rows); colour 0 = the side that forms
        // the pair dots, isolated rows included.  Not bipartite (an odd cycle): the one-kernel form stays.
        std::vector<int> colour(B.n, -1), stack;
        bool bip = true;
        for (int s0 = 0; s0 < B.n && bip; ++s0) {
            if (colour[s0] >= 0) continue;
            colour[s0] = 0;
            stack.push_back(s0);
            while (!stack.empty() && bip) {
                const int p = stack.back();
                stack.pop_back();
                for (int t = hpA.adj_ptr[p]; t < hpA.adj_ptr[p + 1]; ++t) {
                    const int q = hpA.adj_col[t];
                    if (q == p) continue;
                    if (colour[q] < 0) { colour[q] = 1 - colour[p]; stack.push_back(q); }
                    else if (colour[q] == colour[p]) { bip = false; break; }
                }
            }
        }
        if (bip) {
            std::vector<int> rows[2];
            for (int p = 0; p < B.n; ++p) rows[colour[p]].push_back(p);
            if (!rows[1].empty()) {
                if (M.upload(&B.bip_rows[0], rows[0]) || M.upload(&B.bip_rows[1], rows[1]) || M.alloc(&B.bip_we, (size_t)std::max(B.pa.ne, 1))) return 1;
                B.bip_n[0] = (int)rows[0].size();
                B.bip_n[1] = (int)rows[1].size();
            }
        }
    }
    tm.lap("operator kind (diag / single entry / colouring)");
    if (!diag && !B.dense_a && build_gram(M, B, hb, a_e, B.pa.ne)) return 1;
    tm.lap("Gram");
    // Constraint-wise operator (k_cw + k_spmm<CW>): worthwhile when there are enough constraints to fill the device
    // with one wavefront each and none of them is so large that a single wavefront would crawl through it.
    {
        int maxsz = 0;
        for (int i = 0; i < hb.nrow; ++i) maxsz = std::max(maxsz, hb.a_ptr[i + 1] - hb.a_ptr[i]);
        bool want = !diag && !B.entry_only && hb.nrow >= 256 && maxsz <= 512;
        if (c->opt.op_cw >= 0 && !diag && !B.entry_only && hb.nrow > 0) want = c->opt.op_cw == 1; // (forced: tests / comparisons)
        if (B.dense_a) want = false;
        if (want) {
            std::vector<int> deg(B.n + 1, 0);
            for (int t = 0; t < B.na; ++t) {
                deg[hb.a_row[t] + 1]++;
                if (hb.a_row[t] != hb.a_col[t]) deg[hb.a_col[t] + 1]++;
            }
            std::vector<int> ptr(B.n + 1, 0);
            for (int i = 0; i < B.n; ++i) ptr[i + 1] = ptr[i] + deg[i + 1];
            std::vector<int> col(ptr[B.n]), con(ptr[B.n]), fill(ptr.begin(), ptr.end() - 1);
            std::vector<double> av(ptr[B.n]);
            for (int i = 0; i < hb.nrow; ++i)
                for (int t = hb.a_ptr[i]; t < hb.a_ptr[i + 1]; ++t) {
                    const int p = hb.a_row[t], q = hb.a_col[t];
                    col[fill[p]] = q; con[fill[p]] = i; av[fill[p]] = hb.a_val[t]; fill[p]++;
                    if (p != q) { col[fill[q]] = p; con[fill[q]] = i; av[fill[q]] = hb.a_val[t]; fill[q]++; }
                }
            for (int i = 0; i < B.n; ++i) { // neighbours in ascending (row, constraint) order: fixed summation order
                const int s0 = ptr[i], s1 = ptr[i + 1];
                std::vector<std::tuple<int, int, double>> tmp(s1 - s0);
                for (int k = s0; k < s1; ++k) tmp[k - s0] = std::make_tuple(col[k], con[k], av[k]);
                std::sort(tmp.begin(), tmp.end());
                for (int k = s0; k < s1; ++k) { col[k] = std::get<0>(tmp[k - s0]); con[k] = std::get<1>(tmp[k - s0]); av[k] = std::get<2>(tmp[k - s0]); }
            }
            std::vector<int> car(hb.a_row, hb.a_row + B.na), cac(hb.a_col, hb.a_col + B.na);
            std::vector<double> cav(hb.a_val, hb.a_val + B.na);
            if (maxsz <= 32 && (double)hb.nrow * maxsz <= 1.5 * (double)B.na && c->opt.ell) {
                // constraints of (nearly) equal size: fixed-width layout, padding = (row 0, row 0, 0.0)
                B.ca_ell = maxsz;
                car.assign((size_t)hb.nrow * maxsz, 0); cac.assign((size_t)hb.nrow * maxsz, 0); cav.assign((size_t)hb.nrow * maxsz, 0.0);
                for (int i = 0; i < hb.nrow; ++i)
                    for (int t = hb.a_ptr[i]; t < hb.a_ptr[i + 1]; ++t) {
                        const size_t w = (size_t)i * maxsz + (size_t)(t - hb.a_ptr[i]);
                        car[w] = hb.a_row[t]; cac[w] = hb.a_col[t]; cav[w] = hb.a_val[t];
                    }
            }
            // fixed-width image of the slot list for k_spmm_ell: 8 slots per row when (almost) every row fits, else 16
            if (c->opt.slot_ell) {
                long over8 = 0;
                for (int i = 0; i < B.n; ++i) over8 += (ptr[i + 1] - ptr[i]) > 8;
                const int ew = (double)over8 <= 0.005 * (double)B.n ? 8 : 16;
                std::vector<int> ecol((size_t)B.n * ew), econ((size_t)B.n * ew, 0);
                std::vector<double> eav((size_t)B.n * ew, 0.0);
                for (int i = 0; i < B.n; ++i)
                    for (int s = 0; s < ew; ++s) {
                        const int k = ptr[i] + s;
                        const size_t w = (size_t)i * ew + s;
                        if (k < ptr[i + 1]) { ecol[w] = col[k]; econ[w] = con[k]; eav[w] = av[k]; }
                        else ecol[w] = i; // padding: the row itself, coefficient 0
                    }
                if (M.upload(&B.cell_col, ecol) || M.upload(&B.cell_con, econ) || M.upload(&B.cell_a, eav)) return 1;
                B.cell_w = ew;
            }
            for (int i = 0; i < B.n; ++i) B.cell_over += (ptr[i + 1] - ptr[i]) > B.cell_w;
            if (B.cell_w && !B.dense_c) {
                // k_front_cw: the objective's own adjacency (both orientations, duplicates summed, neighbours ascending) ...
                std::vector<std::pair<int, int>> posC(B.nc), uniqC;
                for (int t = 0; t < B.nc; ++t) posC[t] = {hb.c_row[t], hb.c_col[t]};
                std::vector<int> cidx;
                unique_positions(posC, uniqC, cidx);
                std::vector<double> cval(uniqC.size(), 0.0);
                for (int t = 0; t < B.nc; ++t) cval[cidx[t]] += hb.c_val[t];
                HostPattern hpC;
                build_adjacency(B.n, uniqC, hpC);
                std::vector<double> fval(hpC.adj_e.size());
                for (size_t k = 0; k < hpC.adj_e.size(); ++k) fval[k] = cval[hpC.adj_e[k]];
                // ... and for every slot its place in the contribution array: constraint-major, fixed width (the constraint's
                // slots in ascending order of their CSR position = k_wsum's fixed order of summation); padding stays zero
                std::vector<int> ccount(hb.nrow, 0);
                for (int k = 0; k < ptr[B.n]; ++k) ccount[con[k]]++;
                int csw = 1;
                for (int i = 0; i < hb.nrow; ++i) csw = std::max(csw, ccount[i]);
                if ((double)hb.nrow * csw > 4.0 * (double)ptr[B.n] + 1024.0) csw = 0; // (a few huge constraints: keep the older front)
                if (csw > 0) {
                    std::vector<int> dstc(ptr[B.n]), fillc(hb.nrow, 0), dste((size_t)B.n * B.cell_w, 0);
                    for (int k = 0; k < ptr[B.n]; ++k) dstc[k] = con[k] * csw + fillc[con[k]]++;
                    for (int i = 0; i < B.n; ++i)
                        for (int sl = 0; sl < B.cell_w && ptr[i] + sl < ptr[i + 1]; ++sl) dste[(size_t)i * B.cell_w + sl] = dstc[ptr[i] + sl];
                    if (M.upload(&B.fc_ptr, hpC.adj_ptr) || M.upload(&B.fc_col, hpC.adj_col) || M.upload(&B.fc_val, fval) ||
                        M.upload(&B.cadj_dst, dstc) || M.upload(&B.cell_dst, dste) || M.alloc(&B.w_contrib, (size_t)hb.nrow * csw))
                        return 1;
                    HC(hipMemset(B.w_contrib, 0, sizeof(double) * std::max<size_t>((size_t)hb.nrow * csw, 1)));
                    B.cs_w = csw;
                    B.fc_nslot = (int)fval.size();
                    B.front_cw = true;
                }
            }
            if (M.upload(&B.ca_row, car) || M.upload(&B.ca_col, cac) || M.upload(&B.ca_val, cav) ||
                M.upload(&B.cadj_ptr, ptr) || M.upload(&B.cadj_col, col) || M.upload(&B.cadj_con, con) || M.upload(&B.cadj_a, av) ||
                M.alloc(&B.w_uv, (size_t)B.nrow) || M.alloc(&B.w_op, (size_t)B.nrow) || M.alloc(&B.pu.S2, (size_t)2 * B.pu.ne))
                return 1;
            B.cadj_ptr_host_n = ptr[B.n];
            B.use_cw = true;
        }
    }
    tm.lap("constraint-wise operator lists");
    if (hb.is_lp) { // column-wise image + level schedule of the LP block
        for (int t = 0; t < B.na; ++t)
            if (hb.a_row[t] != hb.a_col[t]) return fail_msg("LP block: off-diagonal entry");
        for (int t = 0; t < B.nc; ++t)
            if (hb.c_row[t] != hb.c_col[t]) return fail_msg("LP block: off-diagonal objective entry");
        const int n = B.n;
        std::vector<int> ptr(n + 1, 0), grow(B.na), fill(n, 0);
        std::vector<double> av(B.na), nrm(n, 0.0), cobj(n, 0.0);
        for (int t = 0; t < B.na; ++t) ptr[hb.a_row[t] + 1]++;
        for (int j = 0; j < n; ++j) ptr[j + 1] += ptr[j];
        for (int i = 0; i < hb.nrow; ++i)
            for (int t = hb.a_ptr[i]; t < hb.a_ptr[i + 1]; ++t) {
                const int col = hb.a_row[t], w = ptr[col] + fill[col]++;
                grow[w] = hb.row_idx[i];
                av[w] = hb.a_val[t];
            }
        for (int j = 0; j < n; ++j) {
            double nn = 0.0;
            for (int t = ptr[j]; t < ptr[j + 1]; ++t) nn += av[t] * av[t];
            const double nr = std::sqrt(nn); // nrm2, then squared (data/lorads_lp_conic.c:112-113)
            nrm[j] = nr * nr;
        }
        for (int t = 0; t < B.nc; ++t) cobj[hb.c_row[t]] += hb.c_val[t];
        // level(j) = 1 + max level of the earlier columns that share a constraint row with j
        std::vector<int> row_lvl((size_t)std::max(c->m, 1), 0), lvl(n, 0);
        int nlev = 0;
        for (int j = 0; j < n; ++j) {
            int l = 0;
            for (int t = ptr[j]; t < ptr[j + 1]; ++t) l = std::max(l, row_lvl[grow[t]]);
            lvl[j] = l; // 0-based level
            for (int t = ptr[j]; t < ptr[j + 1]; ++t) row_lvl[grow[t]] = l + 1;
            nlev = std::max(nlev, l + 1);
        }
        std::vector<int> lptr(nlev + 1, 0), lcols(n);
        for (int j = 0; j < n; ++j) lptr[lvl[j] + 1]++;
        for (int l = 0; l < nlev; ++l) lptr[l + 1] += lptr[l];
        std::vector<int> lf(lptr.begin(), lptr.end() - 1);
        for (int j = 0; j < n; ++j) lcols[lf[lvl[j]]++] = j;
        if (M.upload(&B.lp_ptr, ptr) || M.upload(&B.lp_grow, grow) || M.upload(&B.lp_a, av) || M.upload(&B.lp_nrm2sq, nrm) ||
            M.upload(&B.lp_cobj, cobj) || M.upload(&B.lp_lvl_ptr, lptr) || M.upload(&B.lp_lvl_cols, lcols) ||
            M.alloc(&B.lp_cv, (size_t)B.na))
            return 1;
        HC(hipMemset(B.lp_cv, 0, sizeof(double) * (size_t)std::max(B.na, 1)));
        B.is_lp = true;
        B.lp_nlev = nlev;
    }
    return 0;
}

void block_bytes(Block &B) { // SURVEY.md 8(d)
    double F = 8.0 * B.n * B.r;
    B.bytes_mv = 4 * F + 32.0 * B.na + 16.0 * B.nrow;
    B.bytes_cg = B.bytes_mv + 9 * F;
}

// rows of a cone inside the merged cone start at multiples of 32 (= the most rows one workgroup of a row kernel owns)
inline int pad_rows(int n) { return (n + 31) & ~31; }

// Cones that could run as ONE block-diagonal cone (the lockstep sweep, the single-cone forms of phase 1) but for their ranks: every
// cone gets the largest device rank of the context, the columns beyond its own rank are zero and stay zero in both phases (the
// mechanism of the odd ranks' padding column; the caller sees the cone's own rank: Block::rl).  data/lorads_solver.c:290-319,
// 806-906 keep per-cone ranks; what is computed on the extra columns is exact zeros.  LORADS_COMMON_RANK=0: each cone its own.
void common_rank(lorads_hip_ctx *c) {
    if (!c->merged_ok || c->nb < 2 || !opt_common_rank()) return;
    int rmax = 0;
    for (auto &B : c->blk) rmax = std::max(rmax, B.r);
    for (auto &B : c->blk) B.r = rmax;
}

int alloc_factors(lorads_hip_ctx *c) {
    c->all_elem = 0;
    for (auto &B : c->blk) {
        B.off = c->all_elem;
        c->all_elem += (size_t)(c->merged_ok ? pad_rows(B.n) : B.n) * B.r; // pad rows stay zero for ever
        block_bytes(B);
    }
    size_t n = c->all_elem;
    DevPool &M = c->factor_mem;
    double **arrs[] = {&c->R, &c->U, &c->V, &c->G, &c->cr, &c->cp, &c->cQ, &c->rhs, &c->Dtmp};
    for (auto a : arrs) {
        if (M.alloc(a, n)) return 1;
        HC(hipMemset(*a, 0, sizeof(double) * std::max<size_t>(n, 1)));
    }
    for (auto &B : c->blk)
        if ((B.dense_c || B.dense_a) && (M.alloc(&B.Wd, (size_t)B.n * B.r) || M.alloc(&B.Wpart, (size_t)std::max(1, B.ksplit_b) * B.n * B.r))) return 1;
    for (auto &B : c->blk) {
        B.wj_for = nullptr;
        if (B.dense_a && (double)B.nd * B.n * B.r * 8.0 <= 8e9 && (M.alloc(&B.Wj, (size_t)B.nd * B.n * B.r) || (B.dense_c && M.alloc(&B.Wc, (size_t)B.n * B.r)))) return 1;
    }
    c->ring.resize(c->L);
    for (auto &nd : c->ring) {
        if (M.alloc(&nd.s, n) || M.alloc(&nd.y, n)) return 1;
        HC(hipMemset(nd.s, 0, sizeof(double) * std::max<size_t>(n, 1)));
        HC(hipMemset(nd.y, 0, sizeof(double) * std::max<size_t>(n, 1)));
    }
    HC(hipDeviceSynchronize());
    return 0;
}
// The cone the single-cone fast paths may run on: the only cone, or the block-diagonal union of all cones.
Block *solo(lorads_hip_ctx *c) {
    if (shard_vec(c)) return nullptr;
    if (c->nb == 1) return &c->blk[0];
    return c->has_merged ? &c->merged : nullptr;
}

// Several cones with block-separable constraints (every constraint lives in exactly one cone) and equal rank are,
// for every kernel that has no per-cone scalar, ONE cone with a block-diagonal pattern: the flat factor arrays are
// already the concatenation of the cones' n_k x r row-major factors.  Phase 1 (no per-cone scalars at all: the
// L-BFGS runs over the concatenation, lorads_alm.c:230-391) and the evaluation part of phase 2 then cost the
// launches of one cone instead of nb.  The CG solves keep their per-cone launches (per-cone alpha, beta, stopping).
int build_merged(lorads_hip_ctx *c, const lorads_hip_problem *prob) {
    c->merged_ok = c->has_merged = false;
    if (c->nb < 2 || !c->opt.merge) return 0;
    for (int k = 0; k < c->nb; ++k)
        if (prob->blocks[k].is_lp) return 0; // the LP block has its own update; no merged view with one present
    std::vector<char> seen((size_t)std::max(c->m, 1), 0);
    size_t ntot = 0, nrow = 0, na = 0, nc = 0;
    for (int k = 0; k < c->nb; ++k) {
        const lorads_hip_block &hb = prob->blocks[k];
        if (c->blk[k].dense_c || c->blk[k].dense_a) return 0;
        for (int i = 0; i < hb.nrow; ++i) {
            if (seen[hb.row_idx[i]]) return 0; // a constraint couples two cones: the sweep order matters
            seen[hb.row_idx[i]] = 1;
        }
        ntot += pad_rows(hb.n); nrow += hb.nrow; na += hb.a_ptr[hb.nrow]; nc += hb.c_nnz;
    }
    // (a sharded context sees only its own cones' constraints: nrow < m is fine, the single-cone shortcuts that need
    // every constraint check nrow == m themselves)
    if (nblocks_for(ntot, TPB / 8) > c->maxpart) return 0; // partial-sum slots (refresh_merged re-checks per rank)
    std::vector<int> row_idx, a_ptr(1, 0), a_row, a_col, c_row, c_col;
    std::vector<double> a_val, c_val;
    row_idx.reserve(nrow); a_row.reserve(na); a_col.reserve(na); a_val.reserve(na);
    c_row.reserve(nc); c_col.reserve(nc); c_val.reserve(nc);
    int roff = 0;
    for (int k = 0; k < c->nb; ++k) {
        const lorads_hip_block &hb = prob->blocks[k];
        for (int i = 0; i < hb.nrow; ++i) {
            row_idx.push_back(hb.row_idx[i]);
            for (int t = hb.a_ptr[i]; t < hb.a_ptr[i + 1]; ++t) {
                a_row.push_back(hb.a_row[t] + roff); a_col.push_back(hb.a_col[t] + roff); a_val.push_back(hb.a_val[t]);
            }
            a_ptr.push_back((int)a_row.size());
        }
        for (int t = 0; t < hb.c_nnz; ++t) {
            c_row.push_back(hb.c_row[t] + roff); c_col.push_back(hb.c_col[t] + roff); c_val.push_back(hb.c_val[t]);
        }
        c->seg_row0_h.push_back(roff);
        roff += pad_rows(hb.n);
    }
    c->seg_row0_h.push_back(roff);
    lorads_hip_block mb{};
    mb.n = (int)ntot; mb.rank = prob->blocks[0].rank; mb.nrow = (int)nrow; mb.row_idx = row_idx.data(); mb.a_ptr = a_ptr.data();
    mb.a_row = a_row.data(); mb.a_col = a_col.data(); mb.a_val = a_val.data(); mb.c_nnz = (int)nc; mb.c_row = c_row.data();
    mb.c_col = c_col.data(); mb.c_val = c_val.data();
    if (build_block(c, c->merged, mb)) return 1;
    if (c->merged.dense_c) return fail_msg("internal: merged cone classified dense");
    c->merged.off = 0;
    // one constrVal array: the cones' compact vectors are consecutive pieces of the merged one
    size_t o = 0;
    for (auto &B : c->blk) {
        c->mem.free(B.cv);
        B.cv = c->merged.cv + o;
        o += (size_t)B.nrow;
    }
    if (c->mem.upload(&c->seg_row0, c->seg_row0_h) || c->mem.alloc(&c->phase_done, (size_t)2)) return 1;
    HC(hipMemset(c->phase_done, 0, 2 * sizeof(int)));
    if (c->mem.alloc(&c->seg_rr_alt, (size_t)2 * std::max(c->nb, 1))) return 1;
    HC(hipMemset(c->seg_rr_alt, 0, sizeof(double) * 2 * (size_t)std::max(c->nb, 1)));
    c->merged_ok = true;
    return 0;
}
// equal ranks -> the merged view is usable
void refresh_merged(lorads_hip_ctx *c) {
    c->has_merged = false;
    if (!c->merged_ok) return;
    for (auto &B : c->blk)
        if (B.r != c->blk[0].r) return;
    if (nblocks_for((size_t)c->merged.n, TPB / lg_for(c->blk[0].r)) > c->maxpart) return;
    c->merged.r = c->blk[0].r; c->merged.rl = c->blk[0].rl;
    c->merged.t_uv_valid = false;
    block_bytes(c->merged);
    // chunk tables of the per-cone vector kernels (depend on the rank)
    std::vector<int> vt0(1, 0), vt_seg;
    std::vector<long long> vt_e0;
    for (int k = 0; k < c->nb; ++k) {
        const long long e0 = (long long)c->seg_row0_h[k] * c->merged.r, e1 = (long long)c->seg_row0_h[k + 1] * c->merged.r;
        for (long long e = e0; e < e1; e += SEG_CH) { vt_seg.push_back(k); vt_e0.push_back(e); }
        vt0.push_back((int)vt_seg.size());
    }
    if (vt_seg.size() > (size_t)c->maxpart) return;
    DevPool &M = c->mem;
    M.free(c->seg_vt0); M.free(c->seg_vt_seg); M.free(c->seg_vt_e0);
    if (M.upload(&c->seg_vt0, vt0) || M.upload(&c->seg_vt_seg, vt_seg) || M.upload(&c->seg_vt_e0, vt_e0)) return;
    { // row tile -> cone (cone k owns the tiles [row0[k] / rpw, row0[k+1] / rpw))
        const int rpw = TPB / lg_for(c->merged.r);
        std::vector<int> tc((size_t)nblocks_for((size_t)c->merged.n, rpw), c->nb - 1);
        for (int k = 0; k < c->nb; ++k)
            for (int t = c->seg_row0_h[k] / rpw; t < c->seg_row0_h[k + 1] / rpw && t < (int)tc.size(); ++t) tc[t] = k;
        M.free(c->seg_tile_cone);
        if (M.upload(&c->seg_tile_cone, tc)) return;
        // (what a carried convergence test needs of its row tile, in one 16-byte word: see DirArgs.seg_info)
        std::vector<int> info(4 * tc.size());
        for (size_t t = 0; t < tc.size(); ++t) {
            info[4 * t] = tc[t]; info[4 * t + 1] = vt0[tc[t]]; info[4 * t + 2] = vt0[tc[t] + 1];
            info[4 * t + 3] = (t == 0 || tc[t - 1] != tc[t]) ? 1 : 0;
        }
        M.free(c->seg_tile_info);
        if (M.upload(&c->seg_tile_info, info)) return;
    }
    c->seg_nvt = (int)vt_seg.size();
    c->spec_b[0] = c->spec_b[1] = 1;
    c->has_merged = true;
}
void graph_cache_clear(lorads_hip_ctx *c);
void free_factors(lorads_hip_ctx *c) {
    graph_cache_clear(c); // (captured launch chains name the arrays that go away here)
    c->factor_mem.release();
    c->R = c->U = c->V = c->G = c->cr = c->cp = c->cQ = c->rhs = c->Dtmp = nullptr;
    for (auto &B : c->blk) { B.Wd = B.Wpart = B.Wj = B.Wc = nullptr; B.wj_for = nullptr; }
    c->ring.clear();
}

double *mat_base(lorads_hip_ctx *c, int which) {
    switch (which) {
    case LORADS_HIP_MAT_R: return c->R;
    case LORADS_HIP_MAT_U: return c->U;
    case LORADS_HIP_MAT_V: return c->V;
    case LORADS_HIP_MAT_GRAD: return c->G;
    }
    return nullptr;
}
double *vec_base(lorads_hip_ctx *c, int which) {
    switch (which) {
    case LORADS_HIP_VEC_LAMBDA: return c->lambda;
    case LORADS_HIP_VEC_CONSTR_SUM: return c->csum;
    case LORADS_HIP_VEC_Q1: return c->q12;
    case LORADS_HIP_VEC_Q2: return c->q12 + c->m;
    }
    return nullptr;
}

int allreduce_dev(lorads_hip_ctx *c, double *buf, int count) {
    if (!c->ar) return 0;
    if (!c->ar_stream_ordered) HC(hipStreamSynchronize(c->stream));
    if (c->ar(c->ar_user, buf, count, 1)) return fail_msg("allreduce hook failed");
    return 0;
}

