// presolve.inc -- the pattern work of the pre-solve on the device (included by build.inc, inside lorads_hip.hip's anonymous
// namespace).  What AConePresolveData does with qsort and a chained hash table (data/lorads_sdp_conic.c:868-1076: the union
// sparsity pattern of C and the A_i, the map of every stored entry into it) and what build.inc adds for the gather kernels (the
// symmetric adjacency row -> (neighbour, entry), the transpose entry -> (constraint, value)) is three sorts and a few scans:
//   unique positions   sort (col, row) keys with the entry number as payload, flag the first of every run, scan the flags
//   adjacency          two slots per off-diagonal entry, sort (row, col) keys, row pointers from a count + scan
//   transpose          sort (entry, position in the constraint CSR) -- stable, so constraints stay ascending within an entry
// Hand-written LSD radix sort, 4 bits per pass (count per 256-key tile, scan of the 16 x tiles table, stable scatter: a key's rank
// within its tile from one ballot per digit value), and a three-kernel exclusive scan.  Results are the SAME arrays the host code
// builds (same order everywhere: the summation order of every gather kernel hangs on it); LORADS_DEV_PRESOLVE=0 keeps the host
// code, LORADS_PRESOLVE_CHECK=1 runs both and fails the create on any difference (tests).  Small patterns stay on the host (a
// sort is ~30 launches).
__global__ __launch_bounds__(TPB) void k_rs_count(const unsigned long long *__restrict__ keys, int n, int shift, int *__restrict__ hist, int nblk) {
    __shared__ int cnt[16];
    if (threadIdx.x < 16) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) atomicAdd(&cnt[(int)((keys[i] >> shift) & 15ull)], 1);
    __syncthreads();
    if (threadIdx.x < 16) hist[threadIdx.x * nblk + blockIdx.x] = cnt[threadIdx.x];
}
__global__ __launch_bounds__(TPB) void k_rs_scatter(const unsigned long long *__restrict__ keys, const int *__restrict__ vals, int n, int shift,
                                                    const int *__restrict__ offs, int nblk, unsigned long long *__restrict__ keys_out,
                                                    int *__restrict__ vals_out) {
    __shared__ int wcnt[TPB / 64][16];
    const int i = blockIdx.x * TPB + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool act = i < n;
    const unsigned long long key = act ? keys[i] : 0ull;
    const int d = act ? (int)((key >> shift) & 15ull) : -1;
    int rank = 0;
#pragma unroll
    for (int dd = 0; dd < 16; ++dd) { // stable rank within the wavefront: keys of the same digit in front of this lane
        const unsigned long long m = __ballot(d == dd);
        if (d == dd) rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wave][dd] = __popcll(m);
    }
    __syncthreads();
    if (act) {
        int before = 0;
        for (int w = 0; w < wave; ++w) before += wcnt[w][d];
        const int dst = offs[d * nblk + blockIdx.x] + before + rank;
        keys_out[dst] = key;
        vals_out[dst] = vals[i];
    }
}
// exclusive scan of `len` ints in three kernels: tiles of 1024 (sums out), one workgroup over the tile sums, add
__global__ __launch_bounds__(TPB) void k_scan_tile(const int *in, int len, int *out, int *__restrict__ tsum) { // (in == out allowed)
    __shared__ int sh[TPB];
    const int base = blockIdx.x * 4 * TPB + threadIdx.x * 4;
    int v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = base + k < len ? in[base + k] : 0; s += v[k]; }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < TPB; o <<= 1) { // Hillis-Steele over the threads' sums
        const int t = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    int run = sh[threadIdx.x] - s; // exclusive prefix of this thread within the tile
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (base + k < len) out[base + k] = run; run += v[k]; }
    if (threadIdx.x == TPB - 1) tsum[blockIdx.x] = sh[TPB - 1];
}
__global__ __launch_bounds__(TPB) void k_scan_sums(int *tsum, int nt, int *total) { // one workgroup: exclusive scan of the tile sums, in place
    __shared__ int sh[TPB];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b = 0; b < nt; b += TPB) {
        const int i = b + threadIdx.x, v = i < nt ? tsum[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < TPB; o <<= 1) {
            const int t = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nt) tsum[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 0) carry += sh[TPB - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0 && total) *total = carry;
}
__global__ void k_scan_add(int *__restrict__ out, int len, const int *__restrict__ tsum) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) out[i] += tsum[i / (4 * TPB)];
}
__global__ void k_iota(int n, int *__restrict__ v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}
// keys of the unique-position sort: (col, row) of stored entry i
__global__ void k_pos_keys(int n_ent, const int *__restrict__ row, const int *__restrict__ col, unsigned long long dim, unsigned long long *__restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_ent) keys[i] = (unsigned long long)col[i] * dim + (unsigned long long)row[i];
}
__global__ void k_flag_first(int n, const unsigned long long *__restrict__ keys, int *__restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}
// sorted keys + payload (original entry) + exclusive scan of the first-of-run flags -> unique positions and the entry -> position map
__global__ void k_unique_emit(int n, const unsigned long long *__restrict__ keys, const int *__restrict__ orig, const int *__restrict__ flag,
                              const int *__restrict__ excl, unsigned long long dim, int *__restrict__ urow, int *__restrict__ ucol,
                              int *__restrict__ index) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int u = excl[i] + flag[i] - 1; // number of this key's run
    if (flag[i]) { urow[u] = (int)(keys[i] % dim); ucol[u] = (int)(keys[i] / dim); }
    index[orig[i]] = u;
}
// two adjacency slots per unique entry: (p, q) and -- off the diagonal -- (q, p); a diagonal entry's second slot gets a key past
// every real one and is cut off after the sort
__global__ void k_adj_keys(int ne, const int *__restrict__ urow, const int *__restrict__ ucol, unsigned long long dim,
                           unsigned long long *__restrict__ keys, int *__restrict__ vals, int *__restrict__ deg) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const int p = urow[e], q = ucol[e];
    keys[2 * e] = (unsigned long long)p * dim + (unsigned long long)q;
    vals[2 * e] = e;
    atomicAdd(&deg[p], 1);
    if (p != q) { keys[2 * e + 1] = (unsigned long long)q * dim + (unsigned long long)p; atomicAdd(&deg[q], 1); }
    else keys[2 * e + 1] = dim * dim;
    vals[2 * e + 1] = e;
}
__global__ void k_adj_emit(int nslot, const unsigned long long *__restrict__ keys, unsigned long long dim, int *__restrict__ adj_col) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nslot) adj_col[i] = (int)(keys[i] % dim);
}
// transpose of the constraint CSR: keys = pattern entry of stored entry t, payload t
__global__ void k_tr_keys(int na, const int *__restrict__ a_e, unsigned long long *__restrict__ keys, int *__restrict__ cnt) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= na) return;
    keys[t] = (unsigned long long)a_e[t];
    atomicAdd(&cnt[a_e[t]], 1);
}
__global__ void k_tr_emit(int na, const int *__restrict__ tsorted, const int *__restrict__ con_of, const double *__restrict__ a_val,
                          int *__restrict__ e_con, double *__restrict__ e_val) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= na) return;
    const int t = tsorted[k];
    e_con[k] = con_of[t];
    e_val[k] = a_val[t];
}

struct DevPre { // scratch of one build: one allocation, handed out in 256-byte steps, freed at the build's end
    hipStream_t st = nullptr;
    char *base = nullptr;
    size_t cap = 0, used = 0;
    DevPool mem;
    int reserve(size_t bytes) {
        if (mem.alloc(&base, bytes)) return 1;
        cap = bytes;
        return 0;
    }
    template <typename T> T *get(size_t n) {
        const size_t b = (sizeof(T) * (n > 0 ? n : 1) + 255) / 256 * 256;
        if (!base || used + b > cap) return nullptr;
        T *p = (T *)(base + used);
        used += b;
        return p;
    }
};
inline int dp_grid(size_t n) { return (int)std::max<size_t>(1, (n + TPB - 1) / TPB); } // (never an empty grid: a kernel over nothing does nothing)
// exclusive scan in place; *total_dev (may be null) receives the sum
int dev_exclusive_scan(DevPre &D, int *v, int len, int *total_dev, int *tsum) { // tsum: len / 1024 + 1 ints of scratch
    if (len <= 0) { if (total_dev) HC(hipMemsetAsync(total_dev, 0, sizeof(int), D.st)); return 0; }
    const int nt = (len + 4 * TPB - 1) / (4 * TPB);
    hipLaunchKernelGGL(k_scan_tile, dim3(nt), dim3(TPB), 0, D.st, (const int *)v, len, v, tsum);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(TPB), 0, D.st, tsum, nt, total_dev);
    hipLaunchKernelGGL(k_scan_add, dim3(dp_grid((size_t)len)), dim3(TPB), 0, D.st, v, len, (const int *)tsum);
    return 0;
}
// stable LSD radix sort of (keys, vals) on the low `bits` bits; returns the buffers that hold the result
int dev_radix_sort(DevPre &D, unsigned long long *&keys, int *&vals, int n, int bits) {
    if (n <= 1) return 0;
    unsigned long long *k2 = D.get<unsigned long long>((size_t)n);
    int *v2 = D.get<int>((size_t)n);
    const int nblk = dp_grid((size_t)n);
    int *hist = D.get<int>((size_t)16 * nblk), *tsum = D.get<int>((size_t)16 * nblk / (4 * TPB) + 2);
    if (!k2 || !v2 || !hist || !tsum) return fail_msg("device pre-solve: out of memory");
    for (int shift = 0; shift < bits; shift += 4) {
        hipLaunchKernelGGL(k_rs_count, dim3(nblk), dim3(TPB), 0, D.st, (const unsigned long long *)keys, n, shift, hist, nblk);
        if (dev_exclusive_scan(D, hist, 16 * nblk, nullptr, tsum)) return 1;
        hipLaunchKernelGGL(k_rs_scatter, dim3(nblk), dim3(TPB), 0, D.st, (const unsigned long long *)keys, (const int *)vals, n, shift,
                           (const int *)hist, nblk, k2, v2);
        std::swap(keys, k2);
        std::swap(vals, v2);
    }
    return 0;
}
inline int bits_for(unsigned long long maxval) { int b = 1; while (b < 64 && (maxval >> b) != 0ull) ++b; return b; }
template <typename T> int dp_download(DevPre &D, const T *dev, size_t n, std::vector<T> &out) {
    out.resize(n);
    if (n) HC(hipMemcpyAsync(out.data(), dev, sizeof(T) * n, hipMemcpyDeviceToHost, D.st));
    return 0;
}

// unique_positions + build_adjacency + build_transpose of build.inc on the device; fills `uniq`, `index` and `hp` with the same
// contents.  pos = the stored positions (entries [0, na) are the constraints' in CSR order: their transpose is built), dim = cone
// dimension, nrow / a_ptr / a_val = the constraint CSR (a_val has na entries)
int dev_pattern(lorads_hip_ctx *c, const std::vector<std::pair<int, int>> &pos, int dim, int nrow, const int *a_ptr, int na,
                const double *a_val, std::vector<std::pair<int, int>> &uniq, std::vector<int> &index, HostPattern &hp) {
    DevPre D;
    D.st = c->stream;
    const int N = (int)pos.size();
    if (D.reserve(((size_t)N + (size_t)dim + 64) * 224 + ((size_t)1 << 20))) return fail_msg("device pre-solve: out of memory");
    std::vector<int> hrow((size_t)N), hcol((size_t)N);
    for (int i = 0; i < N; ++i) { hrow[i] = pos[i].first; hcol[i] = pos[i].second; }
    int *drow = D.get<int>((size_t)N), *dcol = D.get<int>((size_t)N), *dval = D.get<int>((size_t)N), *flag = D.get<int>((size_t)N),
        *excl = D.get<int>((size_t)N), *dindex = D.get<int>((size_t)N), *dtot = D.get<int>(4),
        *tsum = D.get<int>(((size_t)2 * N + (size_t)dim) / (4 * TPB) + 4);
    unsigned long long *keys = D.get<unsigned long long>((size_t)N);
    if (!drow || !dcol || !dval || !flag || !excl || !dindex || !dtot || !tsum || !keys) return fail_msg("device pre-solve: out of memory");
    if (N) {
        HC(hipMemcpyAsync(drow, hrow.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, D.st));
        HC(hipMemcpyAsync(dcol, hcol.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, D.st));
    }
    const unsigned long long d64 = (unsigned long long)std::max(dim, 1);
    // ---- unique positions
    hipLaunchKernelGGL(k_pos_keys, dim3(dp_grid((size_t)N)), dim3(TPB), 0, D.st, N, (const int *)drow, (const int *)dcol, d64, keys);
    hipLaunchKernelGGL(k_iota, dim3(dp_grid((size_t)N)), dim3(TPB), 0, D.st, N, dval);
    if (dev_radix_sort(D, keys, dval, N, bits_for(d64 * d64))) return 1;
    hipLaunchKernelGGL(k_flag_first, dim3(dp_grid((size_t)N)), dim3(TPB), 0, D.st, N, (const unsigned long long *)keys, flag);
    if (N) HC(hipMemcpyAsync(excl, flag, sizeof(int) * (size_t)N, hipMemcpyDeviceToDevice, D.st));
    if (dev_exclusive_scan(D, excl, N, dtot, tsum)) return 1;
    int ne = 0;
    HC(hipMemcpyAsync(&ne, dtot, sizeof(int), hipMemcpyDeviceToHost, D.st));
    HC(hipStreamSynchronize(D.st));
    int *urow = D.get<int>((size_t)ne), *ucol = D.get<int>((size_t)ne);
    if (!urow || !ucol) return fail_msg("device pre-solve: out of memory");
    hipLaunchKernelGGL(k_unique_emit, dim3(dp_grid((size_t)N)), dim3(TPB), 0, D.st, N, (const unsigned long long *)keys, (const int *)dval,
                       (const int *)flag, (const int *)excl, d64, urow, ucol, dindex);
    // ---- adjacency
    const int ns2 = 2 * ne;
    unsigned long long *akeys = D.get<unsigned long long>((size_t)ns2);
    int *avals = D.get<int>((size_t)ns2), *deg = D.get<int>((size_t)dim + 1);
    if (!akeys || !avals || !deg) return fail_msg("device pre-solve: out of memory");
    HC(hipMemsetAsync(deg, 0, sizeof(int) * ((size_t)dim + 1), D.st));
    hipLaunchKernelGGL(k_adj_keys, dim3(dp_grid((size_t)ne)), dim3(TPB), 0, D.st, ne, (const int *)urow, (const int *)ucol, d64, akeys, avals, deg);
    if (dev_radix_sort(D, akeys, avals, ns2, bits_for(d64 * d64))) return 1;
    if (dev_exclusive_scan(D, deg, dim + 1, nullptr, tsum)) return 1; // deg[0..dim] -> row pointers (deg[dim] = number of slots)
    // ---- transpose of the constraint CSR
    std::vector<int> con_of((size_t)na);
    for (int i = 0; i < nrow; ++i)
        for (int t = a_ptr[i]; t < a_ptr[i + 1]; ++t) con_of[t] = i;
    unsigned long long *tkeys = D.get<unsigned long long>((size_t)na);
    int *tvals = D.get<int>((size_t)na), *ecnt = D.get<int>((size_t)ne + 1), *dcon = D.get<int>((size_t)na), *e_con = D.get<int>((size_t)na);
    double *daval = D.get<double>((size_t)na), *e_val = D.get<double>((size_t)na);
    if (!tkeys || !tvals || !ecnt || !dcon || !e_con || !daval || !e_val) return fail_msg("device pre-solve: out of memory");
    HC(hipMemsetAsync(ecnt, 0, sizeof(int) * ((size_t)ne + 1), D.st));
    if (na) {
        HC(hipMemcpyAsync(dcon, con_of.data(), sizeof(int) * (size_t)na, hipMemcpyHostToDevice, D.st));
        HC(hipMemcpyAsync(daval, a_val, sizeof(double) * (size_t)na, hipMemcpyHostToDevice, D.st));
    }
    hipLaunchKernelGGL(k_tr_keys, dim3(dp_grid((size_t)na)), dim3(TPB), 0, D.st, na, (const int *)dindex, tkeys, ecnt); // (entries [0, na) of `pos` are the constraints')
    hipLaunchKernelGGL(k_iota, dim3(dp_grid((size_t)na)), dim3(TPB), 0, D.st, na, tvals);
    if (dev_radix_sort(D, tkeys, tvals, na, bits_for((unsigned long long)std::max(ne, 1)))) return 1;
    hipLaunchKernelGGL(k_tr_emit, dim3(dp_grid((size_t)na)), dim3(TPB), 0, D.st, na, (const int *)tvals, (const int *)dcon, (const double *)daval, e_con, e_val);
    if (dev_exclusive_scan(D, ecnt, ne + 1, nullptr, tsum)) return 1;
    // ---- the results, in the host structures the rest of build_block works on
    std::vector<int> h_urow, h_ucol, h_adjp, h_adje, h_eptr, h_econ;
    std::vector<unsigned long long> h_akeys;
    std::vector<double> h_eval;
    if (dp_download(D, (const int *)urow, (size_t)ne, h_urow) || dp_download(D, (const int *)ucol, (size_t)ne, h_ucol) ||
        dp_download(D, (const int *)dindex, (size_t)N, index) || dp_download(D, (const int *)deg, (size_t)dim + 1, h_adjp) ||
        dp_download(D, (const int *)ecnt, (size_t)ne + 1, h_eptr) || dp_download(D, (const int *)e_con, (size_t)na, h_econ) ||
        dp_download(D, (const double *)e_val, (size_t)na, h_eval))
        return 1;
    HC(hipStreamSynchronize(D.st));
    const int nslot = h_adjp[(size_t)dim];
    if (dp_download(D, (const unsigned long long *)akeys, (size_t)nslot, h_akeys) || dp_download(D, (const int *)avals, (size_t)nslot, h_adje)) return 1;
    HC(hipStreamSynchronize(D.st));
    uniq.resize((size_t)ne);
    for (int e = 0; e < ne; ++e) uniq[e] = {h_urow[e], h_ucol[e]};
    hp.erow = h_urow; hp.ecol = h_ucol;
    hp.adj_ptr = h_adjp;
    hp.adj_e = h_adje;
    hp.adj_col.resize((size_t)nslot);
    for (int k = 0; k < nslot; ++k) hp.adj_col[k] = (int)(h_akeys[k] % d64);
    hp.e_ptr = h_eptr; hp.e_con = h_econ; hp.e_val = h_eval;
    return 0;
}
