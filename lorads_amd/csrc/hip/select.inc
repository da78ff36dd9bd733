// select.inc -- the exact selection of the largest 128-bit keys of an enumeration that is never stored, included by lorads_hip.hip
// after primal.inc and before its two users: cuts.inc (triangle inequalities, DESIGN.md section 14) and bounds.inc (entry bounds,
// section 15).
//
// A user enumerates items with a value v > min_violation >= 0 and gives each the key (bit pattern of v, complement of a packed
// index): positive doubles order as their bit patterns do, so larger keys come earlier in "v descending, index ascending", and no two
// items share a key.  Its enumeration kernel has three modes:
//   0  count the items and histogram the top digit of their keys
//   1  histogram digit [shift, shift + width) of the keys that agree with a prefix above it
//   2  emit the keys at or above a threshold into the key buffer (cursor: ctl[1])
// The contract is all here: the eleven fields a user's kernel arguments carry by these names (below; the helpers are templates over
// the user's struct), select_begin / select_item (the kernel's prologue and its step per item; what its epilogue has to do is said there too),
// SelectScratch with select_reserve and select_check_range / select_check_outputs (the host's buffers, first-pass arguments and
// argument checks).
// select_largest drives them: digits of CUT_DIGIT bits from the top narrow the prefix of the wanted-th largest key until everything at
// or above it fits the buffer (max_cuts + CUT_SLACK keys); ties of v are told apart by the digits of the index, so any number of them
// is handled exactly.  Every pass enumerates anew.  The emitted keys are sorted by a bitonic network, largest first.

namespace {

constexpr int CUT_DIGIT = 12;
constexpr int CUT_BINS = 1 << CUT_DIGIT;
constexpr int CUT_SLACK = 16384;          // keys the buffer holds beyond max_cuts

// digit [shift, shift + width) of the key (hi, lo), width <= CUT_DIGIT
__device__ __host__ __forceinline__ unsigned cut_digit(unsigned long long hi, unsigned long long lo, int shift, int width) {
    unsigned long long v;
    if (shift >= 64) v = hi >> (shift - 64);
    else if (shift == 0) v = lo;
    else v = (lo >> shift) | (hi << (64 - shift));
    return (unsigned)(v & ((1ull << width) - 1));
}
// do the keys agree on every bit at or above top (0 < top <= 128)?
__device__ __forceinline__ bool cut_same_prefix(unsigned long long hi, unsigned long long lo, unsigned long long phi,
                                                unsigned long long plo, int top) {
    if (top >= 128) return true;
    if (top >= 64) return (hi >> (top - 64)) == (phi >> (top - 64));
    return hi == phi && (lo >> top) == (plo >> top);
}

// the keys at [m, P) become the smallest key (no item has it: v > 0 gives hi > 0)
__global__ __launch_bounds__(TPB) void k_cut_fill(unsigned long long m, unsigned long long P, unsigned long long *__restrict__ hi,
                                                  unsigned long long *__restrict__ lo) {
    const unsigned long long i = m + (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    if (i < P) { hi[i] = 0; lo[i] = 0; }
}

// one compare-exchange step (j inside the stage k) of the bitonic sort of P keys, largest first
__global__ __launch_bounds__(TPB) void k_cut_bitonic(unsigned long long P, unsigned long long j, unsigned long long k,
                                                     unsigned long long *__restrict__ hi, unsigned long long *__restrict__ lo) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x, l = i ^ j;
    if (i >= P || l <= i) return;
    const unsigned long long hi_i = hi[i], lo_i = lo[i], hi_l = hi[l], lo_l = lo[l];
    const bool less = hi_i < hi_l || (hi_i == hi_l && lo_i < lo_l);
    const bool greater = hi_i > hi_l || (hi_i == hi_l && lo_i > lo_l);
    if ((i & k) == 0 ? less : greater) { hi[i] = hi_l; lo[i] = lo_l; hi[l] = hi_i; lo[l] = lo_i; }
}

// The selection's share of an enumeration kernel's arguments.  A user's struct `Args` holds these fields among its own, flat (the helpers are templates
// over the user's struct):
//   int mode, shift, width;              the pass: see the modes above; digit [shift, shift + width)
//   double minv;                         min_violation
//   unsigned long long khi, klo;         mode 1: the prefix (bits below shift + width ignored); mode 2: the threshold key
//   unsigned long long *ctl;             [0] items with v > minv (mode 0), [1] emitted keys (mode 2)
//   unsigned long long *hist;            [CUT_BINS]
//   unsigned long long *ohi, *olo;       emitted keys
//   unsigned long long cap;

// what one thread carries through an enumeration
struct SelAcc {
    unsigned long long cnt = 0;
    int cur_bin = -1;       // a run of equal bins is counted in a register and goes to LDS when the bin changes
    unsigned cur_n = 0;
};

// the kernel's prologue (before its first barrier): hist [CUT_BINS] and total in LDS
template <typename Args>
__device__ __forceinline__ void select_begin(const Args &a, unsigned *hist, unsigned long long *total) {
    if (a.mode != 2)
        for (int b = threadIdx.x; b < CUT_BINS; b += TPB) hist[b] = 0;
    if (threadIdx.x == 0) *total = 0;
}

// one item with its v and packed index: counted, binned or emitted when v > min_violation
template <typename Args>
__device__ __forceinline__ void select_item(const Args &a, double v, unsigned long long index, unsigned *hist, SelAcc &acc) {
    if (!(v > a.minv)) return;
    const unsigned long long hi = (unsigned long long)__double_as_longlong(v), lo = ~index;
    if (a.mode == 2) {
        if (hi > a.khi || (hi == a.khi && lo >= a.klo)) {
            const unsigned long long slot = atomicAdd(a.ctl + 1, 1ull);
            if (slot < a.cap) { a.ohi[slot] = hi; a.olo[slot] = lo; }
        }
        return;
    }
    ++acc.cnt;
    if (a.mode == 1 && !cut_same_prefix(hi, lo, a.khi, a.klo, a.shift + a.width)) return;
    const int bin = (int)cut_digit(hi, lo, a.shift, a.width);
    if (bin != acc.cur_bin) {
        if (acc.cur_n) atomicAdd(&hist[acc.cur_bin], acc.cur_n);
        acc.cur_bin = bin; acc.cur_n = 0;
    }
    ++acc.cur_n;
}

// The kernel's epilogue is each kernel's own code (k_bnd_enum's and k_cut_enum's are the same lines and must stay so): after the last
// item a thread flushes its run into hist, mode 0 adds the workgroup's count to ctl[0], and the workgroup adds its non-zero bins to the
// device's histogram; mode 2 has nothing left to do.  k_cut_enum's cut_handle also carries its own copy of select_item's body, per
// class: it must match select_item.

// the argument checks every user shares, in its words and in two parts, so that a user's own checks keep their place between them:
// max_cuts and min_violation ...
int select_check_range(const char *what, double min_violation, int max_cuts) {
    const std::string w = std::string(what) + ": ";
    if (max_cuts < 0 || max_cuts > (1 << 20)) return fail_msg(w + "max_cuts " + std::to_string(max_cuts) + " is outside [0, 2^20]");
    if (!(min_violation >= 0.0) || !std::isfinite(min_violation)) return fail_msg(w + "min_violation must be finite and not negative");
    return 0;
}
// ... and the outputs: `outs` names the user's output arrays, outs_ok says that none of them is NULL
int select_check_outputs(const char *what, const char *outs, int max_cuts, const int64_t *count, bool outs_ok) {
    const std::string w = std::string(what) + ": ";
    if (!count) return fail_msg(w + "count must not be NULL");
    if (max_cuts > 0 && !outs_ok) return fail_msg(w + outs + " must not be NULL when max_cuts > 0");
    return 0;
}

// the buffers of a selection of max_cuts keys (the key buffer a power of two, untouched when max_cuts = 0) and, in the user's
// arguments, what its first pass starts with
template <typename Args>
int select_reserve(SelectScratch &S, DevPool &mem, int max_cuts, double min_violation, Args &a) {
    size_t P = 1;
    while (P < (size_t)max_cuts + CUT_SLACK) P <<= 1;
    if (max_cuts > 0 && (S.khi.grow(mem, P) || S.klo.grow(mem, P))) return 1;
    if (!S.ctl && mem.alloc(&S.ctl, 2 + (size_t)CUT_BINS)) return 1;
    a.mode = 0; a.shift = 128 - CUT_DIGIT; a.width = CUT_DIGIT;
    a.minv = min_violation;
    a.ctl = S.ctl; a.hist = S.ctl + 2;
    a.ohi = S.khi; a.olo = S.klo;
    a.cap = (unsigned long long)max_cuts + CUT_SLACK;
    return 0;
}

// The driver.  `a` is the user's kernel arguments as select_reserve has left them (khi = klo = 0), and `launch()` enqueues one
// enumeration pass with them as they stand.  *count and *passes (may be NULL) are written after the first pass and
// again at the end; khi_out, klo_out get the min(count, max_cuts) largest keys, largest first.  Launches go straight to the stream.
template <typename Args, typename Launch>
int select_largest(lorads_hip_ctx *c, const char *what, int max_cuts, Args &a, Launch launch, int64_t *count, int32_t *passes,
                   std::vector<unsigned long long> &khi_out, std::vector<unsigned long long> &klo_out) {
    unsigned long long *const ctl = a.ctl, *const khi = a.ohi, *const klo = a.olo;
    const std::string w = std::string(what) + ": ";
    std::vector<unsigned long long> h(2 + (size_t)CUT_BINS);
    // pass 1: the count and the top digit
    HC(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * h.size(), c->stream));
    if (launch()) return 1;
    HC(hipMemcpyAsync(h.data(), ctl, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    int np = 1;
    const unsigned long long total = h[0];
    *count = (int64_t)total;
    if (passes) *passes = np;
    const unsigned long long want = std::min<unsigned long long>(total, (unsigned long long)max_cuts);
    if (want == 0) return 0;
    // narrow the prefix of the want-th largest key until what is at or above it fits the buffer
    unsigned long long above = 0, emit_n = 0;
    for (;;) {
        unsigned long long before = 0;
        int d = (1 << a.width) - 1;
        while (d > 0 && above + before + h[2 + d] < want) before += h[2 + d--];
        if (a.shift >= 64) a.khi |= (unsigned long long)d << (a.shift - 64);
        else {
            a.klo |= (unsigned long long)d << a.shift;
            if (a.shift + a.width > 64) a.khi |= (unsigned long long)d >> (64 - a.shift);
        }
        emit_n = above + before + h[2 + d];
        if (emit_n < want) return fail_msg(w + "the histogram of a pass does not add up to the count");
        if (emit_n <= a.cap) break;
        if (a.shift == 0) return fail_msg(w + "the selection did not close");
        above += before;
        a.width = std::min(CUT_DIGIT, a.shift);
        a.shift -= a.width;
        a.mode = 1;
        HC(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * h.size(), c->stream));
        if (launch()) return 1;
        HC(hipMemcpyAsync(h.data(), ctl, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, c->stream));
        HC(hipStreamSynchronize(c->stream));
        ++np;
    }
    // emit everything at or above the prefix (its lower bits zero), sort, hand the first `want` over
    a.mode = 2;
    HC(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * 2, c->stream));
    if (launch()) return 1;
    ++np;
    unsigned long long emitted = 0;
    HC(hipMemcpyAsync(&emitted, ctl + 1, sizeof emitted, hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    if (emitted != emit_n) return fail_msg(w + "the emit pass found " + std::to_string(emitted) + " keys, the histograms " + std::to_string(emit_n));
    unsigned long long Ps = 1;
    while (Ps < emitted) Ps <<= 1;
    if (Ps > emitted)
        hipLaunchKernelGGL(k_cut_fill, dim3(nblocks_for((size_t)(Ps - emitted), TPB)), dim3(TPB), 0, c->stream, emitted, Ps, khi, klo);
    for (unsigned long long k = 2; k <= Ps; k <<= 1)
        for (unsigned long long j = k >> 1; j > 0; j >>= 1)
            hipLaunchKernelGGL(k_cut_bitonic, dim3(nblocks_for((size_t)Ps, TPB)), dim3(TPB), 0, c->stream, Ps, j, k, khi, klo);
    HC(hipGetLastError());
    khi_out.resize((size_t)want); klo_out.resize((size_t)want);
    HC(hipMemcpyAsync(khi_out.data(), khi, sizeof(unsigned long long) * khi_out.size(), hipMemcpyDeviceToHost, c->stream));
    HC(hipMemcpyAsync(klo_out.data(), klo, sizeof(unsigned long long) * klo_out.size(), hipMemcpyDeviceToHost, c->stream));
    HC(hipStreamSynchronize(c->stream));
    if (passes) *passes = np;
    return 0;
}

// a sorted key back into its value and packed index
inline unsigned long long select_unpack(unsigned long long hi, unsigned long long lo, double &v) {
    memcpy(&v, &hi, sizeof v);
    return ~lo;
}

} // namespace
