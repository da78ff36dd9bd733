// dev_pool.inc -- the one owner of device and pinned memory (included by lorads_hip.hip and rccl_hook.cpp, after their `fail`).
// Every allocation of the backend is made and released by a DevPool.  The fields that hold the addresses stay plain pointers
// (kernels and argument structs see no difference); the pool remembers what it handed out and frees it in release() / its
// destructor.  Nothing else in csrc/hip/ names the runtime's allocation calls (tests/test_host_and_abi.py checks that).
// Not thread-safe: a pool belongs to one thread at a time (the Lanczos worker threads each use a local one).
// >>> DevPool
std::atomic<long long> g_mem_live[4]; // {device allocations, device bytes, pinned allocations, pinned bytes} this process's pools hold

class DevPool {
    struct Rec { void *p; size_t bytes; bool pinned; };
    std::vector<Rec> recs;
    static void count(const Rec &r, long long sign) {
        g_mem_live[r.pinned ? 2 : 0] += sign;
        g_mem_live[r.pinned ? 3 : 1] += sign * (long long)r.bytes;
    }
    static void drop(const Rec &r) {
        if (r.pinned) hipHostFree(r.p); else hipFree(r.p);
        count(r, -1);
    }
    int take(void **p, size_t bytes, bool pinned, unsigned flags) {
        *p = nullptr;
        recs.reserve(recs.size() + 1); // (recording the address cannot fail once the runtime has handed it out)
        const hipError_t e = pinned ? hipHostMalloc(p, bytes, flags) : hipMalloc(p, bytes);
        if (e != hipSuccess) { *p = nullptr; return fail(pinned ? "hipHostMalloc" : "hipMalloc", e); }
        recs.push_back({*p, bytes, pinned});
        count(recs.back(), +1);
        return 0;
    }

public:
    DevPool() = default;
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    DevPool(DevPool &&o) noexcept { swap(o); }
    DevPool &operator=(DevPool &&o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
    ~DevPool() { release(); }
    void swap(DevPool &o) noexcept { recs.swap(o.recs); }
    // n elements (at least one) of device memory, uninitialised / holding a copy of v / of pinned host memory
    template <typename T> int alloc(T **p, size_t n) { return take((void **)p, sizeof(T) * (n > 0 ? n : 1), false, 0); }
    template <typename T> int upload(T **p, const std::vector<T> &v) {
        if (alloc(p, v.size())) return 1;
        const hipError_t e = v.empty() ? hipSuccess : hipMemcpy(*p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
        return e == hipSuccess ? 0 : fail("hipMemcpy (upload)", e);
    }
    template <typename T> int alloc_pinned(T **p, size_t n, unsigned flags) { return take((void **)p, sizeof(T) * (n > 0 ? n : 1), true, flags); }
    // releases ONE buffer and nulls the field (a buffer that is replaced during its owner's life); a null pointer or one this
    // pool does not own is left alone
    template <typename T> void free(T *&p) {
        for (size_t i = recs.size(); p && i-- > 0;)
            if (recs[i].p == (void *)p) { drop(recs[i]); recs.erase(recs.begin() + (long)i); p = nullptr; }
    }
    // releases everything (idempotent); the fields that held the addresses are the caller's to reset
    void release() {
        for (size_t i = recs.size(); i-- > 0;) drop(recs[i]);
        recs.clear();
    }
};
// <<< DevPool
