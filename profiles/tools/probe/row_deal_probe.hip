// Measured before the row deal of k_front_cw / k_spmm_ell was built (launch structure phase 2, item 10): where do the
// workgroups of a launch with the front's shape land?  The model to check: ceil(20000 / 32) = 625 workgroups, three of which fit a
// compute unit, are all placed at once on 256 CUs -- some CUs then hold three workgroups and the rest two, and the launch lasts as
// long as the fullest CU -- while 741 workgroups of 27 rows leave at most three times 27 rows on any CU.
// The kernel has the front's launch shape and no gather: 256 threads and 48 KB of dynamic LDS, which alone caps a CU (160 KB of LDS)
// at three workgroups, as the registers of k_front_cw<3, 16, 4> do as well.  Every workgroup stays for `hold_us` microseconds (the
// front's wavefronts live about 17), so one that had to wait for a place shows by its late start.  Thread 0 of workgroup b writes its
// XCC id, its HW_ID word (shader engine, shader array, CU) and its start time; the host builds the histogram of workgroups per CU.
// Build: hipcc -O3 --offload-arch=gfx950 row_deal_probe.hip -o row_deal_probe
// Run:   row_deal_probe [hold_us = 20] [reps = 5] [grid ...  = 625 741]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>
#define HC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)
constexpr int TPB = 256;
constexpr size_t LDS = 48 * 1024;

struct Where { unsigned xcc, hw; unsigned long long t0; };

__global__ __launch_bounds__(TPB) void k_place(Where *__restrict__ out, long long hold_ticks) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const unsigned long long t0 = wall_clock64();
    lds[threadIdx.x] = (double)threadIdx.x; // (the LDS is really used)
    // at most 2^20 trips whatever the clock says: the kernel ends
    for (int i = 0; i < (1 << 20) && (long long)(wall_clock64() - t0) < hold_ticks; ++i) __builtin_amdgcn_s_sleep(8);
    if (threadIdx.x == 0) {
        unsigned xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID, 0, 32)" : "=s"(hw));
        out[blockIdx.x] = Where{xcc, hw, t0};
        if (lds[1] < 0.0) out[blockIdx.x].hw = 0;
    }
}

int main(int argc, char **argv) {
    const double hold_us = argc > 1 ? atof(argv[1]) : 20.0;
    const int reps = argc > 2 ? atoi(argv[2]) : 5;
    std::vector<int> grids;
    for (int i = 3; i < argc; ++i) grids.push_back(std::max(1, std::min(atoi(argv[i]), 1 << 16)));
    if (grids.empty()) grids = {625, 741};
    int dev = 0, ncu = 0, rate_khz = 0;
    HC(hipGetDevice(&dev));
    HC(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    HC(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, dev));
    if (rate_khz <= 0) rate_khz = 100000;
    HC(hipFuncSetAttribute((const void *)k_place, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS));
    const long long hold = (long long)(hold_us * 1e-3 * rate_khz);
    printf("%d compute units, wall clock %d kHz, every workgroup stays %.1f us (%lld ticks), %d threads, %zu bytes of LDS\n", ncu, rate_khz,
           hold_us, hold, TPB, LDS);
    hipStream_t st;
    HC(hipStreamCreate(&st));
    for (int G : grids) {
        Where *d;
        HC(hipMalloc(&d, sizeof(Where) * G));
        std::vector<Where> h(G);
        for (int rep = -1; rep < reps; ++rep) { // (one warm-up launch)
            HC(hipMemsetAsync(d, 0, sizeof(Where) * G, st));
            hipLaunchKernelGGL(k_place, dim3(G), dim3(TPB), LDS, st, d, hold);
            HC(hipGetLastError());
            HC(hipStreamSynchronize(st));
            if (rep < 0) continue;
            HC(hipMemcpy(h.data(), d, sizeof(Where) * G, hipMemcpyDeviceToHost));
            std::map<unsigned, int> per_cu; // key: XCC id, shader engine, shader array, CU id (HW_ID bits 8..15)
            std::map<unsigned, int> per_xcc;
            unsigned long long first = ~0ull, last = 0;
            for (const Where &w : h) {
                ++per_cu[((w.xcc & 15) << 8) | ((w.hw >> 8) & 255)];
                ++per_xcc[w.xcc & 15];
                first = std::min(first, w.t0);
                last = std::max(last, w.t0);
            }
            int late = 0; // started after half the stay: waited for a place
            for (const Where &w : h) late += (long long)(w.t0 - first) > hold / 2;
            std::vector<int> hist(16, 0);
            int mx = 0;
            for (auto &kv : per_cu) { ++hist[std::min(kv.second, 15)]; mx = std::max(mx, kv.second); }
            hist[0] = std::max(0, ncu - (int)per_cu.size());
            printf("grid %5d launch %d: CUs seen %3zu; CUs holding 0/1/2/3/4/5+ workgroups: %d/%d/%d/%d/%d/%d; fullest CU %d; mean %.2f; "
                   "last start %.1f us after the first, %d workgroups started late; per XCC:",
                   G, rep, per_cu.size(), hist[0], hist[1], hist[2], hist[3], hist[4], (int)per_cu.size() - hist[1] - hist[2] - hist[3] - hist[4], mx,
                   (double)G / std::max(ncu, 1), 1e3 * (double)(last - first) / rate_khz, late);
            for (auto &kv : per_xcc) printf(" %d", kv.second);
            printf("\n");
        }
        HC(hipFree(d));
    }
    return 0;
}
