// wave_launch.hip -- how many waves of a kernel with 8 KB of LDS per wave does a CU hold, and what does it cost to REPLACE a wave?
// Workgroups of WG threads with LDS bytes of LDS that do nothing but wait `cyc` s_memtime ticks, 360 waves queued per CU (360 is a
// multiple of 15, 18 and 20 and of every workgroup's wave count here).  Nothing is assumed about the residency:
//   - every wave stamps its life with s_memtime AND s_memrealtime (100 MHz): the ratio is the clock the first one counts;
//   - generations = the launch's growth between two waits / the growth of one wait at that clock; resident waves = 360 / generations;
//   - cross-check: sum of the waves' lifetimes (s_memrealtime) / (CUs x launch time) = waves resident per CU on average (refill gaps and
//     the drain at the end pull it a little below the slot count);
//   - HW_ID's SIMD field of every wave: how a workgroup's waves spread over the four SIMDs.
// The first version of this file took 20 resident waves (13 generations of 256) for granted; the LDS of a workgroup is granted in steps
// of 1280 bytes, so 8192 bytes occupy 8960 and 18 single-wave workgroups fill the 160 KB (profiles/wave_groups.txt).
// build + run on the GPU box:  hipcc --offload-arch=gfx950 -O3 -o tools/ubench/wave_launch tools/ubench/wave_launch.hip && tools/ubench/wave_launch
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

constexpr int QUEUED = 360;          // waves queued per CU

template <int WG, int LDS>
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(5, 5))) void k_wait(uint32_t cyc, uint64_t* life_c, uint64_t* life_r, uint32_t* simd) {
    __shared__ uint32_t lds[LDS / 4];
    const uint64_t t0 = __builtin_readcyclecounter();
    const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
    lds[threadIdx.x] = (uint32_t)t0;
    uint64_t t;
    do {
        __builtin_amdgcn_s_sleep(8);
        t = __builtin_readcyclecounter();
    } while (t - t0 < cyc);
    const uint64_t r = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63u) == 0u) {
        const uint32_t w = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
        life_c[w] = t - t0 + (lds[threadIdx.x] & 0u);
        life_r[w] = r - r0;
        simd[w] = (__builtin_amdgcn_s_getreg(4 | (4 << 6) | (1 << 11))) & 3u;       // HW_REG_HW_ID, bits [5:4]: SIMD_ID
    }
}

struct Run { float ms; double clock_ghz, life_ms_sum; unsigned simd[4]; };

template <int WG, int LDS>
static Run run(uint32_t cyc, uint64_t* d_c, uint64_t* d_r, uint32_t* d_s, int nw) {
    const int grid = nw / (WG / 64);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    Run o = {1e30f, 0, 0, {0, 0, 0, 0}};
    for (int rep = 0; rep < 4; rep++) {
        hipEventRecord(e0);
        hipLaunchKernelGGL((k_wait<WG, LDS>), dim3(grid), dim3(WG), 0, 0, cyc, d_c, d_r, d_s);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        if (rep && ms < o.ms) o.ms = ms;
    }
    std::vector<uint64_t> c(nw), r(nw);
    std::vector<uint32_t> s(nw);
    hipMemcpy(c.data(), d_c, 8 * nw, hipMemcpyDeviceToHost);
    hipMemcpy(r.data(), d_r, 8 * nw, hipMemcpyDeviceToHost);
    hipMemcpy(s.data(), d_s, 4 * nw, hipMemcpyDeviceToHost);
    double sc = 0, sr = 0;
    for (int w = 0; w < nw; w++) { sc += (double)c[w]; sr += (double)r[w]; o.simd[s[w] & 3u]++; }
    o.clock_ghz = sc / sr * 0.1;                 // s_memtime ticks per 10 ns
    o.life_ms_sum = sr * 1e-5;                   // (of the last repetition; the repetitions do not differ)
    hipEventDestroy(e0); hipEventDestroy(e1);
    return o;
}

// launch = generations x (wait / f + c): two waits give the generations at the measured clock f and the cost c of replacing a wave
template <int WG, int LDS>
static void fit(int ncu, uint64_t* d_c, uint64_t* d_r, uint32_t* d_s) {
    const int nw = ncu * QUEUED;
    const uint32_t w0 = 100000u, w1 = 750000u;
    const Run a = run<WG, LDS>(w0, d_c, d_r, d_s, nw), b = run<WG, LDS>(w1, d_c, d_r, d_s, nw);
    const double f = b.clock_ghz * 1e9;
    const double gens = (b.ms - a.ms) * 1e-3 * f / (double)(w1 - w0);
    const double c = a.ms * 1e-3 / gens - w0 / f;
    printf("workgroups of %3d threads, %6d bytes of LDS (%5d per wave): wait %u ticks: %.3f ms, wait %u ticks: %.3f ms; counter %.3f GHz "
           "(s_memrealtime); %.2f generations of %d -> %.1f waves resident per CU; sum of lifetimes / (CUs x launch) = %.2f; %.2f us to "
           "replace a wave; waves per SIMD id %u %u %u %u\n", WG, LDS, LDS / (WG / 64), w0, a.ms, w1, b.ms, b.clock_ghz, gens, QUEUED,
           QUEUED / gens, b.life_ms_sum / (ncu * (double)b.ms), c * 1e6, b.simd[0], b.simd[1], b.simd[2], b.simd[3]);
    fflush(stdout);
}

int main() {
    int ncu = 256;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess) { printf("no device\n"); return 1; }
    const int nw = ncu * QUEUED;
    uint64_t *d_c, *d_r;
    uint32_t* d_s;
    if (hipMalloc(&d_c, 8 * nw) != hipSuccess || hipMalloc(&d_r, 8 * nw) != hipSuccess || hipMalloc(&d_s, 4 * nw) != hipSuccess) return 1;
    printf("%d CUs, %d waves queued per CU\n", ncu, QUEUED);
    fit<64, 7680>(ncu, d_c, d_r, d_s);
    fit<64, 8192>(ncu, d_c, d_r, d_s);
    fit<64, 8960>(ncu, d_c, d_r, d_s);
    fit<128, 16384>(ncu, d_c, d_r, d_s);
    fit<256, 32768>(ncu, d_c, d_r, d_s);
    fit<320, 40960>(ncu, d_c, d_r, d_s);
    fit<640, 81920>(ncu, d_c, d_r, d_s);
    if (hipDeviceSynchronize() != hipSuccess) { printf("error: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
    return 0;
}
