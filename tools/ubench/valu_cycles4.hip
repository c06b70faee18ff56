// valu_cycles4.hip -- what do the SUB-DWORD (SDWA) forms cost that read one byte of a register as an operand -- v_and_b32_sdwa,
// v_add_u32_sdwa, v_lshlrev_b32_sdwa, v_cmp_le_u32_sdwa with an SGPR pair as its destination -- against the plain forms and the
// byte extracts (v_bfe_u32, v_and 0xff, v_lshrrev 24) they would replace in make_tokens_bits?  Same harness as valu_cycles3.hip.
// build + run:  hipcc --offload-arch=gfx950 -O3 -w -o tools/ubench/valu_cycles4 tools/ubench/valu_cycles4.hip && tools/ubench/valu_cycles4
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>
#include <algorithm>

#define REP8(x) x x x x x x x x

template <int OP>
__global__ void k(uint64_t* ticks, uint32_t* sink, int iters, uint32_t seed) {
    uint32_t a0 = threadIdx.x + seed, a1 = a0 * 3u, a2 = a0 * 5u, a3 = a0 * 7u, a4 = a0 * 11u, a5 = a0 * 13u, a6 = a0 * 17u, a7 = a0 * 19u;
    uint32_t b = seed * 2654435761u + 12345u + threadIdx.x, c = seed | 1u;
    __syncthreads();
    const uint64_t t0 = __builtin_readcyclecounter();
    for (int i = 0; i < iters; i++) {
#define ASM8(txt) asm volatile(txt : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c) \
        : "vcc", "s20", "s21", "s22", "s23", "s24", "s25", "s26", "s27");
#define EIGHT(op, tail) op " %0, %0, %8 " tail "\n\t" op " %1, %1, %8 " tail "\n\t" op " %2, %2, %8 " tail "\n\t" op " %3, %3, %8 " tail "\n\t" \
                        op " %4, %4, %8 " tail "\n\t" op " %5, %5, %8 " tail "\n\t" op " %6, %6, %8 " tail "\n\t" op " %7, %7, %8 " tail "\n\t"
        if (OP == 0) { REP8(ASM8(EIGHT("v_sub_u32", ""))) }                                             // fast class, reference
        if (OP == 1) { REP8(ASM8(EIGHT("v_and_b32", ""))) }
        if (OP == 2) { REP8(ASM8(EIGHT("v_and_b32_sdwa", "dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD"))) }
        if (OP == 3) { REP8(ASM8(EIGHT("v_add_u32_sdwa", "dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD"))) }
        if (OP == 4) { REP8(ASM8(EIGHT("v_lshlrev_b32", ""))) }                                         // slow class, reference
        if (OP == 5) { REP8(ASM8(EIGHT("v_lshlrev_b32_sdwa", "dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3"))) }
        if (OP == 6) { REP8(ASM8(
            "v_bfe_u32 %0, %0, 8, 8\n\tv_bfe_u32 %1, %1, 16, 8\n\tv_bfe_u32 %2, %2, 8, 8\n\tv_bfe_u32 %3, %3, 16, 8\n\t"
            "v_bfe_u32 %4, %4, 8, 8\n\tv_bfe_u32 %5, %5, 16, 8\n\tv_bfe_u32 %6, %6, 8, 8\n\tv_bfe_u32 %7, %7, 16, 8\n\t")) }
        // 7: cmp e64 -> SGPR pair ; cndmask e64 on it (what the extension does per position, without the s_and)
        if (OP == 7) { REP8(ASM8(
            "v_cmp_le_u32_e64 s[20:21], %0, %8\n\tv_cndmask_b32_e64 %1, %1, %9, s[20:21]\n\tv_cmp_le_u32_e64 s[22:23], %2, %8\n\tv_cndmask_b32_e64 %3, %3, %9, s[22:23]\n\t"
            "v_cmp_le_u32_e64 s[24:25], %4, %8\n\tv_cndmask_b32_e64 %5, %5, %9, s[24:25]\n\tv_cmp_le_u32_e64 s[26:27], %6, %8\n\tv_cndmask_b32_e64 %7, %7, %9, s[26:27]\n\t")) }
        // 8: the same with the compare reading one byte of its first operand
        if (OP == 8) { REP8(ASM8(
            "v_cmp_le_u32_sdwa s[20:21], %0, %8 src0_sel:BYTE_1 src1_sel:DWORD\n\tv_cndmask_b32_e64 %1, %1, %9, s[20:21]\n\t"
            "v_cmp_le_u32_sdwa s[22:23], %2, %8 src0_sel:BYTE_2 src1_sel:DWORD\n\tv_cndmask_b32_e64 %3, %3, %9, s[22:23]\n\t"
            "v_cmp_le_u32_sdwa s[24:25], %4, %8 src0_sel:BYTE_3 src1_sel:DWORD\n\tv_cndmask_b32_e64 %5, %5, %9, s[24:25]\n\t"
            "v_cmp_le_u32_sdwa s[26:27], %6, %8 src0_sel:BYTE_0 src1_sel:DWORD\n\tv_cndmask_b32_e64 %7, %7, %9, s[26:27]\n\t")) }
        // 9: cmp -> vcc ; s_and ; cndmask e64: the form hipcc emits in make_tokens_bits today
        if (OP == 9) { REP8(ASM8(
            "v_cmp_le_u32 vcc, %0, %8\n\ts_and_b64 s[20:21], vcc, s[26:27]\n\tv_cndmask_b32_e64 %1, %1, %9, s[20:21]\n\t"
            "v_cmp_le_u32 vcc, %2, %8\n\ts_and_b64 s[22:23], vcc, s[26:27]\n\tv_cndmask_b32_e64 %3, %3, %9, s[22:23]\n\t"
            "v_cmp_le_u32 vcc, %4, %8\n\ts_and_b64 s[20:21], vcc, s[26:27]\n\tv_cndmask_b32_e64 %5, %5, %9, s[20:21]\n\t"
            "v_cmp_le_u32 vcc, %6, %8\n\ts_and_b64 s[22:23], vcc, s[26:27]\n\tv_cndmask_b32_e64 %7, %7, %9, s[22:23]\n\t")) }
        // 10: the same with the byte compare writing an SGPR pair
        if (OP == 10) { REP8(ASM8(
            "v_cmp_le_u32_sdwa s[24:25], %0, %8 src0_sel:BYTE_1 src1_sel:DWORD\n\ts_and_b64 s[20:21], s[24:25], s[26:27]\n\tv_cndmask_b32_e64 %1, %1, %9, s[20:21]\n\t"
            "v_cmp_le_u32_sdwa s[24:25], %2, %8 src0_sel:BYTE_2 src1_sel:DWORD\n\ts_and_b64 s[22:23], s[24:25], s[26:27]\n\tv_cndmask_b32_e64 %3, %3, %9, s[22:23]\n\t"
            "v_cmp_le_u32_sdwa s[24:25], %4, %8 src0_sel:BYTE_3 src1_sel:DWORD\n\ts_and_b64 s[20:21], s[24:25], s[26:27]\n\tv_cndmask_b32_e64 %5, %5, %9, s[20:21]\n\t"
            "v_cmp_le_u32_sdwa s[24:25], %6, %8 src0_sel:BYTE_0 src1_sel:DWORD\n\ts_and_b64 s[22:23], s[24:25], s[26:27]\n\tv_cndmask_b32_e64 %7, %7, %9, s[22:23]\n\t")) }
    }
    const uint64_t t1 = __builtin_readcyclecounter();
    if ((threadIdx.x & 63u) == 0) ticks[blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = t1 - t0;
    if ((a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7) == 0x12345u) sink[0] = a0;
}

template <int OP>
void run(const char* name, int waves_per_simd, int insts_per_iter) {
    const int iters = 2000, blocks = 256, threads = 256 * waves_per_simd;
    uint64_t* d; uint32_t* sink;
    hipMalloc(&d, sizeof(uint64_t) * blocks * 16); hipMalloc(&sink, 64);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(threads), 0, 0, d, sink, 10, 1u);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(threads), 0, 0, d, sink, iters, 7u);
    hipEventRecord(e1);
    hipError_t err = hipDeviceSynchronize();
    if (err != hipSuccess) printf("launch error %s\n", hipGetErrorString(err));
    float ms = 0; hipEventElapsedTime(&ms, e0, e1);
    std::vector<uint64_t> h(blocks * threads / 64);
    hipMemcpy(h.data(), d, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost);
    std::sort(h.begin(), h.end());
    const double med = (double)h[h.size() / 2];
    const double per = med / ((double)iters * insts_per_iter * waves_per_simd);
    printf("%-58s waves/SIMD %d: %5.2f ticks per wave64 VALU instr per SIMD   [%.3f ms wall]\n", name, waves_per_simd, per, ms);
    hipFree(d); hipFree(sink);
}

int main() {
    for (int w : {1, 4}) {
        run<0>("v_sub_u32 (reference, fast class)", w, 64);
        run<1>("v_and_b32", w, 64);
        run<2>("v_and_b32_sdwa src0_sel:BYTE_2", w, 64);
        run<3>("v_add_u32_sdwa src0_sel:BYTE_1", w, 64);
        run<4>("v_lshlrev_b32 (reference, slow class)", w, 64);
        run<5>("v_lshlrev_b32_sdwa src1_sel:BYTE_3", w, 64);
        run<6>("v_bfe_u32 (the extract)", w, 64);
        run<7>("v_cmp_le_u32_e64 -> s[n:n+1] ; v_cndmask_b32_e64", w, 64);
        run<8>("v_cmp_le_u32_sdwa BYTE -> s[n:n+1] ; v_cndmask_b32_e64", w, 64);
        run<9>("v_cmp -> vcc ; s_and_b64 ; v_cndmask_b32_e64", w, 64);
        run<10>("v_cmp_le_u32_sdwa BYTE -> sgpr ; s_and_b64 ; v_cndmask e64", w, 64);
    }
    return 0;
}
