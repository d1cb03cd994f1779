// Developer aid: how fast does a CU of gfx950 issue scalar-side instructions, alone and next to vector work?
// One launch = one mix at one occupancy: a register-only loop (no memory traffic: one store per wave at the end) whose body
// is S scalar-side and V vector instructions, run by 1, 2, 4, 8 or 16 waves on every CU.
//   salu_rate <mix> <waves per CU: 1|2|4|8|16> [iterations]
//   mix: valu (0 + 32 v_add_u32)   salu (32 s_add_u32 + 0)   both (32 + 32, interleaved)   salu2 (64 + 32)
//        nop (32 s_nop 0 + 32)     branch (32 taken s_branch + 32)
// One workgroup per CU (96 KB of LDS each: a second one does not fit); the CU spreads its waves over the four SIMDs round
// robin, so 1 wave has a CU to itself, 2 and 4 waves sit one per SIMD on 2 and 4 SIMDs -- what they lose against 1 is what
// co-resident scalar streams cost each other ACROSS SIMDs --, 8 and 16 waves are 2 and 4 per SIMD.  (Keeping only the waves
// that read SIMD 0 from HW_REG_HW_ID was tried first: every wave read 0 there, so the occupancy is set by the launch alone.)
// Prints the time per loop iteration and the rates it implies at the clock hipDeviceAttributeClockRate reports.
// tools/salu_rate.sh runs every mix at every occupancy, each launch under its own time limit.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

// the four accumulators of each kind are independent, so neither stream waits on its own previous instruction
#define V4 "v_add_u32 %0, %0, %0\n\tv_add_u32 %1, %1, %1\n\tv_add_u32 %2, %2, %2\n\tv_add_u32 %3, %3, %3\n\t"
#define S4 "s_add_u32 %4, %4, %4\n\ts_add_u32 %5, %5, %5\n\ts_add_u32 %6, %6, %6\n\ts_add_u32 %7, %7, %7\n\t"
#define N4 "s_nop 0\n\ts_nop 0\n\ts_nop 0\n\ts_nop 0\n\t"
#define B4 "s_branch 1f\n1:\n\ts_branch 2f\n2:\n\ts_branch 3f\n3:\n\ts_branch 4f\n4:\n\t"
#define R8(x) x x x x x x x x

template <int MIX> __global__ void __launch_bounds__(1024) body(unsigned *out, int iters)
{
    unsigned v0 = threadIdx.x, v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3;
    unsigned s0 = blockIdx.x + 1, s1 = s0 + 1, s2 = s0 + 2, s3 = s0 + 3;
    for (int i = 0; i < iters; ++i) {
        if constexpr (MIX == 0) asm volatile(R8(V4) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");
        if constexpr (MIX == 1) asm volatile(R8(S4) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");
        if constexpr (MIX == 2) asm volatile(R8(S4 V4) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");
        if constexpr (MIX == 3) asm volatile(R8(S4 V4 S4) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");
        if constexpr (MIX == 4) asm volatile(R8(N4 V4) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");
        if constexpr (MIX == 5) asm volatile(R8(B4 V4) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");
    }
    if (threadIdx.x % 64 == 0) out[blockIdx.x * 16 + threadIdx.x / 64] = 0x80000000u | (v0 + v1 + v2 + v3 + s0 + s1 + s2 + s3);
}

int main(int argc, char **argv)
{
    static const char *names[] = {"valu", "salu", "both", "salu2", "nop", "branch"};
    static const int nS[] = {0, 32, 32, 64, 32, 32}, nV[] = {32, 0, 32, 32, 32, 32};
    if (argc < 3) { fprintf(stderr, "usage: salu_rate <mix> <waves per CU> [iterations]\n"); return 1; }
    int mix = -1;
    for (int i = 0; i < 6; ++i) if (!strcmp(argv[1], names[i])) mix = i;
    const int waves = atoi(argv[2]), iters = argc > 3 ? atoi(argv[3]) : 20000;
    if (mix < 0 || (waves != 1 && waves != 2 && waves != 4 && waves != 8 && waves != 16) || iters < 1 || iters > 1000000) { fprintf(stderr, "bad arguments\n"); return 1; }
    int cus = 0, khz = 0;
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, 0));
    unsigned *out = nullptr;
    CHECK(hipMalloc(&out, sizeof(unsigned) * 16 * cus));
    void (*kern[])(unsigned *, int) = {body<0>, body<1>, body<2>, body<3>, body<4>, body<5>};
    const size_t lds = 96 * 1024;
    CHECK(hipFuncSetAttribute((const void *)kern[mix], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    float best = 1e30f;
    CHECK(hipMemset(out, 0, sizeof(unsigned) * 16 * cus));
    for (int rep = 0; rep < 4; ++rep) {                 // the first is the warm-up
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(kern[mix], dim3(cus), dim3(64 * waves), lds, 0, out, iters);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (rep && ms < best) best = ms;
    }
    const double cyc = best * 1e-3 * khz * 1e3 / iters;      // clocks per loop iteration (every wave runs the same loop at once)
    // every wave must have run (the spread of a workgroup's waves over the SIMDs is the hardware's: the rates per SIMD assume it is even)
    unsigned *host = (unsigned *)malloc(sizeof(unsigned) * 16 * cus);
    CHECK(hipMemcpy(host, out, sizeof(unsigned) * 16 * cus, hipMemcpyDeviceToHost));
    int ran = 0;
    for (int i = 0; i < 16 * cus; ++i) ran += host[i] != 0;
    free(host);
    const int simds = waves < 4 ? waves : 4, W = waves < 4 ? 1 : waves / 4;
    if (ran != waves * cus) printf("  (note: %d waves ran, %d expected)\n", ran, waves * cus);
    printf("%-6s %2d waves per CU (%d per SIMD on %d SIMDs): %8.1f clocks per iteration of %2d scalar-side + %2d VALU (+2 of the loop)   per wave %.2f clocks/instr   "
           "per SIMD %.2f instr/clock   per CU: scalar-side %.2f, VALU %.2f instr/clock\n",
           names[mix], waves, W, simds, cyc, nS[mix], nV[mix], cyc / (nS[mix] + nV[mix]), W * (nS[mix] + nV[mix]) / cyc,
           waves * nS[mix] / cyc, waves * nV[mix] / cyc);
    CHECK(hipFree(out));
    return 0;
}
