// branch_cost.hip -- what a scalar branch costs a wavefront on gfx950 that runs one dependent vector stream, with 1 / 2
// wavefronts on its SIMD.
// Build: hipcc -O3 --offload-arch=gfx950 tools/microbench/branch_cost.hip -o tools/microbench/branch_cost
//
// Question (the four-wavefront rollout's ORCA step executed six taken scalar branches beside the loop's back-edge, four of
// them to blocks behind the loop's end and back): is that time, or only text order?  Every variant runs ONE chain of
// dependent v_fma_f32 -- how the ORCA solve's stream looks, as valu_issue.hip's *_DEP rows -- in groups of 15, and behind
// every group one event:
//   NONE       nothing
//   NOP        s_nop 0                                  (a scalar instruction's issue slot, for comparison)
//   NOT_TAKEN  s_cbranch_scc0 with SCC = 1              (a range guard on the fast path, laid out as a fall-through)
//   TAKEN      s_cbranch_scc1 over one s_nop to the next group
//   FAR        s_cbranch_scc1 to a trampoline behind 4 KB of never-executed text, whose s_branch comes back
//              (one per event, 16 trampolines: the round trip the guards made)
//   FAR_COLD   the same with the 16 trampolines 32 KB apart from the loop and 4 KB from each other (other cache lines and
//              sets: what a trampoline costs when its line is not next to anything the step executes)
// An iteration is 16 groups and one counted back-edge (the same in every variant); SCC is set once per iteration, the
// vector instructions leave it alone.  The whole loop is one asm statement, so the compiler neither moves a block nor
// folds a branch.  Reported: shader cycles (s_memtime) per group, and per event over NONE.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

enum { NONE, NOP, NOT_TAKEN, TAKEN, FAR, FAR_COLD };

// 15 dependent v_fma_f32 on %0
#define GROUP ".rept 15\n v_fma_f32 %0, %2, %0, %3\n .endr\n"
#define LOOP_HEAD "s_cmp_eq_u32 0, 0\n"                           /* SCC = 1 */
#define LOOP_TAIL "s_sub_u32 %1, %1, 1\n s_cmp_lg_u32 %1, 0\n s_cbranch_scc1 .Lloop%=\n"
#define IRP16 ".irp k,0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15\n"

template <int V>
__global__ void k(float *out, unsigned long long *cyc, int iters)
{
    const int lane = threadIdx.x & 63;
    float x = 1.0f + lane * 1e-3f;
    const float a = 1.0f + 1e-7f * lane, b = 1e-9f * lane;
    int n = __builtin_amdgcn_readfirstlane(iters);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    if (V == NONE)
        asm volatile(".Lloop%=:\n" LOOP_HEAD ".rept 16\n" GROUP ".endr\n" LOOP_TAIL
                     : "+v"(x), "+s"(n) : "v"(a), "v"(b) : "scc");
    else if (V == NOP)
        asm volatile(".Lloop%=:\n" LOOP_HEAD ".rept 16\n" GROUP "s_nop 0\n .endr\n" LOOP_TAIL
                     : "+v"(x), "+s"(n) : "v"(a), "v"(b) : "scc");
    else if (V == NOT_TAKEN)
        asm volatile(".Lloop%=:\n" LOOP_HEAD ".rept 16\n" GROUP "s_cbranch_scc0 .Lout%=\n .endr\n" LOOP_TAIL ".Lout%=:\n"
                     : "+v"(x), "+s"(n) : "v"(a), "v"(b) : "scc");
    else if (V == TAKEN)
        asm volatile(".Lloop%=:\n" LOOP_HEAD ".rept 16\n" GROUP "s_cbranch_scc1 1f\n s_nop 0\n1:\n .endr\n" LOOP_TAIL
                     : "+v"(x), "+s"(n) : "v"(a), "v"(b) : "scc");
    else if (V == FAR)
        asm volatile(".Lloop%=:\n" LOOP_HEAD
                     IRP16 GROUP "s_cbranch_scc1 .Ltr%=_\\k\n.Lback%=_\\k:\n .endr\n" LOOP_TAIL
                     "s_branch .Lend%=\n"
                     ".fill 1024, 4, 0xbf800000\n"                /* 4 KB of s_nop 0, never executed */
                     IRP16 ".Ltr%=_\\k:\n s_branch .Lback%=_\\k\n .endr\n"
                     ".Lend%=:\n"
                     : "+v"(x), "+s"(n) : "v"(a), "v"(b) : "scc");
    else
        asm volatile(".Lloop%=:\n" LOOP_HEAD
                     IRP16 GROUP "s_cbranch_scc1 .Ltr%=_\\k\n.Lback%=_\\k:\n .endr\n" LOOP_TAIL
                     "s_branch .Lend%=\n"
                     ".fill 8192, 4, 0xbf800000\n"                /* 32 KB */
                     IRP16 ".Ltr%=_\\k:\n s_branch .Lback%=_\\k\n .fill 1023, 4, 0xbf800000\n .endr\n"
                     ".Lend%=:\n"
                     : "+v"(x), "+s"(n) : "v"(a), "v"(b) : "scc");
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * blockDim.x + threadIdx.x] = x;
    if (lane == 0) cyc[blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = t1 - t0;
}

template <int V>
static double run(int waves)
{
    const int iters = 2048, blocks = 256;                         // one workgroup per CU: waves / 4 wavefronts per SIMD
    float *out; unsigned long long *cyc;
    hipMalloc(&out, sizeof(float) * blocks * waves * 64);
    hipMalloc(&cyc, sizeof(unsigned long long) * blocks * waves);
    for (int rep = 0; rep < 3; ++rep) hipLaunchKernelGGL(k<V>, dim3(blocks), dim3(waves * 64), 0, 0, out, cyc, iters);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); exit(1); }
    std::vector<unsigned long long> h(blocks * waves);
    hipMemcpy(h.data(), cyc, h.size() * 8, hipMemcpyDeviceToHost);
    std::sort(h.begin(), h.end());
    hipFree(out); hipFree(cyc);
    return (double)h[h.size() / 2] / (iters * 16.0);              // cycles per group (median wavefront)
}

int main()
{
    for (int waves : {4, 8}) {
        const double base = run<NONE>(waves);
        const double v[] = {base, run<NOP>(waves), run<NOT_TAKEN>(waves), run<TAKEN>(waves), run<FAR>(waves),
                            run<FAR_COLD>(waves)};
        const char *what[] = {"nothing", "s_nop 0", "s_cbranch_scc0, not taken", "s_cbranch_scc1, taken, to the next group",
                              "taken to a trampoline 4 KB on + s_branch back", "the same, trampolines 32 KB on, 4 KB apart"};
        for (int i = 0; i < 6; ++i)
            printf("%d wave(s)/SIMD  15 dependent v_fma_f32 + %-44s %7.2f cycles per group = %6.2f per event over nothing\n",
                   waves / 4, what[i], v[i], v[i] - base);
    }
    return 0;
}
