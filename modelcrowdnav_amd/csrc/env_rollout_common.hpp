// env_rollout_common.hpp -- what the two translation units of the fused rollout share: env_rollout_quad.hip (the one- and
// two-wavefront forms and the dispatch) and env_rollout_wg4.hip (the four-wavefront form, built with its own flags).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mcn.h"
#include "quad_common.hpp"
#include "env_step_params.hpp"
#include "env_common.hpp"
#include "launch.hpp"

namespace mcn {

// Diagnostic build only (make -C modelcrowdnav_amd/csrc stamp -> build_stamp/libmcn_hip.so, tools/fixed_cost.py):
// lane 0 of every wavefront writes the 100 MHz real-time counter at kernel entry (slot 0), after the state load
// (slot 1), at the end of each of its first 36 steps (slots 2..37) and at exit (slot 39) to a buffer nothing else
// reads; the four-wavefront form also stamps each wavefront's arrival at hand-off 1 of its first 20 steps (slots
// 40..59).  The product build compiles none of it.  Each translation unit has a buffer of its own (a device global
// belongs to one code object), and so its own copy of quad_common.hpp's counts; read_*_here read this unit's.
#ifdef MCN_DIAG
#define MCN_STAMP_SLOTS 64
#define MCN_STAMP_WAVES 8192
static __device__ unsigned long long g_stamps[MCN_STAMP_WAVES * MCN_STAMP_SLOTS];
#define STAMP(slot)                                                                                              \
    do {                                                                                                         \
        const int w_ = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);                                      \
        if ((threadIdx.x & 63) == 0 && (slot) < MCN_STAMP_SLOTS && w_ < MCN_STAMP_WAVES)                         \
            g_stamps[w_ * MCN_STAMP_SLOTS + (slot)] = __builtin_amdgcn_s_memrealtime();                          \
    } while (0)
// slot 38: where the wavefront ran -- HW_ID (wave / simd / cu / sh / se fields) in the low word, XCC_ID in the high
#define STAMP_WHERE()                                                                                            \
    do {                                                                                                         \
        const int w_ = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);                                      \
        if ((threadIdx.x & 63) == 0 && w_ < MCN_STAMP_WAVES)                                                     \
            g_stamps[w_ * MCN_STAMP_SLOTS + 38] =                                                                \
                (unsigned long long)__builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11)) |                     \
                ((unsigned long long)__builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11)) << 32);             \
    } while (0)
static inline int read_counts_here(void *dst, size_t bytes, int reset)
{
    if (bytes > sizeof(g_diag_counts)) bytes = sizeof(g_diag_counts);
    const int rc = hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_diag_counts), bytes) == hipSuccess ? (int)(bytes / 4) : -1;
    if (reset) {
        void *sym = nullptr;
        if (hipGetSymbolAddress(&sym, HIP_SYMBOL(g_diag_counts)) == hipSuccess) (void)hipMemset(sym, 0, sizeof(g_diag_counts));
    }
    return rc;
}
static inline int read_stamps_here(void *dst, size_t bytes)
{
    if (bytes > sizeof(g_stamps)) bytes = sizeof(g_stamps);
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps), bytes) == hipSuccess ? (int)(bytes / 8) : -1;
}
#else
#define STAMP(slot)
#define STAMP_WHERE()
#endif

__device__ __forceinline__ int bperm_i(int byte_addr, int v) { return __builtin_amdgcn_ds_bpermute(byte_addr, v); }
__device__ __forceinline__ float bperm_f(int byte_addr, float v)
{
    return __builtin_bit_cast(float, bperm_i(byte_addr, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ double bperm_d(int byte_addr, double v)
{
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = bperm_i(byte_addr, (int)b), hi = bperm_i(byte_addr, (int)(b >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// Pins a wave-uniform value in vector registers.  The kernel argument block is ~110 dwords; left to itself the
// compiler keeps all of it (plus every lane mask) in the ~100 scalar registers across the step loop and spills the
// excess to VGPR lanes, paying v_writelane / v_readlane / s_nop on the critical path of every step.  VGPRs are
// plentiful here (one or two wavefronts per SIMD), so loop-invariant operands live there instead.
template <class V>
__device__ __forceinline__ V in_vgpr(V v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// Operands of the RARE paths (an episode ends: finished-episode record, restart from the pool) are not kept in
// registers at all: the rare block re-reads them from the kernel-argument segment (scalar loads, constant cache).
// The empty asm makes the pointer opaque at that point, so the loads cannot be hoisted out of the step loop and
// turned back into ~30 long-lived registers (which is what spilled to scratch before).
typedef const __attribute__((address_space(4))) StepParams *KernargPtr;
__device__ __forceinline__ KernargPtr kernarg_here()
{
    KernargPtr q = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();                      // StepParams is argument 0
    asm volatile("" : "+s"(q));
    return q;
}

}  // namespace mcn
