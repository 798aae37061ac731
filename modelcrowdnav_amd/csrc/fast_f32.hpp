// fast_f32.hpp -- correctly rounded float32 reciprocal and square root in 3 / 5 instructions, range-guarded (round 4).
//
// hipcc expands `1.0f / x` into v_div_scale x2, v_rcp, 6 fma-class instructions, v_div_fmas, v_div_fixup (11) and
// `sqrtf(x)` into scale-in, v_sqrt, a +-1 ulp fix-up with two fma / compare / select pairs, scale-out and a class test
// (15 + hazard nops).  The ORCA solve of the latency-bound env kernels is ONE dependent instruction stream in which a
// lone wavefront pays ~7 cycles per instruction whatever it is; it walks through ~4 roots and ~3 reciprocals per step
// (half-plane construction: |w|, 1/|w|, the tangent leg, 1/dist^2; the speed-disc clip 1/|v_pref|; the 1-D LP's
// discriminant).
//
//   rcp3(x)  = v_rcp_f32 + one fma Newton step (3 instructions)
//   sqrt5(x) = v_rsq_f32, g = x y, h = y / 2, one fma residual + one fma correction (5 instructions)
//
// tools/microbench/fast_math_exhaustive.hip compares both with the IEEE expansions for ALL 2^32 bit patterns on gfx950
// (profiles/r04_fast_math.txt): rcp3 returns the same bits for every operand with biased exponent 1 .. 252 (all normal
// x with |x| < 2^126, both signs), sqrt5 for every positive operand with biased exponent 25 .. 254 (x >= 2^-102).  A
// proof by exhaustion for this hardware -- and the only kind available: v_rcp_f32 / v_rsq_f32 are specified to 1 ulp,
// not bit by bit.  Outside those ranges (zero, denormals, huge, inf, NaN) the guarded wrappers below take the IEEE
// expansion: ONE wave-uniform branch per guard, so the float state stays bit-identical to the oracle for every input.
// `used` = lanes whose result is consumed; the operands of the others (empty neighbour slots, discarded select sides)
// never force the slow path.
//
// FAST_FIRST (the four-wavefront rollout form only: QuadTable::straight in quad_common.hpp).  `if (fast) return fast(x);
// return ieee(x);` tells the compiler nothing about which side is hot: it laid the IEEE expansion on the fall-through path
// and reached the fast sequence through a taken s_cbranch_scc0 to a block behind the loop's end and an s_branch back.  A
// taken scalar branch costs a lone wavefront 29 cycles, that round trip 98 (profiles/r32_branch_cost.txt), on a path with
// three such guards per step.  With the tag the fast value is computed unconditionally and REPLACED, on every lane as
// before, inside one wave-uniform branch marked unlikely under the same condition: the guard is one not-taken
// s_cbranch_scc0 and the IEEE block lies behind the loop.  In-range lanes get the same bits from either arm (the exhaustive
// result above), so every value is what it was.  The fast value of an out-of-range operand is computed and dropped: rsq /
// rcp of zero, a denormal, inf or NaN raise nothing on this hardware.
#pragma once
#include <hip/hip_runtime.h>

namespace mcn {

__device__ __forceinline__ float rcp3(float x)
{
    const float r0 = __builtin_amdgcn_rcpf(x);
    const float e = __builtin_fmaf(-x, r0, 1.0f);
    return __builtin_fmaf(e, r0, r0);
}

__device__ __forceinline__ float sqrt5(float x)
{
    const float y = __builtin_amdgcn_rsqf(x);
    const float g = x * y, h = 0.5f * y;
    const float d = __builtin_fmaf(-g, g, x);
    return __builtin_fmaf(d, h, g);
}

// The guards are integer range tests on the bit pattern: one subtract and one unsigned compare, which a ballot reads
// straight from the compare's lane mask.  (v_cmp_class_f32 would be one instruction, but its result reaches a ballot
// only through a v_cndmask 0/1 and a v_cmp_ne, two more instructions and a hazard nop on the step's critical path.)
// x positive with biased exponent 25 .. 254 (x in [2^-102, 2^128)): exactly sqrt5's verified range
__device__ __forceinline__ bool sqrt5_ok(float x)
{
    return (unsigned)__builtin_bit_cast(int, x) - (25u << 23) < (230u << 23);
}
// x of either sign with biased exponent 1 .. 252 (normal and |x| < 2^126): exactly rcp3's verified range
__device__ __forceinline__ bool rcp3_ok(float x)
{
    return ((unsigned)__builtin_bit_cast(int, x) & 0x7fffffffu) - (1u << 23) < (252u << 23);
}

// lane mask of a predicate (a compare's own result when `b` is one compare: no vector bool is formed)
__device__ __forceinline__ unsigned long long lanes(bool b) { return __builtin_amdgcn_ballot_w64(b); }

// no active lane that uses its result holds an operand outside the fast range
// (two ballots and a scalar and-not: `used & !ok` as booleans goes through vector registers).  `used` may be given
// as a lane mask when it is a combination of predicates: combined on the scalar unit, the combination is never
// materialised in a vector register.
__device__ __forceinline__ bool wave_fast(unsigned long long used, bool ok) { return (used & ~lanes(ok)) == 0; }
__device__ __forceinline__ bool wave_fast(bool used, bool ok) { return wave_fast(lanes(used), ok); }

// == sqrtf(x), bit for bit
template <bool FAST_FIRST = false, class U = bool>
__device__ __forceinline__ float sqrt_f32(float x, U used = true)
{
    if constexpr (FAST_FIRST) {
        float r = sqrt5(x);
        if (__builtin_expect(!wave_fast(used, sqrt5_ok(x)), 0)) r = sqrtf(x);
        return r;
    } else {
        if (wave_fast(used, sqrt5_ok(x))) return sqrt5(x);
        return sqrtf(x);
    }
}

// == 1.0f / x, bit for bit
template <class U = bool>
__device__ __forceinline__ float rcp_f32(float x, U used = true)
{
    if (wave_fast(used, rcp3_ok(x))) return rcp3(x);
    return 1.0f / x;
}

// == 1.0f / sqrtf(x), bit for bit (two roundings, as written); the root of an x in sqrt5's range lies in [2^-51, 2^64):
// inside rcp3's range, so one guard covers both
template <bool FAST_FIRST = false, class U = bool>
__device__ __forceinline__ float rcp_sqrt_f32(float x, U used = true)
{
    if constexpr (FAST_FIRST) {
        float r = rcp3(sqrt5(x));
        if (__builtin_expect(!wave_fast(used, sqrt5_ok(x)), 0)) r = 1.0f / sqrtf(x);
        return r;
    } else {
        if (wave_fast(used, sqrt5_ok(x))) return rcp3(sqrt5(x));
        return 1.0f / sqrtf(x);
    }
}

}  // namespace mcn
