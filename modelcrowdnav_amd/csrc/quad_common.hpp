// quad_common.hpp -- building blocks shared by the quad-parallel kernels (env_step_quad.hip, env_rollout_quad.hip):
// quad broadcasts, the speculative 1-D / 3-D LP candidates and the per-lane ORCA solve.
#pragma once
#include <hip/hip_runtime.h>
#include "orca_device.hpp"
#include "orca_static.hpp"
#include "quad_take_plan.hpp"

namespace mcn {

// Diagnostic build only: how often a wavefront takes each data-dependent path (tools/fixed_cost.py).
#ifdef MCN_DIAG
static __device__ unsigned int g_diag_counts[8192 * 4];
#define DIAG_COUNT(which)                                                                                        \
    do {                                                                                                         \
        const int w_ = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);                                      \
        if (w_ < 8192 && (int)(threadIdx.x & 63) == __ffsll((unsigned long long)__ballot(1)) - 1)                \
            atomicAdd(&g_diag_counts[w_ * 4 + (which)], 1u);                                                     \
    } while (0)
#else
#define DIAG_COUNT(which)
#endif

// quad broadcast of lane I (0..3) of every quad: a DPP move, no LDS traffic.  No `old` operand: a lane keeps its old
// value only when its source lane is inactive, and every quad is active or inactive as a whole (the callers' control
// flow is quad-uniform), so the value a zero-initialised `old` would add -- one v_mov per broadcast -- is never read.
template <int I>
__device__ __forceinline__ int qbi(int v) { return __builtin_amdgcn_mov_dpp(v, I * 0x55, 0xf, 0xf, false); }
template <int I>
__device__ __forceinline__ float qbf(float v) { return __builtin_bit_cast(float, qbi<I>(__builtin_bit_cast(int, v))); }
template <int I>
__device__ __forceinline__ double qbd(double v)
{
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = qbi<I>((int)b), hi = qbi<I>((int)(b >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
template <int I>
__device__ __forceinline__ float4 qb4(float4 v) { return make_float4(qbf<I>(v.x), qbf<I>(v.y), qbf<I>(v.z), qbf<I>(v.w)); }
// The same broadcast with bound_ctrl set, which changes no value here either (a quad is active or inactive as a whole): the
// form the compiler folds into the instruction that reads it where that is a VOP2's first operand (v_min_i32_dpp).  The
// lean take steps alone use it: the other callers' code stays what it is.
template <int I>
__device__ __forceinline__ int qbi_fold(int v) { return __builtin_amdgcn_mov_dpp(v, I * 0x55, 0xf, 0xf, true); }
template <int I>
__device__ __forceinline__ float qbf_fold(float v) { return __builtin_bit_cast(float, qbi_fold<I>(__builtin_bit_cast(int, v))); }

__device__ __forceinline__ float4 sel4(const float4 (&L)[4], int i)
{
    const float4 a = i == 1 ? L[1] : L[0], b = i == 3 ? L[3] : L[2];
    return i >= 2 ? b : a;
}

// How quad_orca_core shares a quad's sorted half-planes, chosen at compile time.
//   QuadDpp    ds_permute to the rank's lane, then 16 DPP broadcasts: no LDS memory.  Every caller but the
//              four-wavefront rollout form.
//   QuadTable  through a table of 64 float4 slots in LDS that belongs to this wavefront alone: lane l writes its line to
//              slot (l & ~3) | rank and reads its quad's four slots and its own, five 16-byte reads for the 16 DPP
//              moves and four ds_permutes.  A quad touches only its own four slots, so idle quads disturb nobody.  The
//              wavefront's LDS operations execute in order; a wavefront-scope release / acquire pair around a wave
//              barrier keeps the compiler from moving a read above the writes, and a step's write follows the previous
//              step's reads in program order: no s_barrier.  The 3-D LP reads its run-time line from the table too.
//              This path also takes the step's small savings that would change the other callers' code (`slim`): one
//              squared distance for rank and half-plane, the 1-D LP's clamp as two selects.
//              And it spreads the 1-D LP's six (line, earlier line) intersections over the quad as 2 + 2 + 1 + 1
//              (`spread`, lp1_spread below) where the other callers run 0 + 1 + 2 + 3 as three passes on every lane.
//              And its four take steps decide from the minimum beside the test instead of from `fail` behind it
//              (`lean_take`, take_step_lean in quad_take_plan.hpp): per step five instructions in a row where the other
//              callers have eight, and two instructions fewer.  The 3-D LP candidate's three take steps are the same
//              lean steps here (`lean_lp3`; the other callers keep the guarded ones).
//              And the rank's four quad broadcasts of the key sit inside the subtractions that read them (`fold_rank`:
//              four v_sub_u32_dpp for four v_mov_b32_dpp and three v_sub_u32).
//              And its five range guards (half-plane, clip, lp1_spread's discriminant, the 3-D LP candidate's two) compute
//              the fast values first and replace them under a branch marked unlikely (`straight`; fast_f32.hpp: FAST_FIRST),
//              so that the IEEE expansions lie behind the step's text and a guard is one not-taken branch.
struct QuadDpp {
    static constexpr bool table = false, slim = false, spread = false, lean_take = false;
    static constexpr bool fold_rank = false, lean_lp3 = false, straight = false;
};
struct QuadTable {
    static constexpr bool table = true, slim = true, spread = true, lean_take = true;
    static constexpr bool fold_rank = true, lean_lp3 = true, straight = true;
    float4 *tab;                                                 // this wavefront's 64 slots
};

// linearProgram1 on line `no` (run-time, 0..3) against lines [0, no): uniform code, predicated steps.  `ln` is line
// `no` itself (L[no]), handed over by the caller, who holds it without a run-time select (lane k's own sorted line).
template <bool DIR, bool SELECT_CLAMP = false>
__device__ __forceinline__ bool lp1_rt(const float4 (&L)[4], const float4 &ln, int no, float radius, float optx, float opty,
                                       float &rx, float &ry)
{
    const float dp = dot2(ln.x, ln.y, ln.z, ln.w);
    const float disc = dp * dp + radius * radius - dot2(ln.x, ln.y, ln.x, ln.y);
    bool ok = !(disc < 0.0f);
    const float sq = sqrt_f32(disc, ok);
    float tl = -dp - sq;
    float tr = -dp + sq;
    // straight-line: every lane runs all three steps and masks them with selects (a lone wavefront per SIMD pays
    // for every exec-mask instruction; the quotient of a skipped / parallel line is computed and discarded)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float4 li = L[i];
        const float den = det2(ln.z, ln.w, li.z, li.w);
        const float num = det2(li.z, li.w, ln.x - li.x, ln.y - li.y);
        const float t = num / den;
        const bool live = i < no;
        const bool par = fabsf(den) <= kRvoEps;
        const bool cut = live & !par;
        const float ntr = fminf(tr, t), ntl = fmaxf(tl, t);
        tr = (cut & (den >= 0.0f)) ? ntr : tr;
        tl = (cut & !(den >= 0.0f)) ? ntl : tl;
        ok = ok & !(live & ((par ? 0.0f : tl) > (par ? num : tr)));      // parallel: 0 > num, else tl > tr
    }
    float t;
    if (DIR) {
        t = (dot2(optx, opty, ln.z, ln.w) > 0.0f) ? tr : tl;
    } else {
        t = dot2(ln.z, ln.w, optx - ln.x, opty - ln.y);
        if (SELECT_CLAMP) {
            // the same two comparisons as selects (a NaN t, tl or tr answers both with false, as below): the branchy
            // form compiles to two nested exec-mask regions
            const float hi = (t > tr) ? tr : t;
            t = (t < tl) ? tl : hi;
        } else {
            if (t < tl) t = tl; else if (t > tr) t = tr;
        }
    }
    rx = ln.x + t * ln.z;
    ry = ln.y + t * ln.w;
    return ok;
}

// One bound update of the 1-D LP from an intersection (t = num / den) that is handed over: the statements of lp1_rt's
// loop body after the quotient.
__device__ __forceinline__ void lp1_cut(bool live, float t, float den, float num, float &tl, float &tr, bool &ok)
{
    const bool par = fabsf(den) <= kRvoEps;
    const bool cut = live & !par;
    const float ntr = fminf(tr, t), ntl = fmaxf(tl, t);
    tr = (cut & (den >= 0.0f)) ? ntr : tr;
    tl = (cut & !(den >= 0.0f)) ? ntl : tl;
    ok = ok & !(live & ((par ? 0.0f : tl) > (par ? num : tr)));          // parallel: 0 > num, else tl > tr
}

// lp1_rt<false> of lane k's own sorted line `ln` (no = k) with the quad's six intersections (k, i), i < k, dealt
// 2 + 2 + 1 + 1 over the lanes instead of 0 + 1 + 2 + 3: two passes where lp1_rt runs three.
//   pass A  lane k intersects (lnA, liA): lanes 1 - 3 their own line with line 0, as lp1_rt's i = 0; lane 0, whose own
//           1-D LP has no earlier line, line 3 with line 2.  The caller reads both operands from the line table at
//           addresses that differ per lane and never change (lane 0: slots 3 and 2 of its quad; the others: their own
//           slot and slot 0), so no select picks them.
//   pass B  lanes 2 and 3 intersect their own line with line 1 (`liB`); lanes 0 and 1 compute a value nobody reads, as
//           every lane above its `no` does in lp1_rt.
//   then    lane 3 takes lane 0's (t, den, num) of pass A by three quad broadcasts and applies it as its update i = 2,
//           after its own i = 0 and i = 1: the order lp1_rt has.
// Lane 0 forms den, num and num / den of pair (3, 2) by the expressions, on the operands, that lane 3 forms them with
// in lp1_rt's pass i = 2 (ln = line 3, li = line 2: the table's slots hold the bits lane 3's `srt` and L[2] are), and a
// DPP move copies bits, NaN payloads included: every bound, `ok` and the candidate are bit for bit lp1_rt's.
template <bool SELECT_CLAMP, bool STRAIGHT = false>
__device__ __forceinline__ bool lp1_spread(const float4 &ln, const float4 &lnA, const float4 &liA, const float4 &liB, int k,
                                           float radius, float optx, float opty, float &rx, float &ry)
{
    const float dp = dot2(ln.x, ln.y, ln.z, ln.w);
    const float disc = dp * dp + radius * radius - dot2(ln.x, ln.y, ln.x, ln.y);
    bool ok = !(disc < 0.0f);
    const float sq = sqrt_f32<STRAIGHT>(disc, ok);
    float tl = -dp - sq;
    float tr = -dp + sq;
    const float denA = det2(lnA.z, lnA.w, liA.z, liA.w);
    const float numA = det2(liA.z, liA.w, lnA.x - liA.x, lnA.y - liA.y);
    const float tA = numA / denA;
    lp1_cut(0 < k, tA, denA, numA, tl, tr, ok);
    const float denB = det2(ln.z, ln.w, liB.z, liB.w);
    const float numB = det2(liB.z, liB.w, ln.x - liB.x, ln.y - liB.y);
    const float tB = numB / denB;
    lp1_cut(1 < k, tB, denB, numB, tl, tr, ok);
    lp1_cut(k == 3, qbf<0>(tA), qbf<0>(denA), qbf<0>(numA), tl, tr, ok);
    float t = dot2(ln.z, ln.w, optx - ln.x, opty - ln.y);
    if (SELECT_CLAMP) {
        const float hi = (t > tr) ? tr : t;                      // (as lp1_rt: a NaN answers both comparisons with false)
        t = (t < tl) ? tl : hi;
    } else {
        if (t < tl) t = tl; else if (t > tr) t = tr;
    }
    rx = ln.x + t * ln.z;
    ry = ln.y + t * ln.w;
    return ok;
}

// One lean take step (take_step_lean in quad_take_plan.hpp) of an incremental LP on the quad: line I is LN on every lane,
// lane I holds its verdict (fcode) and its candidate (cx, cy); `fail`, rx and ry are the running values.  The verdict's
// broadcast is the form the compiler folds into the minimum (v_min_i32_dpp).  A file-scope macro because two functions
// use it (lp3_candidate_quad<true> and quad_orca_core's lean branch); undefined at the end of this header.
#define MCN_TAKE_LEAN(I, LN)                                                                   \
        {                                                                                      \
            const int code_i = qbi_fold<I>(fcode);                                             \
            const float cx_i = qbf_fold<I>(cx), cy_i = qbf_fold<I>(cy);                         \
            const bool out = det2(LN.z, LN.w, LN.x - rx, LN.y - ry) > 0.0f;                     \
            const TakeStep s = take_step_lean(fail, code_i, out, I);                           \
            fail = s.fail;                                                                     \
            rx = s.take ? cx_i : rx; ry = s.take ? cy_i : ry;                                   \
        }

// 3-D LP candidate of line `i` (run-time, quad-uniform), computed by the four lanes of the quad TOGETHER: lane k
// projects line k on line i (RVO2 linearProgram3's inner loop, one projection per lane instead of three in a row),
// then solves the direction-optimising 1-D LP of ITS projected line against the earlier kept ones speculatively
// (as the 2-D LP of quad_orca_velocity does), and the incremental LP collapses into three compare-and-take steps.
// Lines the reference drops (parallel, same direction) are not compacted away but neutralised: the incremental LP over
// the kept lines in their original order is the same sequence of operations.  Same arithmetic per value as
// lp3() in orca_device.hpp / the oracle, so the same bits.  Returns whether the candidate is valid (the inner
// 2-D LP succeeded); the result is identical on the four lanes.  `li` = line i (L[i]), `lj` = line k, i.e. the sorted
// line this lane holds itself (the quad broadcast of lane k read on lane k): no run-time select for either.
//
// A line that is not kept (dropped, self, or not before i) gets the projected direction (+-0, +-0) -- its 1 / |dd|
// is replaced by 0 -- or NaN when its operands are not finite.  Either way every test that reads it is false without
// a mask: its violation test det2(0, 0, ., .) > 0, and in a kept lane's 1-D LP it is "parallel" with num = +-0 (0 > num
// false) or, with a NaN den, fminf / fmaxf keep tr / tl and tl > tr repeats the previous step's answer.  So no kept
// flag is broadcast, and the take steps are the 2-D LP's `fail > I` form (quad_orca_velocity).
template <bool LEAN = false, bool STRAIGHT = false>
__device__ __forceinline__ bool lp3_candidate_quad(const float4 &li, const float4 &lj, int i, int k, float radius, float &rx,
                                                   float &ry)
{
    const float dt = det2(li.z, li.w, lj.z, lj.w);
    const bool par = fabsf(dt) <= kRvoEps;
    const bool same = dot2(li.z, li.w, lj.z, lj.w) > 0.0f;
    const bool keptb = (k < i) & !(par & same);
    // the same predicate as a lane mask, combined from the compares' own masks (the guards below read it)
    const unsigned long long m_kept = lanes(k < i) & ~(lanes(par) & lanes(same));
    const float sc = det2(lj.z, lj.w, li.x - lj.x, li.y - lj.y) / dt;
    const float ddx = lj.z - li.z, ddy = lj.w - li.w;
    const float inv = keptb ? rcp_sqrt_f32<STRAIGHT>(dot2(ddx, ddy, ddx, ddy), m_kept) : 0.0f;
    const float4 q = make_float4(par ? 0.5f * (li.x + lj.x) : li.x + sc * li.z,
                                 par ? 0.5f * (li.y + lj.y) : li.y + sc * li.w, ddx * inv, ddy * inv);
    const float4 P0 = qb4<0>(q), P1 = qb4<1>(q), P2 = qb4<2>(q);
    const float ox = -li.w, oy = li.z;

    // speculative 1-D LP of projected line k against the projected lines 0 .. min(k, 2) - 1 (dropped ones are no-ops)
    const float dp = dot2(q.x, q.y, q.z, q.w);
    const float disc = dp * dp + radius * radius - dot2(q.x, q.y, q.x, q.y);
    bool ok = !(disc < 0.0f);
    const float sq = sqrt_f32<STRAIGHT>(disc, lanes(!(disc < 0.0f)) & m_kept);
    float tl = -dp - sq;
    float tr = -dp + sq;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float4 pj = j == 0 ? P0 : P1;
        const bool live = j < k;
        const float den = det2(q.z, q.w, pj.z, pj.w);
        const float num = det2(pj.z, pj.w, q.x - pj.x, q.y - pj.y);
        const float t = num / den;
        const bool parj = fabsf(den) <= kRvoEps;
        const bool cut = live & !parj;
        const float ntr = fminf(tr, t), ntl = fmaxf(tl, t);
        tr = (cut & (den >= 0.0f)) ? ntr : tr;
        tl = (cut & !(den >= 0.0f)) ? ntl : tl;
        ok = ok & !(live & ((parj ? 0.0f : tl) > (parj ? num : tr)));      // parallel: 0 > num, else tl > tr
    }
    const float tt = (dot2(ox, oy, q.z, q.w) > 0.0f) ? tr : tl;
    const float cx = q.x + tt * q.z, cy = q.y + tt * q.w;
    // lane k's code for the take steps: 4 when its 1-D LP is feasible, else k (the 2-D LP fails at line k)
    const int fcode = ok ? 4 : k;

    rx = radius * ox; ry = radius * oy;
    // as MCN_LP2_TAKE over the lines 0 .. 2: `fail` stays 3 until a violated line's 1-D LP is infeasible
    int fail = 3;
    if constexpr (LEAN) {
        // (Path::lean_lp3) the same three steps in the 2-D LP's lean form: take_step_lean, the broadcasts foldable
        MCN_TAKE_LEAN(0, P0) MCN_TAKE_LEAN(1, P1) MCN_TAKE_LEAN(2, P2)
    } else {
#define MCN_LP3_INNER_TAKE(I, PI)                                                              \
        {                                                                                      \
            const int code_i = qbi<I>(fcode); const float cx_i = qbf<I>(cx), cy_i = qbf<I>(cy); \
            const bool out = det2(PI.z, PI.w, PI.x - rx, PI.y - ry) > 0.0f;                     \
            fail = ((fail > I) & out) ? min(fail, code_i) : fail;                               \
            const bool take = (fail > I) & out;                                                 \
            rx = take ? cx_i : rx; ry = take ? cy_i : ry;                                       \
        }
        MCN_LP3_INNER_TAKE(0, P0) MCN_LP3_INNER_TAKE(1, P1) MCN_LP3_INNER_TAKE(2, P2)
#undef MCN_LP3_INNER_TAKE
    }
    return fail == 3;
}

// ORCA velocity of the human owning this quad.  Lane k holds candidate neighbour k: `o` = its (px, py, vx, vy) in
// float32, `crd` its radius, `cand_valid` whether the slot is populated.  The result is identical on the four
// lanes of the quad (layout: lane = 4 * human + k).
// inv_th / inv_ts = 1 / timeHorizon, 1 / timeStep: computed by the caller once per launch and handed over as opaque
// values -- left to itself the compiler rewrites `apart ? 1 / a : 1 / b` into `1 / (apart ? a : b)`, i.e. one IEEE
// division (11 instructions) on the critical path of EVERY step instead of two before the step loop.
//
// Two parts.  quad_orca_operands turns a human's float64 state into the solve's float32 operands: pack A =
// (px, py, vx, vy), pack B = (prefx, prefy, frad, ms).  A candidate's `orad` is its own frad (the same expression on
// the same radius) and its `o` its own pack A.  quad_orca_core is the float32 solve on those operands.  The
// four-wavefront rollout form computes the packs on its float64 wavefront and runs the core alone on the ORCA ones.
__device__ __forceinline__ void quad_orca_operands(const mcn_env_cfg &c, double2 pos, double2 vel, double2 goal, double rad,
                                                   double vpref, float4 &A, float4 &B)
{
    const float fpx = (float)pos.x, fpy = (float)pos.y, fvx = (float)vel.x, fvy = (float)vel.y;
    const float frad = (float)(rad + 0.01 + c.orca_safety_space);
    const float ms = (float)vpref;
    const float prefx = (float)(goal.x - pos.x), prefy = (float)(goal.y - pos.y);
    A = make_float4(fpx, fpy, fvx, fvy);
    B = make_float4(prefx, prefy, frad, ms);
}

// The part of the operands that changes with every step: (px, py, prefx, prefy), the same expressions as above.  The
// four-wavefront rollout form recomputes only this per step (the velocity stays the float32 the solve produced, frad
// and ms change on a restart only).
__device__ __forceinline__ float4 quad_orca_position_pack(double2 pos, double2 goal)
{
    return make_float4((float)pos.x, (float)pos.y, (float)(goal.x - pos.x), (float)(goal.y - pos.y));
}

template <class Path = QuadDpp>
__device__ __forceinline__ void quad_orca_core(const mcn_env_cfg &c, int lane, int k, bool cand_valid, float4 A, float4 B,
                                               float4 o, float orad, float inv_th, float inv_ts, float &rx, float &ry,
                                               Path path = Path());

__device__ __forceinline__ void quad_orca_velocity(const mcn_env_cfg &c, int lane, int k, bool cand_valid,
                                                   double2 pos, double2 vel, double2 goal, double rad, double vpref,
                                                   float4 o, double crd, float inv_th, float inv_ts, float &rx, float &ry)
{
    float4 A, B;
    quad_orca_operands(c, pos, vel, goal, rad, vpref, A, B);
    const float orad = (float)(crd + 0.01 + c.orca_safety_space);
    quad_orca_core(c, lane, k, cand_valid, A, B, o, orad, inv_th, inv_ts, rx, ry);
}

template <class Path>
__device__ __forceinline__ void quad_orca_core(const mcn_env_cfg &c, int lane, int k, bool cand_valid, float4 A, float4 B,
                                               float4 o, float orad, float inv_th, float inv_ts, float &rx, float &ry,
                                               Path path)
{
    const float fpx = A.x, fpy = A.y, fvx = A.z, fvy = A.w;
    const float prefx = B.x, prefy = B.y, frad = B.z, ms = B.w;
    const float range_sq = c.orca_neighbor_dist * c.orca_neighbor_dist;
    // squared distance to the candidate.  Slim path: from o - p, which the half-plane construction needs anyway and takes
    // together with this square; p - o is its exact negation, so the squares and their sum are the same bits
    const float ddx = Path::slim ? o.x - fpx : fpx - o.x, ddy = Path::slim ? o.y - fpy : fpy - o.y;
    const float d = dot2(ddx, ddy, ddx, ddy);
    const bool in = cand_valid && (d < range_sq);
    // stable ascending order among the in-range candidates (RVO2 insertAgentNeighbor); the rest fill the remaining
    // slots in lane order so that ranks stay a permutation.  One integer key per lane does both: an in-range d is a
    // finite float >= +0 (a sum of squares below range_sq), so its bits order as the value does; out-of-range slots
    // get +inf's bits, above every in-range key.  Lane q ranks before lane k iff key_q < key_k, or key_q == key_k and
    // q < k, i.e. key_q - key_k < (q < k) (no overflow: keys lie in [0, 0x7f800000]).
    const int key = in ? __builtin_bit_cast(int, d) : 0x7f800000;
    int kd0, kd1, kd2, kd3;
    if constexpr (Path::fold_rank) {
        // the four broadcasts inside their subtractions (v_sub_u32_dpp).  The DPP combiner works per basic block, and left
        // alone the subtractions sink behind the half-plane guard's branch, away from their broadcasts: the empty statement
        // keeps the four differences where they are formed.  (The compiler emits these DPP reads itself, so the two
        // instructions between the write of `key` and the first of them are its to place.)
        kd0 = qbi_fold<0>(key) - key; kd1 = qbi_fold<1>(key) - key; kd2 = qbi_fold<2>(key) - key; kd3 = qbi_fold<3>(key) - key;
        asm volatile("" : "+v"(kd0), "+v"(kd1), "+v"(kd2), "+v"(kd3));
    } else {
        kd0 = qbi<0>(key) - key; kd1 = qbi<1>(key) - key; kd2 = qbi<2>(key) - key; kd3 = qbi<3>(key) - key;
    }
    const int rank = (kd0 < (0 < k ? 1 : 0)) + (kd1 < (1 < k ? 1 : 0)) + (kd2 < (2 < k ? 1 : 0)) + (kd3 < 0);
    // in-range candidates of the quad: the quad's four bits of one ballot
    const int nin = __builtin_popcount((unsigned)(__builtin_amdgcn_ballot_w64(in) >> (lane & ~3)) & 0xfu);
    const int nl = nin < c.orca_max_neighbors ? nin : c.orca_max_neighbors;
    float4 mine;
    if constexpr (Path::slim) {
        const float4 ud = orca_u_dir_rel<Path::straight>(ddx, ddy, d, fvx, fvy, frad, o, orad, inv_th, inv_ts, in);
        mine = make_float4(fvx + 0.5f * ud.x, fvy + 0.5f * ud.y, ud.z, ud.w);          // as orca_line_select
    } else {
        mine = orca_line_select(fpx, fpy, fvx, fvy, frad, o, orad, inv_th, inv_ts, in);
    }
    // route my half-plane to lane `rank` of the quad, then share all four
    float4 srt, L[4];
    [[maybe_unused]] float4 lnA, liA;                            // lp1_spread's pass A operands (Path::spread)
    if constexpr (Path::table) {
        path.tab[(lane & ~3) | rank] = mine;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const float4 *quad = path.tab + (lane & ~3);
        L[0] = quad[0]; L[1] = quad[1]; L[2] = quad[2]; L[3] = quad[3];
        srt = path.tab[lane];
        if constexpr (Path::spread) {
            // lane 0 of the quad: lines 3 and 2; lanes 1 - 3: their own line and line 0.  Two more reads at addresses
            // that do not change from step to step, issued with the five above
            lnA = path.tab[k == 0 ? (lane | 3) : lane];
            liA = quad[k == 0 ? 2 : 0];
        }
    } else {
        const int dst = ((lane & ~3) | rank) << 2;
        srt.x = __builtin_bit_cast(float, __builtin_amdgcn_ds_permute(dst, __builtin_bit_cast(int, mine.x)));
        srt.y = __builtin_bit_cast(float, __builtin_amdgcn_ds_permute(dst, __builtin_bit_cast(int, mine.y)));
        srt.z = __builtin_bit_cast(float, __builtin_amdgcn_ds_permute(dst, __builtin_bit_cast(int, mine.z)));
        srt.w = __builtin_bit_cast(float, __builtin_amdgcn_ds_permute(dst, __builtin_bit_cast(int, mine.w)));
    }
    // the starting point of the take steps, the clipped preferred velocity, first: it depends on no half-plane, so it
    // is computed while the ds_permutes (the table's reads) are in flight
    {
        const float pp = dot2(prefx, prefy, prefx, prefy);
        const bool clip = pp > ms * ms;
        const float inv = rcp_sqrt_f32<Path::straight>(pp, clip);
        rx = clip ? ms * (prefx * inv) : prefx;
        ry = clip ? ms * (prefy * inv) : prefy;
    }
    if constexpr (!Path::table) {
        L[0] = qb4<0>(srt); L[1] = qb4<1>(srt); L[2] = qb4<2>(srt); L[3] = qb4<3>(srt);
    }

    // speculative 1-D LPs, one per lane (lane k's line L[k] is its own `srt`); then the incremental LP is four
    // compare-and-take steps
    float cx, cy;
    // lane k's code for the take steps below: 4 when its 1-D LP is feasible, else k (the 2-D LP fails at line k)
    bool ok1;
    if constexpr (Path::spread) ok1 = lp1_spread<Path::slim, Path::straight>(srt, lnA, liA, L[1], k, ms, prefx, prefy, cx, cy);
    else ok1 = lp1_rt<false, Path::slim>(L, srt, k, ms, prefx, prefy, cx, cy);
    const int fcode = ok1 ? 4 : k;
    // `fail` stays nl until a violated line's 1-D LP is infeasible and then is that line, so "line I is below nl and
    // nothing failed yet" is fail > I; a violation folds the line's code in (min: nl <= 4 keeps a feasible line's 4
    // from changing it), and the candidate is taken where fail is still above I afterwards
    int fail = nl;
    if constexpr (Path::lean_take) {
        // the same four steps, each deciding from min(fail, code_i), which is known before the step's test: behind the
        // compare one mask AND and the selects (take_step_lean: the same `fail` and the same `take` on every input)
        MCN_TAKE_LEAN(0, L[0]) MCN_TAKE_LEAN(1, L[1]) MCN_TAKE_LEAN(2, L[2]) MCN_TAKE_LEAN(3, L[3])
    } else {
#define MCN_LP2_TAKE(I)                                                                        \
        {                                                                                      \
            const int code_i = qbi<I>(fcode); const float cx_i = qbf<I>(cx), cy_i = qbf<I>(cy); \
            const bool out = det2(L[I].z, L[I].w, L[I].x - rx, L[I].y - ry) > 0.0f;             \
            fail = ((fail > I) & out) ? min(fail, code_i) : fail;                               \
            const bool take = (fail > I) & out;                                                 \
            rx = take ? cx_i : rx; ry = take ? cy_i : ry;                                       \
        }
        MCN_LP2_TAKE(0) MCN_LP2_TAKE(1) MCN_LP2_TAKE(2) MCN_LP2_TAKE(3)
#undef MCN_LP2_TAKE
    }
    // (not marked unlikely: with the round loop behind the step's text the headline measured nothing, and the changed
    //  block frequencies rearranged the unicycle form's float64 loop, +2 % per step: profiles/r32_rollout_branch_layout.txt)
    if (fail < nl) {
        // dense crowd: 3-D LP (RVO2 linearProgram3).  fail / nl / the running result are quad-uniform, so the
        // whole region is entered per quad and the quad broadcasts inside see all four lanes.  Per round: find
        // the next line from `i` on that the running result violates by more than `dist`, let the quad's four
        // lanes compute its candidate together, take it if valid, update `dist`.  Measured on the benchmark
        // workload: 0.65 % of the solves get here; 93 % of those need one round, 6 % two, 1 % three.
        DIAG_COUNT(0);
        // The next line is the first one from `i` on (below nl) that the running result violates by more than
        // `dist`: lane k tests ITS line (L[k] = srt, the same operations on the same values as every lane testing
        // L[k]) and the quad's four bits of a ballot name the first.
        float dist = 0.0f;
        int i = fail;
        for (;;) {
            // (the two tests' masks are combined on the scalar unit: as one bool it would be materialised first)
            const unsigned long long over = lanes((unsigned)(k - i) < (unsigned)(nl - i)) &
                                            lanes(det2(srt.z, srt.w, srt.x - rx, srt.y - ry) > dist);
            const unsigned m = (unsigned)(over >> (lane & ~3)) & 0xfu;
            if (m == 0) break;
            const int nxt = __builtin_ctz(m);
            float4 ln;
            if constexpr (Path::table) ln = path.tab[(lane & ~3) | nxt];      // one 16-byte read for sel4's 12 selects
            else ln = sel4(L, nxt);
            float cx3, cy3;
            const bool ok3 = lp3_candidate_quad<Path::lean_lp3, Path::straight>(ln, srt, nxt, k, ms, cx3, cy3);
            rx = ok3 ? cx3 : rx; ry = ok3 ? cy3 : ry;
            dist = det2(ln.z, ln.w, ln.x - rx, ln.y - ry);
            i = nxt + 1;
        }
    }
}

#undef MCN_TAKE_LEAN

}  // namespace mcn
