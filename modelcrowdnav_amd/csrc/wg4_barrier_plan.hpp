// wg4_barrier_plan.hpp -- the workgroup barriers of the four-wavefront rollout form (env_rollout_wg4.hip): which ones a
// role executes, and how often, before its first step and on a step.  Plain constexpr C++ with no HIP in it, so that a
// stand-alone program can include it with the host compiler (tests/wg4_barrier_probe.cpp); both step loops of the
// kernel take every count from here and write none down themselves.
//
// The kernel synchronises with s_barrier alone, and a barrier completes when all four wavefronts of the workgroup have
// arrived: a role that executes one barrier more or fewer than another hangs the workgroup or pairs a hand-off with the
// wrong barrier.  So the two roles must execute the same barriers in the same order on every sequence of restart flags.
#pragma once

namespace mcn {

enum Wg4Role { kWg4Orca, kWg4Float64 };

// Barriers in the order a launch meets them.
//   seed     once, before step 0: the float64 wavefront has written every operand of the first solve (positions and goals
//            to the staging slots, velocities to s_res, frad / maximum speed to s_inv) and set every env's flag.
//   handoff  every step: the ORCA wavefronts have published the step's velocities to s_res[t & 1], the float64 wavefront
//            the step's restart flags to s_flag[t & 1].
//   staged   restart steps only (some env of the workgroup restarts), behind the hand-off: the restart lanes of the
//            float64 wavefront have staged their new humans; the ORCA wavefronts re-read their operands behind it.
struct Wg4StepBarriers {
    int seed, handoff, staged;
    constexpr int total() const { return seed + handoff + staged; }
};

// What `role` executes on a step.  `first`: step 0 of the launch; `restart`: the step's workgroup flag; `last`: the
// launch's last step.  Both roles execute a restart step's staged barrier inside that step, the last step's too (the
// ORCA wavefronts re-read operands nobody uses there: once per launch, and no barrier is left over behind a loop), so the
// answer depends on neither `role` nor `last`; they are arguments because the probe asks per role and per position.
constexpr Wg4StepBarriers wg4_step_barriers(Wg4Role role, bool first, bool restart, bool last)
{
    (void)role; (void)last;
    return Wg4StepBarriers{first ? 1 : 0, 1, restart ? 1 : 0};
}

}  // namespace mcn
