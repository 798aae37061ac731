// wg4_barrier_probe.cpp -- csrc/wg4_barrier_plan.hpp from the outside, with the host compiler alone (no HIP, no GPU).
//
// Replays the two step loops of env_rollout_wg4_kernel as far as barriers go: a role executes its `seed` barriers before
// step 0 and, on step t, its `handoff` barriers and then its `staged` ones, each count taken from wg4_step_barriers with
// the step's restart flag -- nothing else in the kernel executes a workgroup barrier.  For every sequence of restart
// flags of length 1 .. 6 it checks that the ORCA role and the float64 role have executed the same barriers, in the same
// order, after every step and at kernel exit (a difference is a hang or a hand-off paired with the wrong barrier), and
// that a step never has more than one barrier of a kind.  Prints one line per length: "<T> <sequences> <barriers>",
// the barriers summed over the sequences, which the test holds against T + 1 per launch plus one per restart step.
#include <cstdio>
#include <string>
#include "../modelcrowdnav_amd/csrc/wg4_barrier_plan.hpp"

using namespace mcn;

// the barriers `role` has executed when step `upto` (inclusive) of `flags` is over: s = seed, h = hand-off, r = staged
static std::string executed(Wg4Role role, unsigned flags, int T, int upto)
{
    std::string seq;
    for (int t = 0; t <= upto; ++t) {
        const bool restart = (flags >> t) & 1;
        const Wg4StepBarriers first = wg4_step_barriers(role, true, false, false);
        if (t == 0) seq.append(first.seed, 's');                  // before the loop, as the kernel has it
        const Wg4StepBarriers plan = wg4_step_barriers(role, false, restart, t + 1 == T);
        if (plan.seed != 0) return "seed inside the loop";
        seq.append(plan.handoff, 'h');
        seq.append(plan.staged, 'r');
    }
    return seq;
}

int main()
{
    for (int T = 1; T <= 6; ++T) {
        long total = 0;
        for (unsigned flags = 0; flags < (1u << T); ++flags) {
            for (int t = 0; t < T; ++t) {
                const std::string o = executed(kWg4Orca, flags, T, t), f = executed(kWg4Float64, flags, T, t);
                if (o != f) {
                    std::fprintf(stderr, "T=%d flags=%#x after step %d: ORCA %s, float64 %s\n", T, flags, t, o.c_str(), f.c_str());
                    return 1;
                }
                const bool restart = (flags >> t) & 1;
                const Wg4StepBarriers plan = wg4_step_barriers(kWg4Orca, false, restart, t + 1 == T);
                if (plan.handoff != 1 || plan.staged != (restart ? 1 : 0)) {
                    std::fprintf(stderr, "T=%d flags=%#x step %d: %d hand-off, %d staged barriers\n", T, flags, t,
                                 plan.handoff, plan.staged);
                    return 1;
                }
            }
            // kernel exit: nothing follows either loop
            const std::string o = executed(kWg4Orca, flags, T, T - 1), f = executed(kWg4Float64, flags, T, T - 1);
            if (o != f || o.empty() || o[0] != 's') {
                std::fprintf(stderr, "T=%d flags=%#x at exit: ORCA %s, float64 %s\n", T, flags, o.c_str(), f.c_str());
                return 1;
            }
            total += (long)o.size();
        }
        std::printf("%d %u %ld\n", T, 1u << T, total);
    }
    return 0;
}
