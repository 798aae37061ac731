// quad_take_plan.hpp -- one compare-and-take step of the quad-parallel incremental LP (quad_common.hpp: the 2-D LP of
// quad_orca_core), as the decision it makes from integers and one boolean.  Plain constexpr C++ with no HIP in it, so that
// a stand-alone program can include it with the host compiler (tests/quad_take_probe.cpp) and replay every input.
//
// Step I of the sequence tests line I against the running point (`out`: the point violates it).  `fail` starts at nl, the
// number of lines, stays there until a violated line's speculative 1-D LP is infeasible and then is that line; code_i is
// line I's verdict, 4 when its 1-D LP is feasible and I when not.  A step returns the new `fail` and whether the running
// point moves to line I's candidate.
#pragma once

namespace mcn {

struct TakeStep {
    int fail;
    bool take;
};

constexpr int take_min(int a, int b) { return a < b ? a : b; }

// The step as every caller but the four-wavefront rollout form has it (MCN_LP2_TAKE): "line I is below nl and nothing
// failed yet" is fail > I; a violation folds the line's code in (min: nl <= 4 keeps a feasible line's 4 from changing
// it), and the candidate is taken where fail is still above I afterwards.
constexpr TakeStep take_step_guarded(int fail, int code_i, bool out, int I)
{
    const int f = ((fail > I) & out) ? take_min(fail, code_i) : fail;
    return TakeStep{f, bool((f > I) & out)};
}

// The same decision with less between the test and the select (Path::lean_take).
//   * The guard fail > I on the fold is not needed: code_i is I or 4, never below I, so where fail <= I the minimum is
//     fail itself.
//   * The minimum does not depend on this step's test, only on the steps before, and where `out` holds it IS the new
//     fail: "still above I afterwards" can be asked of the minimum, beside the test instead of behind it.
// So behind the step's compare there is one mask AND and the selects, where the guarded form has a compare, an AND, a
// select, a second compare and a second AND; and the step is two instructions shorter.
constexpr TakeStep take_step_lean(int fail, int code_i, bool out, int I)
{
    const int mn = take_min(fail, code_i);
    return TakeStep{out ? mn : fail, bool((mn > I) & out)};
}

}  // namespace mcn
