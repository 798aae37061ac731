// quad_take_probe.cpp -- csrc/quad_take_plan.hpp from the outside, with the host compiler alone (no HIP, no GPU).
//
// Replays the take steps of the quad-parallel incremental LP over every input: the four-line form of the 2-D LP (nl = 0 ..
// 4, F = the lines whose speculative 1-D LP is infeasible, and line I's test against the starting point and against the
// candidates of lines 0, 1, 2 as four nibbles: 5 x 16 x 2^16 inputs) and the three-line form the 3-D LP's candidate uses
// (three lines, `fail` starting at 3; bit 3 of every nibble and the fourth nibble are garbage that must not matter).
// The running point is an index here (-1: the starting point, else the line whose candidate it is) and `out` the bit of
// that point's nibble.  Each input runs once with take_step_guarded, the literal transcription of MCN_LP2_TAKE /
// MCN_LP3_INNER_TAKE, and once with take_step_lean; `fail` and the running point must agree AFTER EVERY STEP, and the
// first difference fails.  Prints one line per form and nl: "<lines> <nl> <inputs> <ended at the start> <at c_0> <at c_1>
// <at c_2> <at c_3> <failed>", which the test holds against counts derived without either function.
#include <cstdio>
#include "../modelcrowdnav_amd/csrc/quad_take_plan.hpp"

using namespace mcn;

static int run(int lines, int nl_lo, int nl_hi)
{
    for (int nl = nl_lo; nl <= nl_hi; ++nl) {
        long n = 0, at[5] = {0, 0, 0, 0, 0}, failed = 0;
        for (unsigned F = 0; F < 16; ++F)
            for (unsigned v = 0; v < (1u << 16); ++v) {
                const unsigned V[4] = {v & 15u, (v >> 4) & 15u, (v >> 8) & 15u, (v >> 12) & 15u};
                int fail_g = nl, cur_g = -1, fail_l = nl, cur_l = -1;
                for (int I = 0; I < lines; ++I) {
                    const int code_i = ((F >> I) & 1u) ? I : 4;  // fcode: 4 when the line's 1-D LP is feasible, else the line
                    const TakeStep g = take_step_guarded(fail_g, code_i, ((V[cur_g + 1] >> I) & 1u) != 0, I);
                    const TakeStep l = take_step_lean(fail_l, code_i, ((V[cur_l + 1] >> I) & 1u) != 0, I);
                    fail_g = g.fail; cur_g = g.take ? I : cur_g;
                    fail_l = l.fail; cur_l = l.take ? I : cur_l;
                    if (fail_g != fail_l || cur_g != cur_l) {
                        std::fprintf(stderr, "lines=%d nl=%d F=%#x V=%#x %#x %#x %#x after step %d: guarded (point %d, fail %d), "
                                     "lean (point %d, fail %d)\n", lines, nl, F, V[0], V[1], V[2], V[3], I, cur_g, fail_g, cur_l, fail_l);
                        return 1;
                    }
                }
                ++n; ++at[cur_g + 1]; failed += fail_g < nl;
            }
        std::printf("%d %d %ld %ld %ld %ld %ld %ld %ld\n", lines, nl, n, at[0], at[1], at[2], at[3], at[4], failed);
    }
    return 0;
}

// both steps are constant expressions: the device code compiles the function this probe replays
static_assert(take_step_lean(4, 4, true, 1).take && take_step_lean(4, 4, true, 1).fail == 4, "a feasible violated line is taken");
static_assert(!take_step_lean(4, 2, true, 2).take && take_step_lean(4, 2, true, 2).fail == 2, "an infeasible one fails there");
static_assert(!take_step_lean(1, 4, true, 2).take && take_step_lean(1, 4, true, 2).fail == 1, "nothing moves after a failure");

int main()
{
    if (run(4, 0, 4)) return 1;
    return run(3, 3, 3);
}
