"""The 1-D LP's six intersections spread over the quad (quad_common.hpp: lp1_spread; env_rollout_wg4_kernel,
rollout_split = 2).

In the four-wavefront rollout form lane 0 of a quad, whose own 1-D LP has no earlier line, computes the intersection of
the quad's line 3 with line 2 from two table slots, and lane 3 takes (t, den, num) from it by three quad broadcasts and
applies it as its third bound update.  Every other kernel keeps the three-pass form.  What can go wrong there and
nowhere else:

  * the helper lane reads the wrong slots, or the consumer takes the values of the wrong lane or applies them in the
    wrong order: every state of pair (3, 2) -- tr lowered, tl raised, parallel and infeasible (the 3-D LP starts at line
    3), parallel and a no-op, the interval emptied by exactly this pair;
  * NaN half-planes at ranks 2 and 3 (the moved values are NaN: bits, not numbers, must arrive);
  * fewer than four candidates in range: ranks 2 and 3 hold lines that are not part of the LP, the helper computes on them;
  * the 3-D LP behind a 2-D LP that failed at line 3: a round on line 3 where projected line 1 moves a bound of projected
    line 2's LP, and a round on line 2, where that pair is dead (the same deal one level down was built on these two and
    measured no gain; whoever tries it again finds the states here);
  * quads that straddle two wavefronts, idle quads, a partial last workgroup, every launch length and cut.

tests/lp1_spread_states.py puts each of these into envs 0 .. 18 and proves from the C oracle on the CPU that they are
there (test_batch_holds_every_state_of_the_pair, no GPU).  The GPU test compares BYTES: full state, step record, Explorer
records and finished-episode arrays of the forced four-wavefront form after EVERY launch against single mcn_env_step
calls at that step, for the first T = 1, 2, 3, 8 steps of one sequence cut at every position, and forms 1 and 0 at the end.
"""
import numpy as np
import pytest

from oracle import cport
from tests import helpers as H
from tests import lp1_spread_states as S
from tests.rollout_harness import every_cut, launches_against, single_steps

SHAPES = (1, 8, 9, 19)
LENGTHS = (1, 2, 3, 8)


@pytest.mark.parametrize("E", SHAPES)
def test_batch_holds_every_state_of_the_pair(E):
    """No GPU: the oracle's replay of the batch shows every situation the GPU test is about inside the first 8 steps; the
    lone env of E = 1 holds a lowered tr, taken, on step 0."""
    ev = S.replay(E)["events"]
    first = {k: (int(np.argmax(v.any((1, 2)))) if v.any() else None) for k, v in ev.items()}
    print("E = %d, first step of each situation: %s" % (E, first))
    assert ev[S.S_TR][0, 0].any(), "env 0, step 0: pair (3, 2) lowers no tr of a line-3 candidate that is taken"
    if E >= 8:
        for k in (S.S_TR, S.S_TL, S.S_PAR_NEG, S.S_PAR_OK, S.S_EMPTY, S.S_NAN2, S.S_NAN3, S.S_FEWER, S.S_LP3_21,
                  S.S_LP3_ON2):
            assert ev[k].any(), "no solve with %s in the first %d steps" % (k, S.T_MAX)
        # on the first step too, where the one-step launches see them
        for k in (S.S_PAR_NEG, S.S_PAR_OK, S.S_NAN2, S.S_NAN3, S.S_FEWER, S.S_LP3_21, S.S_LP3_ON2):
            assert ev[k][0].any(), "no solve with %s on step 0" % k
        # env 3 of a workgroup straddles ORCA wavefronts 0 and 1, env 6 wavefronts 1 and 2
        assert ev[S.S_FEWER][:, 3].any() and (ev[S.S_TR][:, 6].any() or ev[S.S_TL][:, 6].any())
    if E >= 9:
        assert (ev[S.S_TR] | ev[S.S_TL] | ev[S.S_LP3_21])[:, 8:].any(), "nothing in the partial last workgroup"
    if E >= 19:
        for k in (S.S_TR, S.S_TL, S.S_EMPTY):
            assert ev[k][0].any(), "no solve with %s on step 0" % k


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
@pytest.mark.parametrize("E", SHAPES)
def test_spread_lp1_equals_single_steps(E, kinematics, tuning):
    """The first 1, 2, 3 and 8 steps of one sequence, cut at every position: the four-wavefront form leaves the bytes of
    the single steps after every launch, forms 1 and 0 at the end; the single steps are the oracle's (whose replay holds
    every state of pair (3, 2): test_batch_holds_every_state_of_the_pair)."""
    tuning(rollout_fused=1)
    st, acts = S.batch(E)

    def build():
        env = H.make_vec_env(E, S.N, kinematics=kinematics)
        H.upload(env, st)
        env.attach_rollout(gamma=0.9, pool=None, fin_slots=2)
        return env
    env, snaps, _, _ = single_steps(build, acts)
    want = S.replay(E)["states"][-1]
    # (the replay's robot is holonomic; the humans never see it)
    fields = None if kinematics == "holonomic" else cport.EnvState.FIELDS_H
    kw = {} if fields is None else {"fields": fields}
    H.assert_state_equal(H.download(env), want, what="single steps against the oracle, E=%d" % E, **kw)
    what = "spread 1-D LP %s E=%d" % (kinematics, E)
    for T in LENGTHS:
        for cuts in every_cut(T):
            launches_against(build, acts, 2, cuts, snaps, what)
        for split in (1, 0):
            launches_against(build, acts, split, (0, T), snaps, what)
