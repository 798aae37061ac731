"""The four-wavefront rollout form (env_rollout_wg4_kernel, rollout_split = 2) with its range guards computing the fast
values first and replacing them under a branch marked unlikely, the IEEE expansions behind the step's text
(quad_common.hpp: Path::straight): one mcn_env_rollout launch against the same steps taken one mcn_env_step at a time,
byte for byte.  The single-step kernel keeps the guards' `if fast / else IEEE` form.

Either arm of a guard writes the same bits for operands inside the fast range, so a byte can only differ where an arm is
wrong or where the IEEE arm, which now OVERWRITES the fast values on every lane, misses one.  The batteries therefore
send each of the five guard sites down its IEEE arm beside quads that hold ordinary values, and down its fast arm:

  hp    relative velocity = rp / time_step on an overlapping pair: |w|^2 = 0 on a used cut-off-circle lane (_w_zero);
  clip  a goal 2^70 away: |pref|^2 overflows, the clip is active (_far_goal);
  lp1   a half-plane tangent to the speed disc, discriminant exactly 0 (_disc_zero: a neighbour 0.5 away at rest pushes the
        line to (-0.25, 0), v_pref = 0.25), and a discriminant of 2^-104 (_disc_tiny: a neighbour exactly at the radii's
        sum puts the line through the origin, v_pref = 2^-52);
  lp3r, lp3s  the 3-D LP candidate's 1 / |dd| and discriminant: envs of tests/edge_states.py whose 2-D LP fails, with a NaN
        half-plane (block `coincident`) and with a projected line tangent to the disc (block `searched-lp3-tangent`).

The other envs come from the ORCA-edge batch too (overlapping, far-apart, parallel-same-lp3, ...).  Which arm every
wavefront of every step takes is restated on the host (tests/guard_arm_states.py, idle quads included) and asserted BEFORE
anything is launched: per battery each site takes the IEEE arm in at least one wavefront-step and the fast arm in at
least one, and a forcing quad sits beside ordinary ones.  E = 8, 9 and 17 (one workgroup, a partial second, three), 5
humans, 6 steps, both robot kinematics; every forced launch asserts mcn_last_rollout_form() == 2."""
import functools

import numpy as np
import pytest

from tests import edge_states as ES
from tests import guard_arm_states as GA
from tests import helpers as H
from tests.rollout_harness import launches_against, random_actions, single_steps

N, T = 5, 6
HR = ES.HR                       # (float)(HR + 0.01) = 0.3125: the radii's sum is 0.625


def _put(st, e, pos, goal, vel=None, vpref=None):
    pos, goal = np.asarray(pos, np.float64), np.asarray(goal, np.float64)
    st.hpx[e], st.hpy[e], st.hgx[e], st.hgy[e] = pos[:, 0], pos[:, 1], goal[:, 0], goal[:, 1]
    vel = np.zeros((N, 2)) if vel is None else np.asarray(vel, np.float64)
    st.hvx[e], st.hvy[e] = vel[:, 0], vel[:, 1]
    st.hr[e] = HR
    st.hvpref[e] = 1.0 if vpref is None else np.asarray(vpref, np.float64)
    st.human_times[e] = 0


_FAR = [(0, 4), (-4, 0), (0, -4)]                 # three ordinary humans around the pair, walking to the other side
_FAR_GOAL = [(0, -4), (4, 0), (0, 4)]


def _w_zero(st, e):              # 0.125 apart (overlapping), v_0 - v_1 = (0.5, 0) = rp / 0.25: w = (0, 0) on both lanes
    _put(st, e, [(0, 0), (0.125, 0)] + _FAR, [(-4, 0), (4, 0)] + _FAR_GOAL, vel=[(0.5, 0), (0, 0), (0, 0), (0, 0), (0, 0)])


def _far_goal(st, e):            # human 1's goal is 2^70 away
    _put(st, e, [(2, 0), (-2, 0)] + _FAR, [(-2, 0), (2.0 ** 70, 0)] + _FAR_GOAL)


def _disc_zero(st, e):           # u = (4 * 0.625 - 4 * 0.5) * (-1, 0): human 0's line is ((-0.25, 0), (0, 1)), its speed 0.25
    _put(st, e, [(0, 0), (0.5, 0)] + _FAR, [(-4, 0), (4, 0)] + _FAR_GOAL, vpref=[0.25, 1, 1, 1, 1])


def _disc_tiny(st, e):           # u = 0: human 0's line goes through the origin, its discriminant is v_pref^2 = 2^-104
    _put(st, e, [(0, 0), (0.625, 0)] + _FAR, [(-4, 0), (4, 0)] + _FAR_GOAL, vpref=[2.0 ** -52, 1, 1, 1, 1])


# env of the battery -> env of the supplemented edge batch, or a scene.  Wavefronts of a workgroup hold envs 0 - 2, 3 - 5,
# 6 - 7: every scene shares its wavefront with envs of the edge batch.
OVERLAPPING, COINCIDENT, FAR_APART, TANGENT, PARALLEL = 96, 120, 160, 192, 629
LAYOUT = [OVERLAPPING, _w_zero, COINCIDENT,   PARALLEL, _far_goal, _disc_zero,   TANGENT, _disc_tiny,
          COINCIDENT + 4, _disc_zero, FAR_APART + 1,   PARALLEL + 1, _far_goal, OVERLAPPING + 1,   TANGENT, _w_zero,
          COINCIDENT + 1]


@functools.lru_cache(maxsize=None)
def _start(E):
    src, _, _, names = ES.with_supplement(ES.edge_batch(N, False))
    for e, block in ((OVERLAPPING, "overlapping"), (COINCIDENT, "coincident"), (FAR_APART, "far-apart"),
                     (TANGENT, "searched-lp3-tangent"), (PARALLEL, "parallel-same-lp3")):
        assert names[e] == block, (e, names[e])
    st = ES.take(src, [x if isinstance(x, int) else FAR_APART for x in LAYOUT[:E]])
    for e, x in enumerate(LAYOUT[:E]):
        if not isinstance(x, int):
            x(st, e)
    return st


@functools.lru_cache(maxsize=None)
def _battery(E, kinematics):
    """(start state, actions, arms per step, arm counts, mixed): the host's restatement, once per battery"""
    st = _start(E)
    acts = random_actions(kinematics, T, E, 5)
    # the humans do not see the robot and nothing restarts: their states, and so the arms, are those of a holonomic replay
    per_step, mixed = GA.arms(ES.oracle_cfg(False), st, random_actions("holonomic", T, E, 5))
    return st, acts, per_step, GA.arms_taken(per_step), mixed


def _assert_both_arms(E, kinematics):
    _, _, per_step, taken, mixed = _battery(E, kinematics)
    print("E=%d %s: wavefront-steps per arm %s; forcing quad beside ordinary ones %s" % (E, kinematics, taken, mixed))
    for site in GA.SITES:
        assert taken[site]["ieee"] >= 1, ("no wavefront-step takes the IEEE arm", site, taken)
        assert taken[site]["fast"] >= 1, ("no wavefront-step takes the fast arm", site, taken)
    assert any(mixed.values()), mixed
    # the scenes act on the first step, each on the site it is written for
    first = per_step[0]
    assert first[(0, 0)]["hp"] == "ieee" and first[(0, 1)]["clip"] == "ieee" and first[(0, 1)]["lp1"] == "ieee"
    assert first[(0, 2)]["lp1"] == "ieee" and first[(0, 2)]["lp3s"] == "ieee" and first[(0, 0)]["lp3r"] == "ieee"
    assert first[(0, 1)]["hp"] == "fast" and first[(0, 2)]["hp"] == "fast" and first[(0, 0)]["clip"] == "fast"
    assert mixed["hp"] and mixed["clip"] and mixed["lp1"]


def test_the_scenes_force_the_sites_they_are_written_for():
    """No GPU: each scene alone, human by human (the half-plane scene also forces lp1 -- its line is NaN in the oracle too --
    the others force one site each)."""
    cfg = ES.oracle_cfg(False)
    st = _start(8)
    inv_th, inv_ts = np.float32(1) / np.float32(cfg.orca_time_horizon), np.float32(1) / np.float32(cfg.time_step)
    want = {1: {"hp", "lp1"}, 4: {"clip"}, 5: {"lp1"}, 7: {"lp1"}}
    for e, sites in want.items():
        got = set()
        for i in range(N):
            q = GA._real_quad(cfg, st, e, i, inv_th, inv_ts)
            got |= {s for s in ("hp", "clip", "lp1") if q[s]}
            assert not q["unknown"], (e, i)
        assert got == sites, (e, got, sites)
    q = GA._real_quad(cfg, st, 5, 0, inv_th, inv_ts)
    line, *_ = GA.half_plane(np.float32(0), np.float32(0), np.float32(0), np.float32(0), np.float32(0.3125), np.float32(0.5),
                             np.float32(0), np.float32(0), np.float32(0), np.float32(0.3125), inv_th, inv_ts)
    assert GA.disc_of(line, np.float32(0.25)) == 0 and q["lp1"]
    line, *_ = GA.half_plane(np.float32(0), np.float32(0), np.float32(0), np.float32(0), np.float32(0.3125), np.float32(0.625),
                             np.float32(0), np.float32(0), np.float32(0), np.float32(0.3125), inv_th, inv_ts)
    assert GA.disc_of(line, np.float32(2.0 ** -52)) == np.float32(2.0 ** -104)


@pytest.mark.parametrize("E", [8, 9, 17])
def test_every_site_takes_both_arms_on_the_host(E):
    """No GPU: what the byte test below rests on (it asserts the same before it launches)."""
    _assert_both_arms(E, "holonomic")


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
@pytest.mark.parametrize("E", [8, 9, 17])
def test_one_launch_leaves_the_bytes_of_single_steps(E, kinematics, tuning):
    _assert_both_arms(E, kinematics)
    tuning(rollout_fused=1)
    st, acts, _, _, _ = _battery(E, kinematics)

    def build():
        env = H.make_vec_env(E, N, kinematics=kinematics)
        H.upload(env, st)
        return env

    _, snaps, _, _ = single_steps(build, acts)
    launches_against(build, acts, 2, (0, T), snaps, "straight-line step %s E=%d" % (kinematics, E))
    launches_against(build, acts, 2, (0, 1, T), snaps, "straight-line step %s E=%d" % (kinematics, E))
