"""CPU: the host replay of mcn_orca_finish (tests/orca_finish_ref.py) against the reference's own get_human_times()
results, and the conditions that make the GPU test's scenes (tests/test_orca_finish_gpu.py) worth running."""
import os

import numpy as np
import pytest

from oracle import cport
from tests import orca_finish_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_replay_reproduces_the_reference_get_human_times():
    """g16_orca_robot.npz holds what the real reference's CrowdSim.get_human_times() returned after six episodes in
    which the robot arrived: started from the last recorded state, the replay must give the same first-arrival times,
    end positions, clock and number of appended states, bit for bit.  v0_c0 is the zero-step case."""
    g = np.load(os.path.join(GOLDEN, "g16_orca_robot.npz"))
    st, vel = R.fixture_states(g)
    out = R.replay(st, vel)
    for e, key in enumerate(R.FIXTURE_CASES):
        assert np.array_equal(out["human_times"][e], g[key + "_human_times"]), key
        assert np.array_equal(out["rpos"][e], g[key + "_end_rob"][:2]), key
        assert np.array_equal(out["hpos"][e], g[key + "_end_hum"][:, :2]), key
        assert out["gtime"][e] == float(g[key + "_end_time"]), key
        assert g[key + "_states"].shape[0] + out["steps"][e] == int(g[key + "_n_states"]), key
    assert out["steps"].tolist() == [0, 9, 2, 10, 5, 7]
    # the zero-step env is returned as it came
    assert np.array_equal(out["sim_vel"][0], vel[0]) and np.array_equal(out["hpos"][0], st["hpos"][0])


@pytest.mark.parametrize("N,lo,hi,ranged", [(1, 32, 37, 12), (2, 34, 39, 12), (5, 40, 44, 12), (10, 49, 76, 12),
                                            (13, 56, 80, 4)])
def test_gpu_scenes_finish_unevenly_and_reach_the_3d_lp(N, lo, hi, ranged):
    """Circle crossing, `test` cases 0-11, robot on its goal: every scene finishes well below 200 steps, the scenes of
    one batch do not all take equally long (envs of one wavefront stop on different steps), and the N = 5 and N = 10
    batches enter RVO2's linearProgram3.  The step counts lie in the ranges recorded when the scenes were chosen; the
    N = 13 range (56-80) was recorded for cases 0-3, the one wavefront of the GPU test: the twelve cases take
    80 56 69 67 52 58 58 97 62 53 57 60 steps, which is a property of the scenes and the oracle alone."""
    st, vel = R.crossing_scenes(N, range(12))
    entries = []
    steps = []
    for e in range(12):
        one = {k: v[e:e + 1] for k, v in st.items()}
        cport.lp3_entries()
        out = R.replay(one, vel[e:e + 1], max_steps=200)
        entries.append(cport.lp3_entries())
        steps.append(int(out["steps"][0]))
        assert np.all(out["human_times"] != 0)
    print(N, steps, entries)
    assert max(steps) < 200 and len(set(steps)) > 1
    assert lo == min(steps[:ranged]) and max(steps[:ranged]) == hi, steps
    if N == 5:
        assert sum(1 for n in entries if n > 0) == 8
    if N == 10:
        assert all(n > 0 for n in entries)


def test_grid_scene_has_more_candidates_than_lines_and_enters_the_3d_lp():
    """The hand-made N = 32 scene of the GPU test: 8 capped steps, nobody arrives, the 3-D LP is entered."""
    st, vel = R.grid_scenes()
    cport.lp3_entries()
    out = R.replay(st, vel, max_steps=8)
    assert cport.lp3_entries() > 0
    assert out["steps"].tolist() == [8, 8] and np.all(out["human_times"] == 0)
    assert out["gtime"].tolist() == [2.0, 14.5]


def test_capped_replays_continue_to_the_same_result():
    """The contract's continuation rule on the replay itself: 7 + 13 + the rest equals one uncapped run."""
    st, vel = R.crossing_scenes(5, [3, 7])
    whole = R.replay(st, vel)
    cur, v, traj = {k: a.copy() for k, a in st.items()}, vel, [[], []]
    for cap in (7, 13, 8000):
        out = R.replay(cur, v, max_steps=cap)
        for k in ("hpos", "rpos", "gtime", "human_times"):
            cur[k] = out[k]
        v = out["sim_vel"]
        for e in range(2):
            traj[e].append(out["traj"][e])
    for k in ("hpos", "rpos", "gtime", "human_times", "sim_vel"):
        assert np.array_equal(whole[k], out[k]), k
    for e in range(2):
        assert np.array_equal(np.concatenate(traj[e]), whole["traj"][e])
