"""GPU: mcn_orca_finish (orca_finish.hip; CrowdSim.get_human_times, crowd_sim.py:219-258, for a batch in one launch)
through the C ABI against the reference's recorded results and the host replay (tests/orca_finish_ref.py), bit for bit,
and VecCrowdSim.get_human_times against E separate CrowdSim runs."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import orca_finish_ref as R  # noqa: E402

from tests.orca_finish_harness import HELD, WRITTEN, Batch, assert_matches, tiled  # noqa: E402

_crossing = {}


def crossing(N, E):
    """E envs on the circle-crossing test scenes i mod 12, and their replay (computed once per N for the distinct
    scenes; envs are independent)."""
    n = min(E, 12)
    if (N, n) not in _crossing:
        st, vel = R.crossing_scenes(N, range(n))
        _crossing[(N, n)] = (st, vel, R.replay(st, vel, max_steps=200))
    st, vel, ref = _crossing[(N, n)]
    idx = [i % 12 for i in range(E)]
    return {k: v[idx] for k, v in st.items()}, vel[idx], tiled(ref, idx)


def test_fixture_states_reach_the_reference_results(golden_dir):
    """The six arrived episodes of g16_orca_robot.npz as one batch (E = 6, N = 5; 0, 9, 2, 10, 5 and 7 steps): first
    arrival times, end positions and clocks are the real reference's."""
    g = np.load(os.path.join(golden_dir, "g16_orca_robot.npz"))
    st, vel = R.fixture_states(g)
    b = Batch(st, vel, 16)
    out = b.run(16)
    for e, key in enumerate(R.FIXTURE_CASES):
        assert np.array_equal(out["human_times"][e], g[key + "_human_times"]), key
        assert np.array_equal(out["rpos"][e], g[key + "_end_rob"][:2]), key
        assert np.array_equal(out["hpos"][e], g[key + "_end_hum"][:, :2]), key
        assert out["gtime"][e] == float(g[key + "_end_time"]), key
        assert g[key + "_states"].shape[0] + out["steps"][e] == int(g[key + "_n_states"]), key
    assert out["steps"].tolist() == [0, 9, 2, 10, 5, 7]
    H.assert_bits_equal(out["sim_vel"][0], vel[0], "zero-step env")
    b.untouched(out)
    assert_matches(out, R.replay(st, vel), "fixture")


@pytest.mark.parametrize("E,N", [(70, 5), (35, 1), (7, 10), (5, 13)])
def test_kernel_matches_replay(E, N):
    """Every output array against the host replay: seven wavefronts of ten envs whose envs stop on different steps
    (70 x 5), two agents per env (35 x 1), five envs and nine idle lanes per wavefront (7 x 10), more candidates than
    max_neighbors (5 x 13)."""
    st, vel, ref = crossing(N, E)
    assert len(set(ref["steps"][:64 // (N + 1)].tolist())) > 1          # the first wavefront's envs finish apart
    T = int(ref["steps"].max()) + 3
    b = Batch(st, vel, T)
    out = b.run(T)
    assert_matches(out, ref, "%d x %d" % (E, N))
    assert np.all(out["human_times"] != 0)
    b.untouched(out)


def test_kernel_matches_replay_on_a_full_wavefront_env():
    """E = 2, N = 32: one env per wavefront, 33 agents on a grid pushing through its centre, 8 capped steps."""
    st, vel = R.grid_scenes()
    ref = R.replay(st, vel, max_steps=8)
    b = Batch(st, vel, 8)
    out = b.run(8)
    assert_matches(out, ref, "grid")
    assert out["steps"].tolist() == [8, 8] and np.all(out["human_times"] == 0)
    b.untouched(out)


def test_capped_calls_continue_to_the_bytes_of_one_call():
    """max_steps = 7 leaves unfinished times at 0 and steps == 7; 7, then 13, then the rest leave the bytes of one
    uncapped call, and the traj pieces concatenate to its traj."""
    E, N = 12, 5
    st, vel, ref = crossing(N, E)
    T = int(ref["steps"].max()) + 3
    whole = Batch(st, vel, T).run(T)
    assert_matches(whole, ref, "uncapped")
    b = Batch(st, vel, T)
    pieces = [[] for _ in range(E)]
    for i, cap in enumerate((7, 13, T)):
        out = b.run(cap)
        if i == 0:
            assert out["steps"].tolist() == [7] * E and np.all(out["human_times"] == 0)
            assert_matches(out, R.replay(st, vel, max_steps=7), "capped at 7")
        if i == 1:
            assert out["steps"].tolist() == [13] * E
        for e in range(E):
            pieces[e].append(out["traj"][:out["steps"][e], e])
    for k in WRITTEN + ("sim_vel",):
        H.assert_bits_equal(out[k], whole[k], "continued " + k)
    for e in range(E):
        got = np.concatenate(pieces[e])
        assert len(got) == whole["steps"][e]
        H.assert_bits_equal(got, whole["traj"][:len(got), e], "continued traj of env %d" % e)
    b.untouched(out)


def test_unselected_and_finished_envs_keep_every_byte():
    """select == 0 and envs whose times are all set: nothing of them changes in st, sim_vel or traj, steps is 0; their
    neighbours in the wavefront are simulated as without them.  hvel / rvel / rtheta never change."""
    E, N = 12, 5
    st, vel, ref = crossing(N, E)
    st = {k: v.copy() for k, v in st.items()}
    st["human_times"][6] = 3.25                      # all set: nothing to do
    st["human_times"][8, :4] = [1.0, 2.0, 0.5, 4.0]  # one human left
    select = np.ones(E, np.uint8)
    select[[1, 4, 10]] = 0
    want = R.replay(st, vel, select=select, max_steps=200)
    assert want["steps"][6] == 0 and want["steps"][8] > 0
    T = int(want["steps"].max()) + 3
    b = Batch(st, vel, T)
    out = b.run(T, select=select)
    assert_matches(out, want, "select")
    for e in (1, 4, 6, 10):
        assert out["steps"][e] == 0
        for k in WRITTEN:
            H.assert_bits_equal(out[k][e], st[k][e], "idle env %d %s" % (e, k))
        H.assert_bits_equal(out["sim_vel"][e], vel[e], "idle env %d sim_vel" % e)
        assert np.all(out["traj"][:, e] == HELD)
    H.assert_bits_equal(out["human_times"][8, :4], st["human_times"][8, :4], "times already set")
    b.untouched(out)
    # without traj: the same state
    b2 = Batch(st, vel, T)
    out2 = b2.run(T, select=select, traj=False)
    for k in WRITTEN + ("sim_vel", "steps"):
        H.assert_bits_equal(out2[k], out[k], "no traj " + k)
    assert np.all(out2["traj"] == HELD)


def test_bad_arguments_are_rejected_before_any_launch():
    from modelcrowdnav_amd import _hip
    st, vel, _ = crossing(5, 2)
    b = Batch(st, vel, 4)
    sv, sp, tr, s = _hip.ptr(b.sim_vel), _hip.ptr(b.steps), _hip.ptr(b.traj), _hip.stream_ptr(b.dev)
    f = _hip.lib.mcn_orca_finish
    bad = [
        f(None, sv, None, 4, sp, tr, 0.25, 10.0, 10, 5.0, 2, 5, s),
        f(b.st, None, None, 4, sp, tr, 0.25, 10.0, 10, 5.0, 2, 5, s),
        f(b.st, sv, None, 4, None, tr, 0.25, 10.0, 10, 5.0, 2, 5, s),
        f(b.st, sv, None, 0, sp, tr, 0.25, 10.0, 10, 5.0, 2, 5, s),          # max_steps < 1
        f(b.st, sv, None, 4, sp, tr, 0.25, 10.0, 10, 5.0, 0, 5, s),          # E
        f(b.st, sv, None, 4, sp, tr, 0.25, 10.0, 10, 5.0, 2, 0, s),          # N
        f(b.st, sv, None, 4, sp, tr, 0.25, 10.0, 10, 5.0, 2, 33, s),
        f(b.st, sv, None, 4, sp, tr, 0.25, 10.0, 11, 5.0, 2, 5, s),          # max_neighbors > MCN_MAX_LINES
        f(b.st, sv, None, 4, sp, tr, 0.25, 10.0, -1, 5.0, 2, 5, s),
        f(b.st, sv, None, 4, sp, tr, 0.0, 10.0, 10, 5.0, 2, 5, s),           # time_step
        f(b.st, sv, None, 4, sp, tr, 0.25, 10.0, 10, 0.0, 2, 5, s),          # time_horizon
    ]
    for field in ("hpos", "hgoal", "hrad", "hvpref", "rpos", "rgoal", "rrad", "rvpref", "gtime", "human_times"):
        st_ = _hip.EnvState.from_buffer_copy(b.st)
        setattr(st_, field, None)
        bad.append(f(st_, sv, None, 4, sp, tr, 0.25, 10.0, 10, 5.0, 2, 5, s))
    assert bad == [_hip.MCN_EINVAL] * len(bad)
    # the velocity, heading and hcount fields are not part of the contract: NULL is accepted
    st_ = _hip.EnvState.from_buffer_copy(b.st)
    st_.hvel = st_.rvel = st_.rtheta = st_.hcount = None
    import torch
    assert f(st_, sv, None, 4, sp, tr, 0.25, 10.0, 10, 5.0, 2, 5, s) == _hip.MCN_OK
    torch.cuda.synchronize()
    assert b.steps.tolist() == [4, 4]


def test_vec_get_human_times_equals_separate_crowdsim_runs():
    """VecCrowdSim.get_human_times over a batch against CrowdSim.get_human_times (E = 1) on the same scenes: a few
    common steps first so that velocities are not zero, then the robots of envs 0-2 are put on their goals; env 3's
    robot has not arrived: it is left alone by default and raises when selected."""
    import torch
    from modelcrowdnav_amd import configs
    from modelcrowdnav_amd.envs import CrowdSim
    from modelcrowdnav_amd.envs.utils.action import ActionXY
    from modelcrowdnav_amd.envs.utils.robot import Robot
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    cases, N = [0, 3, 7, 11], 5
    env = H.make_vec_env(len(cases), N)
    env.reset("test", test_cases=cases)
    act = torch.tensor([[0.3, 0.4]] * len(cases), dtype=torch.float64, device=env.device)
    for _ in range(4):
        env.step(act)
    with pytest.raises(ValueError):
        env.get_human_times(envs=[0])
    times, steps = env.get_human_times()                         # nobody has arrived: nothing happens
    assert steps.tolist() == [0] * len(cases)
    env.rpos[:3] = env.rgoal[:3]
    before = {k: getattr(env, k).clone() for k in ("hpos", "hvel", "rpos", "rvel", "gtime", "human_times")}
    times, steps = env.get_human_times()
    assert times is env.human_times and steps[3] == 0 and bool((steps[:3] > 30).all())
    for k, v in before.items():
        assert torch.equal(getattr(env, k)[3], v[3]), k          # env 3: every byte as it was
        if k in ("hvel", "rvel"):
            assert torch.equal(getattr(env, k), v), k
    with pytest.raises(ValueError):
        env.get_human_times(envs=[1, 3])
    with pytest.raises(ValueError):
        env.get_human_times(envs=torch.tensor([False, False, False, True]))

    cfg = configs.env_config()
    one = CrowdSim()
    one.configure(cfg)
    robot = Robot(cfg, "robot")
    pol = policy_factory["orca"]()
    pol.configure(cfg)
    robot.set_policy(pol)
    one.set_robot(robot)
    for e, case in enumerate(cases[:3]):
        one.reset("test", case)
        for _ in range(4):
            one.step(ActionXY(0.3, 0.4))
        robot.set_position(robot.get_goal_position())
        n_states = len(one.states)
        got = one.get_human_times()
        assert got == times[e].tolist() and all(x > 0 for x in got), case
        assert one.global_time == float(env.gtime[e]) and len(one.states) == n_states + int(steps[e])
        assert [h.get_position() for h in one.humans] == [tuple(p) for p in env.hpos[e].tolist()]
        assert robot.get_position() == tuple(env.rpos[e].tolist())
