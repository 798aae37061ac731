"""GPU: the closed loop with an ORCA robot over social-force pedestrians (mcn_env_rollout_orca_sf, env_step.hip:
env_step_loop_orca_sf_kernel, VecCrowdSim.rollout_orca, the automatic path of VecExplorer.run_k_episodes).

  device against device, every byte, no tolerance: one T-step launch against the per-step sequence it replaces,
  ORCA.predict_batch -> env.step (mcn_env_step_sf), through both forms of the single-step kernel; split launches; the
  Explorer's automatic path against closed_loop=False;

  device against the host, step by step from the trace (tests/closed_loop_sf_ref.py): the robot's action bit for bit
  against the oracle's float32 ORCA solve, the humans' velocities within 8 * 2^-52 * M of the definition's restatement,
  everything after the velocities bit for bit against the oracle's given-velocity step and the mcn_rollout replay.

test_each_step_against_the_host prints the largest velocity error / tolerance it met and the smallest distance from a
threshold of the reward ladder."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cport  # noqa: E402
from tests import closed_loop_ref as CR  # noqa: E402
from tests import closed_loop_sf_ref as F  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import rollout_ref as R  # noqa: E402
from tests.rollout_harness import need_gpu  # noqa: E402
from tests.test_closed_loop_gpu import (E, GAMMA, TRACES, _assert_equal_envs, _assert_equal_traces,  # noqa: E402
                                        _assert_same_run, _per_step, _robot_policy, _target)

KERNEL = "env_step_loop_orca_sf_kernel"
SF_ENV = {"humans.policy": "socialforce"}
STATE_FIELDS = H.STATE_FIELDS + ("rtheta",)
COUNTS = (1, 5, 10, 32)


def _make(N, visible, time_limit, max_neighbors, count_hh=True):
    """tests/test_closed_loop_gpu.py's env with social-force humans: E test cases with return accounting and pool
    restarts attached (random attributes: a restart changes the radii) and an ORCA robot policy of safety space 0.15.
    Deterministic: two calls give two envs in the same state with equal buffers."""
    from modelcrowdnav_amd.envs import scenarios as S
    over = dict(SF_ENV, **{"env.time_limit": time_limit, "env.randomize_attributes": "true"})
    if N > 10:
        over["sim.circle_radius"] = 8.0           # room for 32 humans on the circle
    env = H.make_vec_env(E, N, robot_visible=visible, **over)
    assert env.human_policy_name == "socialforce"
    env.count_hh = bool(count_hh)
    pol = _robot_policy(max_neighbors)
    env.robot.set_policy(pol)
    if N >= 10:                                   # (the device generator's rejection loops stop: crowd_sim.device_pool)
        pool = env.device_pool(seed=5, first_case=0, count=2 * E, human_num=N)
        env.load_device_scenarios(pool, list(range(E)))
    else:
        pool = S.scenario_pool(env.spec(), "test", list(range(2 * E)), N, "circle_crossing")
        env.load_scenarios(pool[:E])
    bufs = env.attach_rollout(GAMMA, pool=pool, case_stride=E % (2 * E), first_cases=np.arange(E, 2 * E), fin_slots=3,
                              danger_episodes=2, danger_short_from=E - 2)
    return env, pol, bufs


def _is_short(N, visible, max_neighbors):
    return (COUNTS.index(N) + int(visible) + int(max_neighbors == 10)) % 2 == 0


GRID = [(N, vis, mn) for N in COUNTS for vis in (False, True) for mn in (3, 10)]


# ------------------------------------------------------------------------------------- device against device, every byte
@pytest.mark.parametrize("count_hh", (1, 0))
@pytest.mark.parametrize("N,visible,max_neighbors", GRID)
def test_one_launch_equals_the_per_step_sequence(N, visible, max_neighbors, count_hh):
    """One T-step launch against T x (ORCA.predict_batch -> env.step) on a twin env: every state array, the step
    records, the humans' actions, every rollout buffer and all six traces.  Half of the grid runs with a 2 s time limit
    (timeouts and pool restarts inside the launch), the other half 120 steps under the 25 s limit (robots arrive)."""
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    short = _is_short(N, visible, max_neighbors)
    time_limit, T = (2, 40) if short else (25, 120)
    env, pol, bufs = _make(N, visible, time_limit, max_neighbors, count_hh)
    twin, tpol, tbufs = _make(N, visible, time_limit, max_neighbors, count_hh)
    tr = env.rollout_orca(pol, T, trace=True)
    assert _hip.last_dispatch() == KERNEL
    ref = _per_step(twin, tpol, T)
    assert _hip.last_dispatch() == "env_step_kernel"
    torch.cuda.synchronize()
    what = "N=%d visible=%s max_neighbors=%d time_limit=%d count_hh=%d" % (N, visible, max_neighbors, time_limit, count_hh)
    _assert_equal_traces(tr, ref, what)
    _assert_equal_envs(env, twin, bufs, tbufs, what)
    infos = tr["info"].cpu().numpy()
    if short:
        assert int(bufs["fin_count"].min()) >= 1 and (infos == _hip.INFO_TIMEOUT).any(), "no env restarted"
        hr = tr["hrad"].cpu().numpy()
        assert (hr[1:] != hr[:-1]).any(), "a restart should have changed radii"
    else:
        assert (infos == _hip.INFO_REACHGOAL).any(), "no robot reached its goal"
    assert np.array_equal(tr["done"].cpu().numpy() != 0, infos >= _hip.INFO_REACHGOAL)
    assert (np.abs(tr["human_act"].cpu().numpy()).sum(-1) > 0).any()
    if not count_hh:
        assert (tr["hh_count"].cpu().numpy() == 0).all()


@pytest.mark.parametrize("generic", (0, 1))
@pytest.mark.parametrize("N", (5, 10))
def test_per_step_sequence_through_both_single_step_forms(N, generic, tuning):
    """The loop runs the run-time-N body; the per-step twin's mcn_env_step_sf takes the compile-time-N kernels at 5 and
    10 humans and, with force_generic, the run-time-N one.  Both leave the launch's bytes."""
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    tuning(force_generic=generic)
    for visible in (False, True):
        env, pol, bufs = _make(N, visible, 2, 10)
        twin, tpol, tbufs = _make(N, visible, 2, 10)
        tr = env.rollout_orca(pol, 40, trace=True)
        assert _hip.last_dispatch() == KERNEL
        ref = _per_step(twin, tpol, 40)
        assert _hip.last_dispatch() == "env_step_kernel"
        torch.cuda.synchronize()
        what = "N=%d visible=%s force_generic=%d" % (N, visible, generic)
        _assert_equal_traces(tr, ref, what)
        _assert_equal_envs(env, twin, bufs, tbufs, what)
        assert int(bufs["fin_count"].min()) >= 1


def test_split_launches_equal_one_launch():
    """7 + 13 + 20 steps leave the same bytes as one 40-step launch (restarts inside); a run without traces leaves the
    same state and returns None."""
    torch = need_gpu()
    env, pol, bufs = _make(5, True, 2, 10)
    twin, tpol, tbufs = _make(5, True, 2, 10)
    whole = env.rollout_orca(pol, 40, trace=True)
    parts = [twin.rollout_orca(tpol, n, trace=True) for n in (7, 13, 20)]
    torch.cuda.synchronize()
    _assert_equal_traces({k: torch.cat([p[k] for p in parts]) for k in TRACES}, whole, "split")
    _assert_equal_envs(twin, env, tbufs, bufs, "split")
    assert int(bufs["fin_count"].min()) >= 1
    third, hpol, hbufs = _make(5, True, 2, 10)
    assert third.rollout_orca(hpol, 40) is None
    torch.cuda.synchronize()
    _assert_equal_envs(third, env, hbufs, bufs, "no trace")


def test_get_human_times_still_raises():
    need_gpu()
    env, _, _ = _make(5, False, 25, 10)
    with pytest.raises(NotImplementedError, match="social-force"):
        env.get_human_times()


# ---------------------------------------------------------------------------------------------------------- Explorer
def _explore(kind, closed_loop, collect=False, k=20):
    torch = need_gpu()
    from modelcrowdnav_amd.rollout import VecExplorer
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    env = H.make_vec_env(8, 5, **SF_ENV)
    assert env.human_policy_name == "socialforce"
    env.track_human_times = False; env.export_human_actions = False
    pol = _robot_policy()
    env.robot.set_policy(pol)
    mem = ReplayMemory(20000, device=torch.device("cuda", 0))
    ex = VecExplorer(env, env.robot, gamma=GAMMA, policy=pol, memory=mem, target_policy=_target(kind))
    if collect:
        ex.raw_memory, ex.rawob = [], []
    out = ex.run_k_episodes(k, "train", update_memory=True, imitation_learning=True, update_raw_ob=collect,
                            closed_loop=closed_loop)
    states = torch.stack([mem[i][0] for i in range(len(mem))])
    values = torch.stack([mem[i][1] for i in range(len(mem))])
    return ex, out, states, values


def test_explorer_imitation_learning_rows_come_from_the_trace():
    """20 episodes over 8 social-force envs with a SARL target: the automatic path against closed_loop=False."""
    from modelcrowdnav_amd import _hip
    auto = _explore("sarl", None)
    assert _hip.last_dispatch() == KERNEL
    loop = _explore("sarl", False)
    assert auto[0].last_run_closed_loop and not loop[0].last_run_closed_loop
    _assert_same_run(auto, loop)


def test_explorer_collection_is_served_from_the_trace():
    auto, loop = _explore("sarl", None, collect=True), _explore("sarl", False, collect=True)
    assert auto[0].last_run_closed_loop and not loop[0].last_run_closed_loop
    _assert_same_run(auto, loop)
    for name in ("raw_memory", "rawob"):
        got, want = getattr(auto[0], name), getattr(loop[0], name)
        assert len(got) == len(want) > 0
        for g, w in zip(got, want):
            for x, y in zip(g, w):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes() and type(x) is type(y), name


@pytest.mark.parametrize("kind", ("om_sarl", "lstm_rl"))
def test_target_policies_that_need_more_than_the_trace_stay_per_step(kind):
    auto = _explore(kind, None, k=8)
    assert not auto[0].last_run_closed_loop
    with pytest.raises(ValueError, match="social-force"):
        _explore(kind, True, k=8)


# ------------------------------------------------------------------------------------- device against the host, per step
def _cmp(got, want, what):
    H.assert_bits_equal(np.asarray(got), np.asarray(want), what)


def _host_env(w):
    """The env of workload w (tests/closed_loop_sf_ref.py) with its rollout buffers, sentinel-filled."""
    env = H.make_vec_env(F.E, w.N, robot_visible=w.visible, **dict(SF_ENV, **{"env.time_limit": F.TIME_LIMIT}))
    env._sf.strength, env._sf.range, env._sf.relaxation_rate = F.SF_PARAMS
    env.count_hh = True
    pol = _robot_policy(F.ROBOT.max_neighbors, F.ROBOT.safety_space)
    assert (pol.neighbor_dist, pol.time_horizon) == (F.ROBOT.neighbor_dist, F.ROBOT.time_horizon)
    env.robot.set_policy(pol)
    H.upload(env, w.st0)
    bufs = env.attach_rollout(GAMMA, pool=w.scen, first_cases=w.first, **w.roll)
    bufs["fin_return"].fill_(float("nan")); bufs["fin_time"].fill_(float("nan")); bufs["fin_info"].fill_(R.SENTINEL_INFO)
    H.assert_state_equal(H.download(env), w.st0, fields=STATE_FIELDS, what="start")
    assert (env.rvpref.cpu().numpy() == w.rvpref).all()
    want = H.oracle_cfg_for(env, cport.HUMANS_GIVEN)
    for name, _ in want._fields_:
        if not name.startswith("orca_"):
            assert getattr(want, name) == getattr(w.cfg, name), "the host check's oracle runs with another %s" % name
    return env, pol, bufs


@pytest.mark.parametrize("visible", (False, True))
@pytest.mark.parametrize("N", F.HOST_COUNTS)
def test_each_step_against_the_host(N, visible):
    """Every (t, e) of a traced 40-step launch with restarts inside, each from its own "before" state: the robot's action
    bit for bit, the humans' velocities within 8 * 2^-52 * M, everything after the velocities bit for bit."""
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    w = F.workload(N, visible)
    env, pol, bufs = _host_env(w)
    ls = F.LockStep(w, disc=bufs["disc"].cpu().numpy())
    T = F.T_HOST
    tr = env.rollout_orca(pol, T, trace=True)
    assert _hip.last_dispatch() == KERNEL
    torch.cuda.synchronize()
    c = lambda x: np.ascontiguousarray(x.detach().cpu().numpy())
    robot, humans, hrad, action, hact = (c(tr[k]) for k in ("robot", "humans", "hrad", "action", "human_act"))
    trec = c(tr["rec"]).view(CR.STEP_DTYPE).reshape(T, F.E)
    worst, radii_changed = 0.0, False
    for t in range(T):
        what = "N=%d visible=%d step %d" % (N, visible, t)
        # the host state is the trace's "before" state (the step after t - 1, or the start)
        b = ls.before()
        _cmp(robot[t], b["robot"], what + ": trace robot"); _cmp(humans[t], b["humans"], what + ": trace humans")
        _cmp(hrad[t], b["hrad"], what + ": trace hrad")
        radii_changed = radii_changed or (t > 0 and bool((hrad[t] != hrad[t - 1]).any()))
        # 1  the robot's action
        _cmp(action[t], ls.robot_actions(), what + ": the robot's action")
        # 2  the humans' velocities
        want, mag = ls.restatement()
        err, tol = np.abs(hact[t] - want), F.TOL * mag[..., None]
        assert not np.isnan(hact[t]).any(), what
        ratio = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1), 0)))
        worst = max(worst, ratio)
        assert (err <= tol).all(), (what, ratio, np.argwhere(err > tol)[:4].tolist())
        # 3  everything after the velocities
        rec, given = ls.advance(action[t], hact[t])
        assert ls.margin > F.MARGIN, (what, ls.margin)
        for f in ("reward", "dmin", "done", "info", "hh_count"):
            _cmp(trec[f][t], rec[f], "%s: record %s" % (what, f))
        assert (trec["reserved"][t] == 0).all(), what
        _cmp(given, hact[t], what + ": the oracle took other velocities")
    print("N=%d visible=%d: largest velocity error / tolerance %.4f, smallest distance from a threshold %.3g"
          % (N, visible, worst, ls.margin))
    what = "N=%d visible=%d after %d steps" % (N, visible, T)
    H.assert_state_equal(H.download(env), ls.st, fields=STATE_FIELDS, what=what)
    last = c(env.step_rec).view(CR.STEP_DTYPE).reshape(F.E)
    for f in ("reward", "dmin", "done", "info", "hh_count"):
        _cmp(last[f], trec[f][-1], what + ": out->rec " + f)
    _cmp(c(env.human_act), hact[-1], what + ": out->human_act")
    roll = c(bufs["state"]).view(R.ROLL_DTYPE).reshape(F.E)
    for f in R.ROLL_FIELDS:
        _cmp(roll[f], ls.rep.rec[f], "%s: roll.state %s" % (what, f))
    for k in ("fin_return", "fin_time", "fin_info"):
        _cmp(c(bufs[k]), getattr(ls.rep, k), "%s: %s" % (what, k))
    assert ls.covered(), "the launch met only %s" % sorted(ls.infos)
    assert ls.robot_lp3 > 0, "no robot solve went into the 3-D LP (its projected lines live in LDS rows)"
    assert ls.rep.events["restart"] >= F.E and radii_changed, dict(ls.rep.events)


def test_lds_sizing_at_the_largest_request():
    """32 humans and a robot that takes 10 neighbours, in packed crowds with the robot among them (the line-slot scenes of
    tests/test_closed_loop_replay_gpu.py): the social-force step has no line slots, the robot's solve fills all ten rows
    of lines the launcher sized and its 3-D LP the rows behind them (tests/closed_loop_sf_ref.lds_bytes restates that
    sizing).  A row too few would put a line on the staged float32 state of the env's first human, and the launch off the
    per-step twin."""
    torch = need_gpu()
    from tests.test_closed_loop_gpu import STATE, _same
    from tests.test_closed_loop_replay_gpu import E_SLOTS, T_SLOTS, _packed, _policy
    st, vp = _packed(32, 9)
    rp = CR.RobotPolicy(0.0625, 10.0, 10, 5.0)
    cport.lp3_entries(reset=True)
    lines = [CR.robot_lines(st, e, vp, rp, F.DT) for e in range(E_SLOTS)]
    for e in range(E_SLOTS):
        CR.robot_action(st, e, vp, rp, F.DT)
    assert max(lines) == 10 == min(rp.max_neighbors, 32), lines
    assert cport.lp3_entries(reset=True) > 0, "no robot solve of the first step goes into the 3-D LP"
    need = F.lds_bytes(32, rp.max_neighbors)
    assert need == 64 * (16 * (10 + 9) + 104)
    assert need <= torch.cuda.get_device_properties(0).shared_memory_per_block, need
    envs = []
    for _ in range(2):
        env = H.make_vec_env(E_SLOTS, 32, **SF_ENV)
        H.upload(env, st)
        env.rvpref.copy_(torch.from_numpy(np.ascontiguousarray(vp, np.float64)).to(env.device))
        envs.append(env)
    env, twin = envs
    tr = env.rollout_orca(_policy(rp), T_SLOTS, trace=True)
    ref = _per_step(twin, _policy(rp), T_SLOTS)
    torch.cuda.synchronize()
    _assert_equal_traces(tr, ref, "32 humans, 10 neighbours")
    for k in STATE:
        assert _same(getattr(env, k), getattr(twin, k)), "32 humans, 10 neighbours: %s differs" % k
    # and against the oracle's solve, bit for bit (the first step: the host knows its state)
    want = np.array([CR.robot_action(st, e, vp, rp, F.DT) for e in range(E_SLOTS)])
    _cmp(tr["action"][0].cpu().numpy(), want, "32 humans, 10 neighbours: the robot's first action")
