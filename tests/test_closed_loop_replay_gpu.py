"""GPU: mcn_env_rollout_orca (env_step.hip: env_step_loop_orca_kernel) against the host replay of its contract
(tests/closed_loop_ref.py: the C oracle's ORCA solve for the robot, the oracle's env step, the mcn_rollout bookkeeping of
tests/rollout_ref.py), every byte: all state arrays, the step records, the humans' actions, the whole mcn_roll_rec, every
fin_* slot (sentinel-filled first) and all six traces.  tests/test_closed_loop_gpu.py holds the launch to a twin env on
the same GPU; here it is held to the oracle and, through tests/golden/g16_orca_robot.npz, to the reference's own run.

  test_shapes_*                11 workgroups (9 at one human), the last one partial, for every lane layout: timeouts, pool
                               restarts that change the radii, goals, fin slots that overflow, the gated danger counters
  test_edge_batches_*          tests/closed_loop_states.py: ties at the cut, a human at exactly neighbor_dist, NaN
                               half-planes, a zero preferred velocity, one on the speed disc, the 3-D LP, 2^10 and 2^20
  test_line_slots_*            a robot that needs more LDS line slots than its humans, and the reverse
  test_reference_episodes_*    the four g16 cases of a visibility as ONE launch of four envs
  test_optional_pointers_*     roll NULL, a state without a pool, each trace NULL, no human_act, no rtheta, an hcount
  test_margin_order_*          (radius + 0.01) + safety_space, in ORCA.predict, ORCA.predict_batch and the kernel

All comparisons are bitwise (tests/helpers.py bit_mismatch: -0.0 against +0.0 fails, NaN matches NaN); no tolerance
anywhere.  Each test asserts from the replay's own counters that its inputs reached what it is there for.

Which test catches which break (value-only changes of the kernel, each tried once on an MI355X; none moves a store out
of its buffer):

  break                                                          caught by
  -------------------------------------------------------------  -----------------------------------------------------
  margin added as r + (0.01 + s)                                 test_margin_order_* alone (the kernel's action)
  the robot's candidates take the humans' staged float32 radius  shapes (safety space 0.15 against 0), the edge configs
  (the humans' margin instead of the robot policy's)             with 0.0625, line slots, optional pointers, margin order
  one LDS line slot too few for the robot (its last line lands   line slots where the robot needs more (2/10/10, 0/10/5,
  on the staged float32 state of its own env's human 0)          3/10/32, the linear twin), shapes and edge batches of
                                                                 2 .. 10 humans with an invisible robot, g16 invisible
  preferred velocity float32(rgoal) - float32(rpos) instead of   every test but the margin-order one (whose scene is
  float32(rgoal - rpos)                                          dyadic in these operands)"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cport  # noqa: E402
from tests import closed_loop_ref as CR  # noqa: E402
from tests import closed_loop_states as CS  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import rollout_ref as R  # noqa: E402
from tests.rollout_harness import need_gpu  # noqa: E402
from tests.test_closed_loop_ref_cpu import G16_CASES, g16_rows, g16_start, required_events  # noqa: E402

GAMMA = 0.9
STATE_FIELDS = H.STATE_FIELDS + ("rtheta",)
REC_FIELDS = ("reward", "dmin", "done", "info", "hh_count")
PLAIN_TRACES = ("robot", "humans", "hrad", "action", "human_act")


def _policy(pol):
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    p = policy_factory["orca"]()
    p.multiagent_training = True
    p.safety_space, p.neighbor_dist, p.max_neighbors, p.time_horizon = pol
    return p


def _env(st, rvpref, visible, humans=None, **over):
    """A VecCrowdSim holding the oracle state `st` (and the robot's max speeds); humans: the humans' own ORCA parameters."""
    torch = need_gpu()
    env = H.make_vec_env(st.E, st.N, robot_visible=visible, **over)
    for k, v in (humans or {}).items():
        setattr(env._orca, k, v)
    H.upload(env, st)
    env.rvpref.copy_(torch.from_numpy(np.ascontiguousarray(rvpref, np.float64)).to(env.device))
    return env


def _same_cfg(env, cfg):
    want = H.oracle_cfg_for(env)
    for name, _ in want._fields_:
        assert getattr(want, name) == getattr(cfg, name), "the replay's oracle ran with another %s" % name


def _where(bad, names, axis):
    return sorted({names[int(i[axis])] for i in bad})[:6] if names else [tuple(int(x) for x in i) for i in bad[:4]]


def _cmp(got, want, what, names=None, axis=0):
    got, want = np.asarray(got), np.asarray(want)
    bad = H.bit_mismatch(got, want)
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError("%s differs (bitwise) at %d places, %s; first %s: %r vs %r"
                             % (what, len(bad), _where(bad, names, axis), i, got[i], want[i]))


def _rec(a, shape):
    return np.ascontiguousarray(a.detach().cpu().numpy()).view(CR.STEP_DTYPE).reshape(shape)


def _cmp_rec(got, want, what, names=None, axis=0):
    for f in REC_FIELDS:
        _cmp(got[f], want[f], "%s %s" % (what, f), names, axis)
    assert (got["reserved"] == 0).all(), what


def _check_state(env, r, what, names=None, human_act=True):
    """State arrays, the last step's record and the humans' last actions against the replay's end."""
    got = H.download(env)
    for k in STATE_FIELDS:
        _cmp(getattr(got, k), getattr(r.st, k), "%s: state %s" % (what, k), names)
    c = lambda t: t.detach().cpu().numpy()
    _cmp(c(env.rvpref), r.rvpref, what + ": rvpref", names)
    _cmp_rec(_rec(env.step_rec, env.num_envs), r.tr["rec"][-1], what + ": out->rec", names)
    if human_act:
        _cmp(c(env.human_act), r.tr["human_act"][-1], what + ": out->human_act", names)


def _check_traces(tr, r, what, names=None, skip=()):
    T, E = r.tr["action"].shape[:2]
    for k in PLAIN_TRACES:
        if k not in skip:
            _cmp(tr[k].detach().cpu().numpy(), r.tr[k], "%s: trace %s" % (what, k), names, axis=1)
    if "rec" not in skip:
        _cmp_rec(_rec(tr["rec"], (T, E)), r.tr["rec"], what + ": trace rec", names, axis=1)


def _check_roll(bufs, rep, what):
    rec = bufs["state"].cpu().numpy().view(R.ROLL_DTYPE).reshape(rep.E)
    for f in R.ROLL_FIELDS:
        _cmp(rec[f], rep.rec[f], "%s: roll.state %s" % (what, f))
    for k in ("fin_return", "fin_time", "fin_info"):
        _cmp(bufs[k].cpu().numpy(), getattr(rep, k), "%s: %s (slot, env)" % (what, k))


def _sentinels(bufs):
    bufs["fin_return"].fill_(float("nan")); bufs["fin_time"].fill_(float("nan")); bufs["fin_info"].fill_(R.SENTINEL_INFO)


# ------------------------------------------------------------------------------------------------------------ grid shapes
# 64 // N envs per workgroup: more than 8 workgroups, not a multiple of 8 (the XCD chunk mapping's remainder path), the
# last one partial; N = 7 leaves one lane of 64 idle, 13 twelve, 32 none with two envs
SHAPES = {1: 64 * 8 + 3, 2: 32 * 10 + 5, 5: 12 * 10 + 7, 7: 9 * 10 + 4, 10: 6 * 10 + 1, 13: 4 * 10 + 3, 32: 2 * 10 + 1}
T_SHAPES, POOL = 40, 32
ROBOT = CR.RobotPolicy(0.15, 10.0, 10, 5.0)          # imitation learning: a safety space for the robot, none for the humans


def _shape_workload(N, visible):
    """Env, policy, rollout buffers and the host copy of everything the replay needs.  2 s time limit: an episode times
    out on its fifth step; every fourth env starts with its robot 0.875 m from the goal and arrives first."""
    torch = need_gpu()
    from modelcrowdnav_amd.envs import scenarios as S
    E = SHAPES[N]
    over = {"env.time_limit": 2, "env.randomize_attributes": "true"}             # restarts change the radii
    if N > 10:
        over["sim.circle_radius"] = 8.0
    env = H.make_vec_env(E, N, robot_visible=visible, **over)
    env.robot.set_policy(_policy(ROBOT))
    start, first = np.arange(E) % POOL, (np.arange(E) * 5 + 7) % POOL
    if N >= 10:                          # as tests/test_closed_loop_gpu.py::_make: the device generator's loops stop
        pool = env.device_pool(seed=5, first_case=0, count=POOL, human_num=N)
        env.load_device_scenarios(pool, list(start))
        host = {k: v.cpu().numpy() for k, v in pool.items()}
        host["hvel"] = None
    else:
        pool = S.scenario_pool(env.spec(), "test", list(range(POOL)), N, "circle_crossing")
        env.load_scenarios(pool[start])
        host = R.pool_arrays(pool)
    near = torch.arange(E, device=env.device) % 4 == 1
    env.rpos[near] = env.rgoal[near] - torch.tensor([0.0, 0.875], dtype=torch.float64, device=env.device)
    bufs = env.attach_rollout(GAMMA, pool=pool, case_stride=3, first_cases=first, fin_slots=2, danger_episodes=2,
                              danger_short_from=E // 2)
    _sentinels(bufs)
    rr = env.spec().robot_row()
    con = R.Contract(bufs["disc"].cpu().numpy(), 2.0, fin_slots=2, danger_episodes=2, danger_short_from=E // 2, pool=host,
                     case_stride=3, robot_start=(rr[S.PX], rr[S.PY]), robot_goal=(rr[S.GX], rr[S.GY]),
                     robot_theta0=rr[S.TH])
    return env, bufs, R.Replay(E, con, first_cases=first)


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("N", sorted(SHAPES))
def test_shapes_equal_the_replay(N, visible):
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    env, bufs, rep = _shape_workload(N, visible)
    st0, rvpref = H.download(env), env.rvpref.cpu().numpy()
    tr = env.rollout_orca(env.robot.policy, T_SHAPES, trace=True)
    assert _hip.last_dispatch() == "env_step_loop_orca_kernel"
    torch.cuda.synchronize()
    cfg = H.oracle_cfg_for(env)
    assert cfg.orca_safety_space == 0.0 and cfg.time_limit == 2.0 and cfg.robot_visible == int(visible)
    r = CS.replay(st0, rvpref, ROBOT, cfg, T_SHAPES, roll=rep, count=False)
    what = "N=%d E=%d visible=%d" % (N, env.num_envs, visible)
    _check_traces(tr, r, what)
    _check_state(env, r, what)
    _check_roll(bufs, rep, what)
    ev = rep.events
    assert ev["timeout"] > 0 and ev["restart"] > 0 and ev["reach"] + ev["collision"] > 0, (what, dict(ev))
    assert ev["dropped"] > 0 and ev["wrap"] > 0, (what, dict(ev))             # a third episode; next_case past the pool
    hr = r.tr["hrad"]
    assert (hr[1:] != hr[:-1]).any(), "a restart should have changed radii"


# ------------------------------------------------------------------------------------------------------------ edge batches
@pytest.mark.parametrize("N", CS.HUMAN_COUNTS)
def test_edge_batches_equal_the_replay(N):
    torch = need_gpu()
    total = {}
    for c, (mn, nd, ss, visible) in enumerate(CS.CONFIGS):
        r = CS.edge_replay(N, c)
        env = _env(r.st0, r.rvpref, visible)
        _same_cfg(env, r.cfg)
        tr = env.rollout_orca(_policy(r.pol), CS.T_EDGE, trace=True)
        torch.cuda.synchronize()
        what = "N=%d max_neighbors=%d neighbor_dist=%g safety_space=%g visible=%d" % (N, mn, nd, ss, visible)
        _check_traces(tr, r, what, r.names)
        _check_state(env, r, what, r.names)
        for k, v in r.robot_events.items():
            total[k] = total.get(k, 0) + v
    missing = [k for k in required_events(N) if total.get(k, 0) == 0]
    assert not missing, "N=%d: the robot's solves never reached %s (%s)" % (N, missing, total)


# -------------------------------------------------------------------------------------------------------------- line slots
E_SLOTS, T_SLOTS = 37, 6


def _packed(N, seed):
    """E_SLOTS packed crowds (the 'packed' block's two forms) with the robot among them, dyadic."""
    rng = np.random.RandomState(100 + seed)
    st = CS._concat([CS._lattice(rng, E_SLOTS // 2, N, 0.5), CS._random(rng, E_SLOTS - E_SLOTS // 2, N, spread=0.625)])
    st.gtime[:] = 0.0
    return st, rng.choice(CS.VPREF, E_SLOTS)


def _human_lines(st, cfg):
    """The most half-planes any human's own solve fills in state st (orca.py:95-110: the other humans in index order,
    then the robot if visible; margin (r + 0.01) + safety_space)."""
    f = np.float32
    rad = lambda r: f((r + 0.01) + cfg.orca_safety_space)
    most = 0
    for e in range(st.E):
        for i in range(st.N):
            o = [j for j in range(st.N) if j != i]
            pos = [(st.hpx[e, j], st.hpy[e, j]) for j in o]; vel = [(st.hvx[e, j], st.hvy[e, j]) for j in o]
            orad = [rad(st.hr[e, j]) for j in o]
            if cfg.robot_visible:
                pos.append((st.rpx[e], st.rpy[e])); vel.append((st.rvx[e], st.rvy[e])); orad.append(rad(st.rr[e]))
            if not pos:
                continue
            n = len(cport.orca_lines((f(st.hpx[e, i]), f(st.hpy[e, i])), (f(st.hvx[e, i]), f(st.hvy[e, i])), rad(st.hr[e, i]),
                                     np.array(pos, f), np.array(vel, f), np.array(orad, f),
                                     neighbor_dist=cfg.orca_neighbor_dist, max_neighbors=cfg.orca_max_neighbors,
                                     time_horizon=cfg.orca_time_horizon, time_step=f(cfg.time_step)))
            most = max(most, n)
    return most


# (humans' max_neighbors, robot's, N, robot visible)
SLOT_ROWS = [(2, 10, 10, False), (10, 2, 10, True), (0, 10, 5, False), (10, 0, 5, True), (3, 10, 32, False),
             (10, 1, 1, False)]


@pytest.mark.parametrize("hmn,rmn,N,visible", SLOT_ROWS)
def test_line_slots_robot_and_humans_need_different_counts(hmn, rmn, N, visible):
    torch = need_gpu()
    st, vp = _packed(N, SLOT_ROWS.index((hmn, rmn, N, visible)))
    pol = CR.RobotPolicy(0.0625, 10.0, rmn, 5.0)
    env = _env(st, vp, visible, humans=dict(max_neighbors=hmn))
    cfg = H.oracle_cfg_for(env)
    assert cfg.orca_max_neighbors == hmn
    r = CS.replay(st, vp, pol, cfg, T_SLOTS)
    # what launch_env_step_loop_orca sizes from, restated: the humans' slots and the robot's
    human_cap = min(N - 1 + int(visible), hmn)
    robot_cap = min(rmn, N)
    most_h, most_r = _human_lines(st, cfg), int(r.robot_lines.max())
    assert most_h <= human_cap and most_r <= robot_cap
    if robot_cap > human_cap:
        assert most_r > human_cap, "no robot solve fills more lines (%d) than the humans' slots (%d)" % (most_r, human_cap)
    else:
        assert most_h > robot_cap, "no human solve fills more lines (%d) than the robot's slots (%d)" % (most_h, robot_cap)
    tr = env.rollout_orca(_policy(pol), T_SLOTS, trace=True)
    torch.cuda.synchronize()
    what = "humans' max_neighbors=%d robot's=%d N=%d visible=%d" % (hmn, rmn, N, visible)
    _check_traces(tr, r, what)
    _check_state(env, r, what)
    if min(rmn, N) >= 2:
        assert r.robot_events["lp3"] > 0, "the packed scenes should send the robot into the 3-D LP"


def test_line_slots_linear_humans_against_the_per_step_twin():
    """Linear humans have no line slots of their own (nl_cap 0), the robot needs 10 of them at 32 humans.  The oracle
    matches the linear humans' device trigonometry to 1e-12, not bitwise, so the yardstick is the per-step twin."""
    torch = need_gpu()
    from tests.test_closed_loop_gpu import _assert_equal_traces, _per_step, _same, STATE
    st, vp = _packed(32, 9)
    pol = CR.RobotPolicy(0.0625, 10.0, 10, 5.0)
    env, twin = _env(st, vp, False), _env(st, vp, False)
    env.human_policy_name = twin.human_policy_name = "linear"
    assert int(CS.replay(st, vp, pol, H.oracle_cfg_for(env), 1).robot_lines.max()) == 10       # (the first step's solve)
    tr = env.rollout_orca(_policy(pol), T_SLOTS, trace=True)
    ref = _per_step(twin, _policy(pol), T_SLOTS)
    torch.cuda.synchronize()
    _assert_equal_traces(tr, ref, "linear humans")
    for k in STATE:
        assert _same(getattr(env, k), getattr(twin, k)), "linear humans: %s differs" % k


# ------------------------------------------------------------------------------------------------------ reference episodes
@pytest.mark.parametrize("visible", [0, 1])
def test_reference_episodes_in_one_launch(visible, golden_dir):
    torch = need_gpu()
    g = np.load(os.path.join(golden_dir, "g16_orca_robot.npz"))
    keys = ["v%d_c%d_" % (visible, c) for c in G16_CASES]
    lengths = [g[k + "actions"].shape[0] for k in keys]
    T = max(lengths)
    st0, htheta = g16_start()
    env = _env(st0, np.ones(4), bool(visible))
    assert env._roll is None
    tr = env.rollout_orca(_policy(CR.RobotPolicy()), T, trace=True)
    torch.cuda.synchronize()
    c = lambda t: t.detach().cpu().numpy()
    rec, robot, humans, hrad, action = _rec(tr["rec"], (T, 4)), c(tr["robot"]), c(tr["humans"]), c(tr["hrad"]), c(tr["action"])
    end = H.download(env)
    for e, k in enumerate(keys):
        for t in range(lengths[e]):
            what = "%s step %d" % (k, t)
            _cmp(action[t, e], g[k + "actions"][t], what + " action")
            _cmp(rec["reward"][t, e], g[k + "rewards"][t], what + " reward")
            assert int(rec["info"][t, e]) == int(g[k + "info"][t]) and bool(rec["done"][t, e]) == (t == lengths[e] - 1), what
            # the state after step t is the "before" trace of step t + 1, or the env itself after the last step
            if t + 1 < T:
                after = st0.copy()
                after.rpx[e], after.rpy[e], after.rvx[e], after.rvy[e], after.rtheta[e] = robot[t + 1, e]
                after.hpx[e], after.hpy[e], after.hvx[e], after.hvy[e] = humans[t + 1, e].T
                after.hr[e] = hrad[t + 1, e]
            else:
                after = end
            _cmp(g16_rows(after, e, htheta), g[k + "states"][t], what + " state")
    # goals, preferred speeds and radii never change without a pool
    for f in ("hgx", "hgy", "hvpref", "hr", "rgx", "rgy", "rr"):
        _cmp(getattr(end, f), getattr(st0, f), f)


# ------------------------------------------------------------------------------------------------------ optional pointers
E_OPT, N_OPT, T_OPT = 29, 5, 12
POL_OPT = CR.RobotPolicy(0.15, 10.0, 10, 5.0)


def _opt_start():
    """29 circle crossings of 5 humans, 2 s time limit; every fourth robot 0.875 m from its goal."""
    from modelcrowdnav_amd.envs import scenarios as S
    scen = S.scenario_pool(S.ScenarioSpec(), "test", list(range(E_OPT)), N_OPT, "circle_crossing")
    st = R.initial_state(R.pool_arrays(scen), np.arange(E_OPT))
    st.rtheta[:] = 0.625
    st.rpy[np.arange(E_OPT) % 4 == 1] = 3.125
    return st


def _launch(env, pol, T, roll=None, out=None, st=None, null=()):
    """mcn_env_rollout_orca called directly; `null`: the traces passed as NULL.  Returns the trace tensors."""
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    E, N, dev = env.num_envs, env._alloc_N, env.device
    z = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    tr = dict(robot=z(T, E, 5), humans=z(T, E, N, 4), hrad=z(T, E, N), action=z(T, E, 2), rec=z(T, E, 3),
              human_act=z(T, E, N, 2))
    rc = _hip.lib.mcn_env_rollout_orca(env._cfg_struct(None), st if st is not None else env._st, float(pol.safety_space),
                                       float(pol.neighbor_dist), int(pol.max_neighbors), float(pol.time_horizon), T,
                                       out if out is not None else env._out, roll,
                                       *[None if k in null else _hip.ptr(tr[k]) for k in CR.TRACES],
                                       E, N, _hip.stream_ptr(dev))
    _hip.check(rc, "mcn_env_rollout_orca")
    torch.cuda.synchronize()
    return tr


def _opt_env():
    st0 = _opt_start()
    env = _env(st0, np.ones(E_OPT), True, **{"env.time_limit": 2})
    return env, st0, H.oracle_cfg_for(env)


def test_optional_pointers_roll_null_and_each_trace_null():
    env, st0, cfg = _opt_env()
    r = CS.replay(st0, np.ones(E_OPT), POL_OPT, cfg, T_OPT, count=False)
    done = r.tr["rec"]["done"]
    assert done.any() and done[:-1].any(0).sum() >= E_OPT // 4, "envs should go on after `done`"
    tr = _launch(env, POL_OPT, T_OPT)
    _check_traces(tr, r, "roll NULL")
    _check_state(env, r, "roll NULL")
    for k in CR.TRACES:
        env, _, _ = _opt_env()
        tr = _launch(env, POL_OPT, T_OPT, null=(k,))
        what = "tr_%s NULL" % k
        _check_traces(tr, r, what, skip=(k,))
        _check_state(env, r, what)
        assert np.isnan(tr[k].cpu().numpy()).all(), what + ": the buffer that was not passed was written"


def test_optional_pointers_state_without_a_pool():
    """mcn_rollout with `state`, the fin_* arrays and no pool: episodes are booked and the envs go on after `done`, as
    the replay with pool=None does."""
    env, st0, cfg = _opt_env()
    bufs = env.attach_rollout(GAMMA, pool=None, fin_slots=2, danger_episodes=2, danger_short_from=E_OPT // 2)
    _sentinels(bufs)
    con = R.Contract(bufs["disc"].cpu().numpy(), 2.0, fin_slots=2, danger_episodes=2, danger_short_from=E_OPT // 2)
    rep = R.Replay(E_OPT, con)
    r = CS.replay(st0, np.ones(E_OPT), POL_OPT, cfg, T_OPT, roll=rep, count=False)
    tr = _launch(env, POL_OPT, T_OPT, roll=env._roll)
    _check_traces(tr, r, "no pool")
    _check_state(env, r, "no pool")
    _check_roll(bufs, rep, "no pool")
    ev = rep.events
    assert ev["timeout"] > 0 and ev["reach"] > 0 and ev["dropped"] > 0 and ev["restart"] == 0, dict(ev)
    assert (r.st.gtime > 2.0).all(), "without a pool the clock runs on"


def test_optional_pointers_no_human_act_no_rtheta_and_an_hcount():
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    env, st0, cfg = _opt_env()
    r = CS.replay(st0, np.ones(E_OPT), POL_OPT, cfg, T_OPT, count=False)
    # out->human_act NULL: everything else as before, the env's own buffer untouched
    env.human_act.fill_(float("nan"))
    tr = _launch(env, POL_OPT, T_OPT, out=env._out_lean)
    assert not env._out_lean.human_act
    _check_traces(tr, r, "human_act NULL")
    _check_state(env, r, "human_act NULL", human_act=False)
    assert torch.isnan(env.human_act).all()
    # st->rtheta NULL: the theta column of tr_robot is +0.0 and the env's rtheta is not touched (a pool restart included)
    env, _, _ = _opt_env()
    from modelcrowdnav_amd.envs import scenarios as S
    pool = S.scenario_pool(env.spec(), "test", list(range(8)), N_OPT, "circle_crossing")
    bufs = env.attach_rollout(GAMMA, pool=pool, case_stride=3, fin_slots=2)
    _sentinels(bufs)
    rr = env.spec().robot_row()
    con = R.Contract(bufs["disc"].cpu().numpy(), 2.0, fin_slots=2, pool=R.pool_arrays(pool), case_stride=3,
                     robot_theta0=rr[S.TH])
    rep = R.Replay(E_OPT, con)
    rt = CS.replay(st0, np.ones(E_OPT), POL_OPT, cfg, T_OPT, roll=rep, has_rtheta=False, count=False)
    assert rep.events["restart"] > 0
    rt.st.rtheta[:] = st0.rtheta                       # the replay's restart sets it; a kernel without the pointer cannot
    st = _hip.EnvState.from_buffer_copy(env._st)
    st.rtheta = None
    tr = _launch(env, POL_OPT, T_OPT, roll=env._roll, st=st)
    theta = tr["robot"][..., 4].cpu().numpy()
    _cmp(theta, np.zeros_like(theta), "tr_robot theta without st->rtheta")
    _check_traces(tr, rt, "rtheta NULL")
    _check_state(env, rt, "rtheta NULL")
    _check_roll(bufs, rep, "rtheta NULL")
    # st->hcount set: not consulted, bytes identical to the run without it
    env, _, _ = _opt_env()
    ones = torch.ones(E_OPT, dtype=torch.int32, device=env.device)
    st = _hip.EnvState.from_buffer_copy(env._st)
    st.hcount = _hip.ptr(ones)
    tr = _launch(env, POL_OPT, T_OPT, st=st)
    _check_traces(tr, r, "hcount of ones")
    _check_state(env, r, "hcount of ones")


# ------------------------------------------------------------------------------------------------------------ margin order
def test_margin_order_is_the_references_in_all_three_robots():
    """One human of a radius at which (r + 0.01) + 0.1 and r + (0.01 + 0.1) round to different float32 values, straight
    ahead of the robot: ORCA.predict (E = 1), ORCA.predict_batch and mcn_env_rollout_orca all take the action of the
    reference's order."""
    torch = need_gpu()
    from modelcrowdnav_amd.envs.utils.state import FullState, JointState, ObservableState
    cases = CS.radius_order_cases()
    assert len(cases) >= 4
    pol = CR.RobotPolicy(0.1, 10.0, 10, 5.0)
    for r in cases:
        ref, other = CS.radius_order_actions(r)
        assert ref != other
        want = np.array(ref, np.float64)
        st, vp = CS.radius_order_scene(r)
        # E = 1
        p = _policy(pol)
        p.time_step = 0.25
        me = FullState(st.rpx[0], st.rpy[0], st.rvx[0], st.rvy[0], st.rr[0], st.rgx[0], st.rgy[0], vp[0], 0.0)
        hum = ObservableState(st.hpx[0, 0], st.hpy[0, 0], st.hvx[0, 0], st.hvy[0, 0], st.hr[0, 0])
        a = p.predict(JointState(me, [hum]))
        _cmp(np.array([a.vx, a.vy]), want, "ORCA.predict r=%r" % r)
        # batched
        env = _env(st, vp, False)
        a, _ = _policy(pol).predict_batch(env)
        _cmp(a.cpu().numpy()[0], want, "ORCA.predict_batch r=%r" % r)
        # the kernel
        tr = env.rollout_orca(_policy(pol), 1, trace=True)
        torch.cuda.synchronize()
        _cmp(tr["action"].cpu().numpy()[0, 0], want, "mcn_env_rollout_orca r=%r" % r)
