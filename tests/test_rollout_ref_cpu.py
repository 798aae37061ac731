"""CPU: tests/rollout_ref.py -- the host replay of the mcn_rollout contract that tests/test_rollout_accounting_gpu.py holds
every step kernel to -- against the reference's own expressions (explorer.py:88-99,124) and, rule by rule, against
expected values written out by hand."""
import numpy as np
import pytest

from oracle import cport
from tests import rollout_ref as R

NOTHING, DANGER, REACH, COLLISION, TIMEOUT = (cport.INFO_NOTHING, cport.INFO_DANGER, cport.INFO_REACHGOAL,
                                              cport.INFO_COLLISION, cport.INFO_TIMEOUT)


def test_replay_of_whole_episodes_equals_the_reference_explorer():
    """12 test cases over 4 envs (three rounds, in-replay restarts): per episode the return is the reference's own sum
    over the logged rewards, time / info / "too close" are those of the one-case-at-a-time loop (oracle_episode)."""
    from modelcrowdnav_amd.envs import scenarios as S
    E, N, k, gamma = 4, 5, 12, 0.9
    scen = S.scenario_pool(S.ScenarioSpec(), "test", range(k), N, "circle_crossing")
    pool = R.pool_arrays(scen)
    con = R.Contract(R.disc_table(gamma, 0.25, 1.0, 102), 25.0, fin_slots=3, danger_episodes=3, pool=pool, case_stride=E,
                     robot_theta0=np.pi / 2)
    rep = R.Replay(E, con, first_cases=np.arange(E) + E)
    st = R.initial_state(pool, np.arange(E))
    cfg = cport.default_cfg()
    rewards = [[[]] for _ in range(E)]                       # per env, per episode
    dist_sum = [0.0] * E                                     # explorer.py:88-90 over the env's steps, in step order
    for _ in range(400):
        ax, ay = R.host_goal_seeking(st)
        out = rep.step(cfg, st, ax, ay)
        for e in range(E):
            rewards[e][-1].append(float(out["reward"][e]))
            if out["info"][e] == DANGER and len(rewards[e]) <= 3:
                dist_sum[e] = dist_sum[e] + float(out["dmin"][e])
            if out["done"][e]:
                rewards[e].append([])
        if rep.rec["fin_count"].min() >= 3:
            break
    assert rep.rec["fin_count"].min() >= 3
    want = [R.oracle_episode(scen[c], gamma) for c in range(k)]
    for e in range(E):
        for j in range(3):
            w = want[e + E * j]
            ret = sum([pow(gamma, t * 0.25 * 1.0) * r for t, r in enumerate(rewards[e][j])])      # explorer.py:124
            assert rep.fin_return[j, e] == ret == w[0], (e, j)
            assert rep.fin_info[j, e] == w[1] and rep.fin_time[j, e] == w[2], (e, j)
        assert rep.rec["danger_count"][e] == sum(want[e + E * j][3] for j in range(3))
        assert rep.rec["danger_dist_sum"][e] == dist_sum[e]                    # the same additions in the same order
        # oracle_episode adds each episode up from 0 and the three sums are added here: the same terms associated
        # differently, so equal only to rounding (a handful of terms below 0.2: a few ulps of 1, far inside 1e-12)
        assert abs(rep.rec["danger_dist_sum"][e] - sum(want[e + E * j][4] for j in range(3))) < 1e-12
    assert len({w[1] for w in want}) > 1 and sum(w[3] for w in want) > 0


def _replay(E=3, disc=(1.0, 0.5, 0.25, 0.125), **kw):
    kw.setdefault("time_limit", 25.0)
    return R.Replay(E, R.Contract(disc, kw.pop("time_limit"), **{k: v for k, v in kw.items() if k != "first_cases"}),
                    first_cases=kw.get("first_cases"))


def _pool(P, N=2):
    z = np.zeros((P, N, 9))
    z[:, :, R.PX] = np.arange(P)[:, None] + 0.5
    z[:, :, R.VX] = 0.25
    return R.pool_arrays(z)


def test_slots_fill_in_order_and_later_episodes_are_dropped():
    rep = _replay(fin_slots=2)
    for i, (info, clock) in enumerate([(REACH, 3.0), (COLLISION, 1.25), (REACH, 7.0)]):
        assert rep.account(1, 1.0 + i, 1, info, 0.5, clock) is None
    assert rep.fin_return[:, 1].tolist() == [1.0, 2.0] and rep.fin_time[:, 1].tolist() == [3.0, 1.25]
    assert rep.fin_info[:, 1].tolist() == [REACH, COLLISION] and rep.rec["fin_count"][1] == 3
    assert np.isnan(rep.fin_return[:, [0, 2]]).all() and (rep.fin_info[:, [0, 2]] == R.SENTINEL_INFO).all()
    assert rep.events["recorded"] == 2 and rep.events["dropped"] == 1


def test_one_slot_keeps_the_latest_episode():
    rep = _replay(fin_slots=1)
    rep.account(0, 1.0, 1, REACH, 0.5, 3.0)
    rep.account(0, -0.25, 1, COLLISION, -0.01, 0.5)
    assert (rep.fin_return[0, 0], rep.fin_time[0, 0], rep.fin_info[0, 0]) == (-0.25, 0.5, COLLISION)
    assert rep.rec["fin_count"][0] == 2 and rep.events["overwritten"] == 1 and rep.events["recorded"] == 1
    # an episode that repeats the slot's bytes proves nothing about which one is kept: counted apart
    rep.account(0, -0.25, 1, COLLISION, -0.01, 0.5)
    assert rep.events["overwritten"] == 1 and rep.events["overwritten_same"] == 1 and rep.rec["fin_count"][0] == 3
    assert rep.first[0] == (1.0, 3.0, REACH)


def test_timeout_records_the_time_limit_not_the_clock():
    rep = _replay(fin_slots=1, time_limit=31.5)
    rep.account(2, 0.0, 1, TIMEOUT, 1.0, 30.75)
    assert rep.fin_time[0, 2] == 31.5 and rep.fin_info[0, 2] == TIMEOUT and rep.fin_return[0, 2] == 0.0


def test_return_is_two_roundings_per_step_and_restarts_at_zero():
    disc = [1.0, 0.9740037464252967, 0.9486832980505138]
    rep = _replay(disc=disc, fin_slots=1)
    rep.account(0, -0.0125, 0, DANGER, 0.1, 0.25)
    rep.account(0, -0.003, 0, DANGER, 0.17, 0.5)
    assert rep.rec["ep_steps"][0] == 2 and rep.rec["ep_return"][0] == (0.0 + 1.0 * -0.0125) + 0.9740037464252967 * -0.003
    rep.account(0, 1.0, 1, REACH, 0.3, 0.75)
    assert rep.fin_return[0, 0] == ((0.0 + 1.0 * -0.0125) + 0.9740037464252967 * -0.003) + 0.9486832980505138 * 1.0
    assert rep.rec["ep_steps"][0] == 0 and rep.rec["ep_return"][0] == 0.0


def test_discount_index_clamps_to_the_last_entry():
    rep = _replay(disc=(1.0, 0.5, 0.25, 0.125), disc_len=3)          # the fourth entry is never read
    for _ in range(5):
        rep.account(0, 1.0, 0, NOTHING, 1.0, 0.0)
    assert rep.rec["ep_return"][0] == 1.0 + 0.5 + 0.25 + 0.25 + 0.25 and rep.events["clamped"] == 2
    rep.account(0, 8.0, 1, REACH, 1.0, 0.0)
    assert rep.fin_return[0, 0] == 2.25 + 0.25 * 8.0 and rep.events["clamped"] == 3


def test_danger_gate_on_both_sides_of_danger_short_from():
    """danger_episodes = 2, danger_short_from = 2: env 0 counts its first two episodes, envs 1 and 2 their first only."""
    rep = _replay(danger_episodes=2, danger_short_from=2)
    for e in range(3):
        rep.account(e, -0.01, 0, DANGER, 0.125, 0.25)                # episode 0: everybody counts
        rep.account(e, 0.0, 0, NOTHING, 0.125, 0.5)                  # not a danger step: nobody counts
        rep.account(e, 1.0, 1, REACH, 0.5, 0.75)
        rep.account(e, -0.01, 0, DANGER, 0.0625, 0.25)               # episode 1: env 0 only
        rep.account(e, 1.0, 1, REACH, 0.5, 0.5)
        rep.account(e, -0.01, 0, DANGER, 0.03125, 0.25)              # episode 2: nobody
    assert rep.rec["danger_count"].tolist() == [2, 1, 1]
    assert rep.rec["danger_dist_sum"].tolist() == [0.1875, 0.125, 0.125]
    assert rep.events["short_side_gated"] == 2 and rep.events["long_side_counted"] == 1
    assert rep.events["boundary_gated"] == 1 and rep.events["below_boundary_counted"] == 1      # envs 1 and 0
    assert rep.last_danger.tolist() == [True, True, True]
    assert rep.events["danger_counted"] == 4 and rep.events["danger_gated"] == 5


def test_danger_gate_closed_for_everyone_and_open_for_every_step():
    closed, opened = _replay(danger_episodes=1, danger_short_from=1), _replay(danger_episodes=0, danger_short_from=1)
    for rep in (closed, opened):
        for e in range(3):
            for ep in range(3):
                rep.account(e, -0.01, 0, DANGER, 0.125, 0.25)
                rep.account(e, 1.0, 1, REACH, 0.5, 0.5)
    assert closed.rec["danger_count"].tolist() == [0, 0, 0] and closed.rec["danger_dist_sum"].tolist() == [0.0] * 3
    assert opened.rec["danger_count"].tolist() == [3, 3, 3] and opened.rec["danger_dist_sum"].tolist() == [0.375] * 3


def test_danger_distances_add_in_step_order():
    rep = _replay()
    for d in (0.1, 0.2 - 2.0 ** -50, 1e-17, 0.15):
        rep.account(0, -0.01, 0, DANGER, d, 0.0)
    assert rep.rec["danger_dist_sum"][0] == ((0.1 + (0.2 - 2.0 ** -50)) + 1e-17) + 0.15


@pytest.mark.parametrize("P,stride,first,want", [(5, 0, 3, [3, 3, 3, 3]), (5, 4, 3, [3, 2, 1, 0, 4]), (1, 0, 0, [0, 0, 0]),
                                                 (5, 3, 4, [4, 2, 0, 3, 1, 4])])
def test_next_case_walks_the_pool_by_case_stride(P, stride, first, want):
    rep = _replay(E=1, fin_slots=1, pool=_pool(P), case_stride=stride, first_cases=[first])
    got = [rep.account(0, 1.0, 1, REACH, 0.5, 1.0) for _ in want]
    assert got == want and rep.rec["next_case"][0] == (want[-1] + stride) % P
    assert rep.events["wrap"] == sum(1 for c in want if c + stride >= P)
    assert rep.account(0, 0.0, 0, NOTHING, 0.5, 1.0) is None and rep.rec["next_case"][0] == (want[-1] + stride) % P


def test_without_a_pool_nothing_restarts_and_next_case_stays():
    rep = _replay(fin_slots=2)
    assert [rep.account(0, 0.0, 1, TIMEOUT, 1.0, 24.25 + 0.25 * i) for i in range(4)] == [None] * 4
    assert rep.rec["fin_count"][0] == 4 and rep.rec["next_case"][0] == 0 and rep.fin_time[:, 0].tolist() == [25.0, 25.0]


@pytest.mark.parametrize("with_velocities", [True, False])
def test_restart_rewrites_the_env_and_nothing_else(with_velocities):
    z = np.zeros((3, 2, 9))
    z[:, :, R.PX], z[:, :, R.PY], z[:, :, R.GX], z[:, :, R.GY] = 1.5, -2.5, -1.5, 2.5
    z[:, :, R.VX], z[:, :, R.VY], z[:, :, R.RAD], z[:, :, R.VPREF] = 0.25, -0.5, 0.375, 1.25
    z[2, 1, R.PX] = 7.0
    pool = R.pool_arrays(z, with_velocities)
    rep = R.Replay(2, R.Contract([1.0], 25.0, pool=pool, case_stride=1, robot_start=(0.5, -3.0), robot_goal=(-0.5, 3.0),
                                 robot_theta0=0.625))
    st = cport.EnvState(2, 2)
    for k in st.FIELDS_H + st.FIELDS_R + ("gtime", "rtheta", "human_times"):
        getattr(st, k)[...] = 9.0
    before = st.copy()
    rep.restart(st, 1, 2)
    for k in st.FIELDS_H + st.FIELDS_R + ("gtime", "rtheta", "human_times"):
        assert np.array_equal(getattr(st, k)[0], getattr(before, k)[0]), k              # env 0 untouched
    assert st.hpx[1].tolist() == [1.5, 7.0] and st.hpy[1].tolist() == [-2.5, -2.5] and st.hgx[1].tolist() == [-1.5, -1.5]
    assert st.hr[1].tolist() == [0.375] * 2 and st.hvpref[1].tolist() == [1.25] * 2 and st.human_times[1].tolist() == [0, 0]
    assert st.hvx[1].tolist() == ([0.25] * 2 if with_velocities else [0.0] * 2)
    assert st.hvy[1].tolist() == ([-0.5] * 2 if with_velocities else [0.0] * 2)
    assert not np.signbit(st.hvx[1]).any() and not np.signbit(st.rvx[1])
    assert (st.rpx[1], st.rpy[1], st.rgx[1], st.rgy[1], st.rvx[1], st.rvy[1]) == (0.5, -3.0, -0.5, 3.0, 0.0, 0.0)
    assert st.rtheta[1] == 0.625 and st.gtime[1] == 0.0 and st.rr[1] == 9.0               # the radius is not the pool's
    assert rep.events["restart_moving"] == (1 if with_velocities else 0)


@pytest.mark.parametrize("mode,N", [("orca", 5), ("orca", 7), ("orca", 10), ("given", 5), ("given", 10), ("sf", 5), ("sf", 7),
                                    ("sf", 10)])
def test_gpu_workloads_reach_what_they_claim(mode, N):
    """Every parameter set of tests/test_rollout_accounting_gpu.py at every crowd size it runs: the replay passes
    through the events the set is there for (rollout_ref.REQUIRED), none of those it excludes, and the two table sizes
    are the streaming kernel's limit and one more.  Mode "sf" (social-force humans of strength 0) runs every set but
    latest-wins: a zero-strength crowd on a pool of one case never collides, which that set requires; it is covered
    with the shipped parameters in lock step (test_lock_step_forecast_reaches_its_events)."""
    for name in R.SETS:
        if mode == "sf" and name == "latest-wins":
            continue
        w = R.workload(name, N, mode)
        R.check_events(name, w.events)
        assert set(w.snaps) == set(R.CHECKPOINTS) and w.recs["done"].shape == (R.T_ACC, R.E_ACC)
    assert R.workload("table-128", N, mode).contract.disc_len == 128
    assert R.workload("table-129", N, mode).contract.disc_len == 129
    assert R.workload("short-table", N, mode).contract.disc_len == 5
    assert R.workload("explorer-mid", N, mode).events["max_fin_count"] > 3
    for name in ("explorer-mid", "short-table", "table-128", "table-129"):      # the boundary falls inside an env group
        sf = R.workload(name, N, mode).contract.danger_short_from
        assert 2 <= sf - 1 < R.E_ACC - 1 and all((sf - 1) % g for g in R._group_sizes(N)), (name, sf)
    if mode == "sf":
        return
    # one slot: the kept record differs from the env's first episode, so "keeps the first" would show
    assert R.workload("latest-wins", N, mode).events["first_wins_differs"] >= 50


def test_zero_strength_crowd_never_collides_on_a_pool_of_one():
    """Why mode "sf" leaves latest-wins out: with strength 0 that set finishes reach and timeout episodes and not one
    collision (5 humans)."""
    ev = R._simulate("latest-wins", 5, "sf", 0).events
    assert ev.get("collision", 0) == 0 and ev["reach"] > 100 and ev["timeout"] > 50, ev


@pytest.mark.parametrize("visible", (False, True))
@pytest.mark.parametrize("N", (5, 10))
@pytest.mark.parametrize("name", R.LOCKSTEP_SETS)
def test_lock_step_forecast_reaches_its_events(name, N, visible):
    """tests/test_rollout_accounting_gpu.py::test_social_force_accounting_in_lock_step with the host's exp in place of the
    device's (the two differ by ulps of exp; the dynamics are chaotic over 130 steps, so counts are forecasts, not
    expectations): every required event of the set is reached with hundreds of occurrences to spare.  Seen here, N = 5 /
    10, robot invisible / visible -- explorer-first: collisions 431 / 177 / 653 / 392, reach 78 / 167 / 53 / 91, timeouts
    65 / 76 / 62 / 72, dropped 144 / 10 / 315 / 118, wraps 113 / 81 / 149 / 113; latest-wins: overwritten 336 / 84 / 607 /
    256, first_wins_differs 84 / 84 / 100 / 88."""
    ev = R.lockstep_forecast(name, N, visible)
    missing = [k for k in R.lockstep_required(name) if ev.get(k, 0) == 0]
    assert not missing, (name, N, visible, missing, ev)
    assert set(R.lockstep_required(name)) >= set(R.REQUIRED[name]) - set(R._MID_ONLY)
    for k in ("reach", "collision", "timeout"):
        assert ev[k] >= 25, (k, ev)
    if name == "latest-wins":
        assert ev["overwritten"] >= 50 and ev["first_wins_differs"] >= 50, ev
    else:
        assert ev["dropped"] >= 5 and ev["wrap"] >= 40 and ev["danger_gated"] >= 400 and ev["danger_counted"] >= 200, ev

