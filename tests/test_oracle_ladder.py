"""The oracle's ladder counters (mcn_oracle_ladder_counts, cport.ladder_counts), the boundary batches of
tests/ladder_states.py, and the oracle's float64 step half against a plain-Python restatement of the reference on them,
bit for bit.  CPU only.

The restatement below is written from the reference, not from the oracle: crowd_sim.py:345-403 (swept test with its
early break, `(dx ** 2 + dy ** 2) ** (1 / 2)` overlaps, np.linalg.norm goal test, reward ladder), utils.py:4-26
(point_to_segment_dist), agent.py:110-138 (unicycle position, `%` heading, first-arrival test) and
multi_human_rl.py:65-88 (look-ahead reward).  The humans' actions are an input (given velocities): the ladder does not
depend on them, only the integration does."""
import numpy as np
import pytest

from oracle import cport
from tests import ladder_states as LS

NAMES = cport.LADDER_NAMES


# ------------------------------------------------------------------------------ reference restatement
def _p2s(x1, y1, x2, y2, x3, y3):
    px, py = x2 - x1, y2 - y1
    if px == 0 and py == 0:
        return np.linalg.norm((x3 - x1, y3 - y1))
    u = ((x3 - x1) * px + (y3 - y1) * py) / (px * px + py * py)
    if u > 1:
        u = 1
    elif u < 0:
        u = 0
    x, y = x1 + u * px, y1 + u * py
    return np.linalg.norm((x - x3, y - y3))


def ref_step(c, st, e, ax, ay, hact):
    """One env of CrowdSim.step(update=True) with the humans' actions hact [N,2]: (reward, done, info, dmin, hh_count,
    robot (px, py, vx, vy, theta), humans' (px, py), human_times).  dmin is the reference's: up to a collision."""
    N, dt = st.N, c.time_step
    rx, ry, th = st.rpx[e], st.rpy[e], st.rtheta[e]
    dmin, collision = float("inf"), False
    for i in range(N):
        px, py = st.hpx[e, i] - rx, st.hpy[e, i] - ry
        if not c.robot_unicycle:
            vx, vy = st.hvx[e, i] - ax, st.hvy[e, i] - ay
        else:
            vx, vy = st.hvx[e, i] - ax * np.cos(ay + th), st.hvy[e, i] - ax * np.sin(ay + th)
        ex, ey = px + vx * dt, py + vy * dt
        closest = _p2s(px, py, ex, ey, 0, 0) - st.hr[e, i] - st.rr[e]
        if closest < 0:
            collision = True
            break
        elif closest < dmin:
            dmin = closest
    hh = 0
    if c.count_hh:
        for i in range(N):
            for j in range(i + 1, N):
                dx, dy = st.hpx[e, i] - st.hpx[e, j], st.hpy[e, i] - st.hpy[e, j]
                if (dx ** 2 + dy ** 2) ** (1 / 2) - st.hr[e, i] - st.hr[e, j] < 0:
                    hh += 1
    if not c.robot_unicycle:
        end = (rx + ax * dt, ry + ay * dt)
    else:
        t = th + ay
        end = (rx + np.cos(t) * ax * dt, ry + np.sin(t) * ax * dt)
    reaching = np.linalg.norm(np.array(end) - np.array((st.rgx[e], st.rgy[e]))) < st.rr[e]
    if st.gtime[e] >= c.time_limit - 1:
        reward, done, info = 0, True, cport.INFO_TIMEOUT
    elif collision:
        reward, done, info = c.collision_penalty, True, cport.INFO_COLLISION
    elif reaching:
        reward, done, info = c.success_reward, True, cport.INFO_REACHGOAL
    elif dmin < c.discomfort_dist:
        reward, done, info = (dmin - c.discomfort_dist) * c.discomfort_penalty_factor * dt, False, cport.INFO_DANGER
    else:
        reward, done, info = 0, False, cport.INFO_NOTHING
    # robot.step, humans' step, global time, first arrivals
    if not c.robot_unicycle:
        robot = (end[0], end[1], ax, ay, th)
    else:
        nth = (th + ay) % (2 * np.pi)
        robot = (end[0], end[1], ax * np.cos(nth), ax * np.sin(nth), nth)
    hpos = [(st.hpx[e, i] + hact[i, 0] * dt, st.hpy[e, i] + hact[i, 1] * dt) for i in range(N)]
    gtime = st.gtime[e] + dt
    times = list(st.human_times[e])
    for i in range(N):
        if times[i] == 0 and np.linalg.norm(np.array(hpos[i]) - np.array((st.hgx[e, i], st.hgy[e, i]))) < st.hr[e, i]:
            times[i] = gtime
    return float(reward), int(done), info, dmin, hh, collision, robot, hpos, times


def ref_lookahead(st, e, a, dt):
    """MultiHumanRL.compute_reward for the robot after action a (humans propagated at constant velocity)."""
    nx, ny = st.rpx[e] + a[0] * dt, st.rpy[e] + a[1] * dt
    dmin, collision = float("inf"), False
    for i in range(st.N):
        qx, qy = st.hpx[e, i] + st.hvx[e, i] * dt, st.hpy[e, i] + st.hvy[e, i] * dt
        dist = np.linalg.norm((nx - qx, ny - qy)) - st.rr[e] - st.hr[e, i]
        if dist < 0:
            collision = True
            break
        if dist < dmin:
            dmin = dist
    reaching = np.linalg.norm((nx - st.rgx[e], ny - st.rgy[e])) < st.rr[e]
    if collision:
        return -0.25
    if reaching:
        return 1.0
    if dmin < 0.2:
        return (dmin - 0.2) * 0.5 * dt
    return 0.0


def _bits(x):
    return np.float64(x).view(np.uint64)


def _configs(Ns):
    for N in Ns:
        for visible in (False, True):
            for dd in LS.DISCOMFORT:
                for unicycle in (False, True):
                    yield N, visible, dd, unicycle


@pytest.mark.parametrize("family", [(1, 2, 3, 4, 5), (6, 7, 8, 9, 10, 13, 32)])
def test_oracle_equals_reference_restatement_bitwise(family):
    """The oracle's reward, done, info, hh_count, robot state (heading included), human positions and first-arrival
    times against the restatement on every ladder batch, bitwise (-0.0 != +0.0); dmin where no human collides (the
    reference stops looking at the first collision, the oracle keeps the minimum)."""
    for N, visible, dd, unicycle in _configs(family):
        st, ax, ay, gv, names = LS.ladder_batch(N, visible, dd, unicycle)
        for count_hh in (True, False):
            c = LS.cfg(visible, dd, count_hh=count_hh, unicycle=unicycle, policy=cport.HUMANS_GIVEN)
            out = st.copy()
            got = cport.env_step(c, out, ax, ay, update=True, given_v=gv)
            for e in range(st.E):
                reward, done, info, dmin, hh, coll, robot, hpos, times = ref_step(c, st, e, ax[e], ay[e], gv[e])
                where = "N=%d visible=%d dd=%g unicycle=%d count_hh=%d env %d (%s)" % (
                    N, visible, dd, unicycle, count_hh, e, names[e])
                assert _bits(got["reward"][e]) == _bits(reward), (where, got["reward"][e], reward)
                assert (got["done"][e], got["info"][e], got["hh_count"][e]) == (done, info, hh), where
                if not coll:
                    assert _bits(got["dmin"][e]) == _bits(dmin), (where, got["dmin"][e], dmin)
                mine = (out.rpx[e], out.rpy[e], out.rvx[e], out.rvy[e], out.rtheta[e])
                assert [_bits(v) for v in mine] == [_bits(v) for v in robot], (where, mine, robot)
                assert [_bits(v) for p in zip(out.hpx[e], out.hpy[e]) for v in p] == \
                    [_bits(v) for p in hpos for v in p], where
                assert [_bits(v) for v in out.human_times[e]] == [_bits(v) for v in times], where


def test_lookahead_equals_reference_restatement_bitwise():
    table = LS.lookahead_table()
    for N in (1, 2, 3, 5, 8, 10, 13, 32):
        st, names = LS.lookahead_batch(N, table)
        got = cport.lookahead_reward(st, table, 0.25)
        for e in range(st.E):
            for k, a in enumerate(table):
                r = ref_lookahead(st, e, a, 0.25)
                assert _bits(got[e, k]) == _bits(r), (N, e, names[e], k, got[e, k], r)


def _reached(Ns):
    total = dict.fromkeys(NAMES, 0)
    for N, visible, dd, unicycle in _configs(Ns):
        st, ax, ay, gv, names = LS.ladder_batch(N, visible, dd, unicycle)
        assert st.E == len(names) == len(ax) and st.E % 2 == 1
        cport.ladder_counts(reset=True)
        cport.env_step(LS.cfg(visible, dd, unicycle=unicycle), st, ax, ay, update=True)
        for k, v in cport.ladder_counts(reset=True).items():
            total[k] += v
    table = LS.lookahead_table()
    for N in Ns:
        st, _ = LS.lookahead_batch(N, table)
        cport.lookahead_reward(st, table, 0.25)
        for k, v in cport.ladder_counts(reset=True).items():
            total[k] += v
    return total


@pytest.mark.parametrize("family", [(1, 2, 3, 4, 5), (6, 7, 8, 9, 10)])
def test_ladder_batches_reach_every_counter(family):
    """The generated batches (every N of the family, robot visible and not, both discomfort distances, holonomic and
    unicycle, ORCA humans) reach every counted ladder event, so the GPU tests cannot quietly cover less."""
    total = _reached(family)
    missing = [k for k, v in total.items() if v == 0]
    assert not missing, total


# ------------------------------------------------------------------------------ hand-made cases
def _env(N=1, **kw):
    """One env: robot at the origin (radius 0.25) heading for (0, -6), humans (radius 0.25) far up-left, at rest."""
    st = cport.EnvState(1, N)
    st.rr[:] = 0.25; st.rgy[:] = -6.0
    st.hpx[0] = -3.0 - np.arange(N); st.hpy[0] = 3.0
    st.hgx[0] = st.hpx[0]; st.hgy[0] = 8.0
    st.hr[:] = 0.25; st.hvpref[:] = 1.0
    st.human_times[:] = 1.0          # no first-arrival test unless a case asks for it
    for k, v in kw.items():
        getattr(st, k)[...] = v
    return st


def _h(st, i, x, y, vx=0.0, vy=0.0):
    st.hpx[0, i], st.hpy[0, i], st.hvx[0, i], st.hvy[0, i] = x, y, vx, vy
    return st


# name: (EnvState, action (ax, ay), config overrides, counters that move)
def _cases():
    nb = np.nextafter(24.0, 0.0)
    return {
        # (0, 0.5) ahead-left, robot moving (1, 0): u == 0, closest 0.5 == radii
        "swept_touch": (_h(_env(), 0, 0.0, 0.5), (1.0, 0.0), {}, {"swept_touch", "swept_u_zero"}),
        "swept_point": (_h(_env(), 0, 1.0, 0.0, 0.5, 0.0), (0.5, 0.0), {}, {"swept_point"}),
        "swept_u_zero": (_h(_env(), 0, 0.0, 2.0), (1.0, 0.0), {}, {"swept_u_zero"}),
        # from (-0.25, 2) to (0, 2): the segment ends at the foot of the origin
        "swept_u_one": (_h(_env(), 0, -0.25, 2.0, 1.0, 0.0), (0.0, 0.0), {}, {"swept_u_one"}),
        "dmin_tie": (_h(_h(_env(2), 0, 0.0, 2.0), 1, 0.0, -2.0), (1.0, 0.0), {}, {"dmin_tie", "swept_u_zero"}),
        "danger_edge": (_h(_env(), 0, 0.0, 0.75), (1.0, 0.0), {"discomfort_dist": 0.25},
                        {"danger_edge", "swept_u_zero"}),
        "reach_edge": (_env(rgx=0.5, rgy=0.0), (1.0, 0.0), {}, {"reach_edge"}),
        "reach_band": (_env(rgx=0.5 + 5e-7, rgy=0.0), (1.0, 0.0), {}, {"reach_band"}),
        "collision_and_reach": (_h(_env(rgx=0.25, rgy=0.0), 0, 0.0, 0.25), (1.0, 0.0), {},
                                {"collision_and_reach", "swept_u_zero"}),
        "timeout_and_collision": (_h(_env(gtime=24.0), 0, 0.0, 0.25), (1.0, 0.0), {},
                                  {"timeout_and_collision", "timeout_edge", "swept_u_zero"}),
        "timeout_edge": (_env(gtime=24.0), (1.0, 0.0), {}, {"timeout_edge"}),
        "timeout_below": (_env(gtime=nb), (1.0, 0.0), {}, {"timeout_below"}),
        "hh_touch": (_h(_env(2), 1, -2.5, 3.0), (1.0, 0.0), {}, {"hh_touch"}),
        "hh_band6": (_h(_env(2), 1, -2.5 - 5e-7, 3.0), (1.0, 0.0), {}, {"hh_band6"}),
        "hh_band3": (_h(_env(2), 1, -2.5 + 5e-4, 3.0), (1.0, 0.0), {}, {"hh_band3"}),
        # the human walks (0, 0.125) with its given velocity and ends 0.25 below its goal
        "human_time_edge": (_env(human_times=0.0, hgx=-3.0, hgy=3.375), (1.0, 0.0), {}, {"human_time_edge"}),
        "theta_zero_rem": (_env(rtheta=-np.pi), (1.0, -np.pi), {"robot_unicycle": 1}, {"theta_zero_rem"}),
        "theta_neg_rem": (_env(rtheta=-1.0), (1.0, 0.5), {"robot_unicycle": 1}, {"theta_neg_rem"}),
    }


def _run_case(case):
    st, (ax, ay), over, _ = case
    c = cport.default_cfg(human_policy=cport.HUMANS_GIVEN, **over)
    gv = np.zeros((1, st.N, 2)); gv[..., 1] = 0.5
    cport.ladder_counts(reset=True)
    cport.env_step(c, st.copy(), np.array([ax]), np.array([ay]), update=True, given_v=gv)
    return {k for k, v in cport.ladder_counts(reset=True).items() if v}


LA_CASES = {
    # robot (radius 0.25) at the origin, action (0.5, 0) -> next position (0.125, 0); humans at rest
    "la_touch": ([(0.625, 0.0)], (5.0, 0.0), {"la_touch"}),
    "la_danger_edge": (None, (5.0, 0.0), {"la_danger_edge"}),       # searched (below)
    "la_reach_edge": ([(3.0, 3.0)], (0.375, 0.0), {"la_reach_edge"}),
    "la_collision_after_min": ([(3.0, 3.0), (0.25, 0.0), (-3.0, 3.0)], (5.0, 0.0), {"la_collision_after_min"}),
}


def _run_la(humans, goal, hr=0.25):
    st = cport.EnvState(1, len(humans))
    st.rr[:] = 0.25; st.rgx[:], st.rgy[:] = goal
    for i, (x, y) in enumerate(humans):
        st.hpx[0, i], st.hpy[0, i] = x, y
    st.hr[:] = hr
    cport.ladder_counts(reset=True)
    cport.lookahead_reward(st, np.array([[0.5, 0.0]]), 0.25)
    return {k for k, v in cport.ladder_counts(reset=True).items() if v}


def test_every_counter_has_a_hand_made_case():
    assert set(_cases()) | set(LA_CASES) == set(NAMES)


@pytest.mark.parametrize("name", sorted(_cases()))
def test_each_step_case_moves_exactly_its_counters(name):
    case = _cases()[name]
    moved = _run_case(case)
    assert name in moved and moved == case[-1], moved
    # and a plain step moves none
    assert not _run_case((_env(), (0.5, 0.25), {}, set()))


@pytest.mark.parametrize("name", sorted(LA_CASES))
def test_each_lookahead_case_moves_exactly_its_counters(name):
    humans, goal, want = LA_CASES[name]
    if name == "la_danger_edge":
        # d = (|0.125 - x| - 0.25) - hr == 0.2: x searched near 0.125 + 0.45 + hr, for the first radius that admits it
        hr, x = next((hr, x) for hr in (0.25, 0.375, 0.3, 0.5)
                     for x in [LS.search(lambda x: abs(0.125 - x) - 0.25 - hr, 0.575 + hr, 0.2)] if x is not None)
        moved = _run_la([(x, 0.0)], goal, hr=hr)
    else:
        moved = _run_la(humans, goal)
    assert name in moved and moved == want, moved


def test_reset_flag():
    _run_case(_cases()["timeout_edge"])
    c = cport.default_cfg(human_policy=cport.HUMANS_GIVEN)
    st = _env(gtime=24.0)
    cport.ladder_counts(reset=True)
    cport.env_step(c, st, np.array([1.0]), np.array([0.0]), update=False, given_v=np.zeros((1, 1, 2)))
    assert cport.ladder_counts(reset=False)["timeout_edge"] == 1
    assert cport.ladder_counts(reset=True)["timeout_edge"] == 1
    assert cport.ladder_counts(reset=True)["timeout_edge"] == 0


def test_heading_zero_remainder_is_positive_zero():
    """Python's % gives +0.0 for a zero remainder (-0.0 % 2pi, -2pi % 2pi); so do the oracle's heading and velocity."""
    for th, r in ((-0.0, -0.0), (-2 * np.pi, 0.0), (-np.pi, -np.pi)):
        st = _env(rtheta=th)
        c = cport.default_cfg(human_policy=cport.HUMANS_GIVEN, robot_unicycle=1)
        cport.env_step(c, st, np.array([1.0]), np.array([r]), update=True, given_v=np.zeros((1, 1, 2)))
        assert _bits(st.rtheta[0]) == _bits(0.0) and _bits(st.rvy[0]) == _bits((th + r) % (2 * np.pi)), (th, r)


def test_ladder_counters_do_not_change_any_result(tmp_path):
    """The ladder batches with and without the counters (-DMCN_ORACLE_NO_EDGE_COUNTS): the same bits."""
    import ctypes as C
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(cport.__file__))
    so = str(tmp_path / "libmcn_oracle_plain.so")
    subprocess.check_call(["make", "-s", "-C", here, "-B", "OUT=" + so,
                           "CFLAGS=-O2 -fPIC -std=c11 -ffp-contract=off -fno-fast-math -DMCN_ORACLE_NO_EDGE_COUNTS"],
                          stdout=subprocess.DEVNULL)
    plain = C.CDLL(so)
    saved = cport._lib
    for N, visible, dd, unicycle in _configs((3, 8)):
        st, ax, ay, gv, _ = LS.ladder_batch(N, visible, dd, unicycle)
        c = LS.cfg(visible, dd, unicycle=unicycle)
        sa, sb = st.copy(), st.copy()
        ra = cport.env_step(c, sa, ax, ay, update=True)
        try:
            cport._lib = plain
            rb = cport.env_step(c, sb, ax, ay, update=True)
        finally:
            cport._lib = saved
        for k in ra:
            assert np.array_equal(np.asarray(ra[k]).view(np.uint8), np.asarray(rb[k]).view(np.uint8)), (N, k)
        for k in LS._fields():
            assert np.array_equal(getattr(sa, k).view(np.uint8), getattr(sb, k).view(np.uint8)), (N, k)
